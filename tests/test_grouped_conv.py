"""CPU tests of the trainable grouped 3x3 convolution (celldetection_amd/nn/grouped.py, csrc/grouped_conv_train.hip,
csrc/grouped_conv.h): the fp64 statements of tests/grouped_conv_oracle.py against torch's own autograd, the stride-2 identity, the
wrong rules the cases tell apart, the index arithmetic on the host under sanitizers, the host-side entry points and the Python
surface.  Nothing here needs a GPU."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

import celldetection_amd as cda
import grouped_conv_oracle as oracle
from celldetection_amd import _lib, build, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nn = cda.nn
N = 3
# channels per group -> C: the smallest with more than one group, and with more than one bundle where that is small
CHANNELS = {4: 32, 8: 64, 16: 64, 32: 64, 64: 128}
SIZES = [(5, 8), (6, 7)]  # non-square, even and odd H and W both ways
# the shapes of tests/test_gpu_grouped_conv.py: (N, H, W, C, cig)
GPU_SHAPES = [(1, 1, 1, 32, 4), (2, 5, 7, 32, 8), (2, 5, 7, 64, 16), (2, 6, 9, 64, 32), (2, 7, 8, 64, 64), (2, 17, 33, 160, 32),
              (2, 9, 9, 192, 64), (1, 1, 40, 128, 8), (3, 33, 2, 96, 16)]


def _operands(c, cig, h, w, stride, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * cig + 10 * h + stride)
    x = torch.randn(N, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(c, cig, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(c, generator=g, dtype=torch.float64)
    dy = torch.randn(N, c, oracle.out_size(h, stride), oracle.out_size(w, stride), generator=g, dtype=torch.float64)
    return x, wt, b, dy


CASES = list(itertools.product(sorted(CHANNELS), (1, 2), SIZES))


@pytest.mark.parametrize('cig,stride,size', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_statements_equal_torch_autograd(cig, stride, size):
    c = CHANNELS[cig]
    x, wt, b, dy = _operands(c, cig, *size, stride)
    y, dx, dw, db = oracle.autograd64(x, wt, b, dy, stride, c // cig)
    close = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(oracle.forward(x, wt, b, stride), y, **close)
    torch.testing.assert_close(oracle.dgrad(dy, wt, stride, size), dx, **close)
    got, S = oracle.wgrad(x, dy, cig, stride)
    torch.testing.assert_close(got, dw, **close)
    assert bool((S >= got.abs() - 1e-9).all())
    torch.testing.assert_close(oracle.bgrad(dy)[0], db, **close)


@pytest.mark.parametrize('cig,size', [(8, (5, 8)), (32, (6, 7)), (64, (7, 7)), (4, (1, 1)), (16, (2, 9))], ids=str)
def test_stride_2_gradients_are_the_stride_1_gradients_of_the_dilation(cig, size):
    """dZ[2 i][2 j] = dY[i][j]: torch's stride-1 autograd fed with dZ returns the stride-2 dX and dW; the bias sums dY itself."""
    c = CHANNELS[cig]
    x, wt, b, dy = _operands(c, cig, *size, 2)
    _, dx2, dw2, db2 = oracle.autograd64(x, wt, b, dy, 2, c // cig)
    dz = oracle.dilate(dy, size)
    assert dz.shape == x.shape and torch.equal(dz[:, :, ::2, ::2], dy) and int((dz != 0).sum()) == int((dy != 0).sum())
    _, dx1, dw1, db1 = oracle.autograd64(x, wt, b, dz, 1, c // cig)
    close = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dx1, dx2, **close)
    torch.testing.assert_close(dw1, dw2, **close)
    torch.testing.assert_close(db1, db2, **close)
    torch.testing.assert_close(oracle.bgrad(dy)[0], db2, **close)


def test_packs_are_the_layout_of_pack():
    """The forward statement is what graph.pack writes for inference: ``_bundle_geometry``, ``_assemble``'s block diagonal,
    ``_records``, and the zero item ``_Blobs.weights`` appends per bundle."""
    for cig, c in ((4, 64), (8, 32), (16, 96), (32, 64), (64, 128)):
        wt = torch.randn(c, cig, 3, 3, dtype=torch.float64)
        bw, bundles, gpb, items, packed = oracle.geometry(c, cig)
        assert pack._bundle_geometry(c, c, c // cig) == (bundles, bw, bw, gpb) or c == cig
        mine = oracle.pack_forward(wt)
        assert mine.shape == (bundles, packed, bw, 32)
        dense = torch.zeros(bundles, bw, bw, 3, 3, dtype=torch.float64)
        wg = wt.reshape(bundles, gpb, cig, cig, 3, 3)
        for g in range(gpb):
            dense[:, g * cig:(g + 1) * cig, g * cig:(g + 1) * cig] = wg[:, g]
        assert torch.equal(mine[:, :items], pack._records(dense, 32)) and torch.equal(oracle.unpack(mine), dense)
        assert items % 2 == 0 or bool((mine[:, items] == 0).all())
        blobs = pack._Blobs(pack._precision('bf16'))
        blobs.weights(pack._records(dense, 32))
        assert torch.equal(blobs.wparts[0], mine.reshape(-1).to(torch.bfloat16))
        d = oracle.unpack(oracle.pack_dgrad(wt))  # the dgrad records: every group's block transposed, its taps flipped
        for b in range(bundles):
            for g in range(gpb):
                blk = wg[b, g]  # [co, ci, ky, kx]
                assert torch.equal(d[b, g * cig:(g + 1) * cig, g * cig:(g + 1) * cig], blk.transpose(0, 1).flip(2, 3))
        assert int((d != 0).sum()) == int((wt != 0).sum())  # ... and zeros everywhere else


def test_wrong_rules_are_told_apart():
    """Each of the rules of grouped_conv_oracle.WRONG_RULES moves a pack (compared bit for bit by the GPU tests) or some gradient of
    the cases by far more than any bound the GPU tests accept (about 1e-5 of S; the differences below are of the order of the
    values themselves)."""
    assert len(oracle.WRONG_RULES) >= 8
    told = set()
    for cig, size in ((8, (5, 7)), (16, (6, 9))):  # more than one group per bundle, more than one bundle, odd sizes
        c = 64
        x, wt, b, dy = _operands(c, cig, *size, 2)
        _, dx, dw, db = oracle.autograd64(x, wt, b, dy, 2, c // cig)
        sx, sw = dx.abs().mean(), dw.abs().mean()
        right_f, right_d = oracle.pack_forward(wt), oracle.pack_dgrad(wt)
        for rule in ('off_group_not_zeroed', 'padding_item_per_blob'):
            for right, fn in ((right_f, oracle.pack_forward), (right_d, oracle.pack_dgrad)):
                wrong = fn(wt, rule)
                assert wrong.numel() != right.numel() or not torch.equal(wrong.reshape(-1), right.reshape(-1)), rule
            told.add(rule)
        assert oracle.pack_forward(wt, 'padding_item_per_blob').numel() < right_f.numel()  # 2 bundles of 9 items: no zero item at all
        assert (oracle.bundle_conv(x, oracle.unpack(oracle.pack_forward(wt, 'off_group_not_zeroed'))) -
                oracle.forward(x, wt)).abs().max() > .1 * oracle.forward(x, wt).abs().mean()
        for rule in ('taps_not_flipped', 'roles_swapped_across_bundle', 'off_group_not_zeroed', 'dz_on_odd_grid'):
            assert not torch.equal(oracle.pack_dgrad(wt, rule), right_d) or rule == 'dz_on_odd_grid', rule
            assert (oracle.dgrad(dy, wt, 2, size, rule) - dx).abs().max() > .1 * sx, (rule, cig)
            told.add(rule)
        assert oracle.dilate(dy, size, 'dz_sized_2hout').shape != x.shape  # odd H or W: such a dZ is not even x's size ...
        for rule, kw in (('group_offset_missing', {}), ('dz_on_odd_grid', {}), ('dz_sized_2hout', {}),
                         ('last_slab_dropped', dict(slab_rows=3))):
            assert (oracle.wgrad(x, dy, cig, 2, rule, **kw)[0] - dw).abs().max() > .1 * sw, (rule, cig)
            told.add(rule)
    # ... and where H and W are even it is, and equal: the rule can only show at odd sizes, which every GPU case but one has
    x, wt, b, dy = _operands(64, 8, 6, 8, 2)
    assert torch.equal(oracle.dilate(dy, (6, 8), 'dz_sized_2hout'), oracle.dilate(dy, (6, 8)))
    assert told == set(oracle.WRONG_RULES)


def test_host_build_of_the_index_arithmetic_agrees_with_brute_force(tmp_path):
    """``csrc/grouped_conv.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/grouped_conv_host.cpp`` (a program of its own, nothing preloaded): both packs, the fragment mapping of the weight
    gradient and the dilation against brute force inside the program, for every (C, cig) of the family up to C = 512."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'grouped_conv_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'grouped_conv_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 1000000


def test_info_and_workspace_answer_without_a_gpu():
    info = nn.grouped_weight_grad_info
    lib = _lib.load()
    shapes = GPU_SHAPES + [(8, 128, 128, 256, 8), (8, 16, 16, 2048, 64)]
    for (n, h, w, c, cig), stride, slab_rows in itertools.product(shapes, (1, 2), (0, 1, 3)):
        i = info(n, h, w, c, c // cig, stride, slab_rows)
        rows = n * h
        ho, wo = oracle.out_size(h, stride), oracle.out_size(w, stride)
        assert i['slabs'] == -(-rows // i['slab_rows']) and i['reduce_chain'] == i['slabs']
        assert slab_rows == 0 or i['slab_rows'] == min(slab_rows, rows)
        assert i['steps'] == -(-i['slab_rows'] * w // 16)
        assert i['steps'] + 2 + i['reduce_chain'] <= -(-n * h * w // 16) + 2 + i['slabs']
        brows = min(slab_rows, n * ho) if slab_rows else None
        if brows is not None:
            assert i['bias_chain'] == -(-brows * wo // 8) + 8 + -(-n * ho // brows)
        assert i['bias_chain'] <= -(-n * ho * wo // 8) + 8 + n * ho
        frags = c // 16 if cig == 64 else c // 32
        nbytes = lib.cpn_grouped_conv_wgrad_workspace_bytes(n, h, w, c, cig, stride, slab_rows)
        assert nbytes >= i['slabs'] * 9 * frags * 1024 * 4 + c * 4 and nbytes % 4 == 0
    assert info(2, 4, 8, 64, 2, 1, 4)['slabs'] == 2  # a slab boundary between the two images of the batch
    out = (ctypes.c_int32 * 5)()
    for bad, what in (((0, 4, 4, 64, 32, 1, 0), 'N, H and W'), ((2, 4, 4, 48, 16, 1, 0), 'multiple of the bundle width'),
                      ((2, 4, 4, 96, 64, 1, 0), 'multiple of the bundle width'), ((2, 4, 4, 64, 2, 1, 0), 'channels per group'),
                      ((2, 4, 4, 256, 128, 1, 0), 'channels per group'), ((2, 4, 4, 64, 32, 3, 0), 'stride'),
                      ((2, 4, 4, 64, 32, 0, 0), 'stride'), ((2, 4, 4, 64, 32, 1, -1), 'slab_rows'),
                      ((65536, 65536, 1, 64, 32, 1, 0), '2^31 - 1'), ((8, 1024, 1024, 128, 32, 1, 0), '2^30')):
        rc = lib.cpn_grouped_conv_wgrad_info(*bad, out)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and what in lib.cpn_last_error().decode(), (bad, lib.cpn_last_error())
        assert lib.cpn_grouped_conv_wgrad_workspace_bytes(*bad) == 0
        # the launch rejects the same call before it touches a buffer (the pointers are never read)
        assert lib.cpn_grouped_conv_wgrad(16, 16, 16, *bad, 16, 0, 16, 0, 16, 1 << 40, None) == rc
    assert lib.cpn_grouped_conv_wgrad_info(2, 4, 4, 64, 32, 1, 0, None) == _lib.E_INVALID


def test_every_launch_refuses_bad_arguments_before_it_reads_a_pointer():
    lib = _lib.load()
    inv = _lib.E_INVALID
    # pack: channels, dtype, mode, null pointers
    assert lib.cpn_grouped_conv_pack(16, 0, 48, 16, 0, 16, None) == inv
    assert lib.cpn_grouped_conv_pack(16, 0, 64, 12, 0, 16, None) == inv
    assert lib.cpn_grouped_conv_pack(16, 2, 64, 16, 0, 16, None) == inv
    assert lib.cpn_grouped_conv_pack(16, 0, 64, 16, 2, 16, None) == inv
    assert lib.cpn_grouped_conv_pack(None, 0, 64, 16, 0, 16, None) == inv and lib.cpn_grouped_conv_pack(16, 0, 64, 16, 0, None, None) == inv
    # dilate: sizes, channels, null and misaligned pointers, too large a tensor
    assert lib.cpn_grouped_conv_dilate(16, 0, 4, 4, 64, 16, None) == inv
    assert lib.cpn_grouped_conv_dilate(16, 2, 4, 4, 40, 16, None) == inv
    assert lib.cpn_grouped_conv_dilate(None, 2, 4, 4, 64, 16, None) == inv and lib.cpn_grouped_conv_dilate(16, 2, 4, 4, 64, None, None) == inv
    assert lib.cpn_grouped_conv_dilate(8, 2, 4, 4, 64, 16, None) == inv and 'aligned' in lib.cpn_last_error().decode()
    assert lib.cpn_grouped_conv_dilate(16, 8, 1024, 1024, 128, 16, None) == _lib.E_UNSUPPORTED
    # wgrad: null pointers per gradient asked for, dtypes, alignment, workspace
    ok = (2, 4, 4, 64, 32, 1, 0)
    need = lib.cpn_grouped_conv_wgrad_workspace_bytes(*ok)
    assert need > 0
    assert lib.cpn_grouped_conv_wgrad(16, 16, 16, *ok, None, 0, None, 0, 16, need, None) == inv  # neither gradient
    assert lib.cpn_grouped_conv_wgrad(None, 16, 16, *ok, 16, 0, None, 0, 16, need, None) == inv  # dw without x
    assert lib.cpn_grouped_conv_wgrad(16, None, 16, *ok, 16, 0, None, 0, 16, need, None) == inv  # dw without dz
    assert lib.cpn_grouped_conv_wgrad(16, 16, None, *ok, None, 0, 16, 0, 16, need, None) == inv  # db without dy
    assert lib.cpn_grouped_conv_wgrad(16, 16, 16, *ok, 16, 0, 16, 0, None, need, None) == inv  # no workspace
    assert lib.cpn_grouped_conv_wgrad(16, 16, 16, *ok, 16, 2, None, 0, 16, need, None) == inv  # dw dtype
    assert lib.cpn_grouped_conv_wgrad(16, 16, 16, *ok, None, 0, 16, 3, 16, need, None) == inv  # db dtype
    assert lib.cpn_grouped_conv_wgrad(8, 16, 16, *ok, 16, 0, None, 0, 16, need, None) == inv and 'aligned' in lib.cpn_last_error().decode()
    assert lib.cpn_grouped_conv_wgrad(16, 16, 16, *ok, 16, 0, 16, 0, 16, need - 1, None) == _lib.E_WORKSPACE


def test_cpn_conv2d_accepts_every_descriptor_of_the_family():
    """The support predicate rejects exactly what a launch would: ``cpn_conv2d_kernel_info`` (no GPU) takes the forward descriptor
    at stride 1 and 2 and the dgrad descriptor of every GPU test shape and of the encoder's shapes, and names a kernel for it."""
    shapes = GPU_SHAPES + [(8, 128, 128, 256, 8), (8, 64, 64, 512, 16), (8, 32, 32, 1024, 32), (8, 16, 16, 2048, 64), (8, 128, 128, 128, 4)]
    for (n, h, w, c, cig), stride in itertools.product(shapes, (1, 2)):
        assert nn.grouped._grouped_channels(c, c, c // cig) is None
        d = nn.grouped._grouped_desc(c, cig, stride, True)
        assert (d.bundles, d.cin_b, d.cout_b) == oracle.geometry(c, cig)[1::-1] + (oracle.geometry(c, cig)[0],)
        mode = _lib.conv_kernel_info(d, _lib.PRECISION_BF16, n, h, w, c, dst_stride=c)[0]
        assert mode in (('S1', 'N', 'S1F', 'S1Q') if stride == 1 else ('S2',)), (n, h, w, c, cig, stride, mode)
        _lib.conv_kernel_info(nn.grouped._grouped_desc(c, cig, 1, False), _lib.PRECISION_BF16, n, h, w, c, dst_stride=c)
    # ... and what the predicate rejects, the host entry rejects
    out = (ctypes.c_int32 * 5)()
    for c, cig in ((48, 16), (96, 64), (64, 2), (256, 128), (16, 4), (0, 4)):
        assert nn.grouped._grouped_channels(c, c, c // cig if c else 1) is not None
        assert _lib.load().cpn_grouped_conv_wgrad_info(1, 4, 4, c, cig, 1, 0, out) == _lib.E_INVALID


def test_header_binding_and_build_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    names = ('cpn_grouped_conv_pack', 'cpn_grouped_conv_dilate', 'cpn_grouped_conv_wgrad_workspace_bytes',
             'cpn_grouped_conv_wgrad_info', 'cpn_grouped_conv_wgrad')
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r'^(?:int|int64_t)\s+%s\s*\(([^;]*)\)\s*;' % name, hdr, re.M), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    section = flat_hdr[flat_hdr.index('---- Trainable grouped convolution'):]
    for phrase in ('taps flipped', 'roles swapped inside each group', 'ascending slab order', 'No floating-point atomics',
                   '+ one add per slab', 'IN EVERY BUNDLE', 'dz[n][2 i][2 j] = dy[n][i][j]', 'the stride-1 dgrad conv of dz',
                   'the stride-1 weight gradient of (x, dz)', 'never reach dw', '4 x the minimal work'):
        assert phrase in section, phrase
    assert 'grouped_conv_train.hip' in build.SOURCES and {'grouped_conv.h', 'wgrad_bias.h', 'wgrad_slabs.h'} <= set(build.HEADERS)
    for name in build.SOURCES:
        assert os.path.isfile(os.path.join(build.CSRC, name)), name
    for name in build.HEADERS:
        assert os.path.isfile(os.path.join(build.CSRC, name)), name
    assert {'grouped_conv2d', 'GroupedConv2d', 'convert_grouped_conv2d_', 'grouped_weight_grad_info'} <= set(nn.__all__)
    src = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'grouped_conv_train.hip')).read()
    assert 'conv_igemm_kernel' not in src and 'atomicAdd' not in src and 'printf(' not in src.replace('snprintf(', '')


def test_every_unsupported_argument_raises_naming_it():
    x = torch.zeros(1, 64, 4, 4)
    w = torch.zeros(64, 2, 3, 3)  # groups 32
    for args, kw, name in (((torch.zeros(64, 4, 4), w), dict(groups=32), 'input of 3 dimensions'),
                           ((x, torch.zeros(64, 2, 1, 1)), dict(groups=32), 'kernel_size'),
                           ((x, torch.zeros(64, 2, 3, 5)), dict(groups=32), 'kernel_size'),
                           ((x, torch.zeros(64, 2, 3)), dict(groups=32), 'kernel_size'),
                           ((x, w), dict(groups=32), 'groups 32: in_channels / groups = 2'),
                           ((x, torch.zeros(64, 4, 3, 3)), dict(groups=0), 'groups'),
                           ((x, torch.zeros(64, 4, 3, 3)), dict(groups=16.), 'groups'),
                           ((x, torch.zeros(64, 4, 3, 3)), dict(groups=8), 'out_channels'),  # 32 input channels, 64 output channels
                           ((torch.zeros(1, 48, 4, 4), torch.zeros(48, 16, 3, 3)), dict(groups=3), 'in_channels 48'),
                           ((torch.zeros(1, 64, 4, 4), torch.zeros(96, 64, 3, 3)), dict(groups=1), 'out_channels'),
                           ((x, torch.zeros(64, 4, 3, 3)), dict(groups=16, stride=3), 'stride'),
                           ((x, torch.zeros(64, 4, 3, 3)), dict(groups=16, stride=(1, 2)), 'stride'),
                           ((x, torch.zeros(64, 4, 3, 3).double()), dict(groups=16), 'weight dtype'),
                           ((x.half(), torch.zeros(64, 4, 3, 3)), dict(groups=16), 'input dtype'),
                           ((x, torch.zeros(64, 4, 3, 3), torch.zeros(64).double()), dict(groups=16), 'bias'),
                           ((x, torch.zeros(64, 4, 3, 3), torch.zeros(32)), dict(groups=16), 'bias')):
        with pytest.raises(NotImplementedError, match=name):
            nn.grouped_conv2d(*args, **kw)
    with pytest.raises(ValueError, match='channels'):
        nn.grouped_conv2d(torch.zeros(1, 32, 4, 4), torch.zeros(64, 4, 3, 3), groups=16)
    with pytest.raises(RuntimeError, match='MI355X'):  # supported arguments on the CPU: the usual device error, no fallback
        nn.grouped_conv2d(x, torch.zeros(64, 4, 3, 3), groups=16, stride=2)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.GroupedConv2d(64, 64, groups=16)(x)
    base = dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, groups=16)
    for kwargs, name in ((dict(stride=3), 'stride'), (dict(stride=(2, 1)), 'stride'), (dict(groups=1), 'groups'),
                         (dict(groups=32), 'groups'), (dict(dilation=2), 'dilation'), (dict(padding=0), 'padding'),
                         (dict(padding='valid'), 'padding'), (dict(padding='same', stride=2), 'padding'),
                         (dict(padding_mode='reflect'), 'padding_mode'), (dict(kernel_size=1, padding=0), 'kernel_size'),
                         (dict(kernel_size=(3, 5)), 'kernel_size'), (dict(out_channels=128), 'out_channels'),
                         (dict(in_channels=48, out_channels=48, groups=3), 'in_channels')):
        kw = dict(base)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.GroupedConv2d(**kw)
        if not (kw['padding'] == 'same' and kw.get('stride', 1) != 1):  # (torch itself refuses that one)
            left = nn.convert_grouped_conv2d_(torch.nn.Sequential(torch.nn.Conv2d(**kw)))[1]
            assert (list(left) == ['0'] and name in left['0']) or kw['groups'] == 1, (kwargs, left)
    m = nn.GroupedConv2d(128, 128, stride=2, groups=2, bias=False)
    assert m.padding == (1, 1) and m.stride == (2, 2) and m.bias is None and tuple(m.weight.shape) == (128, 64, 3, 3)
    assert nn.GroupedConv2d(64, 64, padding='same', groups=2).padding == 'same'
    # existing behaviour does not move
    with pytest.raises(NotImplementedError, match='groups'):
        nn.Conv2d(64, 64, 3, groups=2)


class Bottleneck(torch.nn.Module):
    """torchvision's layout: conv1 / bn1 / conv2 / bn2 / conv3 / bn3 as attributes (+ the stage-entry shortcut)."""

    def __init__(self, inplanes=64, width=128, groups=32, stride=1, out=256):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(width)
        self.conv2 = torch.nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(width)
        self.conv3 = torch.nn.Conv2d(width, out, 1, bias=False)
        self.bn3 = torch.nn.BatchNorm2d(out)
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = torch.nn.Sequential(torch.nn.Conv2d(inplanes, out, 1, stride, bias=False), torch.nn.BatchNorm2d(out))

    def forward(self, x):
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        return self.relu(self.bn3(self.conv3(y)) + self.downsample(x))


_CONVERTS = dict(conv=lambda m: nn.convert_conv2d_(m), bn=lambda m: nn.convert_batchnorm2d_(m), tail=lambda m: nn.convert_readout_tail_(m),
                 grouped=lambda m: nn.convert_grouped_conv2d_(m))


@pytest.mark.parametrize('order', list(itertools.permutations(_CONVERTS)), ids='-'.join)
def test_convert_grouped_conv2d_on_a_bottleneck_in_any_order(order):
    net = torch.nn.Sequential(Bottleneck(stride=2), Bottleneck(256, 128, 32, 1))
    params = dict(net.named_parameters())
    keys = list(net.state_dict().keys())
    results = {name: _CONVERTS[name](net) for name in order}
    assert results['grouped'] == (['0.conv2', '1.conv2'], {})
    assert sorted(results['conv'][0]) == ['0.conv1', '0.conv3', '1.conv1', '1.conv3', '1.downsample.0']
    left = results['conv'][1]
    if order.index('conv') < order.index('grouped'):  # still plain grouped convs then: left, with the reason, as before
        assert set(left) == {'0.conv2', '1.conv2', '0.downsample.0'} and all('groups' in left[k] for k in ('0.conv2', '1.conv2'))
    else:  # GroupedConv2d is skipped silently
        assert set(left) == {'0.downsample.0'}
    assert 'stride' in left['0.downsample.0']
    for i, stride in ((0, (2, 2)), (1, (1, 1))):
        assert type(net[i].conv2) is nn.GroupedConv2d and net[i].conv2.stride == stride and net[i].conv2.groups == 32
        assert type(net[i].conv1) is nn.Conv2d and type(net[i].bn2) is nn.BatchNorm2d
    after = dict(net.named_parameters())
    assert after.keys() == params.keys() and all(after[k] is params[k] for k in params)  # the same Parameter objects
    assert list(net.state_dict().keys()) == keys
    fresh = torch.nn.Sequential(Bottleneck(stride=2), Bottleneck(256, 128, 32, 1))
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    # a second call of each finds nothing, and no convert names a GroupedConv2d
    assert nn.convert_grouped_conv2d_(net) == ([], {})
    replaced, left = nn.convert_conv2d_(net)
    assert replaced == [] and set(left) == {'0.downsample.0'}
    assert nn.convert_readout_tail_(net)[0] == [] and not any('conv2' in k for k in nn.convert_readout_tail_(net)[1])


def test_convert_grouped_conv2d_root_shared_and_left():
    lone = torch.nn.Conv2d(64, 64, 3, padding=1, groups=2)
    assert nn.convert_grouped_conv2d_(lone) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    assert nn.convert_grouped_conv2d_(torch.nn.Conv2d(64, 64, 3, padding=1)) == ([], {})  # dense: not its business
    assert nn.convert_grouped_conv2d_(nn.GroupedConv2d(64, 64, groups=2)) == ([], {})
    shared = torch.nn.Conv2d(64, 64, 3, padding=1, groups=16)
    net = torch.nn.ModuleDict(dict(a=torch.nn.Sequential(shared, torch.nn.ReLU()), b=torch.nn.Sequential(shared),
                                   odd=torch.nn.Conv2d(48, 48, 3, padding=1, groups=3), dw=torch.nn.Conv2d(64, 64, 3, padding=1, groups=64),
                                   wide=torch.nn.Conv2d(64, 128, 3, padding=1, groups=2), dense=torch.nn.Conv2d(64, 64, 3, padding=1),
                                   fp16=torch.nn.Conv2d(64, 64, 3, padding=1, groups=2).half(),
                                   t=torch.nn.ConvTranspose2d(64, 64, 3, padding=1, groups=2)))
    replaced, left = nn.convert_grouped_conv2d_(net)
    assert replaced == ['a.0', 'b.0'] and net['a'][0] is net['b'][0] and type(net['a'][0]) is nn.GroupedConv2d
    assert net['a'][0].weight is shared.weight and net['a'][0].bias is shared.bias
    assert set(left) == {'odd', 'dw', 'wide', 'fp16'}
    for name, word in (('odd', 'in_channels 48'), ('dw', 'groups 64'), ('wide', 'out_channels'), ('fp16', 'weight dtype')):
        assert word in left[name], left
    assert nn.convert_grouped_conv2d_(net) == ([], left)
    replaced, left2 = nn.convert_conv2d_(net)
    assert replaced == ['dense'] and not any(k in left2 for k in ('a.0', 'b.0'))
