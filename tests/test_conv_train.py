"""CPU tests of the trainable convolution (celldetection_amd/nn/conv.py, csrc/conv_train.hip, csrc/wgrad_slabs.h): the fp64 statements
of tests/conv_train_oracle.py against torch's own autograd, the wrong rules the cases tell apart, the slab partition on the host
under sanitizers, the host-side entry points and the Python surface.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib, build, pack
from conv_train_oracle import (WRONG_RULES, autograd64, bgrad, dgrad, pack_dgrad, pack_forward, unpack, wgrad)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, cin, cout, h, w, k): every kernel size, non-square images, images narrower than the window, cin != cout
CASES = [(2, 32, 32, 5, 7, 1), (2, 32, 32, 5, 7, 3), (2, 32, 32, 5, 7, 5), (2, 32, 32, 5, 7, 7), (2, 64, 32, 3, 9, 3),
         (1, 32, 64, 6, 2, 7)]


def _operands(n, cin, cout, h, w, k, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * k + h)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    dy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    return x, wt, b, dy


@pytest.mark.parametrize('cin,cout,k', [(32, 32, 1), (96, 64, 3), (32, 160, 7), (64, 32, 5)])
def test_forward_pack_statement_is_the_layout_of_pack(cin, cout, k):
    w = torch.randn(cout, cin, k, k, dtype=torch.float64)
    mine = pack_forward(w)
    items = cin // 32 * k * k
    assert mine.shape == (items + items % 2, cout, 32)
    assert torch.equal(mine[:items], pack._records(w[None], 32)[0])
    assert items % 2 == 0 or bool((mine[items] == 0).all())
    assert torch.equal(unpack(mine, cin, k), w)
    blobs = pack._Blobs(pack._precision('bf16'))  # ... and the zero item is the one pack appends
    blobs.weights(pack._records(w[None], 32))
    assert torch.equal(blobs.wparts[0], mine.reshape(-1).to(torch.bfloat16))


@pytest.mark.parametrize('case', CASES, ids=str)
def test_statements_equal_torch_autograd(case):
    n, cin, cout, h, w, k = case
    x, wt, b, dy = _operands(*case)
    _, dx, dw, db = autograd64(x, wt, b, dy)
    torch.testing.assert_close(dgrad(dy, wt), dx, rtol=1e-12, atol=1e-12)
    got, S = wgrad(x, dy, k)
    torch.testing.assert_close(got, dw, rtol=1e-12, atol=1e-12)
    assert bool((S >= got.abs() - 1e-9).all())
    torch.testing.assert_close(bgrad(dy)[0], db, rtol=1e-12, atol=1e-12)
    d = pack_dgrad(wt)
    items = cout // 32 * k * k
    assert d.shape == (items + items % 2, cin, 32) and (items % 2 == 0 or bool((d[items] == 0).all()))


def test_wrong_rules_are_told_apart():
    """Each of the rules of conv_train_oracle.WRONG_RULES moves some gradient of the cases by far more than any bound the GPU tests
    accept (they accept about 1e-5 of S; the smallest difference below is of the order of the values themselves)."""
    assert len(WRONG_RULES) >= 6
    told = set()
    for case in [c for c in CASES if c[5] > 1 and c[1] == c[2]]:
        n, cin, cout, h, w, k = case
        x, wt, b, dy = _operands(*case)
        _, dx, dw, db = autograd64(x, wt, b, dy)
        scale_x, scale_w, scale_b = dx.abs().mean(), dw.abs().mean(), db.abs().mean()
        for rule in ('taps_not_flipped', 'channels_not_swapped', 'tap_shifted'):
            assert (dgrad(dy, wt, rule) - dx).abs().max() > .1 * scale_x, (rule, case)
            told.add(rule)
        for rule, kw in (('tap_shifted', {}), ('padding_ignored_at_one_border', {}), ('last_slab_dropped', dict(slab_rows=3))):
            assert (wgrad(x, dy, k, rule, **kw)[0] - dw).abs().max() > .1 * scale_w, (rule, case)
            told.add(rule)
        assert (bgrad(dy, 'bias_over_wrong_axis')[0] - db).abs().max() > .1 * scale_b, case
        told.add('bias_over_wrong_axis')
    assert told == set(WRONG_RULES)


def test_host_build_of_the_slab_partition_agrees_with_brute_force(tmp_path):
    """``csrc/wgrad_slabs.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/wgrad_slabs_host.cpp`` (a program of its own, nothing preloaded): every pixel in exactly one slab and the step counts,
    for all N * H * W <= 4096 and slab_rows in {0, 1, 2, 3, 8}, against brute force inside the program."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'wgrad_slabs_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'wgrad_slabs_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 100000


def test_wgrad_info_answers_without_a_gpu():
    info = cda.nn.weight_grad_info
    for n, h, w in ((2, 1, 1), (2, 5, 7), (2, 3, 40), (2, 17, 33), (2, 33, 70), (8, 256, 256)):
        for slab_rows in (0, 1, 3):
            for cin, cout, k in ((32, 32, 1), (96, 64, 3), (64, 160, 7), (256, 256, 7)):
                i = info(n, h, w, cin, cout, k, slab_rows)
                rows = n * h
                assert i['slabs'] == -(-rows // i['slab_rows']) and i['reduce_chain'] == i['slabs']
                assert slab_rows == 0 or i['slab_rows'] == min(slab_rows, rows)
                assert i['steps'] == -(-i['slab_rows'] * w // 16)
                assert i['steps'] + 2 + i['reduce_chain'] <= -(-n * h * w // 16) + 2 + i['slabs']
                assert i['bias_chain'] == -(-i['slab_rows'] * w // 8) + 8 + i['slabs']
                nbytes = _lib.load().cpn_conv_wgrad_workspace_bytes(n, h, w, cin, cout, k, slab_rows)
                assert nbytes == i['slabs'] * (cin * cout * k * k + cout) * 4
    assert info(2, 4, 8, 32, 32, 3, 4)['slabs'] == 2  # a slab boundary between the two images of the batch
    lib = _lib.load()
    out = (ctypes.c_int32 * 5)()
    for bad, what in (((0, 4, 4, 32, 32, 3, 0), 'N, H and W'), ((2, 4, 4, 33, 32, 3, 0), 'multiples of 32'),
                      ((2, 4, 4, 32, 0, 3, 0), 'multiples of 32'), ((2, 4, 4, 32, 32, 2, 0), 'k must be'),
                      ((2, 4, 4, 32, 32, 9, 0), 'k must be'), ((2, 4, 4, 32, 32, 3, -1), 'slab_rows'),
                      ((65536, 65536, 1, 32, 32, 3, 0), '2^31 - 1')):
        rc = lib.cpn_conv_wgrad_info(*bad, out)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and what in lib.cpn_last_error().decode(), (bad, lib.cpn_last_error())
        assert lib.cpn_conv_wgrad_workspace_bytes(*bad) == 0
        # the launch rejects the same call before it touches a buffer (the pointers are never read)
        assert lib.cpn_conv_wgrad(1, 1, *bad, 1, 0, 1, 0, 1, 1 << 40, None) == rc
    assert lib.cpn_conv_wgrad_info(2, 4, 4, 32, 32, 3, 0, None) == _lib.E_INVALID
    assert lib.cpn_conv_train_pack(1, 0, 33, 32, 3, 0, 1, None) == _lib.E_INVALID
    assert lib.cpn_conv_train_pack(1, 2, 32, 32, 3, 0, 1, None) == _lib.E_INVALID  # dtype
    assert lib.cpn_conv_train_pack(1, 0, 32, 32, 3, 2, 1, None) == _lib.E_INVALID  # mode
    assert lib.cpn_conv_wgrad(1, 1, 2, 4, 4, 32, 32, 3, 0, 1, 0, 1, 0, 1, 16, None) == _lib.E_WORKSPACE


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in ('cpn_conv_train_pack', 'cpn_conv_wgrad_workspace_bytes', 'cpn_conv_wgrad', 'cpn_conv_wgrad_info'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    modes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define\s+CPN_CONV_PACK_([A-Z]+)\s+(\d+)', hdr)}
    assert modes == _lib.CONV_PACK_MODES
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    assert 'Trainable convolution' in flat_hdr
    for phrase in ('taps flipped', 'roles swapped', 'ascending slab order', 'No floating-point atomics', '+ one add per slab',
                   'one zero item when odd'):
        assert phrase in flat_hdr, phrase
    assert 'conv_train.hip' in build.SOURCES and 'wgrad_slabs.h' in build.HEADERS
    assert 'nn' in cda.__all__ and {'conv2d', 'Conv2d', 'convert_conv2d_', 'is_supported'} <= set(cda.nn.__all__)
    # no instantiation of the inference template, no symbol under its name, in the new unit
    src = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'conv_train.hip')).read()
    assert 'conv_igemm_kernel' not in src


def test_every_unsupported_argument_raises_naming_it():
    nn = cda.nn
    x = torch.zeros(1, 32, 4, 4)
    w = torch.zeros(32, 32, 3, 3)
    for args, name in (((torch.zeros(32, 4, 4), w), 'input of 3 dimensions'),
                       ((x, torch.zeros(32, 32, 3, 5)), 'kernel_size'),
                       ((x, torch.zeros(32, 32, 2, 2)), 'kernel_size'),
                       ((x, torch.zeros(32, 32, 9, 9)), 'kernel_size'),
                       ((torch.zeros(1, 48, 4, 4), torch.zeros(32, 48, 3, 3)), 'in_channels'),
                       ((x, torch.zeros(20, 32, 3, 3)), 'out_channels'),
                       ((x, w.double()), 'weight dtype'),
                       ((x.half(), w), 'input dtype'),
                       ((x, w, torch.zeros(32).double()), 'bias'),
                       ((x, w, None, 0), 'padding'),
                       ((x, w, None, (1, 2)), 'padding')):
        with pytest.raises(NotImplementedError, match=name):
            nn.conv2d(*args)
    with pytest.raises(RuntimeError, match='MI355X'):  # supported arguments on the CPU: the usual device error, no fallback
        nn.conv2d(x, w, None, 1)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.Conv2d(32, 32, 3)(x)
    for kwargs, name in ((dict(stride=2), 'stride'), (dict(groups=2), 'groups'), (dict(dilation=2), 'dilation'),
                         (dict(padding=0), 'padding'), (dict(padding_mode='reflect'), 'padding_mode'),
                         (dict(kernel_size=(3, 5), padding=1), 'kernel_size'), (dict(kernel_size=9), 'kernel_size'),
                         (dict(in_channels=3), 'in_channels'), (dict(out_channels=2), 'out_channels')):
        kw = dict(in_channels=32, out_channels=32, kernel_size=3)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.Conv2d(**kw)
        if 'padding' not in kwargs:
            kw['padding'] = 1
        assert not nn.is_supported(torch.nn.Conv2d(**kw)), kwargs
    assert nn.is_supported(torch.nn.Conv2d(32, 64, 7, padding=3)) and nn.is_supported(torch.nn.Conv2d(64, 32, 1))
    assert nn.is_supported(torch.nn.Conv2d(32, 32, 5, padding='same'))
    assert not nn.is_supported(torch.nn.ConvTranspose2d(32, 32, 3, padding=1)) and not nn.is_supported(torch.nn.Linear(32, 32))
    m = nn.Conv2d(32, 64, 5, bias=False)
    assert m.padding == (2, 2) and m.bias is None and tuple(m.weight.shape) == (64, 32, 5, 5)
    with pytest.raises(NotImplementedError):  # the models stay inference-only
        cda.models.CpnU22(3).train()


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 32, 3, padding=1)                 # 3 input channels: left
        self.trunk = torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.ReLU(),
                                         torch.nn.Conv2d(32, 64, 7, padding=3, bias=False))
        self.down = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1)      # strided: left
        self.grouped = torch.nn.Conv2d(64, 64, 3, padding=1, groups=2)   # grouped: left
        self.heads = torch.nn.ModuleDict(dict(score=torch.nn.Conv2d(64, 2, 1), wide=torch.nn.Conv2d(64, 32, 1)))


def test_convert_conv2d_replaces_the_eligible_convs_in_place():
    net = _Net()
    params = dict(net.named_parameters())
    keys = list(net.state_dict().keys())
    replaced, left = cda.nn.convert_conv2d_(net)
    assert replaced == ['trunk.0', 'trunk.2', 'heads.wide']
    assert set(left) == {'stem', 'down', 'grouped', 'heads.score'}
    for name, word in (('stem', 'in_channels'), ('down', 'stride'), ('grouped', 'groups'), ('heads.score', 'out_channels')):
        assert word in left[name], left
    assert isinstance(net.trunk[0], cda.nn.Conv2d) and isinstance(net.trunk[2], cda.nn.Conv2d) and \
        isinstance(net.heads['wide'], cda.nn.Conv2d)
    assert type(net.stem) is torch.nn.Conv2d and type(net.heads['score']) is torch.nn.Conv2d
    after = dict(net.named_parameters())
    assert after.keys() == params.keys() and all(after[k] is params[k] for k in params)  # the same Parameter objects
    assert list(net.state_dict().keys()) == keys
    assert net.trunk[2].bias is None and net.trunk[2].padding == (3, 3)
    fresh = _Net()
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    assert cda.nn.convert_conv2d_(net) == ([], left)  # a second call finds nothing to replace
    lone = torch.nn.Conv2d(32, 32, 3, padding=1)
    assert cda.nn.convert_conv2d_(lone) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
