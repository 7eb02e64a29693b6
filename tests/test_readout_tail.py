"""CPU tests of the trainable ReadOut tail (celldetection_amd/nn/readout_tail.py, csrc/readout_tail.hip, csrc/tail_slabs.h): the fp64 statements
of tests/readout_tail_oracle.py against torch's own autograd, the wrong rules the cases tell apart, the partitions on the host
under sanitizers, the host-side entry points, the Python surface and ``convert_readout_tail_``.  Nothing here needs a GPU."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib, build
import readout_tail_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('cpn_tail_info', 'cpn_tail_workspace_bytes', 'cpn_tail_forward', 'cpn_tail_backward')


def _operands(n, cin, cout, h, w, p=.5, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * cin + 3 * cout + h)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64) + .5
    dy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64) + 1.
    wt = torch.randn(cout, cin, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64) + 2.
    m = (torch.rand(n, cin, generator=g) >= p).double()
    return x, dy, wt, b, m


# (n, cin, cout, h, w): non-square images, N = 3, every Cout of the issue
SHAPES = [(3, 32, 1, 5, 7), (3, 32, 2, 3, 40), (3, 64, 20, 4, 3), (3, 32, 32, 1, 1), (1, 32, 2, 2, 5)]


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('p', [0., .1, .5, 1.], ids=str)
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
def test_statements_equal_torch_autograd(shape, p, bias):
    x, dy, wt, b, m = _operands(*shape, p=p)
    if p == 1.:
        m = torch.zeros_like(m)
    s = 0. if p == 1. else 1. / (1. - p)
    b = b if bias else None
    close = dict(rtol=1e-12, atol=1e-12)
    y, dx, dw, db = oracle.autograd64(x, dy, wt, b, m, s)
    got = oracle.statements(x, dy, wt, b, m, s)
    torch.testing.assert_close(got['y'], y, **close)
    torch.testing.assert_close(got['dx'], dx, **close)
    torch.testing.assert_close(got['dw'], dw, **close)
    if bias:
        torch.testing.assert_close(got['db'], db, **close)
    for (val, S) in (oracle.forward(x, wt, None, m, s), oracle.input_grad(dy, wt, m, s), oracle.weight_grad(x, dy, m, s),
                     oracle.bias_grad(dy)):
        assert bool((S * max(s, 1.) >= val.abs() - 1e-9).all())
    if p == 1. and bias:
        assert torch.equal(got['y'], b.reshape(1, -1, 1, 1).expand_as(got['y'])) and not bool(got['dx'].any()) and not bool(got['dw'].any())
    assert bool((got['dx'][(m == 0)[:, :, None, None].expand_as(got['dx'])] == 0).all())  # exactly 0 on dropped channels


def test_wrong_rules_are_told_apart():
    """Each rule of readout_tail_oracle.WRONG_RULES moves some result of every case by at least a tenth of that result's mean
    magnitude: far more than any bound the GPU tests accept.  (5 x 7 = 35 pixels with slabs of 16: a slab of the flat range crosses
    an image boundary, and the last slab of an image is partial.)"""
    assert len(oracle.WRONG_RULES) >= 8
    told = set()
    for shape in [(3, 32, 20, 5, 7), (3, 64, 2, 3, 11)]:
        x, dy, wt, b, m = _operands(*shape)
        m[0, :shape[2]], m[1, :shape[2]] = 0., 1.  # (what 'db_masked' looks at)
        assert 0 < float(m.mean()) < 1 and not torch.equal(m[0], m[1])
        s = 2.
        right = oracle.statements(x, dy, wt, b, m, s)
        for rule in oracle.WRONG_RULES:
            wrong = oracle.statements(x, dy, wt, b, m, s, rule, slab_pixels=16)
            moved = [k for k in right if float((wrong[k] - right[k]).abs().max()) > .1 * float(right[k].abs().mean())]
            assert moved, (rule, shape)
            told.add(rule)
        # ... and each named rule moves what its name says
        for rule, key in (('dx_without_s', 'dx'), ('dw_not_masked', 'dw'), ('db_masked', 'db'), ('last_slab_dropped', 'dw'),
                          ('slab_crossing_an_image_takes_the_first_mask', 'dw'), ('mask_per_pixel', 'y'),
                          ('mask_of_the_wrong_image', 'dx'), ('s_applied_twice', 'y'), ('dx_not_masked', 'dx'), ('bias_scaled', 'y')):
            wrong = oracle.statements(x, dy, wt, b, m, s, rule, slab_pixels=16)
            assert float((wrong[key] - right[key]).abs().max()) > .1 * float(right[key].abs().mean()), (rule, key, shape)
    assert told == set(oracle.WRONG_RULES)


# ---- the partitions on the host

def test_host_build_of_the_partitions_agrees_with_brute_force(tmp_path):
    """``csrc/tail_slabs.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/tail_slabs_host.cpp`` (a program of its own, nothing preloaded): every pixel in exactly one slab, no slab across an
    image, the step counts and the forward tiles, for all N <= 4, HW <= 2048 and slab_pixels in {0, 1, 3, 16, 130}, against brute
    force inside the program."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'tail_slabs_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'tail_slabs_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) == 4 * 2048 * 6


# ---- host-side entry points

def test_tail_info_answers_without_a_gpu():
    info = cda.nn.readout_tail_info
    lib = _lib.load()
    for (n, hw), (cin, cout) in itertools.product(((3, 1), (3, 35), (3, 120), (3, 561), (3, 2310), (8, 65536), (4, 262144), (1, (1 << 31) - 1)),
                                                  ((32, 1), (96, 2), (256, 20), (1024, 32), (64, 17))):
        for sp in (0, 1, 3, 130, hw + 5):
            if sp and n * -(-hw // min(sp, hw)) > (1 << 24) - 1:  # more slabs than one launch takes workgroups: refused
                with pytest.raises(RuntimeError, match=r'2\^24 - 1 slabs'):
                    info(n, hw, cin, cout, sp)
                assert lib.cpn_tail_workspace_bytes(n, hw, cin, cout, sp) == 0
                continue
            i = info(n, hw, cin, cout, sp)
            assert i['slabs_per_image'] == -(-hw // i['slab_pixels']) and i['slabs'] == n * i['slabs_per_image']
            assert sp == 0 or i['slab_pixels'] == min(sp, hw)
            assert sp != 0 or i['slab_pixels'] == hw or (i['slab_pixels'] % 64 == 0 and i['slabs'] <= 512 + n)
            assert i['steps'] == -(-i['slab_pixels'] // 16)
            assert i['reduce_chain'] == i['slabs'] + 1
            assert i['steps'] + 2 + i['reduce_chain'] <= -(-n * hw // 16) + 2 + i['slabs'] + 1
            assert i['bias_chain'] == -(-i['slab_pixels'] // 8) + 8 + i['slabs'] <= -(-n * hw // 8) + 8 + i['slabs']
            assert i['forward_chain'] == cin // 16 + 2 <= cin // 16 + 3
            assert i['dx_steps'] == (2 if cout > 16 else 1)
            assert lib.cpn_tail_workspace_bytes(n, hw, cin, cout, sp) == i['slabs'] * (cin * cout + cout) * 4
    assert info(8, 65536, 256, 20)['slabs'] == 512  # the auto partition: two workgroups per CU


BAD = [((0, 35, 32, 2, 0), 'N and HW', _lib.E_INVALID), ((3, 0, 32, 2, 0), 'N and HW', _lib.E_INVALID),
       ((3, 35, 48, 2, 0), 'cin must be', _lib.E_INVALID), ((3, 35, 0, 2, 0), 'cin must be', _lib.E_INVALID),
       ((3, 35, 1056, 2, 0), 'cin must be', _lib.E_INVALID), ((3, 35, 32, 0, 0), 'cout must be', _lib.E_INVALID),
       ((3, 35, 32, 33, 0), 'cout must be', _lib.E_INVALID), ((3, 35, 32, 64, 0), 'cout must be', _lib.E_INVALID),
       ((2, 1 << 30, 32, 2, 0), '2^31 - 1 pixels', _lib.E_UNSUPPORTED), ((1 << 31, 1, 32, 2, 0), '2^31 - 1 pixels', _lib.E_UNSUPPORTED),
       ((3, 35, 32, 2, -1), 'slab_pixels', _lib.E_INVALID), ((1, 1 << 24, 32, 2, 1), '2^24 - 1 slabs', _lib.E_UNSUPPORTED)]


def test_every_launch_refuses_bad_arguments_before_it_reads_a_pointer():
    """The pointers below are the address 1 (or a huge workspace size): a launch that read one would crash the test.  The forward
    has no slab_pixels argument: the two cases that are bad by it alone are judged by info, workspace and the backward."""
    lib = _lib.load()
    out = (ctypes.c_int64 * 8)()
    p = 1
    for (n, hw, cin, cout, sp), what, code in BAD:
        launches = {
            'cpn_tail_info': lambda: lib.cpn_tail_info(n, hw, cin, cout, sp, out),
            'cpn_tail_backward': lambda: lib.cpn_tail_backward(p, p, 0, p, 0, p, 1., n, hw, cin, cout, sp, p, p, 0, p, 0, p, 1 << 40, None),
        }
        if 'slab' not in what:
            launches['cpn_tail_forward'] = lambda: lib.cpn_tail_forward(p, p, 0, p, 0, p, 1., n, hw, cin, cout, p, 0, None)
        for name, call in launches.items():
            assert call() == code and what in lib.cpn_last_error().decode() and name in lib.cpn_last_error().decode(), \
                (name, (n, hw, cin, cout, sp), lib.cpn_last_error())
        assert lib.cpn_tail_workspace_bytes(n, hw, cin, cout, sp) == 0
    assert lib.cpn_tail_info(3, 35, 32, 2, 0, None) == _lib.E_INVALID
    # a tensor or workspace that does not start at a 16-byte aligned address (a = aligned, o = 8 bytes off; never read), a short
    # workspace, dtypes, null pointers, the scale
    a, o = 4096, 4096 + 8
    need = lib.cpn_tail_workspace_bytes(3, 35, 96, 20, 3)
    assert need == 3 * 12 * (96 * 20 + 20) * 4

    def backward(x=a, dy=a, dy_dtype=0, w=a, w_dtype=0, keep=a, scale=2., dx=a, dw=a, dw_dtype=0, db=a, db_dtype=1, ws=a, nbytes=need):
        return lib.cpn_tail_backward(x, dy, dy_dtype, w, w_dtype, keep, scale, 3, 35, 96, 20, 3, dx, dw, dw_dtype, db, db_dtype, ws, nbytes, None)

    def forward(x=a, w=a, w_dtype=0, b=a, b_dtype=0, keep=a, scale=2., y=a, y_dtype=0):
        return lib.cpn_tail_forward(x, w, w_dtype, b, b_dtype, keep, scale, 3, 35, 96, 20, y, y_dtype, None)

    for kw in (dict(x=o), dict(dx=o), dict(ws=o)):
        assert backward(**kw) == _lib.E_INVALID and '16-byte aligned' in lib.cpn_last_error().decode(), kw
    assert backward(dy=a + 2) == _lib.E_INVALID and 'element size' in lib.cpn_last_error().decode()
    assert backward(nbytes=need - 1) == _lib.E_WORKSPACE and 'workspace' in lib.cpn_last_error().decode()
    for kw in (dict(dy_dtype=2), dict(w_dtype=-1), dict(dw_dtype=2), dict(db_dtype=3), dict(dy=None), dict(dx=None, dw=None, db=None),
               dict(w=None), dict(x=None), dict(ws=None), dict(scale=-1.), dict(scale=float('inf')), dict(scale=float('nan'))):
        assert backward(**kw) == _lib.E_INVALID, kw
    assert forward(x=o) == _lib.E_INVALID and '16-byte aligned' in lib.cpn_last_error().decode()
    assert forward(y=a + 2) == _lib.E_INVALID and 'element size' in lib.cpn_last_error().decode()
    for kw in (dict(w_dtype=2), dict(b_dtype=2), dict(y_dtype=2), dict(x=None), dict(w=None), dict(y=None), dict(scale=-1.),
               dict(scale=float('nan'))):
        assert forward(**kw) == _lib.E_INVALID, kw


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    declared = set(re.findall(r'\b(cpn_tail_\w+)\s*\(', hdr))
    assert declared == set(NAMES) == {s for s in _lib.EXPORTED_SYMBOLS if s.startswith('cpn_tail_')}
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    section = flat_hdr[flat_hdr.index('Trainable ReadOut tail'):]
    for phrase in ('Additions to ABI 22', 'the weight operand is masked per image', 'x * s is never rounded', 'y = fmaf(acc, s, bias)',
                   'exactly 0 for a dropped channel', 'reads its bf16 rounding', 'slabs that never cross an image',
                   'ascending (n, slab) order', 'a multiplication by 0 or 1, exact', 'multiplies by s once and rounds once',
                   'No floating-point atomics', 'read zeros and are never written', 'validates before it touches a pointer',
                   '16-byte aligned address', 'CPN_E_WORKSPACE', 'N * HW <= 2^31 - 1'):
        assert phrase in section, phrase
    assert build.SOURCES['readout_tail.hip'] == [] and 'tail_slabs.h' in build.HEADERS
    assert {'dropout_conv1x1', 'DropoutConv1x1', 'convert_readout_tail_', 'readout_tail_info'} <= set(cda.nn.__all__)
    assert 'bernoulli_(1 - p)' in cda.nn.dropout_conv1x1.__doc__ and 'torch.manual_seed' in cda.nn.dropout_conv1x1.__doc__


def test_every_unsupported_argument_raises_naming_it():
    nn = cda.nn
    x = torch.zeros(3, 32, 4, 5)
    w = torch.zeros(2, 32, 1, 1)
    for args, kwargs, name in (((torch.zeros(3, 32, 4), w), {}, 'input of 3 dimensions'),
                               ((x.half(), w), {}, 'input dtype'),
                               ((x.double(), w), {}, 'input dtype'),
                               ((x, torch.zeros(2, 32, 3, 3)), {}, 'kernel_size'),
                               ((x, torch.zeros(2, 32)), {}, 'kernel_size'),
                               ((x, w.double()), {}, 'weight dtype'),
                               ((torch.zeros(3, 48, 4, 5), torch.zeros(2, 48, 1, 1)), {}, 'in_channels 48'),
                               ((torch.zeros(3, 1056, 1, 1), torch.zeros(2, 1056, 1, 1)), {}, 'in_channels 1056'),
                               ((x, torch.zeros(33, 32, 1, 1)), {}, 'out_channels 33'),
                               ((x, torch.zeros(64, 32, 1, 1)), {}, 'out_channels 64'),
                               ((x, w, torch.zeros(3)), {}, 'bias'),
                               ((x, w, torch.zeros(2).double()), {}, 'bias'),
                               ((x, w), dict(p=-.1), 'p -0.1'),
                               ((x, w), dict(p=1.5), 'p 1.5'),
                               ((x, w), dict(p=float('nan')), 'p nan'),
                               ((x, w), dict(out_dtype=torch.float16), 'out_dtype'),
                               ((x, w), dict(p=.5, training=True, keep=torch.ones(3, 32)), 'keep'),
                               ((x, w), dict(p=.5, training=True, keep=torch.ones(2, 32, dtype=torch.bool)), 'keep'),
                               ((torch.zeros(0, 32, 4, 5), w), {}, 'at least one pixel')):
        with pytest.raises(NotImplementedError, match=name):
            nn.dropout_conv1x1(*args, **kwargs)
    with pytest.raises(ValueError, match='channels'):
        nn.dropout_conv1x1(torch.zeros(3, 64, 4, 5), w)
    for kwargs in (dict(), dict(p=.5, training=True), dict(p=.5, training=True, keep=torch.ones(3, 32, dtype=torch.bool)),
                   dict(out_dtype=torch.bfloat16)):  # supported arguments on the CPU: the usual device error, no fallback
        with pytest.raises(RuntimeError, match='MI355X'):
            nn.dropout_conv1x1(x, w, torch.zeros(2), **kwargs)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.dropout_conv1x1_backward(x, torch.zeros(3, 2, 4, 5), w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.DropoutConv1x1(32, 2, p=.1)(x)
    for args, kwargs, name in (((48, 2), {}, 'in_channels 48'), ((32, 64), {}, 'out_channels 64'), ((32, 2, 3), {}, 'kernel_size'),
                               ((32, 2, 1, 2), {}, 'stride'), ((32, 2, 1, 1, 1), {}, 'padding'), ((32, 2), dict(groups=2), 'groups'),
                               ((32, 2), dict(p=2.), 'p 2.0')):
        with pytest.raises(NotImplementedError, match=name):
            nn.DropoutConv1x1(*args, **kwargs)
    m = nn.DropoutConv1x1(64, 20, p=.1, bias=False)
    assert isinstance(m, torch.nn.Conv2d) and m.p == .1 and m.bias is None and list(m.state_dict()) == ['weight'] and 'p=0.1' in repr(m)
    assert list(nn.DropoutConv1x1(32, 2).state_dict()) == list(torch.nn.Conv2d(32, 2, 1).state_dict())
    # the existing family is untouched: the trainable conv still refuses the head convs
    for cout in (2, 20):
        with pytest.raises(NotImplementedError, match='out_channels'):
            nn.Conv2d(32, cout, 1)


# ---- convert_readout_tail_

class _Sub(torch.nn.Conv2d):
    pass


class _Net(torch.nn.Module):
    """The reference model's ReadOut.block layout, and everything the convert must leave alone."""

    def __init__(self):
        super().__init__()
        t = torch.nn
        self.block = t.Sequential(t.Conv2d(32, 32, 7, padding=3), t.BatchNorm2d(32), t.ReLU(), t.Dropout2d(.1), t.Conv2d(32, 2, 1))
        self.plain = t.Sequential(t.Conv2d(32, 32, 3, padding=1), t.ReLU(), t.Conv2d(32, 20, 1, bias=False))  # no dropout: p = 0
        self.other = t.Sequential(t.Dropout(.3), t.Conv2d(64, 1, 1))           # Dropout, not Dropout2d: p = 0, the Dropout stays
        shared = t.Dropout2d(.2)
        self.drop_twice = t.Sequential(shared, t.Conv2d(32, 2, 1), shared, t.Conv2d(32, 2, 1))  # one Dropout2d in two slots: not fused
        again = t.Conv2d(32, 2, 1)
        self.conv_twice = t.Sequential(t.Dropout2d(.4), again, t.ReLU(), again)  # one conv in two slots: one replacement, not fused
        self.wide = t.Sequential(t.Dropout2d(.1), t.Conv2d(32, 64, 1))          # Cout = 64: left
        self.odd = t.Sequential(t.Dropout2d(.1), t.Conv2d(48, 2, 1))            # Cin = 48: left
        self.strided = t.Sequential(t.Dropout2d(.1), t.Conv2d(32, 2, 1, stride=2))
        self.sub = t.Sequential(t.Dropout2d(.1), _Sub(32, 2, 1))
        self.lone = t.Conv2d(32, 2, 1)                                          # no Sequential parent: left
        self.f64 = t.Sequential(t.Dropout2d(.1), t.Conv2d(32, 2, 1).double())


def _check_converted(net, params, keys):
    nn = cda.nn
    assert type(net.block[4]) is nn.DropoutConv1x1 and net.block[4].p == .1 and type(net.block[3]) is torch.nn.Identity
    assert type(net.plain[2]) is nn.DropoutConv1x1 and net.plain[2].p == 0. and net.plain[2].bias is None
    assert type(net.other[1]) is nn.DropoutConv1x1 and net.other[1].p == 0. and type(net.other[0]) is torch.nn.Dropout
    assert net.drop_twice[0] is net.drop_twice[2] and type(net.drop_twice[0]) is torch.nn.Dropout2d
    assert type(net.drop_twice[1]) is type(net.drop_twice[3]) is nn.DropoutConv1x1 and net.drop_twice[1].p == net.drop_twice[3].p == 0.
    assert net.conv_twice[1] is net.conv_twice[3] and type(net.conv_twice[1]) is nn.DropoutConv1x1 and net.conv_twice[1].p == 0. and \
        type(net.conv_twice[0]) is torch.nn.Dropout2d
    for seq in (net.odd, net.strided, net.f64):
        assert type(seq[0]) is torch.nn.Dropout2d and type(seq[1]) is torch.nn.Conv2d
    assert type(net.wide[0]) is torch.nn.Dropout2d and type(net.wide[1]) is nn.Conv2d  # (the trainable conv's business)
    assert type(net.sub[1]) is _Sub and type(net.lone) is torch.nn.Conv2d
    after = dict(net.named_parameters())
    assert after.keys() == params.keys() and all(after[k] is params[k] for k in params)  # the same Parameter objects
    assert list(net.state_dict().keys()) == keys


@pytest.mark.parametrize('order', ['tail first', 'tail last'])
def test_convert_readout_tail_replaces_and_fuses_in_place(order):
    nn = cda.nn
    net = _Net()
    net.plain.eval()
    hook = net.block[4].register_forward_hook(lambda *a: None)
    params = dict(net.named_parameters())
    keys = list(net.state_dict().keys())
    if order == 'tail last':  # (the 1x1 conv to 64 channels is the trainable conv's: it is then no longer reported here)
        assert nn.convert_conv2d_(net)[0] == ['block.0', 'plain.0', 'wide.1'] and \
            nn.convert_batchnorm2d_(net)[:2] == (['block.1'], ['block.1'])
    replaced, left = nn.convert_readout_tail_(net)
    assert replaced == ['block.4', 'plain.2', 'other.1', 'drop_twice.1', 'drop_twice.3', 'conv_twice.1', 'conv_twice.3']
    assert set(left) == {'lone', 'odd.1', 'strided.1', 'sub.1', 'f64.1'} | ({'wide.1'} if order == 'tail first' else set())
    assert 'in_channels 48' in left['odd.1'] and 'stride' in left['strided.1'] and '_Sub' in left['sub.1'] and \
        'Sequential' in left['lone'] and 'dtype' in left['f64.1']
    if order == 'tail first':
        assert 'out_channels 64' in left['wide.1']
        conv_replaced, conv_left = nn.convert_conv2d_(net)
        assert conv_replaced == ['block.0', 'plain.0', 'wide.1']  # the trainable conv neither takes nor reports the replaced tails
        assert 'out_channels' in conv_left['lone'] and 'block.4' not in conv_left and 'plain.2' not in conv_left
        assert nn.convert_batchnorm2d_(net)[:2] == (['block.1'], ['block.1'])
        left.pop('wide.1')
    _check_converted(net, params, keys)
    assert type(net.block[0]) is nn.Conv2d and type(net.block[1]) is nn.BatchNorm2d and type(net.block[2]) is torch.nn.Identity
    # hooks, the training flag and the constructor attributes are kept
    assert net.block[4]._forward_hooks and net.block[4].training and not net.plain[2].training
    assert net.block[4].kernel_size == (1, 1) and net.block[4].out_channels == 2
    hook.remove()
    fresh = _Net()
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    assert nn.convert_readout_tail_(net) == ([], left)  # a second call finds nothing to replace
    lone = torch.nn.Conv2d(32, 2, 1)
    assert nn.convert_readout_tail_(lone) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    root = torch.nn.Sequential(torch.nn.Dropout2d(.25), torch.nn.Conv2d(64, 20, 1))  # the root itself may be the Sequential
    assert nn.convert_readout_tail_(root) == (['1'], {}) and root[1].p == .25 and type(root[0]) is torch.nn.Identity
