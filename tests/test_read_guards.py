"""The read-guard judge (tests/read_guards.py) is not vacuous: numpy emulations of each kind of stray read, all inside allocated
memory, are flagged under the pattern that is there to catch them, and a correct "kernel" passes under all three."""
import numpy as np
import pytest
import torch

import read_guards as rg


def test_patterns_decode_as_documented():
    def decode(pattern, dtype):
        return torch.full((8,), pattern, dtype=torch.uint8).view(dtype)
    for dtype in (torch.bfloat16, torch.float32, torch.float8_e4m3fn):
        assert bool(decode(rg.NAN, dtype).float().isnan().all()), dtype
        assert bool((decode(rg.ZERO, dtype).float() == 0).all()), dtype
    assert decode(rg.NAN, torch.int32).tolist() == [-1, -1] and decode(rg.ZERO, torch.int32).tolist() == [0, 0]
    assert decode(rg.PLAUSIBLE, torch.bfloat16).float().tolist() == [0.01147460937500] * 4   # 0x3C3C
    assert decode(rg.PLAUSIBLE, torch.float32).tolist() == [np.frombuffer(b'\x3c' * 4, np.float32)[0]] * 2
    assert abs(decode(rg.PLAUSIBLE, torch.float32)[0].item() - 0.0115) < 5e-5
    assert decode(rg.PLAUSIBLE, torch.float8_e4m3fn).float().tolist() == [1.5] * 8
    assert decode(rg.PLAUSIBLE, torch.int32).tolist() == [0x3C3C3C3C] * 2 and 0x3C3C3C3C > 2 ** 29


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.uint8, torch.int32])
@pytest.mark.parametrize('shape,channels_last', [((2, 3, 5, 7), False), ((2, 40, 5, 7), True), ((1, 64, 33, 47), True), ((5,), False),
                                                 ((3, 1100), False)])
def test_embedded_keeps_layout_and_bands(dtype, shape, channels_last):
    t = (torch.rand(shape, generator=torch.Generator().manual_seed(1)) * 100).to(dtype)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    for pattern in rg.PATTERNS:
        view, buf = rg.embedded(t, pattern)
        assert view.shape == t.shape and view.dtype == t.dtype and view.is_contiguous(memory_format=torch.channels_last) == channels_last
        assert view.data_ptr() % 256 == 0
        assert torch.equal(rg.view_bytes(view), rg.view_bytes(t))
        front = view.data_ptr() - buf.data_ptr()
        back = buf.numel() - front - t.numel() * t.element_size()
        row = (shape[-1] * (shape[1] if channels_last else shape[-2]) if len(shape) > 1 else 1) * t.element_size()
        assert min(front, back) >= max(row, 4096)
        rg.assert_unwritten(buf, view, pattern, rg.view_bytes(view))


# ---- the emulated kernels: each reduces a float32 operand of n elements that starts at element ``at`` of ``mem`` ---------------------
def correct(mem, at, n):
    return mem[at:at + n].sum(keepdims=True)


def one_before(mem, at, n):
    return mem[at - 1:at + n].sum(keepdims=True)


def one_after(mem, at, n):
    return mem[at:at + n + 1].sum(keepdims=True)


def times_zero(mem, at, n):
    """A masked lane that multiplies what it loaded by zero instead of not loading it."""
    return mem[at:at + n].sum(keepdims=True) + mem[at + n:at + n + 1] * np.float32(0)


def clamped(mem, at, n):
    """A max-pool window one element too wide over non-negative data, then a ReLU: fmax drops a NaN, 0 changes nothing."""
    return np.fmax(np.fmax.reduce(mem[at:at + n + 1], keepdims=True), np.float32(0))


def writes_operand(mem, at, n):
    out = mem[at:at + n].sum(keepdims=True)
    mem[at + n // 2] = 0
    return out


def run(kernel, pattern):
    """-> the result; asserts the operand and its bands unwritten."""
    # every value below the plausible 0.0115, as a ReLU output next to a larger neighbour: the clamped stray read then shows
    x = (torch.rand(1000, generator=torch.Generator().manual_seed(3)) + .5) * 2.0 ** -9
    view, buf = rg.embedded(x, pattern)
    before = rg.view_bytes(view)
    off = view.data_ptr() - buf.data_ptr()
    assert off % 4 == 0
    mem = buf.numpy()[:buf.numel() // 4 * 4].view(np.float32)
    with np.errstate(invalid='ignore'):
        out = kernel(mem, off // 4, x.numel())
    rg.assert_unwritten(buf, view, pattern, before, kernel.__name__)
    return out


def flagged_by(kernel):
    """The patterns whose run differs from the 0x00 run or is not finite, judged by same_bits_across in pairs with 0x00."""
    base = {'out': run(kernel, rg.ZERO)}
    hits = []
    for pattern in (rg.NAN, rg.PLAUSIBLE):
        try:
            rg.same_bits_across({rg.ZERO: base, pattern: {'out': run(kernel, pattern)}})
        except AssertionError as e:
            assert 'out' in str(e)
            hits.append(pattern)
    return hits


def test_a_correct_kernel_passes():
    assert flagged_by(correct) == []
    rg.same_bits_across({p: {'out': run(correct, p)} for p in rg.PATTERNS})


@pytest.mark.parametrize('kernel,expected', [(one_before, [rg.NAN, rg.PLAUSIBLE]), (one_after, [rg.NAN, rg.PLAUSIBLE]),
                                             (times_zero, [rg.NAN]), (clamped, [rg.PLAUSIBLE])],
                         ids=['one_before', 'one_after', 'times_zero:0xFF-only', 'clamped:0x3C-only'])
def test_a_stray_read_is_flagged(kernel, expected):
    got = flagged_by(kernel)
    print(f'{kernel.__name__}: flagged under {[f"0x{p:02X}" for p in got]}')
    assert got == expected
    with pytest.raises(AssertionError, match='out'):
        rg.same_bits_across({p: {'out': run(kernel, p)} for p in rg.PATTERNS})


def test_a_write_into_an_operand_is_flagged():
    with pytest.raises(AssertionError, match='writes_operand: the call wrote into an operand it only reads'):
        run(writes_operand, rg.ZERO)
    x = torch.ones(64)
    view, buf = rg.embedded(x, rg.NAN)
    buf[view.data_ptr() - buf.data_ptr() - 1] = 0
    with pytest.raises(AssertionError, match='the band before the operand was written'):
        rg.assert_unwritten(buf, view, rg.NAN, rg.view_bytes(view))


def test_a_non_finite_result_is_flagged_even_when_the_runs_agree():
    bad = {'out': np.array([1., np.inf], np.float32)}
    with pytest.raises(AssertionError, match=r'out: 1 non-finite values in run 0xFF, first at \(1,\)'):
        rg.same_bits_across({rg.NAN: bad, rg.ZERO: bad})
    rg.same_bits_across({rg.NAN: {'idx': np.array([3, -1])}, rg.ZERO: {'idx': np.array([3, -1])}})   # integers: bits only
    with pytest.raises(AssertionError, match=r'w: 1 of 6 elements differ.*index \(1, 2\): 5.0 vs 6.0'):
        rg.same_bits_across({'a': {'w': torch.tensor([[0., 1, 2], [3, 4, 5]])}, 'b': {'w': torch.tensor([[0., 1, 2], [3, 4, 6]])}})
    # -0.0 and 0.0 are different bits
    with pytest.raises(AssertionError, match='differ'):
        rg.same_bits_across({'a': {'w': torch.tensor([0.])}, 'b': {'w': torch.tensor([-0.])}})


def test_recorded_pointers_sees_structures_and_restores_the_handle():
    import ctypes

    class S(ctypes.Structure):
        _fields_ = [('p', ctypes.c_void_p), ('n', ctypes.c_int32)]

    class Lib:
        def f(self, *a):
            return 7
    lib = Lib()
    orig = lib.f
    with rg.recorded_pointers(lib, ['f']) as seen:
        assert lib.f(ctypes.c_void_p(4096), 5, S(8192, 3), ctypes.byref(S(12288, 1)), (ctypes.c_void_p * 2)(16384, 0), None, 1.5) == 7
    assert {4096, 8192, 12288, 16384} <= seen and lib.f == orig
    t = torch.zeros(4)
    with pytest.raises(AssertionError, match='given a copy'):
        rg.assert_received(seen, x=t)
