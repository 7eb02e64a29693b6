"""Read guards: does a result depend on bytes the kernel was never given?  (test helper, not a conftest)

The suite's output guard bands catch wrong writes, its fp64 references wrong arithmetic on the bytes a kernel was meant to read.
This helper catches the third kind of error: a load one element past a row, a tile past the end of an operand, a region of the
arena no op of this run has written.  The technique is the same at every level: the operand lies inside a larger buffer (or the
arena is pre-filled) with a chosen byte pattern, the call runs once per pattern, and every result must come back with identical
bits.  No tolerance appears: the comparison is between runs of the same code on the same operands.

The patterns are whole-buffer byte fills, so they mean something in every storage type:

    pattern   bf16            fp32            e4m3    int32
    0xFF      NaN             NaN             NaN     -1
    0x00      0               0               0       0
    0x3C      about 0.0115    about 0.0115    1.5     1010580540

0xFF poisons every sum it enters (a product with zero included); 0x3C is plausible data and survives the fmax or clamp that
would mask a NaN; 0x00 is the value an over-read most often "works" with, the run the other two are compared against.

tests/test_read_guards.py shows on the CPU, on numpy emulations of each fault, that the judge is not vacuous.
"""
import contextlib
import ctypes

import numpy as np
import torch

NAN, ZERO, PLAUSIBLE = 0xFF, 0x00, 0x3C
PATTERNS = (NAN, ZERO, PLAUSIBLE)
ALIGN = 256        # a fresh allocation and every arena tensor start at a multiple of 256 bytes
MIN_BAND = 4096    # bytes


def _row_bytes(t):
    """One full row of pixels at the tensor's channel stride: W x C elements of an NHWC (channels_last) tensor, the last two
    dimensions of a contiguous one."""
    if t.dim() == 4 and t.stride(1) == 1 and t.shape[1] > 1 and not t.is_contiguous():
        return t.shape[3] * t.shape[1] * t.element_size()  # channels_last: W x C
    if t.dim() >= 2:
        return t.shape[-1] * t.shape[-2] * t.element_size()
    return t.element_size()


def embedded(t, pattern):
    """-> (view, buffer): ``view`` has the shape, dtype, strides and memory format of ``t`` (contiguous or channels_last) and its
    values, and lies inside the flat uint8 ``buffer`` between two bands filled with the byte ``pattern``.  Each band holds at least
    one full row of pixels and at least MIN_BAND bytes; the view starts at a multiple of ALIGN bytes, like a fresh allocation, so a
    kernel takes the vector paths it takes today."""
    assert isinstance(t, torch.Tensor)
    cl = t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)
    assert t.is_contiguous() or cl, 'embedded() places contiguous and channels_last tensors only'
    nbytes = t.numel() * t.element_size()
    band = -(-max(_row_bytes(t), MIN_BAND) // ALIGN) * ALIGN
    buf = torch.full((band + nbytes + band + ALIGN,), pattern, dtype=torch.uint8, device=t.device)
    start = band + (-(buf.data_ptr() + band)) % ALIGN
    flat = buf[start:start + nbytes].view(t.dtype)
    view = flat.view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2) if cl else flat.view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % ALIGN == 0 and view.data_ptr() - buf.data_ptr() >= band
    assert buf.data_ptr() + buf.numel() - (view.data_ptr() + nbytes) >= band
    same_strides = all(a == b for a, b, n in zip(view.stride(), t.stride(), t.shape) if n > 1)  # (a dimension of one element has no stride)
    assert view.shape == t.shape and same_strides and view.dtype == t.dtype
    return view, buf


def view_bytes(view):
    """The view's storage bytes, in memory order, on the CPU."""
    v = view.detach()
    if v.dim() == 4 and not v.is_contiguous():
        v = v.permute(0, 2, 3, 1)
    assert v.is_contiguous()
    return v.reshape(-1).view(torch.uint8).cpu().clone()


def assert_unwritten(buffer, view, pattern, before=None, name='operand'):
    """Both bands of ``buffer`` still hold ``pattern``; unless the call is documented to update the operand (``before`` None), the
    view holds the bytes ``before`` = view_bytes(view) taken ahead of the call."""
    host = buffer.cpu()
    a = view.data_ptr() - buffer.data_ptr()
    b = a + view.numel() * view.element_size()
    for band, lo in (('before', host[:a]), ('after', host[b:])):
        bad = (lo != pattern).nonzero()
        assert bad.numel() == 0, f'{name}: the band {band} the operand was written ({bad.numel()} bytes, first at byte ' \
                                 f'{int(bad[0])} of the band: 0x{int(lo[int(bad[0])]):02X}, pattern 0x{pattern:02X})'
    if before is not None:
        bad = (host[a:b] != before).nonzero()
        assert bad.numel() == 0, f'{name}: the call wrote into an operand it only reads ({bad.numel()} bytes, first at byte {int(bad[0])})'


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach()
        a = a.float().cpu().numpy() if a.dtype == torch.bfloat16 else a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a, a.reshape(-1).view(np.uint8).reshape(a.size, -1) if a.size else a.reshape(0, 1)


def same_bits_across(results, finite=True):
    """``results``: {pattern or run name: {result name: tensor | array | None}}.  Every result is finite and bit-equal across the
    runs; the first difference is reported by name, index and both values."""
    runs = list(results)
    first = results[runs[0]]
    for run in runs:
        assert list(results[run]) == list(first), f'runs {runs[0]} and {run} return different results: {list(first)} vs {list(results[run])}'
    for name, a in first.items():
        if a is None:
            assert all(results[r][name] is None for r in runs), f'{name}: None in one run only'
            continue
        a, abits = _bits(a)
        if finite and a.dtype.kind == 'f':
            for run in runs:
                v = _bits(results[run][name])[0]
                bad = np.argwhere(~np.isfinite(v))
                assert len(bad) == 0, f'{name}: {len(bad)} non-finite values in run {_tag(run)}, first at {tuple(int(j) for j in bad[0])}: {v[tuple(bad[0])]}'
        for run in runs[1:]:
            b, bbits = _bits(results[run][name])
            assert a.shape == b.shape and a.dtype == b.dtype, f'{name}: {a.shape} {a.dtype} in run {_tag(runs[0])}, {b.shape} {b.dtype} in run {_tag(run)}'
            diff = (abits != bbits).any(1).nonzero()[0]
            if len(diff):
                i = np.unravel_index(int(diff[0]), a.shape) if a.ndim else ()
                raise AssertionError(f'{name}: {len(diff)} of {a.size} elements differ between runs {_tag(runs[0])} and {_tag(run)}: the result '
                                     f'depends on bytes the call was not given; first at index {tuple(int(j) for j in i)}: {a[i].item()!r} vs {b[i].item()!r}')


def _tag(run):
    return f'0x{run:02X}' if isinstance(run, int) else str(run)


# ---- proof that the kernel saw the embedded storage and not a copy ---------------------------------------------------------------------
def _addresses(arg, out, depth=0):
    if arg is None or isinstance(arg, (float, bytes, str)):
        return
    if isinstance(arg, int):
        out.add(arg)
    elif isinstance(arg, ctypes.c_void_p):
        out.add(arg.value or 0)
    elif isinstance(arg, ctypes.Structure) and depth < 3:
        for field in arg._fields_:
            _addresses(getattr(arg, field[0]), out, depth + 1)
    elif isinstance(arg, ctypes.Array) and depth < 3:
        for item in arg:
            _addresses(item, out, depth + 1)
    elif hasattr(arg, '_obj') and depth < 3:  # byref(...)
        _addresses(arg._obj, out, depth + 1)
    elif hasattr(arg, 'value') and isinstance(getattr(arg, 'value'), int):
        out.add(arg.value)


@contextlib.contextmanager
def recorded_pointers(lib, names):
    """Wraps the entry points ``names`` on the loaded library handle for the duration of the block -> the set of every integer the
    library received through them (pointer arguments, the fields of structures and pointer arrays passed by value or reference
    included).  The way the library is loaded stays as it is; the handle gets its own functions back on exit."""
    seen, saved = set(), {}

    def wrap(fn):
        def call(*args):
            for i, a in enumerate(args):
                _addresses(a, seen)
                # a table of records passed as (pointer, count), e.g. the CpnOptimTensor records of cpn_optim_upload
                if isinstance(a, ctypes._Pointer) and issubclass(a._type_, ctypes.Structure) and i + 1 < len(args) \
                        and isinstance(args[i + 1], int) and 0 < args[i + 1] <= 1 << 16:
                    for j in range(args[i + 1]):
                        _addresses(a[j], seen)
            return fn(*args)
        return call

    for name in names:
        saved[name] = getattr(lib, name)
        setattr(lib, name, wrap(saved[name]))
    try:
        yield seen
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def assert_received(seen, **views):
    for name, v in views.items():
        if v is not None:
            assert v.data_ptr() in seen, f'{name}: the library never received the embedded operand at 0x{v.data_ptr():x}: it was given a copy'


class Embedding:
    """The operands of one call embedded under one pattern; with ``pattern`` None every method leaves things as they are, so a
    runner takes an optional ``embed=pattern`` argument at the cost of three lines.

        e = Embedding(embed)
        src = e('src0', src)                      # the view inside its poisoned buffer (None stays None)
        with e.watch(lib, 'cpn_conv2d'):          # records what the entry points receive
            lib.cpn_conv2d(...)
        torch.cuda.synchronize()
        e.check()                                 # every view was received, its bands are intact, its bytes unchanged
    """

    def __init__(self, pattern):
        self.pattern, self.items, self.seen = pattern, {}, set()

    def __bool__(self):
        return self.pattern is not None

    def __call__(self, name, t, updated=False):
        """``updated``: the call is documented to update this operand; its bytes are not compared, its bands are."""
        if self.pattern is None or t is None:
            return t
        view, buf = embedded(t, self.pattern)
        self.items[name] = (view, buf, None if updated else view_bytes(view))
        return view

    @contextlib.contextmanager
    def watch(self, lib, *names):
        if self.pattern is None:
            yield
            return
        with recorded_pointers(lib, names) as seen:
            try:
                yield
            finally:
                self.seen |= seen

    def check(self, received=True):
        for name, (view, buf, before) in self.items.items():
            if received:
                assert_received(self.seen, **{name: view})
            assert_unwritten(buf, view, self.pattern, before, name)
