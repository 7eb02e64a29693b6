"""fp64 statements of the trainable bilinear resize (test helper, not a conftest): what csrc/bilinear_train.hip,
``celldetection_amd.nn.bilinear_resize`` and ``nn.resized_conv2d`` must compute, written index by index from the "Trainable bilinear
resize" section of include/cpn_hip.h, and the bounds the GPU tests hold them to.

* ``taps``: ``ba_tap`` of csrc/bilinear_adjoint.h in numpy -- ``f = max(scale * (d + 0.5) - 0.5, 0)``, ``i0 = int(f)``,
  ``i1 = i0 + (i0 < in - 1)``, ``lambda = fl(f - i0)`` -- in float32 like the kernels, the coordinate ``fused`` (one fma, one
  rounding: the activations' resize and the conv loader, as compiled) or split (product and difference rounded each: the fp32
  planes' resize), or in float64 (torch's own float64 rule);
* ``weights``: the matrix ``M[d, i] = ba_weight(d, i)`` -- ``fl(1 - lambda)`` at ``i0`` plus ``lambda`` at ``i1`` -- as float64;
  ``footprints``: the dst range per source index, ``[first(i - 1), first(i + 1))``;
* ``resize`` = ``My x Mx^T`` and ``adjoint``, its transpose, with ``S`` = the same sums over absolute values and the footprint sizes;
* ``forward`` / ``top_gradient`` (``T``) / ``d_input`` / ``wgrad`` / ``bgrad`` of the resized conv;
* ``WRONG_RULES``: rules one could implement by mistake; tests/test_bilinear_resize.py shows that each of them disagrees with torch's
  own autograd of the stock expression, and that the judges below reject it;
* the judges: ``blend_window`` (forward of the resize), ``adjoint_bounds``, ``conv_operand`` (the hidden bf16 operand of the conv and
  of the weight gradient), ``wgrad_tolerance``; ``emulate_*``: the stated fp32 arithmetic on the CPU.

Bounds (derived, none measured).  u = 2^-24.  A blended value is ``hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11)`` in fp32:
on its way to the result every term meets the rounding of its ``h = 1 - l`` (where it has one), a product, a sum, the second
``h``, a product and the last sum -- three roundings of sums, three of products and differences at most, so the fp32 result lies
within ``gamma(6) * B`` of the fp64 blend with the same fp32 lambdas, ``B = sum w_i |v_i|``; a stored bf16 value is any bf16 value that
window can round to.  The adjoint adds F = footprint size terms ``c * t`` with ``c = fl(wy * wx)``: one rounding of ``c``, one of the
product, at most F of the sums: ``gamma(F + 2) * sum |c t|``, plus one rounding of the result.

Tensors are torch float64 on the CPU, NCHW; ``rule`` selects a wrong rule (None: the right one).
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_bounds as cb
import conv_train_oracle as dense

WRONG_RULES = ('align_corners', 'unclamped', 'i1_not_clamped', 'adjoint_weights_swapped', 'adjoint_last_tap_single', 'dw_unresized')
_TAP_RULES = ('align_corners', 'unclamped', 'i1_not_clamped')


def taps(out_size, in_size, rule=None, dtype=np.float32, fused=True):
    """-> (i0, i1, lam) per dst index: int64, int64 and ``dtype`` arrays [out_size]."""
    t = dtype
    d = np.arange(out_size).astype(t)
    if rule == 'align_corners':
        scale = t(in_size - 1) / t(out_size - 1) if out_size > 1 else t(0)
        f = (scale * d).astype(t)
    else:
        scale = t(t(in_size) / t(out_size))
        if fused and t is np.float32:  # product and difference in one fma: one rounding (the fp64 expression is exact before it)
            f = (np.float64(scale) * (d + t(0.5)).astype(np.float64) - 0.5).astype(t)
        else:
            f = ((scale * (d + t(0.5))).astype(t) - t(0.5)).astype(t)
        if rule != 'unclamped':
            f = np.maximum(f, t(0))
    i0 = np.floor(f).astype(np.int64) if rule == 'unclamped' else f.astype(np.int64)
    lam = (f - i0.astype(t)).astype(t)
    i1 = i0 + 1 if rule == 'i1_not_clamped' else i0 + (i0 < in_size - 1)
    return i0, i1, lam


def weights(out_size, in_size, rule=None, dtype=np.float32, fused=True):
    """-> float64 [out_size, in_size]: M[d, i] = the coefficient with which dst d reads source i.  A tap outside the source (wrong
    rules only) is dropped, as zero padding would."""
    i0, i1, lam = taps(out_size, in_size, rule if rule in _TAP_RULES else None, dtype, fused)
    m = np.zeros((out_size, in_size), dtype=dtype)
    hi = (dtype(1) - lam).astype(dtype)
    if rule == 'adjoint_weights_swapped':
        hi, lam = lam, hi
    for d in range(out_size):
        if 0 <= i0[d] < in_size:
            m[d, i0[d]] = hi[d]
        if 0 <= i1[d] < in_size and not (rule == 'adjoint_last_tap_single' and i1[d] == i0[d]):
            m[d, i1[d]] = dtype(m[d, i1[d]] + lam[d])
    return torch.as_tensor(m.astype(np.float64))


def footprints(out_size, in_size, fused=True):
    """-> [(lo, hi)] per source index: the dst range whose i0 is i - 1 or i (asserts that it IS one contiguous, non-empty range and
    that every dst lies in the ranges of its i0 and i0 + 1 alone)."""
    i0 = taps(out_size, in_size, fused=fused)[0].tolist()
    assert i0 == sorted(i0) and i0[0] == 0 and i0[-1] == in_size - 1, (out_size, in_size)
    out = []
    for i in range(in_size):
        hits = [d for d, v in enumerate(i0) if v in (i - 1, i)]
        assert hits and hits == list(range(hits[0], hits[-1] + 1)), (out_size, in_size, i, hits)
        out.append((hits[0], hits[-1] + 1))
    cover = [sum(lo <= d < hi for lo, hi in out) for d in range(out_size)]
    assert cover == [2 if v < in_size - 1 else 1 for v in i0], (out_size, in_size)
    return out


def resize(x, size, rule=None, dtype=np.float32, fused=True):
    """-> B(x) [N, C, H, W] = My x Mx^T in float64."""
    my, mx = weights(size[0], x.shape[2], rule, dtype, fused), weights(size[1], x.shape[3], rule, dtype, fused)
    return torch.einsum('yi,ncij,xj->ncyx', my, x.double(), mx)


def adjoint(t, size, rule=None, dtype=np.float32, fused=True):
    """-> (B^T(t) [N, C, h, w], S = the same sum over |c t|, F = footprint sizes [h, w])."""
    t = t.double()
    my, mx = weights(t.shape[2], size[0], rule, dtype, fused), weights(t.shape[3], size[1], rule, dtype, fused)
    out = torch.einsum('yi,ncyx,xj->ncij', my, t, mx)
    S = torch.einsum('yi,ncyx,xj->ncij', my.abs(), t.abs(), mx.abs())
    fy, fx = footprints(t.shape[2], size[0], fused), footprints(t.shape[3], size[1], fused)
    count = torch.tensor([[(y1 - y0) * (x1 - x0) for x0, x1 in fx] for y0, y1 in fy], dtype=torch.int64)
    return out, S, count


def forward(x, w, b, size, rule=None, dtype=np.float32, fused=True):
    k = w.shape[2]
    return F.conv2d(resize(x, size, rule, dtype, fused), w.double(), None if b is None else b.double(), 1, k // 2)


def top_gradient(dy, w):
    """T = the gradient of the virtual resized tensor, at ``size``: the stride-1 conv of dY with the taps flipped and the channel
    roles swapped (any channel count; for multiples of 32 it is ``conv_train_oracle.dgrad``)."""
    return F.conv2d(dy.double(), w.double().flip(2, 3).transpose(0, 1), None, 1, w.shape[2] // 2)


def d_input(dy, w, low_size, rule=None, dtype=np.float32, fused=True):
    return adjoint(top_gradient(dy, w), low_size, rule, dtype, fused)[0]


def nearest_taps(x, size):
    """What 'dw_unresized' reads: x at the first tap of every pixel, unblended."""
    iy, ix = taps(size[0], x.shape[2])[0], taps(size[1], x.shape[3])[0]
    return x.double()[:, :, torch.as_tensor(iy)][:, :, :, torch.as_tensor(ix)]


def wgrad(x, dy, k, rule=None, dtype=np.float32, fused=True):
    """-> (dW [Cout, Cin, k, k], S) over the virtual resized tensor."""
    size = tuple(dy.shape[2:])
    operand = nearest_taps(x, size) if rule == 'dw_unresized' else resize(x, size, rule, dtype, fused)
    return dense.wgrad(operand, dy, k)


def bgrad(dy):
    return dense.bgrad(dy)


def autograd64(x, w, b, dy, size):
    """torch's own fp64 autograd of the stock expression -> (y, dx, dW, db | None)."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(F.interpolate(x, size=size, mode='bilinear', align_corners=False), w, b, padding=w.shape[2] // 2)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


# ---- the judges

BLEND_ROUNDINGS = 6


def blend_window(x, size, fused=True):
    """-> (X^ = the fp64 blend with the fp32 lambdas, d = gamma(6) B): the fp32 blend of the kernels lies in [X^ - d, X^ + d]."""
    ref = resize(x, size, fused=fused)
    return ref, cb.gamma(BLEND_ROUNDINGS) * resize(x.double().abs(), size, fused=fused)


def check_blend(name, got, x, size, stored='bf16'):
    """The forward of ``bilinear_resize``: a stored bf16 value is one the window can round to; an fp32 value lies in the window."""
    ref, d = blend_window(x, size, fused=stored == 'bf16')
    lo, hi = (cb.bf16_bounds(ref, d) if stored == 'bf16' else (ref - d, ref + d))
    return cb.check(name, got.double().cpu(), lo, hi, ref)


def adjoint_bounds(t, size, stored='bf16'):
    """-> dict(lo, hi, ref, S, count) for B^T(t): |result - ref| <= gamma(F + 2) S before the one rounding of a stored bf16 value."""
    ref, S, count = adjoint(t, size, fused=stored == 'bf16')
    d = cb.gamma(count.double() + 2.) * S
    lo, hi = (cb.bf16_bounds(ref, d) if stored == 'bf16' else (ref - d, ref + d))
    return dict(lo=lo, hi=hi, ref=ref, S=S, count=count)


def check_adjoint(name, got, t, size, stored='bf16'):
    b = adjoint_bounds(t, size, stored)
    return cb.check(name, got.double().cpu(), b['lo'], b['hi'], b['ref'], b['S'])


def conv_operand(x, size):
    """The operand the conv's loader and the weight gradient's staging hand to the MFMA: bf16(blend) -> (mid, half) with the
    kernel's bf16 value in [mid - half, mid + half] (``cb.hidden_bf16`` of the blend window)."""
    return cb.hidden_bf16(*blend_window(x, size))


def forward_bounds(x, wq, b, size):
    """-> (ref, S, d) of the conv on the virtual operand: the rule of tests/conv_bounds.py on X^, widened by sum |w| delta."""
    k = wq.shape[2]
    mid, half = conv_operand(x, size)
    return cb.conv_with_noise(mid, wq, b, 1, k // 2, n=cb.chain_length(k, k, x.shape[1]), x_half=half)


def wgrad_tolerance(x, dy, k, chain):
    """-> (ref, tol): |dW - ref| <= gamma(chain) sum |dy| (|X^| + delta) + sum |dy| delta + one fp32 rounding of the result."""
    size = tuple(dy.shape[2:])
    mid, half = conv_operand(x, size)
    ref = dense.wgrad(mid, dy, k)[0]
    S = dense.wgrad(mid.abs() + half, dy.abs(), k)[0]
    D = dense.wgrad(half, dy.abs(), k)[0]
    d = cb.gamma(chain) * S + D
    return ref, d + cb.U * (ref.abs() + d)


def check_wgrad(name, got, x, dy, k, chain):
    ref, tol = wgrad_tolerance(x, dy, k, chain)
    err = (got.double().cpu() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f'{name}: chain {chain}, largest error / bound {worst:.3f}')
    assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), (name, worst)
    return worst


# ---- the stated fp32 arithmetic on the CPU (what a kernel that follows the header computes)

def _f32(a):
    return np.asarray(a, dtype=np.float32)


def emulate_blend(x, size, rule=None, fused=True):
    """hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11) in float32, every operation rounded -> float32 tensor [N, C, H, W]."""
    x = _f32(x.numpy())
    y0, y1, ly = taps(size[0], x.shape[2], rule, fused=fused)
    x0, x1, lx = taps(size[1], x.shape[3], rule, fused=fused)
    pad = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))  # a tap outside the source (wrong rules only) reads a zero

    def at(iy, ix):
        return pad[:, :, np.clip(iy + 1, 0, x.shape[2] + 1)][:, :, :, np.clip(ix + 1, 0, x.shape[3] + 1)]

    ly, lx = ly[:, None], lx[None, :]
    hy, hx = _f32(1) - ly, _f32(1) - lx
    top = _f32(_f32(hx * at(y0, x0)) + _f32(lx * at(y0, x1)))
    bottom = _f32(_f32(hx * at(y1, x0)) + _f32(lx * at(y1, x1)))
    return torch.as_tensor(_f32(_f32(hy * top) + _f32(ly * bottom)))


def emulate_adjoint(t, size, rule=None, fused=True):
    """The footprint sum in float32, ascending row-major, c = fl(wy * wx) first, then one product and one add per term -> float32
    tensor [N, C, h, w]."""
    t = _f32(t.numpy())
    my, mx = _f32(weights(t.shape[2], size[0], rule, fused=fused).numpy()), _f32(weights(t.shape[3], size[1], rule, fused=fused).numpy())
    out = np.zeros(t.shape[:2] + tuple(size), dtype=np.float32)
    for i in range(size[0]):
        ys = np.nonzero(my[:, i])[0]
        for j in range(size[1]):
            xs = np.nonzero(mx[:, j])[0]
            acc = np.zeros(t.shape[:2], dtype=np.float32)
            for y in ys:
                for x in xs:
                    acc = _f32(acc + _f32(_f32(my[y, i] * mx[x, j]) * t[:, :, y, x]))
            out[:, :, i, j] = acc
    return torch.as_tensor(out)
