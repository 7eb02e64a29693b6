"""fp64 statements of the trainable concat convolution (test helper, not a conftest): what csrc/cat_conv_train.hip and
``celldetection_amd.nn.cat_conv2d`` must compute, written index by index from the "Trainable concat convolution" section of
include/cpn_hip.h.

* ``src_index``: the nearest map, ``min(floor(fl32(d) * fl32(in / out)), in - 1)`` in float32 like the kernels;
* ``resize``: the resized top; ``forward``: the conv over the concat, the lateral first;
* ``d_lateral`` / ``top_gradient_at_lateral_size`` (``T``): the two halves of the input gradient of the concat, each the stride-1 conv
  of dY with the flipped, role-swapped weights of its half;
* ``d_top``: the footprint sum of ``T`` (the adjoint of the resize), and ``footprints``: the dst ranges per source index;
* ``wgrad`` / ``bgrad``: the weight and bias gradients over the virtual concat with ``S`` = sum |dY| |X|;
* ``inner_then_resize`` / ``inner_gradients``: the 1x1 inner conv applied before the resize, and its gradients;
* ``WRONG_RULES``: rules one could implement by mistake.  tests/test_cat_conv.py shows that each of them disagrees with torch's own
  autograd of the stock expression at the sizes it picks.

Tensors are torch float64 on the CPU, NCHW; ``lateral=None`` is the bridge level (the top resized by exactly 2); ``rule`` selects a
wrong rule (None: the right one).
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_train_oracle as dense

WRONG_RULES = ('round_to_nearest', 'top_first', 'integer_footprint', 'inner_gradient_not_summed', 'taps_not_flipped')


def src_index(out_size, in_size, rule=None):
    """-> int64 [out_size]: the source index every dst index reads."""
    d = np.arange(out_size)
    if rule == 'integer_footprint':
        s = d * in_size // out_size
    else:
        scale = np.float32(in_size) / np.float32(out_size)
        prod = d.astype(np.float32) * scale
        s = (np.rint(prod) if rule == 'round_to_nearest' else np.floor(prod)).astype(np.int64)
    return torch.as_tensor(np.minimum(s, in_size - 1), dtype=torch.int64)


def out_size(lateral, top):
    return (2 * top.shape[2], 2 * top.shape[3]) if lateral is None else tuple(lateral.shape[2:])


def resize(top, size, rule=None):
    sy, sx = src_index(size[0], top.shape[2], rule), src_index(size[1], top.shape[3], rule)
    return top[:, :, sy][:, :, :, sx]


def concat(lateral, top, rule=None):
    up = resize(top.double(), out_size(lateral, top), rule if rule in ('round_to_nearest', 'integer_footprint') else None)
    if lateral is None:
        return up
    return torch.cat((up, lateral.double()) if rule == 'top_first' else (lateral.double(), up), 1)


def forward(lateral, top, w, b=None, rule=None):
    k = w.shape[2]
    return F.conv2d(concat(lateral, top, rule), w.double(), None if b is None else b.double(), 1, k // 2)


def d_lateral(dy, w, c0, rule=None):
    """dcat[:, :C0]: the dgrad conv of the lateral's half of the weights."""
    part = w[:, w.shape[1] - c0:] if rule == 'top_first' else w[:, :c0]
    return dense.dgrad(dy, part.double(), 'taps_not_flipped' if rule == 'taps_not_flipped' else None)


def top_gradient_at_lateral_size(dy, w, c0, rule=None):
    """T = dcat[:, C0:], at the lateral's size."""
    part = w[:, :w.shape[1] - c0] if rule == 'top_first' else w[:, c0:]
    return dense.dgrad(dy, part.double(), 'taps_not_flipped' if rule == 'taps_not_flipped' else None)


def footprints(out_size_, in_size, rule=None):
    """-> [(lo, hi)] per source index: the dst range [lo, hi) that reads it (asserts that it IS one contiguous range)."""
    s = src_index(out_size_, in_size, rule).tolist()
    out = []
    for i in range(in_size):
        hits = [d for d, v in enumerate(s) if v == i]
        assert hits == list(range(hits[0], hits[-1] + 1)) if hits else True, (out_size_, in_size, i, hits)
        out.append((hits[0], hits[-1] + 1) if hits else (0, 0))
    return out


def d_top(t, size, rule=None):
    """-> (d_top [N, C, h, w], S = the footprint sum of |T|, F = footprint sizes [h, w]): d_top[n, c, i, j] = sum of T[n, c, y, x]
    over src(y) = i, src(x) = j."""
    t = t.double()
    h, w = size
    fy = footprints(t.shape[2], h, rule if rule != 'inner_gradient_not_summed' else None)
    fx = footprints(t.shape[3], w, rule if rule != 'inner_gradient_not_summed' else None)
    out = torch.zeros(t.shape[0], t.shape[1], h, w, dtype=torch.float64)
    S = torch.zeros_like(out)
    count = torch.zeros(h, w, dtype=torch.int64)
    for i, (y0, y1) in enumerate(fy):
        for j, (x0, x1) in enumerate(fx):
            if y1 > y0 and x1 > x0:
                if rule == 'inner_gradient_not_summed':  # the first pixel of the footprint stands for all of it
                    out[:, :, i, j], S[:, :, i, j] = t[:, :, y0, x0], t[:, :, y0, x0].abs()
                else:
                    out[:, :, i, j] = t[:, :, y0:y1, x0:x1].sum((2, 3))
                    S[:, :, i, j] = t[:, :, y0:y1, x0:x1].abs().sum((2, 3))
                count[i, j] = (y1 - y0) * (x1 - x0)
    return out, S, count


def wgrad(lateral, top, dy, k, rule=None):
    """-> (dW [Cout, C0 + C1, k, k], S) over the virtual concat."""
    return dense.wgrad(concat(lateral, top, rule), dy, k)


def bgrad(dy):
    return dense.bgrad(dy)


def inner_then_resize(last, wi, bi, size):
    """The decoder's top: the 1x1 inner conv at the low resolution, then the resize (what UNetDecoder computes)."""
    return resize(F.conv2d(last.double(), wi.double(), None if bi is None else bi.double()), size)


def inner_gradients(last, wi, dtop_hi, rule=None):
    """Gradients of ``resize(inner(last))`` for the gradient ``dtop_hi`` at the high resolution -> (d_last, dW_inner, db_inner): the
    footprint sum first, then the 1x1 conv's own gradients at the low resolution."""
    g = d_top(dtop_hi, last.shape[2:], rule)[0]
    d_last = F.conv2d(g, wi.double().transpose(0, 1))
    dw = torch.einsum('nohw,nihw->oi', g, last.double())[:, :, None, None]
    return d_last, dw, g.sum((0, 2, 3))


def autograd64(lateral, top, w, b, dy):
    """torch's own fp64 autograd of the stock expression -> (y, d_lateral | None, d_top, dW, db | None)."""
    lat = None if lateral is None else lateral.double().clone().requires_grad_(True)
    tp = top.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    if lat is None:
        x = F.interpolate(tp, scale_factor=2, mode='nearest')
    else:
        x = torch.cat((lat, F.interpolate(tp, size=lat.shape[2:], mode='nearest')), 1)
    y = F.conv2d(x, w, b, padding=w.shape[2] // 2)
    y.backward(dy.double())
    return y.detach(), None if lat is None else lat.grad, tp.grad, w.grad, None if b is None else b.grad
