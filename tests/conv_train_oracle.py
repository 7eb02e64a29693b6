"""fp64 statements of the trainable convolution (test helper, not a conftest): what csrc/conv_train.hip and
celldetection_amd/nn/conv.py must compute, written index by index from the "Trainable convolution" section of include/cpn_hip.h.

* ``pack_forward`` / ``pack_dgrad``: the two record layouts ``cpn_conv2d`` reads;
* ``dgrad``: the input gradient as the identity states it -- a stride-1 conv of dY with the taps flipped and the channel roles
  swapped;
* ``wgrad`` / ``bgrad``: the weight and bias gradients, and ``S`` = sum |dY| |X| per weight (sum |dY| per bias);
* ``WRONG_RULES``: rules one could implement by mistake.  tests/test_conv_train.py shows that each of them disagrees with torch's own
  autograd on the cases used, so a kernel that follows one of them cannot pass.

Tensors are torch float64 on the CPU, NCHW; ``rule`` selects a wrong rule (None: the right one).
"""
import torch
import torch.nn.functional as F

WRONG_RULES = ('taps_not_flipped', 'channels_not_swapped', 'tap_shifted', 'padding_ignored_at_one_border', 'last_slab_dropped',
               'bias_over_wrong_axis')


def pack_forward(w):
    """w [Cout, Cin, k, k] -> [(Cin / 32) k k items (+ one zero item when odd), Cout, 32]: item (chunk, ky * k + kx), output channel
    co, lane c = w[co, 32 chunk + c, ky, kx]."""
    cout, cin, k, _ = w.shape
    items = cin // 32 * k * k
    out = torch.zeros(items + items % 2, cout, 32, dtype=w.dtype)
    for chunk in range(cin // 32):
        for ky in range(k):
            for kx in range(k):
                out[chunk * k * k + ky * k + kx] = w[:, 32 * chunk:32 * chunk + 32, ky, kx]
    return out


def pack_dgrad(w, rule=None):
    """w [Cout, Cin, k, k] -> [(Cout / 32) k k items (+ one), Cin, 32]: item (chunk, ky * k + kx), output channel ci, lane c =
    w[32 chunk + c, ci, k - 1 - ky, k - 1 - kx]."""
    cout, cin, k, _ = w.shape
    if rule == 'channels_not_swapped':
        assert cout == cin
        w = w.transpose(0, 1)
    items = cout // 32 * k * k
    out = torch.zeros(items + items % 2, cin, 32, dtype=w.dtype)
    for chunk in range(cout // 32):
        for ky in range(k):
            for kx in range(k):
                sy, sx = (ky, kx) if rule == 'taps_not_flipped' else (k - 1 - ky, k - 1 - kx)
                if rule == 'tap_shifted':
                    sx = (sx + 1) % k
                out[chunk * k * k + ky * k + kx] = w[32 * chunk:32 * chunk + 32, :, sy, sx].transpose(0, 1)
    return out


def unpack(records, reduced, k):
    """records (without regard to a zero item) -> the dense conv weight [out channels, reduced channels, k, k] they state."""
    items = reduced // 32 * k * k
    outc = records.shape[1]
    return records[:items].reshape(reduced // 32, k, k, outc, 32).permute(3, 0, 4, 1, 2).reshape(outc, reduced, k, k)


def dgrad(dy, w, rule=None):
    """dX = the stride-1, padding k // 2 conv of dY with the weights the dgrad pack states."""
    cout, cin, k, _ = w.shape
    return F.conv2d(dy.double(), unpack(pack_dgrad(w.double(), rule), cout, k), None, 1, k // 2)


def _shifted(x, ky, kx, k, rule=None):
    """X[n, ci, y + ky - p, x + kx - p] for every (y, x), zeros outside the image."""
    p = k // 2
    n, c, h, w = x.shape
    if rule == 'padding_ignored_at_one_border':  # the left border reads the pixels at the end of the row above instead of zeros
        flat = F.pad(x.reshape(n, c, h * w), (p, p))
        rows = torch.stack([flat[..., y * w:y * w + w + 2 * p] for y in range(h)], 2)  # [n, c, h, w + 2p]
        right = torch.arange(w + 2 * p) >= w + p
        rows = torch.where(right, torch.zeros_like(rows), rows)
        xp = F.pad(rows, (0, 0, p, p))
    else:
        xp = F.pad(x, (p, p, p, p))
    if rule == 'tap_shifted':
        xp = F.pad(xp, (0, 1))
        kx = kx + 1
    return xp[:, :, ky:ky + h, kx:kx + w]


def wgrad(x, dy, k, rule=None, slab_rows=None):
    """-> (dW [Cout, Cin, k, k], S): dW[co, ci, ky, kx] = sum over n, y, x of dY[n, co, y, x] X[n, ci, y + ky - p, x + kx - p]."""
    x, dy = x.double(), dy.double()
    if rule == 'last_slab_dropped':  # the pixels of the last slab of slab_rows image rows (of the N * H rows) take no part
        n, co, h, w = dy.shape
        rows = n * h
        keep = (rows - 1) // slab_rows * slab_rows
        mask = (torch.arange(rows) < keep).reshape(n, 1, h, 1)
        dy = dy * mask
    dw = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=torch.float64)
    S = torch.zeros_like(dw)
    for ky in range(k):
        for kx in range(k):
            xs = _shifted(x, ky, kx, k, rule)
            dw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', dy, xs)
            S[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', dy.abs(), xs.abs())
    return dw, S


def bgrad(dy, rule=None):
    """-> (db [Cout], S): the sum of dY over n, y, x."""
    dy = dy.double()
    if rule == 'bias_over_wrong_axis':  # the NHWC memory read as if it were NCHW
        n, c, h, w = dy.shape
        dy = dy.permute(0, 2, 3, 1).reshape(n, c, h, w)
    return dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def autograd64(x, w, b, dy):
    """torch's own fp64 autograd of F.conv2d(x, w, b, 1, k // 2) -> (y, dX, dW, db)."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(x, w, b, 1, w.shape[2] // 2)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, None if b is None else b.grad
