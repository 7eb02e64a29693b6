"""fp64 statements of the trainable image conv (the "Trainable image conv" section of include/cpn_hip.h), written from the rules and
sharing no code with the kernels (test helper, not a conftest).

The conv: y[n, co, y, x] = sum over (c, ky, kx) of Xq[n, c, y + ky, x + kx] w[co, c, ky, kx] (+ b[co]) with Xq the image with one
zero in front of every row and column (and enough behind); the output has the image's size; dW and db are its gradients.  The pad is
the layout [N][H + 2][W + 3][4] bf16 with the image at (1, 1), the pack the record layout [3][Cout][16], (kx 0..3, c 0..3) with
zeros at kx = 3 and c >= C.

Every statement takes ``rule``: None, or one of WRONG_RULES -- a plausible mistake, which tests/test_image_conv.py shows the cases
tell apart from the right rule.
"""
import torch
import torch.nn.functional as F

WRONG_RULES = ('taps_not_offset', 'kx_ky_swapped', 'kx3_leaks', 'channel_leaks', 'stride_2', 'padding_0', 'last_slab_dropped',
               'bias_twice')


def _padded(x, rule=None):
    """The image with the zero border; 4 columns / 3 rows of taps starting at (y, x) stay inside it."""
    front = 0 if rule == 'taps_not_offset' else 1
    return F.pad(x.double(), (front, 6 - front, front, 6 - front))


def out_size(h, w, rule=None):
    if rule == 'stride_2':
        return (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if rule == 'padding_0':
        return h - 2, w - 2
    return h, w


def _patch(xq, ky, kx, ho, wo, rule=None):
    """Xq[n, c, s y + ky, s x + kx] for all (y, x) of the output."""
    s = 2 if rule == 'stride_2' else 1
    if rule == 'padding_0':  # the window starts one pixel inside the image
        ky, kx = ky + 1, kx + 1
    return xq[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s]


def forward(x, w, b=None, rule=None):
    ho, wo = out_size(*x.shape[2:], rule)
    xq, w = _padded(x, rule), w.double()
    y = torch.zeros(x.shape[0], w.shape[0], max(ho, 0), max(wo, 0), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            tap = w[:, :, kx, ky] if rule == 'kx_ky_swapped' else w[:, :, ky, kx]
            y += torch.einsum('nchw,oc->nohw', _patch(xq, ky, kx, ho, wo, rule), tap)
    if b is not None:
        y = y + (2 if rule == 'bias_twice' else 1) * b.double().reshape(1, -1, 1, 1)
    return y


def wgrad(x, dy, rule=None, slab_rows=None):
    """-> (dW [Cout, C, 3, 3], S the sum of the absolute terms).  ``slab_rows`` matters to 'last_slab_dropped' alone; with the rules
    that change the output's size ``dy`` has that size."""
    n, c, h, w = x.shape
    ho, wo = out_size(h, w, rule)
    assert tuple(dy.shape[2:]) == (ho, wo), (tuple(dy.shape), ho, wo)
    xq, dy = _padded(x, rule), dy.double().clone()
    if rule == 'last_slab_dropped':
        rows = dy.permute(0, 2, 1, 3).reshape(n * ho, -1, wo)  # the N * H output rows in order
        last = (n * ho - 1) // slab_rows * slab_rows
        rows[last:] = 0
        dy = rows.reshape(n, ho, -1, wo).permute(0, 2, 1, 3)
    dw = torch.zeros(dy.shape[1], c, 3, 3, dtype=torch.float64)
    S = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(4 if rule == 'kx3_leaks' else 3):
            p = _patch(xq, ky, kx, ho, wo, rule)
            a, b_ = (kx, ky) if rule == 'kx_ky_swapped' else (ky, min(kx, 2))  # (a leaking column 3 lands in its neighbour)
            dw[:, :, a, b_] += torch.einsum('nohw,nchw->oc', dy, p)
            S[:, :, a, b_] += torch.einsum('nohw,nchw->oc', dy.abs(), p.abs())
    if rule == 'channel_leaks' and c < 4:  # the record's four channels written out as if all were real
        wide = torch.zeros(dy.shape[1], 3, 3, 4, dtype=torch.float64)
        wide[..., :c] = dw.permute(0, 2, 3, 1)
        dw = wide.reshape(-1)[:dw.numel()].reshape(dw.shape)
    return dw, S


def wgrad_slabs(x, dy, slab_rows):
    """dW as the sum over the slab partition: slabs of ``slab_rows`` of the N * H image rows, each summed on its own, the slabs then
    added in ascending order -> (dW, the number of slabs)."""
    n, c, h, w = x.shape
    rows = n * h
    slab_rows = min(slab_rows, rows)
    total, slabs = torch.zeros(dy.shape[1], c, 3, 3, dtype=torch.float64), 0
    for r0 in range(0, rows, slab_rows):
        flat = dy.double().permute(0, 2, 1, 3).reshape(rows, -1, w).clone()
        keep = torch.zeros(rows, dtype=torch.bool)
        keep[r0:r0 + slab_rows] = True
        flat[~keep] = 0
        total += wgrad(x, flat.reshape(n, h, -1, w).permute(0, 2, 1, 3))[0]
        slabs += 1
    return total, slabs


def bgrad(dy):
    dy = dy.double()
    return dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def pad(x):
    """x [N, C, H, W] -> bf16 [N, H + 2, W + 3, 4]: round to nearest even (torch's own conversion), zeros elsewhere."""
    n, c, h, w = x.shape
    xq = torch.zeros(n, h + 2, w + 3, 4, dtype=torch.bfloat16)
    xq[:, 1:h + 1, 1:w + 1, :c] = x.to(torch.bfloat16).permute(0, 2, 3, 1)
    return xq


def pack(weight):
    """weight [Cout, C, 3, 3] -> bf16 [3, Cout, 16]: round to nearest even (torch's own conversion), zeros elsewhere."""
    cout, c = weight.shape[:2]
    rec = torch.zeros(3, cout, 4, 4, dtype=torch.bfloat16)
    rec[:, :, :3, :c] = weight.to(torch.bfloat16).permute(2, 0, 3, 1)  # [ky, co, kx, c]
    return rec.reshape(3, cout, 16)


def autograd64(x, w, b, dy):
    """torch's own float64 CPU autograd of the stock expression -> (y, dW, db)."""
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(x.double(), w, b, stride=1, padding=1)
    y.backward(dy.double())
    return y.detach(), w.grad, None if b is None else b.grad
