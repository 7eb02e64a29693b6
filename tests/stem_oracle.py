"""fp64 statements of the trainable stem and max-pool (the "Trainable stem and max-pool" section of include/cpn_hip.h), written from
the rules and sharing no code with the kernels (test helper, not a conftest).

The stem: y[n, co, oy, ox] = sum over (c, ky, kx) of Xp[n, c, 2 oy + ky, 2 ox + kx] w[co, c, ky, kx] (+ b[co]) with Xp the image
with 3 zeros in front of every row and column (and enough behind), Hout = (H - 1) // 2 + 1; dW and db are its gradients.  The pack
is the record layout [7][Cout][32], (kx 0..7, c 0..3) with zeros at kx = 7 and c >= C.

The pool: windows cut at the border, raster scan, a position takes over only when strictly greater (the first maximum wins); the
stored index is ty * k + tx; the gradient of an input pixel is the sum of dY over the windows whose index names it.

Every statement takes ``rule``: None, or one of WRONG_RULES -- a plausible mistake, which tests/test_stem.py shows the cases tell
apart from the right rule.
"""
import torch
import torch.nn.functional as F

WRONG_RULES = ('taps_not_offset', 'stride_1', 'kx_ky_swapped', 'kx7_leaks', 'channel_leaks', 'last_slab_dropped', 'last_maximum',
               'ties_split', 'every_maximum', 'odd_last_row_gets_gradient', 'window_clamped')


def out_size(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _padded(x, rule=None):
    """The image with the zero border; 8 columns / 7 rows of taps starting at (2 oy, 2 ox) stay inside it."""
    front = 0 if rule == 'taps_not_offset' else 3
    return F.pad(x.double(), (front, 12 - front, front, 12 - front))


def _patch(xp, ky, kx, ho, wo, rule=None):
    """Xp[n, c, s oy + ky, s ox + kx] for all (oy, ox)."""
    s = 1 if rule == 'stride_1' else 2
    return xp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s]


def forward(x, w, b=None, rule=None):
    ho, wo = out_size(*x.shape[2:])
    xp, w = _padded(x, rule), w.double()
    y = torch.zeros(x.shape[0], w.shape[0], ho, wo, dtype=torch.float64)
    for ky in range(7):
        for kx in range(7):
            tap = w[:, :, kx, ky] if rule == 'kx_ky_swapped' else w[:, :, ky, kx]
            y += torch.einsum('nchw,oc->nohw', _patch(xp, ky, kx, ho, wo, rule), tap)
    return y if b is None else y + b.double().reshape(1, -1, 1, 1)


def wgrad(x, dy, rule=None, slab_rows=None):
    """-> (dW [Cout, C, 7, 7], S the sum of the absolute terms).  ``slab_rows`` matters to 'last_slab_dropped' alone."""
    n, c, h, w = x.shape
    ho, wo = out_size(h, w)
    xp, dy = _padded(x, rule), dy.double().clone()
    if rule == 'last_slab_dropped':
        rows = dy.permute(0, 2, 1, 3).reshape(n * ho, -1, wo)  # the N * Hout output rows in order
        last = (n * ho - 1) // slab_rows * slab_rows
        rows[last:] = 0
        dy = rows.reshape(n, ho, -1, wo).permute(0, 2, 1, 3)
    dw = torch.zeros(dy.shape[1], c, 7, 7, dtype=torch.float64)
    S = torch.zeros_like(dw)
    for ky in range(7):
        for kx in range(8 if rule == 'kx7_leaks' else 7):
            p = _patch(xp, ky, kx, ho, wo, rule)
            a, b_ = (kx, ky) if rule == 'kx_ky_swapped' else (ky, min(kx, 6))  # (a leaking column 7 lands in its neighbour)
            dw[:, :, a, b_] += torch.einsum('nohw,nchw->oc', dy, p)
            S[:, :, a, b_] += torch.einsum('nohw,nchw->oc', dy.abs(), p.abs())
    if rule == 'channel_leaks' and c < 4:  # the record's four channels written out as if all were real
        wide = torch.zeros(dy.shape[1], 7, 7, 4, dtype=torch.float64)
        wide[..., :c] = dw.permute(0, 2, 3, 1)
        dw = wide.reshape(-1)[:dw.numel()].reshape(dw.shape)
    return dw, S


def bgrad(dy):
    dy = dy.double()
    return dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def pack(weight):
    """weight [Cout, C, 7, 7] -> bf16 [7, Cout, 32]: round to nearest even (torch's own conversion), zeros elsewhere."""
    cout, c = weight.shape[:2]
    rec = torch.zeros(7, cout, 8, 4, dtype=torch.bfloat16)
    rec[:, :, :7, :c] = weight.to(torch.bfloat16).permute(2, 0, 3, 1)  # [ky, co, kx, c]
    return rec.reshape(7, cout, 32)


def autograd64(x, w, b, dy):
    """torch's own float64 CPU autograd of the stock expression -> (y, dW, db)."""
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(x.double(), w, b, stride=2, padding=3)
    y.backward(dy.double())
    return y.detach(), w.grad, None if b is None else b.grad


# ---- the pool

def pool_out(size, k, s, pad, rule=None):
    if rule == 'odd_last_row_gets_gradient':  # ceil mode
        return -(-(size + 2 * pad - k) // s) + 1
    return (size + 2 * pad - k) // s + 1


def pool_forward(x, k, s, pad, rule=None):
    """-> (y in x's dtype, index uint8 [N, C, Hout, Wout]).  Comparisons are made on the values as they are (no rounding)."""
    n, c, h, w = x.shape
    ho, wo = pool_out(h, k, s, pad, rule), pool_out(w, k, s, pad, rule)
    y = torch.empty(n, c, ho, wo, dtype=x.dtype)
    index = torch.empty(n, c, ho, wo, dtype=torch.uint8)
    for oy in range(ho):
        for ox in range(wo):
            best = idx = None
            for ty in range(k):
                for tx in range(k):
                    iy, ix = oy * s - pad + ty, ox * s - pad + tx
                    if rule == 'window_clamped':
                        iy, ix = min(max(iy, 0), h - 1), min(max(ix, 0), w - 1)
                    if not (0 <= iy < h and 0 <= ix < w):
                        continue
                    v = x[:, :, iy, ix]
                    if best is None:
                        best, idx = v.clone(), torch.full(v.shape, ty * k + tx, dtype=torch.uint8)
                        continue
                    take = v >= best if rule == 'last_maximum' else v > best
                    best = torch.where(take, v, best)
                    idx = torch.where(take, torch.full_like(idx, ty * k + tx), idx)
            y[:, :, oy, ox], index[:, :, oy, ox] = best, idx
    return y, index


def pool_backward(dy, index, size, k, s, pad):
    """The index-routed gradient -> (dx float64 [N, C, H, W], S the sum of the absolute terms, the number of terms)."""
    n, c, ho, wo = dy.shape
    h, w = size
    dy = dy.double()
    dx = torch.zeros(n, c, h, w, dtype=torch.float64)
    S, count = torch.zeros_like(dx), torch.zeros(n, c, h, w, dtype=torch.int64)
    for oy in range(ho):
        for ox in range(wo):
            t = index[:, :, oy, ox].long()
            iy, ix = oy * s - pad + t // k, ox * s - pad + t % k
            assert bool(((iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)).all()), 'an index names a position outside the image'
            flat = (iy * w + ix).reshape(n, c, 1)
            g = dy[:, :, oy, ox].reshape(n, c, 1)
            dx.view(n, c, -1).scatter_add_(2, flat, g)
            S.view(n, c, -1).scatter_add_(2, flat, g.abs())
            count.view(n, c, -1).scatter_add_(2, flat, torch.ones_like(flat))
    return dx, S, count


def pool_gradient(x, dy, k, s, pad, rule=None):
    """The gradient from x itself -> dx float64.  The right rule is pool_backward(pool_forward(x)); 'ties_split' shares a window's
    gradient evenly among its maxima, 'every_maximum' gives each of them all of it."""
    n, c, h, w = x.shape
    if rule not in ('ties_split', 'every_maximum'):
        y, index = pool_forward(x, k, s, pad, rule)
        if rule == 'odd_last_row_gets_gradient':
            full = torch.zeros(n, c, y.shape[2], y.shape[3], dtype=torch.float64)
            full[:, :, :dy.shape[2], :dy.shape[3]] = dy
            full[:, :, dy.shape[2]:] = 1.
            full[:, :, :, dy.shape[3]:] = 1.
            dy = full
        if rule == 'window_clamped':  # a clamped forward names taps outside the image, which no pixel of the gather is: lost
            dx = torch.zeros(n, c, h, w, dtype=torch.float64)
            for oy in range(y.shape[2]):
                for ox in range(y.shape[3]):
                    t = index[:, :, oy, ox].long()
                    iy, ix = oy * s - pad + t // k, ox * s - pad + t % k
                    inside = ((iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)).double()
                    flat = (iy.clamp(0, h - 1) * w + ix.clamp(0, w - 1)).reshape(n, c, 1)
                    dx.view(n, c, -1).scatter_add_(2, flat, (dy.double()[:, :, oy, ox] * inside).reshape(n, c, 1))
            return dx
        return pool_backward(dy, index, (h, w), k, s, pad)[0]
    y, _ = pool_forward(x, k, s, pad)
    dx = torch.zeros(n, c, h, w, dtype=torch.float64)
    for oy in range(y.shape[2]):
        for ox in range(y.shape[3]):
            ys = slice(max(oy * s - pad, 0), min(oy * s - pad + k, h))
            xs = slice(max(ox * s - pad, 0), min(ox * s - pad + k, w))
            hit = (x[:, :, ys, xs] == y[:, :, oy, ox][:, :, None, None]).double()
            if rule == 'ties_split':
                hit = hit / hit.sum((2, 3), keepdim=True)
            dx[:, :, ys, xs] += hit * dy.double()[:, :, oy, ox][:, :, None, None]
    return dx


def pool_autograd64(x, dy, k, s, pad):
    """torch's own float64 CPU max_pool2d and its gradient -> (y, dx)."""
    x = x.double().clone().requires_grad_(True)
    y = F.max_pool2d(x, k, s, pad)
    y.backward(dy.double())
    return y.detach(), x.grad
