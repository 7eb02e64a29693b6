"""fp64 statements of the trainable ReadOut tail (test helper, not a conftest): Dropout2d fused into a 1x1 conv, as the "Trainable
ReadOut tail" section of include/cpn_hip.h states it, for a GIVEN keep mask.

    x [N, Cin, H, W], w [Cout, Cin], b [Cout] | None, m [N, Cin] in {0, 1}, s = 1 / (1 - p), g = grad_output [N, Cout, H, W]

    y  = s * sum_c m[n][c] w[o][c] x[n][c][q] + b[o]
    dx = m[n][c] * s * sum_o w[o][c] g[n][o][q]
    dW = s * sum_n m[n][c] sum_q g[n][o][q] x[n][c][q]
    db = sum_{n, q} g[n][o][q]

Every function returns the value and S, the sum of the absolute products behind each element BEFORE the factor s (the GPU tests
scale it: gamma(chain) * s * S).  ``WRONG_RULES`` names rules a kernel could follow instead; ``statements(..., rule=name)`` follows
one of them, and tests/test_readout_tail.py shows that the cases tell each of them from the right one.
"""
import torch

WRONG_RULES = ('mask_per_pixel', 'mask_of_the_wrong_image', 'dx_without_s', 's_applied_twice', 'dw_not_masked', 'db_masked',
               'slab_crossing_an_image_takes_the_first_mask', 'last_slab_dropped', 'dx_not_masked', 'bias_scaled')


def _flat(t):
    return t.double().reshape(t.shape[0], t.shape[1], -1)


def forward(x, w, b, m, s):
    """-> (y [N, Cout, H, W], S)"""
    x3, w, m = _flat(x), w.double().reshape(w.shape[0], -1), m.double()
    y = torch.einsum('oc,nc,ncq->noq', w, m, x3) * s
    S = torch.einsum('oc,nc,ncq->noq', w.abs(), m, x3.abs())
    if b is not None:
        y = y + b.double().reshape(1, -1, 1)
    shape = (x.shape[0], w.shape[0]) + tuple(x.shape[2:])
    return y.reshape(shape), S.reshape(shape)


def input_grad(g, w, m, s):
    """-> (dx [N, Cin, H, W], S)"""
    g3, w, m = _flat(g), w.double().reshape(w.shape[0], -1), m.double()
    dx = torch.einsum('oc,noq->ncq', w, g3) * m[:, :, None] * s
    S = torch.einsum('oc,noq->ncq', w.abs(), g3.abs()) * m[:, :, None]
    shape = (g.shape[0], w.shape[1]) + tuple(g.shape[2:])
    return dx.reshape(shape), S.reshape(shape)


def weight_grad(x, g, m, s):
    """-> (dW [Cout, Cin], S)"""
    x3, g3, m = _flat(x), _flat(g), m.double()
    dw = torch.einsum('nc,noq,ncq->oc', m, g3, x3) * s
    S = torch.einsum('nc,noq,ncq->oc', m, g3.abs(), x3.abs())
    return dw, S


def bias_grad(g):
    """-> (db [Cout], S)"""
    g3 = _flat(g)
    return g3.sum((0, 2)), g3.abs().sum((0, 2))


def statements(x, g, w, b, m, s, rule=None, slab_pixels=None):
    """All four statements -> dict(y, dx, dw, db), by the right rule (None) or one of WRONG_RULES.  slab_pixels: the slabs of the
    two rules that speak of them (pixels per slab)."""
    assert rule is None or rule in WRONG_RULES, rule
    n, cin, hw = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    m = m.double()
    x3, g3, w2 = _flat(x), _flat(g), w.double().reshape(w.shape[0], -1)
    out = dict(y=forward(x, w, b, m, s)[0], dx=input_grad(g, w, m, s)[0], dw=weight_grad(x, g, m, s)[0], db=bias_grad(g)[0])
    if rule == 'mask_per_pixel':  # a mask of the same density that varies from pixel to pixel
        idx = (torch.arange(cin)[:, None] + torch.arange(hw)[None, :]) % cin
        mp = m[:, idx]  # [N, Cin, HW]
        out['y'] = (torch.einsum('oc,ncq->noq', w2, x3 * mp) * s + (0 if b is None else b.double().reshape(1, -1, 1))).reshape(out['y'].shape)
        out['dx'] = (torch.einsum('oc,noq->ncq', w2, g3) * mp * s).reshape(out['dx'].shape)
        out['dw'] = torch.einsum('noq,ncq->oc', g3, x3 * mp) * s
    elif rule == 'mask_of_the_wrong_image':
        wrong = torch.roll(m, 1, 0)
        out.update(y=forward(x, w, b, wrong, s)[0], dx=input_grad(g, w, wrong, s)[0], dw=weight_grad(x, g, wrong, s)[0])
    elif rule == 'dx_without_s':
        out['dx'] = input_grad(g, w, m, 1.)[0]
    elif rule == 's_applied_twice':
        out.update(y=forward(x, w, b, m, s * s)[0], dx=input_grad(g, w, m, s * s)[0], dw=weight_grad(x, g, m, s * s)[0])
    elif rule == 'dw_not_masked':
        out['dw'] = weight_grad(x, g, torch.ones_like(m), s)[0]
    elif rule == 'dx_not_masked':
        out['dx'] = input_grad(g, w, torch.ones_like(m), s)[0]
    elif rule == 'db_masked':  # the bias gradient of output channel o masked like input channel o
        out['db'] = (g3.sum(2) * m[:, :g3.shape[1]]).sum(0)
    elif rule == 'bias_scaled':
        out['y'] = forward(x, w, None, m, s)[0] + (0 if b is None else s * b.double().reshape(1, -1, 1, 1))
    elif rule in ('slab_crossing_an_image_takes_the_first_mask', 'last_slab_dropped'):
        assert slab_pixels
        xf = x3.permute(1, 0, 2).reshape(cin, n * hw)  # the flat pixel range of the batch
        gf = g3.permute(1, 0, 2).reshape(g3.shape[1], n * hw)
        dw = torch.zeros_like(out['dw'])
        db = torch.zeros_like(out['db'])
        if rule == 'last_slab_dropped':  # slabs per image, the last (partial or not) never added
            for i in range(n):
                starts = list(range(0, hw, slab_pixels))[:-1]
                for q0 in starts:
                    sl = slice(i * hw + q0, i * hw + min(q0 + slab_pixels, hw))
                    dw += torch.einsum('oq,cq->oc', gf[:, sl], xf[:, sl]) * m[i][None, :]
                    db += gf[:, sl].sum(1)
        else:  # slabs over the flat range, each with the mask of the image of its first pixel
            for p0 in range(0, n * hw, slab_pixels):
                sl = slice(p0, min(p0 + slab_pixels, n * hw))
                dw += torch.einsum('oq,cq->oc', gf[:, sl], xf[:, sl]) * m[p0 // hw][None, :]
            db = out['db']
        out.update(dw=dw * s, db=db)
    return out


def autograd64(x, g, w, b, m, s):
    """torch's own float64 autograd of F.conv2d(x * m[:, :, None, None] * s, w, b) -> (y, dx, dw [Cout, Cin], db | None)"""
    x = x.double().clone().requires_grad_(True)
    w4 = w.double().reshape(w.shape[0], -1, 1, 1).clone().requires_grad_(True)
    bb = None if b is None else b.double().clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x * m.double()[:, :, None, None] * s, w4, bb)
    y.backward(g.double())
    return y.detach(), x.grad, w4.grad.reshape(w.shape[0], -1), None if b is None else bb.grad
