"""fp64 statements of what the pieces of ``celldetection_amd.nn.Bottleneck`` must compute (the "Trainable bottleneck block" section of
include/cpn_hip.h), wrong rules the tests tell apart, and the judges the GPU tests apply (test helper, not a conftest).  Everything
here is torch on the CPU in float64.

A. The norm's residual tail.  t = x scale + shift, s = t + r, y = s or its positive part; backward: g = dy [s > 0] (no ReLU: dy),
   dr = g, and dgamma, dbeta, dx are the batch norm's own on g (tests/batch_norm_oracle.py).
B. The strided 1x1 conv: y[i][j] = w x[2 i][2 j] + b; dx = dilate(dgrad(dy)); dW = dW_dense(sub(x), dy); db = sum dy.
C. The fork: dx = dgrad(dy) + dskip.

Bounds of the tail (no allowance counts, no fraction of bad elements), on the coefficients the kernel returned: with p = x scale + shift
and t = p + r in fp64 the kernel's two fp32 roundings (the fma, the add) leave it within d = 2^-24 (|p| + |t|) (1 + 2^-23) of t; an fp32
y lies in [t - d, t + d] (pushed through the ReLU), a bf16 y inside conv_bounds.bf16_bounds(t, d), and y is exactly 0 wherever
t <= -d.  g = dr is dy [y > 0] bit for bit with y AS RETURNED; dgamma, dbeta and dx are judged by the batch norm's bounds with that
mask.
"""
import torch
import torch.nn.functional as F

import batch_norm_oracle as bo
import conv_bounds as cb

U32 = 2.0 ** -24

TAIL_WRONG_RULES = ('mask_without_residual', 'mask_includes_zero', 'dr_unmasked', 'dr_times_a', 'residual_after_relu',
                    'sum_g_unmasked')
CONV_WRONG_RULES = ('subsample_odd_grid', 'dilate_odd_grid', 'skip_dropped', 'skip_twice')


def _pc(v):
    return v.reshape(1, -1, 1, 1)


def _sum(t):
    return t.sum(dim=(0, 2, 3))


# ---- A. the residual tail

def tail(x, r, dy, weight=None, bias=None, running_mean=None, running_var=None, training=True, eps=1e-5, relu=True, rule=None):
    """-> dict(y, t (before the add), s (after it), mask, g, dr, dgamma, dbeta, dx, mean, invstd)."""
    f = bo.forward(x, weight, bias, running_mean, running_var, training, 0.1, eps, False)
    x, r, dy = x.double(), r.double(), dy.double()
    t = f['t']
    s = t + r
    zero = torch.zeros_like(s)
    if rule == 'residual_after_relu':
        y = torch.where(t > 0, t, zero) + r if relu else s
    else:
        y = torch.where(s > 0, s, zero) if relu else s
    if not relu:
        mask = torch.ones_like(s, dtype=torch.bool)
    elif rule in ('mask_without_residual', 'residual_after_relu'):
        mask = t > 0
    elif rule == 'mask_includes_zero':
        mask = s >= 0
    else:
        mask = s > 0
    g = dy * mask.double()
    use_batch = training or running_mean is None
    c = x.shape[1]
    m = x.numel() // c
    mean, invstd = f['mean'], f['invstd']
    gam = f['gamma']
    sg = _sum(dy) if rule == 'sum_g_unmasked' else _sum(g)
    sgx = _sum(g * x)
    dgamma = invstd * (sgx - mean * sg)
    a = gam * invstd
    if use_batch:
        b = -a * invstd * dgamma / m
        cc = -a * sg / m - b * mean
    else:
        b, cc = torch.zeros_like(a), torch.zeros_like(a)
    dx = _pc(a) * g + _pc(b) * x + _pc(cc)
    dr = dy if rule == 'dr_unmasked' else (_pc(a) * g if rule == 'dr_times_a' else g)
    return dict(y=y, t=t, s=s, mask=mask, g=g, dr=dr, dgamma=dgamma, dbeta=sg, dx=dx, mean=mean, invstd=invstd)


def tail_autograd64(x, r, dy, weight, bias, running_mean, running_var, training, eps, relu):
    """torch's own float64 autograd of relu(F.batch_norm(x, ...) + r) -> (y, dx, dr, dgamma, dbeta)."""
    x = x.double().clone().requires_grad_(True)
    r = r.double().clone().requires_grad_(True)
    w = None if weight is None else weight.double().clone().requires_grad_(True)
    b = None if bias is None else bias.double().clone().requires_grad_(True)
    rm = None if running_mean is None else running_mean.double().clone()
    rv = None if running_var is None else running_var.double().clone()
    y = F.batch_norm(x, rm, rv, w, b, training or rm is None, 0.1, eps) + r
    if relu:
        y = torch.relu(y)
    y.backward(dy.double())
    return y.detach(), x.grad, r.grad, None if w is None else w.grad, None if b is None else b.grad


def tail_noise(x, r, scale, shift):
    """-> (t = x scale + shift + r in fp64 with the fp32 coefficients the kernel returned, d)."""
    p = bo.exact_t(x, scale, shift)
    t = p + r.double()
    return t, U32 * (p.abs() + t.abs()) * (1 + 2.0 ** -23)


def judge_tail_y(name, x, r, y, scale, shift, relu):
    t, d = tail_noise(x, r, scale, shift)
    yd = y.double()
    assert bool(torch.isfinite(yd).all()), name
    if relu:
        assert bool((yd[t <= -d] == 0).all()), f'{name}: a non-zero output where t <= -d'
    if y.dtype == torch.bfloat16:
        lo, hi = cb.bf16_bounds(t, d, 'relu' if relu else 'none')
    else:
        lo, hi = t - d, t + d
        if relu:
            lo, hi = lo.clamp_min(0.), hi.clamp_min(0.)
    return cb.check(f'{name} y', yd, lo, hi, t.clamp_min(0.) if relu else t)


def same_bits(a, b):
    ity = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]  # (a view of the same width: any strides)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().cpu().view(ity), b.detach().cpu().view(ity))


def masked(dy, y, relu=True):
    """g = dy where y > 0 and (plus) 0 elsewhere, as torch's own ReLU backward writes it."""
    return torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy


def judge_tail_grads(name, x, dy, y, got, chain, weight, save_mean, save_invstd, relu, training=True, param_dtype=torch.float32):
    """got: dict(dr | None, dx | None, dgamma | None, dbeta | None) as returned; y: the forward's output as returned (its sign is
    the mask).  dr bit for bit; the rest by the batch norm's bounds on g."""
    g = masked(dy, y, relu)
    if got.get('dr') is not None:
        assert same_bits(got['dr'], g), f'{name}: dr is not dy [y > 0] bit for bit ({int((got["dr"] != g).sum())} elements differ)'
    o = bo.backward(x, g, weight, save_mean, save_invstd, None, training)
    g64 = bo.gamma64(chain)
    u = bo.U_OF[param_dtype]
    for key in ('dbeta', 'dgamma'):
        if got.get(key) is not None:
            d = g64 * o['S_' + key]
            bo._within(f'{name} {key}', got[key], o[key], d + u * (o[key].abs() + d))
    if got.get('dx') is not None:
        dx = got['dx']
        d = (cb.gamma(3) + 2.0 ** -40) * o['S_dx']
        lo, hi = cb.bf16_bounds(o['dx'], d) if dx.dtype == torch.bfloat16 else (o['dx'] - d, o['dx'] + d)
        assert bool(torch.isfinite(dx.double()).all()), name
        cb.check(f'{name} dx', dx.double(), lo, hi, o['dx'], o['S_dx'])
    return o


def emulate_tail(x, r, scale, shift, relu, round_t=False):
    """The tail's stated arithmetic on the CPU: one fp32 fma, one fp32 add, one rounding to x's dtype.  round_t: t rounded to bf16
    before the add (a wrong implementation the judge must reject)."""
    t = bo._fma32(x.float(), bo._bc(scale, x), bo._bc(shift, x))
    if round_t:
        t = t.to(torch.bfloat16).float()
    s = t + r.float()  # (IEEE fp32 add: correctly rounded)
    return (torch.where(s > 0, s, torch.zeros_like(s)) if relu else s).to(x.dtype)


# ---- B. the strided 1x1 conv

def out_size(n, stride=2):
    return (n - 1) // stride + 1


def sub(x, rule=None):
    """x[..., 2 i, 2 j]"""
    return x[..., 1::2, 1::2] if rule == 'subsample_odd_grid' else x[..., ::2, ::2]


def dilate(dy, size, rule=None):
    out = torch.zeros(dy.shape[:2] + tuple(size), dtype=dy.dtype)
    if rule == 'dilate_odd_grid':
        out[..., 1::2, 1::2] = dy
    else:
        out[..., ::2, ::2] = dy
    return out


def dgrad1x1(dy, w):
    """dy [N, Cout, h, w], w [Cout, Cin, 1, 1] -> [N, Cin, h, w]"""
    return torch.einsum('noij,oc->ncij', dy.double(), w.double().reshape(w.shape[0], w.shape[1]))


def strided(x, w, b, dy, rule=None):
    """-> dict(y, dx, dw, db) of F.conv2d(x, w, b, stride=2) for a 1x1 w."""
    x, w, dy = x.double(), w.double(), dy.double()
    w2 = w.reshape(w.shape[0], w.shape[1])
    xs = sub(x, rule)
    y = torch.einsum('ncij,oc->noij', xs, w2)
    if b is not None:
        y = y + _pc(b.double())
    dx = dilate(dgrad1x1(dy, w), x.shape[2:], rule)
    dw = torch.einsum('noij,ncij->oc', dy, xs).reshape(w.shape)
    return dict(y=y, dx=dx, dw=dw, db=_sum(dy))


def strided_autograd64(x, w, b, dy):
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(x, w, b, stride=2)
    y.backward(dy.double())
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=None if b is None else b.grad)


# ---- C. the fork

def fork_dx(dy, w, dskip, rule=None):
    """dx of (conv(x, w), x) for gradients (dy, dskip); w [Cout, Cin, k, k], stride 1, padding k // 2."""
    k = w.shape[2]
    dx = F.conv_transpose2d(dy.double(), w.double(), None, 1, k // 2)
    if rule == 'skip_dropped' or dskip is None:
        return dx
    return dx + (2 if rule == 'skip_twice' else 1) * dskip.double()


def fork_autograd64(x, w, dy, dskip):
    x = x.double().clone().requires_grad_(True)
    k = w.shape[2]
    y = F.conv2d(x, w.double(), None, 1, k // 2)
    loss = (y * dy.double()).sum()
    if dskip is not None:
        loss = loss + (x * dskip.double()).sum()
    loss.backward()
    return x.grad
