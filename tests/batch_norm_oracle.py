"""fp64 statements of what celldetection_amd.nn.batch_norm must compute (the "Trainable batch normalisation" section of
include/cpn_hip.h), the magnitude sums its bounds need, wrong rules the tests tell apart, and the judge the GPU tests apply (test
helper, not a conftest).  Everything here is torch on the CPU in float64.

Bounds (no allowance counts, no fraction of bad elements).  u32 = 2^-24, u64 = 2^-53, gamma_u(n) = n u / (1 - n u); `chain` is
what ``batch_norm_info`` reports.  With A1 = sum |x| / M and A2 = sum x^2 / M:

    mean     gamma64(chain) A1                                         + one fp32 rounding
    var      gamma64(chain) (A2 + mean^2)                                (not stored)
    invstd   1/2 invstd d(var) / (var + eps)                           + one fp32 rounding
    scale    |gamma| d(invstd)                                         + one fp32 rounding
    shift    |scale| d(mean) + |mean| |gamma| d(invstd)                + one fp32 rounding
    running  momentum d(mean), momentum d(var) M / (M - 1)             + one rounding to the buffer's dtype
    y        on the returned coefficients: t = x scale + shift in fp64, |fp32 y - t| <= u32 |t|, a bf16 y inside
             conv_bounds.bf16_bounds(t, u32 |t|), exactly 0 wherever t <= 0 under ReLU
    mask     the exact sign of x scale + shift with the returned fp32 coefficients (fp64 keeps the sign of that sum)
    dbeta    gamma64(chain) sum |g|                                    + one rounding to the parameter's dtype
    dgamma   gamma64(chain) invstd (sum |g x| + |mean| sum |g|)        + one rounding to the parameter's dtype
    dx       gamma32(3) S + 2^-40 S, S = |a g| + |b x| + |a sum g / M| + |b mean|, + the output rounding
"""
import torch

import conv_bounds as cb

U32, U64 = 2.0 ** -24, 2.0 ** -53
U_OF = {torch.float32: U32, torch.bfloat16: 2.0 ** -8, torch.float64: 0.}  # unit roundoffs: 24 and 8 significant bits

WRONG_RULES = ('unbiased_variance_normalises', 'biased_running_var', 'eps_outside_root', 'mask_includes_zero',
               'dx_without_mean_term', 'dx_without_projection_term', 'momentum_swapped', 'eval_uses_batch_statistics')


def gamma64(n):
    return n * U64 / (1 - n * U64)


def _pc(v):
    """[C] -> [1, C, 1, 1]"""
    return v.reshape(1, -1, 1, 1)


def _sum(t):
    return t.sum(dim=(0, 2, 3))


def forward(x, weight=None, bias=None, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, relu=False,
            rule=None):
    """-> dict(y, t, mean, var, invstd, scale, shift, running_mean, running_var (the updated buffers or None), A1, A2, M)."""
    x = x.double()
    c = x.shape[1]
    m = x.numel() // c
    g = torch.ones(c, dtype=torch.float64) if weight is None else weight.double()
    b = torch.zeros(c, dtype=torch.float64) if bias is None else bias.double()
    use_batch = training or running_mean is None or rule == 'eval_uses_batch_statistics'
    new_mean = None if running_mean is None else running_mean.double().clone()
    new_var = None if running_var is None else running_var.double().clone()
    a1, a2 = _sum(x.abs()) / m, _sum(x * x) / m
    if use_batch:
        mean = _sum(x) / m
        # (the two-pass form, for the statement's own accuracy; the kernel's one-pass form is what the bound is about)
        var = _sum((x - _pc(mean)) ** 2) / m
        if training and new_mean is not None:
            keep, take = (momentum, 1 - momentum) if rule == 'momentum_swapped' else (1 - momentum, momentum)
            new_mean = keep * new_mean + take * mean
            new_var = keep * new_var + take * var * (1. if rule == 'biased_running_var' else m / (m - 1))
        if rule == 'unbiased_variance_normalises':
            var = var * m / (m - 1)
    else:
        mean, var = running_mean.double(), running_var.double()
    invstd = 1 / (var.sqrt() + eps) if rule == 'eps_outside_root' else 1 / (var + eps).sqrt()
    scale = g * invstd
    shift = b - mean * scale
    t = x * _pc(scale) + _pc(shift)
    y = torch.where(t > 0, t, torch.zeros_like(t)) if relu else t
    return dict(y=y, t=t, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, running_mean=new_mean, running_var=new_var,
                A1=a1, A2=a2, M=m, gamma=g, beta=b)


def mask(t, rule=None):
    return t >= 0 if rule == 'mask_includes_zero' else t > 0


def backward(x, dy, weight, mean, invstd, m_or_none, training=True, rule=None):
    """g = dy (m_or_none None) or dy * mask -> dict(dgamma, dbeta, dx, S_dgamma, S_dbeta, S_dx, a, b, c)."""
    x, g = x.double(), dy.double()
    c = x.shape[1]
    m = x.numel() // c
    if m_or_none is not None:
        g = g * m_or_none.double()
    gam = torch.ones(c, dtype=torch.float64) if weight is None else weight.double()
    mean, invstd = mean.double(), invstd.double()
    sg, sgx = _sum(g), _sum(g * x)
    dbeta = sg
    dgamma = invstd * _sum(g * (x - _pc(mean)))
    s_dbeta = _sum(g.abs())
    s_dgamma = invstd * (_sum((g * x).abs()) + mean.abs() * s_dbeta)
    a = gam * invstd
    if training:
        b = torch.zeros_like(a) if rule == 'dx_without_projection_term' else -a * invstd * dgamma / m
        cc = (torch.zeros_like(a) if rule == 'dx_without_mean_term' else -a * sg / m) - b * mean
    else:
        b, cc = torch.zeros_like(a), torch.zeros_like(a)
    dx = _pc(a) * g + _pc(b) * x + _pc(cc)
    s_dx = (_pc(a) * g).abs() + (_pc(b) * x).abs() + _pc((a * sg / m).abs() if training else torch.zeros_like(a)) + \
        _pc((b * mean).abs()).expand_as(x)
    return dict(dgamma=dgamma, dbeta=dbeta, dx=dx, S_dgamma=s_dgamma, S_dbeta=s_dbeta, S_dx=s_dx, a=a, b=b, c=cc)


def autograd64(x, dy, weight, bias, running_mean, running_var, training, momentum, eps, relu):
    """torch's own float64 autograd of relu(F.batch_norm(...)) -> (y, dx, dgamma, dbeta, running_mean, running_var)."""
    x = x.double().clone().requires_grad_(True)
    w = None if weight is None else weight.double().clone().requires_grad_(True)
    b = None if bias is None else bias.double().clone().requires_grad_(True)
    rm = None if running_mean is None else running_mean.double().clone()
    rv = None if running_var is None else running_var.double().clone()
    y = torch.nn.functional.batch_norm(x, rm, rv, w, b, training, momentum, eps)
    if relu:
        y = torch.relu(y)
    y.backward(dy.double())
    return y.detach(), x.grad, None if w is None else w.grad, None if b is None else b.grad, rm, rv


# ---- the judge ------------------------------------------------------------------------------------------------------------------

def _within(name, got, ref, tol):
    got, ref, tol = got.double(), ref.double(), tol.double()
    err = (got - ref).abs()
    ok = torch.isfinite(got) & (err <= tol)
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.
    print(f'{name}: largest error / bound {worst:.3g}')
    assert bool(ok.all()), f'{name}: {int((~ok).sum())} / {ok.numel()} outside the bound, worst error / bound {worst:.3g}'
    return worst


def judge_stats(name, x, got, chain, weight=None, bias=None, running_mean=None, running_var=None, training=True, momentum=0.1,
                eps=1e-5, running_dtype=torch.float32):
    """got: dict(save_mean, save_invstd, scale, shift[, running_mean, running_var]) as the kernel returned them; running_mean /
    running_var: the buffers BEFORE the call."""
    o = forward(x, weight, bias, running_mean, running_var, training, momentum, eps)
    g64 = gamma64(chain)
    m = o['M']
    use_batch = training or running_mean is None
    d_mean = g64 * o['A1'] if use_batch else torch.zeros_like(o['mean'])
    d_var = g64 * (o['A2'] + o['mean'] ** 2) if use_batch else torch.zeros_like(o['mean'])
    d_inv = .5 * o['invstd'] * d_var / (o['var'] + eps)
    d_scale = o['gamma'].abs() * d_inv
    d_shift = o['scale'].abs() * d_mean + o['mean'].abs() * d_scale

    def rounded(ref, d, u=U32):
        return d + u * (ref.abs() + d)

    _within(f'{name} save_mean', got['save_mean'], o['mean'], rounded(o['mean'], d_mean))
    _within(f'{name} save_invstd', got['save_invstd'], o['invstd'], rounded(o['invstd'], d_inv))
    _within(f'{name} scale', got['scale'], o['scale'], rounded(o['scale'], d_scale))
    _within(f'{name} shift', got['shift'], o['shift'], rounded(o['shift'], d_shift))
    if training and running_mean is not None:
        u = U_OF[running_dtype]
        _within(f'{name} running_mean', got['running_mean'], o['running_mean'],
                rounded(o['running_mean'], momentum * d_mean, u))
        _within(f'{name} running_var', got['running_var'], o['running_var'],
                rounded(o['running_var'], momentum * d_var * m / (m - 1), u))
    return o


def exact_t(x, scale, shift):
    """x scale + shift with the fp32 coefficients the kernel returned, in fp64: the product is exact, the sum keeps its sign."""
    return x.double() * _pc(scale.double()) + _pc(shift.double())


def judge_y(name, x, y, scale, shift, relu):
    t = exact_t(x, scale, shift)
    tiny = (t != 0) & (t.abs() < 2.0 ** -126)
    assert not bool(tiny.any()), f'{name}: the inputs put {int(tiny.sum())} values of t into the fp32 subnormals'
    d = U32 * t.abs()
    yd = y.double()
    assert bool(torch.isfinite(yd).all()), name
    if relu:
        assert bool((yd[t <= 0] == 0).all()), f'{name}: a non-zero output where t <= 0'
    if y.dtype == torch.bfloat16:
        lo, hi = cb.bf16_bounds(t, d, 'relu' if relu else 'none')
    else:
        lo, hi = (t - d, t + d)
        if relu:
            lo, hi = lo.clamp_min(0.), hi.clamp_min(0.)
    return cb.check(f'{name} y', yd, lo, hi, t.clamp_min(0.) if relu else t)


def judge_grads(name, x, dy, got, chain, weight, save_mean, save_invstd, scale, shift, relu, training=True,
                param_dtype=torch.float32):
    """got: dict(dx | None, dgamma | None, dbeta | None) as the kernel returned them; the reference is built on the fp32 vectors the
    forward returned and on the exact mask."""
    mk = mask(exact_t(x, scale, shift)) if relu else None
    o = backward(x, dy, weight, save_mean, save_invstd, mk, training)
    g64 = gamma64(chain)
    u = U_OF[param_dtype]
    for key in ('dbeta', 'dgamma'):
        if got.get(key) is not None:
            d = g64 * o['S_' + key]
            _within(f'{name} {key}', got[key], o[key], d + u * (o[key].abs() + d))
    if got.get('dx') is not None:
        dx = got['dx']
        d = (cb.gamma(3) + 2.0 ** -40) * o['S_dx']
        if dx.dtype == torch.bfloat16:
            lo, hi = cb.bf16_bounds(o['dx'], d)
        else:
            lo, hi = o['dx'] - d, o['dx'] + d
        assert bool(torch.isfinite(dx.double()).all()), name
        cb.check(f'{name} dx', dx.double(), lo, hi, o['dx'], o['S_dx'])
    return o


# ---- the stated arithmetic on the CPU (fp64 sums, fp32 fma), for the judge's own tests -----------------------------------------

def _fma32(a, b, c):
    """fmaf on fp32 operands: the exact a b + c rounded once (the fp64 sum in between is off by at most 2^-53 of it)."""
    return (a.double() * b.double() + c.double()).float()


def _bc(v, like):
    return _pc(v).expand_as(like)


def emulate(x, dy, weight=None, bias=None, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, relu=False,
            sumsq_dtype=torch.float64, mask_from_fp64=False):
    """The kernels' arithmetic as include/cpn_hip.h states it, on x and dy of the kernels' dtype -> dict of everything they return.
    sumsq_dtype float32: the sum of squares accumulated in fp32 (a wrong implementation the judge must reject); mask_from_fp64: the
    backward's mask taken from the unrounded fp64 coefficients (another)."""
    dt = x.dtype
    xd = x.double()
    c = x.shape[1]
    m = x.numel() // c
    g = torch.ones(c, dtype=torch.float64) if weight is None else weight.double()
    b = torch.zeros(c, dtype=torch.float64) if bias is None else bias.double()
    out = {}
    if training or running_mean is None:
        mean = _sum(xd) / m
        sxx = _sum(xd * xd) if sumsq_dtype == torch.float64 else \
            (x.float() * x.float()).permute(1, 0, 2, 3).reshape(c, -1).cumsum(1, dtype=torch.float32)[:, -1].double()
        var = (sxx / m - mean * mean).clamp_min(0.)
        if training and running_mean is not None:
            out['running_mean'] = ((1 - momentum) * running_mean.double() + momentum * mean).to(running_mean.dtype)
            out['running_var'] = ((1 - momentum) * running_var.double() + momentum * var * m / (m - 1)).to(running_var.dtype)
    else:
        mean, var = running_mean.double(), running_var.double()
    invstd = 1 / (var + eps).sqrt()
    scale64 = g * invstd
    shift64 = b - mean * scale64
    out.update(save_mean=mean.float(), save_invstd=invstd.float(), scale=scale64.float(), shift=shift64.float())
    t = _fma32(x.float(), _bc(out['scale'], x), _bc(out['shift'], x))
    out['y'] = (torch.where(t > 0, t, torch.zeros_like(t)) if relu else t).to(dt)
    gd = dy.float()
    if relu:
        keep = (xd * _pc(scale64) + _pc(shift64)) > 0 if mask_from_fp64 else t > 0
        gd = torch.where(keep, gd, torch.zeros_like(gd))
    gd64 = gd.double()
    sg, sgx = _sum(gd64), _sum(gd64 * xd)
    mean32, inv32 = out['save_mean'].double(), out['save_invstd'].double()
    dgamma = inv32 * (sgx - mean32 * sg)
    out['dbeta'], out['dgamma'] = sg.float(), dgamma.float()
    if training or running_mean is None:
        a = g * inv32
        bb = -a * inv32 * dgamma / m
        cc = -a * sg / m - bb * mean32
        inner = _fma32(_bc(bb.float(), x), x.float(), _bc(cc.float(), x))
        out['dx'] = _fma32(_bc(a.float(), x), gd, inner).to(dt)
    else:
        out['dx'] = _fma32(_bc(out['scale'], x), gd, torch.zeros_like(gd)).to(dt)
    return out
