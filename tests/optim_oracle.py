"""The "Optimizer step" rule of include/cpn_hip.h restated in numpy, twice, with the bounds between the two (a helper of
tests/test_optim.py and tests/test_gpu_optim.py, not a test).

``step_f32`` does every operation in ``np.float32`` in the stated order, with the scalars rounded once from fp64: what the kernel
must give bit for bit.  ``step_f64`` does the same in fp64 with unrounded scalars: the real-number result up to 2^-53.
``norm_f64`` is the exactly rounded sum (``math.fsum``) of the fp64 squares, then the square root.

Bounds on |step_f32 - step_f64| after one step from common p, g, m, v (u = 2^-24, every fp32 operation and every rounded scalar
is off by a factor (1 + d), |d| <= u; first order in u, constants rounded up to cover the second).  Primes are the new values.

g' = g c (with a clip coefficient c; else g' = g exactly and e_g = 0).  The product rounds once, and where the two sides computed
c from different norms (fp32 here, fp64 in torch) c itself differs by 2 u: e_g = 3 u |g'|.

m' = m + w1 (g' - m).  The difference rounds (u |g' - m|) and carries e_g; w1 is rounded (u) and the product rounds (u); the sum
rounds (u |m'|).  Because the difference cancels, the error is not relative to m' but to the operands:
    e_m = u (|m'| + 4 w1 |g' - m|) + 1.01 w1 e_g.

v' = v b2 + (g' g') w2.  All terms are >= 0: b2 rounded, v b2 rounded, g' g' rounded, w2 rounded, that product rounded, the sum rounded,
at most three roundings on either term and one on the sum, plus 2 w2 |g'| e_g from g':
    e_v = 4 u v' + 3 w2 |g'| e_g.
Relative to v' >= w2 g'^2 this is at most 4 u + 3 e_g / |g'| = 13 u.

p' = p decay - s (m' / denom), denom = sqrt(v') / b + eps.  sqrt halves the relative error of v' and rounds: 7.5 u; b rounded and the
division rounds: 9.5 u on the quotient; eps rounded and the sum rounds: at most 10.5 u on denom.  m' / denom: e_m / denom plus
11.5 u relative; s rounded and the product rounds: with t = s m' / denom the term is off by 13.5 u |t| + s e_m / denom.  decay
rounded and p decay rounds: 2 u |p decay|.  The difference rounds: u |p'|.
    e_p = 1.01 (u |p'| + 2 u |p decay| + 16 u |t| + s e_m / denom).
A bf16 parameter adds the one rounding of the new value to bf16, whose 8-bit significand has the unit roundoff 2^-8: 2^-8 |p'|
(``bf16=True``).  The bounds need fp32 normal operands
(no subnormal g g or v); the tests stay there.

The norm.  Squares of fp32 or bf16 values are exact in fp64.  A sum of N non-negative fp64 terms in ANY order is off by at most
(N - 1) 2^-53 relative (every partial sum is at most the total); the kernel's chain per element is far shorter (opt_sum_chain),
but N additions bound every order.  The square root halves that and rounds (2^-53), the result is rounded to fp32 (2^-24):
    |norm - norm_f64| <= (2^-24 + (N + 2) 2^-53) norm_f64.
"""
import math

import numpy as np

U = 2. ** -24
F = np.float32


def scalars(lr, betas, eps, weight_decay, step):
    """fp64: (decay, w1, beta2, w2, eps, step_size, bc2_sqrt) of include/cpn_hip.h."""
    b1, b2 = betas
    return (1. - lr * weight_decay, 1. - b1, b2, 1. - b2, eps, lr / (1. - b1 ** step), math.sqrt(1. - b2 ** step))


def step_f32(p, g, m, v, lr, betas, eps, weight_decay, step, coef=None):
    """One step on float32 arrays, every operation in float32 -> (p, m, v).  ``coef``: the float32 clip coefficient."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    decay, w1, b2, w2, eps, s, b = (F(x) for x in scalars(lr, betas, eps, weight_decay, step))
    if coef is not None:
        g = g * F(coef)
    p = p * decay
    m = m + (g - m) * w1
    v = v * b2 + (g * g) * w2
    denom = np.sqrt(v) / b + eps
    p = p - s * (m / denom)
    assert p.dtype == F and m.dtype == F and v.dtype == F
    return p, m, v


def step_f64(p, g, m, v, lr, betas, eps, weight_decay, step, coef=None):
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    decay, w1, b2, w2, eps, s, b = scalars(lr, betas, eps, weight_decay, step)
    if coef is not None:
        g = g * float(coef)
    p = p * decay
    m = m + (g - m) * w1
    v = v * b2 + (g * g) * w2
    denom = np.sqrt(v) / b + eps
    return p - s * (m / denom), m, v


def bounds(p, g, m, v, lr, betas, eps, weight_decay, step, coef=None, bf16=False):
    """-> (e_p, e_m, e_v) of the docstring, computed in fp64 from the common state."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    decay, w1, b2, w2, eps, s, b = scalars(lr, betas, eps, weight_decay, step)
    g1 = g if coef is None else g * float(coef)
    e_g = 0. * g1 if coef is None else 3 * U * np.abs(g1)
    p1, m1, v1 = step_f64(p, g, m, v, lr, betas, eps, weight_decay, step, coef)
    e_m = U * (np.abs(m1) + 4 * w1 * np.abs(g1 - m)) + 1.01 * w1 * e_g
    e_v = 4 * U * v1 + 3 * w2 * np.abs(g1) * e_g
    denom = np.sqrt(v1) / b + eps
    t = s * m1 / denom
    e_p = 1.01 * (U * np.abs(p1) + 2 * U * np.abs(p * decay) + 16 * U * np.abs(t) + s * e_m / denom)
    if bf16:
        e_p = e_p + 2. ** -8 * np.abs(p1)
    return e_p, e_m, e_v


def norm_f64(arrays):
    return math.sqrt(math.fsum(float(x) * float(x) for a in arrays for x in np.asarray(a, dtype=np.float64).ravel()))


def norm_bound(arrays):
    """Relative bound on |norm - norm_f64| of the docstring."""
    n = sum(np.asarray(a).size for a in arrays)
    return 2. ** -24 + (n + 2) * 2. ** -53


def clip_coef(norm, max_norm):
    """The float32 coefficient of the header from the float32 norm: fp64, rounded once."""
    return F(min(1., float(max_norm) / (float(F(norm)) + 1e-6)))


def bf16_rne(x):
    """float32 array -> the nearest bf16 values (ties to even) as float32: the kernel's one rounding of a new bf16 parameter."""
    u = np.asarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F)


def bf16_from_f64(x):
    """fp64 array -> the nearest bf16 values (ties to even) as float32, ONE rounding (through float32 there would be two)."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    e = np.maximum(e, -125)  # below 2^-126 the spacing is that of the subnormals
    return np.ldexp(np.rint(np.ldexp(x, 8 - e)), e - 8).astype(F)


# ---- the checks of one step on the GPU's tensors (shared by tests/test_gpu_optim.py and tests/test_gpu_train_step.py)

def np_of(t):
    """torch tensor -> float32 array on the host (bf16 widens exactly)."""
    return t.detach().float().cpu().numpy()


def same(t, a):
    """Whether the tensor holds exactly the float32 bits of ``a``."""
    return np.array_equal(np_of(t).view(np.uint32), np.asarray(a, dtype=np.float32).view(np.uint32))


def expect(h, bf16, step, hyper, coef=None):
    """h: dict(p, g, m, v) of float32 arrays before the step -> (p, m, v) after it by the float32 rule; a bf16 parameter rounds once."""
    p, m, v = step_f32(h['p'], h['g'], h['m'], h['v'], step=step, coef=coef, **hyper)
    return (bf16_rne(p) if bf16 else p), m, v


def assert_step(opt, params, host, bf16s, step, hyper, coef=None):
    """Every parameter and both moments after ``opt.step()`` are the float32 rule bit for bit, the moments float32, the step count a
    float32 CPU scalar, the gradient untouched.  host: per parameter dict(p, g, m, v) before the step; bf16s: per parameter, whether
    it is bfloat16."""
    for i, (p, h, bf16) in enumerate(zip(params, host, bf16s)):
        want = expect(h, bf16, step, hyper, coef)
        state = opt.state[p]
        assert str(state['exp_avg'].dtype) == str(state['exp_avg_sq'].dtype) == 'torch.float32' and float(state['step']) == step
        assert state['step'].device.type == 'cpu' and str(state['step'].dtype) == 'torch.float32'
        for name, got, w in zip('pmv', (p, state['exp_avg'], state['exp_avg_sq']), want):
            assert same(got, w), (i, p.numel(), bf16, name, float(np.abs(np_of(got) - w).max()))
        assert same(p.grad, h['g']), i  # the gradient is read, never written
