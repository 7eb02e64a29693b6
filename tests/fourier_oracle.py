"""TEST INFRASTRUCTURE ONLY: the rule of ``celldetection_amd.fourier`` (elliptic Fourier descriptors of contours) stated twice.

``efd`` / ``contours2fourier``: the rule in numpy, operation by operation in the order in which the reference's ``cd.data.cpn.efd``
(celldetection/data/cpn.py:23-90) applies numpy to its arrays, so that it reproduces ``tests/golden/fourier.npz`` bit for bit.
``truth``: the same formula in ``mpmath`` at 40 digits on the float64 inputs; every result is judged against it in the unit
``U = 2^-53 N T`` of its contour.  ``MUTANTS``: wrong rules that the bound has to reject.  The generators of the GPU tests live here
too, because the bound's constants are measured over them (``tests/test_fourier.py``).

The rule.  A contour is ``n >= 1`` points.  It is closed if ``|first - last| <= 1e-8 + 1e-5 |last|`` for both coordinates; if it is
not, the first point is appended (a dense array decides once for all its contours, a list per contour).  With ``N`` segments:
``dt_i = sqrt(dx_i^2 + dy_i^2) + epsilon``, ``t_0 = 0``, ``t_(i+1) = t_i + dt_i``, ``T = t_N``; ``phi_(k,i) = k (2 pi t_i / T)``, ``C_k = T / (2 k^2
pi^2)``; ``coeff[k-1] = C_k (sum dx/dt dcos, sum dx/dt dsin, sum dy/dt dcos, sum dy/dt dsin)``; ``location = first + (1/T) sum [d/(2 dt)
(t_(i+1)^2 - t_i^2) + (D_i - d/dt t_(i+1)) dt]`` with ``D_i`` the running sum of ``d``, for ``d = dx`` and ``d = dy``.
"""
import numpy as np

CHUNK = 256  # CPN_EFD_CHUNK of include/cpn_hip.h (tests/test_fourier.py checks that they agree)
MAX_ORDER = 64
MUTANTS = ('float32', 'no_epsilon', 'no_closing_segment', 'T_short', 'inv_k', 'swap_cos_sin', 'no_first_point', 'X_previous')


def is_closed(contour):
    """numpy's ``allclose(first, last)`` over everything the array holds."""
    contour = np.asarray(contour)
    return bool(np.allclose(contour[..., 0, :], contour[..., -1, :]))


def close(contour, autoclose=True):
    contour = np.asarray(contour)
    if not is_closed(contour):
        if not autoclose:
            raise AssertionError('not closed')
        contour = np.concatenate((contour, contour[..., :1, :]), axis=-2)
    return contour


def efd(contour, order=10, epsilon=1e-6, autoclose=True, mutant=None):
    """An array [..., n, 2] -> (coefficients [..., order, 4], locations [..., 2]); a list of arrays [n_k, 2] -> the stacked
    results of every member taken alone (always closing, as the reference's object-array branch does)."""
    if isinstance(contour, (list, tuple)):
        res = [efd(c, order, epsilon, True, mutant) for c in contour]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res])
    pts = close(contour, autoclose)
    if mutant == 'float32':
        pts, epsilon = pts.astype(np.float32), np.float32(epsilon)
    if mutant == 'no_closing_segment':
        pts = pts[..., :-1, :]
    if mutant == 'no_epsilon':
        epsilon = 0.
    d = np.diff(pts, axis=-2)
    dt = np.sqrt(np.sum(np.square(d), axis=-1)) + epsilon
    run = np.cumsum(dt, axis=-1)
    t = np.concatenate([np.zeros(run.shape[:-1] + (1,)), run], axis=-1)
    if mutant == 'float32':
        t = t.astype(np.float32)
    total = t[..., -2:-1] if mutant == 'T_short' else t[..., -1:]
    phi = (2 * np.pi * t) / total
    ks = np.arange(1, order + 1, dtype=phi.dtype)
    consts = total / (2. * (ks if mutant == 'inv_k' else np.square(ks)) * np.square(np.pi))
    phi = np.expand_dims(phi, -2) * np.expand_dims(ks, -1)
    dcos = np.cos(phi[..., 1:]) - np.cos(phi[..., :-1])
    dsin = np.sin(phi[..., 1:]) - np.sin(phi[..., :-1])
    if mutant == 'swap_cos_sin':
        dcos, dsin = dsin, dcos
    rx = np.expand_dims(d[..., 0] / dt, axis=-2)
    ry = np.expand_dims(d[..., 1] / dt, axis=-2)
    coeff = np.stack([consts * np.sum(rx * dcos, axis=-1), consts * np.sum(rx * dsin, axis=-1),
                      consts * np.sum(ry * dcos, axis=-1), consts * np.sum(ry * dsin, axis=-1)], axis=-1)
    loc = []
    for a in (0, 1):
        D = np.cumsum(d[..., a], axis=-1)
        if mutant == 'X_previous':
            D = D - d[..., a]
        rest = D - (d[..., a] / dt) * t[..., 1:]
        t2 = np.diff(t ** 2, axis=-1)
        mean = (1 / total[..., 0]) * np.sum(((d[..., a] / (2 * dt)) * t2) + rest * dt, axis=-1)
        loc.append(mean if mutant == 'no_first_point' else pts[..., 0, a] + mean)
    return np.array(coeff), np.stack(loc, axis=-1)


def contours2fourier(contours, order=5, dtype=np.float32, mutant=None):
    """dict label -> array [n, 1, 2] or [n, 2] -> (fouriers [max label, order, 4], locations [max label, 2])."""
    top = max(contours.keys()) if len(contours) else 0
    fouriers, locations = np.zeros((top, order, 4), dtype=dtype), np.zeros((top, 2), dtype=dtype)
    for key, c in contours.items():
        c = np.asarray(c)
        fouriers[key - 1], locations[key - 1] = efd(c[:, 0] if c.ndim == 3 else c, order, mutant=mutant)
    return fouriers, locations


def truth(contour, order, epsilon, append=None):
    """One contour [n, 2] (float64 values are taken exactly) -> (coefficients [order, 4], locations [2], U) with the formula
    evaluated in mpmath at 40 digits and rounded once to float64; ``U = 2^-53 N T``.  ``append``: whether the first point is
    appended (None: when the contour is not closed)."""
    import mpmath
    mp = mpmath.mp
    contour = np.asarray(contour, dtype=np.float64)
    if append is None:
        append = not is_closed(contour)
    pts = [(mp.mpf(float(x)), mp.mpf(float(y))) for x, y in contour.tolist()]
    if append:
        pts.append(pts[0])
    N = len(pts) - 1
    with mp.workdps(40):
        eps = mp.mpf(float(epsilon))
        dx = [pts[i + 1][0] - pts[i][0] for i in range(N)]
        dy = [pts[i + 1][1] - pts[i][1] for i in range(N)]
        dt = [mp.sqrt(dx[i] * dx[i] + dy[i] * dy[i]) + eps for i in range(N)]
        t = [mp.mpf(0)]
        for v in dt:
            t.append(t[-1] + v)
        T = t[-1]
        coeff = np.zeros((order, 4))
        if N == 0:
            return coeff, np.full((2,), np.nan), 0.
        unit = [mp.expjpi(2 * ti / T) for ti in t]  # e^(i phi_(1,i)); its k-th power is e^(i phi_(k,i))
        power = [mp.mpc(1)] * (N + 1)
        rx, ry = [dx[i] / dt[i] for i in range(N)], [dy[i] / dt[i] for i in range(N)]
        for k in range(1, order + 1):
            power = [p * u for p, u in zip(power, unit)]
            diff = [power[i + 1] - power[i] for i in range(N)]
            ck = T / (2 * k * k * mp.pi * mp.pi)
            coeff[k - 1] = [float(ck * mp.fsum(rx[i] * diff[i].real for i in range(N))),
                            float(ck * mp.fsum(rx[i] * diff[i].imag for i in range(N))),
                            float(ck * mp.fsum(ry[i] * diff[i].real for i in range(N))),
                            float(ck * mp.fsum(ry[i] * diff[i].imag for i in range(N)))]
        loc = []
        for a, d, r in ((0, dx, rx), (1, dy, ry)):
            run, s = mp.mpf(0), mp.mpf(0)
            for i in range(N):
                run += d[i]
                s += d[i] / (2 * dt[i]) * (t[i + 1] ** 2 - t[i] ** 2) + (run - r[i] * t[i + 1]) * dt[i]
            loc.append(float(pts[0][a] + s / T))
        return coeff, np.asarray(loc), float(mp.mpf(2) ** -53 * N * T)


def ratios(coeff, loc, ref):
    """The error of one contour's result in units of the bound's terms -> (largest coefficient ratio, its index (k - 1, j),
    largest location ratio): ``|value - truth| / U`` and ``(|value - truth| - 2^-53 |truth|) / U`` (at least 0)."""
    tc, tl, U = ref
    ec = np.abs(np.asarray(coeff, np.float64) - tc) / U
    el = np.maximum(np.abs(np.asarray(loc, np.float64) - tl) - 2. ** -53 * np.abs(tl), 0.) / U
    at = np.unravel_index(int(np.argmax(np.where(np.isnan(ec), np.inf, ec))), ec.shape)
    worst = lambda e: float(np.inf if np.isnan(e).any() else e.max())
    return worst(ec), tuple(int(i) for i in at), worst(el)


# ---- the generators of the GPU tests (tests/test_gpu_fourier.py); the bound's constants are measured over them ----
def ragged_walk(segments, seed, closed=False, center=(300, 200)):
    """A closed integer walk of ``segments`` segments around a ragged disc (consecutive points about one pixel apart, sometimes
    equal): int32 [segments, 2] given open, or [segments + 1, 2] with the first point repeated at the end."""
    rng = np.random.default_rng(seed)
    n = segments
    if n == 1:
        p = np.asarray([center], np.int32)
        return np.concatenate([p, p])  # the doubled point of labels2contours
    theta = 2 * np.pi * np.arange(n) / n
    radius = max(1.5, n / 5.) * (1 + 0.2 * np.sin(3 * theta + rng.uniform(0, 6)) + 0.1 * rng.uniform(-1, 1, n))
    p = np.stack([center[0] + radius * np.cos(theta), center[1] + radius * np.sin(theta)], -1).round().astype(np.int32)
    if n == 2:
        return p if not closed else np.concatenate([p, p[:1]])
    if (p[0] == p[-1]).all():
        p[-1, 0] += 2  # given open means open
    return np.concatenate([p, p[:1]]) if closed else p


def edge_segments():
    return [1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 5 * CHUNK + 7]


def edge_contours():
    """One contour per chunk edge, alternately given open and closed; the one-segment contour is the doubled point."""
    out = []
    for i, n in enumerate(edge_segments()):
        c = ragged_walk(n, 100 + n, closed=bool(i % 2), center=(300 + 7 * i, 200 + 3 * i))
        assert len(close(c)) - 1 == n, (n, len(c))
        out.append(c)
    return out


def long_contour():
    """20 CHUNK points (given open)."""
    return ragged_walk(20 * CHUNK, 7, center=(2000, 1500))


def tiny_contours(count=20000, seed=11):
    """``count`` contours of 4 - 12 points around slide coordinates -> (points int32 [P, 2], offsets int64 [count + 1])."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(4, 13, count)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    k = np.repeat(np.arange(count), lengths)
    j = np.arange(offsets[-1]) - offsets[k]
    theta = 2 * np.pi * j / lengths[k] + rng.uniform(0, 6, count)[k]
    radius = (1.5 + 0.25 * lengths[k]) * (1 + 0.2 * rng.uniform(-1, 1, offsets[-1]))
    cx, cy = rng.integers(20, 16000, count)[k], rng.integers(20, 16000, count)[k]
    points = np.stack([cx + radius * np.cos(theta), cy + radius * np.sin(theta)], -1).round().astype(np.int32)
    return points, offsets


def tiny_sample(count=20000, take=200):
    return np.random.default_rng(5).choice(count, take, replace=False)
