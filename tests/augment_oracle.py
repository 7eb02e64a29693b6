"""The numpy statement of the augmentation warp (the "Augmentation warp" section of include/cpn_hip.h): fp64 positions, an fp32 blend
in the stated order of operations, integer labels; a float64 ``truth`` of the blend; and the bound between the two, derived from
the roundings of the formula.  Independent of celldetection_amd: nothing here imports the package.

One sample at a time: ``image`` [H, W, K] uint8 or float32, ``labels`` [H, W, C] integers, ``m`` float64[6] (destination pixel ->
source position), ``size`` = (h, w).
"""
import numpy as np

U = 2.0 ** -24  # the unit roundoff of fp32


def positions(m, size):
    """-> (sx, sy) float64 [h, w]: sx = (m0 j + m1 i) + m2, sy = (m3 j + m4 i) + m5, every operation rounded to fp64."""
    h, w = size
    m = np.asarray(m, dtype=np.float64)
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    return (m[0] * j + m[1] * i) + m[2], (m[3] * j + m[4] * i) + m[5]


def index(f, n, border):
    """Integer-valued float64 array -> (index int64 in [0, n), inside bool): 'constant' marks what lies outside, 'reflect' is
    reflect-101 (p = 2 (n - 1), i mod p, p - i where that is >= n; n = 1: 0) and everything is inside."""
    i = f.astype(np.int64)
    if border == 'reflect':
        if n == 1:
            return np.zeros_like(i), np.ones(i.shape, dtype=bool)
        p = 2 * (n - 1)
        i = np.mod(i, p)
        return np.where(i >= n, p - i, i), np.ones(i.shape, dtype=bool)
    assert border == 'constant'
    inside = (i >= 0) & (i <= n - 1)
    return np.where(inside, i, 0), inside


def warp_labels(labels, m, size, border='constant', fill=0):
    """-> int32 [h, w, C]: labels[floor(sy + 0.5), floor(sx + 0.5)], integers all the way."""
    labels = np.asarray(labels)
    assert labels.ndim == 3 and labels.dtype.kind in 'iu'
    H, W = labels.shape[:2]
    sx, sy = positions(m, size)
    nx, okx = index(np.floor(sx + 0.5), W, border)
    ny, oky = index(np.floor(sy + 0.5), H, border)
    out = labels[ny, nx].astype(np.int32)
    out[~(okx & oky)] = np.int32(fill)
    return out


def mapped(image, tables):
    """The intensity transform on the whole source -> float32 [H, W, K].  uint8: tables float32 [K, 256] (None: T[v] = v); float32:
    tables [K, 2] = (scale, offset), t = v * scale + offset with product and sum each rounded (None: scale 1, offset 0)."""
    image = np.asarray(image)
    K = image.shape[2]
    if image.dtype == np.uint8:
        tables = np.broadcast_to(np.arange(256, dtype=np.float32), (K, 256)) if tables is None else np.asarray(tables)
        assert tables.dtype == np.float32 and tables.shape == (K, 256)
        return np.stack([tables[k][image[:, :, k]] for k in range(K)], axis=2)
    assert image.dtype == np.float32
    tables = np.broadcast_to(np.array([1., 0.], dtype=np.float32), (K, 2)) if tables is None else np.asarray(tables)
    assert tables.dtype == np.float32 and tables.shape == (K, 2)
    return (image * tables[:, 0]).astype(np.float32) + tables[:, 1]


def _taps(image, m, size, tables, border, fill, dtype):
    t = mapped(image, tables).astype(dtype)
    H, W = t.shape[:2]
    sx, sy = positions(m, size)
    fx, fy = np.floor(sx), np.floor(sy)
    lx, ly = (sx - fx), (sy - fy)  # exact in fp64
    x0, okx0 = index(fx, W, border)
    x1, okx1 = index(fx + 1.0, W, border)
    y0, oky0 = index(fy, H, border)
    y1, oky1 = index(fy + 1.0, H, border)

    def tap(y, x, ok):
        v = t[y, x]
        v[~ok] = dtype(fill)
        return v

    none = ~((oky0 | oky1) & (okx0 | okx1))  # all four taps outside: the output is the fill itself, not a blend of four fills
    return (tap(y0, x0, oky0 & okx0), tap(y0, x1, oky0 & okx1), tap(y1, x0, oky1 & okx0), tap(y1, x1, oky1 & okx1),
            ly[:, :, None], lx[:, :, None], none)


def bf16_round(x):
    """float32 -> the float32 value of its bfloat16 rounding (to nearest even)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.astype(np.uint32).view(np.float32)


def warp_image(image, m, size, tables=None, border='constant', fill=0., bf16=False):
    """-> float32 [K, h, w]: out = (hy * (hx * t00 + lx * t01)) + (ly * (hx * t10 + lx * t11)) with lx = float32(sx - floor(sx)),
    hx = 1.0f - lx (likewise y), every operation rounded to fp32; where all four taps lie outside under 'constant', the fill itself;
    ``bf16``: rounded once more, to bfloat16 (returned as float32)."""
    t00, t01, t10, t11, ly, lx, none = _taps(image, m, size, tables, border, fill, np.float32)
    lx, ly = lx.astype(np.float32), ly.astype(np.float32)
    one = np.float32(1)
    hx, hy = one - lx, one - ly
    out = (hy * (hx * t00 + lx * t01)) + (ly * (hx * t10 + lx * t11))
    assert out.dtype == np.float32
    out[none] = np.float32(fill)
    out = np.ascontiguousarray(out.transpose(2, 0, 1))
    return bf16_round(out) if bf16 else out


def truth(image, m, size, tables=None, border='constant', fill=0.):
    """-> float64 [K, h, w]: the same blend of the same fp32 tap values with fp64 weights and fp64 arithmetic."""
    t00, t01, t10, t11, ly, lx, none = _taps(image, m, size, tables, border, fill, np.float64)
    out = (1 - ly) * ((1 - lx) * t00 + lx * t01) + ly * ((1 - lx) * t10 + lx * t11)
    out[none] = fill
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def bilinear_bound(max_abs_t):
    """The largest distance between ``warp_image`` and ``truth`` for tap values of magnitude <= M = ``max_abs_t``, to first order in
    u = 2^-24, from the seven fp32 roundings a value meets on its way through the formula:

    * the weights.  lx = fl(sx - x0) is off by <= u / 2 (a value below 1); hx = fl(1 - lx) adds <= u / 2 of its own, so hx is off by
      <= u from 1 - (the true lx).  The blend is linear in each weight pair, so the x pair moves the result by <= (u / 2 + u) M and
      the y pair by as much: 3 u M, three roundings' worth;
    * the arithmetic.  An inner product, the inner sum, the outer product and the outer sum are each one relative rounding <= u of
      a quantity of magnitude <= M (the weights of a pair sum to 1 up to u): 4 u M.

    7 u M, times (1 + 2^-10) for every higher-order term (there are fewer than 2^7 products of two of the u's above)."""
    return 7 * U * float(max_abs_t) * (1 + 2.0 ** -10)
