"""One set of weight-gradient cases per slab-kernel instantiation (test data and helpers: no tests, not a conftest).

csrc/wgrad_dense.h compiles ct_wgrad_slab_kernel<K, MT, Source> once per filter size a route accepts: the plain source of
``nn.conv2d`` (route 'dense'), the concat source of ``nn.cat_conv2d`` ('concat'), the bilinear source of ``nn.resized_conv2d``
('resized').  Which k a route accepts is asked of the library (``accepted_ks``: the info entry points, host arithmetic, no GPU),
not restated here: tests/test_train_tiles.py holds KS below against that answer.  The constants the edges are computed from
(CT_CH, WGS_STEP, mt) are held against the text of the two headers there, too.

Keys: '<route>/k<K>/<geometry>', e.g. 'concat/k5/tiles'; '<route>/k<K>' is one compiled kernel.
Values: n, h, w (the size of dY), cin, cout, the ``slab_rows`` values the entry is run at, for 'concat' c0, c1 and the top's size,
for 'resized' the low size.

The geometries, and what they are for (``edges()`` computes what an entry shows at one slab_rows from the shape, the constants and
the partition the library reports; the union over the entries and slab_rows of an instantiation must be every edge but EXEMPT):

  tiles    N = 3, 5 x 33 (resized: 6 x 34, the exact double of its 3 x 17 source, so that the entry stays in the exact test),
           160 -> 160 channels at MT = 2 and 160 -> 96 at MT = 1: two co tiles and three ci tiles, both last tiles one 32-channel
           fragment.  slab_rows 8: a slab of 264 pixels (chunks of 128, 128 and 8: one partial step) with the second image
           starting inside its second chunk, then a partial last slab of 7 rows.  Concat: C0 = 32, C1 = 128, the first ci tile
           holds both sources.  Two by three tiles, not two by two: ANY one-to-one map of blockIdx.y onto the tile pairs is a
           right decomposition (``% tiles_co`` with ``/ tiles_co`` is one, on every grid), and with equal counts so are the
           roles swapped and the split by the wrong count; with unequal counts those two leave a ci tile unwritten.
  exact    N = 2, 4 x 32, 32 -> 32: slabs of exactly one and exactly two chunks.
  narrow<W>  N = 2, 9 x W for every W <= k / 2: the row neighbours t + kx of a pixel in the staged flat range are pixels of other
           image rows for the off-centre taps, and only the column test keeps them out.  Every tap with |kx - k / 2| >= W has
           S = 0, so the bound demands exactly 0 there.
  short    N = 2, H x 9 with H = min(2, k / 2): filter rows that leave the image from every pixel.

  edge            shown when
  grid            tiles_co >= 2 and tiles_ci >= 2 in one launch (the decomposition of blockIdx.y)
  grid_skew       ... and tiles_co != tiles_ci
  co_part         Cout % (64 MT) == 32: the last co tile holds one 32-channel fragment, the rest are rows of zeros
  ci_part         Cin % 64 == 32
  chunks3         some slab has >= 3 chunks of CT_CH pixels
  step_part       some slab's pixel count is no multiple of WGS_STEP
  chunk_exact     some slab's pixel count is a multiple of CT_CH: the last chunk takes the full-chunk branch
  image_in_chunk  a batch boundary falls strictly inside a chunk of a slab
  n3              N >= 3: ``row % H`` of the column table over a third image
  last_slab       the last slab has fewer rows than the others
  narrow          1 <= W <= k / 2 with H >= 2
  short           1 <= H <= k / 2 with W >= 2
  straddle        concat only: a 64-channel ci tile holds channels of both sources

The exact test (small integers) needs blend weights that are multiples of 1 / 4 per axis: ``dyadic()`` says which resized entries
have them, INEXACT names the others with the reason, and tests/test_train_tiles.py holds the two against each other.
"""
import functools
import re

CT_CH = 128     # pixels per staged chunk (csrc/wgrad_dense.h)
WGS_STEP = 16   # pixels per MFMA step (csrc/wgrad_slabs.h)


def mt(k):
    """ct_mt of csrc/wgrad_dense.h: 32-channel co fragments per wave."""
    return 2 if k <= 3 else 1


ROUTES = ('dense', 'concat', 'resized')
SOURCES = dict(dense='CtDense', concat='CcSources', resized='BlSource')
KS = dict(dense=(1, 3, 5, 7), concat=(1, 3, 5, 7), resized=(3, 5, 7))
EDGES = ('grid', 'grid_skew', 'co_part', 'ci_part', 'chunks3', 'step_part', 'chunk_exact', 'image_in_chunk', 'n3', 'last_slab', 'narrow',
         'short', 'straddle')


def _table():
    out = {}
    for route in ROUTES:
        for k in KS[route]:
            shapes = dict(tiles=dict(n=3, h=5, w=33, cin=160, cout=160 if k <= 3 else 96, slab_rows=(8, 1, 0)),
                          exact=dict(n=2, h=4, w=32, cin=32, cout=32, slab_rows=(4, 8)))
            for w in range(1, k // 2 + 1):
                shapes[f'narrow{w}'] = dict(n=2, h=9, w=w, cin=32, cout=32, slab_rows=(0, 4))
            if k >= 3:
                shapes['short'] = dict(n=2, h=min(2, k // 2), w=9, cin=32, cout=32, slab_rows=(0, 1))
            for name, cfg in shapes.items():
                half = ((cfg['h'] + 1) // 2, 1 if name.startswith('narrow') else (cfg['w'] + 1) // 2)
                if route == 'concat':  # the lateral's 32 channels in front: every first ci tile holds both sources
                    cfg.update(c0=32, c1=cfg['cin'] - 32 if name == 'tiles' else 32, top=half)
                    cfg['cin'] = cfg['c0'] + cfg['c1']
                elif route == 'resized':
                    if name == 'tiles':
                        cfg.update(h=6, w=34)
                    cfg.update(low=(3, 17) if name == 'tiles' else half)
                out[f'{route}/k{k}/{name}'] = cfg
    return out


TABLE = _table()

# edges an instantiation cannot show: key pattern -> (edges, reason)
EXEMPT = (
    (r'(dense|resized)/', ('straddle',), 'one source: no ci tile holds channels of two tensors'),
    (r'\w+/k1$', ('narrow', 'short'), 'a 1x1 filter has no off-centre tap: no image is narrower or shorter than its padding'),
)

# resized entries the exact test leaves out: key pattern -> reason (the bound test runs them all)
INEXACT = (
    (r'resized/k\d/narrow\d$', '9 rows from 5: lambda_y = 5/9 (d + 1/2) - 1/2 is no dyadic fraction, the bf16 blend of integers is rounded'),
    (r'resized/k\d/short$', '9 columns from 5, likewise'),
)


def parse_key(key):
    """'concat/k5/tiles' -> ('concat', 5, 'tiles')"""
    route, k, name = key.split('/')
    return route, int(k[1:]), name


def instantiation(key):
    """The key without its geometry: one compiled kernel."""
    return key.rsplit('/', 1)[0]


def cases():
    """[(key, slab_rows)] of every entry."""
    return [(key, sr) for key, cfg in TABLE.items() for sr in cfg['slab_rows']]


def case_id(case):
    return f'{case[0]}@{case[1]}'


def info(key, slab_rows, cfg=None):
    """The partition the library reports for an entry: dict(slabs, slab_rows, steps, reduce_chain, bias_chain)."""
    from celldetection_amd import nn
    route, k, _ = parse_key(key)
    c = cfg or TABLE[key]
    if route == 'dense':
        return nn.weight_grad_info(c['n'], c['h'], c['w'], c['cin'], c['cout'], k, slab_rows)
    if route == 'concat':
        return nn.cat_weight_grad_info(c['n'], c['h'], c['w'], c['c0'], c['c1'], c['top'], c['cout'], k, slab_rows)
    return nn.resized_weight_grad_info(c['n'], c['h'], c['w'], c['cin'], c['low'], c['cout'], k, slab_rows)


def accepted_ks(route, ks=range(1, 10)):
    """The filter sizes the route's info entry point accepts on a plain 4 x 4 geometry."""
    cfg = dict(n=2, h=4, w=4, cin=64, cout=32, c0=32, c1=32, top=(2, 2), low=(2, 2), slab_rows=(0,))
    out = []
    for k in ks:
        try:
            info(f'{route}/k{k}/probe', 0, cfg)
            out.append(k)
        except RuntimeError:
            pass
    return tuple(out)


def partition(rows, w, requested, reported_slab_rows):
    """wgs_partition of csrc/wgrad_slabs.h for a requested slab_rows; for 0 (auto: ceil(rows / slabs wanted), the kernel's own
    choice) the rows per slab the library reported -> (slab_rows, slabs, steps)."""
    sr = min(requested, rows) if requested > 0 else reported_slab_rows
    return sr, -(-rows // sr), -(-sr * w // WGS_STEP)


def slab_pixels(cfg, part):
    """[(first pixel, pixel count)] of every slab of dict(slabs, slab_rows)."""
    rows, sr, w = cfg['n'] * cfg['h'], part['slab_rows'], cfg['w']
    return [(s * sr * w, (min(rows, (s + 1) * sr) - s * sr) * w) for s in range(part['slabs'])]


def tiles(key):
    """(tiles_co, tiles_ci) of the launch."""
    cfg, k = TABLE[key], parse_key(key)[1]
    return -(-cfg['cout'] // (64 * mt(k))), -(-cfg['cin'] // 64)


def edges(key, slab_rows, part):
    """{edge: shown} of a TABLE entry run at ``slab_rows`` on the partition ``part`` the library reported for it."""
    route, k, _ = parse_key(key)
    cfg = TABLE[key]
    n, h, w = cfg['n'], cfg['h'], cfg['w']
    slabs = slab_pixels(cfg, part)
    counts = [c for _, c in slabs]
    tco, tci = tiles(key)
    image = h * w
    inside = any(p0 < b < p0 + c and (b - p0) % CT_CH for p0, c in slabs for b in range(image, n * image, image))
    return dict(grid=tco >= 2 and tci >= 2, grid_skew=tco >= 2 and tci >= 2 and tco != tci, co_part=cfg['cout'] % (64 * mt(k)) == 32, ci_part=cfg['cin'] % 64 == 32,
                chunks3=any(-(-c // CT_CH) >= 3 for c in counts), step_part=any(c % WGS_STEP for c in counts),
                chunk_exact=any(c % CT_CH == 0 for c in counts), image_in_chunk=inside, n3=n >= 3,
                last_slab=len(counts) >= 2 and counts[-1] < counts[0], narrow=k > 1 and 1 <= w <= k // 2 and h >= 2,
                short=k > 1 and 1 <= h <= k // 2 and w >= 2,
                straddle=route == 'concat' and cfg['c0'] % 64 != 0 and cfg['c1'] > 0)


def exempt(inst):
    out = set()
    for pattern, names, _ in EXEMPT:
        if re.match(pattern, inst):
            out.update(names)
    return out


def inexact(key):
    """The written reason why the exact test leaves the entry out, or None."""
    for pattern, reason in INEXACT:
        if re.match(pattern, key):
            return reason
    return None


def dyadic(key):
    """Whether small integers go through the entry's staging unrounded: always for the plain and the concat source (a gather);
    for the bilinear source when every lambda is a multiple of 1 / 4, so that every blend weight is a multiple of 1 / 16."""
    if parse_key(key)[0] != 'resized':
        return True
    import bilinear_oracle
    cfg = TABLE[key]
    return all(float(lam) * 4 == int(float(lam) * 4)
               for out, low in zip((cfg['h'], cfg['w']), cfg['low']) for lam in bilinear_oracle.taps(out, low)[2])


def locate(key, index):
    """Where the element (co, ci, ky, kx) of dW lies in the launch: the instantiation, its tile and fragment of both channel axes,
    whether that tile is the partial last one, the tap."""
    route, k, _ = parse_key(key)
    cfg = TABLE[key]
    co, ci, ky, kx = (int(v) for v in index)
    m = mt(k)
    tco, tci = tiles(key)

    def part(tile, count, extent, total):
        return ' (the partial last tile)' if tile == count - 1 and total % extent else ''

    where = f'co tile {co // (64 * m)} of {tco}{part(co // (64 * m), tco, 64 * m, cfg["cout"])} fragment {co % (64 * m) // 32}, ' \
            f'ci tile {ci // 64} of {tci}{part(ci // 64, tci, 64, cfg["cin"])} block {ci % 64 // 32}'
    if route == 'concat':
        where += ' (lateral)' if ci < cfg['c0'] else ' (top)'
    return f'{key} <{k},{m},{SOURCES[route]}>: worst element {(co, ci, ky, kx)} in {where}, tap ({ky}, {kx})'


def locate_bias(key, co):
    return f'{key} bias gradient: worst element {int(co)} (block {int(co) // 32} of {TABLE[key]["cout"] // 32})'


def worst_index(err, tol):
    """Index of the largest err / tol (an error where tol is 0 counts as infinite), for naming a failure."""
    import torch
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    return tuple(int(v) for v in torch.unravel_index(torch.argmax(ratio), ratio.shape))


# ---- operands and fp64 references, once per entry

def _seed(key):
    import zlib
    return zlib.crc32(key.encode()) % (1 << 31)


def _draw(key, kind):
    """{x | lateral, top, dy}: bf16-exact normal values ('normal') or integers in [-4, 4] ('integer'), fp32 NCHW on the CPU."""
    import torch
    route = parse_key(key)[0]
    cfg = TABLE[key]
    g = torch.Generator().manual_seed(_seed(key) + (kind == 'integer'))

    def draw(*shape):
        if kind == 'integer':
            return torch.randint(-4, 5, shape, generator=g).float()
        return torch.randn(*shape, generator=g).to(torch.bfloat16).float()

    n, h, w = cfg['n'], cfg['h'], cfg['w']
    if route == 'dense':
        ops = dict(x=draw(n, cfg['cin'], h, w))
    elif route == 'concat':
        ops = dict(lateral=draw(n, cfg['c0'], h, w), top=draw(n, cfg['c1'], *cfg['top']))
    else:
        ops = dict(x=draw(n, cfg['cin'], *cfg['low']))
    ops['dy'] = draw(n, cfg['cout'], h, w)
    return ops


@functools.lru_cache(maxsize=None)
def operands(key, kind):
    """The operands of an entry and the fp64 statements of its gradients, computed once: dict(x | lateral, top, dy, wgrad = (dW, S),
    bgrad = (db, S)).  The resized route's dW statement under random operands is a window (tests/bilinear_oracle.py
    ``wgrad_tolerance``), taken where it is judged; with integers and dyadic weights it is ``bilinear_oracle.wgrad``, exact."""
    import bilinear_oracle
    import cat_conv_oracle
    import conv_train_oracle
    route, k, _ = parse_key(key)
    ops = _draw(key, kind)
    if route == 'dense':
        ops['wgrad'] = conv_train_oracle.wgrad(ops['x'], ops['dy'], k)
    elif route == 'concat':
        ops['wgrad'] = cat_conv_oracle.wgrad(ops['lateral'], ops['top'], ops['dy'], k)
    elif kind == 'integer':
        ops['wgrad'] = bilinear_oracle.wgrad(ops['x'], ops['dy'], k)
    ops['bgrad'] = conv_train_oracle.bgrad(ops['dy'])
    return ops


def weight_grad(key, ops, slab_rows, **kw):
    """The route's public ``*_weight_grad`` on the operands of an entry -> (dW, db)."""
    from celldetection_amd import nn
    route, k, _ = parse_key(key)
    if route == 'dense':
        return nn.conv2d_weight_grad(ops['x'].cuda(), ops['dy'].cuda(), k, slab_rows, **kw)
    if route == 'concat':
        return nn.cat_conv2d_weight_grad(ops['lateral'].cuda(), ops['top'].cuda(), ops['dy'].cuda(), k, slab_rows, **kw)
    return nn.resized_conv2d_weight_grad(ops['x'].cuda(), ops['dy'].cuda(), k, slab_rows, **kw)
