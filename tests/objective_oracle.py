"""Oracle of the CPN training objective (``celldetection_amd.objective``): the reference's ``CPN.forward(inputs, targets)`` in
training mode (celldetection/models/cpn.py:561-692 with ``compute_loss`` :441-559), restated in numpy.  Test infrastructure only.

Everything that feeds a discontinuity is computed in float32 in the reference's order of operations: the decode (sin terms
summed first, then the cos terms), the scaling after the decode, round half to even / clamp / gather / add of every refinement
iteration, the minimum and maximum over the samples, the ``>= 1`` box filter and the differences of the L1 terms.  The loss
elements of the score and iou terms, all sums and the analytic gradients are float64.  The cos / sin tables and the bucket
tables come from torch on the CPU with the reference's expressions: numpy's float32 cos need not round like torch's.

``objective(...)`` returns a dict:
    terms    name -> (value float64 or None, n)     value: the weighted term, n: number of summed elements
    loss     float64 sum of the terms
    grads    name -> (value float64, m int64, A float64) arrays of the map's shape: m contributions of total magnitude A
    detail   proposals [P, S, 2], refined (list of [P, S, 2], clamped), boxes [P, 4], index (b, y, x)       (float32 / int64)

``rules`` switches single wrong rules on, so that the tests can show that the fixture tells them apart (WRONG_RULES).
"""
from collections import OrderedDict

import numpy as np
import torch

F32 = np.float32
KEYS = ('fourier', 'location', 'contour', 'score', 'refinement', 'boxes', 'iou', 'uncertainty')
DEFAULT_WEIGHTS = {'fourier': 1., 'location': 1., 'contour': 3., 'score_bg': 1., 'score_fg': 1., 'refinement': 1., 'boxes': .88,
                   'iou': 1., 'uncertainty': 1.}
WRONG_RULES = ('cos_first', 'scale_first', 'fg_negative', 'last_tie', 'open_clamp', 'filter_targets', 'joint_score_mean',
               'grad_through_round')


def order_weighting(order, max_w=5, min_w=1):
    """ops/cpn.py:230-235 -> float32 [order] (order 1 gives NaN there: 0 / 0)."""
    x = torch.arange(order).float()
    y = min_w + (max_w - min_w) * (1 - (x / (order - 1)).clamp(0., 1.)) ** 2
    return y.numpy()


def sampling_tables(sampling, order):
    """ops/cpn.py:66-78 per image: sampling float32 [N, S] -> cos, sin float32 [N, order, S]."""
    t = torch.as_tensor(np.asarray(sampling, F32))
    c = float(np.pi) * 2 * (torch.arange(1, order + 1)[..., None]) * t[:, None, :]
    return torch.cos(c).numpy(), torch.sin(c).numpy()


def bucket_tables(sampling, buckets):
    """ops/cpn.py:238-255 per image -> (int64 [N, 3, S], float32 [N, 3, S])."""
    base = torch.as_tensor(np.asarray(sampling, F32)) * buckets
    whole = base.long()
    idx, wgt = [], []
    for j in (whole - 1, whole, whole + 1):
        dist = torch.abs(j + 0.5 - base)
        wgt.append(torch.where(dist > 1, torch.zeros_like(dist), 1. - dist))
        idx.append(j % buckets)
    return torch.stack(idx, 1).numpy(), torch.stack(wgt, 1).float().numpy()


def _nearest(out, inn):
    if out == inn:
        return np.arange(out)
    if out == 2 * inn:
        return np.arange(out) >> 1
    scale = F32(inn) / F32(out)
    return np.minimum(np.floor(np.arange(out, dtype=F32) * scale).astype(np.int64), inn - 1)


def downsample_labels(labels, h, w):
    """ops/commons.py:51-78: max pooling with kernel (H // h, W // w), then nearest interpolation when the size still differs."""
    labels = np.asarray(labels).astype(np.int64)
    N, H, W = labels.shape
    if (H, W) == (h, w):
        return labels
    kh, kw = H // h, W // w
    ph, pw = H // kh, W // kw
    r = labels[:, :ph * kh, :pw * kw].reshape(N, ph, kh, pw, kw).max((2, 4))
    if (ph, pw) != (h, w):
        r = r[:, _nearest(h, ph)][:, :, _nearest(w, pw)]
    return r


class _Grad:
    def __init__(self, shape):
        self.v, self.m, self.a = np.zeros(shape), np.zeros(shape, np.int64), np.zeros(shape)

    def add(self, index, values):
        values = np.broadcast_to(np.asarray(values, np.float64), np.broadcast(*index).shape)
        np.add.at(self.v, index, values)
        np.add.at(self.a, index, np.abs(values))
        np.add.at(self.m, index, (values != 0).astype(np.int64))

    def result(self):
        return self.v, self.m, self.a


def _nan0(x):
    return x if np.isfinite(F32(x)) else 0.


def _giou(a, t):
    """1 - GIoU of paired boxes (ops/boxes.py:101-126, ops/loss.py:90-110) and its gradient by the box ``a``, float64.  Ties of
    ``maximum`` / ``minimum`` split the gradient evenly, ``clamp(min=0)`` passes it on ``>= 0`` (torch's rules)."""
    a, t = a.astype(np.float64), t.astype(np.float64)
    g = np.zeros_like(a)
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])

    def part(u, v, larger):  # d max(u, v) / du  or  d min(u, v) / du
        return np.where(u == v, .5, np.where((u > v) if larger else (u < v), 1., 0.))

    lt = np.maximum(a[:, :2], t[:, :2])
    rb = np.minimum(a[:, 2:], t[:, 2:])
    d = rb - lt
    wh = np.maximum(d, 0)
    dm = (d >= 0).astype(np.float64)
    inter = wh[:, 0] * wh[:, 1]
    union = a1 + a2 - inter
    lti = np.minimum(a[:, :2], t[:, :2])
    rbi = np.maximum(a[:, 2:], t[:, 2:])
    di = rbi - lti
    whi = np.maximum(di, 0)
    dim = (di >= 0).astype(np.float64)
    enc = whi[:, 0] * whi[:, 1]
    with np.errstate(all='ignore'):
        giou = inter / union - (enc - union) / enc
        d_union = -inter / union ** 2 + 1 / enc
        d_inter = 1 / union - d_union
        d_enc = -union / enc ** 2
    for c in (0, 1):
        o = 1 - c
        # intersection
        g[:, c] += d_inter * wh[:, o] * dm[:, c] * -part(a[:, c], t[:, c], True)
        g[:, 2 + c] += d_inter * wh[:, o] * dm[:, c] * part(a[:, 2 + c], t[:, 2 + c], False)
        # enclosing box
        g[:, c] += d_enc * whi[:, o] * dim[:, c] * -part(a[:, c], t[:, c], False)
        g[:, 2 + c] += d_enc * whi[:, o] * dim[:, c] * part(a[:, 2 + c], t[:, 2 + c], True)
        # area of a
        g[:, c] += d_union * -(a[:, 2 + o] - a[:, o])
        g[:, 2 + c] += d_union * (a[:, 2 + o] - a[:, o])
    return 1 - giou, -g


def objective(scores, locations, refinement, fourier, targets, size, order, classes=2, refine=True, iterations=4, buckets=1,
              order_weights=None, weights=None, rules=()):
    """The objective on numpy arrays.  ``order_weights``: float32 [order] or None (= 1)."""
    rules = frozenset(rules)
    assert rules <= frozenset(WRONG_RULES), rules
    wts = dict(DEFAULT_WEIGHTS)
    wts.update(weights or {})
    scores, locations, fourier = (np.asarray(a, F32) for a in (scores, locations, fourier))
    N, cs, h, w = scores.shape
    H, W = size
    oc = fourier.shape[1] // 4
    do_refine = bool(refine) and iterations > 0 and refinement is not None
    sampling = np.asarray(targets['sampling'], F32)
    S = sampling.shape[1]
    terms = OrderedDict((k, (None, 0)) for k in KEYS)
    g_scores, g_loc, g_fourier = _Grad(scores.shape), _Grad(locations.shape), _Grad(fourier.shape)
    g_ref = _Grad(np.shape(refinement)) if refinement is not None else None

    lab = downsample_labels(targets['labels'], h, w)
    fg = (lab != 0) if 'fg_negative' in rules else (lab > 0)
    bg = lab == 0
    b, y, x = np.nonzero(fg)
    P = len(b)
    rows = lab[b, y, x] - 1

    # ---- score (cpn.py:508-523)
    def score_elements(sel, foreground):
        sb, sy, sx_ = np.nonzero(sel)
        z = scores[sb, :, sy, sx_].astype(np.float64)  # [n, cs]
        if cs == 1:
            z = z[:, 0]
            t = 1. if foreground else 0.
            e = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
            with np.errstate(over='ignore'):
                sig = np.where(z >= 0, 1 / (1 + np.exp(-z)), np.exp(z) / (1 + np.exp(z)))
            return e, (sig[:, None], np.full((len(sb), 1), -t)), (sb, sy, sx_)
        cls = np.zeros(len(sb), np.int64)
        if foreground:
            cls = np.asarray(targets['classes'])[sb, lab[sb, sy, sx_] - 1].astype(np.int64) if targets.get('classes') is not None \
                else np.ones(len(sb), np.int64)
        zm = z.max(1, keepdims=True)
        ex = np.exp(z - zm)
        lse = zm[:, 0] + np.log(ex.sum(1))
        soft = ex / ex.sum(1, keepdims=True)
        hot = np.zeros_like(soft)
        hot[np.arange(len(sb)), cls] = -1
        return lse - z[np.arange(len(sb)), cls], (soft, hot), (sb, sy, sx_)

    parts = [(score_elements(fg, True), wts['score_fg']), (score_elements(bg, False), wts['score_bg'])]
    n_score = sum(len(p[0][0]) for p in parts)
    value = None
    if 'joint_score_mean' in rules and n_score:
        value = sum(p[0][0].sum() for p in parts) / n_score * wts['score_fg']
    for (e, de, (sb, sy, sx_)), wt in parts:
        if not len(e):
            continue
        if 'joint_score_mean' in rules:
            n = n_score
        else:
            n = len(e)
            value = (value or 0.) + _nan0(e.sum() / n) * wt
        for c in range(cs):  # sigmoid - target, softmax - one-hot: a difference, so two contributions each
            for d in de:
                g_scores.add((sb, np.full_like(sb, c), sy, sx_), d[:, c] * (wt / n))
    terms['score'] = (value, n_score)

    detail = dict(proposals=np.zeros((0, S, 2), F32), refined=[], boxes=np.zeros((0, 4), F32), index=(b, y, x))
    if P:
        cos_t, sin_t = sampling_tables(sampling, order)
        cos_p, sin_p = cos_t[b], sin_t[b]  # [P, order, S]
        coef = fourier.reshape(N, oc, 4, h, w)[b, :order, :, y, x]  # [P, order, 4]
        loc = np.stack((locations[b, 0, y, x] + x.astype(F32), locations[b, 1, y, x] + y.astype(F32)), 1)
        scale = np.array([F32(W) / F32(w), F32(H) / F32(h)], F32)
        scale4 = np.array([scale[0], scale[0], scale[1], scale[1]], F32)
        dcoef, dloc = coef, loc
        if 'scale_first' in rules:
            dcoef, dloc = coef * scale4, loc * scale

        def series(col, table):
            acc = dcoef[:, 0, col, None] * table[:, 0]
            for k in range(1, order):
                acc = acc + dcoef[:, k, col, None] * table[:, k]
            return acc

        prop = np.zeros((P, S, 2), F32)
        for c, (sincol, coscol) in enumerate(((1, 0), (3, 2))):
            first, second = series(sincol, sin_p), series(coscol, cos_p)
            if 'cos_first' in rules:
                first, second = second, first
            prop[:, :, c] = (dloc[:, c, None] + first) + second
        if 'scale_first' not in rules:
            prop = prop * scale
        fs, ls = coef * scale4, loc * scale
        hi = np.array([W - 1, H - 1], F32)

        def closed(c):
            return ((c > 0) & (c < hi)) if 'open_clamp' in rules else ((c >= 0) & (c <= hi))

        f_tar = np.asarray(targets['fourier'], F32)[b, rows]
        l_tar = np.asarray(targets['locations'], F32)[b, rows]
        c_tar = np.asarray(targets['sampled_contours'], F32)[b, rows]
        ow = np.ones(order, F32) if order_weights is None else np.asarray(order_weights, F32).reshape(order)

        # ---- refinement (cpn.py:63-85, 650-663)
        sets, gathers = [], []
        if do_refine:
            ref = np.asarray(refinement, F32)
            if buckets > 1:
                bi, bw = bucket_tables(sampling, buckets)
                bi, bw = bi[b], bw[b]  # [P, 3, S]
            c = prop
            for _ in range(iterations):
                r = np.minimum(np.maximum(np.rint(c), F32(0)), hi)
                ix, iy = r[..., 0].astype(np.int64), r[..., 1].astype(np.int64)
                if buckets <= 1:
                    resp = np.stack((ref[b[:, None], 0, iy, ix], ref[b[:, None], 1, iy, ix]), -1)
                    gathers.append([(None, None, iy, ix)])
                else:
                    resp, g = None, []
                    for k in range(3):
                        cur = np.stack((ref[b[:, None], 2 * bi[:, k], iy, ix] * bw[:, k],
                                        ref[b[:, None], 2 * bi[:, k] + 1, iy, ix] * bw[:, k]), -1)
                        resp = cur if resp is None else resp + cur
                        g.append((bi[:, k], bw[:, k].astype(np.float64), iy, ix))
                    gathers.append(g)
                c = r + resp
                sets.append(c)
        else:
            sets = [prop]
        masks = [closed(c) for c in sets]
        sets = [np.minimum(np.maximum(c, F32(0)), hi) for c in sets]
        if not do_refine:
            prop = sets[0]
        last = sets[-1]

        # ---- L1 terms (cpn.py:525-545)
        n4, n2, ns = P * order * 4, P * 2, P * S * 2
        ef = np.abs(fs - f_tar) * ow[None, :, None]
        terms['fourier'] = (_nan0(ef.astype(np.float64).sum() / n4) * wts['fourier'], n4)
        el = np.abs(ls - l_tar)
        terms['location'] = (_nan0(el.astype(np.float64).sum() / n2) * wts['location'], n2)
        ec = np.abs(prop - c_tar)
        terms['contour'] = (_nan0(ec.astype(np.float64).sum() / ns) * wts['contour'], ns)
        if do_refine:
            terms['refinement'] = (sum(_nan0(np.abs(c - c_tar).astype(np.float64).sum() / ns) * wts['refinement'] for c in sets),
                                   ns * len(sets))

        # ---- boxes and iou (cpn.py:665-670, ops/loss.py:90-110)
        def arg(values, largest):
            v = -values if largest else values
            if 'last_tie' in rules:
                return S - 1 - np.argmin(v[:, ::-1], 1)
            return np.argmin(v, 1)

        args = np.stack([arg(last[:, :, 0], False), arg(last[:, :, 1], False), arg(last[:, :, 0], True), arg(last[:, :, 1], True)], 1)
        pr = np.arange(P)
        boxes = np.stack([last[pr, args[:, j], j % 2] for j in range(4)], 1)
        tboxes = np.concatenate((c_tar.min(1), c_tar.max(1)), 1)
        fb = tboxes if 'filter_targets' in rules else boxes
        valid = ((fb[:, 2] - fb[:, 0]) >= 1) & ((fb[:, 3] - fb[:, 1]) >= 1)
        nv = int(valid.sum())
        e_iou, d_iou = _giou(boxes, tboxes)
        terms['iou'] = (_nan0(e_iou[valid].sum() / nv) * wts['iou'] if nv else 0., nv)
        g_last = np.zeros((4, P, S, 2))  # the four box coordinates apart, so that every one counts as its own contribution
        if nv:
            for j in range(4):
                g_last[j, pr[valid], args[valid, j], j % 2] = d_iou[valid, j] * (wts['iou'] / nv)

        # ---- gradients of the contour points
        def l1(cur, wt, n):
            return np.sign(cur.astype(np.float64) - c_tar) * (wt / n)

        to_decode = []  # contributions [P, S, 2] that flow into the decode
        if do_refine:
            to_decode.append(l1(prop, wts['contour'], ns))
            for it, (c, mask, gather) in enumerate(zip(sets, masks, gathers)):
                point = [l1(c, wts['refinement'], ns) * mask]
                if it == len(sets) - 1:
                    point += [g_last[j] * mask for j in range(4)]
                for gp in point:
                    hit = gathers[:it + 1] if 'grad_through_round' in rules else [gather]
                    for ga in hit:
                        for (gbi, gbw, iy, ix) in ga:
                            for ch in (0, 1):
                                if gbi is None:
                                    g_ref.add((b[:, None], np.full_like(iy, ch), iy, ix), gp[..., ch])
                                else:
                                    g_ref.add((b[:, None], 2 * gbi + ch, iy, ix), gp[..., ch] * gbw)
                    if 'grad_through_round' in rules:
                        to_decode.append(gp)
        else:
            to_decode.append(l1(prop, wts['contour'], ns) * masks[0])
            to_decode += [g_last[j] * masks[0] for j in range(4)]

        # ---- decode backwards, fourier and location terms
        cols = ((0, 0, cos_p), (1, 0, sin_p), (2, 1, cos_p), (3, 1, sin_p))  # coefficient column, coordinate, table
        for gp in to_decode:
            for s in range(S):
                for col, c, table in cols:
                    for k in range(order):
                        g_fourier.add((b, np.full_like(b, k * 4 + col), y, x),
                                      gp[:, s, c] * scale[c].astype(np.float64) * table[:, k, s].astype(np.float64))
                for c in (0, 1):
                    g_loc.add((b, np.full_like(b, c), y, x), gp[:, s, c] * scale[c].astype(np.float64))
        df = np.sign(fs.astype(np.float64) - f_tar) * ow[None, :, None].astype(np.float64) * scale4.astype(np.float64) * \
            (wts['fourier'] / n4)
        for k in range(order):
            for col in range(4):
                g_fourier.add((b, np.full_like(b, k * 4 + col), y, x), df[:, k, col])
        dl = np.sign(ls.astype(np.float64) - l_tar) * scale.astype(np.float64) * (wts['location'] / n2)
        for c in (0, 1):
            g_loc.add((b, np.full_like(b, c), y, x), dl[:, c])
        detail = dict(proposals=prop, refined=sets if do_refine else [], boxes=boxes, index=(b, y, x))

    loss = 0.
    for k in KEYS:
        if terms[k][0] is not None:
            loss += terms[k][0]
    grads = dict(scores=g_scores.result(), locations=g_loc.result(), fourier=g_fourier.result(),
                 refinement=g_ref.result() if g_ref is not None else None)
    return dict(terms=terms, loss=loss, grads=grads, detail=detail, labels=lab)


# ---- the fixture tests/golden/objective.npz (written by tests/golden/make_golden_objective.py)
def load_fixture(path=None):
    """-> OrderedDict name -> dict(maps, targets, config, rec): the inputs as float32 / int64 arrays, the keyword arguments of
    ``objective`` and the reference's recorded results."""
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'objective.npz')
    z = np.load(path)
    cases = OrderedDict()
    for name in z['names'].tolist():
        keys = [k[len(name) + 1:] for k in z.files if k.startswith(name + '/')]
        maps = {k: None for k in ('scores', 'locations', 'refinement', 'fourier')}
        maps.update({k[4:]: z[f'{name}/{k}'].astype(F32) for k in keys if k.startswith('map_')})
        targets = {k[7:]: z[f'{name}/{k}'] for k in keys if k.startswith('target_')}
        targets['labels'] = targets['labels'].astype(np.int64)
        c = z[f'{name}/config'].tolist()
        config = dict(order=c[0], classes=c[1], refine=bool(c[2]), iterations=c[3], buckets=c[4], order_weights=bool(c[5]),
                      size=(c[6], c[7]), weights=dict(zip(sorted(DEFAULT_WEIGHTS), z[f'{name}/weights'].tolist())))
        rec = {k: z[f'{name}/{k}'] for k in keys if not k.startswith(('map_', 'target_')) and k not in ('config', 'weights')}
        cases[name] = dict(maps=maps, targets=targets, config=config, rec=rec)
    return cases


def run_case(case, rules=()):
    m, c = case['maps'], case['config']
    ow = order_weighting(c['order']) if c['order_weights'] else None
    return objective(m['scores'], m['locations'], m['refinement'], m['fourier'], case['targets'], c['size'], c['order'],
                     classes=c['classes'], refine=c['refine'], iterations=c['iterations'], buckets=c['buckets'], order_weights=ow,
                     weights=c['weights'], rules=rules)


L1_TERMS = ('fourier', 'location', 'contour', 'refinement')


def term_bound(key, n):
    """Relative distance allowed between the oracle's float64 term and the reference's recorded float32 one.  L1 terms: the
    reference sums n non-negative float32 elements in some order (relative error at most (n - 1) * 2^-24 whatever the order), and
    rounds the subtraction behind every element (exact here or common to both), the mean, the weight and, for the refinement
    term, the sum over the iterations: (n + 8) * 2^-24.  The score and iou elements are float32 functions there (log, exp,
    divisions) and float64 functions here: a cap of (n + 64) * 2^-24, the measured ratio is in objective_measured.json."""
    return (n + (8 if key in L1_TERMS else 64)) * 2. ** -24


def departs(res, rec, say=None):
    """Does an oracle result break a bound that the tests hold the right rule to, against the recorded results ``rec``?
    say: a function that is told where."""
    say = say or (lambda *a: None)
    d = res['detail']
    last = d['refined'][-1] if d['refined'] else d['proposals']
    if not (np.array_equal(d['proposals'], rec['proposals']) and np.array_equal(d['boxes'], rec['boxes']) and
            np.array_equal(last, rec['contours'])):
        say('contours or boxes')
        return True
    for k in KEYS:
        v, n = res['terms'][k]
        if (v is None) != bool(rec['none_' + k]):
            say('term', k, v, 'None' if rec['none_' + k] else 'not None')
            return True
        r = float(rec['term_' + k])
        if v is not None and abs(v - r) > term_bound(k, n) * abs(r):
            say('term', k, v, r, n)
            return True
    for k in ('scores', 'locations', 'fourier', 'refinement'):
        if res['grads'][k] is None:
            continue
        v, m, a = res['grads'][k]
        r = rec['grad_' + k].astype(np.float64)
        with np.errstate(invalid='ignore'):
            bad = ~(np.abs(v - r) <= (m + 8) * 2. ** -24 * a) & ~(np.isnan(v) & np.isnan(r))
        if bad.any():
            i = tuple(int(j) for j in np.argwhere(bad)[0])
            say('gradient', k, int(bad.sum()), 'of', bad.size, 'first', i, v[i], r[i], m[i], a[i])
            return True
    return False
