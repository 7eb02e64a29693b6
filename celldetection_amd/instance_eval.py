"""Instance evaluation of label images on the MI355X: ``LabelMatcher`` / ``LabelMatcherList`` of the reference's ``cd.data``
(celldetection/data/instance_eval.py), backed by ``csrc/instance_eval.hip``.

    y = model(x)
    labels = cda.contours2labels(y['contours'][0], x.shape[2:])
    f1 = cda.LabelMatcher(labels, target_labels, iou_thresh=.5).f1

Both label images stay on the GPU: one HIP pass reads them once and counts, in a hash table, the pixels of every
(input label, target label) pair and the elements of every label; the table is compacted and sorted on the device, and the
one-to-one matching at ``iou_thresh`` runs there as well.  The scores need three numbers from the device; the arrays
(``matches``, ``intersections``, ``unions``, ``ious``, ...) are copied to numpy on first access, as the reference returns them.

Semantics (the reference's): values <= 0 are background; a pixel contributes each distinct (input, target) pair once,
however many channels repeat a value; the area of a label counts ELEMENTS over all channels; ``unions = input area +
target area - intersection``; ``ious = intersections / unions`` in float64.  Pairs are taken from the largest IoU down if
their IoU is ``>= iou_thresh`` and neither label belongs to a pair already taken.

The one rule that is this package's own: the reference orders pairs of EQUAL IoU by numpy's unstable ``argsort``, i.e. not
at all.  Here the order is total: larger IoU first, compared exactly as ``i1 * u2`` against ``i2 * u1`` in integers (two
quotients that differ never tie by rounding), and among equal IoU the pair with the smaller (input label, target label)
first, which is the pair that comes first in ``matches``.

``input_counts`` / ``target_counts`` are dicts ``{label: elements}`` over the positive labels (the reference's dicts also
carry negative values, which nothing reads).
"""
from ctypes import c_int64
from warnings import warn

import numpy as np
import torch

from . import _lib
from ._label_input import aligned16, to_int32, upload_numpy
from ._lib import check, ptr, stream_ptr
from ._tables import check_capacity, default_capacity, grow_until_it_fits

__all__ = ['LabelMatcher', 'LabelMatcherList', 'label_pair_table']

MAX_CHANNELS = 8


def _as_device_labels(x, name):
    """-> contiguous, 16-byte aligned int32 Tensor[H, W, C] on the GPU."""
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in 'iub':
            raise TypeError(f'LabelMatcher: {name} must hold integers (got {x.dtype})')
        x = upload_numpy(x, 'LabelMatcher', f'{name} holds labels')
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'LabelMatcher: {name} must be a Tensor on the GPU or a numpy array (got {type(x).__name__})')
    if not x.is_cuda:
        raise RuntimeError('celldetection_amd.LabelMatcher runs on the MI355X only (got a CPU tensor).')
    if x.is_floating_point() or x.is_complex():
        raise TypeError(f'LabelMatcher: {name} must hold integers (got {x.dtype})')
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError(f'LabelMatcher: {name} must be [H, W] or [H, W, C] (got {tuple(x.shape)})')
    if x.shape[2] < 1:
        raise ValueError(f'LabelMatcher: {name} has no channel')
    return aligned16(to_int32(x, f'LabelMatcher: {name} holds labels that do not fit int32'))


def label_pair_table(inputs, targets, table_capacity=None, return_stats=False):
    """The packed, sorted table of the pixel pass: int64 Tensor[N, 2] of (key, count) rows on the GPU, keys ascending.
    ``key = input << 32 | target`` counts the pixels that carry the pair; ``key = label << 32`` the elements of an input
    label; ``key = label`` those of a target label.  ``table_capacity`` (a power of two) is the first size of the hash table;
    it is doubled until every key found a slot."""
    a, b = _as_device_labels(inputs, 'inputs'), _as_device_labels(targets, 'targets')
    if a.shape[:2] != b.shape[:2]:
        raise ValueError(f'LabelMatcher: inputs {tuple(a.shape[:2])} and targets {tuple(b.shape[:2])} differ in size')
    if a.device != b.device:
        raise ValueError('LabelMatcher: inputs and targets are on different devices')
    lib = _lib.load()
    pixels = int(a.shape[0]) * int(a.shape[1])
    cap = default_capacity(pixels, 16) if table_capacity is None else int(table_capacity)
    check_capacity(cap)
    status = (c_int64 * 2)()

    def attempt(cap):
        nbytes = int(lib.cpn_eval_workspace_bytes(cap, 0, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        check(lib.cpn_eval_pairs(ptr(a), int(a.shape[2]), ptr(b), int(b.shape[2]), pixels, cap, ptr(ws), nbytes, stream_ptr()),
              'eval_pairs')
        check(lib.cpn_eval_table_status(ptr(ws), cap, status, stream_ptr()), 'eval_table_status')
        return ws, int(status[0]), int(status[1])

    with torch.cuda.device(a.device):
        ws, cap, grown, n = grow_until_it_fits(cap, attempt)
        keys = torch.empty(n, dtype=torch.int64, device=a.device)
        counts = torch.empty(n, dtype=torch.int64, device=a.device)
        check(lib.cpn_eval_compact(ptr(ws), cap, ptr(keys), ptr(counts), n, stream_ptr()), 'eval_compact')
        keys, order = torch.sort(keys)  # keys are distinct and < 2 ** 63: the order is unique
        table = torch.stack((keys, counts[order]), 1)
    if return_stats:
        return table, dict(table_capacity=cap, grown=grown, entries=n)
    return table


class LabelMatcher:
    """Evaluation of a label image against a target label image (interface of the reference's ``cd.data.LabelMatcher``).

    ``iou_thresh`` is the minimum IoU two objects must have to count as a match; every target object is matched with at
    most one input object and the other way round.  Assigning ``iou_thresh`` selects again from the stored pair table
    without touching the images."""

    def __init__(self, inputs=None, targets=None, iou_thresh=None, zero_division='warn', epsilon=1e-12, table_capacity=None):
        """inputs / targets: label images [H, W] or [H, W, C] (channel counts may differ): integer Tensors on the GPU, or
        numpy arrays, which are uploaded.  zero_division: one of ``('warn', 0, 1)``, the value a score takes when its
        denominator is zero (``'warn'``: 0 with a warning).  table_capacity: first size of the pair hash table (a power
        of two; it grows on demand)."""
        self._iou_thresh = 0. if iou_thresh is None else iou_thresh
        self.zero_division = zero_division if isinstance(zero_division, int) else 0
        self.zero_division_warn = zero_division == 'warn'
        self.epsilon = epsilon
        self.table_capacity = table_capacity
        self._dev = None  # device tensors of the current images
        self._host = {}  # numpy copies, made on first access
        self.stats = {}
        if inputs is not None and targets is not None:
            self.update(inputs, targets, iou_thresh)

    # ---- device side ----------------------------------------------------------------------------------------------------
    def update(self, inputs, targets, iou_thresh=None):
        table, stats = label_pair_table(inputs, targets, self.table_capacity, return_stats=True)
        lib = _lib.load()
        dev = table.device
        keys, counts = table[:, 0].contiguous(), table[:, 1].contiguous()
        hi, lo = keys >> 32, keys & 0xffffffff
        is_t, is_in = hi == 0, lo == 0
        is_pair = ~(is_t | is_in)
        d = dict(target_labels=lo[is_t].contiguous(), target_counts=counts[is_t].contiguous(),
                 input_labels=hi[is_in].contiguous(), input_counts=counts[is_in].contiguous(),
                 pair_keys=keys[is_pair].contiguous(), intersections=counts[is_pair].contiguous())
        P, n_in, n_t = int(d['pair_keys'].shape[0]), int(d['input_labels'].shape[0]), int(d['target_labels'].shape[0])
        d['unions'] = torch.empty(P, dtype=torch.int64, device=dev)
        d['input_index'] = torch.empty(P, dtype=torch.int32, device=dev)
        d['target_index'] = torch.empty(P, dtype=torch.int32, device=dev)
        d['selected'] = torch.zeros(P, dtype=torch.uint8, device=dev)
        nbytes = int(lib.cpn_eval_workspace_bytes(0, P, max(n_in, n_t)))
        d['workspace'] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.cpn_eval_unions(ptr(d['pair_keys']), ptr(d['intersections']), P, ptr(d['input_labels']),
                                      ptr(d['input_counts']), n_in, ptr(d['target_labels']), ptr(d['target_counts']), n_t,
                                      ptr(d['unions']), ptr(d['input_index']), ptr(d['target_index']), ptr(d['workspace']),
                                      stream_ptr()), 'eval_unions')
        self._dev, self._host = d, {}
        self._sizes = (P, n_in, n_t)
        self.stats = dict(stats, pairs=P)
        self.iou_thresh = self.iou_thresh if iou_thresh is None else iou_thresh  # selects

    def _require(self):
        if self._dev is None:
            raise ValueError('No labels found. Add labels before retrieving results.')
        return self._dev

    def filter_and_threshold(self):
        d = self._require()
        lib = _lib.load()
        P, n_in, n_t = self._sizes
        res = (c_int64 * 2)()
        with torch.cuda.device(d['selected'].device):
            check(lib.cpn_eval_select(ptr(d['intersections']), ptr(d['unions']), ptr(d['input_index']), ptr(d['target_index']),
                                      P, n_in, n_t, float(self._iou_thresh), ptr(d['selected']), ptr(d['workspace']),
                                      int(d['workspace'].numel()), res, stream_ptr()), 'eval_select')
        if P == 0:
            d['selected'].zero_()
        self._tp = int(res[0])
        self.stats['selection_rounds'] = int(res[1])
        self._host.pop('_sel', None)

    @property
    def iou_thresh(self):
        return self._iou_thresh

    @iou_thresh.setter
    def iou_thresh(self, v):
        self._require()
        self._iou_thresh = v
        self.filter_and_threshold()

    # ---- arrays (numpy, copied on first access) -------------------------------------------------------------------------
    def _np(self, name, make):
        if name not in self._host:
            self._host[name] = make(self._require())
        return self._host[name]

    @property
    def matches(self):
        """int64 [P, 2]: the distinct (input label, target label) pairs in lexicographic order."""
        def make(d):
            k = d['pair_keys'].cpu().numpy()
            return np.stack((k >> 32, k & 0xffffffff), 1).reshape(-1, 2)
        return self._np('matches', make)

    @property
    def intersections(self):
        return self._np('intersections', lambda d: d['intersections'].cpu().numpy())

    @property
    def unions(self):
        return self._np('unions', lambda d: d['unions'].cpu().numpy())

    @property
    def ious(self):
        return self._np('ious', lambda d: self.intersections / self.unions)

    @property
    def input_labels(self):
        return self._np('input_labels', lambda d: d['input_labels'].cpu().numpy())

    @property
    def target_labels(self):
        return self._np('target_labels', lambda d: d['target_labels'].cpu().numpy())

    @property
    def input_counts(self):
        return self._np('input_counts', lambda d: dict(zip(self.input_labels.tolist(), d['input_counts'].cpu().tolist())))

    @property
    def target_counts(self):
        return self._np('target_counts', lambda d: dict(zip(self.target_labels.tolist(), d['target_counts'].cpu().tolist())))

    @property
    def _sel(self):
        return self._np('_sel', lambda d: d['selected'].cpu().numpy().astype(bool))

    # ---- label sets and counts ------------------------------------------------------------------------------------------
    @property
    def true_positive_labels(self):
        return set(self.matches[:, 0][self._sel])

    @property
    def false_positive_labels(self):
        return set(self.input_labels) - set(self.matches[:, 0][self._sel])

    @property
    def false_negative_labels(self):
        return set(self.target_labels) - set(self.matches[:, 1][self._sel])

    @property
    def true_positives(self):
        self._require()
        return self._tp

    @property
    def false_positives(self):
        self._require()
        return self._sizes[1] - self._tp  # taken pairs have distinct input labels

    @property
    def false_negatives(self):
        self._require()
        return self._sizes[2] - self._tp

    # ---- scores ---------------------------------------------------------------------------------------------------------
    def _zero_div(self, name):
        if self.zero_division_warn:
            warn(f'ZeroDivisionError in {name} calculation. Assuming {self.zero_division} as result.')
        return self.zero_division

    def _score(self, name, fn):
        try:
            return fn(self.true_positives, self.false_positives, self.false_negatives, self.epsilon)
        except ZeroDivisionError:
            return self._zero_div(name)

    @property
    def precision(self):
        return self._score('precision', _precision)

    @property
    def recall(self):
        return self._score('recall', _recall)

    @property
    def f1(self):
        pr, rc = self.precision, self.recall
        try:
            return (2 * pr * rc) / (pr + rc + self.epsilon)
        except ZeroDivisionError:
            return self._zero_div('f1')

    @property
    def jaccard(self):
        return self._score('jaccard', _jaccard)

    @property
    def fowlkes_mallows(self):
        return self._score('fowlkes_mallows', _fowlkes_mallows)


def _precision(tp, fp, fn, eps):
    return tp / (tp + fp + eps)


def _recall(tp, fp, fn, eps):
    return tp / (tp + fn + eps)


def _jaccard(tp, fp, fn, eps):
    return tp / (tp + fn + fp + eps)


def _f1_counts(tp, fp, fn, eps):
    return (2 * tp) / (2 * tp + fn + fp + eps)


def _fowlkes_mallows(tp, fp, fn, eps):
    return tp / np.sqrt((tp + fp) * (tp + fn) + eps)


class LabelMatcherList(list):
    """A list of ``LabelMatcher`` objects with averaged and summed results (interface of the reference's
    ``cd.data.LabelMatcherList``).

        lml = LabelMatcherList([LabelMatcher(p, t) for p, t in zip(predictions, targets)])
        for lml.iou_thresh in (.5, .75):
            print(lml.iou_thresh, lml.avg_f1)

    With ``rank`` and ``num_ranks`` (> 1) the results are combined over all ranks with ``torch.distributed`` collectives on
    ``device``; every example is expected exactly once over the ranks and every rank calls the same members in the same
    order.  ``cache`` keeps combined results until the list or the threshold changes."""

    def __init__(self, *args, epsilon=1e-12, rank=None, num_ranks=None, device=None, cache=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.epsilon = epsilon
        if (rank is None) != (num_ranks is None):
            raise AssertionError('Please provide both `rank` and `num_ranks`.')
        self.rank, self.num_ranks, self.device, self.cache = rank, num_ranks, device, cache
        self._cache = {}
        self._iou_thresh = None

    @property
    def distributed(self):
        return self.rank is not None and self.num_ranks is not None and self.num_ranks > 1

    def clear_cache(self):
        self._cache = {}

    def _cached(self, key, compute):
        if self.cache and key in self._cache:
            return self._cache[key]
        res = compute()
        if self.cache:
            self._cache[key] = res
        return res

    @property
    def iou_thresh(self):
        """The threshold of the items if they agree, the array of distinct thresholds if not."""
        if len(self):
            uni = np.unique([m.iou_thresh for m in self])
            return uni[0] if len(uni) == 1 else uni
        return self._iou_thresh

    @iou_thresh.setter
    def iou_thresh(self, v):
        if self.distributed:  # every rank must ask for the same threshold: rank 0 checks
            import torch.distributed as dist
            mine = torch.tensor([v], device=self.device)
            gathered = [torch.zeros_like(mine) for _ in range(self.num_ranks)] if self.rank == 0 else None
            dist.gather(mine, gather_list=gathered, dst=0)
            if self.rank == 0:
                allv = torch.cat(gathered).ravel()
                if not torch.allclose(allv[:1], allv):
                    raise ValueError(f'IoU threshold is not equal across all ranks: {allv}')
        self._cache = {}
        self._iou_thresh = v
        for m in self:
            m.iou_thresh = v

    def _all_reduce(self, values, dtype=torch.float32):
        import torch.distributed as dist
        t = torch.tensor(values, dtype=dtype, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    @property
    def length(self):
        n = len(self)
        if not self.distributed:
            return n
        return self._cached('length', lambda: self._all_reduce([n], dtype=torch.int64).item())

    def _avg_x(self, x):
        vals = [getattr(m, x) for m in self]
        s, n = (np.sum(vals), len(vals)) if vals else (0., 0.)
        if not self.distributed:
            return s / n if n != 0 else 0

        def compute():
            ts, tn = self._all_reduce([s, n]).tolist()
            return ts / tn if tn != 0 else 0
        return self._cached(f'_avg_{x}', compute)

    def _sum_x(self, x):
        s = np.sum([getattr(m, x) for m in self])
        if not self.distributed:
            return s
        return self._cached(f'_sum_{x}', lambda: self._all_reduce(s).item())

    def _zero_div(self, name):
        warn(f'ZeroDivisionError in {name} calculation. Assuming 0 as result.')
        return 0

    def _score(self, name, fn):
        try:
            return fn(self.true_positives, self.false_positives, self.false_negatives, self.epsilon)
        except ZeroDivisionError:
            return self._zero_div(name)

    true_positives = property(lambda self: self._sum_x('true_positives'))
    false_positives = property(lambda self: self._sum_x('false_positives'))
    false_negatives = property(lambda self: self._sum_x('false_negatives'))
    avg_f1 = property(lambda self: self._avg_x('f1'), doc='Average F1 score.')
    avg_jaccard = property(lambda self: self._avg_x('jaccard'), doc='Average Jaccard index.')
    avg_fowlkes_mallows = property(lambda self: self._avg_x('fowlkes_mallows'))
    avg_recall = property(lambda self: self._avg_x('recall'), doc='Average recall.')
    avg_precision = property(lambda self: self._avg_x('precision'), doc='Average precision.')
    precision = property(lambda self: self._score('precision', _precision), doc='Precision from the summed counts.')
    recall = property(lambda self: self._score('recall', _recall), doc='Recall from the summed counts.')
    f1_np = property(lambda self: self._score('f1_np', _f1_counts), doc='F1 score from the summed counts.')
    jaccard_np = property(lambda self: self._score('jaccard_np', _jaccard))
    fowlkes_mallows_np = property(lambda self: self._score('fowlkes_mallows_np', _fowlkes_mallows))

    @property
    def f1(self):
        """F1 score from average recall and average precision."""
        rc, pr = self.avg_recall, self.avg_precision
        try:
            return (2 * rc * pr) / (rc + pr + self.epsilon)
        except ZeroDivisionError:
            return self._zero_div('f1')


def _invalidating(name):
    def method(self, *a, **k):
        self.clear_cache()
        return getattr(list, name)(self, *a, **k)
    method.__name__ = name
    return method


for _name in ('append', 'extend', 'insert', 'pop', 'clear', 'copy', '__add__', '__iadd__', '__setitem__', '__delitem__'):
    setattr(LabelMatcherList, _name, _invalidating(_name))
