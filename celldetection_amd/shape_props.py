"""Shape properties of label images on the MI355X: ``perimeter``, ``perimeter_crofton``, ``euler_number``, ``area_convex`` and
``solidity`` of ``skimage.measure.regionprops_table`` (the reference documents its property table with ``-p 'area'
'perimeter'``, docs/source/inference.rst), backed by ``csrc/shape_props.hip`` and ``csrc/hull_count.h``.

    cols = cda.shape_properties(labels, ('label', 'perimeter', 'euler_number', 'solidity'))         # name -> Tensor on the GPU
    table = cda.labels2property_table(labels, 'label', 'area', 'perimeter', 'solidity')           # mixed with region_props

The pass runs after the accumulate / sort of ``region_props`` on the same image: it looks the slot of every key up and adds
integer counts to a workspace of its own.  One more streaming read of the label image serves every requested shape property:
per pixel the perimeter class (a 5 x 5 dependency), four Crofton transitions, the bit-quad term of its 2 x 2 window, and for
the hull the ends of row runs.  The hull of an object is then counted by one lane from the column extents of its rows, in
integers.  Only the row count and the total of the box heights cross to the host.

scikit-image is absent from the build image, so the arithmetic is third-party and restated, unpinned: the definitions in
``include/cpn_hip.h`` (section "Shape property tables") are this package's contract, ``tests/shape_props_oracle.py`` states
them in numpy, and the GPU result equals that oracle exactly, float columns bit for bit.

Rows are those of ``region_properties``.  The predicate of every property is *same label*: a neighbouring pixel of another
label counts as outside, as cropping to the bounding box does.  ``perimeter`` / ``perimeter_crofton`` take isotropic spacings
only.  Not implemented anywhere: ``feret_diameter_max``, ``area_filled``, ``moments*``, ``image*``, ``coords``.
"""
from collections import OrderedDict
from ctypes import c_int32

import torch

from . import _lib, region_props
from ._lib import SHAPE_CODES, SHAPE_NAMES, check, ptr, stream_ptr

__all__ = ['shape_properties', 'SUPPORTED', 'ALIASES']

SUPPORTED = SHAPE_NAMES
ALIASES = dict(convex_area='area_convex')
MAX_PROPERTIES = 64
_INTEGER = ('label', 'num_pixels', 'euler_number')
_LENGTHS = ('perimeter', 'perimeter_crofton')
_HULL = ('area_convex', 'solidity')


def shape_only(name):
    """Whether ``name`` is a property that only this module computes (``label`` and ``num_pixels`` are region_props' too)."""
    return ALIASES.get(name, name) in SUPPORTED[2:]


def _resolve(properties):
    """-> [(name as requested, canonical name)]; unknown names raise NotImplementedError."""
    if isinstance(properties, str):
        properties = (properties,)
    out = []
    for p in properties:
        canon = ALIASES.get(p, p)
        if canon not in SHAPE_CODES:
            raise NotImplementedError(f'shape_properties: property {p!r} is not implemented on the HIP path; supported: '
                                      f'{", ".join(SUPPORTED)} (and the old name {", ".join(ALIASES)}); region_properties has '
                                      f'{", ".join(region_props.SUPPORTED[3:])}')
        out.append((p, canon))
    if len(out) > MAX_PROPERTIES:
        raise NotImplementedError(f'shape_properties: more than {MAX_PROPERTIES} properties')
    return out


def _check_spacing(props, sy, sx):
    if sy != sx and any(canon in _LENGTHS for _, canon in props):
        raise NotImplementedError(f'shape_properties: perimeter and perimeter_crofton support isotropic spacings only (got {(sy, sx)})')


def _column_names(props):
    return [asked for asked, _ in props], ['i' if canon in _INTEGER else 'f' for _, canon in props]


def _finalise(acc, props, sy, sx, timings=None):
    """Shape pass, hull pass and finalisation on an accumulated table (``region_props._accumulate``) -> (int64
    Tensor[columns + 1, rows] on the GPU (last row: channel), total of the box heights or 0 without a hull property)."""
    lib = _lib.load()
    dev, n = acc.x.device, acc.rows
    codes = (c_int32 * len(props))(*[SHAPE_CODES[canon] for _, canon in props])
    ncols = int(lib.cpn_shape_columns(codes, len(props)))
    assert ncols == len(props), ncols
    hull = any(canon in _HULL for _, canon in props)
    total, row_begin, extents, counts = 0, None, None, None
    with torch.cuda.device(dev):
        if hull and n > 0:
            heights = torch.empty(n, dtype=torch.int64, device=dev)
            check(lib.cpn_shape_heights(ptr(acc.ws), acc.cap, acc.K, n, ptr(heights), stream_ptr()), 'shape_heights')
            row_begin = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            row_begin[1:] = torch.cumsum(heights, 0)  # the exclusive scan, with the total at the end
            total = int(row_begin[-1])  # to the host once, for the allocation
            extents = torch.empty(2 * total, dtype=torch.int32, device=dev)
        nbytes = int(lib.cpn_shape_workspace_bytes(acc.cap))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mark = (lambda: None) if timings is None else (lambda: timings.append(_event()))
        mark()
        check(lib.cpn_shape_accumulate(ptr(acc.x), acc.H, acc.W, acc.C, ptr(acc.ws), acc.cap, acc.K, n, ptr(ws), nbytes, ptr(row_begin),
                                       ptr(extents), total, stream_ptr()), 'shape_accumulate')
        mark()
        if hull and n > 0:
            sbytes = int(lib.cpn_shape_hull_scratch_bytes(n, total))
            scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
            counts = torch.empty(n, dtype=torch.int64, device=dev)
            check(lib.cpn_shape_hull(n, ptr(row_begin), ptr(extents), total, ptr(scratch), sbytes, ptr(counts), stream_ptr()), 'shape_hull')
        mark()
        out = torch.empty((ncols + 1, n), dtype=torch.int64, device=dev)
        check(lib.cpn_shape_finalise(ptr(acc.ws), acc.cap, acc.K, n, ptr(ws), ptr(counts), codes, len(props), sy, sx, ptr(out), ncols + 1,
                                     stream_ptr()), 'shape_finalise')
    return out, total


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def shape_properties(labels, properties=('label', 'perimeter'), spacing=None, separator='-', table_capacity=None, return_stats=False):
    """Label image Tensor[H, W] or [H, W, C] (integers, on the GPU) -> ``OrderedDict`` column name -> 1-D Tensor on the GPU, one
    entry per object, in the rows of ``region_properties``: channel by channel, labels ascending within a channel.

    properties: names of ``SUPPORTED`` or ``ALIASES`` (the column carries the name asked for).  ``label``, ``num_pixels`` and
    ``euler_number`` are int64, the others float64.  ``label`` and ``num_pixels`` are there so that a result can be joined.
    spacing: pixel spacing ``(row, column)`` or one number for both; ``perimeter`` and ``perimeter_crofton`` need both equal.
    separator: accepted for symmetry with ``region_properties`` (every shape property is one column).
    table_capacity: first size of the hash table (a power of two; it is doubled until every key found a slot).
    return_stats: additionally ``dict(table_capacity, grown, rows, channels, hull_rows)``."""
    props = _resolve(properties)
    sy, sx = region_props._spacing(spacing)
    _check_spacing(props, sy, sx)
    acc = region_props._accumulate(labels, None, True, table_capacity)
    out, total = _finalise(acc, props, sy, sx)
    names, kinds = _column_names(props)
    cols = OrderedDict()
    for i, (name, kind) in enumerate(zip(names, kinds)):
        cols[name] = out[i].view(torch.float64) if kind == 'f' else out[i]
    if return_stats:
        return cols, dict(acc.stats(), hull_rows=total)
    return cols
