"""Region property tables of label images on the MI355X: ``labels2property_table`` of the reference's ``cd.data``
(celldetection/data/misc.py:320-347, called from celldetection_scripts/cpn_inference.py:824-837), backed by
``csrc/region_props.hip``.

    labels = cda.contours2labels(y['contours'][0], x.shape[2:])      # int32 [H, W, C]
    cols = cda.region_properties(labels, ('label', 'bbox', 'area', 'centroid', 'orientation'))   # name -> Tensor on the GPU
    table = cda.labels2property_table(labels, 'label', 'area', 'centroid', spacing=(.5, .5))     # pandas.DataFrame

One HIP pass reads the label image (and an integer intensity image) once and accumulates per (channel, label), in integers:
pixel count, bounding box, the sums of r, c, r^2, r * c, c^2 and per intensity channel sum, minimum and maximum.  The rows are
sorted by (channel, label) on the device and a last kernel computes the requested columns in fp64.  Only the row count and
the table status cross to the host.

The reference hands each channel to ``skimage.measure.regionprops_table``.  scikit-image is absent from the build image, so
the property arithmetic is third-party and restated from its documentation, as cv2's fill and dilate are for
``contours2labels`` / ``resolve_label_channels``: the definitions in ``include/cpn_hip.h`` (section "Region property tables")
are this package's contract, ``tests/property_table_oracle.py`` states them in numpy, and the GPU result equals that oracle
exactly in every column made of ``+ - * /`` (1 ulp through ``sqrt``, 8 ulp for ``orientation``).  What the fixture
``tests/golden/property_table.npz`` pins to the reference's own function is the wrapper: channel loop, concatenation, index.

Rows come channel by channel, labels ascending within a channel; a label in two channels has two rows; values <= 0 have none.
Supported are the properties that follow from bounding box, pixel count, first and second moments and intensity sums
(``SUPPORTED``, plus the old scikit-image names in ``ALIASES``); every other name raises ``NotImplementedError``.
"""
from collections import OrderedDict
from ctypes import c_int32, c_int64

import numpy as np
import torch

from . import _lib
from ._label_input import INT32_MAX, aligned16, to_int32, upload_numpy
from ._lib import PROP_CODES, PROP_NAMES, check, ptr, stream_ptr
from ._tables import check_capacity, default_capacity, grow_until_it_fits

__all__ = ['region_properties', 'labels2property_table', 'SUPPORTED', 'ALIASES']

SUPPORTED = PROP_NAMES
ALIASES = dict(bbox_area='area_bbox', equivalent_diameter='equivalent_diameter_area', major_axis_length='axis_major_length',
               minor_axis_length='axis_minor_length', local_centroid='centroid_local', mean_intensity='intensity_mean',
               min_intensity='intensity_min', max_intensity='intensity_max')
MAX_CHANNELS, MAX_INTENSITY_CHANNELS, MAX_SIDE, MAX_PROPERTIES = 11, 4, 65536, 64
_SHAPES = dict(bbox=(4,), centroid=(2,), centroid_local=(2,), inertia_tensor=(2, 2), inertia_tensor_eigvals=(2,))
_INTEGER = ('label', 'bbox', 'num_pixels', 'intensity_min', 'intensity_max')
_INTENSITY = ('intensity_mean', 'intensity_min', 'intensity_max')
_INTENSITY_DTYPES = {torch.uint8: _lib.PROPS_U8, torch.int16: _lib.PROPS_I16, torch.int32: _lib.PROPS_I32}


def _check_integers(x, what):
    """Type and dtype of an image argument, before anything needs a device."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise TypeError(f'region_properties: {what} must be a Tensor on the GPU or a numpy array (got {type(x).__name__})')
    floating = x.dtype.kind not in 'iub' if isinstance(x, np.ndarray) else x.is_floating_point() or x.is_complex()
    if floating:
        raise TypeError(f'region_properties: {what} must hold integers (got {x.dtype}); float images are not supported, '
                        'their sums would depend on the order of the additions')


def _upload(x, what):
    if isinstance(x, np.ndarray):
        x = upload_numpy(x, 'region_properties', f'{what} holds values')
    if not x.is_cuda:
        raise RuntimeError('celldetection_amd.region_properties runs on the MI355X only (got a CPU tensor).')
    return x


def _resolve(properties):
    """-> [(name as requested, canonical name)]; unknown names raise NotImplementedError."""
    if isinstance(properties, str):
        properties = (properties,)
    out = []
    for p in properties:
        canon = ALIASES.get(p, p)
        if canon not in PROP_CODES:
            raise NotImplementedError(f'region_properties: property {p!r} is not implemented on the HIP path; supported: '
                                      f'{", ".join(SUPPORTED)} (and the old names {", ".join(ALIASES)}); perimeter, '
                                      'perimeter_crofton, euler_number, area_convex and solidity come from shape_properties '
                                      'and labels2property_table')
        out.append((p, canon))
    if len(out) > MAX_PROPERTIES:
        raise NotImplementedError(f'region_properties: more than {MAX_PROPERTIES} properties')
    return out


def _column_names(props, sep, K):
    """Column names as regionprops_table writes them, and per column its kind: 'f' float64, 'i' int64, 'v' an intensity
    value (the dtype of the intensity image)."""
    names, kinds = [], []
    for asked, canon in props:
        shape = _SHAPES.get(canon, ())
        if canon in _INTENSITY and K > 1:
            shape = (K,)
        if len(shape) == 0:
            sub = [asked]
        elif len(shape) == 1:
            sub = [f'{asked}{sep}{i}' for i in range(shape[0])]
        else:
            sub = [f'{asked}{sep}{i}{sep}{j}' for i in range(shape[0]) for j in range(shape[1])]
        names += sub
        kinds += ['v' if canon in ('intensity_min', 'intensity_max') else 'i' if canon in _INTEGER else 'f'] * len(sub)
    return names, kinds


def _spacing(spacing):
    if spacing is None:
        return 1., 1.
    if np.isscalar(spacing):
        return float(spacing), float(spacing)
    sy, sx = (float(s) for s in spacing)
    return sy, sx


class _Accumulated:
    """The sorted table of one label image on the device: what the accumulate, status and sort calls leave behind, for the
    finalisation of this module and the shape pass of ``shape_props``."""
    __slots__ = ('x', 'H', 'W', 'C', 'K', 'img_dtype', 'ws', 'cap', 'grown', 'rows')

    def stats(self):
        return dict(table_capacity=self.cap, grown=self.grown, rows=self.rows, channels=self.C)


def _accumulate(labels, intensity_image, iter_channels, table_capacity, intensity_requested=False):
    """Checks the images, uploads them and runs accumulate / table_status / compact_sort -> ``_Accumulated``."""
    x = labels
    _check_integers(x, 'labels')
    if x.ndim == 3 and not iter_channels:
        raise NotImplementedError('region_properties: iter_channels=False on a 3-D image is not implemented (the reference '
                                  'would measure it as a volume)')
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError(f'region_properties: labels must be [H, W] or [H, W, C] (got {tuple(x.shape)})')
    H, W, C = (int(s) for s in x.shape)
    if C < 1:
        raise ValueError('region_properties: labels has no channel')
    if H * W > INT32_MAX or max(H, W) > MAX_SIDE:
        raise NotImplementedError(f'region_properties: images of more than 2 ** 31 - 1 pixels or more than {MAX_SIDE} pixels a '
                                  f'side are not implemented (got {H} x {W})')
    if C > MAX_CHANNELS:
        raise NotImplementedError(f'region_properties: more than {MAX_CHANNELS} label channels')
    x = _upload(x, 'labels')
    K, img, idt, img_dtype = 0, None, 0, None
    if intensity_image is not None:
        _check_integers(intensity_image, 'intensity_image')
        img = _upload(intensity_image, 'intensity_image')
        if img.ndim not in (2, 3) or tuple(img.shape[:2]) != (H, W):
            raise ValueError(f'region_properties: intensity_image must be [{H}, {W}] or [{H}, {W}, K] (got {tuple(img.shape)})')
        K = 1 if img.ndim == 2 else int(img.shape[2])
        if not 1 <= K <= MAX_INTENSITY_CHANNELS:
            raise NotImplementedError(f'region_properties: 1 to {MAX_INTENSITY_CHANNELS} intensity channels are implemented (got {K})')
        if img.device != x.device:
            raise ValueError('region_properties: labels and intensity_image are on different devices')
        img_dtype = img.dtype
        if img.dtype in (torch.int8, torch.bool):
            img = img.to(torch.int16)
        elif img.dtype not in _INTENSITY_DTYPES:  # uint16 (where torch has it), int64, ...
            img = to_int32(img, 'region_properties: intensity_image holds values that do not fit int32')
        idt = _INTENSITY_DTYPES[img.dtype]
        img = img.contiguous()
    elif intensity_requested:
        raise AttributeError('region_properties: an intensity property was requested without an intensity_image')
    x = aligned16(to_int32(x, 'region_properties: labels holds values that do not fit int32'))
    lib = _lib.load()
    cap = default_capacity(H * W, 64) if table_capacity is None else int(table_capacity)
    check_capacity(cap)
    status = (c_int64 * 2)()

    def attempt(cap):
        nbytes = int(lib.cpn_props_workspace_bytes(cap, K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(lib.cpn_props_accumulate(ptr(x), H, W, C, ptr(img), K, idt, cap, ptr(ws), nbytes, stream_ptr()), 'props_accumulate')
        check(lib.cpn_props_table_status(ptr(ws), cap, status, stream_ptr()), 'props_table_status')
        return ws, int(status[0]), int(status[1])

    with torch.cuda.device(x.device):
        ws, cap, grown, n = grow_until_it_fits(cap, attempt)
        check(lib.cpn_props_compact_sort(ptr(ws), cap, K, n, stream_ptr()), 'props_compact_sort')
    acc = _Accumulated()
    acc.x, acc.H, acc.W, acc.C, acc.K, acc.img_dtype, acc.ws, acc.cap, acc.grown, acc.rows = x, H, W, C, K, img_dtype, ws, cap, grown, n
    return acc


def _finalise(acc, props, sy, sx):
    """-> int64 Tensor[columns + 1, rows] on the GPU (last row: channel) for the resolved properties."""
    lib = _lib.load()
    codes = (c_int32 * len(props))(*[PROP_CODES[canon] for _, canon in props])
    ncols = int(lib.cpn_props_columns(codes, len(props), acc.K))
    with torch.cuda.device(acc.x.device):
        out = torch.empty((ncols + 1, acc.rows), dtype=torch.int64, device=acc.x.device)
        check(lib.cpn_props_finalise(ptr(acc.ws), acc.cap, acc.K, acc.rows, codes, len(props), sy, sx, ptr(out), ncols + 1,
                                     stream_ptr()), 'props_finalise')
    return out


def _table(labels, properties, intensity_image, spacing, separator, iter_channels, table_capacity):
    """-> (column names, column kinds, int64 Tensor[columns + 1, rows] on the GPU (last row: channel), intensity dtype, stats)."""
    props = _resolve(properties)
    acc = _accumulate(labels, intensity_image, iter_channels, table_capacity, any(canon in _INTENSITY for _, canon in props))
    sy, sx = _spacing(spacing)
    names, kinds = _column_names(props, separator, acc.K)
    out = _finalise(acc, props, sy, sx)
    assert out.shape[0] == len(names) + 1, (out.shape, names)
    return names, kinds, out, acc.img_dtype, acc.stats()


def _mixed_table(labels, properties, intensity_image, spacing, separator, iter_channels, table_capacity):
    """``_table`` for a property list that names shape properties (``shape_props``) among the others: one accumulate / sort,
    each engine finalises its own columns, and the rows of both results are put in the order asked for on the device."""
    from . import shape_props
    if isinstance(properties, str):
        properties = (properties,)
    owners = [shape_props.shape_only(p) for p in properties]
    rprops = _resolve([p for p, s in zip(properties, owners) if not s])
    sprops = shape_props._resolve([p for p, s in zip(properties, owners) if s])
    sy, sx = _spacing(spacing)
    shape_props._check_spacing(sprops, sy, sx)
    acc = _accumulate(labels, intensity_image, iter_channels, table_capacity, any(canon in _INTENSITY for _, canon in rprops))
    parts = []
    if rprops:
        parts.append(_finalise(acc, rprops, sy, sx)[:-1])
    sout, _ = shape_props._finalise(acc, sprops, sy, sx)
    parts.append(sout)  # its last row is the channel
    names, kinds, order = [], [], []
    r_at, s_at = 0, (parts[0].shape[0] if rprops else 0)
    r_it, s_it = iter(rprops), iter(sprops)
    for shape in owners:
        if shape:
            nm, kd = shape_props._column_names([next(s_it)])
            at, s_at = s_at, s_at + len(nm)
        else:
            nm, kd = _column_names([next(r_it)], separator, acc.K)
            at, r_at = r_at, r_at + len(nm)
        names += nm
        kinds += kd
        order += list(range(at, at + len(nm)))
    out = torch.cat(parts)
    order.append(out.shape[0] - 1)
    out = out[torch.tensor(order, dtype=torch.int64, device=out.device)]
    return names, kinds, out, acc.img_dtype, acc.stats()


def region_properties(labels, properties=('label', 'bbox'), intensity_image=None, spacing=None, separator='-', iter_channels=True,
                      table_capacity=None, return_stats=False):
    """Label image Tensor[H, W] or [H, W, C] (integers, on the GPU) -> ``OrderedDict`` column name -> 1-D Tensor on the GPU,
    one entry per object: channel by channel, labels ascending within a channel.

    properties: names of ``SUPPORTED`` or ``ALIASES`` (the column carries the name asked for); columns are named as
    ``skimage.measure.regionprops_table`` names them (``bbox-0``, ``inertia_tensor-0-1``, with ``separator``) and come in the
    order asked for.  Integer columns are int64 (``intensity_min`` / ``intensity_max``: the dtype of the intensity image), the
    others float64.
    intensity_image: integer Tensor[H, W] or [H, W, K <= 4] on the GPU; with K > 1 the intensity columns get ``{separator}k``.
    spacing: pixel spacing ``(row, column)`` or one number for both.
    iter_channels: ``False`` is accepted for 2-D images only.
    table_capacity: first size of the hash table (a power of two; it is doubled until every key found a slot).
    return_stats: additionally ``dict(table_capacity, grown, rows, channels)``."""
    names, kinds, out, img_dtype, stats = _table(labels, properties, intensity_image, spacing, separator, iter_channels,
                                                   table_capacity)
    cols = OrderedDict()
    for i, (name, kind) in enumerate(zip(names, kinds)):
        col = out[i]
        if kind == 'f':
            col = col.view(torch.float64)
        elif kind == 'v':
            col = col.to(img_dtype)
        cols[name] = col
    if return_stats:
        return cols, stats
    return cols


def labels2property_table(labels, *properties, iter_channels=True, **kwargs):
    """The reference's ``labels2property_table`` (data/misc.py:320-347) on the GPU: label image [H, W(, C)] ->
    ``pandas.DataFrame`` with one row per object and one column per property component, built from ONE device-to-host copy.

    *properties: property names, or a single list / tuple of them (default: ``('label', 'bbox')`` as ``regionprops_table``).
    The names of ``shape_props.SUPPORTED`` (``perimeter``, ``perimeter_crofton``, ``euler_number``, ``area_convex``,
    ``solidity``; ``convex_area``) may be mixed with those of ``SUPPORTED``: the image is accumulated and sorted once.
    **kwargs: ``intensity_image``, ``spacing``, ``separator`` as ``region_properties``; ``df_kwargs``: keyword arguments of
    every per-channel ``pandas.DataFrame``; ``table_capacity``.  The index is the one the reference's per-channel ``pd.concat``
    produces: it restarts at 0 in every channel."""
    try:
        import pandas as pd
    except ImportError as e:
        raise ImportError('celldetection_amd.labels2property_table needs pandas for its DataFrame; '
                          'celldetection_amd.region_properties returns the same columns as GPU tensors without it') from e
    if len(properties) == 1 and isinstance(properties[0], (list, tuple)):
        properties, = properties
    if len(properties) == 0:
        properties = ('label', 'bbox')
    df_kwargs = kwargs.pop('df_kwargs', {})
    kwargs.pop('cache', None)
    if kwargs.pop('extra_properties', None) is not None:
        raise NotImplementedError('labels2property_table: extra_properties are not implemented on the HIP path')
    unknown = set(kwargs) - {'intensity_image', 'spacing', 'separator', 'table_capacity'}
    if unknown:
        raise TypeError(f'labels2property_table: unexpected keyword arguments {sorted(unknown)}')
    sep = kwargs.get('separator', '-')
    from . import shape_props
    if any(shape_props.shape_only(p) for p in properties):
        names, kinds, out, img_dtype, stats = _mixed_table(labels, properties, kwargs.get('intensity_image'), kwargs.get('spacing'),
                                                             sep, iter_channels, kwargs.get('table_capacity'))
    else:
        names, kinds, out, img_dtype, stats = _table(labels, properties, kwargs.get('intensity_image'), kwargs.get('spacing'), sep,
                                                       iter_channels, kwargs.get('table_capacity'))
    host = out.cpu().numpy()  # the one copy
    channel = host[-1]
    np_dtype = None if img_dtype is None else torch.empty(0, dtype=img_dtype).numpy().dtype
    cols = []
    for i, (name, kind) in enumerate(zip(names, kinds)):
        col = host[i]
        if kind == 'f':
            col = col.view(np.float64)
        elif kind == 'v':
            col = col.astype(np_dtype)
        cols.append(col)
    bounds = np.searchsorted(channel, np.arange(stats['channels'] + 1))
    tab = None
    for z in range(stats['channels'] if iter_channels else 1):
        part = OrderedDict((name, col[bounds[z]:bounds[z + 1]]) for name, col in zip(names, cols))
        tab = pd.concat((tab, pd.DataFrame(part, **df_kwargs)))
    return tab
