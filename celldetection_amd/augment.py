"""Training augmentation on the MI355X: the joint affine warp of a batch of images and their label stacks, backed by
``csrc/augment.hip``.  It stands for the albumentations pipeline of the reference's training recipe (``conf2augmentation`` and the
demos: Transpose, RandomRotate90, rotations and scalings, random crops, RandomGamma / RandomBrightnessContrast, normalisation), which
runs on a CPU worker there.  albumentations and ``cv2.warpAffine`` are third-party, unpinned and absent here; the rule is stated
once, in the "Augmentation warp" section of ``include/cpn_hip.h`` (numpy statement: ``tests/augment_oracle.py``), and anchored to
torch's float64 CPU ``grid_sample(align_corners=True)``.

    aug = cda.augment.RandomAffine((512, 512), angle=(-180, 180), scale=(.8, 1.25), gamma=(.7, 1.4), mean=.5, std=.25)
    inputs, lab = aug(images, labels)        # uint8 [B, H, W, K], int [B, H, W, C]  ->  float32 [B, K, h, w], int32 [B, h, w, C]
    for b in range(B):
        cda.relabel_(lab[b])                 # in place on the view
        gens[b].feed(lab[b])

A nearest-sampled rotation can split a thin object, and a reflecting border duplicates objects: ``relabel_`` is what makes "one
object = one component" true again, so it belongs between the warp and ``CPNTargetGenerator.feed``.

One kernel launch per call: bilinear interpolation of the image with the intensity transform folded in (a 256-entry table per
sample and channel for ``uint8``, scale and offset for ``float32``), nearest sampling of the labels in integers (no label passes
through a float), one border mode for both.  The dihedral maps and integer crops reproduce ``rot90`` / ``flip`` / ``transpose`` /
slicing bit for bit.

Known limits: no anti-aliasing when scaling down; affine maps only (no optical or elastic distortion, no blur, no noise);
table-then-blend (albumentations blends the uint8 image, rounds and then applies its tables); all samples of a call share the source
size.
"""
import math

import numpy as np
import torch

from . import _lib
from ._label_input import to_int32
from ._lib import check, ptr, stream_ptr
from .components import MAX_CHANNELS

__all__ = ['warp', 'affine_map', 'crop_map', 'intensity_table', 'intensity_scale_offset', 'RandomAffine']

BORDERS = {'constant': _lib.AUGMENT_BORDER_CONSTANT, 'reflect': _lib.AUGMENT_BORDER_REFLECT}
MAX_IMAGE_CHANNELS = 4
FAR = 2. ** 30  # a map that sends a destination corner further than this from the origin is refused
DRAWS = ('rot90', 'transpose', 'flip_h', 'flip_v', 'angle', 'scale', 'shear', 'translate_x', 'translate_y', 'gamma', 'contrast',
         'brightness')  # the uniform numbers of one sample, in the order they are drawn


def _dihedral_inverse(rot90, transpose, flip_h, flip_v):
    """2 x 2 integer matrix that takes centred destination (x, y) to centred source (x, y) for
    ``flip_v(flip_h(rot90^k(transpose(source))))`` in numpy's sense (``np.rot90`` turns counter-clockwise)."""
    a = np.eye(2)
    if transpose:
        a = a @ np.array([[0., 1.], [1., 0.]])
    for _ in range(int(rot90) % 4):
        a = a @ np.array([[0., -1.], [1., 0.]])
    if flip_h:
        a = a @ np.array([[-1., 0.], [0., 1.]])
    if flip_v:
        a = a @ np.array([[1., 0.], [0., -1.]])
    return a


def affine_map(src_size, dst_size, rot90=0, transpose=False, flip_h=False, flip_v=False, angle=0., scale=1., shear=0.,
               translate=(0., 0.)):
    """-> float64[6], the map ``warp`` takes (destination pixel -> source position): the inverse of

        D (dihedral) -> scale -> shear -> rotate by ``angle`` about the source centre ((W - 1) / 2, (H - 1) / 2),
        onto the destination centre ((w - 1) / 2, (h - 1) / 2), plus ``translate`` = (tx, ty) in destination pixels.

    D is ``flip_v(flip_h(np.rot90(transpose(source), rot90)))``: the transpose first, then ``rot90`` quarter turns counter-clockwise,
    then the flips, with exact integer sines and cosines.  ``angle`` (degrees) turns counter-clockwise as displayed, ``shear``
    (degrees) moves x by tan(shear) * y, ``scale`` > 1 magnifies.  With ``angle = shear = 0``, ``scale = 1`` and matching sizes every
    entry is an exact integer.  ``src_size = (H, W)``, ``dst_size = (h, w)``."""
    (H, W), (h, w) = (int(s) for s in src_size), (int(s) for s in dst_size)
    if min(H, W, h, w) < 1:
        raise ValueError(f'affine_map: src_size and dst_size must be positive (got {tuple(src_size)}, {tuple(dst_size)})')
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f'affine_map: scale must be positive and finite (got {scale!r})')
    tx, ty = (float(t) for t in translate)
    a = _dihedral_inverse(rot90, transpose, flip_h, flip_v)
    if scale != 1.:
        a = a @ np.array([[1. / scale, 0.], [0., 1. / scale]])
    if shear != 0.:
        a = a @ np.array([[1., -math.tan(math.radians(float(shear)))], [0., 1.]])
    if angle != 0.:
        c, s = math.cos(math.radians(float(angle))), math.sin(math.radians(float(angle)))
        a = a @ np.array([[c, -s], [s, c]])  # the inverse of (x, y) -> (c x + s y, -s x + c y): counter-clockwise with y down
    d = np.array([(w - 1) / 2. + tx, (h - 1) / 2. + ty])
    o = np.array([(W - 1) / 2., (H - 1) / 2.]) - a @ d
    return np.array([a[0, 0], a[0, 1], o[0], a[1, 0], a[1, 1], o[1]], dtype=np.float64) + 0.  # (+ 0.: no negative zeros)


def crop_map(y, x):
    """-> float64[6]: destination (i, j) reads source (y + i, x + j): the slices of the reference's ``random_crop``."""
    return np.array([1., 0., float(x), 0., 1., float(y)], dtype=np.float64)


def _per_channel(value, K, name, who):
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    if v.size not in (1, K) or not np.all(np.isfinite(v)):
        raise ValueError(f'{who}: {name} must be one finite number or {K} of them (got {value!r})')
    return np.broadcast_to(v, (K,))


def intensity_table(K, gamma=1., contrast=1., brightness=0., scale=1 / 255, mean=0., std=1.):
    """-> float32[K, 256], the tables ``warp`` applies to the taps of a ``uint8`` image.  Entry i of a channel, in float64 and rounded
    once: ``v = i``; ``gamma != 1``: ``v = (i / 255) ** gamma * 255``, the expression of ``preprocess``
    (``np.arange(0, 256. / 255, 1. / 255) ** gamma * 255``); ``v = clip(v * contrast + 255 * brightness, 0, 255)`` (albumentations'
    ``brightness_contrast_adjust`` with ``beta_by_max``); then ``(v * scale - mean) / std``.  Nothing is truncated to uint8 in
    between.  Every argument is one number or one per channel."""
    K = int(K)
    if not 1 <= K <= MAX_IMAGE_CHANNELS:
        raise ValueError(f'intensity_table: K must be 1 ... {MAX_IMAGE_CHANNELS} (got {K})')
    who = 'intensity_table'
    gamma, contrast, brightness = (_per_channel(v, K, n, who) for v, n in ((gamma, 'gamma'), (contrast, 'contrast'),
                                                                            (brightness, 'brightness')))
    scale, mean, std = (_per_channel(v, K, n, who) for v, n in ((scale, 'scale'), (mean, 'mean'), (std, 'std')))
    if np.any(gamma <= 0) or np.any(std == 0):
        raise ValueError('intensity_table: gamma must be positive and std non-zero')
    out = np.empty((K, 256), dtype=np.float32)
    for k in range(K):
        v = np.arange(256, dtype=np.float64)
        if gamma[k] != 1.:
            v = np.arange(0, 256. / 255, 1. / 255) ** gamma[k] * 255
        if contrast[k] != 1. or brightness[k] != 0.:
            v = np.clip(v * contrast[k] + 255. * brightness[k], 0., 255.)
        out[k] = (v * scale[k] - mean[k]) / std[k]
    return out


def intensity_scale_offset(K, contrast=1., brightness=0., scale=1., mean=0., std=1.):
    """-> float32[K, 2], the (scale, offset) pairs ``warp`` applies to the taps of a ``float32`` image: ``t = v * s + o`` with
    ``s = contrast * scale / std`` and ``o = (brightness * scale - mean) / std``, i.e. ``((v * contrast + brightness) * scale - mean) /
    std`` without the clip, computed in float64 and rounded once."""
    K = int(K)
    if not 1 <= K <= MAX_IMAGE_CHANNELS:
        raise ValueError(f'intensity_scale_offset: K must be 1 ... {MAX_IMAGE_CHANNELS} (got {K})')
    who = 'intensity_scale_offset'
    contrast, brightness, scale, mean, std = (_per_channel(v, K, n, who) for v, n in (
        (contrast, 'contrast'), (brightness, 'brightness'), (scale, 'scale'), (mean, 'mean'), (std, 'std')))
    if np.any(std == 0):
        raise ValueError('intensity_scale_offset: std must be non-zero')
    return np.stack([contrast * scale / std, (brightness * scale - mean) / std], axis=1).astype(np.float32)


def _check_maps(maps, B, h, w):
    if isinstance(maps, torch.Tensor):
        if maps.is_cuda:
            raise ValueError('warp: maps must be a CPU tensor or array (it is uploaded once per call)')
        maps = maps.detach().numpy()
    maps = np.asarray(maps)
    if maps.dtype != np.float64:
        raise TypeError(f'warp: maps must be float64 (got {maps.dtype})')
    if maps.shape == (6,):
        maps = np.broadcast_to(maps, (B, 6))
    if maps.shape != (B, 6):
        raise ValueError(f'warp: maps must be [{B}, 6] or [6] (got {tuple(maps.shape)})')
    if not np.all(np.isfinite(maps)):
        raise ValueError('warp: maps holds a non-finite entry')
    j, i = np.array([0., w - 1., 0., w - 1.]), np.array([0., 0., h - 1., h - 1.])
    with np.errstate(over='ignore', invalid='ignore'):
        sx = maps[:, 0:1] * j + maps[:, 1:2] * i + maps[:, 2:3]
        sy = maps[:, 3:4] * j + maps[:, 4:5] * i + maps[:, 5:6]
    if not (np.all(np.abs(sx) <= FAR) and np.all(np.abs(sy) <= FAR)):  # (an overflow to inf fails it too)
        raise ValueError('warp: maps sends a destination corner further than 2 ** 30 from the origin')
    return np.ascontiguousarray(maps)


def _check_tables(tables, B, K, u8):
    n = 256 if u8 else 2
    if tables is None:  # the identity: T[v] = v, or scale 1 and offset 0
        tables = np.arange(256, dtype=np.float32) if u8 else np.array([1., 0.], dtype=np.float32)
        return np.ascontiguousarray(np.broadcast_to(tables, (B, K, n)))
    if isinstance(tables, torch.Tensor):
        if tables.is_cuda:
            raise ValueError('warp: tables must be a CPU tensor or array (it is uploaded once per call, with maps)')
        tables = tables.detach().numpy()
    tables = np.asarray(tables)
    if tables.dtype != np.float32:
        raise TypeError(f'warp: tables must be float32 (got {tables.dtype})')
    if tables.shape == (K, n):
        tables = np.broadcast_to(tables, (B, K, n))
    if tables.shape != (B, K, n):
        raise ValueError(f'warp: tables must be [{B}, {K}, {n}] or [{K}, {n}] for {"uint8" if u8 else "float32"} images '
                         f'(got {tuple(tables.shape)})')
    if not np.all(np.isfinite(tables)):
        raise ValueError('warp: tables holds a non-finite entry')
    return np.ascontiguousarray(tables)


def warp(image, labels, maps, size, tables=None, border='constant', image_fill=0., label_fill=0, out_dtype=torch.float32):
    """Warps images and label stacks together, every sample by its own map -> ``(inputs, labels)`` on the GPU.

    image: Tensor[B, H, W, K] or [H, W, K] / [H, W], ``uint8`` or ``float32``, on the GPU (channels-last, K <= 4), or None.
    labels: Tensor[B, H, W, C] or [H, W, C] / [H, W] of integers on the same GPU (values must fit int32), or None.
    maps: float64 [B, 6] or [6] (shared), a CPU tensor or array: ``affine_map`` / ``crop_map``; destination pixel -> source position.
    size: (h, w) of the output.
    tables: None (the identity), or float32 [B, K, 256] / [K, 256] for ``uint8`` images (``intensity_table``) and [B, K, 2] / [K, 2]
    (scale, offset) for ``float32`` images (``intensity_scale_offset``); CPU.
    border: 'constant' (``image_fill``, in the output's units, and ``label_fill``; a pixel all of whose four taps lie outside is
    exactly ``image_fill``) or 'reflect' (reflect-101), for both.
    Returns inputs ``out_dtype`` (float32 or bfloat16) [B, K, h, w] and labels int32 [B, h, w, C]; None for a part that was not
    given; unbatched arguments come back unbatched ([K, h, w]; [h, w, C], or [h, w] for [H, W] labels).  Inputs are not changed.
    The rule is the "Augmentation warp" section of include/cpn_hip.h; results are bit-identical from run to run."""
    if image is None and labels is None:
        raise ValueError('warp: image and labels are both None')
    for name, t in (('image', image), ('labels', labels)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f'warp: {name} must be a Tensor on the GPU or None (got {type(t).__name__})')
    if border not in BORDERS:
        raise ValueError(f"warp: border must be 'constant' or 'reflect' (got {border!r})")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f'warp: out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})')
    try:
        h, w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f'warp: size must be (h, w) (got {size!r})') from None
    if h < 1 or w < 1:
        raise ValueError(f'warp: size must be positive (got {size!r})')
    if isinstance(label_fill, bool) or int(label_fill) != label_fill or not -2 ** 31 <= int(label_fill) <= 2 ** 31 - 1:
        raise ValueError(f'warp: label_fill must be an int32 value (got {label_fill!r})')
    with np.errstate(over='ignore'):
        image_fill = float(np.float32(image_fill))
    if not math.isfinite(image_fill):
        raise ValueError('warp: image_fill must be a finite float32')
    batched, x, y, flat_labels = None, None, None, False
    if image is not None:
        if image.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f'warp: image must be uint8 or float32 (got {image.dtype})')
        if image.ndim not in (2, 3, 4):
            raise ValueError(f'warp: image must be [B, H, W, K], [H, W, K] or [H, W] (got {tuple(image.shape)})')
        batched = image.ndim == 4
        x = image if batched else (image[None, :, :, None] if image.ndim == 2 else image[None])
        if not 1 <= x.shape[3] <= MAX_IMAGE_CHANNELS:
            raise NotImplementedError(f'warp: image must have 1 ... {MAX_IMAGE_CHANNELS} channels, channels-last '
                                      f'(got {tuple(image.shape)})')
    if labels is not None:
        if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
            raise TypeError(f'warp: labels must hold integers (got {labels.dtype})')
        if labels.ndim not in (2, 3, 4):
            raise ValueError(f'warp: labels must be [B, H, W, C], [H, W, C] or [H, W] (got {tuple(labels.shape)})')
        if batched is not None and batched != (labels.ndim == 4):
            raise ValueError(f'warp: image and labels must both be batched or both not (got {tuple(image.shape)} and '
                             f'{tuple(labels.shape)})')
        batched, flat_labels = labels.ndim == 4, labels.ndim == 2
        y = labels if batched else (labels[None, :, :, None] if labels.ndim == 2 else labels[None])
        if y.shape[3] < 1:
            raise ValueError('warp: labels has no channel')
        if y.shape[3] > MAX_CHANNELS:
            raise NotImplementedError(f'warp: more than {MAX_CHANNELS} label channels')
        if x is not None and (tuple(y.shape[:3]) != tuple(x.shape[:3]) or y.device != x.device):
            raise ValueError(f'warp: image and labels must share batch, height, width and device (got {tuple(image.shape)} on '
                             f'{image.device} and {tuple(labels.shape)} on {labels.device})')
    first = x if x is not None else y
    B, H, W = (int(s) for s in first.shape[:3])
    if min(B, H, W) < 1:
        raise ValueError(f'warp: empty input {tuple(first.shape)}')
    if H * W >= 2 ** 31 or h * w >= 2 ** 31 or B > 65535:
        raise NotImplementedError('warp: 2 ** 31 or more pixels in a source or a destination, or more than 65535 samples')
    K, C = (int(x.shape[3]) if x is not None else 0), (int(y.shape[3]) if y is not None else 0)
    maps = _check_maps(maps, B, h, w)
    u8 = x is not None and x.dtype == torch.uint8
    host = maps.view(np.uint8).reshape(-1)
    if x is not None:
        host = np.concatenate([host, _check_tables(tables, B, K, u8).view(np.uint8).reshape(-1)])
    elif tables is not None:
        raise ValueError('warp: tables without an image')
    if y is not None:
        y = to_int32(y, 'warp: labels holds values that do not fit int32')
    if not first.is_cuda:
        raise RuntimeError('celldetection_amd.augment.warp runs on the MI355X only (got a CPU tensor).')
    if x is not None:
        x = x.contiguous()
    lib = _lib.load()
    with torch.cuda.device(first.device):
        dev = torch.from_numpy(host).to(first.device)  # maps and tables: one upload
        out = torch.empty((B, K, h, w), dtype=out_dtype, device=first.device) if x is not None else None
        lab = torch.empty((B, h, w, C), dtype=torch.int32, device=first.device) if y is not None else None
        check(lib.cpn_augment_warp(ptr(x), _lib.AUGMENT_IMAGE_U8 if u8 else _lib.AUGMENT_IMAGE_F32, ptr(y), B, H, W, K, C, ptr(dev),
                                   ptr(dev[B * 48:]) if x is not None else None, BORDERS[border], image_fill, int(label_fill), ptr(out),
                                   _lib.CONV_TRAIN_BF16 if out_dtype == torch.bfloat16 else _lib.CONV_TRAIN_F32, ptr(lab), h, w,
                                   stream_ptr()), 'augment_warp')
    if not batched:
        out = out[0] if out is not None else None
        lab = (lab[0, :, :, 0] if flat_labels else lab[0]) if lab is not None else None
    return out, lab


def _range(value, name, positive=False):
    """None or one number -> no draw (lo = hi); (lo, hi) -> the range."""
    if value is None:
        return None
    lo, hi = (float(value), float(value)) if isinstance(value, (int, float)) else (float(v) for v in value)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi) or (positive and lo <= 0):
        raise ValueError(f'RandomAffine: {name} must be a finite range (lo, hi) with lo <= hi{" and lo > 0" if positive else ""} '
                         f'(got {value!r})')
    return lo, hi


class RandomAffine:
    """Random dihedral + affine + intensity augmentation of a batch, one ``warp`` call.

        aug = RandomAffine((h, w), angle=(-180, 180), scale=(.8, 1.25), gamma=(.7, 1.4))
        inputs, labels = aug(image, labels, generator=None)

    size: (h, w) of the output: a crop (or a padded frame) about the centre of the transformed source, shifted by ``translate``.
    rot90 / transpose / flip: draw the dihedral part (quarter turns, a transpose, both flips).
    angle, shear: ranges in degrees; scale: a positive range, drawn log-uniformly; translate: (tx, ty), the largest shift in
    destination pixels; the drawn shift is uniform in [-tx, tx] x [-ty, ty] and rounded to whole pixels, so that a pure crop stays
    exact.  gamma, contrast: positive ranges (``uint8`` images only for gamma); brightness: a range, as a fraction of 255 for
    ``uint8`` and in the image's units for ``float32``; None: not applied.  mean, std: the normalisation (of the image scaled to
    [0, 1] for ``uint8``), one number or one per channel.

    Draw order.  The parameters come from a CPU ``torch.Generator`` (``generator=None``: the default one, so ``torch.manual_seed``
    makes a run reproducible) in ONE call ``torch.rand(B, 12, dtype=torch.float64)``: row b belongs to sample b and its columns
    are, in this order, ``DRAWS`` = rot90, transpose, flip_h, flip_v, angle, scale, shear, translate_x, translate_y, gamma,
    contrast, brightness.  A column is drawn whether or not its part is enabled.  With u the number: rot90 = floor(4 u);
    transpose, flip_h, flip_v = (u < 0.5); a range gives lo + u (hi - lo), scale exp(log lo + u (log hi - log lo)), a shift
    round((2 u - 1) t).

    ``last_params`` holds what the last call drew: a dict of arrays [B] under the names of ``DRAWS`` (``translate`` [B, 2] in place
    of its two columns), ``uniform`` [B, 12], ``maps`` [B, 6] and ``tables``: enough to replay a sample with ``warp`` or to map its
    contours."""

    def __init__(self, size, rot90=True, transpose=True, flip=True, angle=(0, 0), scale=(1, 1), shear=(0, 0), translate=(0, 0),
                 gamma=None, contrast=None, brightness=None, mean=0., std=1., border='constant', label_fill=0,
                 out_dtype=torch.float32):
        try:
            self.size = tuple(int(s) for s in size)
            assert len(self.size) == 2 and min(self.size) >= 1
        except (TypeError, ValueError, AssertionError):
            raise ValueError(f'RandomAffine: size must be (h, w), positive (got {size!r})') from None
        self.rot90, self.transpose, self.flip = bool(rot90), bool(transpose), bool(flip)
        self.angle, self.shear = _range(angle, 'angle'), _range(shear, 'shear')
        self.scale = _range(scale, 'scale', positive=True)
        self.translate = _range((-abs(float(translate[0])), abs(float(translate[0]))), 'translate'), \
            _range((-abs(float(translate[1])), abs(float(translate[1]))), 'translate')
        self.gamma, self.contrast = _range(gamma, 'gamma', positive=True), _range(contrast, 'contrast', positive=True)
        self.brightness = _range(brightness, 'brightness')
        if border not in BORDERS:
            raise ValueError(f"RandomAffine: border must be 'constant' or 'reflect' (got {border!r})")
        self.mean, self.std, self.border, self.label_fill, self.out_dtype = mean, std, border, label_fill, out_dtype
        self.last_params = None

    def draw(self, B, src_size, K=0, u8=True, generator=None):
        """Draws the parameters of ``B`` samples of source size ``src_size`` and ``K`` image channels -> the ``last_params`` dict."""
        u = torch.rand(int(B), len(DRAWS), dtype=torch.float64, generator=generator).numpy()
        col = {name: u[:, n] for n, name in enumerate(DRAWS)}

        def lin(r, name, neutral):
            return np.full(B, neutral) if r is None else r[0] + col[name] * (r[1] - r[0])

        p = dict(uniform=u)
        p['rot90'] = np.floor(4 * col['rot90']).astype(np.int64) if self.rot90 else np.zeros(B, np.int64)
        p['transpose'] = (col['transpose'] < .5) & self.transpose
        p['flip_h'], p['flip_v'] = (col['flip_h'] < .5) & self.flip, (col['flip_v'] < .5) & self.flip
        p['angle'], p['shear'] = lin(self.angle, 'angle', 0.), lin(self.shear, 'shear', 0.)
        p['scale'] = np.exp(lin(tuple(math.log(s) for s in self.scale), 'scale', 0.))
        if self.scale[0] == self.scale[1]:
            p['scale'] = np.full(B, self.scale[0])  # (exp(log s) need not be s)
        p['translate'] = np.stack([np.round(lin(self.translate[0], 'translate_x', 0.)),
                                   np.round(lin(self.translate[1], 'translate_y', 0.))], axis=1) + 0.
        p['gamma'], p['contrast'] = lin(self.gamma, 'gamma', 1.), lin(self.contrast, 'contrast', 1.)
        p['brightness'] = lin(self.brightness, 'brightness', 0.)
        p['maps'] = np.stack([affine_map(src_size, self.size, int(p['rot90'][b]), bool(p['transpose'][b]), bool(p['flip_h'][b]),
                                         bool(p['flip_v'][b]), p['angle'][b], p['scale'][b], p['shear'][b], p['translate'][b])
                              for b in range(B)])
        p['tables'] = None
        if K:
            if u8:
                p['tables'] = np.stack([intensity_table(K, p['gamma'][b], p['contrast'][b], p['brightness'][b], 1 / 255, self.mean,
                                                        self.std) for b in range(B)])
            else:
                if self.gamma is not None:
                    raise NotImplementedError('RandomAffine: gamma is implemented for uint8 images only (a table look-up)')
                p['tables'] = np.stack([intensity_scale_offset(K, p['contrast'][b], p['brightness'][b], 1., self.mean, self.std)
                                        for b in range(B)])
        return p

    def __call__(self, image, labels, generator=None):
        first = image if image is not None else labels
        if not isinstance(first, torch.Tensor):
            raise TypeError('RandomAffine: image or labels must be a Tensor on the GPU')
        batched = first.ndim == 4
        if first.ndim < 2:
            raise ValueError(f'RandomAffine: image and labels must have at least two dimensions (got {tuple(first.shape)})')
        B = int(first.shape[0]) if batched else 1
        src = tuple(int(s) for s in (first.shape[1:3] if batched else first.shape[:2]))
        K = 0 if image is None else (int(image.shape[-1]) if image.ndim > 2 else 1)
        p = self.draw(B, src, K, image is None or image.dtype == torch.uint8, generator)
        self.last_params = p
        return warp(image, labels, p['maps'] if batched else p['maps'][0], self.size,
                    None if p['tables'] is None else (p['tables'] if batched else p['tables'][0]), self.border, 0., self.label_fill,
                    self.out_dtype)
