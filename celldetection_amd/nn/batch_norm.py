"""Batch normalisation with an optional fused ReLU ("Trainable batch normalisation" of include/cpn_hip.h, csrc/batch_norm.hip)

In the reference model every trainable conv is followed by BatchNorm2d and ReLU.  ``batch_norm`` runs both as one autograd
function on the channels-last tensor the conv hands over: statistics (1 read), apply (1 read, 1 write), backward reduce (2 reads),
backward input (2 reads, 1 write).  It saves ``x`` and per-channel fp32 vectors only: the ReLU mask is recomputed bit for bit from
``x`` by the forward's own fma.  Sums over pixels are fp64 in a fixed order (no floating-point atomics); supported: a 4-D input
on the GPU, float32 or bfloat16, ``C`` a positive multiple of 8.  With ``residual`` the apply adds it before the ReLU (3 passes) and
the backward masks by the stored output (4 + 3 passes; ``x`` and ``y`` saved).  Known limit: statistics not folded into the conv
epilogue.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _dt, _nhwc

ACTIVATIONS = (None, 'relu')
_INFO_KEYS = ('slabs', 'slab_pixels', 'rows', 'channel_blocks', 'chain')


def batch_norm_info(m, c, slab_pixels=0):
    """What the batch-norm kernels would run on ``m`` pixels of ``c`` channels -> dict(slabs, slab_pixels, rows (pixels per step of
    the first channel block), channel_blocks, chain (terms of the fp64 chain of one channel sum)).  Host arithmetic only: needs no
    GPU.  Raises like the launch for a call it rejects."""
    info = (ctypes.c_int64 * 5)()
    _lib.check(_lib.load().cpn_bn_info(int(m), int(c), int(slab_pixels), info), 'bn_info')
    return dict(zip(_INFO_KEYS, (int(v) for v in info)))


def _check_bn(x, running_mean, running_var, weight, bias, activation):
    """Raises NotImplementedError naming the argument the kernels do not run."""
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f'activation {activation!r}: the fused batch norm runs {ACTIVATIONS} only')
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the batch norm takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the batch norm takes float32 or bfloat16 activations')
    c = int(x.shape[1])
    if c < 8 or c % 8:
        raise NotImplementedError(f'num_features {c}: the batch norm needs a positive multiple of 8 channels')
    for name, t in (('weight', weight), ('bias', bias), ('running_mean', running_mean), ('running_var', running_var)):
        if t is not None and (t.dtype not in _DTYPES or tuple(t.shape) != (c,)):
            raise NotImplementedError(f'{name} {tuple(t.shape)} {t.dtype}: the batch norm takes a float32 or bfloat16 [{c}] vector')
    for name, t in (('running_mean', running_mean), ('running_var', running_var)):
        if t is not None and not t.is_contiguous():
            raise NotImplementedError(f'{name} with strides {t.stride()}: the batch norm updates a contiguous buffer in place')
    if (running_mean is None) != (running_var is None) or \
            (running_mean is not None and running_mean.dtype != running_var.dtype):
        raise NotImplementedError('running_mean / running_var: both or neither, of one dtype')


def _workspace(lib, m, c, slab_pixels, device):
    nbytes = int(lib.cpn_bn_workspace_bytes(m, c, slab_pixels))
    if nbytes <= 0:
        _lib.check(lib.cpn_bn_info(m, c, slab_pixels, (ctypes.c_int64 * 5)()), 'bn')
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def _bn_forward(xs, running_mean, running_var, weight, bias, use_batch, momentum, eps, relu, slab_pixels, residual=None):
    """xs (and residual, if any, of its dtype and shape): channels-last, on the GPU -> (y, save_mean, save_invstd, scale, shift);
    updates the running buffers when use_batch."""
    n, c, h, w = (int(v) for v in xs.shape)
    m = n * h * w
    lib = _lib.load()
    coeffs = torch.empty((4, c), dtype=torch.float32, device=xs.device)
    mean, invstd, scale, shift = coeffs[0], coeffs[1], coeffs[2], coeffs[3]
    y = torch.empty_like(xs, memory_format=torch.channels_last)
    if use_batch:
        ws, nbytes = _workspace(lib, m, c, slab_pixels, xs.device)
        _lib.check(lib.cpn_bn_train_stats(_lib.ptr(xs), _dt(xs), m, c, slab_pixels, _lib.ptr(weight), _dt(weight), _lib.ptr(bias),
                                          _dt(bias), _lib.ptr(running_mean), _lib.ptr(running_var), _dt(running_mean),
                                          float(momentum), float(eps), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(scale),
                                          _lib.ptr(shift), _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'bn_train_stats')
    else:
        _lib.check(lib.cpn_bn_eval_coeffs(c, _lib.ptr(weight), _dt(weight), _lib.ptr(bias), _dt(bias), _lib.ptr(running_mean),
                                          _lib.ptr(running_var), _dt(running_mean), float(eps), _lib.ptr(mean), _lib.ptr(invstd),
                                          _lib.ptr(scale), _lib.ptr(shift), _lib.stream_ptr()), 'bn_eval_coeffs')
    if residual is not None:
        _lib.check(lib.cpn_residual_bn_apply(_lib.ptr(xs), _lib.ptr(residual), _lib.ptr(y), _dt(xs), m, c, slab_pixels, _lib.ptr(scale),
                                             _lib.ptr(shift), int(relu), _lib.stream_ptr()), 'bn_apply_residual')
        return y, mean, invstd, scale, shift
    _lib.check(lib.cpn_bn_apply(_lib.ptr(xs), _lib.ptr(y), _dt(xs), m, c, slab_pixels, _lib.ptr(scale), _lib.ptr(shift), int(relu),
                                _lib.stream_ptr()), 'bn_apply')
    return y, mean, invstd, scale, shift


def _prepare(x, running_mean, running_var, weight, bias, training, activation, residual=None):
    _check_bn(x, running_mean, running_var, weight, bias, activation)
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or tuple(residual.shape) != tuple(x.shape):
            raise NotImplementedError(f'residual of shape {tuple(getattr(residual, "shape", ()))}: the batch norm adds a tensor of the '
                                      f"input's shape {tuple(x.shape)}")
        if residual.dtype not in _DTYPES:
            raise NotImplementedError(f'residual dtype {residual.dtype}: the batch norm adds a float32 or bfloat16 tensor')
        _need_cuda(residual)
    use_batch = bool(training) or running_mean is None
    n, c, h, w = (int(v) for v in x.shape)
    if use_batch and n * h * w == 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
    if n * h * w == 0:
        raise NotImplementedError(f'input of shape {tuple(x.shape)}: the batch norm needs at least one pixel')
    _need_cuda(x, running_mean, running_var, weight, bias)
    return use_batch


def batch_norm_forward(x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5,
                       activation=None, slab_pixels=0, residual=None):
    """The forward of ``batch_norm`` without autograd -> (y, save_mean, save_invstd, scale, shift): ``y`` in ``x``'s dtype and
    ``torch.channels_last``, four fp32 ``[C]`` vectors (eval: the running mean, its invstd and the coefficients from them).  In
    training the running buffers are updated in place.  ``slab_pixels``: pixels per slab of the sums (0: chosen by the library).
    ``residual``: as in ``batch_norm``."""
    use_batch = _prepare(x, running_mean, running_var, weight, bias, training, activation, residual)
    det = [None if t is None else t.detach().contiguous() for t in (weight, bias)]
    xs = _nhwc(x)
    rs = None if residual is None else _nhwc(residual, xs.dtype)
    return _bn_forward(xs, running_mean, running_var, det[0], det[1], use_batch, momentum, eps, activation == 'relu', slab_pixels, rs)


class _BatchNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, use_batch, momentum, eps, relu, slab_pixels):
        xs = _nhwc(x)
        wd = None if weight is None else weight.detach().contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        y, mean, invstd, scale, shift = _bn_forward(xs, running_mean, running_var, wd, bd, use_batch, momentum, eps, relu, slab_pixels)
        ctx.save_for_backward(xs, weight, mean, invstd, scale, shift)
        ctx.use_batch, ctx.relu, ctx.slab_pixels = use_batch, relu, slab_pixels
        ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight, mean, invstd, scale, shift = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_w = need_w and weight is not None
        need_b = need_b and ctx.bias_dtype is not None
        n, c, h, w = (int(v) for v in xs.shape)
        m, sp, relu = n * h * w, ctx.slab_pixels, int(ctx.relu)
        lib = _lib.load()
        gs = _nhwc(grad_output, xs.dtype)
        wd = None if weight is None else weight.detach().contiguous()
        dx = dw = db = abc = None
        if need_w or need_b or (need_x and ctx.use_batch):
            dw = torch.empty((c,), dtype=weight.dtype, device=xs.device) if need_w else None
            db = torch.empty((c,), dtype=ctx.bias_dtype, device=xs.device) if need_b else None
            abc = torch.empty((3, c), dtype=torch.float32, device=xs.device) if need_x and ctx.use_batch else None
            ws, nbytes = _workspace(lib, m, c, sp, xs.device)
            _lib.check(lib.cpn_bn_backward_reduce(_lib.ptr(xs), _lib.ptr(gs), _dt(xs), m, c, sp, _lib.ptr(scale), _lib.ptr(shift), relu,
                                                  _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(wd), _dt(wd), _lib.ptr(dw), _dt(dw),
                                                  _lib.ptr(db), _dt(db), _lib.ptr(abc), _lib.ptr(ws), nbytes, _lib.stream_ptr()),
                       'bn_backward_reduce')
        if need_x:
            dx = torch.empty_like(xs, memory_format=torch.channels_last)
            a, b, cc = (abc[0], abc[1], abc[2]) if ctx.use_batch else (scale, None, None)
            _lib.check(lib.cpn_bn_backward_input(_lib.ptr(xs), _lib.ptr(gs), _lib.ptr(dx), _dt(xs), m, c, sp, _lib.ptr(scale),
                                                 _lib.ptr(shift), relu, _lib.ptr(a), _lib.ptr(b), _lib.ptr(cc), _lib.stream_ptr()),
                       'bn_backward_input')
        return dx, dw, db, None, None, None, None, None, None, None


class _BatchNormResidualFunction(torch.autograd.Function):
    """activation(bn(x) + residual).  Saves x, its own output y and the per-channel vectors -- not the residual: the ReLU mask is
    ``y > 0`` on the stored output, as in torch's own ReLU backward."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, use_batch, momentum, eps, relu, slab_pixels):
        xs = _nhwc(x)
        rs = _nhwc(residual, xs.dtype)
        wd = None if weight is None else weight.detach().contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        y, mean, invstd, scale, shift = _bn_forward(xs, running_mean, running_var, wd, bd, use_batch, momentum, eps, relu, slab_pixels,
                                                    rs)
        ctx.save_for_backward(xs, y, weight, mean, invstd, scale, shift)
        ctx.use_batch, ctx.relu, ctx.slab_pixels = use_batch, relu, slab_pixels
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.residual_dtype = residual.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        xs, y, weight, mean, invstd, scale, shift = ctx.saved_tensors
        need_x, need_r, need_w, need_b = ctx.needs_input_grad[:4]
        need_w = need_w and weight is not None
        need_b = need_b and ctx.bias_dtype is not None
        n, c, h, w = (int(v) for v in xs.shape)
        m, sp = n * h * w, ctx.slab_pixels
        lib = _lib.load()
        gs = _nhwc(grad_output, xs.dtype)
        wd = None if weight is None else weight.detach().contiguous()
        dx = dw = db = abc = None
        sums = need_w or need_b or (need_x and ctx.use_batch)
        g = gs  # without ReLU g = dy: nothing is masked and nothing is written
        if sums or (ctx.relu and (need_x or need_r)):
            dw = torch.empty((c,), dtype=weight.dtype, device=xs.device) if need_w else None
            db = torch.empty((c,), dtype=ctx.bias_dtype, device=xs.device) if need_b else None
            abc = torch.empty((3, c), dtype=torch.float32, device=xs.device) if need_x and ctx.use_batch else None
            if ctx.relu:
                g = torch.empty_like(xs, memory_format=torch.channels_last)
            ws, nbytes = _workspace(lib, m, c, sp, xs.device)
            _lib.check(lib.cpn_residual_bn_backward_reduce(_lib.ptr(xs), _lib.ptr(gs), _lib.ptr(y), _lib.ptr(g), _dt(xs), m, c, sp,
                                                           _lib.ptr(scale), _lib.ptr(shift), int(ctx.relu), _lib.ptr(mean),
                                                           _lib.ptr(invstd), _lib.ptr(wd), _dt(wd), _lib.ptr(dw), _dt(dw), _lib.ptr(db),
                                                           _dt(db), _lib.ptr(abc), _lib.ptr(ws), nbytes, _lib.stream_ptr()),
                       'bn_backward_reduce_residual')
        if need_x:
            dx = torch.empty_like(xs, memory_format=torch.channels_last)
            a, b, cc = (abc[0], abc[1], abc[2]) if ctx.use_batch else (scale, None, None)
            _lib.check(lib.cpn_bn_backward_input(_lib.ptr(xs), _lib.ptr(g), _lib.ptr(dx), _dt(xs), m, c, sp, _lib.ptr(None),
                                                 _lib.ptr(None), 0, _lib.ptr(a), _lib.ptr(b), _lib.ptr(cc), _lib.stream_ptr()),
                       'bn_backward_input')
        dr = g.to(ctx.residual_dtype) if need_r else None
        return dx, dr, dw, db, None, None, None, None, None, None, None


def batch_norm(x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5, activation=None,
               slab_pixels=0, residual=None):
    """``torch.nn.functional.batch_norm`` (its argument order) for a 4-D input on the GPU, followed by ``activation`` (None |
    'relu') in the same kernels, with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> ``x``'s dtype in
    ``torch.channels_last``.  Batch statistics are used when ``training`` or when the running buffers are absent; in training the
    running buffers are updated in place with ``momentum``.  Anything unsupported raises ``NotImplementedError`` naming the
    argument; training on a single value per channel raises ``ValueError`` like torch.

    ``residual`` (``[N, C, H, W]``, float32 | bfloat16, brought to ``x``'s dtype and channels-last as ``grad_output`` is): the tail
    of a residual block, ``activation(bn(x) + residual)`` in one pass behind the unchanged statistics: ``t = fmaf(x, scale, shift)``
    and ``t + residual`` are fp32 operations, the result is rounded once to the dtype.  Its backward takes the ReLU mask from the
    stored output (``y > 0``), so it saves ``x`` and its own output ``y``, which the next conv saves anyway, and not ``residual``; an
    in-place operation on ``y`` downstream therefore makes autograd raise.  The masked gradient is the residual's gradient bit for
    bit (returned in ``residual``'s dtype).  ``residual=None``: the same launches and bits as without the argument."""
    use_batch = _prepare(x, running_mean, running_var, weight, bias, training, activation, residual)
    if residual is not None:
        return _BatchNormResidualFunction.apply(x, residual, weight, bias, running_mean, running_var, use_batch, float(momentum),
                                                float(eps), activation == 'relu', int(slab_pixels))
    return _BatchNormFunction.apply(x, weight, bias, running_mean, running_var, use_batch, float(momentum), float(eps),
                                    activation == 'relu', int(slab_pixels))


_MODULE_S = object()  # BatchNorm2d.forward(activation=...): "the module's own"


class BatchNorm2d(torch.nn.BatchNorm2d):
    """``torch.nn.BatchNorm2d`` with torch's constructor arguments, parameter and buffer names (``state_dict``s interchange) plus
    ``activation`` (None | 'relu'), whose forward is ``batch_norm``.  ``num_batches_tracked`` and ``momentum=None`` (cumulative
    average) behave as in torch."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None,
                 activation=None):
        if activation not in ACTIVATIONS:
            raise NotImplementedError(f'activation {activation!r}: the fused batch norm runs {ACTIVATIONS} only')
        if num_features < 8 or num_features % 8:
            raise NotImplementedError(f'num_features {num_features}: the batch norm needs a positive multiple of 8 channels')
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device, dtype)
        self.activation = activation

    def forward(self, x, residual=None, activation=_MODULE_S):
        """``residual``, ``activation`` (default: the module's): as in ``batch_norm``, for this call."""
        activation = self.activation if activation is _MODULE_S else activation
        factor = 0. if self.momentum is None else self.momentum
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            if self.momentum is None:
                factor = 1. / float(self.num_batches_tracked)
        use_buffers = not self.training or self.track_running_stats
        return batch_norm(x, self.running_mean if use_buffers else None, self.running_var if use_buffers else None, self.weight,
                          self.bias, self.training or self.running_mean is None, factor, self.eps, activation, residual=residual)

    def extra_repr(self):
        return super().extra_repr() + f', activation={self.activation!r}'


def _bn_why_not(bn):
    if type(bn) is not torch.nn.BatchNorm2d:
        return f'{type(bn).__name__}: torch.nn.BatchNorm2d itself only'
    if bn.num_features < 8 or bn.num_features % 8:
        return f'num_features {bn.num_features}: multiples of 8 only'
    for name, t in list(bn.named_parameters(recurse=False)) + list(bn.named_buffers(recurse=False)):
        if name != 'num_batches_tracked' and t.dtype not in _DTYPES:
            return f'{name} dtype {t.dtype}: float32 or bfloat16 only'
    return None
