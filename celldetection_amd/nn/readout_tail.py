"""The ReadOut tail: Dropout2d fused into a 1x1 conv to few channels ("Trainable ReadOut tail" of include/cpn_hip.h,
csrc/readout_tail.hip)

The last two modules of a ReadOut head read the largest activation of a training step.  Stock torch moves it about seven times
(dropout forward and backward, conv forward, weight gradient, input gradient) and saves two copies; ``dropout_conv1x1`` reads it
once forward and once backward, writes ``dx`` once and saves ``x`` alone.  The dropout never touches ``x``: the weight operand of
the MFMA is masked per image and the factor 1 / (1 - p) is applied to the fp32 sum, so ``x / (1 - p)`` is never rounded to bf16.
Supported: a 4-D input on the GPU, float32 or bfloat16, ``Cin`` a positive multiple of 32 up to 1024, 1 <= ``Cout`` <= 32.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _dt, _nhwc, _pair

TAIL_MAX_CIN, TAIL_MAX_COUT = 1024, 32
_TAIL_INFO_KEYS = ('slabs', 'slab_pixels', 'steps', 'reduce_chain', 'bias_chain', 'forward_chain', 'slabs_per_image', 'dx_steps')


def readout_tail_info(n, hw, cin, cout, slab_pixels=0):
    """What the ReadOut-tail kernels would run on ``n`` images of ``hw`` pixels -> dict(slabs, slab_pixels, steps (MFMA steps per
    slab), reduce_chain, bias_chain, forward_chain, slabs_per_image, dx_steps).  Host arithmetic only: needs no GPU.  Raises like
    the launch for a call it rejects."""
    info = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().cpn_tail_info(int(n), int(hw), int(cin), int(cout), int(slab_pixels), info), 'tail_info')
    return dict(zip(_TAIL_INFO_KEYS, (int(v) for v in info)))


def _tail_channels(cin, cout):
    """The first channel count the tail kernels do not run, as a sentence, or None."""
    if cin < 32 or cin % 32 or cin > TAIL_MAX_CIN:
        return f'in_channels {cin}: positive multiples of 32 up to {TAIL_MAX_CIN} only'
    if cout < 1 or cout > TAIL_MAX_COUT:
        return f'out_channels {cout}: 1 ... {TAIL_MAX_COUT} only'
    return None


def _check_tail(x, weight, bias, p, keep, out_dtype):
    """Raises NotImplementedError naming the argument the kernels do not run -> (keep as [N, Cin] or None)."""
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the ReadOut tail takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the ReadOut tail takes float32 or bfloat16 activations')
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1):
        raise NotImplementedError(f'kernel_size / weight {tuple(weight.shape)}: the ReadOut tail runs [Cout, Cin, 1, 1] weights only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the ReadOut tail takes float32 or bfloat16 parameters')
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    why = _tail_channels(cin, cout)
    if why is not None:
        raise NotImplementedError(why)
    if int(x.shape[1]) != cin:
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {cin}')
    if bias is not None and (bias.dim() != 1 or int(bias.shape[0]) != cout or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the ReadOut tail takes a float32 or bfloat16 [{cout}] bias')
    if not isinstance(p, (int, float)) or not 0. <= p <= 1.:
        raise NotImplementedError(f'p {p!r}: a dropout probability in [0, 1]')
    if out_dtype not in _DTYPES:
        raise NotImplementedError(f'out_dtype {out_dtype}: float32 or bfloat16 only')
    if int(x.shape[0]) * int(x.shape[2]) * int(x.shape[3]) == 0:
        raise NotImplementedError(f'input of shape {tuple(x.shape)}: the ReadOut tail needs at least one pixel')
    if keep is not None:
        n = int(x.shape[0])
        if keep.dtype not in (torch.bool, torch.uint8) or keep.numel() != n * cin or \
                tuple(keep.shape) not in ((n, cin), (n, cin, 1, 1)):
            raise NotImplementedError(f'keep {tuple(keep.shape)} {keep.dtype}: a bool or uint8 [{n}, {cin}] mask of the channels kept')


def _tail_scale(p):
    return 0. if p >= 1. else 1. / (1. - p)


def _plane_grad(grad_output):
    g = grad_output.detach()
    return (g if g.dtype in _DTYPES else g.float()).contiguous()


def _tail_backward(xs, grad_output, weight, keep, scale, slab_pixels, need_x, need_w, need_b, bias_dtype):
    """xs: bf16 NHWC memory, 16-byte aligned; keep: uint8 [N, Cin] or None -> (dx bf16 channels-last, dW, db), None where not asked."""
    n, cin, h, w = (int(v) for v in xs.shape)
    cout = int(weight.shape[0])
    lib = _lib.load()
    g = _plane_grad(grad_output)
    assert tuple(g.shape) == (n, cout, h, w), (tuple(g.shape), (n, cout, h, w))
    wd = weight.detach().reshape(cout, cin).contiguous()
    dx = torch.empty_like(xs, memory_format=torch.channels_last) if need_x else None
    dw = torch.empty((cout, cin, 1, 1), dtype=weight.dtype, device=xs.device) if need_w else None
    db = torch.empty((cout,), dtype=bias_dtype, device=xs.device) if need_b else None
    if not (need_x or need_w or need_b):
        return None, None, None
    ws, nbytes = None, 0
    if need_w or need_b:
        nbytes = int(lib.cpn_tail_workspace_bytes(n, h * w, cin, cout, slab_pixels))
        if nbytes <= 0:
            _lib.check(lib.cpn_tail_info(n, h * w, cin, cout, slab_pixels, (ctypes.c_int64 * 8)()), 'tail_backward')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xs.device)
    _lib.check(lib.cpn_tail_backward(_lib.ptr(xs), _lib.ptr(g), _dt(g), _lib.ptr(wd), _dt(wd), _lib.ptr(keep), float(scale), n, h * w,
                                     cin, cout, int(slab_pixels), _lib.ptr(dx), _lib.ptr(dw), _dt(dw), _lib.ptr(db), _dt(db),
                                     _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'tail_backward')
    return dx, dw, db


class _DropoutConv1x1Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, keep, scale, out_dtype, slab_pixels):
        xs = _nhwc(x, torch.bfloat16)
        n, cin, h, w = (int(v) for v in xs.shape)
        cout = int(weight.shape[0])
        wd = weight.detach().reshape(cout, cin).contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        y = torch.empty((n, cout, h, w), dtype=out_dtype, device=xs.device)
        _lib.check(_lib.load().cpn_tail_forward(_lib.ptr(xs), _lib.ptr(wd), _dt(wd), _lib.ptr(bd), _dt(bd), _lib.ptr(keep), float(scale),
                                                n, h * w, cin, cout, _lib.ptr(y), _dt(y), _lib.stream_ptr()), 'tail_forward')
        ctx.save_for_backward(xs, weight, keep)
        ctx.scale, ctx.slab_pixels, ctx.x_dtype = scale, slab_pixels, x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight, keep = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.bias_dtype is not None
        dx, dw, db = _tail_backward(xs, grad_output, weight, keep, ctx.scale, ctx.slab_pixels, need_x, need_w, need_b, ctx.bias_dtype)
        return (None if dx is None else dx.to(ctx.x_dtype)), dw, db, None, None, None, None


def _tail_mask(x, p, training, keep):
    """-> (keep as contiguous uint8 [N, Cin] on x's device or None, s)."""
    if not (training and p > 0):
        return None, 1.
    n, cin = int(x.shape[0]), int(x.shape[1])
    if keep is None:
        if p >= 1.:
            keep = torch.zeros((n, cin), dtype=torch.uint8, device=x.device)
        else:
            keep = torch.empty((n, cin, 1, 1), dtype=x.dtype, device=x.device).bernoulli_(1 - p) != 0
    return keep.detach().reshape(n, cin).to(torch.uint8).contiguous(), _tail_scale(p)


def dropout_conv1x1(x, weight, bias=None, p=0., training=False, keep=None, out_dtype=torch.float32, slab_pixels=0):
    """``F.conv2d(F.dropout2d(x, p, training), weight, bias)`` for a 1x1 ``weight`` ``[Cout <= 32, Cin, 1, 1]`` as one autograd
    function, with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> ``[N, Cout, H, W]``, contiguous NCHW,
    in ``out_dtype`` (float32 | bfloat16).  ``dx`` comes in ``x``'s dtype and ``torch.channels_last``, ``dW`` and ``db`` in the
    parameter's dtype.

    ``keep``: bool / uint8 ``[N, Cin]``, the channels kept per image.  When ``training and p > 0`` and ``keep`` is None it is drawn
    as ``torch.empty((N, Cin, 1, 1), dtype=x.dtype, device=x.device).bernoulli_(1 - p)`` from torch's default generator, so it is
    reproducible under ``torch.manual_seed``; ``p == 1`` drops everything without a draw (the output is the bias).  In eval, or
    with ``p == 0``, nothing is dropped, nothing is drawn and ``keep`` is not looked at.  The kept channels are scaled by
    ``1 / (1 - p)`` on the fp32 sum, never on ``x``.  ``slab_pixels``: pixels per slab of the weight gradient's reduction (0:
    chosen by the library).  Anything unsupported raises ``NotImplementedError`` naming the argument; there is no fallback."""
    _check_tail(x, weight, bias, p, keep, out_dtype)
    _need_cuda(x, weight, bias, keep)
    mask, scale = _tail_mask(x, float(p), bool(training), keep)
    return _DropoutConv1x1Function.apply(x, weight, bias, mask, scale, out_dtype, int(slab_pixels))


def dropout_conv1x1_backward(x, grad_output, weight, keep=None, p=0., slab_pixels=0, input_grad=True, weight_grad=True,
                             bias_grad=True, bias_dtype=None):
    """The gradients ``dropout_conv1x1`` returns for an explicit mask, without autograd: (x [N, Cin, H, W], grad_output [N, Cout, H,
    W], weight, keep [N, Cin] | None = all kept, p) -> (dx bf16 in ``torch.channels_last``, dW in ``weight``'s dtype, db in
    ``bias_dtype`` (default: ``weight``'s)), None for a gradient not asked for."""
    _check_tail(x, weight, None, p, keep, torch.float32)
    _need_cuda(x, grad_output, weight, keep)
    mask = None if keep is None else keep.detach().reshape(int(x.shape[0]), int(x.shape[1])).to(torch.uint8).contiguous()
    scale = _tail_scale(float(p)) if mask is not None else 1.
    return _tail_backward(_nhwc(x, torch.bfloat16), grad_output, weight, mask, scale, int(slab_pixels), input_grad, weight_grad,
                          bias_grad, bias_dtype or weight.dtype)


def _tail_unsupported(kernel_size, stride, padding, dilation, groups, in_channels, out_channels, transposed=False):
    """The first argument the ReadOut tail does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if _pair(kernel_size) != (1, 1):
        return f'kernel_size {kernel_size}: 1x1 only'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if _pair(stride) != (1, 1):
        return f'stride {stride}: stride 1 only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if padding not in ('same', 'valid') and (isinstance(padding, str) or _pair(padding) != (0, 0)):
        return f'padding {padding}: no padding only'
    return _tail_channels(in_channels, out_channels)


class DropoutConv1x1(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` (1x1, torch's constructor arguments and parameter names: ``state_dict``s interchange) with the
    ``Dropout2d(p)`` in front of it folded in: its forward is ``dropout_conv1x1(x, weight, bias, p, training)``."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None, p=0.):
        why = _tail_unsupported(kernel_size, stride, padding, dilation, groups, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        if not 0. <= p <= 1.:
            raise NotImplementedError(f'p {p!r}: a dropout probability in [0, 1]')
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)
        self.p = float(p)

    def forward(self, x):
        return dropout_conv1x1(x, self.weight, self.bias, self.p, self.training)

    def extra_repr(self):
        return super().extra_repr() + f', p={self.p}'


def _tail_why_not(conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _tail_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.in_channels,
                             conv.out_channels, conv.transposed)
