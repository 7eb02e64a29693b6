"""What the label-image operations share on the way to their int32 kernels: the int32 range check, the 16-byte alignment of
vector loads and the upload of numpy arrays.  Every caller passes the text of its own errors; checks that differ between
the operations (ranks, ``bool`` labels) stay in their modules."""
import numpy as np
import torch

__all__ = ['INT32_MIN', 'INT32_MAX', 'to_int32', 'aligned16', 'upload_numpy', 'check_labels']

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
_FITS = (torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool)  # no range check needed


def to_int32(x, message):
    """-> contiguous int32 Tensor; ``ValueError(message)`` when a value does not fit."""
    if x.dtype not in _FITS and x.numel() and (int(x.min()) < INT32_MIN or int(x.max()) > INT32_MAX):
        raise ValueError(message)
    return x.to(torch.int32).contiguous()


def aligned16(x):
    """``x``, or a copy of it that begins at a multiple of 16 bytes."""
    return x.clone() if x.data_ptr() % 16 else x


def upload_numpy(x, who, what):
    """Integer numpy array -> Tensor on the GPU.  The unsigned dtypes torch does not compute with are widened, their range is
    checked here (``what``: '<argument> holds labels' or '... holds values')."""
    if x.dtype in (np.uint16, np.uint32, np.uint64):
        if x.size and int(x.max()) > INT32_MAX:
            raise ValueError(f'{who}: {what} that do not fit int32')
        x = x.astype(np.int32 if x.dtype == np.uint16 else np.int64)
    if not torch.cuda.is_available():
        raise RuntimeError(f'celldetection_amd.{who} runs on the MI355X only (no GPU to upload the arrays to).')
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def check_labels(labels, name, ranks=(3,)):
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f'{name}: labels must be a Tensor on the GPU (got {type(labels).__name__})')
    if labels.ndim not in ranks:
        raise ValueError(f'{name}: labels must be {" or ".join("[H, W, C]" if r == 3 else "[H, W]" for r in ranks)} '
                         f'(got {tuple(labels.shape)})')
    if labels.ndim == 3 and labels.shape[2] < 1:
        raise ValueError(f'{name}: labels has no channel')
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError(f'{name}: labels must hold integers (got {labels.dtype})')
    if not labels.is_cuda:
        raise RuntimeError(f'celldetection_amd.{name} runs on the MI355X only (got a CPU tensor).')
