"""The end of a training step on the MI355X: gradient clipping by the global L2 norm and the AdamW update, as multi-tensor launches
of this library's HIP kernels (csrc/optim.hip; the rule is the "Optimizer step" section of include/cpn_hip.h).  ``cd.optim`` of the
reference holds its schedulers; they and ``torch.optim.lr_scheduler.*`` drive ``AdamW`` below unchanged.

* ``AdamW``: a ``torch.optim.Optimizer`` whose ``step()`` is one upload and one launch (three with ``max_grad_norm``: the sum of
  squares, the norm and clip coefficient, the update with the coefficient folded into its read of the gradient).
* ``clip_grad_norm_`` / ``grad_norm``: the stand-alone forms of ``torch.nn.utils.clip_grad_norm_`` / ``get_total_norm``.  They
  return a float32 0-d GPU tensor and never read it on the host.
* ``step_info``: the chunk partition a launch over tensors of the given sizes uses (host arithmetic, needs no GPU).

Host work per step.  The per-tensor scalars are computed in Python floats (fp64) from the Python value of ``step`` and rounded once
to float32 when they are written into the table of ``CpnOptimTensor`` records, together with the addresses of p, g, m and v.  The
table is built in a pinned staging buffer and sent with one ``hipMemcpyAsync`` (``cpn_optim_upload``).  Staging buffers form a ring
of ``RING`` per device; a slot carries the event recorded behind its last upload and is rewritten only after that event has
completed, so a buffer is never changed under a copy in flight.  The wait is on a copy issued ``RING`` calls earlier: nothing in
steady state, back-pressure if the host runs further ahead than that.  The chunk map depends on the sizes alone and is uploaded once
per list of sizes (the last ``MAPS`` lists are kept).  Nothing else is copied, and no result is read back.  All calls on one device
share its staging, table and partial-sum buffers: issue them on one stream, or order the streams yourself.

Known limits: no hipGraph capture of a step (a call during stream capture raises); AdamW only, and no fp32 master copy of a bf16
parameter (it is updated in fp32 and rounded once); a non-finite norm is not detected and the step is not skipped (NaN and inf
propagate as in torch); the packed bf16 weights of the convs are still repacked from the parameter by ``cpn_conv_train_pack`` on
every forward instead of being written here; one workgroup per chunk of ``step_info()['chunk_elements']`` elements, so hundreds of
tiny tensors run mostly idle lanes (profiles/optim.txt has the figures).
"""
import ctypes
import math
from collections import OrderedDict
from itertools import chain

import numpy as np
import torch

from . import _lib
from .nn._common import _DTYPES
from .objective import DeviceError

__all__ = ['AdamW', 'clip_grad_norm_', 'grad_norm', 'step_info']

RING = 4  # staging buffers per device
MAPS = 8  # chunk maps kept per device
NONTEMPORAL = 0  # the store policy of m and v (profiles/optim.txt: the non-temporal hint measured against plain stores)
_MOMENTS = ('exp_avg', 'exp_avg_sq')
_UNSUPPORTED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'foreach', 'fused')


def _record_dtype(struct):
    """The numpy dtype of a ctypes Structure: the same names, offsets and size, a pointer as its address ('<u8').  (np.dtype(struct)
    itself refuses pointer fields.)"""
    names = [name for name, _ in struct._fields_]
    return np.dtype(dict(names=names, formats=['<u8' if t is ctypes.c_void_p else np.dtype(t).str for _, t in struct._fields_],
                         offsets=[getattr(struct, name).offset for name in names], itemsize=ctypes.sizeof(struct)))


_RECORD = _record_dtype(_lib.OptimTensor)  # CpnOptimTensor of include/cpn_hip.h
_SCALARS = ('lr', 'decay', 'w1', 'beta2', 'w2', 'eps', 'step_size', 'bc2_sqrt')


def step_info(numels, dtypes=None):
    """The partition a launch over tensors of ``numels`` elements uses -> dict(chunk_elements, chunks, partials, tensors, vectors):
    ``tensors[i]`` = (first chunk, chunks, elements of the last chunk) of tensor i (an empty tensor has no chunk and tail 0),
    ``partials`` the fp64 partial sums of the norm (one per chunk), ``vectors[i]`` the elements of a 16-byte item of ``dtypes[i]``
    (None without ``dtypes``; the partition does not depend on them).  Host arithmetic only: needs no GPU."""
    numels = [int(v) for v in numels]
    n = len(numels)
    if dtypes is not None:
        dtypes = list(dtypes)
        if len(dtypes) != n or any(d not in _DTYPES for d in dtypes):
            raise NotImplementedError(f'dtypes {dtypes}: one of float32 and bfloat16 per tensor')
    info, per = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * (3 * max(n, 1)))()
    _lib.check(_lib.load().cpn_optim_info((ctypes.c_int64 * max(n, 1))(*numels), n, info, per), 'optim_info')
    return dict(chunk_elements=int(info[0]), chunks=int(info[1]), partials=int(info[2]),
                tensors=[tuple(int(v) for v in per[3 * i:3 * i + 3]) for i in range(n)],
                vectors=None if dtypes is None else [{torch.float32: 4, torch.bfloat16: 8}[d] for d in dtypes])


def scalars(lr, betas, eps, weight_decay, step):
    """The eight scalars of a table record in Python floats (fp64), in the order of the record: lr, decay, w1, beta2, w2, eps,
    step_size, bc2_sqrt.  They are rounded once to float32 when the record is written."""
    beta1, beta2 = betas
    return (lr, 1. - lr * weight_decay, 1. - beta1, beta2, 1. - beta2, eps, lr / (1. - beta1 ** step), math.sqrt(1. - beta2 ** step))


class _Engine:
    """What the calls on one device share: the ring of pinned staging buffers with their events, the device table, the fp64
    partials and the chunk maps."""

    def __init__(self, device):
        self.device = device
        self.ring = [[None, None] for _ in range(RING)]  # [pinned uint8 tensor, event behind its last upload | None]
        self.slot = 0
        self.table = self.partials = None
        self.maps = OrderedDict()

    def plan(self, numels):
        """-> (device int32 map [chunks][2] | None, chunks) of a list of sizes."""
        key = tuple(numels)
        hit = self.maps.get(key)
        if hit is not None:
            self.maps.move_to_end(key)
            return hit
        n = len(key)
        lib = _lib.load()
        sizes, info = (ctypes.c_int64 * max(n, 1))(*key), (ctypes.c_int64 * 3)()
        _lib.check(lib.cpn_optim_info(sizes, n, info, None), 'optim_info')
        chunks = int(info[1])
        dev = None
        if chunks:
            host = np.empty((chunks, 2), dtype=np.int32)
            _lib.check(lib.cpn_optim_chunk_map(sizes, n, host.ctypes.data, chunks), 'optim_chunk_map')
            dev = torch.from_numpy(host).to(self.device)
        self.maps[key] = (dev, chunks)
        while len(self.maps) > MAPS:
            self.maps.popitem(last=False)
        if self.partials is None or self.partials.numel() < chunks:
            self.partials = torch.empty((max(chunks, 1),), dtype=torch.float64, device=self.device)
        return dev, chunks

    def stage(self, n):
        """-> (slot, records [n]): the next staging buffer of the ring, free to be written."""
        slot = self.ring[self.slot]
        self.slot = (self.slot + 1) % RING
        if slot[1] is not None:
            slot[1].synchronize()  # the upload issued RING calls ago
            slot[1] = None
        if slot[0] is None or slot[0].numel() < n * _RECORD.itemsize:
            slot[0] = torch.empty((max(2 * n, 64) * _RECORD.itemsize,), dtype=torch.uint8, pin_memory=True)
        if self.table is None or self.table.numel() < n * _RECORD.itemsize:
            self.table = torch.empty((max(2 * n, 64) * _RECORD.itemsize,), dtype=torch.uint8, device=self.device)
        return slot, slot[0].numpy().view(_RECORD)[:n]

    def upload(self, slot, n, with_state):
        records = ctypes.cast(slot[0].data_ptr(), ctypes.POINTER(_lib.OptimTensor))
        _lib.check(_lib.load().cpn_optim_upload(records, n, int(with_state), _lib.ptr(self.table), _lib.stream_ptr()), 'optim_upload')
        slot[1] = torch.cuda.Event()
        slot[1].record()

    def norm(self, n, plan, max_norm):
        """The norm of the gradients of the uploaded table -> float32 [2] on the device: (norm, clip coefficient)."""
        dev_map, chunks = plan
        lib, out = _lib.load(), torch.empty((2,), dtype=torch.float32, device=self.device)
        _lib.check(lib.cpn_optim_sumsq(_lib.ptr(self.table), n, _lib.ptr(dev_map), chunks, _lib.ptr(self.partials), _lib.stream_ptr()),
                   'optim_sumsq')
        _lib.check(lib.cpn_optim_norm(_lib.ptr(self.partials), chunks, float(max_norm), _lib.ptr(out), _lib.stream_ptr()), 'optim_norm')
        return out


_ENGINES = {}


def _engine(device):
    if torch.cuda.is_current_stream_capturing():
        raise NotImplementedError('stream capture: the optimizer kernels upload their tensor table per call and cannot be captured')
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _ENGINES:
        _ENGINES[key] = _Engine(torch.device('cuda', key))
    return _ENGINES[key]


def _check_kind(t, what, who):
    if t.is_sparse or t.layout != torch.strided:
        raise NotImplementedError(f'{who}: sparse {what}')
    if t.is_complex():
        raise NotImplementedError(f'{who}: complex {what}')


def _check_tensor(t, what, who):
    _check_kind(t, what, who)
    if t.device.type != 'cuda':
        raise DeviceError(f'{who} runs on the MI355X GPU only (a {what} is on {t.device}); there is no CPU fallback.')
    if t.dtype not in _DTYPES:
        raise NotImplementedError(f'{who}: {what} of dtype {t.dtype}: float32 or bfloat16')
    if not t.is_contiguous():
        raise NotImplementedError(f'{who}: non-contiguous {what} (strides {tuple(t.stride())} of shape {tuple(t.shape)})')


def _gradients(parameters, who):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        _check_tensor(g, 'gradient', who)
    if not grads:
        if not parameters:
            raise ValueError(f'{who}: no parameters')
        if parameters[0].device.type != 'cuda':
            raise DeviceError(f'{who} runs on the MI355X GPU only; there is no CPU fallback.')
        return grads, parameters[0].device
    if any(g.device != grads[0].device for g in grads):
        raise NotImplementedError(f'{who}: gradients on more than one device')
    return grads, grads[0].device


def _gradient_table(grads, device):
    """Stages and uploads the table of a list of gradients alone -> (engine, n, plan)."""
    eng = _engine(device)
    n = len(grads)
    plan = eng.plan([g.numel() for g in grads])
    if n:
        slot, rec = eng.stage(n)
        rec[:] = 0
        rec['g'] = [g.data_ptr() for g in grads]
        rec['numel'] = [g.numel() for g in grads]
        rec['dtype'] = [_DTYPES[g.dtype] for g in grads]
        eng.upload(slot, n, False)
    return eng, n, plan


@torch.no_grad()
def grad_norm(parameters):
    """The L2 norm of all gradients of ``parameters`` (those with ``.grad``) as one vector -> float32 0-d GPU tensor, not read by the
    host.  fp64 sums in a fixed order: bit-identical from run to run."""
    grads, device = _gradients(parameters, 'celldetection_amd.optim.grad_norm')
    with torch.cuda.device(device):
        eng, n, plan = _gradient_table(grads, device)
        return eng.norm(n, plan, math.inf)[0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` for the L2 norm: scales the gradients in place by min(1, max_norm / (norm + 1e-6)), each
    rounded once to its dtype, and returns the norm before clipping as a float32 0-d GPU tensor.  No host synchronisation."""
    if float(norm_type) != 2.:
        raise NotImplementedError(f'norm_type {norm_type}: the L2 norm only')
    if error_if_nonfinite:
        raise NotImplementedError('error_if_nonfinite: the norm is never read by the host')
    if foreach:
        raise NotImplementedError('foreach: there is one implementation')
    grads, device = _gradients(parameters, 'celldetection_amd.optim.clip_grad_norm_')
    with torch.cuda.device(device):
        eng, n, plan = _gradient_table(grads, device)
        out = eng.norm(n, plan, float(max_norm))
        _lib.check(_lib.load().cpn_optim_scale(_lib.ptr(eng.table), n, _lib.ptr(plan[0]), plan[1], _lib.ptr(out[1:]), _lib.stream_ptr()),
                   'optim_scale')
    return out[0]


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (decoupled weight decay) on this library's kernels, with an optional fused clip of the global gradient
    norm.  State per parameter as torch keeps it: ``step`` (float32 scalar on the CPU), ``exp_avg`` and ``exp_avg_sq`` (float32
    whatever the parameter's dtype); a ``state_dict()`` of ``torch.optim.AdamW`` loads here and the other way round.  Parameters are
    float32 or bfloat16 on the GPU, contiguous, with dense gradients of their dtype; one without ``.grad`` is skipped.

    ``max_grad_norm``: the gradients this step uses, over all groups, are clipped to that L2 norm as ``clip_grad_norm_`` would,
    but the coefficient is applied where the update reads g: ``.grad`` stays unscaled.  The norm of the last step is
    ``last_grad_norm`` and its coefficient ``last_clip_coef``, float32 0-d GPU tensors (None without ``max_grad_norm``)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, *, amsgrad=False,
                 maximize=False, capturable=False, differentiable=False, foreach=None, fused=None):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError('lr: a tensor lr is not supported (pass a float)')
        if not 0. <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0. <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not (0. <= betas[0] < 1. and 0. <= betas[1] < 1.):
            raise ValueError(f'Invalid betas: {betas}')
        if not 0. <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.:
            raise ValueError(f'Invalid max_grad_norm: {max_grad_norm}')
        # (the keys torch.optim.AdamW keeps in a group, so that either state_dict loads into the other)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
        self._check_group(defaults)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = self.last_clip_coef = None
        self._admitted = {}  # parameter -> what _admit returned for it

    def __getstate__(self):
        return dict(super().__getstate__(), max_grad_norm=self.max_grad_norm)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('max_grad_norm', None)
        self.last_grad_norm = self.last_clip_coef = None
        self._admitted = {}

    @staticmethod
    def _check_group(group):
        for key in _UNSUPPORTED:
            if group.get(key):
                raise NotImplementedError(f'{key}: celldetection_amd.optim.AdamW has one implementation and does not support {key}={group[key]}')
        if isinstance(group['lr'], torch.Tensor):
            raise NotImplementedError('lr: a tensor lr is not supported (pass a float)')
        if not group.get('decoupled_weight_decay', True):
            raise NotImplementedError('decoupled_weight_decay: False is Adam with L2 regularisation, not AdamW')

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # torch casts every floating-point state to the parameter's dtype; the moments here are float32 from the saved values
        saved = chain.from_iterable(g['params'] for g in state_dict['param_groups'])
        for key, p in zip(saved, chain.from_iterable(g['params'] for g in self.param_groups)):
            src = state_dict['state'].get(key)
            if not src:
                continue
            state = self.state[p]
            for name in _MOMENTS:
                state[name] = src[name].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
            step = src['step']
            state['step'] = torch.tensor(float(step), dtype=torch.float32)
        for group in self.param_groups:
            self._check_group(group)

    def _admit(self, p, g):
        """Every check of one parameter, its gradient and its state (created here where there is none) -> the entry ``step()`` keeps
        while the tensors stay the same objects at the same place: (p address, dtype, shape, device, dtype code, numel, exp_avg,
        exp_avg_sq, their addresses, step tensor)."""
        who = 'celldetection_amd.optim.AdamW'
        _check_kind(p, 'parameter', who)
        _check_kind(g, 'gradient', who)
        _check_tensor(p, 'parameter', who)
        _check_tensor(g, 'gradient', who)
        if g.dtype != p.dtype or g.shape != p.shape or g.device != p.device:
            raise NotImplementedError(f'{who}: a gradient of {g.dtype} {tuple(g.shape)} on {g.device} for a parameter of {p.dtype} '
                                      f'{tuple(p.shape)} on {p.device}')
        state = self.state[p]
        if not state:
            state['step'] = torch.tensor(0., dtype=torch.float32)
            for name in _MOMENTS:
                state[name] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        for name in _MOMENTS:  # (a loaded or edited state: the kernels trust these sizes)
            m = state[name]
            if m.dtype != torch.float32 or m.device != p.device or m.numel() != p.numel() or not m.is_contiguous():
                raise ValueError(f'{who}: state {name} must be a contiguous float32 tensor of the parameter\'s size on its device')
        step = state['step']
        if not (isinstance(step, torch.Tensor) and step.device.type == 'cpu' and step.dtype == torch.float32 and step.dim() == 0):
            step = state['step'] = torch.tensor(float(step), dtype=torch.float32)
        m, v = state['exp_avg'], state['exp_avg_sq']
        return (p.data_ptr(), p.dtype, p.shape, p.device, _DTYPES[p.dtype], p.numel(), m, v, m.data_ptr(), v.data_ptr(), step)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # the host side of a step is a loop over several hundred tensors: a parameter whose tensors are the objects _admit checked,
        # at the same address, takes the short way (its gradient, a new tensor every step, is checked every time)
        entries, grads, steps, groups = [], [], [], []
        cache, states, strided = self._admitted, self.state, torch.strided
        for index, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                state = states.get(p)
                e = cache.get(p)
                if (e is None or state is None or g.dtype is not e[1] or g.shape != e[2] or g.device != e[3] or g.layout is not strided
                        or not g.is_contiguous() or p.dtype is not e[1] or p.data_ptr() != e[0] or state.get('exp_avg') is not e[6]
                        or state.get('exp_avg_sq') is not e[7] or state.get('step') is not e[10]):
                    e = cache[p] = self._admit(p, g)
                entries.append(e)
                grads.append(g)
                steps.append(e[10])
                groups.append(index)
        if not entries:
            return loss
        device = entries[0][3]
        if any(e[3] != device for e in entries):
            raise NotImplementedError('celldetection_amd.optim.AdamW: parameters on more than one device')
        with torch.cuda.device(device):
            eng = _engine(device)  # (refuses a stream capture before any state changes)
            torch._foreach_add_(steps, 1.)
            counts = torch.stack(steps).tolist()
            rows, row_of, row_index = [], {}, []
            for index, t in zip(groups, counts):
                key = (index, t)
                if key not in row_of:
                    group = self.param_groups[index]
                    row_of[key] = len(rows)
                    rows.append(scalars(float(group['lr']), group['betas'], group['eps'], group['weight_decay'], t))
                row_index.append(row_of[key])
            n = len(entries)
            numels = [e[5] for e in entries]
            plan = eng.plan(numels)
            slot, rec = eng.stage(n)
            rec['p'] = [e[0] for e in entries]
            rec['g'] = [g.data_ptr() for g in grads]
            rec['m'] = [e[8] for e in entries]
            rec['v'] = [e[9] for e in entries]
            rec['numel'] = numels
            rec['dtype'] = [e[4] for e in entries]
            rec['flags'] = 0
            columns = np.asarray(rows, dtype=np.float64)[row_index]
            for i, name in enumerate(_SCALARS):
                rec[name] = columns[:, i]  # fp64 -> fp32, to nearest: the one rounding
            eng.upload(slot, n, True)
            coef = None
            if self.max_grad_norm is not None:
                out = eng.norm(n, plan, self.max_grad_norm)
                self.last_grad_norm, self.last_clip_coef = out[0], out[1]
                coef = out[1:]
            _lib.check(_lib.load().cpn_optim_adamw(_lib.ptr(eng.table), n, _lib.ptr(plan[0]), plan[1], _lib.ptr(coef), NONTEMPORAL,
                                                   _lib.stream_ptr()), 'optim_adamw')
        return loss
