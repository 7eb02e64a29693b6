"""The recorder and the judges of the training-step tests (test helper, not a conftest).

A whole-net gradient comparison against fp64 cannot tell a right bf16 implementation from a wrong one (tests/test_train_step.py
measures it: the parameter gradients of stock bf16 autocast are tens of percent off stock fp64).  So every leaf module is judged on
the operands IT saw.  ``Recorder`` hooks every leaf of a net -- this library's modules in a converted net, every childless module in
a stock one -- and keeps per call: the operands (positional and keyword), the outputs, the gradient that arrived at each output,
the gradient this call sent to each tensor operand, the parameter gradients, the buffers before and after, the RNG state before.

One consumer's share of a gradient is seen alone through an alias: a forward pre-hook hands the module ``x.view_as(x)`` with a
tensor hook on it, so what autograd later adds for the other consumers of ``x`` never reaches that hook.

The judges that need no arithmetic model live here: ``replay`` (a recorded call run again, alone, on clones of what it saw),
``fan_out`` / ``judge_fan_out`` (the shares of a tensor with several consumers add up to what its producer received),
``judge_routes`` (every consumer read the tensor its producer wrote) and ``judge_buffers`` (a norm's buffers moved by exactly one
update from the statistics of the input it saw).  tests/test_train_step.py plants one fault at a time in fp64 records and shows that
each is flagged.
"""
import copy

import torch

U_OF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float64: 0.}  # unit roundoffs


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def rel_l2(got, ref):
    return float((got.detach().double().cpu() - ref.double()).norm() / ref.double().norm())


def keep(t):
    return t.detach().clone()  # (clone keeps the memory format)


class Call:
    """One call of one leaf: ``operands`` {key: tensor} and ``extras`` {key: anything else} by position (int) or keyword (str),
    ``outputs`` [tensor], ``grad_out`` {output index: gradient}, ``grad_in`` {key: gradient}, ``param_grads`` {name: gradient},
    ``buffers_before`` / ``buffers_after`` {name: tensor}, ``saved`` (a norm's per-channel saved vectors), ``rng``."""

    def __init__(self, name, index, module):
        self.name, self.index, self.module = name, index, module
        self.operands, self.extras, self.needs, self.inputs = {}, {}, {}, {}
        self.outputs, self.out_refs, self.grad_out, self.grad_in, self.param_grads = [], [], {}, {}, {}
        self.buffers_before, self.buffers_after, self.saved, self.rng, self.nargs = {}, {}, [], None, 0

    def __repr__(self):
        return f'Call({self.name}#{self.index})'


class _Functional(torch.nn.Module):
    """A function as a module, so that the same hooks record it."""

    def __init__(self, fn):
        super().__init__()
        self.fn = [fn]  # (a list: not a child, not deep-copied into something else)

    def forward(self, *args, **kwargs):
        return self.fn[0](*args, **kwargs)


def _saved_vectors(out):
    fn = getattr(out, 'grad_fn', None)
    saved = getattr(fn, 'saved_tensors', None) if fn is not None else None
    return [] if saved is None else [keep(t) for t in saved if t is not None and t.dim() == 1 and not t.requires_grad]


class Recorder:
    """``with Recorder(net, is_leaf) as rec: forward and backward`` then ``rec.finish()``.  ``functions``: {name: (namespace,
    attribute)}, functions recorded like leaves (``bilinear_resize`` of the converted core).  ``rec.calls``: in call order;
    ``rec[name]``: the first call of that leaf, ``rec.get(name, i)``: its call i."""

    def __init__(self, net, is_leaf, functions=None, norm_types=()):
        self.net, self.is_leaf, self.functions, self.norm_types = net, is_leaf, dict(functions or {}), tuple(norm_types)
        self.calls, self.by_name, self._open, self._handles, self._patched = [], {}, {}, [], []

    def __enter__(self):
        for name, m in self.net.named_modules():
            if self.is_leaf(m):
                self._hook(name, m)
        for name, (space, attribute) in self.functions.items():
            fn = getattr(space, attribute)
            wrapped = _Functional(fn)
            self._hook(name, wrapped)
            setattr(space, attribute, wrapped)
            self._patched.append((space, attribute, fn))
        return self

    def __exit__(self, *exc):
        for h in self._handles:
            h.remove()
        for space, attribute, fn in self._patched:
            setattr(space, attribute, fn)
        self._handles, self._patched = [], []

    def _hook(self, name, m):
        self._handles.append(m.register_forward_pre_hook(lambda mod, a, kw: self._before(name, mod, a, kw), with_kwargs=True))
        self._handles.append(m.register_forward_hook(lambda mod, a, kw, out: self._after(name, out), with_kwargs=True))

    def _before(self, name, module, args, kwargs):
        call = Call(name, len(self.by_name.setdefault(name, [])), module)
        call.nargs = len(args)
        first = next((a for a in list(args) + list(kwargs.values()) if torch.is_tensor(a)), None)
        call.rng = torch.cuda.get_rng_state(first.device) if first is not None and first.is_cuda else torch.get_rng_state()
        call.buffers_before = {k: keep(b) for k, b in module.named_buffers(recurse=False)}

        def take(key, value):
            if not torch.is_tensor(value):
                call.extras[key] = value
                return value
            call.operands[key], call.inputs[key], call.needs[key] = keep(value), value, value.requires_grad
            if not value.requires_grad:
                return value
            alias = value.view_as(value)
            alias.register_hook(lambda g: call.grad_in.__setitem__(key, keep(g)))
            return alias

        new_args = tuple(take(i, a) for i, a in enumerate(args))
        new_kwargs = {k: take(k, v) for k, v in kwargs.items()}
        self.by_name[name].append(call)
        self.calls.append(call)
        self._open[name] = call
        return new_args, new_kwargs

    def _after(self, name, output):
        call = self._open.pop(name)
        outs = list(output) if isinstance(output, (tuple, list)) else [output]
        call.outputs, call.out_refs = [keep(o) for o in outs], outs
        for i, o in enumerate(outs):
            if o.requires_grad:
                o.register_hook(lambda g, i=i: call.grad_out.__setitem__(i, keep(g)))
        call.buffers_after = {k: keep(b) for k, b in call.module.named_buffers(recurse=False)}
        if isinstance(call.module, self.norm_types):
            call.saved = _saved_vectors(outs[0])

    def finish(self):
        """After ``backward()``: the parameter gradients of every call's module."""
        for call in self.calls:
            call.param_grads = {k: keep(p.grad) for k, p in call.module.named_parameters(recurse=False) if p.grad is not None}
        return self

    def __getitem__(self, name):
        return self.by_name[name][0]

    def get(self, name, index=0):
        return self.by_name[name][index]


def stock_leaf(m):
    """Every childless module of a stock net but ``Identity`` (it hands its input on as the object it is)."""
    return next(m.children(), None) is None and not isinstance(m, (torch.nn.Identity, _Functional))


def library_leaf(nn):
    leaves = (nn.Conv2d, nn.StridedConv1x1, nn.GroupedConv2d, nn.StemConv2d, nn.MaxPool2d, nn.CatConv2d, nn.BatchNorm2d,
              nn.DropoutConv1x1)  # (ResizedConv2d is a Conv2d)
    return lambda m: isinstance(m, leaves)


# ---- a recorded call run again, alone

def _functional(call, m, args, kwargs, nn):
    """The family's functional entry point on the deep copy's parameters and buffers."""
    t = type(m)
    w, b = getattr(m, 'weight', None), getattr(m, 'bias', None)
    if t is _Functional:
        return nn.bilinear_resize(*args, **kwargs)
    if t is nn.BatchNorm2d:
        activation = kwargs['activation'] if 'activation' in kwargs else (args[2] if len(args) > 2 else m.activation)
        residual = kwargs['residual'] if 'residual' in kwargs else (args[1] if len(args) > 1 else None)
        assert m.training and m.track_running_stats and m.momentum is not None
        m.num_batches_tracked.add_(1)
        return nn.batch_norm(args[0], m.running_mean, m.running_var, w, b, True, m.momentum, m.eps, activation, residual=residual)
    if t is nn.ResizedConv2d and (len(args) > 1 or 'size' in kwargs):
        return nn.resized_conv2d(args[0], w, b, kwargs['size'] if 'size' in kwargs else args[1])
    if t in (nn.Conv2d, nn.ResizedConv2d):
        fork = kwargs.get('fork', args[1] if len(args) > 1 else False)
        return nn.conv2d_fork(args[0], w, b) if fork else nn.conv2d(args[0], w, b)
    if t is nn.CatConv2d:
        return nn.cat_conv2d(args[0], args[1], w, b) if len(args) > 1 else nn.conv2d(args[0], w, b)
    if t is nn.StridedConv1x1:
        return nn.strided_conv1x1(args[0], w, b)
    if t is nn.GroupedConv2d:
        return nn.grouped_conv2d(args[0], w, b, m.stride, m.groups)
    if t is nn.StemConv2d:
        return nn.stem_conv2d(args[0], w, b)
    if t is nn.MaxPool2d:
        return nn.max_pool2d(args[0], m.kernel_size, m.stride, m.padding)
    if t is nn.DropoutConv1x1:
        return nn.dropout_conv1x1(args[0], w, b, m.p, m.training)
    raise AssertionError(f'{call}: no functional entry point for {t.__name__}')


def replay(call, nn=None):
    """The recorded call once more on fresh clones of its operands (same dtype and memory format), through a deep copy of its module
    whose buffers are set back to what they were, with the RNG state it had -> a ``Call`` holding what came out.  ``nn``: go through
    the family's functional entry point of this library instead of the module's ``forward``."""
    m = copy.deepcopy(call.module)
    m._forward_hooks.clear(), m._forward_pre_hooks.clear()
    with torch.no_grad():
        for k, buf in m.named_buffers(recurse=False):
            buf.copy_(call.buffers_before[k])
    for p in m.parameters(recurse=False):
        p.grad = None
    fresh = {key: keep(t).requires_grad_(call.needs[key]) for key, t in call.operands.items()}
    merged = dict(call.extras)
    merged.update(fresh)
    args = [merged[i] for i in range(call.nargs)]
    kwargs = {k: v for k, v in merged.items() if isinstance(k, str)}
    device = next(iter(call.operands.values())).device
    if device.type == 'cuda':
        torch.cuda.set_rng_state(call.rng, device)
    else:
        torch.set_rng_state(call.rng)
    out = m(*args, **kwargs) if nn is None else _functional(call, m, args, kwargs, nn)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    again = Call(call.name, call.index, m)
    again.outputs = [keep(o) for o in outs]
    again.buffers_after = {k: keep(b) for k, b in m.named_buffers(recurse=False)}
    again.saved = _saved_vectors(outs[0]) if call.saved else []
    if call.grad_out:
        idx = sorted(call.grad_out)
        torch.autograd.backward([outs[i] for i in idx], [keep(call.grad_out[i]) for i in idx])
    again.grad_in = {key: keep(t.grad) for key, t in fresh.items() if t.grad is not None}
    again.param_grads = {k: keep(p.grad) for k, p in m.named_parameters(recurse=False) if p.grad is not None}
    return again


def compare_calls(call, again, same):
    """Everything ``replay`` returns against the record, by ``same(name, got, want)``; the key sets must agree."""
    tag = f'{call.name}#{call.index}'
    assert len(call.outputs) == len(again.outputs), tag
    for i, (a, b) in enumerate(zip(again.outputs, call.outputs)):
        same(f'{tag} output {i}', a, b)
    for kind in ('grad_in', 'param_grads', 'buffers_after'):
        got, want = getattr(again, kind), getattr(call, kind)
        assert sorted(map(str, got)) == sorted(map(str, want)), (tag, kind, sorted(map(str, got)), sorted(map(str, want)))
        for key in want:
            same(f'{tag} {kind} {key}', got[key], want[key])
    assert len(call.saved) == len(again.saved), tag
    for i, (a, b) in enumerate(zip(again.saved, call.saved)):
        same(f'{tag} saved vector {i}', a, b)


def assert_same_bits(name, got, want):
    assert same_bits(got, want), (name, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape),
                                  float((got.double() - want.double()).abs().max()) if got.shape == want.shape else None)


def assert_close64(name, got, want):
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12, msg=lambda m: f'{name}: {m}')


# ---- tensors with several consumers

def fan_out(rec):
    """{(producer name, call index, output index): [(consumer name, call index, operand key), ...]} as the recorder found them, by
    the identity of the tensor objects (before the alias), for every output that some recorded call read."""
    made = {}
    for call in rec.calls:
        for i, o in enumerate(call.out_refs):
            made.setdefault(id(o), (call.name, call.index, i))
    found = {}
    for call in rec.calls:
        for key, t in call.inputs.items():
            if id(t) in made:
                found.setdefault(made[id(t)], []).append((call.name, call.index, key))
    return found


def gamma(n, u):
    return n * u / (1 - n * u)


def judge_fan_out(name, got, shares):
    """The gradient a producer received against the fp64 sum of the recorded shares: within k - 1 roundings (of the dtype the sum is
    held in: the shares') of the sum of the absolute shares, elementwise; in fp64 to 1e-12.  -> the largest fraction of the bound
    used."""
    assert len(shares) >= 1 and all(s.shape == got.shape for s in shares), (name, [tuple(s.shape) for s in shares], tuple(got.shape))
    assert all(s.dtype == got.dtype for s in shares), (name, got.dtype, [s.dtype for s in shares])
    total = sum(s.double().cpu() for s in shares)
    S = sum(s.double().cpu().abs() for s in shares)
    err = (got.double().cpu() - total).abs()
    if got.dtype == torch.float64:
        tol = 1e-12 * (1 + S)
    else:
        tol = gamma(len(shares) - 1, U_OF[got.dtype]) * S
    bad = err > tol
    assert not bool(bad.any()), f'{name}: {int(bad.sum())} / {err.numel()} elements are not the sum of the {len(shares)} shares ' \
                                f'(largest error {float(err.max()):.3e}, bound there {float(tol.reshape(-1)[int(err.argmax())]):.3e})'
    return float((err / tol.clamp_min(1e-300)).max()) if len(shares) > 1 else 0.


def judge_routes(rec, routes, same=assert_same_bits):
    """``routes``: [((producer, call index, output index), (consumer, call index, key))]: what the consumer saw is what the producer
    wrote."""
    for (pn, pi, po), (cn, ci, key) in routes:
        same(f'{pn}#{pi} -> {cn}#{ci} operand {key}', rec.get(cn, ci).operands[key], rec.get(pn, pi).outputs[po])


# ---- a norm's buffers

def batch_statistics64(x):
    """-> (mean, unbiased variance) per channel of the input a norm saw, in fp64."""
    x = x.double().cpu()
    return x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=True)


def judge_buffers(call, within):
    """One training-mode call of a norm moved ``num_batches_tracked`` by exactly one and the running statistics by exactly one
    update with the module's momentum from the statistics of the recorded input, by ``within(name, got, want64, scale)`` (scale: the
    sum of the absolute terms of the update)."""
    m, before, after = call.module, call.buffers_before, call.buffers_after
    tag = f'{call.name}#{call.index}'
    assert int(after['num_batches_tracked']) == int(before['num_batches_tracked']) + 1, (tag, after['num_batches_tracked'])
    mean, var = batch_statistics64(call.operands[0])
    f = m.momentum
    for key, stat in (('running_mean', mean), ('running_var', var)):
        old = before[key].double().cpu()
        within(f'{tag} {key}', after[key].double().cpu(), (1 - f) * old + f * stat, (1 - f) * old.abs() + f * stat.abs())
