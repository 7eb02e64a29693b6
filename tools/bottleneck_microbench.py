"""Times the pieces of the trainable bottleneck block (celldetection_amd.nn: batch_norm(..., residual=), strided_conv1x1,
Bottleneck / convert_bottleneck_) against what they replace on one MI355X and writes profiles/bottleneck.txt.

    python tools/bottleneck_microbench.py [--out profiles/bottleneck.txt] [--rounds 7] [--reps 3] [--parts tail,strided,block]
    python tools/bottleneck_microbench.py --bn-child          (one process of the old-against-new comparison; prints one JSON line)
    python tools/bottleneck_microbench.py --bn-ab PARENT_TREE (starts such children in turn: on the package and library of a built
                                                               checkout of the parent commit, on this tree's, twice)

Shapes are those of a ResNeXt encoder at an 8 x 512^2 input: the block outputs 256 x 128^2, 512 x 64^2, 1024 x 32^2, 2048 x 16^2 and
the three stride-2 stage entries.  Everything is bf16 channels-last; all versions run in one process and alternate round by round;
every number is the median over the rounds of a HIP-event time around `reps` back-to-back calls after a warm-up.  The yardstick is
a 16-byte-per-lane copy of the same tensor (1 read + 1 write): each new kernel's time is divided by the time that rate needs for
the kernel's bytes (3 passes for the apply, 4 for the masked sum, 1 1/4 of the input for the subsample).  There is no CPU
fallback: without a GPU the script fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get('CPN_MICROBENCH_TREE') or ROOT)  # (--bn-ab: the tree whose package and library a child loads)
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402

N = 8
STAGES = [(256, 128), (512, 64), (1024, 32), (2048, 16)]  # (channels of the block's output, its size)
ENTRIES = [(256, 512, 128), (512, 1024, 64), (1024, 2048, 32)]  # (cin, cout, input size) of the stride-2 stage entries
EPS = 1e-5
CL = torch.channels_last
# compiled for gfx950 with -Rpass-analysis=kernel-resource-usage (bf16 / fp32 instantiation): no scratch in any of them
RESOURCES = ['bn_apply_residual_kernel    VGPRs 36 / 40 (with ReLU; 31 / 40 without), scratch 0, occupancy 8 waves / SIMD',
             'bn_sum_residual_kernel      VGPRs 66 / 80, scratch 0, occupancy 5 waves / SIMD',
             'gc_subsample_kernel         VGPRs 10, scratch 0, occupancy 8 waves / SIMD']


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(calls, rounds, reps):
    for fn in calls.values():  # warm-up: code objects, the stock library's kernel choice, the allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(rounds):  # alternating: every round times every call once
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    return {key: statistics.median(v) for key, v in times.items()}, {key: (min(v), max(v)) for key, v in times.items()}


def rand(*shape, seed=0, grad=False):
    g = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.randn(*shape, device='cuda', generator=g).to(torch.bfloat16)
    t = t.contiguous(memory_format=CL) if t.dim() == 4 else t
    return t.requires_grad_(grad)


def line(label, med, spread, key, extra=''):
    return f'  {label:<26s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]{extra}'


def copy_pair(x):
    y = torch.empty_like(x)
    return [t.permute(0, 2, 3, 1).reshape(-1).view(torch.complex128) for t in (x, y)]  # the NHWC memory as 16-byte elements


def bench_tail(c, size, rounds, reps):
    nn, lib = cda.nn, _lib.load()
    x, r, dy = rand(N, c, size, size, seed=1), rand(N, c, size, size, seed=2), rand(N, c, size, size, seed=3)
    wt, b = torch.randn(c, device='cuda').requires_grad_(True), torch.randn(c, device='cuda').requires_grad_(True)
    w2, b2 = wt.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    rm, rv, rm2, rv2 = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda'), torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    xo, ro, xs, rs = (t.clone().requires_grad_(True) for t in (x, r, x, r))
    m, tensor_bytes = N * size * size, x.numel() * 2
    y, g = torch.empty_like(x), torch.empty_like(x)
    src16, dst16 = copy_pair(x)
    coeffs, abc = torch.empty(4, c, device='cuda'), torch.empty(3, c, device='cuda')
    dg, db = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    nbytes = int(lib.cpn_bn_workspace_bytes(m, c, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    p, st = _lib.ptr, _lib.stream_ptr
    _lib.check(lib.cpn_bn_train_stats(p(x), 1, m, c, 0, p(wt.detach()), 0, p(b.detach()), 0, None, None, 0, .1, EPS, p(coeffs[0]),
                                      p(coeffs[1]), p(coeffs[2]), p(coeffs[3]), p(ws), nbytes, st()), 'stats')

    def k_apply():
        _lib.check(lib.cpn_residual_bn_apply(p(x), p(r), p(y), 1, m, c, 0, p(coeffs[2]), p(coeffs[3]), 1, st()), 'apply')

    def k_sum():
        _lib.check(lib.cpn_residual_bn_backward_reduce(p(x), p(dy), p(y), p(g), 1, m, c, 0, None, None, 1, p(coeffs[0]), p(coeffs[1]),
                                                       p(wt.detach()), 0, p(dg), 0, p(db), 0, p(abc), p(ws), nbytes, st()), 'sum')

    def ours_forward():
        nn.batch_norm(xo, rm, rv, wt, b, True, .1, EPS, 'relu', residual=ro)

    def ours_step():
        xo.grad = ro.grad = wt.grad = b.grad = None
        nn.batch_norm(xo, rm, rv, wt, b, True, .1, EPS, 'relu', residual=ro).backward(dy)

    def stock_forward():
        F.relu(F.batch_norm(xs, rm2, rv2, w2, b2, True, .1, EPS) + rs)

    def stock_step():
        xs.grad = rs.grad = w2.grad = b2.grad = None
        F.relu(F.batch_norm(xs, rm2, rv2, w2, b2, True, .1, EPS) + rs).backward(dy)

    calls = {'copy': lambda: dst16.copy_(src16), 'apply': k_apply, 'sum': k_sum, 'forward': ours_forward, 'step': ours_step,
             'stock forward': stock_forward, 'stock step': stock_step}
    med, spread = measure(calls, rounds, reps)
    rate = 2 * tensor_bytes / (med['copy'] * 1e-3)
    out = [f'relu(bn(x) + r), {N} x {c} x {size}^2   (tensor {tensor_bytes / 2 ** 20:.0f} MiB of bf16)',
           line('copy, 16 B / lane', med, spread, 'copy', f'   {rate / 1e12:.2f} TB/s (1 read + 1 write)')]
    for key, label, passes in (('apply', 'apply + residual', 3), ('sum', 'masked sum (+ finalise)', 4)):
        at_copy = passes * tensor_bytes / rate * 1e3
        out.append(line(label, med, spread, key, f'   {passes} passes: {med[key] / at_copy:.2f} of the time at copy rate'))
    for key, label in (('forward', 'forward'), ('step', 'forward + backward'), ('stock forward', 'stock forward'),
                       ('stock step', 'stock fwd + bwd')):
        out.append(line(label, med, spread, key))
    out.append(f'  new / stock: forward {med["forward"] / med["stock forward"]:.2f}, forward + backward '
               f'{med["step"] / med["stock step"]:.2f} (below 1: the new path is faster)')
    return out


def bench_strided(cin, cout, size, rounds, reps):
    nn, lib = cda.nn, _lib.load()
    x, dy = rand(N, cin, size, size, seed=4), rand(N, cout, size // 2, size // 2, seed=5)
    wt = (torch.randn(cout, cin, 1, 1, device='cuda') / cin ** .5).requires_grad_(True)
    w2 = wt.detach().to(torch.bfloat16).requires_grad_(True)  # stock: bf16 parameters, as under autocast
    xo, xs = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    sub = torch.empty(N, cin, size // 2, size // 2, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=CL)
    src16, dst16 = copy_pair(x)
    p, st = _lib.ptr, _lib.stream_ptr

    def k_sub():
        _lib.check(lib.cpn_subsample2d(p(x), N, size, size, cin, 2, p(sub), st()), 'subsample')

    def ours_forward():
        nn.strided_conv1x1(xo, wt)

    def ours_step():
        xo.grad = wt.grad = None
        nn.strided_conv1x1(xo, wt).backward(dy)

    def stock_forward():
        F.conv2d(xs, w2, None, 2)

    def stock_step():
        xs.grad = w2.grad = None
        F.conv2d(xs, w2, None, 2).backward(dy)

    calls = {'copy': lambda: dst16.copy_(src16), 'sub': k_sub, 'forward': ours_forward, 'step': ours_step,
             'stock forward': stock_forward, 'stock step': stock_step}
    med, spread = measure(calls, rounds, reps)
    tensor_bytes = x.numel() * 2
    rate = 2 * tensor_bytes / (med['copy'] * 1e-3)
    at_copy = 1.25 * tensor_bytes / rate * 1e3
    out = [f'strided 1x1 conv, {N} x {cin} x {size}^2 -> {cout} x {size // 2}^2   (input {tensor_bytes / 2 ** 20:.0f} MiB of bf16)',
           line('copy of the input', med, spread, 'copy', f'   {rate / 1e12:.2f} TB/s (1 read + 1 write)'),
           line('subsample', med, spread, 'sub', f'   1 1/4 passes of the input: {med["sub"] / at_copy:.2f} of the time at copy rate')]
    for key, label in (('forward', 'forward'), ('step', 'forward + backward'), ('stock forward', 'stock forward'),
                       ('stock step', 'stock fwd + bwd')):
        out.append(line(label, med, spread, key))
    out.append(f'  new / stock: forward {med["forward"] / med["stock forward"]:.2f}, forward + backward '
               f'{med["step"] / med["stock step"]:.2f} (below 1: the new path is faster)')
    return out


class Block(torch.nn.Module):
    """torchvision's bottleneck layout (ResNeXt 32 x 8d widths: width = out / 2) with a forward of its own."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        t, width = torch.nn, cout // 2
        self.conv1, self.bn1 = t.Conv2d(cin, width, 1, bias=False), t.BatchNorm2d(width)
        self.conv2, self.bn2 = t.Conv2d(width, width, 3, stride, 1, groups=32, bias=False), t.BatchNorm2d(width)
        self.conv3, self.bn3 = t.Conv2d(width, cout, 1, bias=False), t.BatchNorm2d(cout)
        self.relu = t.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = t.Sequential(t.Conv2d(cin, cout, 1, stride, bias=False), t.BatchNorm2d(cout))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out += identity
        return self.relu(out)


def bench_block(cin, cout, size, stride, rounds, reps):
    nn = cda.nn
    x, dy = rand(N, cin, size, size, seed=6), rand(N, cout, size // stride, size // stride, seed=7)
    torch.manual_seed(0)
    nets = {'stock': torch.nn.Sequential(Block(cin, cout, stride))}
    for key in ('four converts', 'convert_bottleneck_'):
        nets[key] = torch.nn.Sequential(Block(cin, cout, stride))
        nets[key].load_state_dict(nets['stock'].state_dict())
    m = nets['four converts']
    nn.convert_conv2d_(m), nn.convert_batchnorm2d_(m), nn.convert_readout_tail_(m), nn.convert_grouped_conv2d_(m)
    assert nn.convert_bottleneck_(nets['convert_bottleneck_'], block_types=(Block,))[0] == ['0']
    nets['stock'] = nets['stock'].to(torch.bfloat16)  # stock: bf16 parameters, as under autocast
    for mod in m.modules():  # ... and so is the strided shortcut the four converts leave stock
        if type(mod) is torch.nn.Conv2d:
            mod.to(torch.bfloat16)
    xs = {key: x.clone().requires_grad_(True) for key in nets}
    for net in nets.values():
        net.cuda().to(memory_format=CL)

    def step(key):
        def fn():
            xs[key].grad = None
            for prm in nets[key].parameters():
                prm.grad = None
            nets[key](xs[key]).backward(dy)
        return fn

    med, spread = measure({key: step(key) for key in nets}, rounds, reps)
    out = [f'one block, forward + backward, {N} x {cin} x {size}^2 -> {cout} x {size // stride}^2, stride {stride}']
    out += [line(key, med, spread, key) for key in nets]
    out.append(f'  convert_bottleneck_ / four converts {med["convert_bottleneck_"] / med["four converts"]:.2f}, '
               f'convert_bottleneck_ / stock {med["convert_bottleneck_"] / med["stock"]:.2f} (below 1: the new path is faster)')
    return out


BN_SHAPES = [(8, 256, 256, 256), (4, 64, 512, 512), (8, 1024, 64, 64)]  # the shapes of profiles/batch_norm.txt


def bn_child(rounds, reps):
    """batch_norm WITHOUT residual on the package this process imported: forward and forward + backward at BN_SHAPES."""
    nn = cda.nn
    result = {}
    for n, c, h, w in BN_SHAPES:
        x, dy = rand(n, c, h, w, seed=1, grad=True), rand(n, c, h, w, seed=2)
        wt, b = torch.randn(c, device='cuda').requires_grad_(True), torch.randn(c, device='cuda').requires_grad_(True)
        rm, rv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')

        def forward():
            nn.batch_norm(x, rm, rv, wt, b, True, .1, EPS, 'relu')

        def step():
            x.grad = wt.grad = b.grad = None
            nn.batch_norm(x, rm, rv, wt, b, True, .1, EPS, 'relu').backward(dy)

        med, _ = measure({'forward': forward, 'step': step}, rounds, reps)
        result[f'{n} x {c} x {h}^2'] = med
    print(json.dumps(result), flush=True)


def bn_ab(parent_tree, rounds, reps):
    """Children in turn: the parent's tree, this one, three times over.  The GPU is opened by the children only."""
    runs = []
    for which, tree in (('parent', parent_tree), ('new', None)) * 3:
        env = dict(os.environ)
        env.pop('CPN_HIP_LIB', None)
        env.pop('CPN_MICROBENCH_TREE', None)
        if tree:
            env['CPN_MICROBENCH_TREE'] = os.path.abspath(tree)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--bn-child', '--rounds', str(rounds), '--reps', str(reps)],
                              env=env, capture_output=True, text=True, timeout=240)
        if done.returncode != 0:
            raise RuntimeError(f'child ({which}) failed with {done.returncode}: {done.stderr[-2000:]}')
        runs.append((which, json.loads(done.stdout.strip().splitlines()[-1])))
    out = ['batch_norm without residual, the parent commit\'s package and library against this tree\'s (processes in turn: parent, new, '
           'three times)']
    inside = True
    for shape in runs[0][1]:
        for key in ('forward', 'step'):
            old = [r[1][shape][key] for r in runs if r[0] == 'parent']
            new = [r[1][shape][key] for r in runs if r[0] == 'new']
            spread, diff = max(old) - min(old), statistics.mean(new) - statistics.mean(old)
            inside = inside and abs(diff) <= spread
            out.append(f'  {shape:<20s} {key:<8s} parent {" / ".join(f"{v:.4f}" for v in old)} ms, new '
                       f'{" / ".join(f"{v:.4f}" for v in new)} ms: new - parent (means) {diff:+.4f} ms, the parent\'s own run-to-run '
                       f'spread {spread:.4f} ms')
    out.append('  every difference lies inside the parent\'s spread' if inside else '  A DIFFERENCE LIES OUTSIDE THE PARENT\'S SPREAD')
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'bottleneck.txt'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--parts', default='tail,strided,block')
    ap.add_argument('--bn-child', action='store_true')
    ap.add_argument('--bn-ab', default=None, metavar='PARENT_TREE')
    args = ap.parse_args()
    if args.bn_ab:
        lines = bn_ab(args.bn_ab, args.rounds, args.reps)
        print('\n'.join(lines))
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if not torch.cuda.is_available():
        raise RuntimeError('bottleneck_microbench needs an MI355X: there is no CPU fallback')
    if args.bn_child:
        return bn_child(args.rounds, args.reps)
    out = [f'The trainable bottleneck block (cda.nn.Bottleneck and its pieces) against what it replaces, training mode, bf16, '
           f'channels-last, one MI355X (torch.cuda.get_device_name: "{torch.cuda.get_device_name(0)}", '
           f'{getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")}, '
           f'{torch.cuda.get_device_properties(0).multi_processor_count} CUs).',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over '
           f'the rounds.', 'tools/bottleneck_microbench.py writes this file.', '', 'Registers of the new kernels:'] + \
          ['  ' + r for r in RESOURCES] + ['']
    parts = args.parts.split(',')
    jobs = []
    if 'tail' in parts:
        jobs += [(bench_tail, (c, s)) for c, s in STAGES]
    if 'strided' in parts:
        jobs += [(bench_strided, e) for e in ENTRIES]
    if 'block' in parts:
        jobs += [(bench_block, (c, c, s, 1)) for c, s in STAGES] + [(bench_block, (cin, cout, s, 2)) for cin, cout, s in ENTRIES]
    for fn, a in jobs:
        lines = fn(*a, rounds=args.rounds, reps=args.reps)
        print('\n'.join(lines), flush=True)
        out += lines + ['']
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
