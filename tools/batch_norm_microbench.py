"""Times the fused batch norm + ReLU (celldetection_amd.nn.batch_norm) against stock F.relu(F.batch_norm(...)) on one MI355X and
writes the table of profiles/batch_norm.txt.

    python tools/batch_norm_microbench.py [--out profiles/batch_norm.txt] [--rounds 10] [--reps 5] [--shapes 0,1,2]

Both paths run in the same process, alternating round by round, on the same operands (bf16, channels-last, fp32 parameters,
training mode).  Every number is the median over the rounds of a HIP-event time around `reps` back-to-back calls, after a warm-up
of every call at the shape.  Per shape: a 16-byte-per-lane copy of the same tensor (torch's copy of the bytes viewed as 16-byte
elements: 1 read + 1 write), which gives the copy rate every kernel is held against; each of the four launches of the new path with
the bytes it must move (statistics 1 pass over the tensor, apply 2, backward reduce 2, backward input 3) and its time divided by the
time the copy rate needs for those bytes (1.00 = copy rate); forward and forward + backward() of both paths; the peak memory of
one forward + backward() above the operands.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402

# (name, N, H, W, C)
SHAPES = [('8 x 256^2 x 256', 8, 256, 256, 256), ('4 x 512^2 x 64', 4, 512, 512, 64), ('8 x 64^2 x 1024', 8, 64, 64, 1024)]
EPS = 1e-5


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench_shape(name, n, h, w, c, rounds, reps):
    nn = cda.nn
    lib = _lib.load()
    g = torch.Generator(device='cuda').manual_seed(0)
    cl = torch.channels_last
    x = torch.randn(n, c, h, w, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(n, c, h, w, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    wt = torch.randn(c, device='cuda', generator=g).requires_grad_(True)
    b = torch.randn(c, device='cuda', generator=g).requires_grad_(True)
    w16, b16 = wt.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    rm, rv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    rm2, rv2 = rm.clone(), rv.clone()
    xo, xs = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    m, tensor_bytes = n * h * w, x.numel() * 2
    y, dx = torch.empty_like(x), torch.empty_like(x)
    src16, dst16 = (t.permute(0, 2, 3, 1).view(-1).view(torch.complex128) for t in (x, y))  # the NHWC memory as 16-byte elements
    coeffs, abc = torch.empty(4, c, device='cuda'), torch.empty(3, c, device='cuda')
    dg, db = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    nbytes = int(lib.cpn_bn_workspace_bytes(m, c, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    p, st = _lib.ptr, _lib.stream_ptr
    wd, bd = wt.detach(), b.detach()
    state = {}

    def k_stats():
        _lib.check(lib.cpn_bn_train_stats(p(x), 1, m, c, 0, p(wd), 0, p(bd), 0, p(rm), p(rv), 0, .1, EPS, p(coeffs[0]), p(coeffs[1]),
                                          p(coeffs[2]), p(coeffs[3]), p(ws), nbytes, st()), 'stats')

    def k_apply():
        _lib.check(lib.cpn_bn_apply(p(x), p(y), 1, m, c, 0, p(coeffs[2]), p(coeffs[3]), 1, st()), 'apply')

    def k_reduce():
        _lib.check(lib.cpn_bn_backward_reduce(p(x), p(dy), 1, m, c, 0, p(coeffs[2]), p(coeffs[3]), 1, p(coeffs[0]), p(coeffs[1]), p(wd),
                                              0, p(dg), 0, p(db), 0, p(abc), p(ws), nbytes, st()), 'reduce')

    def k_input():
        _lib.check(lib.cpn_bn_backward_input(p(x), p(dy), p(dx), 1, m, c, 0, p(coeffs[2]), p(coeffs[3]), 1, p(abc[0]), p(abc[1]),
                                             p(abc[2]), st()), 'input')

    def ours_forward():
        state['yo'] = nn.batch_norm(xo, rm, rv, wt, b, True, .1, EPS, 'relu')

    def ours_step():
        xo.grad = wt.grad = b.grad = None
        nn.batch_norm(xo, rm, rv, wt, b, True, .1, EPS, 'relu').backward(dy)

    def stock_forward():
        state['ys'] = F.relu(F.batch_norm(xs, rm2, rv2, w16, b16, True, .1, EPS))

    def stock_step():
        xs.grad = w16.grad = b16.grad = None
        F.relu(F.batch_norm(xs, rm2, rv2, w16, b16, True, .1, EPS)).backward(dy)

    calls = {'copy': lambda: dst16.copy_(src16), 'statistics': k_stats, 'apply': k_apply, 'backward reduce': k_reduce,
             'backward input': k_input, 'forward': ours_forward, 'step': ours_step, 'stock forward': stock_forward,
             'stock step': stock_step}
    for fn in calls.values():  # warm-up: code objects, the stock library's kernel choice, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(rounds):  # alternating: every round times every call once
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    med = {key: statistics.median(v) for key, v in times.items()}
    spread = {key: (min(v), max(v)) for key, v in times.items()}
    rate = 2 * tensor_bytes / (med['copy'] * 1e-3)  # bytes / s of the copy
    ours_forward()
    stock_forward()
    rel = float((state['yo'].detach().float() - state['ys'].detach().float()).abs().max() / state['ys'].detach().float().abs().max())
    state.clear()
    peak_ours, peak_stock = peak_above(ours_step), peak_above(stock_step)
    info = nn.batch_norm_info(m, c)
    lines = [f'{name}   (N {n}, H {h}, W {w}, C {c}; tensor {tensor_bytes / 2 ** 20:.0f} MiB of bf16; {info["slabs"]} slabs of '
             f'{info["slab_pixels"]} pixels, {info["rows"]} pixels per step, {info["channel_blocks"]} channel block(s))',
             f'  {"copy, 16 B / lane":<18s} {med["copy"]:8.3f} ms  [{spread["copy"][0]:.3f} .. {spread["copy"][1]:.3f}]   '
             f'{rate / 1e12:.2f} TB/s (1 read + 1 write)']
    for key, passes in (('statistics', 1), ('apply', 2), ('backward reduce', 2), ('backward input', 3)):
        at_copy = passes * tensor_bytes / rate * 1e3
        lines.append(f'  {key:<18s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]   {passes} pass(es), '
                     f'{passes * tensor_bytes / 2 ** 20:.0f} MiB: {med[key] / at_copy:.2f} of the time at copy rate')
    for key, label in (('forward', 'forward'), ('step', 'forward + backward'), ('stock forward', 'stock forward'),
                       ('stock step', 'stock fwd + bwd')):
        lines.append(f'  {label:<18s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]')
    lines.append(f'  new / stock: forward {med["forward"] / med["stock forward"]:.2f}, forward + backward '
                 f'{med["step"] / med["stock step"]:.2f} (below 1: the new path is faster)')
    lines.append(f'  peak memory of forward + backward above the operands: new {peak_ours / 2 ** 20:.0f} MiB, stock '
                 f'{peak_stock / 2 ** 20:.0f} MiB')
    lines.append(f'  largest |y - y_stock| / max |y_stock| = {rel:.2e}')
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'batch_norm.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='0,1,2')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('batch_norm_microbench needs an MI355X: there is no CPU fallback')
    out = [f'Fused batch norm + ReLU (cda.nn.batch_norm) against stock F.relu(F.batch_norm(...)), training mode, bf16, channels-last, '
           f'one MI355X (torch.cuda.get_device_name: "{torch.cuda.get_device_name(0)}", '
           f'{getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")}, '
           f'{torch.cuda.get_device_properties(0).multi_processor_count} CUs).',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over '
           f'the rounds.', 'tools/batch_norm_microbench.py writes this file.', '']
    for i in (int(s) for s in args.shapes.split(',')):
        lines = bench_shape(*SHAPES[i], rounds=args.rounds, reps=args.reps)
        print('\n'.join(lines), flush=True)
        out += lines + ['']
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
