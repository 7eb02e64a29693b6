"""Times the trainable conv (celldetection_amd.nn) against stock torch.nn.functional.conv2d forward + backward() on one MI355X and
writes the table of profiles/conv_train.txt.

    python tools/conv_train_microbench.py [--out profiles/conv_train.txt] [--rounds 10] [--reps 5] [--shapes 0,1,2,3]

Both paths run in the same process, alternating round by round, on the same operands (bf16, channels-last; fp32 parameters for the
new path, their bf16 rounding for the stock one).  Every number is the median over the rounds of a HIP-event time around `reps`
back-to-back calls, after a warm-up of every call at the shape.  Per shape: forward, dgrad, wgrad (with the bias gradient) and the
two weight packs of the new path in ms, each conv's fraction of 2.5 PFLOP/s (2 N H W Cin Cout k k FLOP over its time: a whole-call
rate, not a kernel's share of peak), the whole autograd step of the new path, and the stock forward and backward().  There is no CPU
fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402

PEAK = 2.5e15
# (name, N, H, W, Cin, Cout, k)
SHAPES = [('7x7 256->256 at 8 x 256^2', 8, 256, 256, 256, 256, 7),
          ('3x3 320->256 at 8 x 256^2', 8, 256, 256, 320, 256, 3),
          ('7x7 64->64 at 4 x 512^2', 4, 512, 512, 64, 64, 7),
          ('1x1 2048->1024 at 8 x 64^2', 8, 64, 64, 2048, 1024, 1)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(name, n, h, w, cin, cout, k, rounds, reps):
    nn = cda.nn
    g = torch.Generator(device='cuda').manual_seed(0)
    cl = torch.channels_last
    x = torch.randn(n, cin, h, w, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(n, cout, h, w, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    wt = (torch.randn(cout, cin, k, k, device='cuda', generator=g) / (cin * k * k) ** .5).requires_grad_(True)
    b = torch.randn(cout, device='cuda', generator=g).requires_grad_(True)
    w16 = wt.detach().to(torch.bfloat16).contiguous(memory_format=cl).requires_grad_(True)
    b16 = b.detach().to(torch.bfloat16).requires_grad_(True)
    xs = x.clone().requires_grad_(True)   # stock input (a leaf that wants its gradient)
    xo = x.clone().requires_grad_(True)   # the new path's
    pf, pd = nn.pack_weight(wt, 'forward'), nn.pack_weight(wt, 'dgrad')
    b32 = b.detach()
    state = {}

    def ours_step():
        xo.grad = wt.grad = b.grad = None
        nn.conv2d(xo, wt, b).backward(dy)

    def stock_forward():
        state['y'] = torch.nn.functional.conv2d(xs, w16, b16, padding=k // 2)

    def stock_backward():
        xs.grad = w16.grad = b16.grad = None
        state['y'].backward(dy, retain_graph=True)

    calls = {
        'pack': lambda: (nn.pack_weight(wt, 'forward'), nn.pack_weight(wt, 'dgrad')),
        'forward': lambda: nn._common._run_conv(x, pf, b32, cin, cout, k),
        'dgrad': lambda: nn._common._run_conv(dy, pd, None, cout, cin, k),
        'wgrad': lambda: nn.conv2d_weight_grad(x, dy, k),
        'step': ours_step,
        'stock forward': stock_forward,
        'stock backward': stock_backward,
    }
    for fn in calls.values():  # warm-up: code objects, the stock library's algorithm search, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(rounds):  # alternating: every round times every call once
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    med = {key: statistics.median(v) for key, v in times.items()}
    spread = {key: (min(v), max(v)) for key, v in times.items()}
    # same operands, same results (bf16 outputs against each other; the gradients against the stock bf16 ones)
    y_ours = nn._common._run_conv(x, pf, b32, cin, cout, k).float()
    stock_forward()
    rel = float((y_ours - state['y'].detach().float()).abs().max() / state['y'].detach().float().abs().max())
    flop = 2. * n * h * w * cin * cout * k * k
    info = nn.weight_grad_info(n, h, w, cin, cout, k)
    lines = [f'{name}   (N {n}, H {h}, W {w}, Cin {cin}, Cout {cout}, k {k}; {flop / 1e9:.1f} GFLOP per conv; wgrad: {info["slabs"]} slabs of '
             f'{info["slab_rows"]} rows)']
    for key in ('forward', 'dgrad', 'wgrad'):
        lines.append(f'  {key:<15s} {med[key]:9.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]   {flop / (med[key] * 1e-3) / PEAK:6.3f} of 2.5 PFLOP/s')
    lines.append(f'  {"pack (both)":<15s} {med["pack"]:9.3f} ms  [{spread["pack"][0]:.3f} .. {spread["pack"][1]:.3f}]')
    lines.append(f'  {"step (autograd)":<15s} {med["step"]:9.3f} ms  [{spread["step"][0]:.3f} .. {spread["step"][1]:.3f}]   forward + backward() of cda.nn.conv2d')
    stock = med['stock forward'] + med['stock backward']
    for key in ('stock forward', 'stock backward'):
        lines.append(f'  {key:<15s} {med[key]:9.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]')
    lines.append(f'  stock forward + backward {stock:.3f} ms; new step / stock = {med["step"] / stock:.2f} (below 1: the new path is faster); '
                 f'forward {med["forward"] / med["stock forward"]:.2f}, backward {(med["step"] - med["forward"]) / med["stock backward"]:.2f}')
    lines.append(f'  largest |y - y_stock| / max |y_stock| = {rel:.2e} (two bf16 roundings of the same sums)')
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'conv_train.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='0,1,2,3')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('conv_train_microbench needs an MI355X: there is no CPU fallback')
    out = [f'Trainable conv (cda.nn.conv2d) against stock torch.nn.functional.conv2d + backward(), bf16, channels-last, one {torch.cuda.get_device_name(0)}.',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over the rounds.',
           'tools/conv_train_microbench.py writes this file.', '']
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
