"""Times the fused ReadOut tail (celldetection_amd.nn.dropout_conv1x1) against stock F.conv2d(F.dropout2d(x, p, True), w, b) on one
MI355X and writes the table of profiles/readout_tail.txt.

    python tools/readout_tail_microbench.py [--out profiles/readout_tail.txt] [--rounds 10] [--reps 5] [--shapes 0,1,2,3]

Both paths run in the same process, alternating round by round, on the same operands (bf16, channels-last, p = 0.1, training
mode; the new path with fp32 parameters and an fp32 NCHW output, stock with bf16 parameters, as autocast would run it).  Every
number is the median over the rounds of a HIP-event time around `reps` back-to-back calls, after a warm-up of every call at the
shape.  Per shape: a 16-byte-per-lane copy of the same tensor (torch's copy of the bytes viewed as 16-byte elements: 1 read +
1 write), which gives the copy rate the new path is held against -- it must move the tensor three times (forward reads x, backward
reads x and writes dx), the forward once; forward and forward + backward() of both paths with both ratios; the peak memory of one
forward + backward() above the operands.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402

# (name, N, H, W, Cin, Cout)
SHAPES = [('8 x 256^2 x 256 -> 1', 8, 256, 256, 256, 1), ('8 x 256^2 x 256 -> 2', 8, 256, 256, 256, 2),
          ('8 x 256^2 x 256 -> 20', 8, 256, 256, 256, 20), ('4 x 512^2 x 64 -> 2', 4, 512, 512, 64, 2)]
P = .1


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


def bench_shape(name, n, h, w, cin, cout, rounds, reps):
    nn = cda.nn
    g = torch.Generator(device='cuda').manual_seed(0)
    cl = torch.channels_last
    x = torch.randn(n, cin, h, w, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(n, cout, h, w, device='cuda', generator=g)
    dy16 = dy.to(torch.bfloat16).contiguous(memory_format=cl)
    wt = (torch.randn(cout, cin, 1, 1, device='cuda', generator=g) / cin ** .5).requires_grad_(True)
    b = torch.randn(cout, device='cuda', generator=g).requires_grad_(True)
    w16, b16 = (t.detach().to(torch.bfloat16).requires_grad_(True) for t in (wt, b))
    xo, xs = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    tensor_bytes = x.numel() * 2
    y = torch.empty_like(x)
    src16, dst16 = (t.permute(0, 2, 3, 1).view(-1).view(torch.complex128) for t in (x, y))  # the NHWC memory as 16-byte elements
    state = {}

    def ours_forward():
        state['yo'] = nn.dropout_conv1x1(xo, wt, b, P, True)

    def ours_step():
        xo.grad = wt.grad = b.grad = None
        nn.dropout_conv1x1(xo, wt, b, P, True).backward(dy)

    def stock_forward():
        state['ys'] = F.conv2d(F.dropout2d(xs, P, True), w16, b16)

    def stock_step():
        xs.grad = w16.grad = b16.grad = None
        F.conv2d(F.dropout2d(xs, P, True), w16, b16).backward(dy16)

    calls = {'copy': lambda: dst16.copy_(src16), 'forward': ours_forward, 'step': ours_step, 'stock forward': stock_forward,
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
    keep = torch.rand(n, cin, device='cuda', generator=g) >= P  # one mask for both paths: the values agree
    yo = nn.dropout_conv1x1(x, wt.detach(), b.detach(), P, True, keep)
    ys = F.conv2d(x * keep[:, :, None, None].to(x.dtype) / (1 - P), w16.detach(), b16.detach())
    rel = float((yo.float() - ys.float()).abs().max() / ys.float().abs().max())
    state.clear()
    peak_ours, peak_stock = peak_above(ours_step), peak_above(stock_step)
    info = nn.readout_tail_info(n, h * w, cin, cout)
    lines = [f'{name}   (N {n}, H {h}, W {w}, Cin {cin}, Cout {cout}; x {tensor_bytes / 2 ** 20:.0f} MiB of bf16; backward: '
             f'{info["slabs"]} slabs of {info["slab_pixels"]} pixels)',
             f'  {"copy, 16 B / lane":<18s} {med["copy"]:8.3f} ms  [{spread["copy"][0]:.3f} .. {spread["copy"][1]:.3f}]   '
             f'{rate / 1e12:.2f} TB/s (1 read + 1 write)']
    for key, label, passes in (('forward', 'forward', 1), ('step', 'forward + backward', 3)):
        at_copy = passes * tensor_bytes / rate * 1e3
        lines.append(f'  {label:<18s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]   {passes} pass(es) over x, '
                     f'{passes * tensor_bytes / 2 ** 20:.0f} MiB: {med[key] / at_copy:.2f} of the time at copy rate')
    for key, label in (('stock forward', 'stock forward'), ('stock step', 'stock fwd + bwd')):
        lines.append(f'  {label:<18s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]')
    lines.append(f'  new / stock: forward {med["forward"] / med["stock forward"]:.2f}, forward + backward '
                 f'{med["step"] / med["stock step"]:.2f} (below 1: the new path is faster)')
    lines.append(f'  peak memory of forward + backward above the operands: new {peak_ours / 2 ** 20:.0f} MiB, stock '
                 f'{peak_stock / 2 ** 20:.0f} MiB')
    lines.append(f'  largest |y - y_stock| / max |y_stock| on one mask = {rel:.2e}')
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'readout_tail.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='0,1,2,3')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('readout_tail_microbench needs an MI355X: there is no CPU fallback')
    out = [f'Fused ReadOut tail (cda.nn.dropout_conv1x1) against stock F.conv2d(F.dropout2d(x, {P}, True), w, b), training mode, bf16, '
           f'channels-last, one MI355X (torch.cuda.get_device_name: "{torch.cuda.get_device_name(0)}", '
           f'{getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")}, '
           f'{torch.cuda.get_device_properties(0).multi_processor_count} CUs).',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over '
           f'the rounds.', 'tools/readout_tail_microbench.py writes this file.', '']
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
