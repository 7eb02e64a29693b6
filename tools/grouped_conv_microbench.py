"""Times the trainable grouped 3x3 conv (celldetection_amd.nn.grouped_conv2d) against stock torch.nn.functional.conv2d(groups=32)
forward + backward() on one MI355X and writes the table of profiles/grouped_conv.txt.

    python tools/grouped_conv_microbench.py [--out profiles/grouped_conv.txt] [--rounds 10] [--reps 5] [--shapes 0,1,...,6]

The shapes are the conv2 shapes of ResNeXt101_32x8d at an 8 x 512^2 input (seven distinct ones): 256 / 512 / 1024 / 2048 channels in 32 groups at
128^2 / 64^2 / 32^2 / 16^2 with stride 1, and the three stage-entry convs at stride 2.  Both paths run in the same process,
alternating round by round, on the same operands (bf16, channels-last; fp32 parameters for the new path, their bf16 rounding for the
stock one).  Every number is the median over the rounds of a HIP-event time around `reps` back-to-back calls, after a warm-up of
every call at the shape.  Per shape: forward, dx (the dgrad conv; stride 2: of the dilated gradient), dW (with the bias gradient),
the dilation (stride 2) and the two weight packs of the new path in ms, the whole autograd step of the new path, the stock forward
and backward(), and -- the yardstick of the memory-bound parts -- a 16-byte-per-lane copy (torch's copy of the bytes viewed as 16-byte
elements) of x, of dY and (stride 2) of dZ with the rate it reaches (bytes read + written over its time).  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402

GROUPS = 32
# (name, N, H, W, C, stride): H x W is the conv's INPUT
SHAPES = [('stage 1, 256 ch at 128^2, stride 1', 8, 128, 128, 256, 1),
          ('stage 2 entry, 512 ch at 128^2, stride 2', 8, 128, 128, 512, 2),
          ('stage 2, 512 ch at 64^2, stride 1', 8, 64, 64, 512, 1),
          ('stage 3 entry, 1024 ch at 64^2, stride 2', 8, 64, 64, 1024, 2),
          ('stage 3, 1024 ch at 32^2, stride 1', 8, 32, 32, 1024, 1),
          ('stage 4 entry, 2048 ch at 32^2, stride 2', 8, 32, 32, 2048, 2),
          ('stage 4, 2048 ch at 16^2, stride 1', 8, 16, 16, 2048, 1)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(name, n, h, w, c, stride, rounds, reps):
    nn = cda.nn
    cig = c // GROUPS
    g = torch.Generator(device='cuda').manual_seed(0)
    cl = torch.channels_last
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randn(n, c, h, w, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(n, c, ho, wo, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    wt = (torch.randn(c, cig, 3, 3, device='cuda', generator=g) / (cig * 9) ** .5).requires_grad_(True)
    b = torch.randn(c, device='cuda', generator=g).requires_grad_(True)
    w16 = wt.detach().to(torch.bfloat16).contiguous(memory_format=cl).requires_grad_(True)
    b16 = b.detach().to(torch.bfloat16).requires_grad_(True)
    xs = x.clone().requires_grad_(True)   # stock input (a leaf that wants its gradient)
    xo = x.clone().requires_grad_(True)   # the new path's
    pf, pd = nn.grouped_pack_weight(wt, GROUPS, 'forward'), nn.grouped_pack_weight(wt, GROUPS, 'dgrad')
    dz = nn.grouped_dilate(dy, (h, w)) if stride == 2 else dy
    b32 = b.detach()

    def as16(t):  # the NHWC memory as 16-byte elements: torch's copy then moves 16 bytes per lane
        return t.permute(0, 2, 3, 1).reshape(-1).view(torch.complex128)

    x16, dy16, dz16 = as16(x), as16(dy), as16(dz)
    x2, dy2, dz2 = torch.empty_like(x16), torch.empty_like(dy16), torch.empty_like(dz16)
    state = {}

    def ours_step():
        xo.grad = wt.grad = b.grad = None
        nn.grouped_conv2d(xo, wt, b, stride, GROUPS).backward(dy)

    def stock_forward():
        state['y'] = torch.nn.functional.conv2d(xs, w16, b16, stride, 1, 1, GROUPS)

    def stock_backward():
        xs.grad = w16.grad = b16.grad = None
        state['y'].backward(dy, retain_graph=True)

    calls = {
        'pack': lambda: (nn.grouped_pack_weight(wt, GROUPS, 'forward'), nn.grouped_pack_weight(wt, GROUPS, 'dgrad')),
        'forward': lambda: nn.grouped._run_grouped(x, pf, b32, c, cig, stride),
        'dx': lambda: nn.grouped._run_grouped(dz, pd, None, c, cig, 1),
        'dW': lambda: nn.grouped_conv2d_weight_grad(x, dy, GROUPS, stride, dilated=dz),
        'step': ours_step,
        'stock forward': stock_forward,
        'stock backward': stock_backward,
        'copy x': lambda: x2.copy_(x16),
        'copy dY': lambda: dy2.copy_(dy16),
    }
    if stride == 2:
        calls['dilate'] = lambda: nn.grouped_dilate(dy, (h, w))
        calls['copy dZ'] = lambda: dz2.copy_(dz16)
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
    # same operands, same results (bf16 outputs against each other)
    y_ours = nn.grouped._run_grouped(x, pf, b32, c, cig, stride).float()
    stock_forward()
    rel = float((y_ours - state['y'].detach().float()).abs().max() / state['y'].detach().float().abs().max())
    flop = 2. * n * ho * wo * c * cig * 9
    info = nn.grouped_weight_grad_info(n, h, w, c, GROUPS, stride)
    lines = [f'{name}   (N {n}, H {h}, W {w}, C {c}, {GROUPS} groups of {cig}, stride {stride}; {flop / 1e9:.2f} GFLOP per conv; dW: '
             f'{info["slabs"]} slabs of {info["slab_rows"]} rows)']

    def line(key, label=None, note=''):
        return f'  {label or key:<15s} {med[key]:9.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]{note}'

    nbytes = {'copy x': x.numel() * 4, 'copy dY': dy.numel() * 4, 'copy dZ': dz.numel() * 4}  # 2 bytes read + 2 written
    for key in ('forward', 'dx', 'dW'):
        lines.append(line(key))
    if stride == 2:
        lines.append(line('dilate', note=f'   writes {dz.numel() * 2 / 1e6:.1f} MB, reads {dy.numel() * 2 / 1e6:.1f} MB'))
    lines.append(line('pack', 'pack (both)'))
    lines.append(line('step', 'step (autograd)', '   forward + backward() of cda.nn.grouped_conv2d'))
    stock = med['stock forward'] + med['stock backward']
    for key in ('stock forward', 'stock backward'):
        lines.append(line(key))
    for key in ('copy x', 'copy dY') + (('copy dZ',) if stride == 2 else ()):
        lines.append(line(key, note=f'   {nbytes[key] / 1e6:.1f} MB moved, {nbytes[key] / (med[key] * 1e-3) / 1e12:.2f} TB/s'))
    lines.append(f'  stock forward + backward {stock:.3f} ms; new step / stock = {med["step"] / stock:.2f} (below 1: the new path is faster); '
                 f'forward {med["forward"] / med["stock forward"]:.2f}, backward {(med["step"] - med["forward"]) / med["stock backward"]:.2f}')
    lines.append(f'  largest |y - y_stock| / max |y_stock| = {rel:.2e} (two bf16 roundings of the same sums)')
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'grouped_conv.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default=','.join(str(i) for i in range(len(SHAPES))))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('grouped_conv_microbench needs an MI355X: there is no CPU fallback')
    out = [f'Trainable grouped 3x3 conv (cda.nn.grouped_conv2d) against stock torch.nn.functional.conv2d(groups={GROUPS}) + backward(), bf16, '
           f'channels-last, one {torch.cuda.get_device_name(0)}.',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over the rounds.',
           'tools/grouped_conv_microbench.py writes this file.', '']
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
