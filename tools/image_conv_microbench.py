"""Times the trainable image conv against stock torch on one MI355X and writes the table of profiles/image_conv.txt.

    python tools/image_conv_microbench.py [--out profiles/image_conv.txt] [--rounds 7] [--reps 3]

At 8 x 3 x 512^2 -> 64, 4 x 3 x 512^2 -> 64, 8 x 1 x 512^2 -> 32 and 8 x 3 x 256^2 -> 128, bf16 channels-last:
(a) stock ``F.conv2d(x, w, b, stride=1, padding=1)`` forward + ``backward()`` against ``cda.nn.image_conv2d``, and both forwards alone;
(b) each launch of the new path alone (pad, pack, the forward kernel, the weight gradient) against a 16-byte-per-lane copy of the
    bytes it must move, and the peak of allocated memory above the operands during one step;
(c) the chain conv -> norm -> ReLU -> conv -> norm -> ReLU of the encoder's level 0, stock modules in bf16 against the converted ones.
All versions run in the same process, alternating round by round, on the same operands.  Every number is the median over the rounds
of a HIP-event time around `reps` back-to-back calls, after a warm-up of every version; [min .. max] is the spread over the rounds.
There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd.nn import image_conv as ic  # noqa: E402

CL = torch.channels_last
nn = cda.nn
CASES = ((8, 3, 512, 64), (4, 3, 512, 64), (8, 1, 512, 32), (8, 3, 256, 128))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_above_operands(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def alternate(versions, rounds, reps):
    """{name: fn} -> {name: (median, min, max)} in ms, the versions taking turns round by round after one warm-up each."""
    for fn in versions.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in versions}
    for _ in range(rounds):
        for name, fn in versions.items():
            times[name].append(timed(fn, reps))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def fmt(t):
    return f'{t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]'


def copy_rate(nbytes, rounds, reps):
    """Time of a 16-byte-per-lane copy that reads and writes nbytes in all (torch's contiguous copy of a bf16 tensor)."""
    src = torch.empty(max(nbytes // 4, 8), dtype=torch.bfloat16, device='cuda').normal_()
    dst = torch.empty_like(src)
    return alternate({'copy': lambda: dst.copy_(src)}, rounds, reps)['copy']


def step(fn, params, dy):
    def run():
        for p in params:
            p.grad = None
        fn().backward(dy)
    return run


def bench_conv(n, c, size, cout, rounds, reps, out):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(n, c, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    w = (torch.randn(cout, c, 3, 3, device='cuda', generator=g) / 5).requires_grad_(True)
    b = torch.randn(cout, device='cuda', generator=g).requires_grad_(True)
    wb = w.detach().to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    bb = b.detach().to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(n, cout, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    out(f'\n== image conv: 3x3 stride 1, {n} x {c} x {size}^2 -> {cout} x {size}^2, bf16 channels-last, with a bias')
    versions = {'(a) stock F.conv2d fwd+bwd': step(lambda: F.conv2d(x, wb, bb, 1, 1), [wb, bb], dy),
                '(a) cda.nn.image_conv2d fwd+bwd': step(lambda: nn.image_conv2d(x, w, b), [w, b], dy),
                'stock forward alone': lambda: F.conv2d(x, wb.detach(), bb.detach(), 1, 1),
                'image_conv2d forward alone': lambda: nn.image_conv2d(x, w.detach(), b.detach())}
    res = alternate(versions, rounds, reps)
    for name, t in res.items():
        out(f'  {name:36s} {fmt(t)}')
    out(f'  ratio fwd+bwd new / stock: {res["(a) cda.nn.image_conv2d fwd+bwd"][0] / res["(a) stock F.conv2d fwd+bwd"][0]:.2f}'
        f'   forward alone new / stock: {res["image_conv2d forward alone"][0] / res["stock forward alone"][0]:.2f}')
    for name, fn in list(versions.items())[:2]:
        out(f'  peak memory above the operands, {name}: {peak_above_operands(fn):.1f} MiB')
    # (b) each launch alone
    xq = ic._image_pad(x)
    packed = nn.image_pack_weight(w)
    b32 = b.detach().float()
    size3 = (n, size, size)
    pieces = {'pad + convert the input': (lambda: ic._image_pad(x), x.numel() * 4 + xq.numel() * 2),
              'pack the weight': (lambda: nn.image_pack_weight(w), w.numel() * 4 + packed.numel() * 2),
              'forward kernel': (lambda: ic._image_forward(xq, size3, packed, b32), xq.numel() * 2 + dy.numel() * 2),
              'weight gradient (slabs + reduce)': (lambda: ic._image_wgrad(xq, size3, c, dy, 0, True, False, torch.float32, torch.float32),
                                                   xq.numel() * 2 + dy.numel() * 2),
              'weight and bias gradient': (lambda: ic._image_wgrad(xq, size3, c, dy, 0, True, True, torch.float32, torch.float32),
                                           xq.numel() * 2 + 2 * dy.numel() * 2)}
    for name, (fn, nbytes) in pieces.items():
        t = alternate({name: fn}, rounds, reps)[name]
        cp = copy_rate(nbytes, rounds, reps)
        out(f'  {name:36s} {fmt(t)}   copy of its {nbytes / 2 ** 20:.1f} MiB: {cp[0]:.3f} ms   ratio {t[0] / cp[0]:.2f}')
    out(f'  weight-gradient partition: {nn.image_weight_grad_info(n, size, size, cout)}')


def bench_chain(n, c, size, cout, rounds, reps, out):
    t = torch.nn

    def make():
        torch.manual_seed(0)
        return t.Sequential(t.Conv2d(c, cout, 3, 1, 1), t.BatchNorm2d(cout), t.ReLU(inplace=True),
                            t.Conv2d(cout, cout, 3, 1, 1), t.BatchNorm2d(cout), t.ReLU(inplace=True)).cuda()

    stock = make().to(torch.bfloat16).to(memory_format=CL)
    ours = make()
    nn.convert_image_conv2d_(ours), nn.convert_conv2d_(ours), nn.convert_batchnorm2d_(ours)
    assert [type(m).__name__ for m in ours] == ['ImageConv2d', 'BatchNorm2d', 'Identity', 'Conv2d', 'BatchNorm2d', 'Identity']
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(n, c, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    dy = torch.randn(n, cout, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    out(f'\n== chain conv -> norm -> ReLU -> conv -> norm -> ReLU: {n} x {c} x {size}^2 -> {cout} x {size}^2, training mode, forward + backward()')
    versions = {'(c) stock modules, bf16': step(lambda: stock(x), list(stock.parameters()), dy),
                '(c) converted modules': step(lambda: ours(x), list(ours.parameters()), dy)}
    res = alternate(versions, rounds, reps)
    for name, tm in res.items():
        out(f'  {name:36s} {fmt(tm)}')
    out(f'  ratio new / stock: {res["(c) converted modules"][0] / res["(c) stock modules, bf16"][0]:.2f}')
    for name, fn in versions.items():
        out(f'  peak memory above the operands, {name}: {peak_above_operands(fn):.1f} MiB')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f'tools/image_conv_microbench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: medians of {args.rounds} rounds of '
        f'{args.reps} calls, [min .. max] over the rounds, versions alternating in one process')
    for case in CASES:
        bench_conv(*case, args.rounds, args.reps, out)
    for case in CASES:
        bench_chain(*case, args.rounds, args.reps, out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
