"""Times the trainable stem and max-pool against stock torch on one MI355X and writes the table of profiles/stem.txt.

    python tools/stem_microbench.py [--out profiles/stem.txt] [--rounds 7] [--reps 3]

At 8 x 3 x 512^2 and 4 x 3 x 512^2, bf16 channels-last, Cout = 64:
(a) stock ``F.conv2d(x, w, stride=2, padding=3)`` forward + ``backward()`` against ``cda.nn.stem_conv2d``;
(b) stock ``F.max_pool2d(h, 3, 2, 1)`` forward + ``backward()`` against ``cda.nn.max_pool2d`` on the stem's output, and both at
    (2, 2, 0) on 8 x 64 x 512^2;
(c) the chain conv -> norm -> ReLU -> pool, stock modules in bf16 against the converted ones;
then each launch of the new path alone against a 16-byte-per-lane copy of the bytes it must move, and the peak of allocated memory
above the operands during one step.  All versions run in the same process, alternating round by round, on the same operands.  Every
number is the median over the rounds of a HIP-event time around `reps` back-to-back calls, after a warm-up of every version;
[min .. max] is the spread over the rounds.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402

CL = torch.channels_last
nn = cda.nn


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


def bench_stem(n, size, rounds, reps, out):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(n, 3, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    w = (torch.randn(64, 3, 7, 7, device='cuda', generator=g) / 12).requires_grad_(True)
    wb = w.detach().to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    ho = (size - 1) // 2 + 1
    dy = torch.randn(n, 64, ho, ho, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    out(f'\n== stem: 7x7 stride 2, {n} x 3 x {size}^2 -> 64 x {ho}^2, bf16 channels-last')
    versions = {'(a) stock F.conv2d fwd+bwd': step(lambda: F.conv2d(x, wb, None, 2, 3), [wb], dy),
                '(a) cda.nn.stem_conv2d fwd+bwd': step(lambda: nn.stem_conv2d(x, w), [w], dy),
                'stock forward alone': lambda: F.conv2d(x, wb.detach(), None, 2, 3),
                'stem_conv2d forward alone': lambda: nn.stem_conv2d(x, w.detach())}
    res = alternate(versions, rounds, reps)
    for name, t in res.items():
        out(f'  {name:36s} {fmt(t)}')
    out(f'  ratio fwd+bwd new / stock: {res["(a) cda.nn.stem_conv2d fwd+bwd"][0] / res["(a) stock F.conv2d fwd+bwd"][0]:.2f}')
    for name, fn in list(versions.items())[:2]:
        out(f'  peak memory above the operands, {name}: {peak_above_operands(fn):.1f} MiB')
    # each launch alone
    xp = nn.stem._stem_pad(x)
    packed = nn.stem_pack_weight(w)
    gs = dy
    pieces = {'pad + convert the input': (lambda: nn.stem._stem_pad(x), x.numel() * 4 + xp.numel() * 2),
              'pack the weight': (lambda: nn.stem_pack_weight(w), w.numel() * 4 + packed.numel() * 2),
              'forward kernel': (lambda: nn.stem._stem_forward(xp, (n, size, size), packed, None), xp.numel() * 2 + dy.numel() * 2),
              'weight gradient (slabs + reduce)': (lambda: nn.stem._stem_wgrad(xp, (n, size, size), 3, gs, 0, True, False, torch.float32, torch.float32),
                                                   xp.numel() * 2 + dy.numel() * 2)}
    for name, (fn, nbytes) in pieces.items():
        t = alternate({name: fn}, rounds, reps)[name]
        c = copy_rate(nbytes, rounds, reps)
        out(f'  {name:36s} {fmt(t)}   copy of its {nbytes / 2 ** 20:.1f} MiB: {c[0]:.3f} ms   ratio {t[0] / c[0]:.2f}')
    out(f'  weight-gradient partition: {nn.stem_weight_grad_info(n, size, size, 64)}')


def bench_pool(n, c, size, geometry, rounds, reps, out):
    k, s, pad = geometry
    g = torch.Generator(device='cuda').manual_seed(1)
    h = torch.randn(n, c, size, size, device='cuda', generator=g).clamp_min(0.).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    ho = (size + 2 * pad - k) // s + 1
    dy = torch.randn(n, c, ho, ho, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    out(f'\n== pool {geometry}: {n} x {c} x {size}^2 -> {ho}^2, bf16 channels-last, post-ReLU input')
    versions = {'(b) stock F.max_pool2d fwd+bwd': step(lambda: F.max_pool2d(h, k, s, pad), [h], dy),
                '(b) cda.nn.max_pool2d fwd+bwd': step(lambda: nn.max_pool2d(h, k, s, pad), [h], dy),
                'stock forward alone': lambda: F.max_pool2d(h.detach(), k, s, pad),
                'max_pool2d forward alone': lambda: nn.max_pool2d(h.detach(), k, s, pad)}
    res = alternate(versions, rounds, reps)
    for name, t in res.items():
        out(f'  {name:36s} {fmt(t)}')
    out(f'  ratio fwd+bwd new / stock: {res["(b) cda.nn.max_pool2d fwd+bwd"][0] / res["(b) stock F.max_pool2d fwd+bwd"][0]:.2f}')
    for name, fn in list(versions.items())[:2]:
        out(f'  peak memory above the operands, {name}: {peak_above_operands(fn):.1f} MiB')
    fwd_bytes = h.numel() * 2 + dy.numel() * 3          # x read, y and the index written
    bwd_bytes = dy.numel() * 3 + h.numel() * 2          # dY and the index read once (the overlap of the windows left to the caches), dx written
    y = nn.max_pool2d(h, k, s, pad)
    pieces = {'forward with index': (lambda: nn.max_pool2d(h.detach(), k, s, pad), fwd_bytes),
              'backward gather': (lambda: torch.autograd.grad(y, h, dy, retain_graph=True), bwd_bytes)}
    for name, (fn, nbytes) in pieces.items():
        t = alternate({name: fn}, rounds, reps)[name]
        cpy = copy_rate(nbytes, rounds, reps)
        out(f'  {name:36s} {fmt(t)}   copy of its {nbytes / 2 ** 20:.1f} MiB: {cpy[0]:.3f} ms   ratio {t[0] / cpy[0]:.2f}')


def bench_chain(n, size, rounds, reps, out):
    t = torch.nn

    def make():
        torch.manual_seed(0)
        return t.Sequential(t.Conv2d(3, 64, 7, 2, 3, bias=False), t.BatchNorm2d(64), t.ReLU(inplace=True), t.MaxPool2d(3, 2, 1)).cuda()

    stock = make().to(torch.bfloat16).to(memory_format=CL)
    ours = make()
    nn.convert_stem_conv2d_(ours), nn.convert_batchnorm2d_(ours), nn.convert_maxpool2d_(ours)
    assert [type(m).__name__ for m in ours] == ['StemConv2d', 'BatchNorm2d', 'Identity', 'MaxPool2d']
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(n, 3, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    ho = ((size - 1) // 2 + 1 - 1) // 2 + 1
    dy = torch.randn(n, 64, ho, ho, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    out(f'\n== chain conv -> norm -> ReLU -> pool: {n} x 3 x {size}^2 -> 64 x {ho}^2, training mode, forward + backward()')
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

    out(f'tools/stem_microbench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: medians of {args.rounds} rounds of {args.reps} '
        f'calls, [min .. max] over the rounds, versions alternating in one process')
    for n in (8, 4):
        bench_stem(n, 512, args.rounds, args.reps, out)
    for n in (8, 4):
        bench_pool(n, 64, 256, (3, 2, 1), args.rounds, args.reps, out)
    bench_pool(8, 64, 512, (2, 2, 0), args.rounds, args.reps, out)
    for n in (8, 4):
        bench_chain(n, 512, args.rounds, args.reps, out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
