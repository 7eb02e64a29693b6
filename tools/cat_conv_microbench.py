"""Times the first conv of a U-Net decoder level -- nearest resize + concat + conv, forward + backward() -- in three versions on one
MI355X and writes the table of profiles/cat_conv.txt.

    python tools/cat_conv_microbench.py [--out profiles/cat_conv.txt] [--rounds 7] [--reps 3] [--shapes 0,1,2,3,4]

(a) stock torch: ``F.conv2d(torch.cat((lateral, F.interpolate(top, size=..., mode='nearest')), 1), w, b, padding=1)``;
(b) stock resize + cat feeding ``cda.nn.conv2d`` (the best the library could do before ``cat_conv2d``);
(c) ``cda.nn.cat_conv2d(lateral, top, w, b)``.
The three run in the same process, alternating round by round, on the same operands (bf16, channels-last; fp32 parameters for (b) and
(c), their bf16 rounding for (a)); every input and parameter wants its gradient.  Every number is the median over the rounds of a
HIP-event time around `reps` back-to-back forward + backward() steps, after a warm-up of every version at the shape; [min .. max] is
the spread over the rounds.  The yardstick of (c) is (b) in the same job, its margin (b)'s own spread.  Per shape also: the level's
1x1 inner conv at the low resolution (``cda.nn.conv2d`` before the resize, as ``UNetDecoder`` runs it) against stock's at the high one
(after the resize, as the reference runs it), and the peak of allocated memory above the operands during one step.  The shapes are the
five decoder levels of CpnResNeXt101UNet at 8 x 512^2; they are checked against what ``graph.build_plan`` derives.  There is no CPU
fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import graph  # noqa: E402

BATCH, TILE = 8, 512
# (name, lateral channels (0: bridge), top channels, Cout, output size at 512^2, channels of the inner conv's input (0: Identity))
SHAPES = [('level 4: 3x3 (1024 + 2048) -> 2048 at 32^2', 1024, 2048, 2048, 32, 0),
          ('level 3: 3x3 (512 + 1024) -> 1024 at 64^2', 512, 1024, 1024, 64, 2048),
          ('level 2: 3x3 (256 + 512) -> 512 at 128^2', 256, 512, 512, 128, 1024),
          ('level 1: 3x3 (64 + 256) -> 256 at 256^2', 64, 256, 256, 256, 512),
          ('level 0 (bridge): 3x3 64 -> 64 at 512^2 over the 256^2 map', 0, 64, 64, 512, 256)]


def check_shapes():
    """The table above against the decoder levels of the inference graph (host arithmetic only)."""
    plan = graph.build_plan('ResNeXt101UNet', 3)
    convs = {o['w']: o for o in plan.ops if o['op'] == 'conv' and o.get('sub') is None}
    for level, (name, c0, c1, cout, size, inner) in zip((4, 3, 2, 1, 0), SHAPES):
        o = convs[f'core.backbone.unet.layer_blocks.{level}.0.']
        t0 = plan.tensors[o['src0']]
        got = (o['k'], o['cin'], o['cout'], TILE // plan.tensors[o['dst']]['down'])
        assert got == (3, c0 + c1, cout, size), (name, got)
        if c0:
            t1 = plan.tensors[o['src1']]
            assert (t0['c'], t1['c'], o['up1'], t1['down']) == (c0, c1, True, 2 * t0['down']), (name, t0, t1)
        else:
            assert (t0['c'], o['src1'], o['up0']) == (c1, None, True), (name, t0)
        i = convs.get(f'core.backbone.unet.inner_blocks.{level}.')
        assert (0 if i is None else i['cin']) == inner and (i is None or (i['k'], i['cout']) == (1, c1)), (name, i)


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


def bench_shape(name, c0, c1, cout, size, inner, rounds, reps):
    nn = cda.nn
    g = torch.Generator(device='cuda').manual_seed(0)
    cl = torch.channels_last
    n, k, lo = BATCH, 3, size // 2

    def act(c, s):
        return torch.randn(n, c, s, s, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl).requires_grad_(True)

    lateral = act(c0, size) if c0 else None
    top = act(c1, lo)
    dy = torch.randn(n, cout, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    wt = (torch.randn(cout, c0 + c1, k, k, device='cuda', generator=g) / ((c0 + c1) * k * k) ** .5).requires_grad_(True)
    b = torch.randn(cout, device='cuda', generator=g).requires_grad_(True)
    w16 = wt.detach().to(torch.bfloat16).contiguous(memory_format=cl).requires_grad_(True)
    b16 = b.detach().to(torch.bfloat16).requires_grad_(True)
    leaves = [t for t in (lateral, top, wt, b, w16, b16) if t is not None]

    def concat():
        if lateral is None:
            return F.interpolate(top, scale_factor=2, mode='nearest')
        return torch.cat((lateral, F.interpolate(top, size=lateral.shape[2:], mode='nearest')), 1)

    def clear():
        for t in leaves:
            t.grad = None

    def stock():
        clear()
        F.conv2d(concat(), w16, b16, padding=k // 2).backward(dy)

    def parent():
        clear()
        nn.conv2d(concat(), wt, b).backward(dy)

    def ours():
        clear()
        nn.cat_conv2d(lateral, top, wt, b).backward(dy)

    calls = {'(a) stock': stock, '(b) cat + nn.conv2d': parent, '(c) nn.cat_conv2d': ours}
    if inner:  # the level's inner conv: inner -> c1 channels, at the low resolution (ours) or behind the resize (stock)
        last = act(inner, lo)
        wi = (torch.randn(c1, inner, 1, 1, device='cuda', generator=g) / inner ** .5).requires_grad_(True)
        bi = torch.randn(c1, device='cuda', generator=g).requires_grad_(True)
        wi16 = wi.detach().to(torch.bfloat16).contiguous(memory_format=cl).requires_grad_(True)
        bi16 = bi.detach().to(torch.bfloat16).requires_grad_(True)
        dlo = torch.randn(n, c1, lo, lo, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
        dhi = torch.randn(n, c1, size, size, device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
        leaves += [last, wi, bi, wi16, bi16]

        def inner_stock():
            clear()
            F.conv2d(F.interpolate(last, size=(size, size), mode='nearest'), wi16, bi16).backward(dhi)

        def inner_ours():
            clear()
            nn.conv2d(last, wi, bi).backward(dlo)

        calls['inner 1x1, stock (high res)'] = inner_stock
        calls['inner 1x1, nn.conv2d (low res)'] = inner_ours
    for fn in calls.values():  # warm-up: code objects, the stock library's algorithm search, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(rounds):  # alternating: every round times every version once
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    med = {key: statistics.median(v) for key, v in times.items()}
    spread = {key: (min(v), max(v)) for key, v in times.items()}
    peak = {key: peak_above_operands(fn) for key, fn in calls.items()}
    clear()
    # same operands, same results: (c) against (b), forward and every gradient
    y_c = nn.cat_conv2d(lateral, top, wt, b)
    y_c.backward(dy)
    grads_c = [t.grad.float().clone() for t in (lateral, top, wt, b) if t is not None]
    clear()
    y_b = nn.conv2d(concat(), wt, b)
    y_b.backward(dy)
    grads_b = [t.grad.float() for t in (lateral, top, wt, b) if t is not None]
    rel = [float((y_c.float() - y_b.float()).abs().max() / y_b.float().abs().max())] + \
        [float((p - q).abs().max() / q.abs().max()) for p, q in zip(grads_c, grads_b)]
    clear()
    flop = 2. * n * size * size * (c0 + c1) * cout * k * k
    mb = 2 * n * size * size / 2 ** 20
    lines = [f'{name}   (N {n}; {flop / 1e9:.1f} GFLOP per conv, 3 convs per step; lateral {mb * c0:.0f} MiB, top {mb * c1 / 4:.0f} MiB, resized '
             f'top {mb * c1:.0f} MiB, concat {mb * (c0 + c1):.0f} MiB, output {mb * cout:.0f} MiB)']
    for key in calls:
        lines.append(f'  {key:<32s} {med[key]:9.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]   peak above the operands '
                     f'{peak[key]:8.1f} MiB')
    mb_, mc = med['(b) cat + nn.conv2d'], med['(c) nn.cat_conv2d']
    lo_b, hi_b = spread['(b) cat + nn.conv2d']
    verdict = 'faster' if mc < lo_b else ('slower' if mc > hi_b else "within (b)'s spread")
    lines.append(f'  (c) / (b) = {mc / mb_:.3f}, (c) / (a) = {mc / med["(a) stock"]:.3f} (below 1: cat_conv2d is faster); against (b): {verdict}')
    if inner:
        lines.append(f'  inner conv, low res / stock high res = {med["inner 1x1, nn.conv2d (low res)"] / med["inner 1x1, stock (high res)"]:.3f}')
    lines.append('  largest relative difference (c) - (b): y %.1e, %s' % (rel[0], ', '.join(
        f'd_{nm} {v:.1e}' for nm, v in zip([s for s, t in zip(('lateral', 'top', 'w', 'b'), (lateral, top, wt, b)) if t is not None], rel[1:]))))
    return lines, (name, mb_, (lo_b, hi_b), mc, med['(a) stock'])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'cat_conv.txt'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='0,1,2,3,4')
    args = ap.parse_args()
    check_shapes()
    if not torch.cuda.is_available():
        raise RuntimeError('cat_conv_microbench needs an MI355X: there is no CPU fallback')
    out = [f'First conv of a U-Net decoder level, forward + backward(), bf16, channels-last, one {torch.cuda.get_device_name(0)}: (a) stock '
           f'torch, (b) stock resize + cat feeding cda.nn.conv2d, (c) cda.nn.cat_conv2d.',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} steps, HIP events; [min .. max] over the rounds.',
           'tools/cat_conv_microbench.py writes this file.', '']
    summary = []
    for i in (int(s) for s in args.shapes.split(',')):
        lines, row = bench_shape(*SHAPES[i], rounds=args.rounds, reps=args.reps)
        print('\n'.join(lines), flush=True)
        out += lines + ['']
        summary.append(row)
        torch.cuda.empty_cache()
    out.append('Summary: step time in ms, (c) against (b) and (b)\'s own spread')
    for name, mb_, (lo_b, hi_b), mc, ma in summary:
        out.append(f'  {name:<62s} (a) {ma:8.3f}  (b) {mb_:8.3f} [{lo_b:.3f} .. {hi_b:.3f}]  (c) {mc:8.3f}  (c)/(b) {mc / mb_:.3f}'
                   f'{"  SLOWER than (b)" if mc > hi_b else ""}')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
