"""Resized conv and bilinear resize on one MI355X: forward + backward() with every gradient asked for, three versions alternating in
one process, device events around each repeat, median and spread (min ... max) per version.

    python tools/resized_conv_microbench.py [repeats]

  (a) stock torch:         F.conv2d(F.interpolate(x, size, 'bilinear'), w, b, padding=k // 2) in bf16
  (b) the best before:     stock F.interpolate feeding cda.nn.conv2d
  (c) cda.nn.resized_conv2d

Shapes: 7x7 64 -> 64 from 256^2 to 512^2 at 4 and 8 images (the refinement head of CpnResNeXt101UNet), 3x3 256 -> 256 from 64^2 to
128^2; the plane resize on 8 x 2 and 8 x 12 planes from 256^2 to 512^2, stock against cda.nn.bilinear_resize.  Also printed: the time
of each kernel of (c) on its own, the time a copy of the same bytes takes (``Tensor.copy_`` of a contiguous tensor: 16 bytes per
lane), the ratio of the blended weight gradient to ``cpn_conv_wgrad`` on a materialised resize, peak memory above the operands, and
the bytes each version saves for backward (from the saved tensors, not from the allocator).  Prints one JSON line per shape.
"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import celldetection_amd as cda  # noqa: E402

nn = cda.nn


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def alternate(versions, repeats, warmup=3):
    """Every version once per round, in turn -> {name: [ms]}."""
    for _ in range(warmup):
        for fn in versions.values():
            fn()
    out = {k: [] for k in versions}
    for _ in range(repeats):
        for name, fn in versions.items():
            out[name] += timed(fn, 1, warmup=0)
    return out


def saved_bytes(fn):
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        fn()
    return sum(t.numel() * t.element_size() for t in saved)


def peak_above(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def conv_shape(n, c, cout, k, low, high, repeats):
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, c, low, low, generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (torch.randn(cout, c, k, k, generator=g) / (c * k * k) ** .5).to(dev).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(n, cout, high, high, generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    size = (high, high)
    w16, b16 = w.detach().to(torch.bfloat16).requires_grad_(True), b.detach().to(torch.bfloat16).requires_grad_(True)

    def fwd_a():
        return F.conv2d(F.interpolate(x, size=size, mode='bilinear', align_corners=False), w16, b16, padding=k // 2)

    def fwd_b():
        return nn.conv2d(F.interpolate(x, size=size, mode='bilinear', align_corners=False), w, b)

    def fwd_c():
        return nn.resized_conv2d(x, w, b, size)

    def step(fwd):
        def run():
            for t in (x, w, b, w16, b16):
                t.grad = None
            fwd().backward(dy)
        return run

    versions = {'a_stock': step(fwd_a), 'b_interpolate_conv2d': step(fwd_b), 'c_resized_conv2d': step(fwd_c)}
    times = alternate(versions, repeats)
    out = dict(shape=dict(n=n, cin=c, cout=cout, k=k, low=low, high=high), step={k_: summary(v) for k_, v in times.items()})
    out['saved_bytes'] = {name: saved_bytes(f) for name, f in (('a_stock', fwd_a), ('b_interpolate_conv2d', fwd_b), ('c_resized_conv2d', fwd_c))}
    out['peak_bytes_above_operands'] = {name: peak_above(f) for name, f in versions.items()}
    # the kernels of (c) on their own, and the dense weight gradient on a materialised resize
    with torch.no_grad():
        xs, gs = x.detach(), dy
        packed_f, packed_d = nn.pack_weight(w, 'forward'), nn.pack_weight(w, 'dgrad')
        b32 = b.detach().float()
        t = nn._common._run_conv(gs, packed_d, None, cout, c, k)
        big = nn.bilinear_resize(xs, size)
        kernels = {
            'forward (loader blends)': lambda: nn.resize._run_resized_conv(xs, packed_f, b32, c, cout, k, size),
            'forward, dense conv on a materialised resize': lambda: nn._common._run_conv(big, packed_f, b32, c, cout, k),
            'dgrad conv (T)': lambda: nn._common._run_conv(gs, packed_d, None, cout, c, k),
            'bilinear_sum (T -> dx)': lambda: nn.bilinear_resize_backward(t, (low, low)),
            'weight gradient (staging blends)': lambda: nn.resized_conv2d_weight_grad(xs, gs, k),
            'weight gradient, dense on a materialised resize': lambda: nn.conv2d_weight_grad(big, gs, k),
            'stock resize forward': lambda: F.interpolate(xs, size=size, mode='bilinear', align_corners=False),
            'copy of T': lambda: torch.empty_like(t).copy_(t),
            'copy of x': lambda: torch.empty_like(xs).copy_(xs),
        }
        ktimes = alternate(kernels, repeats)
    out['kernels'] = {k_: summary(v) for k_, v in ktimes.items()}
    out['wgrad_ratio_blended_over_dense'] = round(statistics.median(ktimes['weight gradient (staging blends)']) /
                                                  statistics.median(ktimes['weight gradient, dense on a materialised resize']), 3)
    spread_b = max(times['b_interpolate_conv2d']) - min(times['b_interpolate_conv2d'])
    out['c_minus_b_ms'] = round(statistics.median(times['c_resized_conv2d']) - statistics.median(times['b_interpolate_conv2d']), 4)
    out['b_spread_ms'] = round(spread_b, 4)
    return out


def plane_shape(n, c, low, high, repeats):
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, c, low, low, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(n, c, high, high, generator=g).to(dev)
    size = (high, high)

    def step(fwd):
        def run():
            x.grad = None
            fwd().backward(dy)
        return run

    versions = {'stock': step(lambda: F.interpolate(x, size=size, mode='bilinear', align_corners=False)),
                'bilinear_resize': step(lambda: nn.bilinear_resize(x, size))}
    times = alternate(versions, repeats)
    with torch.no_grad():
        kernels = {'forward': lambda: nn.bilinear_resize(x.detach(), size), 'bilinear_sum_f32': lambda: nn.bilinear_resize_backward(dy, (low, low)),
                   'copy of the large planes': lambda: torch.empty_like(dy).copy_(dy)}
        ktimes = alternate(kernels, repeats)
    return dict(shape=dict(planes=n * c, low=low, high=high), step={k_: summary(v) for k_, v in times.items()},
                kernels={k_: summary(v) for k_, v in ktimes.items()})


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    if not torch.cuda.is_available():
        raise SystemExit('resized_conv_microbench needs the GPU: a CPU run says nothing about these times')
    for args in ((4, 64, 64, 7, 256, 512), (8, 64, 64, 7, 256, 512), (8, 256, 256, 3, 64, 128)):
        print(json.dumps(conv_shape(*args, repeats)), flush=True)
    for args in ((8, 2, 256, 512), (8, 12, 256, 512)):
        print(json.dumps(plane_shape(*args, repeats)), flush=True)


if __name__ == '__main__':
    main()
