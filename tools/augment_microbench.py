"""Times the augmentation warp (celldetection_amd.augment.warp) against stock torch on one MI355X and writes the table of
profiles/augment.txt.

    python tools/augment_microbench.py [--out profiles/augment.txt] [--rounds 10] [--reps 5]

Workload: 8 crops of 512 x 512 from 8 uint8 sources of 1024 x 1024 x 3 with 3 int32 label channels, at a 27 degree rotation and at
the identity (a centred crop), gamma and normalisation folded in, float32 output.  All paths run in the same process, alternating
round by round.  Every number is the median over the rounds of a HIP-event time around `reps` back-to-back calls, after a warm-up
of every call.  Per map:
  the whole call (cda.augment.warp: host checks, one upload of maps and tables, one launch) and its kernel alone (cpn_augment_warp
  on maps and tables already on the device);
  (a) the best stock formulation found: positions from the map by broadcasting in float64, F.grid_sample(bilinear, zeros,
  align_corners=True) on the image converted to float32 NCHW, gamma and normalisation on the warped crop (pow, then one fused
  multiply-add: blend-then-transform, the cheaper order), and for the labels the nearest index from the same positions and one
  torch.gather over [B, H W, C] plus the fill;
  (b) the time the rate of a 16-byte-per-lane copy (torch's copy of 256 MiB viewed as 16-byte elements: 1 read + 1 write) needs for
  the bytes the warp reads and writes: every output element once (B K h w float32 + B h w C int32) and, at these maps of scale 1,
  about one source pixel per output pixel (K bytes + 4 C bytes).
Both ratios are reported (below 1: the warp is faster than (a); 1.00: the kernel runs at copy rate).  Host time per call (enqueue
only) is listed too.  The kernels' registers and LDS are read from hipcc's resource remarks.  There is no CPU fallback: without a
GPU the script fails.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib, build  # noqa: E402

B, H, W, K, C, SIZE = 8, 1024, 1024, 3, 3, (512, 512)
GAMMA, MEAN, STD = 1.3, .5, .25


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def host_time(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = (time.perf_counter() - t) / reps * 1e3
    torch.cuda.synchronize()
    return dt


def stock(image, labels, maps_dev, jj, ii, gamma_dev):
    """(a): the same result up to rounding with stock torch ops (fill 0)."""
    h, w = SIZE
    m = maps_dev[:, :, None, None]
    sx = m[:, 0] * jj + m[:, 1] * ii + m[:, 2]  # float64 [B, h, w]
    sy = m[:, 3] * jj + m[:, 4] * ii + m[:, 5]
    grid = torch.stack([sx * (2. / (W - 1)) - 1, sy * (2. / (H - 1)) - 1], dim=-1).float()
    x = F.grid_sample(image.permute(0, 3, 1, 2).float(), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    x = x.mul_(1 / 255).pow_(gamma_dev).mul_(1 / STD).sub_(MEAN / STD)
    nx, ny = torch.floor(sx + .5).long(), torch.floor(sy + .5).long()
    inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
    index = (ny.clamp_(0, H - 1) * W + nx.clamp_(0, W - 1)).view(B, h * w, 1).expand(-1, -1, C)
    lab = labels.view(B, H * W, C).gather(1, index).view(B, h, w, C)
    return x, lab * inside[..., None]


def bench(name, maps, image, labels, rounds, reps, rate):
    h, w = SIZE
    tables = np.broadcast_to(cda.augment.intensity_table(K, gamma=GAMMA, mean=MEAN, std=STD), (B, K, 256)).copy()
    maps_dev = torch.from_numpy(maps).cuda()
    tables_dev = torch.from_numpy(tables).cuda()
    out = torch.empty((B, K, h, w), dtype=torch.float32, device='cuda')
    lab = torch.empty((B, h, w, C), dtype=torch.int32, device='cuda')
    jj = torch.arange(w, dtype=torch.float64, device='cuda')[None, None, :]
    ii = torch.arange(h, dtype=torch.float64, device='cuda')[None, :, None]
    gamma_dev = torch.full((B, 1, 1, 1), GAMMA, device='cuda')
    lib = _lib.load()

    def kernel_alone():
        _lib.check(lib.cpn_augment_warp(_lib.ptr(image), _lib.AUGMENT_IMAGE_U8, _lib.ptr(labels), B, H, W, K, C, _lib.ptr(maps_dev),
                                        _lib.ptr(tables_dev), _lib.AUGMENT_BORDER_CONSTANT, 0., 0, _lib.ptr(out), 0, _lib.ptr(lab), h, w,
                                        _lib.stream_ptr()), 'augment_warp')

    calls = {'warp, whole call': lambda: cda.augment.warp(image, labels, maps, SIZE, tables),
             'warp, kernel alone': kernel_alone,
             'stock (a)': lambda: stock(image, labels, maps_dev, jj, ii, gamma_dev)}
    got, want = calls['warp, whole call'](), calls['stock (a)']()
    torch.cuda.synchronize()
    image_gap = float((got[0] - want[0]).abs().max())
    label_differ = int((got[1] != want[1]).sum())
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(rounds):  # alternating: every round times every call once
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    med = {key: statistics.median(v) for key, v in times.items()}
    host = {key: host_time(fn, reps) for key, fn in calls.items()}
    nbytes = B * h * w * (K * 4 + C * 4) + B * h * w * (K + C * 4)
    at_copy_rate = nbytes / rate * 1e3
    lines = [f'{name}   ({B} x {H} x {W} x {K} uint8 + {C} int32 label channels -> {B} x {K} x {h} x {w} float32 + {B} x {h} x {w} x {C} '
             f'int32; {nbytes / 2 ** 20:.1f} MiB read and written: {at_copy_rate:.4f} ms at copy rate (b))']
    for key in calls:
        lines.append(f'  {key:<22s} {med[key]:8.4f} ms  [{min(times[key]):.4f} .. {max(times[key]):.4f}]   host, enqueue only: {host[key]:.4f} ms')
    lines += [f'  warp, whole call / stock (a): {med["warp, whole call"] / med["stock (a)"]:.2f}   kernel alone / stock (a): '
              f'{med["warp, kernel alone"] / med["stock (a)"]:.2f}   (below 1: the warp is faster)',
              f'  warp, kernel alone / (b): {med["warp, kernel alone"] / at_copy_rate:.2f}   whole call / (b): '
              f'{med["warp, whole call"] / at_copy_rate:.2f}   (1.00 = copy rate)',
              f'  warp against stock (a) on this input: image max |difference| {image_gap:.3e} (float32 positions and blend-then-'
              f'transform in (a)), {label_differ} of {B * h * w * C} labels differ (float64 positions in both)']
    return lines


def kernel_resources():
    """VGPRs, LDS and spills of the kernels of csrc/augment.hip as hipcc reports them."""
    src = os.path.join(build.CSRC, 'augment.hip')
    cmd = [build._hipcc(), f'--offload-arch={build.ARCH}', '-O3', '-std=c++17', '-c', src, '-o', os.devnull, '--cuda-device-only',
           '-Rpass-analysis=kernel-resource-usage'] + build.SOURCES['augment.hip']
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out = []
    for block in text.split('Function Name: ')[1:]:
        name = re.search(r'au_warp_kernelILb([01])ELb([01])E', block)
        field = {k: re.search(k + r'[^:]*: (\d+)', block) for k in ('VGPRs', 'VGPRs Spill', 'SGPRs Spill', 'ScratchSize', 'LDS Size', 'Occupancy')}
        if name and all(field.values()):
            kind = f'au_warp_kernel<{"uint8" if name.group(1) == "1" else "float32"} in, {"bf16" if name.group(2) == "1" else "float32"} out>'
            out.append(f'  {kind:<44s} {field["VGPRs"].group(1)} VGPRs, {field["LDS Size"].group(1)} B LDS, '
                       f'{field["Occupancy"].group(1)} waves / SIMD, spills {field["VGPRs Spill"].group(1)} + '
                       f'{field["SGPRs Spill"].group(1)}, scratch {field["ScratchSize"].group(1)} B')
    return out or ['  not measured (hipcc gave no resource remarks)']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'augment.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('augment_microbench needs an MI355X: there is no CPU fallback')
    g = torch.Generator(device='cuda').manual_seed(0)
    image = torch.randint(0, 256, (B, H, W, K), device='cuda', generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 4000, (B, H // 16, W // 16, C), device='cuda', generator=g, dtype=torch.int32)
    labels = labels.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()  # blocks of 16 x 16: objects, not noise
    src = torch.empty(64 * 2 ** 20, device='cuda').normal_()
    dst = torch.empty_like(src)
    src16, dst16 = src.view(torch.complex128), dst.view(torch.complex128)
    for _ in range(3):
        dst16.copy_(src16)
    copy = statistics.median(timed(lambda: dst16.copy_(src16), args.reps) for _ in range(args.rounds))
    rate = 2 * src.numel() * 4 / (copy * 1e-3)
    del src, dst, src16, dst16
    out = [f'Joint affine warp of image and labels (cda.augment.warp) against stock torch (F.grid_sample + intensity passes + an index '
           f'gather), one MI355X (torch.cuda.get_device_name: "{torch.cuda.get_device_name(0)}", '
           f'{getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")}, '
           f'{torch.cuda.get_device_properties(0).multi_processor_count} CUs).',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over '
           f'the rounds.', 'tools/augment_microbench.py writes this table.', '',
           f'copy, 16 B / lane: {copy:.3f} ms for 256 MiB read + 256 MiB written: {rate / 1e12:.2f} TB/s', '']
    for name, maps in (('rotation by 27 degrees', np.stack([cda.augment.affine_map((H, W), SIZE, angle=27.)] * B)),
                       ('identity (a centred crop)', np.stack([cda.augment.affine_map((H, W), SIZE)] * B))):
        lines = bench(name, maps, image, labels, args.rounds, args.reps, rate)
        print('\n'.join(lines), flush=True)
        out += lines + ['']
    out += ['Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):'] + kernel_resources() + ['']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
