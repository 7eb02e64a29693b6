"""Times the optimizer step (celldetection_amd.optim: global-norm clip + AdamW) against stock torch on one MI355X and writes the
table of profiles/optim.txt.

    python tools/optim_microbench.py [--out profiles/optim.txt] [--rounds 10] [--reps 5] [--workloads 0,1]

Workloads: the float32 parameters of CpnResNeXt101UNet (the shapes of the 'param' entries of graph.build_plan: no reference and no
weights needed) and one flat tensor of 64 Mi float32 elements.  All paths run in the same process, alternating round by round.
Every number is the median over the rounds of a HIP-event time around `reps` back-to-back calls, after a warm-up of every call.
Per workload: a 16-byte-per-lane copy of 256 MiB (torch's copy of the bytes viewed as 16-byte elements: 1 read + 1 write), which
gives the copy rate every kernel is held against; the norm pass (reads g: 4 B per element), the step (reads p, g, m, v, writes p, m,
v: 28 B; also its kernel alone, launched on a table already on the device) and clip + step (32 B), each with its time divided by
the time the copy rate needs for those bytes (1.00 = copy rate); the step with non-temporal stores of m and v;
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with foreach=True and, where this torch build offers it, fused=True.  Host time
per call (a host clock around the enqueue, no synchronise) is listed too, since a step of several hundred tensors can be bound by
the host.  The kernels' registers and LDS are read from hipcc's resource remarks.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import math
import os
import re
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib, build, graph  # noqa: E402

HYPER = dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=1e-2)
MAX_NORM = 1.


def workload_shapes(index):
    if index == 0:
        plan = graph.build_plan('ResNeXt101UNet', 3)
        return 'CpnResNeXt101UNet parameters', [tuple(shape) for _, shape, kind in plan.entries if kind == 'param']
    return 'one flat tensor', [(64 * 2 ** 20,)]


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


def make_params(shapes, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    params = []
    for s in shapes:
        p = torch.nn.Parameter(torch.randn(s, device='cuda', generator=g))
        p.grad = torch.randn(s, device='cuda', generator=g) * .01
        params.append(p)
    return params


def bench_workload(index, rounds, reps):
    name, shapes = workload_shapes(index)
    elements = sum(math.prod(s) for s in shapes)
    info = cda.optim.step_info([math.prod(s) for s in shapes])
    ours, ours_clip, stock, stock_fused = (make_params(shapes, 0) for _ in range(4))
    opt = cda.optim.AdamW(ours, **HYPER)
    opt_clip = cda.optim.AdamW(ours_clip, max_grad_norm=MAX_NORM, **HYPER)
    opt_stock = torch.optim.AdamW(stock, foreach=True, **HYPER)
    try:
        opt_fused = torch.optim.AdamW(stock_fused, fused=True, **HYPER)
        opt_fused.step()
    except Exception as e:  # this build has no fused AdamW for the device
        opt_fused, why_not = None, f'{type(e).__name__}: {e}'
    src = torch.empty(64 * 2 ** 20, device='cuda').normal_()
    dst = torch.empty_like(src)
    src16, dst16 = src.view(torch.complex128), dst.view(torch.complex128)
    copy_bytes = 2 * src.numel() * 4

    def step_plain():
        cda.optim.NONTEMPORAL = 0
        opt.step()

    def step_nt():
        cda.optim.NONTEMPORAL = 1
        opt.step()
        cda.optim.NONTEMPORAL = 0

    def stock_step():
        torch.nn.utils.clip_grad_norm_(stock, MAX_NORM, foreach=True)
        opt_stock.step()

    def fused_step():
        torch.nn.utils.clip_grad_norm_(stock_fused, MAX_NORM, foreach=True)
        opt_fused.step()

    # the update kernel alone on a private copy of the table the last step uploaded (the tensors it names stay alive and in place)
    opt.step()
    eng = cda.optim._ENGINES[torch.cuda.current_device()]
    dev_map, chunks = eng.plan([p.numel() for p in ours])
    table = eng.table[:len(ours) * cda.optim._RECORD.itemsize].clone()
    lib = _lib.load()

    def kernel_alone():
        _lib.check(lib.cpn_optim_adamw(_lib.ptr(table), len(ours), _lib.ptr(dev_map), chunks, None, 0, _lib.stream_ptr()), 'optim_adamw')

    calls = {'copy': lambda: dst16.copy_(src16), 'step, kernel alone': kernel_alone, 'norm': lambda: cda.optim.grad_norm(ours), 'step': step_plain,
             'step, non-temporal m, v': step_nt, 'clip + step': opt_clip.step, 'stock foreach clip + step': stock_step,
             'stock foreach step alone': opt_stock.step}
    if opt_fused is not None:
        calls['stock fused clip + step'] = fused_step
        calls['stock fused step alone'] = opt_fused.step
    for fn in calls.values():  # warm-up: code objects, the allocator, the chunk maps, the optimizers' lazy state
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(rounds):  # alternating: every round times every call once
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    med = {key: statistics.median(v) for key, v in times.items()}
    spread = {key: (min(v), max(v)) for key, v in times.items()}
    host = {key: host_time(fn, reps) for key, fn in calls.items() if key in ('step', 'clip + step', 'stock foreach clip + step',
                                                                            'stock fused clip + step')}
    rate = copy_bytes / (med['copy'] * 1e-3)
    lines = [f'{name}   ({len(shapes)} float32 tensors, {elements / 1e6:.1f} M elements, {info["chunks"]} chunks of '
             f'{info["chunk_elements"]}, {sum(1 for t in info["tensors"] if t[1] == 1 and t[2] < info["chunk_elements"])} tensors '
             f'smaller than a chunk)',
             f'  {"copy, 16 B / lane":<28s} {med["copy"]:8.3f} ms  [{spread["copy"][0]:.3f} .. {spread["copy"][1]:.3f}]   '
             f'{rate / 1e12:.2f} TB/s (256 MiB: 1 read + 1 write)']
    for key, per_element in (('norm', 4), ('step, kernel alone', 28), ('step', 28), ('step, non-temporal m, v', 28), ('clip + step', 32)):
        nbytes = per_element * elements
        lines.append(f'  {key:<28s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]   {per_element} B / element, '
                     f'{nbytes / 2 ** 20:.0f} MiB, {nbytes / (med[key] * 1e-3) / 1e12:.2f} TB/s: {med[key] / (nbytes / rate * 1e3):.2f} of the '
                     f'time at copy rate')
    for key in calls:
        if key.startswith('stock'):
            lines.append(f'  {key:<28s} {med[key]:8.3f} ms  [{spread[key][0]:.3f} .. {spread[key][1]:.3f}]')
    if opt_fused is None:
        lines.append(f'  stock fused: not offered by this build ({why_not[:120]})')
    best = min(med[k] for k in med if k.startswith('stock') and k.endswith('clip + step'))
    lines.append(f'  clip + step / best stock clip + step: {med["clip + step"] / best:.2f} (below 1: the new path is faster)')
    lines.append('  host time per call, enqueue only: ' + ', '.join(f'{k} {v:.3f} ms' for k, v in host.items()))
    return lines


def kernel_resources():
    """VGPRs, LDS and spills of the kernels of csrc/optim.hip as hipcc reports them."""
    src = os.path.join(build.CSRC, 'optim.hip')
    cmd = [build._hipcc(), f'--offload-arch={build.ARCH}', '-O3', '-std=c++17', '-c', src, '-o', os.devnull, '--cuda-device-only',
           '-Rpass-analysis=kernel-resource-usage'] + build.SOURCES['optim.hip']
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out = []
    for block in text.split('Function Name: ')[1:]:
        name = re.search(r'optim_[a-z]+_kernel(ILb[01]E)?', block)
        field = {k: re.search(k + r'[^:]*: (\d+)', block) for k in ('VGPRs', 'VGPRs Spill', 'SGPRs Spill', 'ScratchSize', 'LDS Size', 'Occupancy')}
        if name and all(field.values()):
            out.append(f'  {name.group(0):<28s} {field["VGPRs"].group(1)} VGPRs, {field["LDS Size"].group(1)} B LDS, '
                       f'{field["Occupancy"].group(1)} waves / SIMD, spills {field["VGPRs Spill"].group(1)} + '
                       f'{field["SGPRs Spill"].group(1)}, scratch {field["ScratchSize"].group(1)} B')
    return out or ['  not measured (hipcc gave no resource remarks)']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join('profiles', 'optim.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--workloads', default='0,1')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('optim_microbench needs an MI355X: there is no CPU fallback')
    out = [f'Global-norm clip + AdamW (cda.optim) against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, float32, one MI355X '
           f'(torch.cuda.get_device_name: "{torch.cuda.get_device_name(0)}", '
           f'{getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")}, '
           f'{torch.cuda.get_device_properties(0).multi_processor_count} CUs).',
           f'torch {torch.__version__}; median of {args.rounds} alternating rounds of {args.reps} calls, HIP events; [min .. max] over '
           f'the rounds.', 'tools/optim_microbench.py writes this table.', '']
    for i in (int(s) for s in args.workloads.split(',')):
        lines = bench_workload(i, rounds=args.rounds, reps=args.reps)
        print('\n'.join(lines), flush=True)
        out += lines + ['']
        torch.cuda.empty_cache()
    out += ['Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):'] + kernel_resources() + ['']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
