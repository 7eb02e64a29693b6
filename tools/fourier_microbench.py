"""Times cda.fourier.efd_packed and cda.labels2fourier on slide-sized label images and prints one JSON line per image.
    python tools/fourier_microbench.py [size=16384] [objects=100000,1000000] [repeats=5] [radius=0.6] [limit_s=300]

Images, each in a child process of its own under ``limit_s`` seconds (the first one that fails or runs out of time ends the tool),
the same as ``tools/label_contours_microbench.py``:
  labels3   the first 3 channels of ``contours2labels`` of the seeded circle grid of ``tools/eval_microbench.py``, per object count
  wide      one object as wide as the image (a band of 16 rows): ONE contour of about 2 * size points
Reported per image and per order (5 and 25), in device-event ms (one warm-up call, then the median of ``repeats``):
  efd_ms            ``efd_packed`` on the int32 points and offsets of ``labels2contours_packed`` (whole call, its host read included)
  prepare_ms ..     its passes, timed by events inside the call: checks and work list (with the host read), single-chunk
  finish_ms         contours, chunk sums and bases, partial sums, finish
  stock_ms          the same formula in stock torch operations on the same tensors (float64; running sums through ``cumsum``,
                    per-contour sums through ``index_add_``, one order at a time), and the largest difference of its result
  resample_ms       ``resample_contours_packed`` to 32 points on the same input (it reads the same points once)
  labels2fourier_ms the whole call from the label image
These are records, not gates: there is no preset target."""
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

ORDERS = (5, 25)


def stock_efd(points, offsets, order, epsilon=1e-6):
    """The rule of celldetection_amd/fourier.py in stock torch operations; every contour gets its first point appended (the
    contours of labels2contours are open, except the doubled point, which gets one more segment of length epsilon here)."""
    import torch
    P, K = points.shape[0], offsets.numel() - 1
    p = points.to(torch.float64)
    lengths = offsets[1:] - offsets[:-1]
    seg = torch.repeat_interleave(torch.arange(K, device=p.device), lengths)
    nxt = torch.arange(1, P + 1, device=p.device)
    nxt[offsets[1:] - 1] = offsets[:-1]
    first = p[offsets[:-1]]
    d = p[nxt] - p
    dt = torch.sqrt((d * d).sum(1)) + epsilon
    run = torch.cumsum(dt, 0)
    start = (run - dt)[offsets[:-1]]
    t1 = run - start[seg]
    t0 = t1 - dt
    T = t1[offsets[1:] - 1]
    r = d / dt[:, None]
    phi0, phi1 = 2 * math.pi * t0 / T[seg], 2 * math.pi * t1 / T[seg]
    coeff = torch.zeros((K, order, 4), dtype=torch.float64, device=p.device)
    for k in range(1, order + 1):
        dcos, dsin = torch.cos(phi1 * k) - torch.cos(phi0 * k), torch.sin(phi1 * k) - torch.sin(phi0 * k)
        terms = torch.stack((r[:, 0] * dcos, r[:, 0] * dsin, r[:, 1] * dcos, r[:, 1] * dsin), 1)
        coeff[:, k - 1] = torch.zeros((K, 4), dtype=torch.float64, device=p.device).index_add_(0, seg, terms) * \
            (T / (2 * k * k * math.pi ** 2))[:, None]
    X = p[nxt] - first[seg]
    term = d / (2 * dt)[:, None] * (t1 * t1 - t0 * t0)[:, None] + (X - r * t1[:, None]) * dt[:, None]
    loc = first + torch.zeros((K, 2), dtype=torch.float64, device=p.device).index_add_(0, seg, term) / T[:, None]
    return coeff, loc


def one(kind, size, objects, repeats, radius):
    import torch
    import celldetection_amd as cda
    from celldetection_amd import fourier as fo
    from celldetection_amd import label_contours as lc
    from eval_microbench import contours
    from flat_labels_microbench import event_ms
    dev = torch.device('cuda:0')
    if kind == 'wide':
        labels = torch.zeros((size, size, 1), dtype=torch.int32, device=dev)
        labels[size // 2 - 8:size // 2 + 8] = 1
    else:
        labels = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
        made = int(labels.shape[2])
        labels = labels[:, :, :3].contiguous() if made >= 3 else torch.cat((labels, labels.new_zeros((size, size, 3 - made))), 2)
    ids, offsets, points = lc.labels2contours_packed(labels, raise_fragmented=False)
    lengths = offsets[1:] - offsets[:-1]
    res = dict(image=kind, size=size, contours=int(ids.numel()), points=int(points.shape[0]), longest=int(lengths.max()),
               mean_points=round(float(lengths.double().mean()), 1), single_chunk=int((lengths <= fo.CHUNK).sum()))
    r_ms, r_all, _ = event_ms(lambda: lc.resample_contours_packed(points, offsets, 32), repeats)
    res.update(resample_ms=round(r_ms, 3), resample_ms_all=r_all)
    for order in ORDERS:
        out = fo.efd_packed(points, offsets, order)  # warm-up
        runs = []
        for _ in range(repeats):
            t = {}
            again = fo.efd_packed(points, offsets, order, timings=t)
            runs.append(t)
        o = {'repeatable': bool(torch.equal(again[0], out[0]) and torch.equal(again[1].nan_to_num(-1), out[1].nan_to_num(-1))),
             'chunks': runs[0]['chunks']}
        for p in fo.PASSES:
            o[f'{p}_ms'] = round(float(np.median([r[p] for r in runs])), 3)
        e_ms, e_all, _ = event_ms(lambda: fo.efd_packed(points, offsets, order), repeats)
        o.update(efd_ms=round(e_ms, 3), efd_ms_all=e_all, efd_over_resample=round(e_ms / r_ms, 2))
        s_ms, s_all, stock = event_ms(lambda: stock_efd(points, offsets, order), max(repeats // 2, 1))
        many = lengths > 2  # (the doubled point is closed already: stock_efd gives it one more segment)
        o.update(stock_ms=round(s_ms, 3), stock_ms_all=s_all, stock_over_efd=round(s_ms / e_ms, 1),
                 stock_max_abs_diff=float((stock[0][many] - out[0][many]).abs().max()) if bool(many.any()) else 0.)
        del stock
        l_ms, l_all, _ = event_ms(lambda: cda.labels2fourier(labels, order=order, raise_fragmented=False), max(repeats // 2, 1))
        o.update(labels2fourier_ms=round(l_ms, 3), labels2fourier_ms_all=l_all)
        res[f'order{order}'] = o
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--one':
        one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]))
        return
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    counts = [int(c) for c in sys.argv[2].split(',')] if len(sys.argv) > 2 else [100000, 1000000]
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    radius = float(sys.argv[4]) if len(sys.argv) > 4 else .6
    limit = float(sys.argv[5]) if len(sys.argv) > 5 else 300.
    steps = [('labels3', objects) for objects in counts] + [('wide', 1)]
    for kind, objects in steps:  # a fresh process per step, under its own time limit; nothing more is started after a failure
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', kind, str(size), str(objects), str(repeats),
                                 str(radius)], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f'{kind} {objects}: no result within {limit:.0f} s', flush=True)
            sys.exit(124)
        if rc != 0:
            print(f'{kind} {objects}: exit status {rc}', flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == '__main__':
    main()
