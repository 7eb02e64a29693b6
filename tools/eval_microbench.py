"""Times cda.LabelMatcher on two synthetic slide-sized label images and prints one JSON line.
    python tools/eval_microbench.py [size=16384] [objects=100000] [repeats=5] [radius=0.4]

The images come from ``contours2labels`` on seeded contours (jittered grid of noisy circles); the second image is the first
one with jittered contours.  Reported: ms of the pixel pass (``cpn_eval_pairs``, device events), of the table step (status,
compaction, sort, split, unions) and of the selection at IoU 0.5; the bytes the pixel pass reads ((C_in + C_t) x H x W x 4)
and the rate it reaches."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402
from celldetection_amd._tables import default_capacity  # noqa: E402
from celldetection_amd.instance_eval import _as_device_labels  # noqa: E402

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X (spec 8.0 TB/s)


def contours(size, objects, seed, jitter=0., samples=32, radius=.4):
    """[K, samples, 2] float32 xy: noisy circles on a jittered grid."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(objects)))
    pitch = size / side
    gy, gx = np.divmod(np.arange(side * side)[:objects], side)
    cy = (gy + .5) * pitch + rng.uniform(-.3, .3, objects) * pitch
    cx = (gx + .5) * pitch + rng.uniform(-.3, .3, objects) * pitch
    r = rng.uniform(.5 * radius, radius, objects) * pitch  # radius: largest radius as a fraction of the grid pitch
    wobble = 1 + .15 * rng.standard_normal((objects, 1)) * np.sin(np.linspace(0, 2 * np.pi, samples, endpoint=False)[None] * 3)
    if jitter:
        rj = np.random.default_rng(seed + 1)
        cy, cx, r = cy + rj.normal(0, jitter, objects), cx + rj.normal(0, jitter, objects), r * rj.uniform(.92, 1.08, objects)
    ang = np.linspace(0, 2 * np.pi, samples, endpoint=False)[None]
    rr = r[:, None] * wobble
    return np.stack((cx[:, None] + rr * np.cos(ang), cy[:, None] + rr * np.sin(ang)), -1).astype(np.float32)


def host_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, r


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    objects = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    radius = float(sys.argv[4]) if len(sys.argv) > 4 else .4
    dev = torch.device('cuda:0')
    t0 = time.perf_counter()
    a = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
    b = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, jitter=1.5, radius=radius)).to(dev), (size, size))
    torch.cuda.synchronize()
    labels_s = time.perf_counter() - t0
    a, b = _as_device_labels(a, 'inputs'), _as_device_labels(b, 'targets')
    lib = _lib.load()
    pixels = size * size
    cap = default_capacity(pixels, 16)
    nbytes = int(lib.cpn_eval_workspace_bytes(cap, 0, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    run = lambda: _lib.check(lib.cpn_eval_pairs(_lib.ptr(a), int(a.shape[2]), _lib.ptr(b), int(b.shape[2]), pixels, cap,
                                                _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'eval_pairs')
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    del ws
    pixel_ms = float(np.median(times))
    m = cda.LabelMatcher()
    update_ms, _ = host_ms(lambda: m.update(a, b, .5), repeats)
    select_ms, _ = host_ms(m.filter_and_threshold, repeats)
    f1_ms, f1 = host_ms(lambda: cda.LabelMatcher(a, b, iou_thresh=.5).f1, repeats)
    rounds = {}
    for thr in (0., .5, .75):
        m.iou_thresh = thr
        rounds[str(thr)] = m.stats['selection_rounds']
    m.iou_thresh = .5
    read = (int(a.shape[2]) + int(b.shape[2])) * pixels * 4
    print(json.dumps(dict(
        size=size, channels=[int(a.shape[2]), int(b.shape[2])], objects=[len(m.input_labels), len(m.target_labels)],
        pairs=m.stats['pairs'], table_capacity=m.stats['table_capacity'], table_grown=m.stats['grown'],
        pixel_pass_ms=round(pixel_ms, 3), pixel_pass_ms_all=[round(t, 3) for t in times],
        table_ms=round(update_ms - pixel_ms - select_ms, 3), selection_ms=round(select_ms, 3),
        label_matcher_f1_ms=round(f1_ms, 3), bytes_read=read, pixel_pass_gb_per_s=round(read / pixel_ms / 1e6, 1),
        share_of_hbm_copy_rate=round(read / pixel_ms / 1e9 / HBM_COPY_TBS, 3), selection_rounds=rounds,
        f1_at_0p5=f1, true_positives=m.true_positives, contours2labels_s=round(labels_s, 2))))


if __name__ == '__main__':
    main()
