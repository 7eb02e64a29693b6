"""Times cda.resolve_label_channels on a synthetic slide-sized label image and prints one JSON line.
    python tools/flat_labels_microbench.py [size=16384] [objects=100000] [repeats=5] [radius=0.6]

The image comes from ``contours2labels`` on the seeded circle grid of ``tools/eval_microbench.py``; ``radius`` is the largest
contour radius as a fraction of the grid pitch, large enough that neighbours overlap.  Reported: device-event ms of the
classify pass (``cpn_flat_classify``) with the bytes it moves ((C + 1) x H x W x 4) and its share of the measured float4 copy
rate; of the propagation (all ``cpn_flat_step`` launches, host round trips included) with steps,
launches and the tiles run per launch; and of the whole call.

The yardstick is the same rule written with stock tensor operations on the same GPU in the same process (padded shifts,
``torch.maximum``, ``torch.where`` over the whole image per step): what a user would write without the HIP path.  Its result
must equal the HIP result, and the HIP path must not be slower (asserted)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402
from celldetection_amd.flat_labels import CROSS, MAX_STEPS  # noqa: E402
from eval_microbench import HBM_COPY_TBS, contours  # noqa: E402


def yardstick(labels, max_iter=999):
    """The rule in stock tensor operations: int32 [H, W, C] -> int32 [H, W]."""
    count = (labels > 0).sum(-1)
    over = count > 1
    top = labels.max(-1).values
    if not bool(over.any()):
        return top, 0
    lbl = torch.where(count == 1, top, torch.zeros_like(top))
    steps = 0
    for _ in range(max_iter):
        m = over & (lbl <= 0)
        if not bool(m.any()):
            break
        p = F.pad(lbl, (1, 1, 1, 1))  # zeros never win against a label
        d = torch.maximum(torch.maximum(p[1:-1, :-2], p[1:-1, 2:]), torch.maximum(p[:-2, 1:-1], p[2:, 1:-1]))
        new = torch.where(m, d, lbl)
        steps += 1
        if torch.equal(new, lbl):
            break
        lbl = new
    return lbl, steps


def event_ms(fn, repeats):
    """Median device-event time of fn() and its last result."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 3) for t in times], r


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    objects = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    radius = float(sys.argv[4]) if len(sys.argv) > 4 else .6
    dev = torch.device('cuda:0')
    labels = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
    H, W, C = (int(s) for s in labels.shape)
    lib = _lib.load()
    from ctypes import c_int64
    status = (c_int64 * 2)()
    moved = (C + 1) * H * W * 4
    res = dict(size=size, objects=objects, radius=radius, channels=C, classify_bytes=moved)
    nbytes = int(lib.cpn_flat_workspace_bytes(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((H, W), dtype=torch.int32, device=dev)
    classify = lambda st=None: _lib.check(lib.cpn_flat_classify(_lib.ptr(labels), C, H, W, 0, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                                                st, _lib.stream_ptr()), 'flat_classify')
    c_ms, c_all, _ = event_ms(classify, repeats)
    classify(status)
    overlap = int(status[0])

    def propagate():
        left, launch, tiles = overlap, 0, []
        while left > 0:
            _lib.check(lib.cpn_flat_step(_lib.ptr(out), H, W, MAX_STEPS, CROSS, launch, _lib.ptr(ws), nbytes, status,
                                         _lib.stream_ptr()), 'flat_step')
            launch += 1
            tiles.append(int(status[1]))
            left -= int(status[0])
            if int(status[0]) == 0:
                break
        return launch, tiles, left
    p_times = []
    for _ in range(repeats):
        classify(status)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches, tiles, left = propagate()
        e1.record()
        e1.synchronize()
        p_times.append(e0.elapsed_time(e1))
    del ws, out
    w_ms, w_all, (flat, stats) = event_ms(lambda: cda.resolve_label_channels(labels, return_stats=True), repeats)
    res.update(
        overlap_pixels=stats['overlap_pixels'], overlap_share=round(stats['overlap_pixels'] / (H * W), 5),
        unresolved_pixels=stats['unresolved_pixels'],
        classify_ms=round(c_ms, 3), classify_ms_all=c_all, classify_gb_per_s=round(moved / c_ms / 1e6, 1),
        classify_share_of_hbm_copy_rate=round(moved / c_ms / 1e9 / HBM_COPY_TBS, 3),
        propagation_ms=round(float(np.median(p_times)), 3), propagation_ms_all=[round(t, 3) for t in p_times],
        steps=stats['steps'], launches=launches, tiles_total=-(-H // 32) * -(-W // 32), active_tiles=tiles,
        whole_call_ms=round(w_ms, 3), whole_call_ms_all=w_all)
    y_ms, y_all, (yard, y_steps) = event_ms(lambda: yardstick(labels), max(repeats // 2, 1))
    equal = bool(torch.equal(yard, flat))
    best = res['whole_call_ms']
    res.update(yardstick_ms=round(y_ms, 3), yardstick_ms_all=y_all, yardstick_steps=y_steps, yardstick_equal=equal,
               yardstick_over_hip=round(y_ms / best, 2))
    print(json.dumps(res))
    assert equal, 'the tensor-op yardstick and the HIP path disagree'
    assert best <= y_ms, f'the HIP path ({best} ms) is slower than the tensor-op yardstick ({y_ms} ms)'


if __name__ == '__main__':
    main()
