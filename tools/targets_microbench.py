"""Times cda.labels2distances and the CPN target generator on synthetic label images and prints one JSON line.
    python tools/targets_microbench.py [size=16384] [objects=100000] [repeats=5] [radius=0.6]
    python tools/targets_microbench.py square [side=4096] [repeats=3]

The image comes from ``contours2labels`` on the seeded circle grid of ``tools/eval_microbench.py`` (576 with 760 objects is the
case of the reference's own note: 54.9 ms for 576 x 576 x 3 with 762 instances on a CPU host).  Reported: device-event ms of
the classify and seed pass, of the relaxation (all ``cpn_label_distances_step`` launches, host round trips included) with its
launches and the tiles run per launch, of the keyed reduction and of the finalise pass, the whole call in both modes, the
masking, ``filter_instances_`` and ``CPNTargetGenerator.feed`` with every property read, and as yardstick the one streaming read
of ``region_properties`` on the same image.  ``square``: ONE object with an inradius far beyond the halo, the known limit (one
launch per 8 pixels of inradius)."""
import json
import os
import sys
from ctypes import c_int64

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402
from celldetection_amd.targets import MAX_STEPS  # noqa: E402
from eval_microbench import contours  # noqa: E402


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
    return round(float(np.median(times)), 3), [round(t, 3) for t in times], r


def passes(labels, repeats, per_instance=1):
    """Per-pass times through the C ABI."""
    H, W, C = (int(s) for s in labels.shape)
    lib = _lib.load()
    dev = labels.device
    status = (c_int64 * 2)()
    nbytes = int(lib.cpn_label_distances_workspace_bytes(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ck, p, s = _lib.check, _lib.ptr, _lib.stream_ptr
    classify = lambda st=None: ck(lib.cpn_label_distances_classify(p(labels), C, H, W, 2, per_instance, p(ws), nbytes, st, s()), 'classify')

    def relax():
        launch, tiles = 0, []
        while True:
            ck(lib.cpn_label_distances_step(H, W, MAX_STEPS, 2, per_instance, launch, p(ws), nbytes, status, s()), 'step')
            launch += 1
            tiles.append(int(status[1]))
            if int(status[0]) == 0:
                return launch, tiles
    c_ms, c_all, _ = event_ms(classify, repeats)
    r_times = []
    for _ in range(repeats):
        classify(status)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches, tiles = relax()
        e1.record()
        e1.synchronize()
        r_times.append(round(e0.elapsed_time(e1), 3))
    cap = 1 << 21
    table = torch.empty(cap * 12, dtype=torch.uint8, device=dev)
    red_ms, red_all, _ = event_ms(lambda: ck(lib.cpn_label_distances_reduce(H, W, p(ws), nbytes, p(table), cap, None, s()), 'reduce'),
                                  repeats)
    ck(lib.cpn_label_distances_reduce(H, W, p(ws), nbytes, p(table), cap, status, s()), 'reduce')
    assert int(status[0]) == 0
    dist = torch.empty((H, W), dtype=torch.float32, device=dev)
    out = torch.empty((H, W, C), dtype=torch.int32, device=dev)
    f_ms, f_all, _ = event_ms(lambda: ck(lib.cpn_label_distances_finalise(p(labels), C, H, W, per_instance, 36, p(ws), nbytes, p(table),
                                                                          cap, p(dist), p(out), s()), 'finalise'), repeats)
    return dict(classify_seed_ms=c_ms, classify_seed_ms_all=c_all, relax_ms=float(np.median(r_times)), relax_ms_all=r_times,
                launches=launches, active_tiles=tiles, tiles_total=-(-H // 32) * -(-W // 32), reduce_ms=red_ms, reduce_ms_all=red_all,
                finalise_ms=f_ms, finalise_ms_all=f_all)


def main():
    dev = torch.device('cuda:0')
    if sys.argv[1:2] == ['square']:
        side = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
        repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
        labels = torch.zeros((side + 64, side + 64, 1), dtype=torch.int32, device=dev)
        labels[32:-32, 32:-32] = 1
        res = dict(case='square', side=side, inradius=side // 2)
        w_ms, w_all, (d, _, st) = event_ms(lambda: cda.labels2distances(labels, return_stats=True), repeats)
        res.update(whole_call_ms=w_ms, whole_call_ms_all=w_all, launches=st['launches'], tiles_total=(-(-(side + 64) // 32)) ** 2,
                   active_tiles_first_last=[st['active_tiles'][0], st['active_tiles'][-2]], centre=float(d[side // 2 + 32, side // 2 + 32]))
        print(json.dumps(res))
        return
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    objects = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    radius = float(sys.argv[4]) if len(sys.argv) > 4 else .6
    labels = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
    H, W, C = (int(s) for s in labels.shape)
    res = dict(size=size, objects=objects, radius=radius, channels=C)
    res.update(passes(labels, repeats))
    w_ms, w_all, (d, l, st) = event_ms(lambda: cda.labels2distances(labels, return_stats=True), repeats)
    res.update(whole_call_ms=w_ms, whole_call_ms_all=w_all, table_capacity=st['table_capacity'],
               owner_pixel_share=round(float((d > 0).float().mean()), 4))
    fg_ms, fg_all, _ = event_ms(lambda: cda.labels2distances(labels, per_instance=False), repeats)
    res.update(fg_mode_whole_call_ms=fg_ms, fg_mode_whole_call_ms_all=fg_all)
    m_ms, m_all, _ = event_ms(lambda: cda.mask_labels_by_distance_(l, d, .5, .75, return_reduced=True), repeats)
    res.update(mask_ms=m_ms, mask_ms_all=m_all)
    p_ms, p_all, _ = event_ms(lambda: cda.region_properties(labels, ('label', 'num_pixels')), repeats)
    res.update(region_properties_ms=p_ms, region_properties_ms_all=p_all, whole_call_over_region_properties=round(w_ms / p_ms, 2))
    fi_ms, fi_all, _ = event_ms(lambda: cda.filter_instances_(labels.clone(), min_area=30), max(repeats // 2, 1))
    res.update(filter_instances_ms_with_clone=fi_ms, filter_instances_ms_all=fi_all)

    def generator():
        gen = cda.CPNTargetGenerator(samples=32, order=5)
        gen.feed(labels.clone())
        return gen.reduced_labels, gen.sampled_contours, gen.resampled_contours, gen.sampled_sizes
    g_ms, g_all, r = event_ms(generator, max(repeats // 2, 1))
    res.update(generator_ms_with_clone=g_ms, generator_ms_all=g_all, generator_rows=int(r[1].shape[0]))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
