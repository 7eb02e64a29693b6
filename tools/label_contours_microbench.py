"""Times cda.labels2contours and cda.resample_contours on slide-sized label images and prints one JSON line per image.
    python tools/label_contours_microbench.py [size=16384] [objects=100000,1000000] [repeats=5] [radius=0.6] [limit_s=300]

Images, each in a child process of its own under ``limit_s`` seconds (the first one that fails or runs out of time ends the tool):
  labels3   the first 3 channels of ``contours2labels`` of the seeded circle grid of ``tools/eval_microbench.py``, per object count
  flat      ``resolve_label_channels`` of the same label image
  wide      one object as wide as the image (a band of 16 rows): ONE contour of about 2 * size points, followed by a single lane,
            the known limit of the one-lane-per-object trace
Reported per image, in device-event ms (one warm-up call, then the median of ``repeats``; every pass ends with the host read of
its counts, which is inside its time):
  components_ms  tile-local union-find, seams, flattening (``cpn_contours_components``)
  table_ms       slots, pixel counts, sort, fragmented runs, selection (``cpn_contours_table``)
  count_ms       the trace that counts points, and the scan (``cpn_contours_count``)
  write_ms       the trace that writes points (``cpn_contours_write``)
  resample_ms    ``resample_contours_packed`` of all contours to 32 points
  props_ms       ``cda.region_properties(labels, ('label', 'area'))`` on the same image: it reads the image once, the streaming floor
These are records, not gates: there is no preset target."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PASSES = ('components', 'table', 'count', 'write')


def one(kind, size, objects, repeats, radius):
    import torch
    import celldetection_amd as cda
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
        if kind == 'flat':
            labels = cda.resolve_label_channels(labels)[:, :, None].contiguous()
        else:
            labels = labels[:, :, :3].contiguous() if made >= 3 else torch.cat((labels, labels.new_zeros((size, size, 3 - made))), 2)
    res = dict(image=kind, size=size, objects_asked=objects if kind != 'wide' else 1, channels=int(labels.shape[2]),
               bytes_read=labels.numel() * 4)
    ids, offsets, points = lc.labels2contours_packed(labels, raise_fragmented=False)  # warm-up
    res.update(contours=int(ids.numel()), points=int(points.shape[0]), longest=int((offsets[1:] - offsets[:-1]).max()))
    runs = []
    for _ in range(repeats):
        t = {}
        again = lc.labels2contours_packed(labels, raise_fragmented=False, timings=t)
        runs.append(t)
    res['repeatable'] = bool(torch.equal(again[2], points) and torch.equal(again[1], offsets) and torch.equal(again[0], ids))
    for p in PASSES:
        res[f'{p}_ms'] = round(float(np.median([r[p] for r in runs])), 3)
        res[f'{p}_ms_all'] = [round(r[p], 3) for r in runs]
    res['components_gb_per_s'] = round(labels.numel() * 4 / res['components_ms'] / 1e6, 1)
    c_ms, c_all, _ = event_ms(lambda: lc.labels2contours_packed(labels, raise_fragmented=False), max(repeats // 2, 1))
    res.update(call_ms=round(c_ms, 3), call_ms_all=c_all)
    r_ms, r_all, out = event_ms(lambda: lc.resample_contours_packed(points, offsets, 32), repeats)
    res.update(resample_ms=round(r_ms, 3), resample_ms_all=r_all, resample_shape=list(out.shape))
    p_ms, p_all, _ = event_ms(lambda: cda.region_properties(labels, ('label', 'area')), repeats)
    res.update(props_ms=round(p_ms, 3), props_ms_all=p_all, call_over_props=round(c_ms / p_ms, 1))
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
    steps = [(kind, objects) for objects in counts for kind in ('labels3', 'flat')] + [('wide', 1)]
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
