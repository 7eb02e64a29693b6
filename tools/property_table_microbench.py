"""Times cda.region_properties on a synthetic slide-sized label image and prints one JSON line per object count.
    python tools/property_table_microbench.py [size=16384] [objects=100000,1000000] [repeats=5] [radius=0.6] [channels=3]

The image comes from ``contours2labels`` on the seeded circle grid of ``tools/eval_microbench.py`` (``radius``: the largest
contour radius as a fraction of the grid pitch), cut or padded to ``channels`` channels.  Reported per object count, in
device-event ms (median of ``repeats``):
  accumulate_ms     the accumulate pass alone (``cpn_props_accumulate``: table memset + the streaming kernel)
  empty_image_accumulate_ms / table_memset_ms   the same pass on an image without objects (loads, run masks, LDS set-up and
                    barriers, no table traffic) and the memset of its workspace: where the pass stands before any run is added
  whole_call_ms     ``cda.region_properties`` with every geometric property (accumulate, status, sort, finalise, host round trip)
  copy_ms           a device-to-device copy of the label image (the same bytes read, and as many written)
  yardstick_ms      the same accumulators in stock tensor operations on the device (``torch.unique`` per channel, then
                    ``index_add_`` for count and sums, ``scatter_reduce`` for the bounding box), what a user would write
                    without the HIP path; its integers must equal the HIP table's (asserted)
and the two ratios accumulate / copy and yardstick / accumulate.  There is no preset target.

The reference's own time (scikit-image's ``regionprops_table`` per channel on the host) cannot be measured where scikit-image
is not installed; the yardstick on the device is the stand-in."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402
from celldetection_amd._tables import default_capacity  # noqa: E402
from eval_microbench import contours  # noqa: E402
from flat_labels_microbench import event_ms  # noqa: E402

PROPS = ('label', 'bbox', 'num_pixels', 'area', 'area_bbox', 'extent', 'equivalent_diameter_area', 'centroid', 'centroid_local',
         'inertia_tensor', 'inertia_tensor_eigvals', 'axis_major_length', 'axis_minor_length', 'eccentricity', 'orientation')


def yardstick(labels):
    """The accumulators in stock tensor operations: int32 [H, W, C] -> int64 [rows, 12] (channel, label, n, sum r, sum c,
    sum r^2, sum rc, sum c^2, r0, c0, r1, c1), rows ordered by (channel, label)."""
    H, W, C = labels.shape
    out = []
    for ch in range(C):
        v = labels[:, :, ch].reshape(-1)
        idx = torch.nonzero(v > 0).reshape(-1)
        if idx.numel() == 0:
            continue
        r, c = torch.div(idx, W, rounding_mode='floor'), idx % W
        uniq, inv = torch.unique(v[idx], return_inverse=True)
        n = uniq.numel()
        acc = torch.zeros((6, n), dtype=torch.int64, device=labels.device)
        for k, x in enumerate((torch.ones_like(r), r, c, r * r, r * c, c * c)):
            acc[k].index_add_(0, inv, x)
        r0 = torch.full((n,), H, dtype=torch.int64, device=labels.device).scatter_reduce(0, inv, r, 'amin')
        c0 = torch.full((n,), W, dtype=torch.int64, device=labels.device).scatter_reduce(0, inv, c, 'amin')
        r1 = torch.zeros((n,), dtype=torch.int64, device=labels.device).scatter_reduce(0, inv, r, 'amax') + 1
        c1 = torch.zeros((n,), dtype=torch.int64, device=labels.device).scatter_reduce(0, inv, c, 'amax') + 1
        out.append(torch.stack((torch.full_like(r0, ch), uniq.to(torch.int64), *acc, r0, c0, r1, c1), 1))
    return torch.cat(out) if out else torch.zeros((0, 12), dtype=torch.int64, device=labels.device)


def one(size, objects, repeats, radius, channels, dev):
    labels = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
    made = int(labels.shape[2])
    if made > channels:
        labels = labels[:, :, :channels].contiguous()
    elif made < channels:
        labels = torch.cat((labels, labels.new_zeros((size, size, channels - made))), 2).contiguous()
    H, W, C = (int(s) for s in labels.shape)
    lib = _lib.load()
    cap = default_capacity(H * W, 64)
    res = dict(size=size, objects_asked=objects, radius=radius, channels=C, channels_made=made, bytes_read=H * W * C * 4)
    cols, stats = cda.region_properties(labels, PROPS, return_stats=True)
    cap = stats['table_capacity']
    nbytes = int(lib.cpn_props_workspace_bytes(cap, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    acc = lambda: _lib.check(lib.cpn_props_accumulate(_lib.ptr(labels), H, W, C, None, 0, 0, cap, _lib.ptr(ws), nbytes,
                                                      _lib.stream_ptr()), 'props_accumulate')
    a_ms, a_all, _ = event_ms(acc, repeats)
    empty = torch.zeros_like(labels)  # no object: what the pass costs before any run reaches a table
    floor = lambda: _lib.check(lib.cpn_props_accumulate(_lib.ptr(empty), H, W, C, None, 0, 0, cap, _lib.ptr(ws), nbytes,
                                                        _lib.stream_ptr()), 'props_accumulate')
    f_ms, f_all, _ = event_ms(floor, repeats)
    m_ms, _, _ = event_ms(lambda: ws.zero_(), repeats)
    del ws, empty
    w_ms, w_all, _ = event_ms(lambda: cda.region_properties(labels, PROPS), repeats)
    dst = torch.empty_like(labels)
    c_ms, c_all, _ = event_ms(lambda: dst.copy_(labels), repeats)
    del dst
    y_ms, y_all, yard = event_ms(lambda: yardstick(labels), max(repeats // 2, 1))
    # the yardstick's integers against the HIP table (centroid * n is not exact in fp64: compare the integer columns)
    same = yard.shape[0] == stats['rows'] and bool(torch.equal(yard[:, 1], cols['label'])) and \
        bool(torch.equal(yard[:, 2], cols['num_pixels'])) and \
        all(bool(torch.equal(yard[:, 8 + i], cols[f'bbox-{i}'])) for i in range(4)) and \
        bool(torch.equal((yard[:, 3].double() / yard[:, 2].double()), cols['centroid-0']))
    fg = float((labels > 0).sum()) / (H * W * C)
    res.update(rows=stats['rows'], table_capacity=cap, table_grown=stats['grown'], foreground_share=round(fg, 4),
               mean_object_pixels=round(fg * H * W * C / max(stats['rows'], 1), 1),
               accumulate_ms=round(a_ms, 3), accumulate_ms_all=a_all, accumulate_gb_per_s=round(H * W * C * 4 / a_ms / 1e6, 1),
               empty_image_accumulate_ms=round(f_ms, 3), empty_image_accumulate_ms_all=f_all, table_memset_ms=round(m_ms, 3),
               whole_call_ms=round(w_ms, 3), whole_call_ms_all=w_all, copy_ms=round(c_ms, 3), copy_ms_all=c_all,
               yardstick_ms=round(y_ms, 3), yardstick_ms_all=y_all, yardstick_equal=same,
               accumulate_over_copy=round(a_ms / c_ms, 2), yardstick_over_accumulate=round(y_ms / a_ms, 1),
               yardstick_over_whole_call=round(y_ms / w_ms, 1))
    print(json.dumps(res), flush=True)
    assert same, 'the tensor-op yardstick and the HIP table disagree'


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    counts = [int(c) for c in sys.argv[2].split(',')] if len(sys.argv) > 2 else [100000, 1000000]
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    radius = float(sys.argv[4]) if len(sys.argv) > 4 else .6
    channels = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    for objects in counts:
        one(size, objects, repeats, radius, channels, torch.device('cuda:0'))
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
