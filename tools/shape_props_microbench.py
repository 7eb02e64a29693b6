"""Times cda.shape_properties on a synthetic slide-sized label image and prints one JSON line per object count.
    python tools/shape_props_microbench.py [size=16384] [objects=100000,1000000] [repeats=5] [radius=0.6] [channels=3]

The image is the one of ``tools/property_table_microbench.py`` (``contours2labels`` on the seeded circle grid of
``tools/eval_microbench.py``, cut or padded to ``channels`` channels).  Reported per object count, in device-event ms (median of
``repeats``):
  shape_pass_ms        ``cpn_shape_accumulate`` without the hull (workspace memset + the streaming kernel: perimeter classes,
                       Crofton transitions, bit quads)
  shape_pass_hull_ms   the same call with the row extents of the hull (row_begin scatter, extents memset, the kernel)
  hull_ms              ``cpn_shape_hull``: one lane per object
  whole_call_ms        ``cda.shape_properties`` with every property (accumulate, status, sort, heights, scan, the total to
                       the host, shape pass, hull, finalise)
  region_call_ms       ``cda.region_properties`` with every geometric property on the same image (the call that existed before)
  mixed_call_ms        both engines on one accumulate / sort, as ``labels2property_table`` runs them (without the host copy)
  copy_ms              a device-to-device copy of the label image
  yardstick_ms         the four Crofton transition counts per object in stock tensor operations on the device (per channel
                       ``torch.unique`` with inverse, four shifted comparisons, ``bincount``), a part of what the shape pass
                       counts; the perimeter_crofton built from them must equal the HIP column bit for bit (asserted)
and the ratios.  There is no preset target."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import celldetection_amd as cda  # noqa: E402
from celldetection_amd import region_props, shape_props  # noqa: E402
from eval_microbench import contours  # noqa: E402
from flat_labels_microbench import event_ms  # noqa: E402
from property_table_microbench import PROPS as REGION_PROPS  # noqa: E402

ALL = shape_props.SUPPORTED
NO_HULL = ALL[:5]


def yardstick(labels):
    """perimeter_crofton (spacing 1) of every object from stock tensor operations, rows ordered by (channel, label)."""
    H, W, C = labels.shape
    out = []
    for ch in range(C):
        v = labels[:, :, ch]
        uniq, inv = torch.unique(v.clamp(min=0), return_inverse=True)
        n = uniq.numel()
        p = torch.nn.functional.pad(v, (1, 1, 1, 1))
        fg = v > 0
        cnt = []
        for dr, dc in ((-1, 0), (0, 1), (-1, -1), (1, -1)):
            m = fg & (p[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] != v)
            cnt.append(torch.bincount(inv[m], minlength=n))
        keep = uniq > 0
        straight, diagonal = (cnt[0] + cnt[1])[keep].double(), (cnt[2] + cnt[3])[keep].double()
        out.append((straight + diagonal / torch.full_like(diagonal, math.sqrt(2.0))) * (math.pi / 4.0))  # a true division
    return torch.cat(out)


def one(size, objects, repeats, radius, channels, dev):
    labels = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
    made = int(labels.shape[2])
    if made > channels:
        labels = labels[:, :, :channels].contiguous()
    elif made < channels:
        labels = torch.cat((labels, labels.new_zeros((size, size, channels - made))), 2).contiguous()
    H, W, C = (int(s) for s in labels.shape)
    res = dict(size=size, objects_asked=objects, radius=radius, channels=C, channels_made=made, bytes_read=H * W * C * 4)
    cols, stats = cda.shape_properties(labels, ALL, return_stats=True)
    acc = region_props._accumulate(labels, None, True, None)

    def passes(props):
        t = []
        shape_props._finalise(acc, shape_props._resolve(props), 1., 1., timings=t)
        torch.cuda.synchronize()
        return t[0].elapsed_time(t[1]), t[1].elapsed_time(t[2])
    passes(ALL)
    hull_runs = [passes(ALL) for _ in range(repeats)]
    plain_runs = [passes(NO_HULL) for _ in range(repeats)]
    med = lambda x: float(sorted(x)[len(x) // 2])
    sp_h, hull = med([a for a, _ in hull_runs]), med([b for _, b in hull_runs])
    sp = med([a for a, _ in plain_runs])
    w_ms, w_all, _ = event_ms(lambda: cda.shape_properties(labels, ALL), repeats)
    n_ms, n_all, _ = event_ms(lambda: cda.shape_properties(labels, NO_HULL), repeats)
    r_ms, r_all, _ = event_ms(lambda: cda.region_properties(labels, REGION_PROPS), repeats)
    mixed = REGION_PROPS + ALL[2:]
    x_ms, x_all, _ = event_ms(lambda: region_props._mixed_table(labels, mixed, None, None, '-', True, None), repeats)
    dst = torch.empty_like(labels)
    c_ms, c_all, _ = event_ms(lambda: dst.copy_(labels), repeats)
    del dst
    y_ms, y_all, yard = event_ms(lambda: yardstick(labels), max(repeats // 2, 1))
    same = yard.shape == cols['perimeter_crofton'].shape and bool(torch.equal(yard.view(torch.int64), cols['perimeter_crofton'].view(torch.int64)))
    res.update(rows=stats['rows'], table_capacity=stats['table_capacity'], hull_rows=stats['hull_rows'],
               mean_object_pixels=round(float(cols['num_pixels'].double().mean()), 1),
               mean_solidity=round(float(cols['solidity'].mean()), 4), euler_min=int(cols['euler_number'].min()),
               shape_pass_ms=round(sp, 3), shape_pass_hull_ms=round(sp_h, 3), hull_ms=round(hull, 3),
               whole_call_ms=round(w_ms, 3), whole_call_ms_all=w_all, whole_call_no_hull_ms=round(n_ms, 3), whole_call_no_hull_ms_all=n_all,
               region_call_ms=round(r_ms, 3), region_call_ms_all=r_all, mixed_call_ms=round(x_ms, 3), mixed_call_ms_all=x_all,
               copy_ms=round(c_ms, 3), copy_ms_all=c_all, yardstick_ms=round(y_ms, 3), yardstick_ms_all=y_all, yardstick_equal=same,
               shape_pass_over_copy=round(sp / c_ms, 2), whole_call_over_region_call=round(w_ms / r_ms, 2),
               mixed_call_over_region_call=round(x_ms / r_ms, 2), yardstick_over_shape_pass=round(y_ms / sp, 1),
               yardstick_over_whole_call=round(y_ms / w_ms, 1))
    print(json.dumps(res), flush=True)
    assert same, 'the tensor-op yardstick and the HIP column disagree'


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
