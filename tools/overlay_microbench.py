"""Times cda.contours2overlay and cda.label_cmap on slide-sized inputs and prints one JSON line per object count.
    python tools/overlay_microbench.py [size=16384] [objects=100000,1000000] [repeats=5] [radius=0.6] [limit_s=300]

The contours are the seeded circle grid of ``tools/eval_microbench.py`` (``radius``: the largest contour radius as a fraction of
the grid pitch), the label image is ``contours2labels`` of them, as in ``tools/property_table_microbench.py``.  Every object
count runs in a child process of its own under ``limit_s`` seconds; the first one that fails or runs out of time ends the tool.
Reported per object count, in device-event ms (warm-up call, then the median of ``repeats``):
  paint_ms            the overlay pass alone (``cpn_overlay_paint`` on prepared points and tile lists)
  lists_ms            the (tile, contour) lists: count, scan, fill
  overlay_call_ms     ``cda.contours2overlay`` with given colours, end to end (prepare, lists, paint, the read of the largest overlap)
  labels_call_ms      ``cda.contours2labels`` on the same contours: the sibling that rasterises the same polygons
  cmap3_ms / cmap1_ms ``cda.label_cmap`` on the first 3 channels of the label image and on the flat image (resolve_label_channels)
  cmap3_stock_ms / cmap1_stock_ms   the same colour-map rule in stock tensor operations on the device (index the table, sum,
                      divide, multiply and add per channel, cast); ``*_stock_equal``: its bytes equal the kernel's
There is no preset target.  The reference's own functions are timed on the host by ``tests/golden/make_golden_overlay.py time``."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def stock_cmap(labels, table):
    """The rule of label_cmap(ubyte=True) in stock tensor operations: int32 [H, W(, C)], uint8 table [n + 1, 4] -> uint8 [H, W, 4]."""
    import torch
    n = table.shape[0] - 1
    rows = torch.where(labels != 0, labels % n + 1, torch.zeros_like(labels))
    if labels.ndim == 2:
        return table[rows.long()]
    acc = None
    cols = [table[rows[:, :, c].long()] for c in range(labels.shape[2])]
    den = sum(col[..., 3].to(torch.int32) for col in cols).float() + 1e-12
    for col in cols:
        term = (col[..., 3].float() / den)[..., None] * col.float()
        acc = term if acc is None else acc + term
    return acc.to(torch.uint8)


def one(size, objects, repeats, radius):
    import torch
    import celldetection_amd as cda
    from celldetection_amd import _lib
    from celldetection_amd.overlay import _color_table, _tile_lists
    from ctypes import c_uint32
    from eval_microbench import contours
    from flat_labels_microbench import event_ms
    dev = torch.device('cuda:0')
    con = torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev)
    K, S = int(con.shape[0]), int(con.shape[1])
    rng = np.random.default_rng(0)
    col = torch.as_tensor(rng.integers(0, 256, (K, 3)).astype(np.uint8)).to(dev)
    lib = _lib.load()
    res = dict(size=size, objects=K, points=S, radius=radius)
    out, st = cda.contours2overlay(con, (size, size), colors=col, intermediate_dtype='uint32', return_stats=True)
    res.update(st, covered_share=round(float((out[..., 3] != 0).float().mean()), 4))
    # the pass alone
    pts = torch.empty((K, S, 2), dtype=torch.int32, device=dev)
    boxes = torch.empty((K, 4), dtype=torch.int32, device=dev)
    _lib.check(lib.cpn_labels_prepare(_lib.ptr(con), K, S, size, size, 1, 1, _lib.ptr(pts), _lib.ptr(boxes), _lib.stream_ptr()), 'prepare')
    l_ms, l_all, (begin, lst, pairs) = event_ms(lambda: _tile_lists(lib, boxes, K, size, size), repeats)
    most = torch.zeros(1, dtype=torch.int32, device=dev)
    host = c_uint32(0)
    paint = lambda: _lib.check(lib.cpn_overlay_paint(_lib.ptr(pts), _lib.ptr(boxes), _lib.ptr(col), K, S, size, size, _lib.ptr(begin),
                                                     _lib.ptr(lst), _lib.ptr(out), _lib.ptr(most), None, _lib.stream_ptr()), 'paint')
    p_ms, p_all, _ = event_ms(paint, repeats)
    del pts, boxes, begin, lst
    o_ms, o_all, again = event_ms(lambda: cda.contours2overlay(con, (size, size), colors=col, intermediate_dtype='uint32'), repeats)
    res.update(paint_ms=round(p_ms, 3), paint_ms_all=p_all, paint_gb_per_s_written=round(size * size * 4 / p_ms / 1e6, 1),
               lists_ms=round(l_ms, 3), lists_ms_all=l_all, overlay_call_ms=round(o_ms, 3), overlay_call_ms_all=o_all,
               overlay_repeatable=bool(torch.equal(again, out)))
    del out, again
    c_ms, c_all, labels = event_ms(lambda: cda.contours2labels(con, (size, size)), max(repeats // 2, 1))
    res.update(labels_call_ms=round(c_ms, 3), labels_call_ms_all=c_all, label_channels=int(labels.shape[2]),
               labels_call_over_overlay_call=round(c_ms / o_ms, 1))
    made = int(labels.shape[2])
    lab3 = labels[:, :, :3].contiguous() if made >= 3 else torch.cat((labels, labels.new_zeros((size, size, 3 - made))), 2)
    flat = cda.resolve_label_channels(labels)
    del labels
    np.random.seed(0)
    colors = cda.random_colors_hsv(9999)
    table = torch.as_tensor(_color_table(colors, 1, None)).to(dev)
    for name, x in (('cmap3', lab3), ('cmap1', flat)):
        k_ms, k_all, got = event_ms(lambda: cda.label_cmap(x, colors=colors, ubyte=True), repeats)
        s_ms, s_all, exp = event_ms(lambda: stock_cmap(x, table), max(repeats // 2, 1))
        res.update({f'{name}_ms': round(k_ms, 3), f'{name}_ms_all': k_all, f'{name}_stock_ms': round(s_ms, 3),
                    f'{name}_stock_ms_all': s_all, f'{name}_stock_equal': bool(torch.equal(got, exp)),
                    f'{name}_stock_over_kernel': round(s_ms / k_ms, 1),
                    f'{name}_gb_per_s': round((x.numel() * 4 + size * size * 4) / k_ms / 1e6, 1)})
        del got, exp
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--one':
        one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]))
        return
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    counts = [int(c) for c in sys.argv[2].split(',')] if len(sys.argv) > 2 else [100000, 1000000]
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    radius = float(sys.argv[4]) if len(sys.argv) > 4 else .6
    limit = float(sys.argv[5]) if len(sys.argv) > 5 else 300.
    for objects in counts:  # a fresh process per step, under its own time limit; nothing more is started after a failure
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', str(size), str(objects), str(repeats), str(radius)],
                                timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f'objects {objects}: no result within {limit:.0f} s', flush=True)
            sys.exit(124)
        if rc != 0:
            print(f'objects {objects}: exit status {rc}', flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == '__main__':
    main()
