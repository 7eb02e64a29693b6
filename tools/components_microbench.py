"""Times component labelling (cda.label_components / relabel_ / masks2labels) on slide-sized label images and prints one JSON
line per step.
    python tools/components_microbench.py [size=16384] [objects=100000,1000000] [repeats=5] [radius=0.6] [limit_s=300]
    python tools/components_microbench.py --ab <other libcpn_hip.so> [size] [objects] [repeats] [radius] [limit_s] [rounds=3]
    python tools/components_microbench.py --kernels <size> <objects> [radius]     (the workload only, for a kernel trace)

Steps, each in a child process of its own under ``limit_s`` seconds (the first one that fails or runs out of time ends the tool):
  labels3   the first 3 channels of ``contours2labels`` of the seeded circle grid of ``tools/eval_microbench.py``, per object count
            (the images of ``tools/label_contours_microbench.py``)
  masks     25 binary masks of 256 x 256 (seeded discs), the shape the reference's docstring times at 11.7 ms on a CPU host
Reported, in device-event ms (one warm-up call, then the median of ``repeats``; every call ends with a host read, which is inside
its time):
  label8_ms / label4_ms  ``label_components`` out of place at connectivity 8 / 4: components pass, numbering, labelling
  relabel_ms             ``relabel_`` as a whole, in place on a fresh copy of the image (the copy is outside the time)
  contours_components_ms ``cpn_contours_components``, the pass ``labels2contours`` runs on the shared header
  copy_ms                one streaming copy of the image (``labels.clone()``): the yardstick
  masks2labels_ms        ``masks2labels(masks)`` with its defaults (8-connectivity, channel maximum)
The launches of one call (components pass: local, seam, flatten; numbering: count, scan, rank, label) are separated by a kernel
trace of the ``--kernels`` workload (three ``label_components`` calls per connectivity), taken in a run of its own.
``--ab``: per image one child that times ``cpn_contours_components`` of the other library and of this tree's in turn, ``rounds``
times (other this, this other, ...; each time one warm-up call and ``repeats`` timed calls); prints both medians over all timed
calls and each library's own run-to-run spread (its slowest minus its fastest call).  The other library is loaded by its path next to the tree's own (which builds
the image): ``CPN_HIP_LIB`` cannot select a library from before this feature, because the binding refuses a library that lacks
an entry point it declares.
These are records, not gates: there is no preset target."""
import json
import os
import subprocess
import sys
from ctypes import c_int64

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def image(size, objects, radius):
    import torch
    import celldetection_amd as cda
    from eval_microbench import contours
    dev = torch.device('cuda:0')
    labels = cda.contours2labels(torch.as_tensor(contours(size, objects, 0, radius=radius)).to(dev), (size, size))
    made = int(labels.shape[2])
    return labels[:, :, :3].contiguous() if made >= 3 else torch.cat((labels, labels.new_zeros((size, size, 3 - made))), 2)


def contours_components_ms(labels, repeats, lib_path=None, buffers=None):
    """lib_path: time this library's cpn_contours_components instead of the tree's (loaded next to it, its own kernels).
    buffers: a dict that keeps the roots image and the workspace from one call to the next (the same memory for both libraries)."""
    import torch
    from celldetection_amd import _lib
    from celldetection_amd._lib import ptr, stream_ptr
    from flat_labels_microbench import event_ms
    lib = _lib.bind(lib_path) if lib_path else _lib.load()

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f'{what} failed (code {rc})')
    H, W, C = (int(s) for s in labels.shape)
    nbytes = int(lib.cpn_contours_workspace_bytes(0))
    buffers = {} if buffers is None else buffers
    if 'roots' not in buffers:
        buffers['roots'] = torch.empty((C, H, W), dtype=torch.int32, device=labels.device)
        buffers['ws'] = torch.empty((nbytes,), dtype=torch.uint8, device=labels.device)
    roots, ws = buffers['roots'], buffers['ws']
    status = (c_int64 * 2)()

    def run():
        check(lib.cpn_contours_components(ptr(labels), C, H, W, ptr(roots), ptr(ws), nbytes, status, stream_ptr()), 'components')
        return int(status[0])
    return event_ms(run, repeats)


def one(kind, size, objects, repeats, radius, other=None, rounds=3):
    import torch
    import celldetection_amd as cda
    from flat_labels_microbench import event_ms
    dev = torch.device('cuda:0')
    if kind == 'masks':
        yy, xx = torch.meshgrid(torch.arange(256, device=dev), torch.arange(256, device=dev), indexing='ij')
        rng = np.random.default_rng(0)
        masks = torch.zeros((25, 256, 256), dtype=torch.uint8, device=dev)
        for i in range(25):
            for cy, cx, r in zip(rng.uniform(0, 256, 12), rng.uniform(0, 256, 12), rng.uniform(6, 20, 12)):
                masks[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
        ms, runs, out = event_ms(lambda: cda.masks2labels(masks), repeats)
        print(json.dumps(dict(step='masks', shape=list(masks.shape), components=int(out.max()), masks2labels_ms=round(ms, 3),
                              masks2labels_ms_all=runs)), flush=True)
        return
    labels = image(size, objects, radius)
    res = dict(step=kind, size=size, objects_asked=objects, channels=int(labels.shape[2]), bytes_read=labels.numel() * 4)
    if kind == 'ab':  # nothing but the shared pass, the two libraries in turn
        from celldetection_amd import _lib
        ms, every, buffers = dict(other=[], this=[]), dict(other=[], this=[]), {}
        for r in range(rounds):  # other this, this other, ...: neither library is always the first of a round
            order = (('other', other), ('this', _lib.LIB_PATH))
            for name, path in (order if r % 2 == 0 else order[::-1]):
                m, runs, n = contours_components_ms(labels, repeats, path, buffers)
                ms[name].append(round(m, 3))
                every[name] += runs
                res[f'components_{name}'] = n
        for name, v in ms.items():  # spread: the largest minus the smallest of all single calls of that library
            res.update({f'{name}_ms': round(float(np.median(every[name])), 3), f'{name}_round_medians': v, f'{name}_calls': every[name],
                        f'{name}_spread_ms': round(max(every[name]) - min(every[name]), 3)})
        res['difference_ms'] = round(res['this_ms'] - res['other_ms'], 3)
        print(json.dumps(res), flush=True)
        return
    ms, runs, n = contours_components_ms(labels, repeats)
    res.update(components=n, contours_components_ms=round(ms, 3), contours_components_ms_all=runs)
    for conn in (8, 4):
        ms, runs, (out, counts) = event_ms(lambda: cda.label_components(labels, conn), repeats)
        again = cda.label_components(labels, conn)[0]
        res.update({f'label{conn}_ms': round(ms, 3), f'label{conn}_ms_all': runs, f'components{conn}': int(counts.sum()),
                    f'repeatable{conn}': bool(torch.equal(again, out))})
        del out, again
    copies = [labels.clone() for _ in range(repeats + 1)]
    ms, runs, _ = event_ms(lambda: cda.relabel_(copies.pop()), repeats)
    res.update(relabel_ms=round(ms, 3), relabel_ms_all=runs)
    del copies
    ms, runs, _ = event_ms(lambda: labels.clone(), repeats)
    res.update(copy_ms=round(ms, 3), copy_ms_all=runs, label8_over_copy=round(res['label8_ms'] / ms, 1))
    print(json.dumps(res), flush=True)


def kernels(size, objects, radius):
    import torch
    import celldetection_amd as cda
    labels = image(size, objects, radius)
    for conn in (8, 4):
        for _ in range(3):
            cda.label_components(labels, conn)
    torch.cuda.synchronize()


def child(args, limit):
    """-> the JSON lines the child printed; ends the tool when the child fails or runs out of time."""
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), '--one'] + [str(a) for a in args], timeout=limit,
                             stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        print(f'{args}: no result within {limit:.0f} s', flush=True)
        sys.exit(124)
    if run.returncode != 0:
        print(run.stdout[-2000:], flush=True)
        print(f'{args}: exit status {run.returncode}', flush=True)
        sys.exit(run.returncode if run.returncode > 0 else 1)
    return [json.loads(line) for line in run.stdout.splitlines() if line.startswith('{')]


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == '--one':
        one(argv[1], int(argv[2]), int(argv[3]), int(argv[4]), float(argv[5]), *(argv[6:7] + [int(a) for a in argv[7:8]]))
        return
    if argv and argv[0] == '--kernels':
        kernels(int(argv[1]), int(argv[2]), float(argv[3]) if len(argv) > 3 else .6)
        return
    other = None
    if argv and argv[0] == '--ab':
        other, argv = os.path.abspath(argv[1]), argv[2:]
    size = int(argv[0]) if len(argv) > 0 else 16384
    counts = [int(c) for c in argv[1].split(',')] if len(argv) > 1 else [100000, 1000000]
    repeats = int(argv[2]) if len(argv) > 2 else 5
    radius = float(argv[3]) if len(argv) > 3 else .6
    limit = float(argv[4]) if len(argv) > 4 else 300.
    if other is None:
        for objects in counts:
            for line in child(('labels3', size, objects, repeats, radius), limit):
                print(json.dumps(line), flush=True)
        for line in child(('masks', 256, 0, repeats, radius), limit):
            print(json.dumps(line), flush=True)
        return
    rounds = int(argv[5]) if len(argv) > 5 else 3
    for objects in counts:
        for line in child(('ab', size, objects, repeats, radius, other, rounds), limit):
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
