"""Digests everything plan building and weight packing produce, for comparing two versions of them byte for byte without a GPU.

    python tools/pack_digest.py > digest.txt

Plans: the grid of tools/plan_dump.py -- every entry of tests/model_specs.ALL_SPECS plus the two full-width bench models, each in
bf16, bf16g (score-gated heads), fp32 and fp8 -- packed on the CPU, ``torch.manual_seed(0)`` in front of every model.  One line per
plan: the SHA-1 over the plan (entries, tensors, ops, meta), both descriptor arrays, the weight and the bias blob and, for fp8, the
multiplier blob, the op scales and every ``effective_weights`` entry.  A plan that does not pack contributes its exception text.
The last line is the SHA-1 over all plans: two versions pack the same iff their outputs are equal.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)


def _blob_bytes(t):
    import torch
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def plan_digests(only=None):
    """Yields (name, precision label, number of ops, hex digest, note) per plan of the grid."""
    import torch
    import celldetection_amd as cda
    from celldetection_amd import graph
    from celldetection_amd.synth import synth_state_dict
    from model_specs import ALL_SPECS
    from plan_dump import FULL_WIDTH, PRECISIONS
    for name, spec in list(ALL_SPECS.items()) + list(FULL_WIDTH.items()):
        if only and only not in name:
            continue
        torch.manual_seed(0)
        model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
        sd = synth_state_dict(model.state_dict(), seed=0) if name in FULL_WIDTH else model.state_dict()
        for label in PRECISIONS:
            precision = label.rstrip('g')
            plan = model.plan_for(precision, gate=True) if label == 'bf16g' else model.plan_for(precision)
            sha = hashlib.sha1()
            for part in (plan.entries, plan.tensors, plan.ops, sorted(plan.meta.items())):
                sha.update(repr(part).encode())
            kw, eff, note = {}, [], ''
            if precision == 'fp8':
                kw = dict(act_scales=[.01 + .001 * i for i in range(len(plan.tensors))], effective_weights=eff)
            try:
                out = graph.pack(plan, sd, 'cpu', precision=precision, **kw)
            except Exception as e:  # (e.g. a bicubic resize op in an fp8 plan)
                note = f'not packed: {type(e).__name__}: {e}'
                sha.update(note.encode())
                yield name, label, len(plan.ops), sha.hexdigest(), note[:72]
                continue
            tens, ops, wblob, bblob = out[:4]
            for part in (bytes(tens), bytes(ops), _blob_bytes(wblob), _blob_bytes(bblob)):
                sha.update(part)
            if precision == 'fp8':
                sha.update(_blob_bytes(out[4]))
                sha.update(repr(out[5]).encode())
                for e in eff:
                    for key in ('w', 'b'):
                        sha.update(b'None' if e[key] is None else _blob_bytes(e[key].to(torch.float64)))
            yield name, label, len(plan.ops), sha.hexdigest(), note


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    total, count = hashlib.sha1(), 0
    for name, label, nops, digest, note in plan_digests(only):
        total.update(digest.encode())
        count += 1
        print(f'{name:34s} {label:5s} {nops:3d} ops {digest}  {note}'.rstrip())
    print(f'{count} plans, pack sha1 {total.hexdigest()}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
