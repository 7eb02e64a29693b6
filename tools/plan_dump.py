"""Dumps everything the native plan executor decides on the host, for comparing two builds of it without a GPU.

    CPN_HIP_LIB=/path/to/libcpn_hip.so python tools/plan_dump.py --out dump.txt > summary.txt

Plans: every entry of tests/model_specs.ALL_SPECS plus the two full-width bench models (CpnResNeXt101UNet, CpnResNet50FPN), each
in bf16 (plain and with score-gated heads), fp32 and -- where it packs -- fp8, packed on the CPU (planning never dereferences a
blob).  Grid: N in BATCHES x (H, W) in SIZES x the settings of the executor's switches in SWITCHES.  Per combination the dump holds cpn_plan_workspace_bytes,
cpn_plan_max_tensor_elements, cpn_plan_output_dims of all outputs, cpn_plan_executed_flops and cpn_plan_tensor_info (or its error
text) of every tensor.  Two builds decide the same iff their dump files are equal.

The summary (stdout) has one line per plan with the SHA-1 of its part of the dump, and counts, per size-dependent decision, the
combinations where it was taken / not taken -- a comparison over a grid in which a decision never flips would be vacuous:
  head    sub-pixel triple: the phase tensor of a CPN_SUBPIXEL_HEAD unit is written      (default switches)
  bl      bilinear triple: executed FLOPs differ from those under CPN_BLPHASE=0           (default switches)
  stem    fast stem pair: executed FLOPs differ from those of the plan built with stem_fast=False
  pair    conv pair: the tensor between the two convs a CPN_OP_CONV_PAIR op restates is never written
  bridge  bridge fusion: the same for a CPN_OP_CONV_BRIDGE op
(3 x 3 is in the grid for the stem alone: the padded 4-channel input layout fits the input tensor from 4 x 4 pixels on.)
"""
import argparse
import hashlib
import os
import sys
from collections import Counter
from ctypes import byref, c_int32, c_int64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

BATCHES = (1, 2, 16)
SIZES = ((64, 64), (64, 96), (75, 101), (100, 140), (512, 512), (3, 3))
SWITCHES = ({}, {'CPN_BLPHASE': '0'}, {'CPN_BLPHASE': '2'}, {'CPN_PAIR': '0'}, {'CPN_PAIR': '2'}, {'CPN_BRIDGE': '0'})
PRECISIONS = ('bf16', 'bf16g', 'fp32', 'fp8')  # bf16g: the bf16 plan with score-gated (deferred) heads
FULL_WIDTH = {'full_CpnResNeXt101UNet': dict(cls='CpnResNeXt101UNet', kwargs=dict(in_channels=3)),
              'full_CpnResNet50FPN': dict(cls='CpnResNet50FPN', kwargs=dict(in_channels=3))}


def packed_plans(precisions=PRECISIONS, generic_stem=False):
    """Yields (name, precision, tensor descs, op descs, weight blob, bias blob) of every plan of the comparison; with
    ``generic_stem`` additionally the descriptors of the same plan built without the fast stem pair (or None)."""
    import celldetection_amd as cda
    from celldetection_amd import graph
    from celldetection_amd.synth import synth_state_dict
    from model_specs import ALL_SPECS
    for name, spec in list(ALL_SPECS.items()) + list(FULL_WIDTH.items()):
        model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
        sd = synth_state_dict(model.state_dict(), seed=0) if name in FULL_WIDTH else model.state_dict()
        for label in precisions:
            precision = label.rstrip('g')
            plan = model.plan_for(precision, gate=True) if label == 'bf16g' else model.plan_for(precision)
            kw = dict(act_scales=[.01 + .001 * i for i in range(len(plan.tensors))]) if precision == 'fp8' else {}
            try:
                out = graph.pack(plan, sd, 'cpu', precision=precision, **kw)[:4]
            except NotImplementedError as e:  # (bicubic resize ops: bf16 / fp32 plans only)
                yield (name, label, str(e), None, None, None) + ((None,) if generic_stem else ())
                continue
            if not generic_stem:
                yield (name, label) + tuple(out)
                continue
            generic = None
            if precision == 'bf16' and any(o.get('alt') for o in plan.ops):  # the same plan without the fast stem pair
                gplan = graph.build_plan(**model._plan_kwargs, sparse_heads=label == 'bf16g', subpixel=bool(model.subpixel),
                                         stem_fast=False, fuse_blocks=True, bilinear_phases=bool(model.subpixel))
                generic = graph.pack(gplan, sd, 'cpu', precision=precision)[:4]
            yield (name, label) + tuple(out) + (generic,)


def create(lib, tens, ops, wblob, bblob, precision):
    from celldetection_amd import _lib
    handle = c_void_p()
    code = {'bf16': _lib.PRECISION_BF16, 'fp32': _lib.PRECISION_F32, 'fp8': _lib.PRECISION_FP8}[precision.rstrip('g')]
    _lib.check(lib.cpn_plan_create(handle, tens, len(tens), ops, len(ops), _lib.ptr(wblob), wblob.numel() * wblob.element_size(),
                                   _lib.ptr(bblob), bblob.numel(), code), 'plan_create')
    return handle


def set_switches(setting):
    for k in ('CPN_BLPHASE', 'CPN_PAIR', 'CPN_BRIDGE'):
        os.environ.pop(k, None)
    os.environ.update(setting)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True, help='file that receives the full dump')
    ap.add_argument('--only', default=None, help='substring of the plan names to dump')
    args = ap.parse_args()
    from celldetection_amd import _lib
    lib = _lib.load()
    err = lambda: lib.cpn_last_error().decode()
    total = hashlib.sha1()
    grand = Counter()
    print(f'grid: N {BATCHES} x (H, W) {SIZES} x switches {[s or "default" for s in SWITCHES]}')
    with open(args.out, 'w') as out:
        for name, precision, tens, ops, wblob, bblob, generic in packed_plans(generic_stem=True):
            if args.only and args.only not in name:
                continue
            if ops is None:
                print(f'{name:34s} {precision:5s} not packed: {tens[:60]}')
                continue
            plan = create(lib, tens, ops, wblob, bblob, precision)
            gplan = create(lib, *generic, precision) if generic else None
            sha, taken = hashlib.sha1(), Counter()
            heads = [i for i, o in enumerate(ops) if o.op == _lib.OP_CONV and o.subpixel == _lib.SUBPIXEL_HEAD]
            has_bl = any(o.subpixel == _lib.SUBPIXEL_BL_HEAD for o in ops)
            fused = {kind: [i for i, o in enumerate(ops) if o.op == kind] for kind in (_lib.OP_CONV_PAIR, _lib.OP_CONV_BRIDGE)}
            for n in BATCHES:
                for h, w in SIZES:
                    flops = {}
                    for si, setting in enumerate(SWITCHES):
                        set_switches(setting)
                        lines = [f'## {name} {precision} N={n} H={h} W={w} {setting or "default"}']
                        ws = lib.cpn_plan_workspace_bytes(plan, n, h, w)
                        lines.append(f'workspace {ws}' + (f' ({err()})' if ws < 0 else ''))
                        lines.append(f'max_tensor_elements {lib.cpn_plan_max_tensor_elements(plan, h, w)}')
                        oh, ow = c_int32(), c_int32()
                        for k in range(_lib.NUM_OUTPUTS):
                            rc = lib.cpn_plan_output_dims(plan, h, w, k, byref(oh), byref(ow))
                            lines.append(f'output {k} ' + (f'{oh.value} x {ow.value}' if rc == 0 else f'error {rc} ({err()})'))
                        flops[si] = lib.cpn_plan_executed_flops(plan, n, h, w)
                        lines.append(f'executed_flops {flops[si]!r}' + (f' ({err()})' if flops[si] < 0 else ''))
                        unwritten = set()
                        off, th, tw, cs = c_int64(), c_int32(), c_int32(), c_int32()
                        for t in range(len(tens)):
                            rc = lib.cpn_plan_tensor_info(plan, n, h, w, t, byref(off), byref(th), byref(tw), byref(cs))
                            if rc:
                                unwritten.add(t)
                                lines.append(f'tensor {t} error {rc} ({err()})')
                            else:
                                lines.append(f'tensor {t} offset {off.value} {th.value} x {tw.value} x {cs.value}')
                        text = '\n'.join(lines) + '\n'
                        out.write(text)
                        sha.update(text.encode())
                        if si == 0 and ws >= 0:  # the decisions of the default setting
                            for i in heads:
                                taken['head', ops[i + 1].dst not in unwritten] += 1
                            for kind, key in ((_lib.OP_CONV_PAIR, 'pair'), (_lib.OP_CONV_BRIDGE, 'bridge')):
                                for i in fused[kind]:
                                    taken[key, ops[i - 2].dst in unwritten] += 1
                            if gplan is not None:
                                taken['stem', lib.cpn_plan_executed_flops(gplan, n, h, w) != flops[0]] += 1
                    if has_bl and flops[0] >= 0:
                        taken['bl', flops[0] != flops[1]] += 1
            lib.cpn_plan_destroy(plan)
            if gplan is not None:
                lib.cpn_plan_destroy(gplan)
            total.update(sha.digest())
            grand.update(taken)
            counts = ' '.join(f'{k} {taken[k, True]}/{taken[k, False]}' for k in ('head', 'bl', 'stem', 'pair', 'bridge')
                              if taken[k, True] + taken[k, False])
            print(f'{name:34s} {precision:5s} {len(ops):3d} ops {sha.hexdigest()}  taken/not: {counts}')
    set_switches({})
    print('decisions over the whole grid, taken / not taken: ' +
          ', '.join(f'{k} {grand[k, True]} / {grand[k, False]}' for k in ('head', 'bl', 'stem', 'pair', 'bridge')))
    print(f'dump sha1 {total.hexdigest()}')
    return 0 if all(grand[k, True] and grand[k, False] for k in ('head', 'bl', 'stem', 'pair', 'bridge')) else 1


if __name__ == '__main__':
    sys.exit(main())
