"""Launch trace of the native plan executor without a GPU: what cpn_plan_run hands to every launcher, as text.

    python -m celldetection_amd.build                      # the conv kernel objects the trace program links
    python tools/plan_trace.py --workdir DIR               # this tree's executor      -> DIR/trace.txt, DIR/malformed_trace.txt
    python tools/plan_trace.py --workdir DIR2 --executor OTHER/celldetection_amd/csrc/cpn_abi.hip     # another commit's
    python tools/plan_trace.py --workdir DIR3 --sanitize   # the same program under host ASan + UBSan

Two executors launch the same iff their trace.txt files are equal.  The program is tools/plan_trace_main.hip: the executor's host
units + the real conv kernel objects (kernel selection, pair support, FLOP functions), with the launch_* references of the unit
that holds the run loop renamed to recording stand-ins on its compile line; no hook in product code, no HIP call on the path.
Plans: those of tools/plan_dump.py, N = 2 at 64 x 96, 75 x 101 and 512 x 512.  malformed_trace.txt: every malformed plan of
tests/test_plan_validation.py, created and -- where creation accepts it -- planned and run at the size of its case.
--sanitize compiles the host units and the program with -fsanitize=address,undefined (host side only; the program is stand-alone,
runs on the CPU and is never loaded into another process); a clean run prints no report and exits 0.
"""
import argparse
import ctypes
import hashlib
import os
import re
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)
CSRC = os.path.join(ROOT, 'celldetection_amd', 'csrc')
EXECUTOR = [os.path.join(CSRC, f) for f in ('plan_validate.hip', 'plan_shapes.hip', 'conv_args.hip', 'cpn_abi.hip')]
KERNEL_OBJECTS = ('conv_igemm.o', 'conv_fp8.o', 'conv_pair.o')
SIZES = ((2, 64, 96), (2, 75, 101), (2, 512, 512))


def write_record(f, name, precision, tens, ops, weight_bytes, bias_count, sizes):
    from celldetection_amd import _lib
    code = {'bf16': _lib.PRECISION_BF16, 'fp32': _lib.PRECISION_F32, 'fp8': _lib.PRECISION_FP8}.get(precision, precision)
    raw = name.encode()
    f.write(struct.pack('<i', len(raw)) + raw)
    f.write(struct.pack('<4i2q', code, len(tens), len(ops), len(sizes), weight_bytes, bias_count))
    f.write(struct.pack(f'<{3 * len(sizes)}i', *[v for s in sizes for v in s]))
    f.write(bytes(tens) + bytes(ops))


def export(workdir):
    """The raw TensorDesc / OpDesc bytes + blob sizes of every plan -> workdir/plans.bin, workdir/malformed.bin"""
    from celldetection_amd import _lib
    from plan_dump import packed_plans
    import test_plan_validation as tv
    header = struct.pack('<2i', ctypes.sizeof(_lib.TensorDesc), ctypes.sizeof(_lib.OpDesc))
    with open(os.path.join(workdir, 'plans.bin'), 'wb') as f:
        f.write(header)
        for name, precision, tens, ops, wblob, bblob in packed_plans():
            if ops is not None:
                write_record(f, f'{name} {precision}', precision.rstrip('g'), tens, ops, wblob.numel() * wblob.element_size(), bblob.numel(), SIZES)
    with open(os.path.join(workdir, 'malformed.bin'), 'wb') as f:
        f.write(header)
        cases = [c[:6] + ((1, 64, 64),) for c in tv.CREATE_CASES + tv.INDEX_CASES] + [c[:7] for c in tv.PLANNING_CASES]
        for name, base, precision, target, field, value, size in cases:
            tens, ops, wblob, bblob = tv.mutate(base, precision, target, field, value)
            write_record(f, name, precision, tens, ops, wblob.numel() * wblob.element_size(), bblob.numel(), [size])
        valid = tv.mutate('u22', 'bf16', None, None, None)
        write_record(f, 'unknown_precision', 7, valid[0], valid[1], valid[2].numel() * 2, valid[3].numel(), [])


def build(workdir, executor, sanitize):
    from celldetection_amd.build import ARCH, _hipcc
    names = sorted(set(re.findall(r'\bint (launch_\w+)\(', open(os.path.join(CSRC, 'cpn_kernels.h')).read())))
    renames = [f'-D{n}=trace_{n}' for n in names]
    san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-omit-frame-pointer', '-g'] if sanitize else []
    objs = []
    for src in executor + [os.path.join(ROOT, 'tools', 'plan_trace_main.hip')]:
        obj = os.path.join(workdir, os.path.basename(src).replace('.hip', '.o'))
        extra = renames if os.path.basename(src) in ('cpn_abi.hip', 'plan_trace_main.hip') else []
        subprocess.check_call([_hipcc(), f'--offload-arch={ARCH}', '-O1' if sanitize else '-O2', '-std=c++17', '-fPIC', '-c', src, '-o', obj] +
                              extra + san)
        objs.append(obj)
    kernels = [os.path.join(ROOT, 'celldetection_amd', 'build', o) for o in KERNEL_OBJECTS]
    exe = os.path.join(workdir, 'plan_trace')
    subprocess.check_call([_hipcc(), f'--offload-arch={ARCH}'] + objs + kernels + ['-o', exe] +
                          (['-fsanitize=address,undefined'] if sanitize else []))
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workdir', required=True)
    ap.add_argument('--executor', nargs='+', default=EXECUTOR, help="the executor's host sources (default: this tree's units)")
    ap.add_argument('--sanitize', action='store_true')
    ap.add_argument('--each', action='store_true', help='run every malformed plan in a process of its own and print how it ended')
    args = ap.parse_args()
    os.makedirs(args.workdir, exist_ok=True)
    export(args.workdir)
    exe = build(args.workdir, [os.path.abspath(e) for e in args.executor], args.sanitize)
    if args.each:  # (an executor without the index checks: its first sanitizer report ends the process)
        import test_plan_validation as tv
        for case in tv.CREATE_CASES + tv.PLANNING_CASES + tv.INDEX_CASES:
            r = subprocess.run([exe, os.path.join(args.workdir, 'malformed.bin'), case[0]], capture_output=True, text=True)
            report = [l for l in r.stderr.splitlines() if 'Sanitizer' in l or 'runtime error' in l][:1]
            print(f'{case[0]:32s} exit {r.returncode:4d}  {r.stdout.splitlines()[0][:90] if r.stdout else ""}  {report[0][:150] if report else "no report"}')
        return 0
    status = 0
    for records, trace in (('plans.bin', 'trace.txt'), ('malformed.bin', 'malformed_trace.txt')):
        with open(os.path.join(args.workdir, trace), 'wb') as out:
            rc = subprocess.call([exe, os.path.join(args.workdir, records)], stdout=out)
        text = open(os.path.join(args.workdir, trace), 'rb').read()
        print(f'{trace}: exit {rc}, {text.count(b"## run 0")} runs, {sum(l.startswith(b"  ") for l in text.splitlines())} launches, '
              f'sha1 {hashlib.sha1(text).hexdigest()}')
        status |= rc
    return status


if __name__ == '__main__':
    sys.exit(main())
