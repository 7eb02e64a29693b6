"""Compares the conv kernels a profiler saw with the case table of tests/conv_tiles.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python -m pytest tests/test_gpu_conv_tiles.py -m gpu
    python tools/conv_tile_trace.py DIR > profiles/conv_tile_coverage.txt

Reads every *kernel_stats*.csv / *kernel_trace*.csv under DIR, takes the conv_igemm_kernel<TH, BN, WM, WN, MODE> names (the
cpn:: namespace is the bf16 unit, cpn_fp8:: the e4m3 unit) with their dispatch counts, and prints them next to the keys of
the table: the two sets must be equal -- what cpn_conv2d_kernel_info says a case runs is what ran.  Exit status 1 otherwise.
"""
import csv
import glob
import os
import re
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
csv.field_size_limit(1 << 30)

NAME = re.compile(r'(cpn|cpn_fp8)::conv_igemm_kernel<(\d+), ?(\d+), ?(\d+), ?(\d+), ?\(?(?:cpn::)?(?:Mode\)?)?(\d+)>')


def traced(d):
    from celldetection_amd import _lib
    stats, trace = Counter(), Counter()
    for f in sorted(glob.glob(os.path.join(d, '**', '*.csv'), recursive=True)):
        base = os.path.basename(f)
        if 'kernel_stats' in base:
            rows, col, into = csv.DictReader(open(f)), 'Name', stats
        elif 'kernel_trace' in base:
            rows, col, into = csv.DictReader(open(f)), 'Kernel_Name', trace
        else:
            continue
        for r in rows:
            m = NAME.search(r.get(col) or '')
            if m:
                th, bn, wm, wn, mode = (int(x) for x in m.groups()[1:])
                key = f'{"bf16" if m.group(1) == "cpn" else "e4m3"}/{_lib.CONV_MODE_NAMES[mode]}/{th}x{bn} <{th},{bn},{wm},{wn}>'
                into[key] += int(float(r['Calls'])) if into is stats else 1
    return trace or stats


def main(d):
    import conv_tiles as ct
    seen = traced(d)
    lib = ct.library_instantiations()
    want = {f'{k} <{ct.parse_key(k)[2]},{ct.parse_key(k)[3]},{lib[k][0]},{lib[k][1]}>' for k in map(ct.instantiation, ct.TABLE)}
    print(f'conv_igemm_kernel instantiations: {len(want)} table keys, {len(seen)} kernel names in the trace, '
          f'{sum(seen.values())} dispatches')
    print(f'{"instantiation":34s} {"table":>6s} {"dispatches":>11s}')
    for k in sorted(want | set(seen)):
        print(f'{k:34s} {"yes" if k in want else "NO":>6s} {seen.get(k, 0):11d}')
    print('compiled, selected by no valid call (conv_tiles.UNREACHABLE), not in the trace: ' + ', '.join(sorted(ct.UNREACHABLE)))
    missing, extra = sorted(want - set(seen)), sorted(set(seen) - want)
    if missing or extra:
        print(f'MISMATCH: table keys that did not run: {missing}; kernels that ran without a key: {extra}')
        return 1
    print('trace names == table keys')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1]))
