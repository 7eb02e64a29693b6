"""Golden-vector generator of the elliptic Fourier descriptors (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and runs its own ``efd`` and ``contours2fourier``
(celldetection/data/cpn.py:23-90, 213-227) on small cases; writes ``fourier.npz`` next to this file: per case the inputs, the
keywords and the reference's float64 results.  Arrays only.  ``efd`` is pure numpy in the reference, so everything is pinned.

Cases: ``efd.<name>`` with ``points`` (the contours one after the other), ``lengths``, ``lead`` (the leading shape of a dense array, or
-1 for a list), ``order``, ``epsilon``, ``autoclose``, ``coefficients`` [K, order, 4], ``locations`` [K, 2]; ``c2f.<name>`` with ``keys``,
``points``, ``lengths``, ``squeeze`` (1: the contour was given as [n, 1, 2]), ``order`` and the results as float64 and float32.

Run:  python tests/golden/make_golden_fourier.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import ref_shim  # noqa: E402

ref_shim.import_reference()
import celldetection.data.cpn as ref_cpn  # noqa: E402
import fourier_oracle as oracle  # noqa: E402


def efd_cases():
    """-> [(name, contours (an array [..., n, 2] or a list of arrays [n_k, 2]), order, epsilon, autoclose)]."""
    walk = oracle.ragged_walk
    rng = np.random.default_rng(3)
    cases = [('open_int', walk(37, 1, center=(40, 60)), 10, 1e-6, True),
             ('closed_int', walk(37, 2, closed=True, center=(90, 30)), 10, 1e-6, True),
             ('closed_no_autoclose', walk(21, 3, closed=True, center=(50, 50)), 10, 1e-6, False),
             ('one_point', np.asarray([[7, 9]], np.int32), 5, 1e-6, True),
             ('doubled_point', np.asarray([[7, 9], [7, 9]], np.int32), 5, 1e-6, True),
             ('two_points', np.asarray([[3, 4], [8, 6]], np.int32), 5, 1e-6, True),
             ('three_points', np.asarray([[3, 4], [8, 6], [5, 11]], np.int32), 5, 1e-6, True)]
    closed = np.stack([walk(8, 10 + i, closed=True, center=(30 + 9 * i, 40)) for i in range(3)])
    one_open = closed.copy()
    one_open[1, -1] += (2, 1)
    cases += [('dense_closed', closed.reshape(3, 1, 9, 2), 5, 1e-6, True), ('dense_one_open', one_open, 5, 1e-6, True)]
    cases.append(('object_list', [walk(n, 20 + n, closed=bool(n % 2), center=(100 + n, 80)) for n in (5, 12, 1, 30, 9, 64)], 7, 1e-6,
                  True))
    ring = 16000. + 25. * np.stack([np.cos(np.linspace(0, 2 * np.pi, 41)), np.sin(np.linspace(0, 2 * np.pi, 41))], -1)
    ring += rng.uniform(-.3, .3, ring.shape)
    loose = ring.copy()
    loose[-1] = loose[0] + (0.1, -0.12)  # |first - last| <= 1e-8 + 1e-5 * 16000 = 0.16: allclose calls it closed
    apart = ring.copy()
    apart[-1] = loose[0] + (0.1, -0.3)  # not closed: 0.3 > 0.16
    cases += [('float_16000_loose', loose, 5, 1e-6, True), ('float_16000_apart', apart, 5, 1e-6, True),
              ('float_small', rng.uniform(2, 60, (23, 2)), 10, 1e-6, True)]
    cases += [(f'order_{o}', walk(90, 5, center=(120, 140)), o, 1e-6, True) for o in (1, 5, 10, 25)]
    cases += [('epsilon_1e-3', walk(50, 6, center=(70, 90)), 10, 1e-3, True),
              ('two_chunks', walk(oracle.CHUNK + 44, 8, center=(400, 300)), 5, 1e-6, True)]
    return cases


def c2f_cases():
    walk = oracle.ragged_walk
    gaps = {2: walk(14, 31, center=(20, 20))[:, None], 5: walk(40, 32, closed=True, center=(60, 30)),
            9: walk(1, 33, center=(5, 6))[:, None], 6: walk(25, 34, center=(90, 90))[:, None]}
    return [('gaps', gaps, 5), ('one', {1: walk(11, 35, center=(15, 15))[:, None]}, 3), ('empty', {}, 5)]


def main():
    out = {'efd_cases': np.asarray([c[0] for c in efd_cases()]), 'c2f_cases': np.asarray([c[0] for c in c2f_cases()])}
    for name, contours, order, eps, autoclose in efd_cases():
        if isinstance(contours, list):
            arg = np.empty(len(contours), dtype=object)
            for i, c in enumerate(contours):
                arg[i] = c
            members, lead = contours, (-1,)
        else:
            arg, members, lead = contours, list(contours.reshape((-1,) + contours.shape[-2:])), contours.shape[:-2]
        coeff, loc = ref_cpn.efd(arg, order=order, epsilon=eps, autoclose=autoclose)
        ours = oracle.efd(contours, order, eps, autoclose)
        assert np.array_equal(ours[0], coeff, equal_nan=True) and np.array_equal(ours[1], loc, equal_nan=True), name
        out.update({f'efd.{name}.points': np.concatenate(members), f'efd.{name}.lengths': np.asarray([len(m) for m in members]),
                    f'efd.{name}.lead': np.asarray(lead, np.int64), f'efd.{name}.order': np.asarray(order),
                    f'efd.{name}.epsilon': np.asarray(eps), f'efd.{name}.autoclose': np.asarray(autoclose),
                    f'efd.{name}.coefficients': np.asarray(coeff, np.float64).reshape(-1, order, 4),
                    f'efd.{name}.locations': np.asarray(loc, np.float64).reshape(-1, 2)})
    for name, contours, order in c2f_cases():
        f64 = ref_cpn.contours2fourier(contours, order=order, dtype=np.float64)
        f32 = ref_cpn.contours2fourier(contours, order=order)
        assert f32[0].dtype == np.float32
        vals = list(contours.values())
        out.update({f'c2f.{name}.keys': np.asarray(list(contours.keys()), np.int64),
                    f'c2f.{name}.points': np.concatenate([v.reshape(-1, 2) for v in vals]) if vals else np.zeros((0, 2), np.int32),
                    f'c2f.{name}.lengths': np.asarray([len(v) for v in vals], np.int64),
                    f'c2f.{name}.squeeze': np.asarray([int(v.ndim == 3) for v in vals], np.int64),
                    f'c2f.{name}.order': np.asarray(order), f'c2f.{name}.fouriers': f64[0], f'c2f.{name}.locations': f64[1],
                    f'c2f.{name}.fouriers_f32': f32[0], f'c2f.{name}.locations_f32': f32[1]})
    for v in out.values():
        assert v.dtype.kind in 'iufbU'
    path = os.path.join(HERE, 'fourier.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(efd_cases()), 'efd cases')


if __name__ == '__main__':
    main()
