"""Golden-vector generator of the region property tables (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and runs its own ``labels2property_table``
(celldetection/data/misc.py:320-347) on small label images; writes ``property_table.npz`` next to this file: per case the
label image, the call (property names, call form, separator, spacing, intensity image, ``df_kwargs`` as name lists and small
arrays) and the resulting table: column names, index and values.  Arrays and name lists only.

WHAT THIS PINS AND WHAT IT DOES NOT.  The reference calls ``skimage.measure.regionprops_table`` for every channel; scikit-image
is absent here, so ``tests/property_table_oracle.regionprops_table`` -- written from scikit-image's documentation -- is put onto
the stub ``skimage.measure`` module at run time.  The PROPERTY ARITHMETIC in this fixture is therefore that restatement's, not
scikit-image's: third-party, restated and unpinned.  What the fixture pins to the reference's own code is the wrapper: the
single-list call form, the channel loop, what is handed to ``regionprops_table`` and ``pandas.DataFrame`` (``df_kwargs``), the
concatenation and the resulting index, which restarts at 0 in every channel.  pandas is the real package.

Run:  python tests/golden/make_golden_property_table.py
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
import celldetection.data.misc as ref_misc  # noqa: E402
from property_table_oracle import ALL_GEOMETRY, regionprops_table  # noqa: E402
from test_instance_eval import disc_labels  # noqa: E402  (the synthetic images are the tests' own, not the reference's)

ref_misc.measure.regionprops_table = regionprops_table
labels2property_table = ref_misc.labels2property_table


def cases():
    """name -> (labels, properties, list_form, kwargs)."""
    out = {}
    a = disc_labels(48, 60, 14, 1, seed=5)[:, :, 0]
    a[a == 3] = 65537  # labels need not be 1 .. N
    out['image_2d'] = (a, ALL_GEOMETRY, False, {})
    b = disc_labels(40, 52, 16, 3, seed=7, rmax=9.)
    b[2:5, 3:9, 2] = int(b[:, :, 0].max())  # the largest label of channel 0 once more in channel 2
    b[30:32, 1:3, 1] = -4  # not an object
    assert (b[:, :, 1] > 0).any() and (b[:, :, 2] > 0).sum() > 18
    out['channels_repeated_label'] = (b, ('label', 'bbox', 'area', 'centroid', 'orientation', 'inertia_tensor'), False, {})
    out['list_form'] = (b, ['label', 'num_pixels', 'local_centroid', 'major_axis_length', 'bbox_area'], True, {})
    out['df_kwargs'] = (b, ('label', 'area', 'eccentricity'), False, dict(df_kwargs=dict(dtype=np.float64)))
    img = (np.random.default_rng(3).integers(0, 255, (40, 52, 2))).astype(np.uint8)
    out['separator_spacing_intensity'] = (b, ('label', 'centroid', 'inertia_tensor_eigvals', 'equivalent_diameter_area',
                                              'intensity_mean', 'max_intensity', 'intensity_min', 'extent'), False,
                                          dict(separator='_', spacing=(0.5, 2.0), intensity_image=img))
    e = np.zeros((9, 7, 2), np.int32)  # a channel without objects in between: the index restarts, nothing else happens
    e[1:4, 2:6, 1] = 9
    out['empty_channel'] = (e, ('label', 'bbox'), False, {})
    return out


def main():
    out = dict(cases=np.asarray(list(cases())))
    for name, (a, props, list_form, kw) in cases().items():
        tab = labels2property_table(a, list(props), **kw) if list_form else labels2property_table(a, *props, **kw)
        out[f'{name}.labels'] = a
        out[f'{name}.properties'] = np.asarray(list(props))
        out[f'{name}.list_form'] = np.asarray(int(list_form), np.int64)
        out[f'{name}.separator'] = np.asarray(kw.get('separator', '-'))
        out[f'{name}.spacing'] = np.asarray(kw.get('spacing', ()), np.float64)
        out[f'{name}.intensity_image'] = kw.get('intensity_image', np.zeros((0,), np.uint8))
        out[f'{name}.df_dtype'] = np.asarray(np.dtype(kw['df_kwargs']['dtype']).name if 'df_kwargs' in kw else '')
        out[f'{name}.columns'] = np.asarray([str(c) for c in tab.columns])
        out[f'{name}.index'] = np.asarray(tab.index, np.int64)
        for c in tab.columns:
            v = tab[c].to_numpy()
            assert v.dtype.kind in 'iuf', (name, c, v.dtype)
            out[f'{name}.col.{c}'] = v
        print(f'{name}: {a.shape}, {len(tab)} rows, columns {list(tab.columns)}, index {list(tab.index)[:12]} ...')
    path = os.path.join(HERE, 'property_table.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
