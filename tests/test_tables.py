"""The host side of the keyed device tables (celldetection_amd/_tables.py) and of the label-image inputs
(celldetection_amd/_label_input.py), without the library; and the tiny images of tests/test_gpu_label_table.py, whose
expected values the numpy oracles of this folder must give before the GPU tests rely on them."""
import gc
import weakref

import numpy as np
import pytest
import torch

from celldetection_amd import _label_input, _tables
from property_table_oracle import property_table
from shape_props_oracle import shape_table
from test_instance_eval import pair_table


# ---- capacities and the growth loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('pixels,per_slot,cap', [(0, 16, 4096), (65536, 16, 4096), (65537, 16, 4096), (65552, 16, 8192),
                                                 (2 ** 40, 64, 2 ** 21)])
def test_default_capacity(pixels, per_slot, cap):
    assert _tables.default_capacity(pixels, per_slot) == cap


def test_check_capacity():
    assert _tables.check_capacity(2) is None
    for cap in (0, 1, 3, 100):
        with pytest.raises(ValueError) as e:
            _tables.check_capacity(cap)
        assert str(e.value) == 'table_capacity must be a power of two'


class Workspace:
    pass


def test_grow_until_it_fits_doubles_and_holds_one_workspace():
    alive, caps = [], []

    def attempt(cap):
        gc.collect()
        assert [r for r in alive if r() is not None] == [], 'the workspace of the failed attempt is still held'
        caps.append(cap)
        ws = Workspace()
        alive.append(weakref.ref(ws))
        return ws, max(0, 3 - len(caps)), 10 * cap  # overflows twice

    ws, cap, grown, entries = _tables.grow_until_it_fits(8, attempt)
    assert caps == [8, 16, 32] and cap == 32 and grown == 2 and entries == 320
    assert ws is alive[-1]() and [r() for r in alive[:-1]] == [None, None]


def test_grow_until_it_fits_first_attempt():
    ws, cap, grown, entries = _tables.grow_until_it_fits(4, lambda cap: ('ws', 0, 3))
    assert (ws, cap, grown, entries) == ('ws', 4, 0, 3)


# ---- label-image inputs -----------------------------------------------------------------------------------------------------
def test_to_int32_raises_with_exactly_the_message_passed():
    for bad in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(ValueError) as e:
            _label_input.to_int32(torch.tensor([[0, bad]], dtype=torch.int64), 'someone: something does not fit')
        assert str(e.value) == 'someone: something does not fit'
    x = torch.tensor([[-2 ** 31, 2 ** 31 - 1]], dtype=torch.int64).t()  # the limits fit; the result is contiguous int32
    y = _label_input.to_int32(x, 'unused')
    assert y.dtype == torch.int32 and y.is_contiguous() and y.tolist() == x.tolist()
    assert _label_input.to_int32(torch.ones(3, dtype=torch.bool), 'unused').tolist() == [1, 1, 1]
    assert (_label_input.INT32_MIN, _label_input.INT32_MAX) == (-2 ** 31, 2 ** 31 - 1)


def test_aligned16():
    base = torch.zeros(16, dtype=torch.int32)
    assert base.data_ptr() % 16 == 0 and _label_input.aligned16(base) is base
    off = base[1:]
    got = _label_input.aligned16(off)
    assert got.data_ptr() % 16 == 0 and got is not off and torch.equal(got, off)


def test_upload_numpy_checks_the_range_before_it_needs_a_device():
    with pytest.raises(ValueError) as e:
        _label_input.upload_numpy(np.array([[2 ** 31]], np.uint32), 'LabelMatcher', 'inputs holds labels')
    assert str(e.value) == 'LabelMatcher: inputs holds labels that do not fit int32'


def test_check_labels_messages():
    with pytest.raises(TypeError, match=r'^op: labels must be a Tensor on the GPU \(got ndarray\)$'):
        _label_input.check_labels(np.zeros((2, 2, 1), np.int32), 'op')
    with pytest.raises(ValueError, match=r'^op: labels must be \[H, W\] or \[H, W, C\] \(got \(2,\)\)$'):
        _label_input.check_labels(torch.zeros(2, dtype=torch.int32), 'op', ranks=(2, 3))
    with pytest.raises(TypeError, match=r'^op: labels must hold integers \(got torch.bool\)$'):
        _label_input.check_labels(torch.zeros((2, 2, 1), dtype=torch.bool), 'op')
    with pytest.raises(RuntimeError, match=r'^celldetection_amd.op runs on the MI355X only \(got a CPU tensor\).$'):
        _label_input.check_labels(torch.zeros((2, 2, 1), dtype=torch.int32), 'op')


# ---- the images of the smallest tables --------------------------------------------------------------------------------------
def four_key_images():
    """8 x 8 inputs / targets with exactly four table keys: input labels 1 and 2, target label 1, and the pair (1, 1)."""
    a, b = np.zeros((8, 8), np.int32), np.zeros((8, 8), np.int32)
    a[0:3, 0:3], a[5:8, 4:8] = 1, 2
    b[1:4, 1:4] = 1  # overlaps input 1 in 2 x 2 pixels and input 2 nowhere
    return a, b


def label_image(labels):
    """8 x 8 x 1 with 2 or 3 objects: a 3 x 3 square, a 2 x 4 rectangle and a single pixel."""
    a = np.zeros((8, 8, 1), np.int32)
    a[0:3, 0:3, 0], a[5:7, 3:7, 0] = 1, 2
    if labels == 3:
        a[7, 0, 0] = 3
    return a


def test_oracle_on_the_four_key_images():
    t = pair_table(*four_key_images())
    assert t['matches'].tolist() == [[1, 1]] and t['intersections'].tolist() == [4] and t['unions'].tolist() == [14]
    assert t['input_counts'] == {1: 9, 2: 12} and t['target_counts'] == {1: 9}
    assert len(t['input_counts']) + len(t['target_counts']) + len(t['matches']) == 4


def test_oracles_on_the_label_images():
    for n in (2, 3):
        cols, channel, _ = property_table(label_image(n), ('label', 'num_pixels', 'bbox'))
        assert cols['label'].tolist() == [1, 2, 3][:n] and channel.tolist() == [0] * n
        assert cols['num_pixels'].tolist() == [9, 8, 1][:n]
        assert [cols[f'bbox-{i}'].tolist() for i in range(4)] == [[0, 5, 7][:n], [0, 3, 0][:n], [3, 7, 8][:n], [3, 7, 1][:n]]
        cols, channel = shape_table(label_image(n), ('label', 'perimeter', 'euler_number', 'area_convex', 'solidity'))
        assert cols['label'].tolist() == [1, 2, 3][:n] and len(channel) == n
        assert cols['euler_number'].tolist() == [1] * n and cols['area_convex'].tolist() == [9., 8., 1.][:n]
        assert cols['solidity'].tolist() == [1.] * n and cols['perimeter'][0] == 8.  # the 8 border pixels of the square
