"""The keyed table that instance evaluation and the region / shape properties share (csrc/label_table.h) at its edges on the
MI355X: the smallest legal tables, exactly full, and the repeatable status call.  With a capacity of at most 4096 slots the
probe limit is the capacity, so a full table must still take every key (the probe wraps around), and a lookup in it meets no
empty slot.  The images and what the numpy oracles make of them are in tests/test_tables.py."""
from ctypes import c_int64

import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib
from celldetection_amd._lib import check, ptr, stream_ptr
from test_gpu_instance_eval import check_against_table
from test_gpu_property_table import check as check_region
from test_gpu_shape_props import check as check_shape
from test_instance_eval import pair_table
from test_tables import four_key_images, label_image

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def test_label_matcher_table_of_four_slots_exactly_full():
    a, b = four_key_images()
    t = pair_table(a, b)
    m = cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV), table_capacity=4)
    assert m.stats['grown'] == 0 and m.stats['entries'] == 4 and m.stats['table_capacity'] == 4
    check_against_table(m, t, (None, .25, .5), 'capacity 4')
    m = cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV), table_capacity=2)
    assert m.stats['grown'] >= 1 and m.stats['entries'] == 4 and m.stats['table_capacity'] == 2 << m.stats['grown']
    check_against_table(m, t, (None, .25, .5), 'capacity 2')


@pytest.mark.parametrize('check_props', [check_region, check_shape], ids=['region_properties', 'shape_properties'])
def test_property_table_of_two_slots_exactly_full(check_props):
    _, st = check_props(label_image(2), what='two labels', table_capacity=2)  # shape: lookups in a table without an empty slot
    assert st['grown'] == 0 and st['rows'] == 2 and st['table_capacity'] == 2
    _, st = check_props(label_image(3), what='three labels', table_capacity=2)
    assert st['grown'] >= 1 and st['rows'] == 3 and st['table_capacity'] == 2 << st['grown']


def test_table_status_is_repeatable():
    lib = _lib.load()
    a, b = (torch.as_tensor(x).to(DEV)[:, :, None].contiguous() for x in four_key_images())
    cap = 16
    first, second = (c_int64 * 2)(), (c_int64 * 2)()
    with torch.cuda.device(DEV):
        nbytes = int(lib.cpn_eval_workspace_bytes(cap, 0, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        check(lib.cpn_eval_pairs(ptr(a), 1, ptr(b), 1, 64, cap, ptr(ws), nbytes, stream_ptr()), 'eval_pairs')
        check(lib.cpn_eval_table_status(ptr(ws), cap, first, stream_ptr()), 'eval_table_status')
        check(lib.cpn_eval_table_status(ptr(ws), cap, second, stream_ptr()), 'eval_table_status')
        assert list(first) == [0, 4] and list(second) == [0, 4]
        x = torch.as_tensor(label_image(3)).to(DEV)
        nbytes = int(lib.cpn_props_workspace_bytes(cap, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        check(lib.cpn_props_accumulate(ptr(x), 8, 8, 1, ptr(None), 0, 0, cap, ptr(ws), nbytes, stream_ptr()), 'props_accumulate')
        check(lib.cpn_props_table_status(ptr(ws), cap, first, stream_ptr()), 'props_table_status')
        check(lib.cpn_props_table_status(ptr(ws), cap, second, stream_ptr()), 'props_table_status')
        assert list(first) == [0, 3] and list(second) == [0, 3]
