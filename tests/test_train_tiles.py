"""The weight-gradient case table of tests/train_tiles.py against the built library and the headers, without a GPU.

* the library accepts exactly the table's (route, k) pairs through its info entry points and rejects every other k in 1 ... 9;
* the constants the edges are computed from are the ones csrc/wgrad_dense.h and csrc/wgrad_slabs.h state (read as text);
* for every instantiation the union of the edges its entries show, over their slab_rows values, is every edge but the written
  exemptions, and every exemption is used;
* the partition the library reports for every (entry, slab_rows) is the one the edge computation assumes, and the chain the bound
  is taken from obeys the limit the existing weight-gradient tests hold it to;
* the entries the exact test leaves out are exactly the resized ones whose blend weights are not dyadic, each with its reason.
"""
import os
import re

import pytest

import train_tiles as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANTIATIONS = sorted({tt.instantiation(key) for key in tt.TABLE})


def _text(name):
    return open(os.path.join(ROOT, 'celldetection_amd', 'csrc', name)).read()


def test_library_accepts_exactly_the_tables_filter_sizes():
    """A k added to a route's switch without an entry, or an entry for a k the route rejects, fails."""
    accepted = {route: tt.accepted_ks(route) for route in tt.ROUTES}
    assert accepted == tt.KS, accepted
    assert sum(len(ks) for ks in accepted.values()) == 11
    with_entries = {tt.instantiation(key) for key in tt.TABLE}
    assert with_entries == {f'{route}/k{k}' for route, ks in accepted.items() for k in ks}
    for key in tt.TABLE:
        route, k, name = tt.parse_key(key)
        assert route in tt.ROUTES and k in accepted[route] and name, key


def test_constants_are_the_headers():
    dense, slabs = _text('wgrad_dense.h'), _text('wgrad_slabs.h')
    assert int(re.search(r'constexpr int CT_CH = (\d+);', dense).group(1)) == tt.CT_CH == 128
    assert 'static constexpr int CH = CT_CH, FR = MT, DYB = 2 * MT, XB = 2;' in dense  # ... which is the dense grid's chunk
    assert int(re.search(r'constexpr int WGS_STEP = (\d+);', slabs).group(1)) == tt.WGS_STEP == 16
    body = re.search(r'constexpr int ct_mt\(int k\) \{ return (.*?); \}', dense).group(1)
    assert body == 'k <= 3 ? 2 : 1', body
    assert [tt.mt(k) for k in (1, 3, 5, 7)] == [2, 2, 1, 1]
    # the tile extents and the split of blockIdx.y the edges 'grid', 'co_part' and 'ci_part' speak of: the dense Tiling (CtGrid)
    assert 'co0 = (int) (by / tiles_ci) * 64 * MT, ci0 = (int) (by % tiles_ci) * 64;' in dense
    assert 'tiling.tile(blockIdx.y, wave, lane)' in dense and 'class Tiling = CtGrid<MT>>' in dense
    assert 'return (cout + 64 * ct_mt(k) - 1) / (64 * ct_mt(k));' in dense and 'tci = (cin + 63) / 64;' in dense
    assert 'constexpr int PAD = K / 2, CH = Tiling::CH, FR = Tiling::FR;' in dense
    assert 'const int steps = left >= CH ? CH / WGS_STEP : wgs_steps(left);' in dense


@pytest.mark.parametrize('inst', INSTANTIATIONS)
def test_every_instantiation_shows_every_edge_but_its_exemptions(inst):
    shown = set()
    entries = [key for key in tt.TABLE if tt.instantiation(key) == inst]
    assert f'{inst}/tiles' in entries and f'{inst}/exact' in entries
    for key in entries:
        for slab_rows in tt.TABLE[key]['slab_rows']:
            e = tt.edges(key, slab_rows, tt.info(key, slab_rows))
            assert set(e) == set(tt.EDGES)
            shown |= {name for name, ok in e.items() if ok}
    missing = set(tt.EDGES) - shown
    assert missing == tt.exempt(inst), f'{inst}: edges not shown {sorted(missing)}, written exemptions {sorted(tt.exempt(inst))}'
    # the tiles entry alone shows the whole launch grid: both tile counts above one and unequal, both last tiles partial
    e = tt.edges(f'{inst}/tiles', 8, tt.info(f'{inst}/tiles', 8))
    assert e['grid'] and e['grid_skew'] and e['co_part'] and e['ci_part'] and e['chunks3'] and e['image_in_chunk'] and e['n3'] and e['last_slab']
    assert tt.tiles(f'{inst}/tiles') == (2, 3)
    assert all(tt.edges(f'{inst}/exact', sr, tt.info(f'{inst}/exact', sr))['chunk_exact'] for sr in (4, 8))


def test_every_exemption_is_used():
    for pattern, names, reason in tt.EXEMPT:
        assert reason and any(re.match(pattern, inst) for inst in INSTANTIATIONS), pattern
    for pattern, reason in tt.INEXACT:
        assert reason and any(re.match(pattern, key) for key in tt.TABLE), pattern


@pytest.mark.parametrize('case', tt.cases(), ids=tt.case_id)
def test_reported_partition_is_the_one_the_edges_assume(case):
    key, slab_rows = case
    cfg = tt.TABLE[key]
    rows, w = cfg['n'] * cfg['h'], cfg['w']
    info = tt.info(key, slab_rows)
    assert 1 <= info['slab_rows'] <= rows
    assert (info['slab_rows'], info['slabs'], info['steps']) == tt.partition(rows, w, slab_rows, info['slab_rows']), info
    assert info['reduce_chain'] == info['slabs']
    pixels = tt.slab_pixels(cfg, info)
    assert sum(c for _, c in pixels) == rows * w and all(c > 0 for _, c in pixels)
    assert [p for p, _ in pixels] == [sum(c for _, c in pixels[:s]) for s in range(len(pixels))]
    assert info['steps'] == max(-(-c // tt.WGS_STEP) for _, c in pixels)
    # the library cannot widen its own bound
    assert info['steps'] + 2 + info['reduce_chain'] <= -(-rows * w // 16) + 2 + info['slabs'], info


def test_exact_test_leaves_out_exactly_the_entries_without_dyadic_weights():
    for key in tt.TABLE:
        assert tt.dyadic(key) == (tt.inexact(key) is None), key
    for inst in INSTANTIATIONS:  # the tiles and the exact geometry stay in the exact test on all three routes
        assert tt.dyadic(f'{inst}/tiles') and tt.dyadic(f'{inst}/exact')


def test_locate_names_tile_fragment_and_tap():
    assert tt.locate('dense/k3/tiles', (159, 159, 2, 0)) == \
        'dense/k3/tiles <3,2,CtDense>: worst element (159, 159, 2, 0) in co tile 1 of 2 (the partial last tile) fragment 0, ' \
        'ci tile 2 of 3 (the partial last tile) block 0, tap (2, 0)'
    assert tt.locate('concat/k7/tiles', (70, 40, 0, 6)) == \
        'concat/k7/tiles <7,1,CcSources>: worst element (70, 40, 0, 6) in co tile 1 of 2 (the partial last tile) fragment 0, ' \
        'ci tile 0 of 3 block 1 (top), tap (0, 6)'
    assert tt.locate('resized/k5/exact', (3, 31, 4, 4)).startswith('resized/k5/exact <5,1,BlSource>: worst element (3, 31, 4, 4) in co tile 0 of 1 ')
