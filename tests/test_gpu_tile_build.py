"""The tiles' arrays as the set-up leaves them (skm_quant_setup.hip: tile sizes from the packing walk, two
placement kernels that drop the members into their tiles in any order, tile_build_kernel that orders every tile in
LDS) against the rule restated in numpy (tile_list_reference.py), through skm_quant_tile_arrays.  Every array is
compared exactly, as far as it belongs to a tile; the launch order is a permutation of the tiles by size bin (the
tiles of a bin stand in no fixed order).  On every table the tile EM equals the whole-table EM bit for bit and step
for step.  The tables are laid out from the library's own run length and capacities."""
import numpy as np
import pytest

import tile_list_reference as R
from test_gpu_em_components import _both, _em_inputs, _switch_off_by_default   # noqa: F401 (the fixture is autouse)
from test_gpu_em_tile_runs import _built_for

pytestmark = pytest.mark.gpu


def _tile_arrays(native, quant, n_tx, n_classes, n_pairs, n_tiles):
    """The arrays of skm_quant_tile_arrays, every entry the call does not write left at -1 (uint16: 0xffff)."""
    out = {'tile_tx': np.full(n_tiles + 1, -1, np.int64), 'tile_cls': np.full(n_tiles + 1, -1, np.int64),
           'tx_list': np.full(n_tx, -1, np.int32), 'cls_list': np.full(max(n_classes, 1), -1, np.int32),
           'tx_pair': np.full(n_tx + 1, -1, np.int64), 'cls_pair': np.full(n_classes + 1, -1, np.int64),
           'cls_tx': np.full(max(n_pairs, 1), 0xffff, np.uint16), 'tx_cls': np.full(max(n_pairs, 1), 0xffff, np.uint16),
           'order': np.full(max(n_tiles, 1), -1, np.int32), 'perm': np.full(max(n_classes, 1), -1, np.int32)}
    p64, p32 = native.c_i64p, native.c_i32p
    native.check(native.hip().skm_quant_tile_arrays(
        quant.handle, native.ptr(out['tile_tx'], p64), native.ptr(out['tile_cls'], p64), native.ptr(out['tx_list'], p32),
        native.ptr(out['cls_list'], p32), native.ptr(out['tx_pair'], p64), native.ptr(out['cls_pair'], p64),
        out['cls_tx'].ctypes.data, out['tx_cls'].ctypes.data, native.ptr(out['order'], p32), native.ptr(out['perm'], p32)))
    return out


def _defined(got, n_tiles, n_classes):
    """The part of every array that belongs to the tiles (skm_quant_tile_arrays says which)."""
    n_listed_tx, n_listed_cls = int(got['tile_tx'][n_tiles]), int(got['tile_cls'][n_tiles])
    pairs = int(got['cls_pair'][n_listed_cls])
    return {'tile_tx': got['tile_tx'], 'tile_cls': got['tile_cls'], 'tx_list': got['tx_list'][:n_listed_tx],
            'cls_list': got['cls_list'][:n_listed_cls], 'tx_pair': got['tx_pair'][:n_listed_tx + 1],
            'cls_pair': got['cls_pair'][:n_listed_cls + 1], 'cls_tx': got['cls_tx'][:pairs], 'tx_cls': got['tx_cls'][:pairs],
            'order': got['order'][:n_tiles], 'perm': got['perm'][:n_classes]}


def _check(native, quant, n_tx, offsets, targets):
    """Every array of the probe against the reference; returns (info, the device's arrays, the reference)."""
    info, _, tx_tile, class_tile = quant.components()
    assert info['built']
    ref = R.tile_lists(n_tx, offsets, targets, info['segment'], info['capacity'])
    assert info['tiles'] == ref['tiles'] and info['oversize'] == ref['oversize']
    n_classes, n_tiles = offsets.size - 1, info['tiles']
    got = _defined(_tile_arrays(native, quant, n_tx, n_classes, int(targets.size), n_tiles), n_tiles, n_classes)
    np.testing.assert_array_equal(tx_tile, ref['tx_tile'])
    np.testing.assert_array_equal(got['perm'], ref['perm'])
    np.testing.assert_array_equal(class_tile[ref['perm']], ref['cls_tile'])
    for name in ('tile_tx', 'tile_cls', 'tx_list', 'cls_list', 'tx_pair', 'cls_pair', 'cls_tx', 'tx_cls'):
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    np.testing.assert_array_equal(np.sort(got['order']), np.arange(n_tiles))
    assert (np.diff(R.order_bins(ref, info['capacity'])[got['order']]) >= 0).all()
    return info, got, ref


@pytest.mark.parametrize('name', sorted(R.TABLES))
def test_hand_made_tables(native_libs, name):
    from seekmer_amd import infer
    segment, capacity = _built_for(infer)
    n_tx, offsets, targets, counts = R.TABLES[name](segment, capacity)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, got, ref = _check(native_libs, quant, n_tx, offsets, targets.astype(np.int64))
        tile_of = ref['tx_tile']
        if name == 'capacity_exact':
            assert np.diff(got['tile_tx'])[tile_of[0]] == capacity[2]
            assert np.diff(got['tile_cls'])[tile_of[segment]] == capacity[1]
            assert np.diff(got['cls_pair'][got['tile_cls']])[tile_of[2 * segment]] == capacity[0]
        if name == 'capacity_one_more':
            for small, filler in ((0, 2), (segment, segment + 2), (2 * segment, 2 * segment + 5)):
                assert tile_of[small] + 1 == tile_of[filler]
        if name == 'oversize':
            assert info['oversize'] == 3 and info['tiles'] > 0 and info['em_uses_tiles']
            outside = np.nonzero(tile_of == n_tx)[0]
            assert outside.size and not np.isin(outside, got['tx_list']).any()
            assert not np.isin(np.nonzero(ref['cls_tile'] == n_tx)[0], got['cls_list']).any()
        if name == 'one_oversize_component':
            assert info['tiles'] == 0 and info['oversize'] == 1 and not info['em_uses_tiles']
            assert got['tile_tx'][0] == 0 and got['tile_cls'][0] == 0 and got['cls_pair'][0] == 0 and got['tx_pair'][0] == 0
        if name == 'odd_members':
            assert np.diff(got['tile_cls'])[-1] == 0 and np.diff(got['tile_tx'])[-1] == 3
            empty = np.nonzero(ref['length'] == 0)[0]
            first = got['cls_list'][got['tile_cls'][tile_of[0]]:got['tile_cls'][tile_of[0] + 1]]
            assert empty.size == 3 and np.isin(empty, first).all()
        if name == 'turn_caps':
            assert ref['degree'].max() > R.LONGEST * R.ROW_LANES and (ref['length'] > R.LONGEST * R.CLASS_BATCH).sum() == 2
        if name == 'scattered':
            assert n_tx % 256 and n_tx % 64 and info['tiles'] > 4
        x0, l = _em_inputs(n_tx, np.random.default_rng(5))
        _both(quant, x0, l)
        assert _both(quant, x0, l, fixed_iters=17)[1] == 17
    finally:
        quant.close()


def test_a_mapped_table_set_up_twice(native_libs):
    """The places the lanes draw differ from run to run; what the tiles' workgroups leave does not."""
    from seekmer_amd import common, index_builder, infer, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(7, 63)
    n_tx = len(ids)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 500 * 63
    bases, offsets = synth.reads(7, pool, tx_offsets, 0, n_units, 100, True)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
    class_offsets, class_targets, _, _, _ = result.export()
    class_offsets, class_targets = np.asarray(class_offsets, dtype=np.int64), np.asarray(class_targets, dtype=np.int64)
    seen = []
    for _ in range(2):
        quant = infer._QuantHandle.from_map_result(result, n_tx)
        try:
            info, got, ref = _check(native_libs, quant, n_tx, class_offsets, class_targets)
            assert info['em_uses_tiles'] and info['tiles'] > 1
            seen.append(got)
            if len(seen) == 2:
                x0, l = _em_inputs(n_tx, np.random.default_rng(7))
                _both(quant, x0, l)
        finally:
            quant.close()
    bins = R.order_bins(ref, info['capacity'])
    for name in seen[0]:
        if name == 'order':
            np.testing.assert_array_equal(bins[seen[0][name]], bins[seen[1][name]])
        else:
            np.testing.assert_array_equal(seen[0][name], seen[1][name], err_msg=name)
