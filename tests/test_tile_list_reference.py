"""The numpy restatement of the tiles' arrays (tile_list_reference.py) checked on its own, without a GPU, on the
tables test_gpu_tile_build.py lays out (here from the default run length and capacities): the tiles' starts in
transcripts, classes and pairs equal those tile_table of tile_pack_reference.py derives, every list is a
permutation of its tile's members in the order the rule states, and every pair of both views names the same
(class, transcript) incidence."""
import numpy as np
import pytest

import tile_list_reference as R
from tile_pack_reference import tile_table

SEGMENT, CAPACITY = 256, (2048, 512, 128)               # pairs, classes, transcripts


@pytest.mark.parametrize('name', sorted(R.TABLES))
def test_reference_agrees_with_the_packing_rule_and_lists_every_member_once(name):
    n_tx, offsets, targets, _ = R.TABLES[name](SEGMENT, CAPACITY)
    ref = R.tile_lists(n_tx, offsets, targets, SEGMENT, CAPACITY)
    # tile_table takes every class to hold a transcript: the classes without one are taken out for it and
    # counted back in from the tile of transcript 0 on
    filled = np.diff(offsets) > 0
    kept_offsets = np.concatenate([[0], np.cumsum(np.diff(offsets)[filled])])
    want_tile, want_tx, want_cls, want_pairs, want_oversize, _ = tile_table(n_tx, kept_offsets, targets.astype(np.int64),
                                                                            SEGMENT, CAPACITY)
    n_empty = int((~filled).sum())
    if n_empty and want_tile[0] < n_tx:
        want_cls = want_cls + n_empty * (np.arange(want_cls.size) > want_tile[0])
    np.testing.assert_array_equal(ref['tx_tile'], want_tile)
    assert ref['tiles'] == want_tx.size - 1 and ref['oversize'] == want_oversize
    np.testing.assert_array_equal(ref['tile_tx'], want_tx)
    np.testing.assert_array_equal(ref['tile_cls'], want_cls)
    np.testing.assert_array_equal(ref['cls_pair'][ref['tile_cls']], want_pairs)
    np.testing.assert_array_equal(ref['tx_pair'][ref['tile_tx']], want_pairs)
    tuples = [targets[offsets[c]:offsets[c + 1]] for c in ref['perm']]
    for tile in range(ref['tiles']):
        txs = ref['tx_list'][ref['tile_tx'][tile]:ref['tile_tx'][tile + 1]]
        classes = ref['cls_list'][ref['tile_cls'][tile]:ref['tile_cls'][tile + 1]]
        np.testing.assert_array_equal(np.sort(txs), np.nonzero(ref['tx_tile'] == tile)[0])
        np.testing.assert_array_equal(np.sort(classes), np.nonzero(ref['cls_tile'] == tile)[0])
        assert txs.size <= CAPACITY[2] and classes.size <= CAPACITY[1] and want_pairs[tile + 1] - want_pairs[tile] <= CAPACITY[0]
        # the order: turns descending with the cap, index ascending among equals
        for members, size, per in ((txs, ref['degree'], R.ROW_LANES), (classes, ref['length'], R.CLASS_BATCH)):
            turns = np.minimum(-(-size[members] // per), R.LONGEST)
            assert all((turns[i] > turns[i + 1]) or (turns[i] == turns[i + 1] and members[i] < members[i + 1])
                       for i in range(members.size - 1))
        # both views hold the same incidences
        by_class, by_tx = set(), set()
        for k, c in enumerate(classes):
            first = ref['cls_pair'][ref['tile_cls'][tile] + k]
            local = ref['cls_tx'][first:first + tuples[c].size]
            np.testing.assert_array_equal(txs[local], tuples[c])
            by_class |= {(int(c), int(t)) for t in tuples[c]}
        for i, t in enumerate(txs):
            first = ref['tx_pair'][ref['tile_tx'][tile] + i]
            local = ref['tx_cls'][first:first + ref['degree'][t]]
            assert (np.diff(classes[local]) > 0).all()
            by_tx |= {(int(c), int(t)) for c in classes[local]}
        assert by_class == by_tx
    bins = R.order_bins(ref, CAPACITY)
    assert bins.size == ref['tiles'] and ((bins >= 0) & (bins < 256)).all()


def test_the_tables_hold_what_their_names_say():
    tables = {name: R.tile_lists(make(SEGMENT, CAPACITY)[0], *make(SEGMENT, CAPACITY)[1:3], SEGMENT, CAPACITY)
              for name, make in R.TABLES.items()}
    cap_pairs, cap_classes, cap_tx = CAPACITY
    exact, more = tables['capacity_exact'], tables['capacity_one_more']
    # (the transcripts that no class names are components of one: they fill further tiles of every run)
    assert exact['oversize'] == more['oversize'] == 0
    tile_of = exact['tx_tile']
    assert np.diff(exact['tile_tx'])[tile_of[0]] == cap_tx and np.diff(exact['tile_cls'])[tile_of[SEGMENT]] == cap_classes
    assert np.diff(exact['cls_pair'][exact['tile_cls']])[tile_of[2 * SEGMENT]] == cap_pairs
    for small, filler in ((0, 2), (SEGMENT, SEGMENT + 2), (2 * SEGMENT, 2 * SEGMENT + 5)):
        assert exact['tx_tile'][small] == exact['tx_tile'][filler] and more['tx_tile'][small] + 1 == more['tx_tile'][filler]
    assert tables['oversize']['oversize'] == 3 and tables['oversize']['tiles'] >= 3
    assert tables['one_oversize_component']['tiles'] == 0 and tables['one_oversize_component']['oversize'] == 1
    assert tables['single_transcript']['tiles'] == 1
    odd = tables['odd_members']
    assert odd['tiles'] == 3 and np.diff(odd['tile_cls'])[2] == 0 and np.diff(odd['tile_tx'])[2] == 3
    assert (odd['length'] == 0).sum() == 3 and (odd['cls_tile'][odd['length'] == 0] == odd['tx_tile'][0]).all()
    caps = tables['turn_caps']
    assert caps['degree'].max() > R.LONGEST * R.ROW_LANES and (caps['length'] > R.LONGEST * R.CLASS_BATCH).sum() == 2
    scattered = tables['scattered']
    assert scattered['tiles'] > 4 and scattered['oversize'] == 0
    first_tile = scattered['tx_list'][:scattered['tile_tx'][1]]
    assert first_tile.min() == 0 and first_tile.max() >= scattered['tx_tile'].size - 64      # run 0 to the last ids
