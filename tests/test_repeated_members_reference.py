"""tile_list_reference.py on tables whose classes name a transcript more than once, against the stable sort of the
whole table's pairs (repeated_members_reference.py): the GPU tests of the tile set-up lean on the former."""
import numpy as np
import pytest

import repeated_members_reference as M
import tile_list_reference as R

SEGMENT, CAPACITY = 256, (2048, 512, 128)


def _views_agree(n_tx, offsets, targets):
    ref = R.tile_lists(n_tx, offsets, targets, SEGMENT, CAPACITY)
    tx_offset, tx_cls = M.transposed_by_stable_sort(n_tx, offsets, targets)
    np.testing.assert_array_equal(np.diff(tx_offset), ref['degree'])
    assert ref['tiles'] > 0
    for tile in range(ref['tiles']):
        classes = ref['cls_list'][ref['tile_cls'][tile]:ref['tile_cls'][tile + 1]]
        name = {int(c): k for k, c in enumerate(classes)}
        for place in range(ref['tile_tx'][tile], ref['tile_tx'][tile + 1]):
            t = ref['tx_list'][place]
            row = ref['tx_cls'][ref['tx_pair'][place]:ref['tx_pair'][place + 1]]
            whole = tx_cls[tx_offset[t]:tx_offset[t + 1]]
            assert row.size == ref['degree'][t]
            np.testing.assert_array_equal(row, [name[int(c)] for c in whole])
    return ref


def test_repeated_member_table():
    n_tx, offsets, targets, _ = M.repeated_member_table()
    ref = _views_agree(n_tx, offsets, targets)
    assert ref['tiles'] == 1 and ref['oversize'] == 0
    assert ref['degree'][0] == 520 and ref['degree'][7] == 3 + 3          # (three times in one class, once in three)
    # a class that names a transcript twice stands twice in its row, side by side
    row0 = ref['tx_cls'][ref['tx_pair'][list(ref['tx_list']).index(0)]:][:520]
    assert (row0[0::2] == row0[1::2]).all() and np.unique(row0).size == 260
    # ... and the transcript stands twice in the class's tuple of the class-major view
    assert ref['cls_tx'].size == 783 and np.bincount(ref['cls_tx']).max() == 520


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_tables_with_repeats(seed):
    rng = np.random.default_rng(seed)
    classes = []
    for first in range(0, 600, 6):                       # components of six ids, members drawn WITH replacement
        for _ in range(int(rng.integers(1, 9))):
            classes.append([int(t) for t in first + rng.integers(0, 6, int(rng.integers(1, 7)))])
    n_tx, offsets, targets, _ = R._finish(classes, 600, seed)
    assert (np.diff(offsets) > np.array([np.unique(targets[a:b]).size for a, b in zip(offsets[:-1], offsets[1:])])).any()
    _views_agree(n_tx, offsets, targets)
