"""The packing rule of the tile EM stated twice on the CPU -- tests/tile_pack_reference.py, which the GPU
tests compare the device's tiles with, and scripts/em_tile_lane_model.py, which the tile counts in
DESIGN.md come from -- on one small class table: both must give the same tiles."""
import os
import sys

import numpy as np

from tile_pack_reference import component_sizes, labels, pack, tile_table

SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts')


def _table(seed=9, n_tx=700):
    """Components of 1-6 transcripts in 5-60 classes, one transcript in 3000 classes of its own."""
    rng = np.random.default_rng(seed)
    classes, t = [], 0
    while t < n_tx - 1:
        n = min(int(rng.integers(1, 7)), n_tx - 1 - t)
        members = np.arange(t, t + n)
        classes += [[v, v + 1] for v in range(t, t + n - 1)] or [[t]]
        classes += [list(rng.permutation(members)[:int(rng.integers(1, n + 1))]) for _ in range(int(rng.integers(5, 61)))]
        t += n
    classes += [[n_tx - 1]] * 3000
    order = rng.permutation(len(classes))
    classes = [classes[i] for i in order]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int64)
    return n_tx, offsets, np.concatenate([np.asarray(c, dtype=np.int64) for c in classes])


def test_restatement_equals_the_lane_model():
    sys.path.insert(0, SCRIPTS)
    try:
        import em_tile_lane_model as model
    finally:
        sys.path.remove(SCRIPTS)
    k = model.constants()
    n_tx, offsets, targets = _table()
    capacity = (k['EM_TILE_PAIRS'], k['EM_TILE_CLASSES'], k['EM_TILE_TX'])
    tx_tile, tx_start, _, _, oversize, cuts = tile_table(n_tx, offsets, targets, k['EM_TILE_SEGMENT'], capacity)
    model_tile, model_tiles = model.pack_tiles(n_tx, offsets, targets, k)
    assert model_tiles == tx_start.size - 1 and model_tiles > -(-n_tx // k['EM_TILE_SEGMENT'])
    np.testing.assert_array_equal(np.where(model_tile >= 0, model_tile, n_tx), tx_tile)
    assert oversize == 1 and tx_tile[n_tx - 1] == n_tx and cuts


def test_rule_by_hand():
    """Capacity (10 pairs, 4 classes, 3 transcripts), runs of 4 ids, ten transcripts."""
    c_tx = np.array([1, 1, 2, 0, 1, 1, 1, 4, 0, 1])
    c_pairs = np.array([6, 5, 1, 0, 1, 1, 1, 1, 0, 11])
    c_classes = np.array([1, 1, 1, 0, 3, 2, 1, 1, 0, 1])
    root_tile, n_tiles, cuts = pack((c_tx, c_pairs, c_classes), 4, (10, 4, 3))
    # run 0: [0] | [1, 2] (pairs 6 + 5 > 10); run 1: [4] | [5, 6] (classes 3 + 2 > 4), 7 above the capacity in
    # transcripts; run 2: 9 above the capacity in pairs: no tile
    np.testing.assert_array_equal(root_tile, [0, 1, 1, -1, 2, 3, 3, -2, -1, -2])
    assert n_tiles == 4 and cuts == [(0, 1, {'pairs'}), (1, 3, {'classes'})]
    label = labels(4, [0, 2, 3], [0, 2, 3])
    np.testing.assert_array_equal(label, [0, 1, 0, 3])
    np.testing.assert_array_equal(component_sizes(4, [0, 2, 3], [0, 2, 3], label), [[2, 1, 0, 1], [2, 0, 0, 1], [1, 0, 0, 1]])
