"""A class table whose classes name a transcript more than once, and the transcript-major view of such a table
stated the way the whole-table set-up makes it: ONE stable sort of all pairs by transcript, the pairs taken in
class-major order of the internal classes.  tile_list_reference.py builds the same view class by class
(rows[tx].append(k) for every entry of every tuple); the tile set-up of skm_quant_setup.hip builds it per tile with a
counting sort in LDS.  test_repeated_members_reference.py holds the two restatements against each other, the GPU
tests (test_gpu_rows_on_demand.py) the device against tile_list_reference.py."""
import numpy as np

import tile_list_reference as R

ROW_CAP = 512                 # EM_ROW_CAP of skm_kernels.h: pairs of one row of the whole-table EM


def repeated_member_table(seed=43):
    """260 classes that name transcript 0 twice -- at every pair of tuple positions -- and one of 100 other
    transcripts, and a class that names transcript 7 three times: one component of 101 transcripts, 261 classes
    and 783 pairs, within one tile; transcript 0 has 520 pairs, more than a row of the whole-table EM holds."""
    classes = []
    for i in range(260):
        other = 1 + i % 100
        classes.append([[0, 0, other], [0, other, 0], [other, 0, 0]][i % 3])
    classes.append([7, 7, 7])
    n_tx, offsets, targets, counts = R._finish(classes, 101, seed)
    assert np.bincount(targets)[0] == 520 > ROW_CAP and targets.size == 783
    return n_tx, offsets, targets, counts


def transposed_by_stable_sort(n_tx, offsets, targets):
    """(tx_offset [n_tx + 1], tx_cls [pairs]): internal class index of every pair, transcript-major, as a stable
    sort of the class-major pairs by transcript leaves them."""
    offsets, targets = np.asarray(offsets, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    perm = R.internal_order(offsets, targets)
    pair_tx = np.concatenate([targets[offsets[c]:offsets[c + 1]] for c in perm] + [np.zeros(0, dtype=np.int64)])
    pair_cls = np.repeat(np.arange(perm.size), np.diff(offsets)[perm])
    order = np.argsort(pair_tx, kind='stable')
    tx_offset = np.concatenate([[0], np.cumsum(np.bincount(pair_tx, minlength=n_tx))]).astype(np.int64)
    return tx_offset, pair_cls[order]
