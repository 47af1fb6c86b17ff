"""What the tile EM's set-up must leave in the tiles' arrays (skm_quant_setup.hip: the two placement kernels and
tile_build_kernel; EmTiles in skm_kernels.h), restated in numpy: the tiles of tile_pack_reference.py, and inside a
tile
  the transcripts by min(ceil(degree / 8), 31) descending, then id ascending,
  the classes by min(ceil(length / 4), 31) descending, then internal index ascending
(8: the lanes the chunk kernel's row phase gives a transcript; 4: the tuple entries a lane of its class phase
fetches together), internal = the classes in stable order of their smallest transcript id, one without
transcripts last.  A tile's pairs follow each other in both views: class-major in tuple order, transcript-major in
ascending internal class index (the order of the global transposed view), each entry renamed to the place of the
transcript / class in the tile's list.  Also the hand-made tables the tests of both kinds lay out from a run length
and the three capacities."""
import numpy as np

from tile_pack_reference import labels, pack

ROW_LANES, CLASS_BATCH, LONGEST = 8, 4, 31


def internal_order(offsets, targets):
    """perm[k] = the caller's index of internal class k."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    key = np.full(lens.size, 2 ** 32 - 1, dtype=np.int64)
    for c in np.nonzero(lens)[0]:
        key[c] = np.min(targets[offsets[c]:offsets[c + 1]])
    return np.argsort(key, kind='stable')


def sizes_with_empty_classes(n_tx, offsets, targets, label):
    """component_sizes of tile_pack_reference.py, a class without transcripts counted with transcript 0's component."""
    offsets, targets = np.asarray(offsets, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    filled = np.diff(offsets) > 0
    first = np.zeros(offsets.size - 1, dtype=np.int64)
    first[filled] = targets[offsets[:-1][filled]]
    return (np.bincount(label, minlength=n_tx), np.bincount(label[targets], minlength=n_tx),
            np.bincount(label[first], minlength=n_tx))


def _turns_key(size, per):
    return LONGEST - np.minimum(-(-size // per), LONGEST)


def tile_lists(n_tx, offsets, targets, segment, capacity, class_order=True):
    """The arrays of skm_quant_tile_arrays as far as they are defined (see there), as a dict, with 'tiles',
    'oversize', 'tx_tile' [n_tx] and 'cls_tile' [classes, internal order] (n_tx: in no tile)."""
    offsets, targets = np.asarray(offsets, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    n_classes = offsets.size - 1
    label = labels(n_tx, offsets, targets)
    root_tile, n_tiles, _ = pack(sizes_with_empty_classes(n_tx, offsets, targets, label), segment, capacity)
    tx_tile = np.where(root_tile[label] >= 0, root_tile[label], n_tx)
    perm = internal_order(offsets, targets)
    tuples = [targets[offsets[c]:offsets[c + 1]] for c in perm]               # internal order from here on
    length = np.array([t.size for t in tuples], dtype=np.int64)
    cls_tile = np.array([tx_tile[t[0] if t.size else 0] for t in tuples], dtype=np.int64).reshape(n_classes)
    degree = np.bincount(targets, minlength=n_tx) if targets.size else np.zeros(n_tx, dtype=np.int64)
    rows = [[] for _ in range(n_tx)]                                          # ascending internal class index
    for k, t in enumerate(tuples):
        for tx in t:
            rows[tx].append(k)
    tx_key, cls_key = _turns_key(degree, ROW_LANES), _turns_key(length, CLASS_BATCH)
    if not class_order:
        cls_key = np.zeros_like(cls_key)
    out = {k: [] for k in ('tx_list', 'cls_list', 'tx_pair', 'cls_pair', 'cls_tx', 'tx_cls')}
    tile_tx, tile_cls, pairs = [0], [0], 0
    for tile in range(n_tiles):
        txs = np.nonzero(tx_tile == tile)[0]
        txs = txs[np.lexsort((txs, tx_key[txs]))]
        classes = np.nonzero(cls_tile == tile)[0]
        classes = classes[np.lexsort((classes, cls_key[classes]))]
        tx_local = {int(t): i for i, t in enumerate(txs)}
        cls_local = {int(c): i for i, c in enumerate(classes)}
        at = pairs
        for t in txs:
            out['tx_pair'].append(at)
            out['tx_cls'] += [cls_local[c] for c in rows[t]]
            at += degree[t]
        at = pairs
        for c in classes:
            out['cls_pair'].append(at)
            out['cls_tx'] += [tx_local[int(t)] for t in tuples[c]]
            at += length[c]
        assert at - pairs == degree[txs].sum()
        pairs = at
        out['tx_list'] += list(txs)
        out['cls_list'] += list(classes)
        tile_tx.append(len(out['tx_list']))
        tile_cls.append(len(out['cls_list']))
    out['tx_pair'].append(pairs)
    out['cls_pair'].append(pairs)
    out = {k: np.array(v, dtype=np.int64) for k, v in out.items()}
    out.update(tile_tx=np.array(tile_tx, dtype=np.int64), tile_cls=np.array(tile_cls, dtype=np.int64), perm=perm,
               tiles=n_tiles, oversize=int((root_tile == -2).sum()), tx_tile=tx_tile, cls_tile=cls_tile,
               degree=degree, length=length)
    return out


def order_bins(ref, capacity, bins=256):
    """Size bin of every tile as tile_order_kernel forms it (bin 0: the fullest tiles)."""
    pairs = np.diff(ref['cls_pair'][ref['tile_cls']])
    return bins - 1 - np.minimum(np.maximum(pairs, 0), capacity[0]) * (bins - 1) // capacity[0]


# ---- the tables -------------------------------------------------------------------------------------------------
def chain(members):
    """One component of the given transcripts in len - 1 classes of two (one transcript: one class of one)."""
    members = list(members)
    return [[a, b] for a, b in zip(members, members[1:])] if len(members) > 1 else [[members[0]]]


def _finish(classes, n_tx, seed):
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(classes))
    classes = [classes[i] for i in order]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int64)
    targets = np.concatenate([np.asarray(c, dtype=np.int32) for c in classes] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    counts = rng.integers(1, 40, len(classes)).astype('f8')
    return n_tx, offsets, targets, counts


def capacity_edge_table(segment, capacity, extra):
    """Three runs.  Run 0: a chain of two, then a chain of cap_tx - 2 (+ extra) transcripts.  Run 1: a chain of two in
    its one class, then two transcripts in cap_classes - 1 (+ extra) classes.  Run 2: a chain of five with its eight
    pairs, then eight transcripts in classes of all eight that come to cap_pairs - 8 (+ 8 extra) pairs.  With
    extra = 0 the second component fills the run's first tile exactly, with extra = 1 it opens the next."""
    cap_pairs, cap_classes, cap_tx = capacity
    assert cap_tx <= segment - 2 and cap_pairs % 8 == 0 and cap_pairs // 8 + 4 < cap_classes and cap_tx >= 13
    classes = chain([0, 1]) + chain(range(2, 2 + cap_tx - 2 + extra))
    t = segment
    classes += chain([t, t + 1]) + [[t + 2, t + 3]] + [[t + 2 + (i & 1)] for i in range(cap_classes - 2 + extra)]
    t = 2 * segment
    classes += chain(range(t, t + 5)) + [list(range(t + 5, t + 13))] * (cap_pairs // 8 - 1 + extra)
    return _finish(classes, 2 * segment + 15, 11 + extra)


def oversize_table(segment, capacity):
    """A component above each capacity (transcripts, classes, pairs), each between components that fit."""
    cap_pairs, cap_classes, cap_tx = capacity
    assert cap_tx + 1 <= segment - 8
    classes = chain([0, 1, 2]) + chain(range(3, 3 + cap_tx + 1)) + chain([cap_tx + 4, cap_tx + 5])
    t = segment
    classes += chain([t, t + 1]) + [[t + 2]] * (cap_classes + 1) + chain([t + 3, t + 4, t + 5])
    t = 2 * segment
    classes += chain([t]) + [[t + 1, t + 2, t + 3, t + 4, t + 5, t + 6, t + 7, t + 8]] * (cap_pairs // 8 + 1) + chain([t + 9, t + 10])
    return _finish(classes, 2 * segment + 11, 13)


def scattered_table(segment, capacity, seed=17):
    """Components whose transcripts lie far apart: component i of `comps` holds the ids i, i + comps, i + 2 comps, ...
    up to the last ids (so the transcripts of every tile are met interleaved with the others', and the lanes draw
    their places out of list order); component 0 reaches from id 0 into the last ids.  n_tx is no multiple of 64."""
    cap_pairs, cap_classes, cap_tx = capacity
    n_tx = 3 * segment + 37
    assert n_tx % 256 and n_tx % 64
    comps = 29
    rng = np.random.default_rng(seed)
    classes = []
    for i in range(comps):
        members = list(range(i, n_tx, comps))
        assert len(members) <= cap_tx
        classes += chain(members)
        for _ in range(int(rng.integers(5, 40))):
            classes.append([int(t) for t in rng.permutation(members)[:int(rng.integers(1, 12))]])
    assert n_tx - 1 - (n_tx - 1) % comps in range(0, n_tx)
    return _finish(classes, n_tx, seed)


def odd_members_table(segment, capacity):
    """Transcripts in no class (ids 3-5: a tile without classes when they are a run's only roots -- run 1 holds
    nothing else), classes without transcripts (listed with transcript 0's tile), and ordinary components."""
    classes = chain([0, 1, 2]) + [[], []] + chain([7, 8]) + [[8], []]
    n_tx = segment + 3                                       # (ids segment .. segment + 2: in no class, a run of their own)
    return _finish(classes, n_tx, 19)


def turn_caps_table(segment, capacity):
    """Ties and the caps of both keys: a transcript in more than 31 x 8 classes, a class of more than 31 x 4
    transcripts -- both within a tile's capacity -- and many members with equal keys."""
    cap_pairs, cap_classes, cap_tx = capacity
    wide = LONGEST * CLASS_BATCH + 3
    assert wide <= cap_tx and wide + 2 * 40 + 20 <= cap_pairs and wide <= segment
    classes = [list(range(wide)), list(range(1, wide))] + [[t] for t in range(20)] + [[t, t + 1] for t in range(0, 80, 2)]
    many = LONGEST * ROW_LANES + 5
    assert many + 40 <= cap_classes and many + 80 <= cap_pairs
    t = segment
    classes += [[t]] * many + [[t, t + 1 + (i % 9)] for i in range(36)] + [[t + 1 + i] for i in range(9)]
    return _finish(classes, segment + 12, 23)


def one_oversize_component_table(segment, capacity):
    """A table that is one component above the capacity in transcripts: no tiles at all."""
    return _finish(chain(range(capacity[2] + 1)), capacity[2] + 1, 29)


def single_transcript_table(segment, capacity):
    return _finish([[0], [0], [0]], 1, 31)


TABLES = {
    'capacity_exact': lambda s, c: capacity_edge_table(s, c, 0),
    'capacity_one_more': lambda s, c: capacity_edge_table(s, c, 1),
    'oversize': oversize_table,
    'scattered': scattered_table,
    'odd_members': odd_members_table,
    'turn_caps': turn_caps_table,
    'one_oversize_component': one_oversize_component_table,
    'single_transcript': single_transcript_table,
}
