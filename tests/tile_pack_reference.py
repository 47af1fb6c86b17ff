"""The packing rule of the tile EM's set-up (skm_quant_setup.hip: tile_pack_kernel) restated in plain
Python: the connected components of the (class, transcript) graph, named by their smallest transcript id,
go into tiles in id order within runs of `segment` transcript ids; a new tile begins with the run's first
component and whenever the next component would carry the open tile above one of the three capacities; a
component above a capacity by itself goes into no tile.  Tiles are numbered run after run."""
import numpy as np


def labels(n_tx, offsets, targets):
    """Smallest transcript id of every transcript's component (union-find, the smaller id on top)."""
    parent = list(range(n_tx))

    def root(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for c in range(len(offsets) - 1):
        tuple_ = targets[offsets[c]:offsets[c + 1]]
        for t in tuple_[1:]:
            a, b = root(int(tuple_[0])), root(int(t))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([root(t) for t in range(n_tx)], dtype=np.int64)


def component_sizes(n_tx, offsets, targets, label):
    """(transcripts, pairs, classes) of the component rooted at every transcript id (0 where none is).
    Every class is taken to hold at least one transcript."""
    offsets, targets = np.asarray(offsets, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    return (np.bincount(label, minlength=n_tx), np.bincount(label[targets], minlength=n_tx),
            np.bincount(label[targets[offsets[:-1]]], minlength=n_tx))


def pack(sizes, segment, capacity):
    """root_tile[r] of every transcript id r (-1: not a root, -2: above the capacity by itself), the number
    of tiles, and for every tile but a run's first the capacities that ended the tile before it: a subset
    of 'pairs', 'classes', 'tx', listed as (run, tile, kinds)."""
    c_tx, c_pairs, c_classes = sizes
    cap_pairs, cap_classes, cap_tx = capacity
    n_tx = len(c_tx)
    root_tile = np.full(n_tx, -1, dtype=np.int64)
    n_tiles, cuts = 0, []
    for first in range(0, n_tx, segment):
        tx = pairs = classes = 0
        opened = False
        for t in range(first, min(n_tx, first + segment)):
            if c_tx[t] == 0:
                continue
            if c_tx[t] > cap_tx or c_pairs[t] > cap_pairs or c_classes[t] > cap_classes:
                root_tile[t] = -2
                continue
            kinds = set()
            if pairs + c_pairs[t] > cap_pairs:
                kinds.add('pairs')
            if classes + c_classes[t] > cap_classes:
                kinds.add('classes')
            if tx + c_tx[t] > cap_tx:
                kinds.add('tx')
            if not opened or kinds:
                if opened:
                    cuts.append((first // segment, n_tiles, kinds))
                n_tiles += 1
                opened = True
                tx = pairs = classes = 0
            tx += c_tx[t]
            pairs += c_pairs[t]
            classes += c_classes[t]
            root_tile[t] = n_tiles - 1
    return root_tile, n_tiles, cuts


def tile_table(n_tx, offsets, targets, segment, capacity):
    """What the set-up must leave for a class table: tx_tile[n_tx] (n_tx: in no tile), the tiles' starts in
    transcripts, classes and pairs ([n_tiles + 1] each), the number of components in no tile, the cuts."""
    label = labels(n_tx, offsets, targets)
    sizes = component_sizes(n_tx, offsets, targets, label)
    root_tile, n_tiles, cuts = pack(sizes, segment, capacity)
    roots = np.nonzero(root_tile >= 0)[0]
    starts = []
    for size in sizes:
        per_tile = np.bincount(root_tile[roots], weights=size[roots], minlength=n_tiles).astype(np.int64)
        starts.append(np.concatenate([[0], np.cumsum(per_tile)]))
    tx_tile = np.where(root_tile[label] >= 0, root_tile[label], n_tx)
    return tx_tile, starts[0], starts[2], starts[1], int((root_tile == -2).sum()), cuts
