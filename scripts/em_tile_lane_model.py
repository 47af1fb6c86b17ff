#!/usr/bin/env python
"""Lane use of the tile EM (skm_em.hip: em_local_chunk_kernel) on a mapped table, modelled on the CPU:
the tiles as tile_pack_kernel packs them, the order of a tile's lists as build_tiles sorts them, and per
EM step the turns every wave of a tile takes in the class phase (one lane per class, a wave loops as long
as the longest of its 64 classes) and in the row phase (eight lanes per transcript, a wave loops as long
as the longest of its eight transcripts).  The host library builds the index and draws the reads, the
oracle maps them and counts the classes.

    python scripts/em_tile_lane_model.py --genes 2000 --pairs 1000000

prints the figures under three rules for the class phase: one entry a turn with the classes in internal
order (how the kernel began), one entry a turn with the classes by length, and the tree's rule -- batches
of EM_TILE_CLASS_BATCH entries a turn, the classes by their number of batches.
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from em_component_census import labels    # noqa: E402


def constants():
    text = open(os.path.join(ROOT, 'seekmer_amd', 'csrc', 'skm_kernels.h')).read()
    return {name: int(re.search(r'(?:#define SKM_%s|\b%s =) (\d+)' % (name, name), text).group(1))
            for name in ('EM_TILE_PAIRS', 'EM_TILE_CLASSES', 'EM_TILE_TX', 'EM_TILE_SEGMENT', 'EM_TILE_CLASS_BATCH', 'EM_ROW_CAP')}


def internal_order(class_map, n_tx):
    """(offsets, targets) of the classes in the set-up's order: by smallest transcript id, then first seen."""
    cls, tx = np.asarray(class_map[0], dtype=np.int64), np.asarray(class_map[1], dtype=np.int64)
    n = int(cls.max()) + 1
    lens = np.bincount(cls, minlength=n)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    low = np.full(n, n_tx, dtype=np.int64)
    np.minimum.at(low, cls, tx)
    order = np.argsort(low, kind='stable')
    new_offsets = np.concatenate([[0], np.cumsum(lens[order])])
    targets = np.concatenate([tx[offsets[c]:offsets[c + 1]] for c in order])
    return new_offsets, targets


def pack_tiles(n_tx, offsets, targets, k):
    """tile_pack_kernel: tile of every transcript (-1: its component is above the capacity)."""
    lens = np.diff(offsets)
    cls = np.repeat(np.arange(lens.size), lens)
    label = labels(n_tx, cls, targets)
    c_tx = np.bincount(label, minlength=n_tx)
    c_pairs = np.bincount(label[targets], minlength=n_tx)
    c_classes = np.bincount(label[targets[offsets[:-1][lens > 0]]], minlength=n_tx)
    root_tile = np.full(n_tx, -1, dtype=np.int64)
    n_tiles = 0
    for first in range(0, n_tx, k['EM_TILE_SEGMENT']):
        tx = pairs = classes = 0
        opened = False
        for t in range(first, min(n_tx, first + k['EM_TILE_SEGMENT'])):
            if c_tx[t] == 0:
                continue
            if c_tx[t] > k['EM_TILE_TX'] or c_pairs[t] > k['EM_TILE_PAIRS'] or c_classes[t] > k['EM_TILE_CLASSES']:
                continue
            if (not opened or tx + c_tx[t] > k['EM_TILE_TX'] or pairs + c_pairs[t] > k['EM_TILE_PAIRS']
                    or classes + c_classes[t] > k['EM_TILE_CLASSES']):
                n_tiles += 1
                opened = True
                tx = pairs = classes = 0
            tx += c_tx[t]
            pairs += c_pairs[t]
            classes += c_classes[t]
            root_tile[t] = n_tiles - 1
    return root_tile[label], n_tiles


def wave_turns(turns_in_list_order, per_wave, waves=4):
    """Turns of the four waves of one tile: the list is dealt `per_wave` items a wave, pass after pass; a
    wave's pass lasts as long as its longest item."""
    total = np.zeros(waves, dtype=np.int64)
    n = turns_in_list_order.size
    for first in range(0, n, per_wave * waves):
        for w in range(waves):
            part = turns_in_list_order[first + w * per_wave:first + (w + 1) * per_wave]
            if part.size:
                total[w] += part.max()
    return total


def by_turns(turns, bits=5):
    """build_tiles' sort inside a tile: many turns first (capped at 2^bits - 1), stable."""
    cap = (1 << bits) - 1
    return np.argsort(cap - np.minimum(turns, cap), kind='stable')


def report(name, per_tile, useful, lanes_per_item):
    """per_tile: the four waves' turns of every tile; useful: lane-turns that do work (ideal: no lane idles)."""
    per_tile = np.array(per_tile)
    wave_iterations = int(per_tile.sum())
    ideal = useful * lanes_per_item / 64.0
    print('  %-44s %7d wave-iterations (ideal %7d), lane use %.2f, slowest wave of a tile %.1f, mean wave %.1f'
          % (name, wave_iterations, int(ideal), ideal / max(wave_iterations, 1), per_tile.max(axis=1).mean(), per_tile.mean()))


def model(n_tx, class_map):
    k = constants()
    offsets, targets = internal_order(class_map, n_tx)
    lens = np.diff(offsets)
    tx_tile, n_tiles = pack_tiles(n_tx, offsets, targets, k)
    cls_tile = tx_tile[targets[offsets[:-1]]]
    degree = np.bincount(targets, minlength=n_tx)
    in_tiles = tx_tile >= 0
    print('%d tiles; per tile %.0f pairs, %.0f classes, %.0f transcripts; %d transcripts in components above the capacity'
          % (n_tiles, lens[cls_tile >= 0].sum() / max(n_tiles, 1), (cls_tile >= 0).sum() / max(n_tiles, 1),
             in_tiles.sum() / max(n_tiles, 1), int((~in_tiles).sum())))
    batch = k['EM_TILE_CLASS_BATCH']
    cls_by_tile = [[] for _ in range(n_tiles)]
    for c in np.nonzero(cls_tile >= 0)[0]:
        cls_by_tile[cls_tile[c]].append(c)
    tx_by_tile = [[] for _ in range(n_tiles)]
    for t in np.nonzero(in_tiles)[0]:
        tx_by_tile[tx_tile[t]].append(t)
    serial, serial_sorted, batched, rows = [], [], [], []
    for tile in range(n_tiles):
        n = lens[np.array(cls_by_tile[tile], dtype=np.int64)]
        serial.append(wave_turns(n, 64))
        serial_sorted.append(wave_turns(n[by_turns(n)], 64))
        b = (n + batch - 1) // batch
        batched.append(wave_turns(b[by_turns(b)], 64))
        d = degree[np.array(tx_by_tile[tile], dtype=np.int64)]
        full, rest = d // k['EM_ROW_CAP'], d % k['EM_ROW_CAP']
        turns = full * (k['EM_ROW_CAP'] // 8) + (rest + 7) // 8
        rows.append(wave_turns(turns[by_turns((d + 7) // 8)], 8))
    in_tile_lens = lens[cls_tile >= 0]
    print('class phase, per EM step:')
    report('one entry a turn, internal class order', serial, in_tile_lens.sum(), 1)
    report('one entry a turn, classes by length', serial_sorted, in_tile_lens.sum(), 1)
    report('%d entries a turn, classes by turns (the tree)' % batch, batched, ((in_tile_lens + batch - 1) // batch).sum(), 1)
    print('row phase, per EM step (a turn is one division per lane):')
    report('transcripts by turns (the tree)', rows, degree[in_tiles].sum(), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--pairs', type=int, default=0, help='read pairs (default: 500 per gene)')
    ap.add_argument('--read-len', type=int, default=100)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    from oracle import oracle as O
    from seekmer_amd import index_builder, synth
    O.build_library()
    ids, pool, tx_offsets = synth.transcriptome(args.seed, args.genes)
    n_units = args.pairs or 500 * args.genes
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    bases, offsets = synth.reads(args.seed, pool, tx_offsets, 0, n_units, args.read_len, True)
    oindex = O.OracleIndex(index.kmers, index.contigs, index.sequences, index.targets, lengths=np.diff(tx_offsets))
    fld = np.zeros(2000, dtype=np.int64)
    mapped = O.map_batch(oindex, bases, offsets, n_units, True, fld)
    classes = O.Classes()
    classes.update(mapped)
    class_map, _ = classes.summarize()
    print('synthetic, %d genes, %d pairs of 2 x %d, %d unaligned' % (args.genes, n_units, args.read_len, classes.unaligned))
    model(len(ids), class_map)


if __name__ == '__main__':
    main()
