#!/usr/bin/env python
"""Census of the connected components of the (class, transcript) graph: what the component EM
(skm_em.hip: em_local_chunk_kernel) keeps in one tile, and what share of a table lies in components
above the tile capacity (the residual).  CPU only: the host library builds the index and draws the
reads, the oracle maps them and counts the classes, numpy labels the components.

    python scripts/em_component_census.py --genes 2000 --pairs 1000000
    python scripts/em_component_census.py --chr21            # tests/golden/human.cdna.21.fa.bz2
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tile_capacity():
    """(pairs, classes, transcripts): EM_TILE_* as seekmer_amd/csrc/skm_kernels.h defines them."""
    import re
    text = open(os.path.join(ROOT, 'seekmer_amd', 'csrc', 'skm_kernels.h')).read()
    return tuple(int(re.search(r'#define SKM_%s (\d+)' % name, text).group(1))
                 for name in ('EM_TILE_PAIRS', 'EM_TILE_CLASSES', 'EM_TILE_TX'))


CAPACITY = tile_capacity()



def labels(n_tx, cls, tx):
    """Smallest transcript id of every transcript's component (min-label propagation + pointer jumping)."""
    label = np.arange(n_tx, dtype=np.int64)
    n_classes = int(cls.max()) + 1 if cls.size else 0
    while True:
        low = np.full(n_classes, n_tx, dtype=np.int64)
        np.minimum.at(low, cls, label[tx])
        new = label.copy()
        np.minimum.at(new, tx, low[cls])
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def census(name, n_tx, class_map):
    cls, tx = np.asarray(class_map[0], dtype=np.int64), np.asarray(class_map[1], dtype=np.int64)
    label = labels(n_tx, cls, tx)
    used = np.zeros(n_tx, dtype=bool)
    used[tx] = True
    roots = np.unique(label[used])
    index = np.full(n_tx, -1, dtype=np.int64)
    index[roots] = np.arange(roots.size)
    pairs = np.bincount(index[label[tx]], minlength=roots.size)
    first = np.ones(cls.size, dtype=bool)
    first[1:] = cls[1:] != cls[:-1]
    classes = np.bincount(index[label[tx[first]]], minlength=roots.size)
    transcripts = np.bincount(index[label[used.nonzero()[0]]], minlength=roots.size)
    print('%s: %d transcripts (%d in no class), %d classes, %d pairs, %d components'
          % (name, n_tx, int((~used).sum()), int(first.sum()), cls.size, roots.size))
    print('  %-12s %8s %8s %8s %8s' % ('', 'mean', 'median', '99th', 'max'))
    for what, v in (('pairs', pairs), ('classes', classes), ('transcripts', transcripts)):
        print('  %-12s %8.1f %8d %8d %8d' % (what, v.mean(), np.median(v), np.percentile(v, 99), v.max()))
    over = (pairs > CAPACITY[0]) | (classes > CAPACITY[1]) | (transcripts > CAPACITY[2])
    print('  above the capacity %s: %d components, %.2f %% of the pairs, %.2f %% of the classes, %.2f %% of the transcripts'
          % (CAPACITY, int(over.sum()), 100.0 * pairs[over].sum() / max(pairs.sum(), 1),
             100.0 * classes[over].sum() / max(classes.sum(), 1), 100.0 * transcripts[over].sum() / max(n_tx, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--pairs', type=int, default=0, help='read pairs (default: 500 per gene; chr21: 50 per transcript)')
    ap.add_argument('--read-len', type=int, default=100)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--chr21', action='store_true', help='the chr21 cDNA of tests/golden instead of a synthetic transcriptome')
    args = ap.parse_args()
    from oracle import oracle as O
    from seekmer_amd import index_builder, synth
    O.build_library()
    if args.chr21:
        ids, seqs = O.read_fasta(os.path.join(ROOT, 'tests', 'golden', 'human.cdna.21.fa.bz2'))
        lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        tx_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        pool = np.frombuffer(b''.join(seqs) + b'\0', dtype=np.uint8).copy()
        n_units = args.pairs or 50 * len(ids)
        name = 'chr21'
    else:
        ids, pool, tx_offsets = synth.transcriptome(args.seed, args.genes)
        n_units = args.pairs or 500 * args.genes
        name = 'synthetic, %d genes' % args.genes
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    bases, offsets = synth.reads(args.seed, pool, tx_offsets, 0, n_units, args.read_len, True)
    oindex = O.OracleIndex(index.kmers, index.contigs, index.sequences, index.targets, lengths=np.diff(tx_offsets))
    fld = np.zeros(2000, dtype=np.int64)
    mapped = O.map_batch(oindex, bases, offsets, n_units, True, fld)
    classes = O.Classes()
    classes.update(mapped)
    class_map, _ = classes.summarize()
    print('%d pairs of 2 x %d, %d unaligned' % (n_units, args.read_len, classes.unaligned))
    census(name, len(ids), class_map)


if __name__ == '__main__':
    main()
