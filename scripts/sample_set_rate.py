"""Rate of the mapping stage for many small samples: N cells of P read pairs each from packed host arrays to
exported class tables, through one sample set (mapper.map_sample_set) and through a mapper per cell
(mapper.map_multiple_samples), alternating in one process, with equality of all tables asserted.
    python3 scripts/sample_set_rate.py --cells 64 --pairs 20000 --genes 100
    python3 scripts/sample_set_rate.py --cells 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
    python3 scripts/sample_set_rate.py --cells 4 --pairs 2000000 --genes 100
Generating the reads and packing them to 2-bit codes (what a FASTQ reader hands out) happens before the
clock starts; the timed region of a form runs from the call that maps to the last exported table.
--lengths per_sample: the set keeps a fragment-length histogram per sample (spans stored by the map kernel, counted
by sample after every launch); the timed region then also reads the histograms, and they are compared with the
per-cell mappers' own.  --only set|per_cell runs one form alone (for a kernel trace); --tree DIR measures the seekmer_amd of another
checkout -- on one without sample sets only the per-cell form exists, which is how the parent commit is timed.
On a shared GPU machine run every invocation under a time limit of its own (`timeout -k 10 600 python3 ...`).
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--cells', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', choices=['set', 'per_cell'], default=None)
ap.add_argument('--lengths', choices=['pooled', 'per_sample'], default='pooled')
ap.add_argument('--cache', default='')
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='the checkout whose seekmer_amd is measured (default: this one)')
args = ap.parse_args()
sys.path.insert(0, args.tree)
from seekmer_amd import common, index_builder, mapper, synth   # noqa: E402


class Cell:
    """A cell's reads as a feeder: the two mates as packed pieces over arrays of their own."""
    paired = True

    def __init__(self, pieces):
        self.pieces = pieces

    def __iter__(self):
        return iter(self.pieces)


def make_cells():
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    if args.cache and os.path.exists(args.cache):
        index = common.KMerIndex.load(args.cache)
    else:
        index = index_builder.build_pooled(ids, pool, tx_offsets)
        if args.cache:
            index.save(args.cache)
    t0 = time.perf_counter()
    cells = []
    length = args.read_len
    for cell in range(args.cells):
        # two expression profiles, every cell its own stretch of the profile's read stream
        bases, _ = synth.reads(100 + cell % 2, pool, tx_offsets, cell * args.pairs, args.pairs, length, True)
        reads = bases[:args.pairs * 2 * length].reshape(args.pairs, 2, length)
        offsets = np.arange(args.pairs + 1, dtype=np.int64) * length
        cells.append(Cell([common.PackedReads.from_ascii(np.append(reads[:, mate].reshape(-1), np.uint8(0)), offsets,
                                                         stream=mate, first_read=0, paired=True) for mate in (0, 1)]))
    print('%d cells x %d pairs of 2 x %d bases on %d transcripts; reads made and packed in %.1f s (not timed)'
          % (args.cells, args.pairs, length, len(ids), time.perf_counter() - t0), flush=True)
    return index, cells


def through_set(index, cells):
    t0 = time.perf_counter()
    per_sample = args.lengths == 'per_sample'
    sample_set = mapper.map_sample_set(index, cells, job_count=args.jobs, **({'per_sample_lengths': True} if per_sample else {}))
    sizes = sample_set.sizes()
    tables = sample_set.export()
    flds = sample_set.sample_fragment_length_counts if per_sample else None
    dt = time.perf_counter() - t0
    return ([(tuple(int(v) for v in size), table) for size, table in zip(sizes, tables)],
            flds if per_sample else sample_set.fragment_length_counts, dt)


def per_cell(index, cells):
    t0 = time.perf_counter()
    results = mapper.map_multiple_samples(index, cells, job_count=args.jobs)
    tables = [(result.sizes(), result.export()) for result in results]
    dt = time.perf_counter() - t0
    flds = np.asarray([table[4] for _, table in tables], dtype=np.int64)
    fld = flds if args.lengths == 'per_sample' else np.sum(flds, axis=0, dtype=np.int64)
    return [(size, table[:4]) for size, table in tables], fld, dt


def report(name, times):
    n = args.cells
    rest = times[1:] or times
    print('%-8s first repetition %.1f ms (%.2f ms per cell); then %s ms -> best %.2f ms per cell, %.2f M pairs/s; '
          'spread of the later repetitions %.1f ms'
          % (name, times[0] * 1e3, times[0] * 1e3 / n, ', '.join('%.1f' % (t * 1e3) for t in rest), min(rest) * 1e3 / n,
             n * args.pairs / min(rest) / 1e6, (max(rest) - min(rest)) * 1e3), flush=True)


def main():
    index, cells = make_cells()
    forms = [('set', through_set), ('per_cell', per_cell)]
    if not hasattr(mapper, 'map_sample_set'):
        forms = forms[1:]
        print('this tree has no sample sets: the per-cell form alone', flush=True)
    if args.only:
        forms = [form for form in forms if form[0] == args.only]
    times = {name: [] for name, _ in forms}
    last = {}
    for _ in range(args.reps):
        for name, run in forms:
            tables, fld, dt = run(index, cells)
            last[name] = (tables, fld)
            times[name].append(dt)
    for name, _ in forms:
        report(name, times[name])
    if len(forms) == 2:
        (ours, our_fld), (theirs, their_fld) = last['set'], last['per_cell']
        assert len(ours) == len(theirs) == args.cells
        for i, ((size, table), (want_size, want)) in enumerate(zip(ours, theirs)):
            assert size == want_size, 'sizes of cell %d differ' % i
            for a, b in zip(table, want):
                assert np.array_equal(a, b), 'tables of cell %d differ' % i
        assert np.array_equal(our_fld, their_fld), 'the %s differ' % ('histograms by sample' if args.lengths == 'per_sample'
                                                                      else 'pooled histograms')
        classes = [size[0] for size, _ in ours]
        print('all %d tables and the %s agree (classes per cell %d .. %d); per_cell / set = %.2f '
              '(best of the later repetitions)'
              % (args.cells, 'histograms by sample' if args.lengths == 'per_sample' else 'pooled histogram', min(classes), max(classes),
                 min(times['per_cell'][1:] or times['per_cell']) / min(times['set'][1:] or times['set'])), flush=True)


if __name__ == '__main__':
    main()
