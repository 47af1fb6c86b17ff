"""Rate of the first round of `impute` / the main estimates of `infer-many`: N cells, mapped through one
sample set, quantified each on its own class table in three forms --
    set     mapper.SampleSet.quantify(): shared EM launches on the set's resident table
    tables  infer.quantify_tables(summaries): the same launches from the summaries' host tables
    loop    [infer.quantify(summary) for summary in summaries]: today's loop
alternating in one process, a warm-up and then --reps repetitions each, with bit-equality of the TPM asserted.
    python3 scripts/set_quant_rate.py --cells 64 --pairs 20000 --genes 100
    python3 scripts/set_quant_rate.py --cells 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
--only set|tables|loop runs one form alone (for a kernel trace, or for a tree that lacks the others);
--tree DIR measures the seekmer_amd of another checkout: the parent commit's loop is taken with
`--tree <parent checkout> --only loop`.  On a shared GPU machine run every invocation under a time limit of
its own (`timeout -k 10 600 python3 ...`).
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
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--own-lengths', action='store_true', help='a fragment-length histogram per cell (infer-many), not the pooled one (impute)')
ap.add_argument('--only', choices=['set', 'tables', 'loop'], default=None)
ap.add_argument('--cache', default='')
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='the checkout whose seekmer_amd is measured (default: this one)')
args = ap.parse_args()
sys.path.insert(0, args.tree)
from seekmer_amd import common, index_builder, infer, mapper, synth   # noqa: E402


def mapped_set():
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    if args.cache and os.path.exists(args.cache):
        index = common.KMerIndex.load(args.cache)
    else:
        index = index_builder.build_pooled(ids, pool, tx_offsets)
        if args.cache:
            index.save(args.cache)
    t0 = time.perf_counter()
    sample_set = mapper.SampleSet(index, True, per_sample_lengths=args.own_lengths)
    for cell in range(args.cells):
        # two expression profiles, every cell its own stretch of the profile's read stream
        bases, offsets = synth.reads(100 + cell % 2, pool, tx_offsets, cell * args.pairs, args.pairs, args.read_len, True)
        sample_set.add_batch(cell, 0, common.ReadBatch(args.pairs, bases, offsets, True))
    summaries = sample_set.summarize()
    classes = [s.class_count.size for s in summaries]
    print('%d cells x %d pairs on %d transcripts (%s lengths): made, mapped + summarized in %.1f s; classes per cell %d .. %d, '
          '%d in all, %d pairs' % (args.cells, args.pairs, len(ids), 'own' if args.own_lengths else 'pooled',
                                   time.perf_counter() - t0, min(classes), max(classes), sum(classes),
                                   sum(s.class_map.shape[1] for s in summaries if s.class_map.size)), flush=True)
    return sample_set, summaries


def report(name, times):
    n = args.cells
    print('%-7s warm-up %.1f ms; then %s ms -> %.2f .. %.2f ms per cell, best %.1f cells/s'
          % (name, times[0] * 1e3, ', '.join('%.1f' % (t * 1e3) for t in times[1:]), min(times[1:]) * 1e3 / n,
             max(times[1:]) * 1e3 / n, n / min(times[1:])), flush=True)


def main():
    sample_set, summaries = mapped_set()
    forms = {'set': lambda: sample_set.quantify(return_iters=True),
             'tables': lambda: infer.quantify_tables(summaries, return_iters=True),
             'loop': lambda: tuple(map(np.asarray, zip(*[infer.quantify(s, return_iters=True) for s in summaries])))}
    names = [args.only] if args.only else list(forms)
    times = {name: [] for name in names}
    last = {}
    for _ in range(args.reps + 1):                   # (the first repetition of every form is its warm-up)
        for name in names:
            t0 = time.perf_counter()
            last[name] = forms[name]()
            times[name].append(time.perf_counter() - t0)
    for name in names:
        report(name, times[name])
    steps = np.asarray(last[names[0]][1])
    print('steps per cell: min %d, quartiles %d / %d / %d, max %d, mean %.1f'
          % (steps.min(), *np.percentile(steps, [25, 50, 75]).astype(int), steps.max(), steps.mean()), flush=True)
    for name in names[1:]:
        assert np.array_equal(last[name][0], last[names[0]][0]), 'TPM of %s and %s differ' % (name, names[0])
        assert np.array_equal(last[name][1], last[names[0]][1]), 'steps of %s and %s differ' % (name, names[0])
    if len(names) > 1:
        loop = times['loop'][1:]
        print('the forms agree bit for bit (%d x %d TPM values, and the step counts)' % last[names[0]][0].shape, flush=True)
        for name in names:
            if name != 'loop':
                print('loop / %s = %.2f (best of each); the loop\'s own spread: %.1f .. %.1f ms'
                      % (name, min(loop) / min(times[name][1:]), min(loop) * 1e3, max(loop) * 1e3), flush=True)


if __name__ == '__main__':
    main()
