"""Rate of the second round of `impute`: N cells quantified again on the blend of all cells' class
tables, as the batched EM with device-made counts (the default) and as the loop over the cells
(SKM_IMPUTE_SERIAL=1), alternating in one process, with bit-equality of the two asserted.
    python3 scripts/impute_rate.py --cells 64 --pairs 20000 --genes 100
    python3 scripts/impute_rate.py --cells 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
The batched form is measured whatever the shape (the rule of requantify_blend that keeps the loop outside
the measured regime, impute.BATCH_*, is set aside while it is timed: the numbers behind it come from here).
On a shared GPU machine run every invocation under a time limit of its own (`timeout -k 10 600 python3 ...`).
--only batched|serial runs one form alone (for a kernel trace); on a tree without the batched path the
serial form is whatever requantify_blend does there.
"""
import argparse
import os
import sys
import time
import types

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--cells', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--power', type=int, default=4)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', choices=['batched', 'serial'], default=None)
ap.add_argument('--cache', default='')
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='the checkout whose seekmer_amd is measured (default: this one)')
args = ap.parse_args()
sys.path.insert(0, args.tree)
from seekmer_amd import common, impute, index_builder, infer, mapper, synth   # noqa: E402

SERIAL = 'SKM_IMPUTE_SERIAL'
# the rule of requantify_blend that keeps the loop outside the measured regime, set aside while the
# batched form is timed (and put back afterwards)
RULE = {'BATCH_MIN_CELLS': 1, 'BATCH_MAX_CLASSES': 1 << 62, 'BATCH_MAX_TRANSCRIPTS': 1 << 62}


def cells_and_weights():
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    if args.cache and os.path.exists(args.cache):
        index = common.KMerIndex.load(args.cache)
    else:
        index = index_builder.build_pooled(ids, pool, tx_offsets)
        if args.cache:
            index.save(args.cache)
    results = []
    t0 = time.perf_counter()
    for cell in range(args.cells):
        # two expression profiles, every cell its own stretch of the profile's read stream
        bases, offsets = synth.reads(100 + cell % 2, pool, tx_offsets, cell * args.pairs, args.pairs, args.read_len, True)
        result = mapper.MapResult(index)
        mapper.ReadMapper(index, result).map_batch(common.ReadBatch(args.pairs, bases, offsets, True))
        results.append(result)
    impute.pool_fragment_lengths(results)
    full = [result.summarize() for result in results]
    t_map = time.perf_counter() - t0
    t0 = time.perf_counter()
    base = np.asarray([infer.quantify(summary) for summary in full])
    t_first = time.perf_counter() - t0
    # (only what the second round reads is kept: the cells' device tables go)
    summaries = [types.SimpleNamespace(class_map=s.class_map, class_count=s.class_count,
                                       effective_lengths=s.effective_lengths) for s in full]
    del full, results
    # the reference's weights need gene names: four consecutive transcripts a gene
    transcripts = np.zeros(len(ids), dtype=[('transcript_id', 'S16'), ('gene_id', 'S12'), ('length', 'f8')])
    transcripts['gene_id'] = [b'GENE%07d' % (t // 4) for t in range(len(ids))]
    named = types.SimpleNamespace(transcripts=transcripts)
    weight = impute.cell_weights(named, base, seed=0) ** args.power
    classes = [s.class_count.size for s in summaries]
    print('%d cells x %d pairs on %d transcripts: mapped + summarized in %.1f s, first round %.1f ms per cell; '
          'classes per cell %d .. %d, blended structure %d classes, %d pairs; weights: %.0f %% zero'
          % (args.cells, args.pairs, len(ids), t_map, t_first * 1e3 / args.cells, min(classes), max(classes),
             sum(classes), sum(s.class_map.shape[1] for s in summaries), 100.0 * (weight == 0).mean()), flush=True)
    return summaries, weight


def second_round(summaries, weight, serial):
    rule = {name: getattr(impute, name) for name in RULE if hasattr(impute, name)}
    if serial:
        os.environ[SERIAL] = '1'
    else:
        os.environ.pop(SERIAL, None)
        for name in rule:
            setattr(impute, name, RULE[name])
    try:
        t0 = time.perf_counter()
        columns = impute.requantify_blend(summaries, weight)
        dt = time.perf_counter() - t0
    finally:
        os.environ.pop(SERIAL, None)
        for name, value in rule.items():
            setattr(impute, name, value)
    return np.asarray(columns), dt


def report(name, times):
    n = args.cells
    rest = times[1:] or times
    print('%-8s first repetition %.1f ms (%.2f ms per cell); then %s ms -> best %.2f ms per cell, %.1f cells/s'
          % (name, times[0] * 1e3, times[0] * 1e3 / n, ', '.join('%.1f' % (t * 1e3) for t in rest),
             min(rest) * 1e3 / n, n / min(rest)), flush=True)


def counts_cost(summaries, weight):
    """What making and moving the counts costs each form, measured apart from the EM."""
    t0 = time.perf_counter()
    offsets, targets, counts = impute.blend(summaries, weight)
    t_blend = time.perf_counter() - t0
    n_tx = summaries[0].effective_lengths.size
    handle = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts[0])
    try:
        t0 = time.perf_counter()
        for row in counts:
            handle.set_counts(row)
        t_set = time.perf_counter() - t0
        print('counts, loop over the cells: numpy blend() %.1f ms + %d x set_counts (sum, upload, permute) %.1f ms'
              % (t_blend * 1e3, len(counts), t_set * 1e3), flush=True)
        if not hasattr(handle, 'em_blend'):
            return
        l = summaries[0].effective_lengths.astype('f8')
        x0 = 1.0 / l
        x0 /= x0.sum()
        own, class_cell, cell_total = impute.blend_sources(summaries)
        handle.set_counts(own)
        rows = np.asarray(counts)
        times = {}
        for name, call in (('rows uploaded (em_many)', lambda: handle.em_many(rows, x0, l, tpm=True)),
                           ('rows made on the device (em_blend)',
                            lambda: handle.em_blend(class_cell, weight, cell_total, x0, l, tpm=True))):
            call()
            t0 = time.perf_counter()
            out = call()
            times[name] = time.perf_counter() - t0
            print('batched EM, %s: %.1f ms' % (name, times[name] * 1e3), flush=True)
        steps = np.asarray(out[1])
        print('steps per cell: min %d, quartiles %d / %d / %d, max %d, mean %.1f'
              % (steps.min(), *np.percentile(steps, [25, 50, 75]).astype(int), steps.max(), steps.mean()), flush=True)
    finally:
        handle.close()


def main():
    summaries, weight = cells_and_weights()
    forms = [('batched', False), ('serial', True)]
    if args.only:
        forms = [form for form in forms if form[0] == args.only]
    times = {name: [] for name, _ in forms}
    last = {}
    for _ in range(args.reps):
        for name, serial in forms:
            last[name], dt = second_round(summaries, weight, serial)
            times[name].append(dt)
    for name, _ in forms:
        report(name, times[name])
    if len(forms) == 2:
        assert np.array_equal(last['batched'], last['serial']), 'the two forms differ'
        print('the two forms agree bit for bit (%d x %d TPM values); serial / batched = %.2f (best of the later repetitions)'
              % (*last['batched'].shape, min(times['serial'][1:] or times['serial']) / min(times['batched'][1:] or times['batched'])),
              flush=True)
        counts_cost(summaries, weight)


if __name__ == '__main__':
    main()
