"""What `infer-many --bias` costs by either route: N samples of P read pairs each, mapped, quantified, corrected
for sequence bias and quantified again
    set         as infer.run_many does it for the samples of a sample set: one mapper.SampleSet(bias=True), the first
                estimates from SampleSet.quantify() (inside the regime of impute.use_set_quant), then
                infer.bias_pass_many -- one skm_bias_correct_many call and the second EM in shared launches
    per_sample  as SKM_INFER_MANY_PER_SAMPLE=1 does it (and as every `infer-many --bias` did before sample sets
                counted hexamers): a mapper of its own, quantify(), bias_pass() per sample
alternating in one process, a warm-up and then --reps repetitions each, with bit-equality of the corrected TPM,
eff', b and O asserted.  Host wall time per phase: mapping (with the summaries and the observed counts brought
home), first EM, correction (the skm_bias_correct* calls), second EM.
    python3 scripts/set_bias_rate.py --samples 64 --pairs 20000 --genes 100
    python3 scripts/set_bias_rate.py --samples 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
--only set|per_sample runs one route alone; --tree DIR measures the seekmer_amd of another checkout (a parent
commit knows `--only per_sample`).  --only correction maps once and then times infer.bias_correct_many alone: run
it once per tuning build of the lengths kernel,
    scripts/build_variant.sh g4 "-DSKM_BIAS_LENGTHS_G=4" skm_bias.hip
    SKM_HIP_LIB=seekmer_amd/libseekmer_hip_g4.so python3 scripts/set_bias_rate.py ... --only correction
(the variants differ in that kernel alone, so the difference between their times is the kernel's).  On a shared GPU
machine run every invocation under a time limit of its own (`timeout -k 10 600 python3 ...`), one per shape.
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--samples', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', choices=['set', 'per_sample', 'correction'], default=None)
ap.add_argument('--cache', default='')
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='the checkout whose seekmer_amd is measured (default: this one)')
args = ap.parse_args()
sys.path.insert(0, args.tree)
from seekmer_amd import common, impute, index_builder, infer, mapper, synth   # noqa: E402

PHASES = ('mapping', 'first EM', 'correction', 'second EM')


class Clock:
    """Wall time by phase; `inside` moves the time of a wrapped call from the phase around it to its own."""

    def __init__(self):
        self.seconds = dict.fromkeys(PHASES, 0.0)

    def phase(self, name, call):
        t0 = time.perf_counter()
        out = call()
        self.seconds[name] += time.perf_counter() - t0
        return out

    def inside(self, outer, inner, function):
        def timed(*a, **k):
            t0 = time.perf_counter()
            out = function(*a, **k)
            dt = time.perf_counter() - t0
            self.seconds[inner] += dt
            self.seconds[outer] -= dt
            return out
        return timed


def inputs():
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    if args.cache and os.path.exists(args.cache):
        index = common.KMerIndex.load(args.cache)
    else:
        index = index_builder.build_pooled(ids, pool, tx_offsets)
        if args.cache:
            index.save(args.cache)
    index.device_handle(0)
    batches = []
    for sample in range(args.samples):
        # two expression profiles, every sample its own stretch of the profile's read stream
        bases, offsets = synth.reads(100 + sample % 2, pool, tx_offsets, sample * args.pairs, args.pairs, args.read_len, True)
        batches.append(common.ReadBatch(args.pairs, bases, offsets, True))
    return index, batches


def route_set(index, batches, clock):
    def mapping():
        sample_set = mapper.SampleSet(index, True, per_sample_lengths=True, bias=True)
        for sample, batch in enumerate(batches):
            sample_set.add_batch(sample, 0, batch)
        return sample_set, sample_set.summarize(), sample_set.bias_observed()
    sample_set, summaries, observed = clock.phase('mapping', mapping)

    def first():
        if impute.use_set_quant(len(summaries), index.transcripts.size, sum(s.class_count.size for s in summaries)):
            return sample_set.quantify()
        return np.vstack([infer.quantify(s) for s in summaries])
    tpms = clock.phase('first EM', first)
    del sample_set
    passed, second = clock.phase('second EM', lambda: infer.bias_pass_many(index, summaries, tpms, observed, None))
    return second, np.vstack([s.effective_lengths for s in passed]), np.vstack([s.bias_weights for s in passed]), observed


def route_per_sample(index, batches, clock):
    second, eff, weights, observed = [], [], [], []
    for batch in batches:
        def mapping():
            result = mapper.MapResult(index, bias=True)
            mapper.ReadMapper(index, result).map_batch(batch)
            return result.summarize().detach(), result.bias_observed()
        summary, counts = clock.phase('mapping', mapping)
        tpm = clock.phase('first EM', lambda: infer.quantify(summary))
        summary, tpm = clock.phase('second EM', lambda: infer.bias_pass(index, summary, tpm, counts, None))
        second.append(tpm), eff.append(summary.effective_lengths), weights.append(summary.bias_weights), observed.append(counts)
    return tuple(map(np.vstack, (second, eff, weights, observed)))


def report(name, runs):
    n = args.samples
    totals = [sum(run.values()) for run in runs]
    print('%-10s warm-up %.1f ms; then %s ms -> %.2f .. %.2f ms per sample'
          % (name, totals[0] * 1e3, ', '.join('%.1f' % (t * 1e3) for t in totals[1:]), min(totals[1:]) * 1e3 / n,
             max(totals[1:]) * 1e3 / n), flush=True)
    for phase in PHASES:
        times = [run[phase] * 1e3 for run in runs[1:]]
        print('  %-10s %s ms (best %.2f ms per sample)' % (phase, ', '.join('%.1f' % t for t in times), min(times) / n), flush=True)
    return totals[1:]


def correction_only(index, batches):
    clock = Clock()
    sample_set = mapper.SampleSet(index, True, per_sample_lengths=True, bias=True)
    for sample, batch in enumerate(batches):
        sample_set.add_batch(sample, 0, batch)
    summaries, observed = sample_set.summarize(), sample_set.bias_observed()
    tpms = np.vstack([infer.quantify(s) for s in summaries]) if not impute.use_set_quant(
        len(summaries), index.transcripts.size, sum(s.class_count.size for s in summaries)) else sample_set.quantify()
    times = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        out = infer.bias_correct_many(index, summaries, tpms, observed, None)
        times.append(time.perf_counter() - t0)
    del clock
    print('correction (%s): warm-up %.1f ms; then %s ms -> best %.3f ms per sample; eff\' checksum %.17g'
          % (os.environ.get('SKM_HIP_LIB') or 'the product library', times[0] * 1e3, ', '.join('%.1f' % (t * 1e3) for t in times[1:]),
             min(times[1:]) * 1e3 / args.samples, float(np.nansum(out[0]))), flush=True)


def main():
    t0 = time.perf_counter()
    index, batches = inputs()
    print('%d samples x %d pairs on %d transcripts: index and reads made in %.1f s'
          % (args.samples, args.pairs, index.transcripts.size, time.perf_counter() - t0), flush=True)
    if args.only == 'correction':
        return correction_only(index, batches)
    routes = {'set': route_set, 'per_sample': route_per_sample}
    names = [args.only] if args.only else list(routes)
    runs, last = {name: [] for name in names}, {}
    for _ in range(args.reps + 1):                   # (the first repetition of every route is its warm-up)
        for name in names:
            clock = Clock()
            saved = infer.bias_correct, getattr(infer, 'bias_correct_many', None)
            infer.bias_correct = clock.inside('second EM', 'correction', saved[0])
            if saved[1] is not None:
                infer.bias_correct_many = clock.inside('second EM', 'correction', saved[1])
            try:
                last[name] = routes[name](index, batches, clock)
            finally:
                infer.bias_correct = saved[0]
                if saved[1] is not None:
                    infer.bias_correct_many = saved[1]
            runs[name].append(clock.seconds)
    totals = {name: report(name, runs[name]) for name in names}
    print('observed hexamers per sample: %d .. %d' % (last[names[0]][3].sum(axis=1).min(), last[names[0]][3].sum(axis=1).max()), flush=True)
    if len(names) > 1:
        for got, want, what in zip(last['set'], last['per_sample'], ('corrected TPM', "eff'", 'b', 'O')):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), what + ' differs between the routes'
        print('the routes agree bit for bit (corrected TPM, eff\', b, O of %d samples)' % args.samples, flush=True)
        per_sample = totals['per_sample']
        print('per_sample / set = %.2f (best of each); per_sample\'s own spread: %.1f .. %.1f ms; set: %.1f .. %.1f ms'
              % (min(per_sample) / min(totals['set']), min(per_sample) * 1e3, max(per_sample) * 1e3,
                 min(totals['set']) * 1e3, max(totals['set']) * 1e3), flush=True)


if __name__ == '__main__':
    main()
