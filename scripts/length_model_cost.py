#!/usr/bin/env python3
"""What the fragment-length model costs where it is used once per sample: skm_effective_lengths_weights against
skm_effective_lengths at the 190 402 transcripts of BASELINE configs[1], whole calls (lengths up, kernel, lengths
home), the forms alternating in one process, one JSON line per form.

    timeout 600 python scripts/length_model_cost.py [--reps R] [--warmup W] [--transcripts T] [--histogram-only] [--label L]

The kernel's loop visits the bins with p != 0, so the cost follows their number: the histogram of 10 M pairs drawn
from N(200, 20) occupies about 200 bins, the model's weights for (200, 20) are non-zero on 970 (down to the
denormals), and a histogram with a count in each of those 970 bins is timed as well, so that the two sources of p
are compared at equal work.  Against the parent commit: build its libseekmer_hip.so, name it in SKM_HIP_LIB (the
library is chosen when the package loads) and run this script with --histogram-only --label parent before and
after a run on this commit's library.  Give every invocation a `timeout` of its own, as for the other scripts."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ('skm_effective_lengths_weights', 'skm_mapper_set_length_weights', 'skm_sample_set_set_length_weights')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--transcripts', type=int, default=190_402)
    ap.add_argument('--histogram-only', action='store_true', help='time skm_effective_lengths alone (a library without the model)')
    ap.add_argument('--label', default='this')
    args = ap.parse_args()

    from seekmer_amd import _native, mapper
    if args.histogram_only:
        for name in NEW_SYMBOLS:
            _native.HIP_SYMBOLS.pop(name, None)
    rng = np.random.default_rng(1)
    lengths = np.ascontiguousarray(np.clip(rng.lognormal(7.2, 0.8, args.transcripts), 30, 100_000).round())
    weights = mapper.fragment_length_weights(200, 20)
    observed = np.bincount(np.clip(rng.normal(200, 20, 10_000_000).round().astype(np.int64), 1, 1999), minlength=2000)
    same_bins = (weights > 0).astype(np.int64)

    def histogram(fld):
        return lambda: mapper._effective_lengths(lengths, fld, 0)

    forms = [('histogram, observed', int((observed > 0).sum()), histogram(observed)),
             ('histogram, the model\'s bins', int(same_bins.sum()), histogram(same_bins))]
    if not args.histogram_only:
        forms.append(('weights, model (200, 20)', int((weights > 0).sum()), lambda: mapper._effective_lengths_weights(lengths, weights, 0)))
    times = {name: [] for name, _, _ in forms}
    for rep in range(args.warmup + args.reps):
        for name, _, call in forms:              # (alternating: what else the machine does falls on all forms alike)
            t0 = time.perf_counter()
            call()                               # (synchronous: the lengths are home when it returns)
            if rep >= args.warmup:
                times[name].append(1e3 * (time.perf_counter() - t0))
    for name, bins, _ in forms:
        ms = sorted(times[name])
        print(json.dumps({'library': args.label, 'form': name, 'transcripts': args.transcripts, 'bins': bins, 'reps': args.reps,
                          'ms_min': round(ms[0], 4), 'ms_median': round(statistics.median(ms), 4),
                          'ms_p90': round(ms[int(0.9 * (len(ms) - 1))], 4)}), flush=True)


if __name__ == '__main__':
    main()
