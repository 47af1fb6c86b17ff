#!/usr/bin/env python3
"""What --bias costs: the mapping stage with hexamer counting on and off on BASELINE configs[1]'s workload
(10 M 2x100 synthetic pairs, resident in HBM, `reset` between steps), the one-off transcript pool of the
benchmark index (190 k transcripts), one skm_bias_correct call, and the second EM.  One JSON line each.

    python scripts/bias_cost.py [--steps K] [--warmup W] [--pairs N] [--index-cache PATH]

The two mapping modes alternate, `--rounds` times, in one process; a mapper that does not count runs exactly
the launches of the parent commit.  Under `rocprofv3 --kernel-trace --stats -- python scripts/bias_cost.py
...` the stats give bias_observed_kernel's time beside map_units_kernel's."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=10_000_000)
    ap.add_argument('--read-len', type=int, default=100)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--index-cache', default='')
    args = ap.parse_args()

    import bench
    from seekmer_amd import _native, infer, mapper, synth
    hip = _native.hip()
    ids, pool, tx_offsets = synth.transcriptome(args.seed, args.genes)
    path = args.index_cache or bench.index_cache_path(args.seed, args.genes)
    index = bench.bench_index(ids, pool, tx_offsets, path, 0, 1, None)
    handle = index.device_handle(0)
    bases, offsets = synth.reads(args.seed, pool, tx_offsets, 0, args.pairs, args.read_len, True)
    d_bases, d_offsets = ctypes.c_void_p(), ctypes.c_void_p()
    _native.check(hip.skm_device_malloc(0, bases.size, ctypes.byref(d_bases)))
    _native.check(hip.skm_device_malloc(0, offsets.size * 8, ctypes.byref(d_offsets)))
    _native.check(hip.skm_device_upload(0, d_bases, bases.ctypes.data, bases.size))
    _native.check(hip.skm_device_upload(0, d_offsets, offsets.ctypes.data, offsets.size * 8))

    def timed(call, steps, warmup):
        for _ in range(warmup):
            call()
        _native.check(hip.skm_device_synchronize(0))
        t0 = time.perf_counter()
        for _ in range(steps):
            call()
        _native.check(hip.skm_device_synchronize(0))
        return 1e3 * (time.perf_counter() - t0) / steps

    try:
        results = {False: mapper.MapResult(index), True: mapper.MapResult(index, bias=True)}
        for round_ in range(args.rounds):
            for counting in (False, True):
                result = results[counting]

                def step():
                    result.reset()
                    result.map_resident(d_bases, d_offsets, args.pairs, True, args.read_len)

                ms = timed(step, args.steps, args.warmup if round_ == 0 else 1)
                print(json.dumps({'stage': 'mapping', 'counting': counting, 'round': round_, 'pairs': args.pairs,
                                  'steps': args.steps, 'ms_per_step': round(ms, 3)}), flush=True)
        result = results[True]
        observed = result.bias_observed()
        summary = result.summarize()
        del results[False]

        lengths = np.ascontiguousarray(index.transcripts['length'], dtype='f8')
        # what skm_index_create keeps on the host for the pool until it is built: 8 bytes a target row, 24 a contig
        print(json.dumps({'stage': 'host rows kept by the index handle', 'targets': int(index.targets.size),
                          'contigs': int(index.contigs.size),
                          'bytes': int(8 * index.targets.size + 24 * index.contigs.size)}), flush=True)
        t0 = time.perf_counter()
        _native.check(hip.skm_index_build_transcripts(handle, _native.ptr(lengths, _native.c_f64p), lengths.size))
        print(json.dumps({'stage': 'transcript pool (once per index)', 'transcripts': int(lengths.size),
                          'bases': int(lengths.sum()), 'ms': round(1e3 * (time.perf_counter() - t0), 3)}), flush=True)

        first, first_steps = infer.quantify(summary, return_iters=True)
        ms = timed(lambda: infer.quantify(summary), 3, 0)
        print(json.dumps({'stage': 'first EM (quantify)', 'em_steps': first_steps, 'ms': round(ms, 3)}), flush=True)
        ms = timed(lambda: infer.bias_correct(index, summary, first, observed, None), 10, 2)
        corrected, b, _ = infer.bias_correct(index, summary, first, observed, None)
        print(json.dumps({'stage': 'skm_bias_correct', 'observed': int(observed.sum()), 'expressed': int((first > 0).sum()),
                          'b_min': float(b.min()), 'b_max': float(b.max()), 'ms': round(ms, 3)}), flush=True)
        second_summary = mapper.SummarizedResult(
            summary.aligned, summary.unaligned, summary.total, summary.class_map, summary.class_count,
            summary.fragment_length_frequencies, corrected, class_offsets=summary.class_offsets,
            class_targets=summary.class_targets)
        _, second_steps = infer.quantify(second_summary, x0=first, return_iters=True)
        ms = timed(lambda: infer.quantify(second_summary, x0=first), 3, 0)
        print(json.dumps({'stage': 'second EM (quantify from the first result)', 'em_steps': second_steps,
                          'ms': round(ms, 3)}), flush=True)
    finally:
        hip.skm_device_free(0, d_bases)
        hip.skm_device_free(0, d_offsets)


if __name__ == '__main__':
    main()
