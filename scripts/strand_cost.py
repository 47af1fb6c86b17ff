#!/usr/bin/env python3
"""What a strand-specific library costs the mapper: BASELINE configs[1]'s workload (10 M 2x100
synthetic pairs, resident in HBM, `reset` between steps) mapped unstranded and in mode fr, ms per
step of each, one JSON line per mode.

    python scripts/strand_cost.py [--steps K] [--warmup W] [--pairs N] [--index-cache PATH]

The synthetic reads are unstranded, so mode fr empties about half of the units; the strand filter
visits every record either way.  Under `rocprofv3 --kernel-trace --stats -- python
scripts/strand_cost.py ...` the stats give strand_filter_kernel's time beside class_insert_kernel's."""
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
    ap.add_argument('--pairs', type=int, default=10_000_000)
    ap.add_argument('--read-len', type=int, default=100)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--index-cache', default='')
    args = ap.parse_args()

    import bench
    from seekmer_amd import _native, mapper, synth
    hip = _native.hip()
    ids, pool, tx_offsets = synth.transcriptome(args.seed, args.genes)
    path = args.index_cache or bench.index_cache_path(args.seed, args.genes)
    index = bench.bench_index(ids, pool, tx_offsets, path, 0, 1, None)
    index.device_handle(0)
    bases, offsets = synth.reads(args.seed, pool, tx_offsets, 0, args.pairs, args.read_len, True)
    d_bases, d_offsets = ctypes.c_void_p(), ctypes.c_void_p()
    _native.check(hip.skm_device_malloc(0, bases.size, ctypes.byref(d_bases)))
    _native.check(hip.skm_device_malloc(0, offsets.size * 8, ctypes.byref(d_offsets)))
    _native.check(hip.skm_device_upload(0, d_bases, bases.ctypes.data, bases.size))
    _native.check(hip.skm_device_upload(0, d_offsets, offsets.ctypes.data, offsets.size * 8))
    try:
        for strand in (None, 'fr'):
            result = mapper.MapResult(index, strand=strand)

            def step():
                result.reset()
                result.map_resident(d_bases, d_offsets, args.pairs, True, args.read_len)

            for _ in range(args.warmup):
                step()
            _native.check(hip.skm_device_synchronize(0))
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            _native.check(hip.skm_device_synchronize(0))
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            classes, _, unaligned, units = result.sizes()
            print(json.dumps({'strand': strand or 'none', 'pairs': args.pairs, 'steps': args.steps,
                              'ms_per_step': round(ms, 3), 'classes': classes, 'unaligned': unaligned,
                              'units': units}), flush=True)
            del result
    finally:
        hip.skm_device_free(0, d_bases)
        hip.skm_device_free(0, d_offsets)


if __name__ == '__main__':
    main()
