#!/usr/bin/env python
"""Where a chunk of the tile EM (skm_em.hip: em_local_chunk_kernel) spends its time: the kernel run for
a FIXED number of steps (skm_quant_em's fixed_iters: the stopping rule is not consulted) on the
benchmark's class table -- 20 000 synthetic genes, 10 M pairs of 2 x 100 -- by the product library and by
the two timing builds that leave a phase out:

    scripts/build_variant.sh noclass "-DSKM_EM_TILE_EXPERIMENT=1" skm_em.hip      # no class phase
    scripts/build_variant.sh norow   "-DSKM_EM_TILE_EXPERIMENT=2" skm_em.hip      # no row phase
    python scripts/em_tile_phase_cost.py [--index-cache FILE] [--steps 160] [--timeout 600]

Every build runs in a process of its own under `timeout -k 10`; after a run that fails none is started.
The first run maps the reads and keeps the class table in a temporary file for the other two.  The
abundances the timing builds compute are wrong by design and are compared with nothing.  Needs a GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUILDS = (('whole kernel', 'libseekmer_hip.so'), ('without the class phase', 'libseekmer_hip_noclass.so'),
          ('without the row phase', 'libseekmer_hip_norow.so'))
CHUNK = 16                 # EM_CHUNK_MAX: steps of one launch


def class_table(args, path):
    """(n_tx, offsets, targets, counts, lengths) of the benchmark's table: mapped here and stored at `path`, or loaded."""
    if os.path.exists(path):
        with np.load(path) as f:
            return int(f['n_tx']), f['offsets'], f['targets'], f['counts'], f['lengths']
    import ctypes
    from seekmer_amd import _native, common, index_builder, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(args.seed, args.genes)
    if args.index_cache and os.path.exists(args.index_cache):
        index = common.KMerIndex.load(args.index_cache)
    else:
        index = index_builder.build_pooled(ids, pool, tx_offsets)
        if args.index_cache:
            index.save(args.index_cache)
    bases, offsets = synth.reads(args.seed, pool, tx_offsets, 0, args.pairs, 100, True)
    # (the reads to HBM and one launch over them, as bench.py maps its resident batch)
    hip = _native.hip()
    d_bases, d_offsets = ctypes.c_void_p(), ctypes.c_void_p()
    _native.check(hip.skm_device_malloc(0, bases.size, ctypes.byref(d_bases)))
    _native.check(hip.skm_device_malloc(0, offsets.size * 8, ctypes.byref(d_offsets)))
    _native.check(hip.skm_device_upload(0, d_bases, bases.ctypes.data, bases.size))
    _native.check(hip.skm_device_upload(0, d_offsets, offsets.ctypes.data, offsets.size * 8))
    result = mapper.MapResult(index, device=0)
    result.map_resident(d_bases, d_offsets, args.pairs, True, 100)
    class_offsets, class_targets, counts, _, _ = result.export()
    _native.check(hip.skm_device_free(0, d_bases))
    _native.check(hip.skm_device_free(0, d_offsets))
    lengths = np.diff(tx_offsets).astype('f8')
    np.savez(path, n_tx=len(ids), offsets=class_offsets, targets=class_targets, counts=counts, lengths=lengths)
    return len(ids), class_offsets, class_targets, counts, lengths


def child(args):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, lengths = class_table(args, args.child)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, np.asarray(counts, dtype='f8'))
    try:
        info, _, tile, class_tile = quant.components()
        x0 = 1.0 / lengths
        x0 /= x0.sum()
        quant.em(x0, lengths, fixed_iters=CHUNK)                     # (warm-up: first launches, allocations)

        def fastest():
            best = None
            for _ in range(args.repeats):
                before = quant.timing()
                _, steps = quant.em(x0, lengths, fixed_iters=args.steps)
                after = quant.timing()
                assert steps == args.steps
                us = (after['em_ns'] - before['em_ns']) * 1e-3 / (args.steps / CHUNK)
                best = us if best is None else min(best, us)
            return best

        best = fastest()
        n_tiles = info['tiles']
        lens = np.diff(offsets)
        inside, cls_inside = tile < n_tx, class_tile < n_tx
        if args.orders:
            # the launch orders of the tiles (SKM_EM_TILE_ORDER is looked up at every run) and the sizes they sort
            by_order = {'largest first': best}
            for form in ('identity', 'reverse'):
                os.environ['SKM_EM_TILE_ORDER'] = form
                by_order[form] = fastest()
            del os.environ['SKM_EM_TILE_ORDER']
            pairs = np.bincount(class_tile[cls_inside], weights=lens[cls_inside], minlength=n_tiles)
            print(json.dumps({'us_per_chunk_by_order': by_order, 'tiles': n_tiles, 'capacity': info['capacity'],
                              'tiles_below_half_fill': int((pairs < info['capacity'][0] / 2).sum()),
                              'pairs_quartiles': [float(q) for q in np.percentile(pairs, (0, 25, 50, 75, 100))]}), flush=True)
            return
        fill = [float(np.bincount(class_tile[cls_inside], weights=lens[cls_inside], minlength=n_tiles).mean()),
                float(np.bincount(class_tile[cls_inside], minlength=n_tiles).mean()),
                float(np.bincount(tile[inside], minlength=n_tiles).mean())] if n_tiles else [0.0, 0.0, 0.0]
        print(json.dumps({'us_per_chunk': best, 'tiles': n_tiles, 'oversize': info['oversize'], 'capacity': info['capacity'],
                          'segment': info.get('segment', 0), 'em_uses_tiles': info['em_uses_tiles'], 'mean_fill': fill,
                          'classes': int(offsets.size - 1), 'pairs': int(targets.size), 'transcripts': n_tx}), flush=True)
    finally:
        quant.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--pairs', type=int, default=10_000_000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--steps', type=int, default=160, help='EM steps per timed run (a multiple of %d)' % CHUNK)
    ap.add_argument('--repeats', type=int, default=3, help='timed runs per build; the fastest is reported')
    ap.add_argument('--timeout', type=int, default=600, help='seconds per build')
    ap.add_argument('--index-cache', default='', help='load the index from this file / store it there')
    ap.add_argument('--orders', action='store_true',
                    help='the product library alone: the chunk under the three launch orders of the tiles '
                         '(SKM_EM_TILE_ORDER) and the distribution of the tiles\' pair counts, one JSON line')
    ap.add_argument('--child', default='', help='(internal) measure the library in SKM_HIP_LIB on the table in this file')
    args = ap.parse_args()
    if args.steps % CHUNK:
        ap.error('--steps must be a multiple of %d' % CHUNK)
    if args.child:
        return child(args)
    folder = tempfile.mkdtemp(prefix='skm_phase_')
    table = os.path.join(folder, 'table.npz')
    rows = []
    try:
        for name, lib in BUILDS[:1] if args.orders else BUILDS:
            path = os.path.join(ROOT, 'seekmer_amd', lib)
            if not os.path.exists(path):
                raise SystemExit('%s is missing: build it first (see the top of this file)' % path)
            env = dict(os.environ, SKM_HIP_LIB=path)
            cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--child', table,
                   '--genes', str(args.genes), '--pairs', str(args.pairs), '--seed', str(args.seed), '--steps', str(args.steps),
                   '--repeats', str(args.repeats)] + (['--index-cache', args.index_cache] if args.index_cache else [])
            cmd += ['--orders'] if args.orders else []
            t0 = time.perf_counter()
            done = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
            if done.returncode:
                raise SystemExit('%s: exit status %d after %.0f s; nothing further is run'
                                 % (name, done.returncode, time.perf_counter() - t0))
            if args.orders:
                print(done.stdout.decode().strip().splitlines()[-1])
                return
            rows.append((name, json.loads(done.stdout.decode().strip().splitlines()[-1])))
    finally:
        for f in (table,):
            if os.path.exists(f):
                os.unlink(f)
        os.rmdir(folder)
    first = rows[0][1]
    print('%d transcripts, %d classes, %d pairs; packing run %d ids, capacity %s (pairs, classes, transcripts)'
          % (first['transcripts'], first['classes'], first['pairs'], first['segment'], tuple(first['capacity'])))
    print('%d tiles, %d components above the capacity; mean fill %.0f pairs (%.2f), %.0f classes (%.2f), %.0f transcripts (%.2f)'
          % (first['tiles'], first['oversize'], first['mean_fill'][0], first['mean_fill'][0] / first['capacity'][0],
             first['mean_fill'][1], first['mean_fill'][1] / first['capacity'][1],
             first['mean_fill'][2], first['mean_fill'][2] / first['capacity'][2]))
    print('us per chunk of %d steps (EM kernel time of %d steps, the judging launch of every chunk included; fastest of %d):'
          % (CHUNK, args.steps, args.repeats))
    for name, row in rows:
        assert row['em_uses_tiles'] and row['tiles'] == first['tiles']
        print('  %-26s %8.1f' % (name, row['us_per_chunk']))


if __name__ == '__main__':
    main()
