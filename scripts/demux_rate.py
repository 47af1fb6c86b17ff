"""What `seekmer_amd infer-many --barcodes` costs: N cells of P read pairs each, quantified
    (demux) by one `infer-many --barcodes` on ONE pooled pair of FASTQ files plus a barcode file, the cells' pairs
            interleaved by a seeded permutation, 85 % of the barcodes exact, 10 % with one substitution, 5 % unreadable,
    (files) by `infer-many` on the N per-cell FASTQ pairs of the assigned reads (what a CPU demultiplexer would have
            had to write first; writing them is NOT part of the time),
with SKM_TRACE_INFER's phase times of both printed, and every cell's abundance.tsv compared byte for byte where
both forms ran.
    python3 scripts/demux_rate.py --cells 64 --pairs 20000 --genes 100
    python3 scripts/demux_rate.py --cells 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
Wall time of whole processes.  Making the index and the files happens before any clock starts.  Every step that
uses the GPU is a child process under a time limit of its own (`timeout -k 10 SECONDS ...`); the script stops at
the first step that fails and starts nothing again.
"""
import argparse
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--cells', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--barcode-len', type=int, default=16)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--only', choices=('demux', 'files'), default=None)
ap.add_argument('--cache', default='', help='keep the index in this file between invocations')
ap.add_argument('--step-limit', type=int, default=300, help='seconds one child process may take')
ap.add_argument('--work', default='', help='folder for the files (default: a temporary one)')
args = ap.parse_args()


def step(name, arguments):
    """One child process under its own time limit; the first failure ends the script.  Returns (seconds, trace)."""
    t0 = time.perf_counter()
    done = subprocess.run(['timeout', '-k', '10', str(args.step_limit), sys.executable, '-m', 'seekmer_amd'] + arguments,
                          cwd=ROOT, env=dict(os.environ, SKM_TRACE_INFER='1'), stdout=subprocess.DEVNULL,
                          stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    text = done.stderr.decode(errors='replace')
    if done.returncode != 0:
        sys.stderr.write(text[-4000:])
        sys.exit('%s ended with status %d after %.1f s: nothing more is started' % (name, done.returncode, dt))
    return dt, [line for line in text.splitlines() if line.startswith('[run_many]') or 'Barcodes of' in line]


def write_fastq(path, reads, read_len):
    """reads uint8[n, read_len] as FASTQ text (numpy only: a record is a fixed-width row)"""
    n = reads.shape[0]
    names = numpy.char.zfill(numpy.arange(n).astype('S10'), 10).view(numpy.uint8).reshape(n, 10)
    record = numpy.empty((n, 2 + 10 + 1 + read_len + 3 + read_len + 1), dtype=numpy.uint8)
    record[:, 0:2] = numpy.frombuffer(b'@r', dtype=numpy.uint8)
    record[:, 2:12] = names
    record[:, 12] = 10
    record[:, 13:13 + read_len] = reads
    record[:, 13 + read_len:16 + read_len] = numpy.frombuffer(b'\n+\n', dtype=numpy.uint8)
    record[:, 16 + read_len:16 + 2 * read_len] = ord('I')
    record[:, -1] = 10
    record.tofile(path)


def main():
    from seekmer_amd import index_builder, synth            # (host code only: this process never opens the GPU)
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix='skm_demux_'))
    work.mkdir(parents=True, exist_ok=True)
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index_path = pathlib.Path(args.cache) if args.cache else work / 'index.npz'
    if not index_path.exists():
        index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    rng = numpy.random.default_rng(1)
    letters = numpy.frombuffer(b'ACGT', dtype=numpy.uint8)
    while True:        # barcodes at Hamming distance >= 3 from each other: one substitution never reaches another cell
        whitelist = numpy.unique(letters[rng.integers(0, 4, size=(2 * args.cells, args.barcode_len))], axis=0)
        whitelist = whitelist[rng.permutation(len(whitelist))[:args.cells]]
        distance = (whitelist[:, None, :] != whitelist[None, :, :]).sum(axis=2)
        if len(whitelist) == args.cells and (distance + 99 * numpy.eye(args.cells, dtype=int)).min() >= 3:
            break
    names = ['c%04d' % c for c in range(args.cells)]
    (work / 'whitelist.tsv').write_text(''.join('%s\t%s\n' % (w.tobytes().decode(), n) for w, n in zip(whitelist, names)))
    mates = [[], []]
    for c in range(args.cells):
        bases, _ = synth.reads(100 + c % 2, pool, tx_offsets, c * args.pairs, args.pairs, args.read_len, True)
        pairs = bases[:-1].reshape(args.pairs, 2, args.read_len)
        mates[0].append(pairs[:, 0]); mates[1].append(pairs[:, 1])
    n_units = args.cells * args.pairs
    shuffle = rng.permutation(n_units)
    truth = shuffle // args.pairs
    mates = [numpy.concatenate(mate)[shuffle] for mate in mates]
    for mate in (0, 1):
        write_fastq(work / ('pool_%d.fastq' % (mate + 1)), mates[mate], args.read_len)
    barcodes = whitelist[truth].copy()
    chance = rng.random(n_units)
    one = numpy.flatnonzero((chance >= 0.85) & (chance < 0.95))
    place = rng.integers(0, args.barcode_len, size=one.size)
    barcodes[one, place] = letters[(numpy.searchsorted(letters, barcodes[one, place]) + rng.integers(1, 4, size=one.size)) % 4]
    unreadable = chance >= 0.95                       # two N: no cell, whatever the rest says
    barcodes[unreadable, :2] = ord('N')
    write_fastq(work / 'barcodes.fastq', barcodes, args.barcode_len)
    # the per-cell files a demultiplexer would have written: every cell's assigned pairs in pooled order
    files = []
    for c in range(args.cells):
        units = numpy.flatnonzero((truth == c) & ~unreadable)
        for mate in (0, 1):
            files.append(work / ('%s_%d.fastq' % (names[c], mate + 1)))
            write_fastq(files[-1], mates[mate][units], args.read_len)
    print('%d cells x %d pairs of 2 x %d bases on %d transcripts, barcodes of %d bases; index of %.0f MiB' %
          (args.cells, args.pairs, args.read_len, len(ids), args.barcode_len, index_path.stat().st_size / 2 ** 20), flush=True)
    took = {}
    if args.only in (None, 'files'):
        took['files'], trace = step('infer-many on per-cell files',
                                    ['infer-many', str(index_path), str(work / 'out_files'), *map(str, files), '-j', str(args.jobs),
                                     '--names', ','.join(names)])
        print('infer-many, %d per-cell file pairs:   %.2f s' % (args.cells, took['files']), flush=True)
        print('\n'.join('    ' + line for line in trace), flush=True)
    if args.only in (None, 'demux'):
        took['demux'], trace = step('infer-many --barcodes',
                                    ['infer-many', str(index_path), str(work / 'out_demux'), str(work / 'pool_1.fastq'),
                                     str(work / 'pool_2.fastq'), '--barcodes', str(work / 'whitelist.tsv'), '--barcode-file',
                                     str(work / 'barcodes.fastq'), '-j', str(args.jobs)])
        print('infer-many --barcodes, pooled files:   %.2f s' % took['demux'], flush=True)
        print('\n'.join('    ' + line for line in trace), flush=True)
    if len(took) == 2:
        for name in names:
            one, other = [(work / form / name / 'abundance.tsv').read_bytes() for form in ('out_files', 'out_demux')]
            assert one == other, 'abundance.tsv of %s differs between the two forms' % name
        assert (work / 'out_files' / 'samples.tsv').read_bytes() == (work / 'out_demux' / 'samples.tsv').read_bytes()
        print('all %d abundance.tsv and samples.tsv agree byte for byte between the two forms' % args.cells, flush=True)


if __name__ == '__main__':
    main()
