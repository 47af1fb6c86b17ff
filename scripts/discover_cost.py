"""What `seekmer_amd infer-many --discover-cells` costs: N cells of P read pairs each (and A ambient pairs under random
barcodes) in ONE pooled pair of FASTQ files plus a barcode file -- the files of scripts/demux_rate.py: the cells'
pairs interleaved by a seeded permutation, 85 % of the barcodes exact, 10 % with one substitution, 5 % unreadable --
quantified
    (discover)  by `infer-many --discover-cells N --barcode-length L`, and
    (whitelist) by `infer-many --barcodes` on the barcodes.discovered.txt that the first form wrote: the route that
                needs no discovery, the baseline,
with SKM_TRACE_INFER's phase times of both printed and every table compared byte for byte where both forms ran.
The census pass is also timed on its own, in a process that does nothing else: mapper.discover_barcodes over the
barcode file, twice (the second time with the code objects loaded and the pool warm), units/s and distinct keys.
    python3 scripts/discover_cost.py --cells 64 --pairs 20000 --genes 100
    python3 scripts/discover_cost.py --cells 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
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
ap.add_argument('--ambient', type=int, default=None, help='pairs under random barcodes (default: 2 %% of the cells\' pairs)')
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--barcode-len', type=int, default=16)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--only', choices=('discover', 'whitelist'), default=None,
                help='whitelist: the list of an earlier --only discover in the same --work folder')
ap.add_argument('--cache', default='', help='keep the index in this file between invocations')
ap.add_argument('--step-limit', type=int, default=300, help='seconds one child process may take')
ap.add_argument('--work', default='', help='folder for the files (default: a temporary one)')
ap.add_argument('--census-of', default='', help=argparse.SUPPRESS)        # the child that times the census pass alone
args = ap.parse_args()


def census_child():
    """the census pass alone, in this process: the barcode file -> the picked barcodes, twice"""
    from seekmer_amd import common, mapper
    for attempt in ('first', 'second'):
        t0 = time.perf_counter()
        picked, counts, info = mapper.discover_barcodes(common.PackedReadFeeder([args.census_of], paired=False, threads=args.jobs),
                                                        args.barcode_len, args.cells)
        dt = time.perf_counter() - t0
        print('census pass alone (%s time): %.1f ms, %.1f M units/s: %d units, %d counted, %d distinct keys, threshold %d, '
              '%d candidates, %d dropped, %d picked' % (attempt, dt * 1e3, info['units'] / dt / 1e6, info['units'], info['counted'],
                                                        info['distinct'], info['threshold'], info['candidates'], info['dropped'],
                                                        info['picked']), flush=True)


def step(name, command, keep_stdout=False):
    """One child process under its own time limit; the first failure ends the script.  Returns (seconds, lines)."""
    t0 = time.perf_counter()
    done = subprocess.run(['timeout', '-k', '10', str(args.step_limit), sys.executable] + command, cwd=ROOT,
                          env=dict(os.environ, SKM_TRACE_INFER='1'), stdout=subprocess.PIPE if keep_stdout else subprocess.DEVNULL,
                          stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    text = done.stderr.decode(errors='replace')
    if done.returncode != 0:
        sys.stderr.write(text[-4000:])
        sys.exit('%s ended with status %d after %.1f s: nothing more is started' % (name, done.returncode, dt))
    if keep_stdout:
        return dt, done.stdout.decode(errors='replace').splitlines()
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
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix='skm_discover_'))
    work.mkdir(parents=True, exist_ok=True)
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index_path = pathlib.Path(args.cache) if args.cache else work / 'index.npz'
    if not index_path.exists():
        index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    ambient = args.cells * args.pairs // 50 if args.ambient is None else args.ambient
    if not (work / 'barcodes.fastq').exists():
        rng = numpy.random.default_rng(1)
        letters = numpy.frombuffer(b'ACGT', dtype=numpy.uint8)
        while True:    # barcodes at Hamming distance >= 3 from each other: one substitution never reaches another cell
            cells = numpy.unique(letters[rng.integers(0, 4, size=(2 * args.cells, args.barcode_len))], axis=0)
            cells = cells[rng.permutation(len(cells))[:args.cells]]
            distance = (cells[:, None, :] != cells[None, :, :]).sum(axis=2)
            if len(cells) == args.cells and (distance + 99 * numpy.eye(args.cells, dtype=int)).min() >= 3:
                break
        mates = [[], []]
        for c in range(args.cells + 1):                  # (the last "cell" is the ambient pairs)
            n = args.pairs if c < args.cells else ambient
            if n:
                bases, _ = synth.reads(100 + c % 2, pool, tx_offsets, c * args.pairs, n, args.read_len, True)
                pairs = bases[:-1].reshape(n, 2, args.read_len)
                mates[0].append(pairs[:, 0]); mates[1].append(pairs[:, 1])
        n_units = args.cells * args.pairs + ambient
        shuffle = rng.permutation(n_units)
        truth = shuffle // args.pairs
        mates = [numpy.concatenate(mate)[shuffle] for mate in mates]
        for mate in (0, 1):
            write_fastq(work / ('pool_%d.fastq' % (mate + 1)), mates[mate], args.read_len)
        barcodes = numpy.concatenate([cells, cells[:1]])[numpy.minimum(truth, args.cells)].copy()
        is_ambient = truth >= args.cells
        barcodes[is_ambient] = letters[rng.integers(0, 4, size=(int(is_ambient.sum()), args.barcode_len))]
        chance = rng.random(n_units)
        one = numpy.flatnonzero((chance >= 0.85) & (chance < 0.95))
        place = rng.integers(0, args.barcode_len, size=one.size)
        barcodes[one, place] = letters[(numpy.searchsorted(letters, barcodes[one, place]) + rng.integers(1, 4, size=one.size)) % 4]
        barcodes[chance >= 0.95, :2] = ord('N')           # two N: unreadable, whatever the rest says
        write_fastq(work / 'barcodes.fastq', barcodes, args.barcode_len)
    print('%d cells x %d pairs of 2 x %d bases and %d ambient pairs on %d transcripts, barcodes of %d bases; index of %.0f MiB' %
          (args.cells, args.pairs, args.read_len, ambient, len(ids), args.barcode_len, index_path.stat().st_size / 2 ** 20), flush=True)
    pooled = [str(work / 'pool_1.fastq'), str(work / 'pool_2.fastq'), '--barcode-file', str(work / 'barcodes.fastq'), '-j', str(args.jobs)]
    took = {}
    if args.only in (None, 'discover'):
        _, lines = step('the census pass alone',
                        [os.path.abspath(__file__), '--census-of', str(work / 'barcodes.fastq'), '--cells', str(args.cells),
                         '--barcode-len', str(args.barcode_len), '--jobs', str(args.jobs)], keep_stdout=True)
        print('\n'.join(lines), flush=True)
        took['discover'], trace = step('infer-many --discover-cells',
                                       ['-m', 'seekmer_amd', 'infer-many', str(index_path), str(work / 'out_discover'), *pooled,
                                        '--discover-cells', str(args.cells), '--barcode-length', str(args.barcode_len)])
        print('infer-many --discover-cells, pooled files:   %.2f s' % took['discover'], flush=True)
        print('\n'.join('    ' + line for line in trace), flush=True)
    if args.only in (None, 'whitelist'):
        took['whitelist'], trace = step('infer-many --barcodes',
                                        ['-m', 'seekmer_amd', 'infer-many', str(index_path), str(work / 'out_whitelist'), *pooled,
                                         '--barcodes', str(work / 'out_discover' / 'barcodes.discovered.txt')])
        print('infer-many --barcodes on the discovered list:   %.2f s' % took['whitelist'], flush=True)
        print('\n'.join('    ' + line for line in trace), flush=True)
    if len(took) == 2:
        names = [line.split('\t')[0] for line in (work / 'out_discover' / 'samples.tsv').read_text().splitlines()]
        for name in names + ['samples.tsv', 'barcodes.tsv']:
            path = pathlib.Path(name) / 'abundance.tsv' if name in names else pathlib.Path(name)
            one, other = [(work / form / path).read_bytes() for form in ('out_discover', 'out_whitelist')]
            assert one == other, '%s differs between the two forms' % path
        print('all %d abundance.tsv, samples.tsv and barcodes.tsv agree byte for byte between the two forms' % len(names), flush=True)


if __name__ == '__main__':
    if args.census_of:
        census_child()
    else:
        main()
