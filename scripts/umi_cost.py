"""What `--umi-length` costs `seekmer_amd infer-many --barcodes`: N cells of P read pairs each in ONE pooled pair of
FASTQ files plus a barcode file (barcode, then a UMI of 12 bases), in which every cell's pairs are copies of P / C
molecules drawn at random, so that a molecule appears C times on average; the cells interleaved by a seeded
permutation, 85 % of the barcodes exact, 10 % with one substitution, 5 % unreadable.  The same files are quantified
    (plain) by `infer-many --barcodes`, every read counted, and
    (umi)   by `infer-many --barcodes --umi-start L --umi-length 12`, duplicates collapsed on the GPU,
    (near)  with --mismatches 1 also by the same command with `--umi-mismatches 1`: every surviving unit then looks up
            its 36 one-substitution neighbours in the molecule set (with --only umi this form alone),
with SKM_TRACE_INFER's phase times of both printed: "demultiplexing" (which holds the UMI windows, the UMIs' way
through the chunks and the set's launches that ran meanwhile) and "mapping (set)" (what was left of the set's
mapping, and its summaries) separately.  The yardstick for the option's cost is the same command without it.
    python3 scripts/umi_cost.py --cells 64 --pairs 20000 --genes 100 --copies 2
    python3 scripts/umi_cost.py --cells 64 --pairs 50000 --genes 20000 --copies 2 --cache /tmp/skm_idx.npz
Wall time of whole processes.  Making the index and the files happens before any clock starts.  Every step that
uses the GPU is a child process under a time limit of its own (`timeout -k 10 SECONDS ...`); the script stops at
the first step that fails and starts nothing again.
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UMI_LENGTH = 12

ap = argparse.ArgumentParser()
ap.add_argument('--cells', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--copies', type=float, default=2.0, help='copies of a molecule, on average')
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--barcode-len', type=int, default=16)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--only', choices=('umi', 'plain'), default=None)
ap.add_argument('--mismatches', type=int, choices=(0, 1), default=0,
                help='1: also run the UMI form with --umi-mismatches 1 (with --only umi: that form alone)')
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
    return dt, [line for line in text.splitlines() if line.startswith('[run_many]') or 'Barcodes of' in line or 'UMIs of' in line]


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
    if args.copies < 1:
        sys.exit('--copies must be 1 or more')
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix='skm_umi_'))
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
    molecules = max(1, int(round(args.pairs / args.copies)))
    mates, umis = [[], []], []
    for c in range(args.cells):
        bases, _ = synth.reads(100 + c % 2, pool, tx_offsets, c * molecules, molecules, args.read_len, True)
        pairs = bases[:-1].reshape(molecules, 2, args.read_len)
        drawn = rng.integers(0, molecules, size=args.pairs)              # the molecule every unit of the cell copies
        mates[0].append(pairs[drawn, 0]); mates[1].append(pairs[drawn, 1])
        umis.append(letters[rng.integers(0, 4, size=(molecules, UMI_LENGTH))][drawn])
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
    barcodes[chance >= 0.95, :2] = ord('N')           # two N: no cell, whatever the rest says
    write_fastq(work / 'barcodes.fastq', numpy.concatenate([barcodes, numpy.concatenate(umis)[shuffle]], axis=1),
                args.barcode_len + UMI_LENGTH)
    print('%d cells x %d pairs of 2 x %d bases (%d molecules a cell, %.2f copies each on average) on %d transcripts, barcodes '
          'of %d bases + UMIs of %d; index of %.0f MiB' % (args.cells, args.pairs, args.read_len, molecules, args.pairs / molecules,
                                                           len(ids), args.barcode_len, UMI_LENGTH, index_path.stat().st_size / 2 ** 20),
          flush=True)
    pooled = ['infer-many', str(index_path), None, str(work / 'pool_1.fastq'), str(work / 'pool_2.fastq'), '--barcodes',
              str(work / 'whitelist.tsv'), '--barcode-file', str(work / 'barcodes.fastq'), '-j', str(args.jobs)]
    if args.only in (None, 'plain'):
        pooled[2] = str(work / 'out_plain')
        took, trace = step('infer-many --barcodes', pooled)
        print('infer-many --barcodes, every read counted:   %.2f s' % took, flush=True)
        print('\n'.join('    ' + line for line in trace), flush=True)
    forms = [args.mismatches]                    # the UMI forms to run: --umi-mismatches 0 and / or 1
    if args.only == 'plain':
        forms = []
    if args.only is None and args.mismatches:
        forms = [0, 1]
    for mismatches in forms:
        out = work / ('out_near' if mismatches else 'out_umi')
        pooled[2] = str(out)
        extra = ['--umi-mismatches', '1'] if mismatches else []
        took, trace = step('infer-many --barcodes --umi-length' + ' --umi-mismatches 1' * mismatches,
                           pooled + ['--umi-start', str(args.barcode_len), '--umi-length', str(UMI_LENGTH)] + extra)
        print('infer-many --barcodes --umi-length %d%s:      %.2f s' % (UMI_LENGTH, ' --umi-mismatches 1' * mismatches, took), flush=True)
        print('\n'.join('    ' + line for line in trace), flush=True)
        summary = json.loads((out / 'barcodes.json').read_text())
        units = sum(int(line.split('\t')[4]) for line in (out / 'barcodes.tsv').read_text().splitlines())
        print('%d units with a cell and a UMI, %d removed as duplicates (%.1f %%)%s'
              % (units, summary['umi_duplicates'], 100.0 * summary['umi_duplicates'] / max(units, 1),
                 ', %d of them only for a UMI one substitution away' % summary['umi_near_duplicates'] if mismatches else ''),
              flush=True)


if __name__ == '__main__':
    main()
