"""What the count matrix costs and saves: N cells of P read pairs each on the synthetic index of G genes, with the gene
map of the tests (gene = transcript // 4, every tenth gene unnamed).
    (a) sparse / dense   SampleSet.gene_count_matrix against SampleSet.gene_unique_counts on the same resident table --
                         the N cells added to one sample set, each call timed warm-up + best of --reps, equality of the
                         densified matrix and the dense rows asserted when both run;
    (b) full / matrix_only   the pooled run of scripts/umi_cost.py (one pair of FASTQ files, a barcode file with a UMI of
                         12 bases, --copies copies of a molecule on average) through `infer-many --barcodes ...
                         --umi-length 12` as it is without the new options, against the same command with
                         `--gene-map FILE --matrix-only`, SKM_TRACE_INFER's phase times of both printed.
    python3 scripts/count_matrix_cost.py --cells 64 --pairs 20000 --genes 100
    python3 scripts/count_matrix_cost.py --cells 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
--only sparse|dense|full|matrix_only runs one form alone (sparse alone is for cell counts whose dense rows no longer
fit).  Wall time of whole processes for (b).  Making the index and the files happens before any clock starts.  Every
step that uses the GPU is a child process under a time limit of its own (`timeout -k 10 SECONDS ...`); the script stops
at the first step that fails and starts nothing again.  On a shared GPU machine run every invocation under
`timeout -k 10 600`, one per shape.
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

UMI_LENGTH = 12

ap = argparse.ArgumentParser()
ap.add_argument('--cells', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--copies', type=float, default=2.0, help='copies of a molecule, on average (the pooled run)')
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--barcode-len', type=int, default=16)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', choices=('sparse', 'dense', 'full', 'matrix_only'), default=None)
ap.add_argument('--cache', default='', help='keep the index in this file between invocations')
ap.add_argument('--step-limit', type=int, default=300, help='seconds one child process may take')
ap.add_argument('--work', default='', help='folder for the files (default: a temporary one)')
ap.add_argument('--resident', default='', help=argparse.SUPPRESS)       # (the child process of part (a): the index file)
args = ap.parse_args()


def gene_names(n_tx):
    gene = numpy.arange(n_tx) // 4
    return [b'' if g % 10 == 0 else b'G%07d' % g for g in gene]


def resident_part():
    """The child process of part (a): the cells in one sample set, the two calls on its resident table."""
    import logging
    logging.disable(logging.CRITICAL)
    from seekmer_amd import common, infer, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index = common.KMerIndex.load(args.resident)
    named = numpy.asarray(gene_names(index.transcripts.size))
    gene_ids = numpy.unique(named[named != b''])
    tx_gene = numpy.full(named.size, -1, dtype=numpy.int32)
    tx_gene[named != b''] = numpy.searchsorted(gene_ids, named[named != b''])
    index.device_handle(0)
    sample_set = mapper.SampleSet(index, True, per_sample_lengths=True)
    for cell in range(args.cells):
        bases, offsets = synth.reads(100 + cell % 2, pool, tx_offsets, cell * args.pairs, args.pairs, args.read_len, True)
        sample_set.add_batch(cell, 0, common.ReadBatch(args.pairs, bases, offsets, True))
    sizes = sample_set.sizes()
    print('%d cells, %d classes in the set\'s table, %d transcripts, %d genes; dense rows: %.1f MB'
          % (len(sizes), sizes[:, 0].sum(), tx_gene.size, gene_ids.size, 8e-6 * len(sizes) * gene_ids.size), flush=True)

    def best(call):
        times = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            out = call()
            times.append(1e3 * (time.perf_counter() - t0))
        return out, times[0], min(times[1:])
    sparse = dense = None
    if args.only in (None, 'sparse'):
        sparse = best(lambda: sample_set.gene_count_matrix(tx_gene, gene_ids.size))
        indptr, _, data, _ = sparse[0]
        print('SampleSet.gene_count_matrix  (sparse): warm-up %.2f ms, best %.3f ms; %d entries, %.1f per cell, %d units inside one gene'
              % (sparse[1], sparse[2], indptr[-1], indptr[-1] / max(len(sizes), 1), data.sum()), flush=True)
    if args.only in (None, 'dense'):
        dense = best(lambda: sample_set.gene_unique_counts(tx_gene, gene_ids.size))
        print('SampleSet.gene_unique_counts (dense):  warm-up %.2f ms, best %.3f ms' % (dense[1], dense[2]), flush=True)
    if sparse and dense:
        indptr, indices, data, other = sparse[0]
        rows = numpy.repeat(numpy.arange(len(sizes)), numpy.diff(indptr))
        densified = numpy.zeros_like(dense[0][0])
        densified[rows, indices] = data
        assert numpy.array_equal(densified, dense[0][0]) and numpy.array_equal(other, dense[0][1]), 'sparse and dense differ'
        print('sparse / dense = %.2f (best of each); the two agree entry for entry' % (sparse[2] / dense[2]), flush=True)
    del infer


def step(name, arguments, module=True):
    """One child process under its own time limit; the first failure ends the script.  Returns (seconds, stdout, trace)."""
    t0 = time.perf_counter()
    command = [sys.executable, '-m', 'seekmer_amd'] if module else [sys.executable, os.path.abspath(__file__)]
    done = subprocess.run(['timeout', '-k', '10', str(args.step_limit)] + command + arguments, cwd=ROOT,
                          env=dict(os.environ, SKM_TRACE_INFER='1'), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    text = done.stderr.decode(errors='replace')
    if done.returncode != 0:
        sys.stderr.write(text[-4000:])
        sys.exit('%s ended with status %d after %.1f s: nothing more is started' % (name, done.returncode, dt))
    return dt, done.stdout.decode(errors='replace'), [line for line in text.splitlines() if line.startswith('[run_many]')]


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


def pooled_files(work, ids, pool, tx_offsets):
    """The pooled run of scripts/umi_cost.py: pool_1.fastq, pool_2.fastq, barcodes.fastq, whitelist.tsv"""
    from seekmer_amd import synth
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
    return molecules


def main():
    from seekmer_amd import index_builder, synth            # (host code only: this process never opens the GPU)
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix='skm_count_matrix_'))
    work.mkdir(parents=True, exist_ok=True)
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index_path = pathlib.Path(args.cache) if args.cache else work / 'index.npz'
    if not index_path.exists():
        index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    print('%d cells x %d pairs of 2 x %d bases on %d transcripts; index of %.0f MiB'
          % (args.cells, args.pairs, args.read_len, len(ids), index_path.stat().st_size / 2 ** 20), flush=True)
    if args.only in (None, 'sparse', 'dense'):
        forward = ['--cells', str(args.cells), '--pairs', str(args.pairs), '--genes', str(args.genes), '--read-len',
                   str(args.read_len), '--reps', str(args.reps), '--resident', str(index_path)]
        if args.only:
            forward += ['--only', args.only]
        _, out, _ = step('the calls on the resident table', forward, module=False)
        print(out, end='', flush=True)
    if args.only in (None, 'full', 'matrix_only'):
        with open(work / 'genes.tsv', 'wb') as f:
            for id_, gene in zip(ids, gene_names(len(ids))):
                if gene:
                    f.write(id_ + b'\t' + gene + b'\n')
        molecules = pooled_files(work, ids, pool, tx_offsets)
        print('pooled run: %d molecules a cell, %.2f copies each on average, barcodes of %d bases + UMIs of %d'
              % (molecules, args.pairs / molecules, args.barcode_len, UMI_LENGTH), flush=True)
        pooled = ['infer-many', str(index_path), None, str(work / 'pool_1.fastq'), str(work / 'pool_2.fastq'), '--barcodes',
                  str(work / 'whitelist.tsv'), '--barcode-file', str(work / 'barcodes.fastq'), '-j', str(args.jobs),
                  '--umi-start', str(args.barcode_len), '--umi-length', str(UMI_LENGTH)]
        took = {}
        for form, extra in (('full', []), ('matrix_only', ['--gene-map', str(work / 'genes.tsv'), '--matrix-only'])):
            if args.only in (None, form):
                pooled[2] = str(work / ('out_' + form))
                took[form], _, trace = step('infer-many --barcodes --umi-length ' + ' '.join(extra[-1:]), pooled + extra)
                print('infer-many --barcodes --umi-length %d%s:   %.2f s'
                      % (UMI_LENGTH, ' --matrix-only' if extra else ' (every table)', took[form]), flush=True)
                print('\n'.join('    ' + line for line in trace), flush=True)
        if len(took) == 2:
            print('matrix_only / full = %.3f' % (took['matrix_only'] / took['full']), flush=True)
            cells = (work / 'out_matrix_only' / 'counts' / 'cells.tsv').read_text().splitlines()
            print('counts/: %d cells, %d entries' % (len(cells), sum(int(line.split('\t')[6]) for line in cells)), flush=True)


if __name__ == '__main__':
    if args.resident:
        resident_part()
    else:
        main()
