"""What distributing molecules costs: N cells of P read pairs each (--copies copies of a molecule on average, UMIs of 12
bases) on the synthetic index of G genes, with the gene map of the tests (gene = transcript // 4, every tenth unnamed)
-- the cells, files and options of scripts/resolve_molecules_cost.py.
    (a) distributed / resolved   SampleSet.gene_distributed_matrix against SampleSet.gene_resolved_matrix on the same
                         resident set -- the N cells added to one sample set that keeps UMIs, each call timed warm-up +
                         best of --reps; when both run, the tally identities are asserted: resolved, unnamed and
                         collision are equal, distributed + wide is the resolved matrix's multi-gene.  The EM's steps
                         per cell (smallest, mean, largest) and the capped cells are printed;
    (b) with / without   the pooled run through `infer-many --barcodes ... --umi-length 12 --gene-map FILE --matrix-only
                         --resolve-molecules`, against the same command with `--distribute-molecules`, SKM_TRACE_INFER's
                         phase times of both printed.
    python3 scripts/distribute_molecules_cost.py --cells 64 --pairs 20000 --genes 100 --copies 2
--only distributed|resolved runs one form alone, in both parts.  A synthetic pair is one fragment, so a molecule here
falls into one class; a cell's UMIs are drawn from half as many values as it has molecules, so two molecules share a
UMI now and then.  The sets are the ambiguous classes and such pairs: the figures are the cost of the pass on this
shape, not what it shares out on real libraries.  Wall time of whole processes for (b).  Making the index and the
files happens before any clock starts.  Every step that uses the GPU is a child process under a time limit of its own
(`timeout -k 10 SECONDS ...`), one at a time; the script stops at the first step that fails and starts nothing again.
On a shared GPU machine run every invocation under `timeout -k 10 600`, one per shape.
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
ap.add_argument('--copies', type=float, default=2.0, help='copies of a molecule, on average')
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--barcode-len', type=int, default=16)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', choices=('distributed', 'resolved'), default=None)
ap.add_argument('--cache', default='', help='keep the index in this file between invocations')
ap.add_argument('--step-limit', type=int, default=300, help='seconds one child process may take')
ap.add_argument('--work', default='', help='folder for the files (default: a temporary one)')
ap.add_argument('--resident', default='', help=argparse.SUPPRESS)       # (the child process of part (a): the index file)
args = ap.parse_args()


def gene_names(n_tx):
    gene = numpy.arange(n_tx) // 4
    return [b'' if g % 10 == 0 else b'G%07d' % g for g in gene]


def cell_units(rng, pool, tx_offsets, cell, molecules):
    """(pairs uint8[P, 2, read_len], umi uint32[P]) of one cell: P units that copy `molecules` distinct pairs"""
    from seekmer_amd import synth
    bases, _ = synth.reads(100 + cell % 2, pool, tx_offsets, cell * molecules, molecules, args.read_len, True)
    pairs = bases[:-1].reshape(molecules, 2, args.read_len)
    drawn = rng.integers(0, molecules, size=args.pairs)                  # the molecule every unit of the cell copies
    umi = rng.integers(0, max(molecules // 2, 1), size=molecules).astype(numpy.uint32) * 2654435761 % (4 ** UMI_LENGTH)
    return pairs[drawn], umi.astype(numpy.uint32)[drawn]


def resident_part():
    """The child process of part (a): the cells in one sample set that keeps UMIs, the two calls on its resident state."""
    import logging
    logging.disable(logging.CRITICAL)
    from seekmer_amd import common, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index = common.KMerIndex.load(args.resident)
    named = numpy.asarray(gene_names(index.transcripts.size))
    gene_ids = numpy.unique(named[named != b''])
    tx_gene = numpy.full(named.size, -1, dtype=numpy.int32)
    tx_gene[named != b''] = numpy.searchsorted(gene_ids, named[named != b''])
    index.device_handle(0)
    rng = numpy.random.default_rng(1)
    molecules = max(1, int(round(args.pairs / args.copies)))
    sample_set = mapper.SampleSet(index, True, per_sample_lengths=True, umi_bases=UMI_LENGTH)
    offsets = numpy.arange(args.pairs + 1, dtype=numpy.int64) * args.read_len
    for cell in range(args.cells):
        pairs, umi = cell_units(rng, pool, tx_offsets, cell, molecules)
        pieces = [common.PackedReads.from_ascii(numpy.append(pairs[:, mate].ravel(), numpy.uint8(65)), offsets, stream=mate)
                  for mate in (0, 1)]
        sample_set.add_packed(cell, 0, *pieces, umis=umi)
    sizes = sample_set.sizes()
    print('%d cells, %d classes in the set\'s table, %d units left of %d after collapse, %d transcripts, %d genes'
          % (len(sizes), sizes[:, 0].sum(), sizes[:, 3].sum(), args.cells * args.pairs, tx_gene.size, gene_ids.size), flush=True)

    def best(call):
        times = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            out = call()
            times.append(1e3 * (time.perf_counter() - t0))
        return out, times[0], min(times[1:])
    resolved = distributed = None
    if args.only in (None, 'resolved'):
        resolved = best(lambda: sample_set.gene_resolved_matrix(tx_gene, gene_ids.size))
        tally = resolved[0][3]
        print('SampleSet.gene_resolved_matrix (resolved):       warm-up %.2f ms, best %.3f ms; %d entries; distinct UMIs per cell %d: '
              'resolved %d (rescued %d), multi-gene %d, unnamed %d, collisions %d'
              % (resolved[1], resolved[2], resolved[0][0][-1], tally[:, [0, 2, 3, 4]].sum(), *tally.sum(axis=0)), flush=True)
    if args.only in (None, 'distributed'):
        distributed = best(lambda: sample_set.gene_distributed_matrix(tx_gene, gene_ids.size))
        indptr, _, data, tally, to_unnamed = distributed[0]
        print('SampleSet.gene_distributed_matrix (distributed): warm-up %.2f ms, best %.3f ms; %d entries; distinct UMIs per cell %d: '
              'resolved %d, distributed %d, wide %d, unnamed %d, collisions %d'
              % (distributed[1], distributed[2], indptr[-1], tally[:, :5].sum(), *tally[:, :5].sum(axis=0)), flush=True)
        print('    EM: rows per cell %d .. %d, steps per cell %d .. %d (mean %.1f), %d cells capped; weight in genes %.3f, to no gene %.3f'
              % (tally[:, 5].min(), tally[:, 5].max(), tally[:, 6].min(), tally[:, 6].max(), tally[:, 6].mean(), tally[:, 7].sum(),
                 data.sum(), to_unnamed.sum()), flush=True)
        placed = tally[:, 0].sum() + tally[:, 1].sum() + tally[:, 3].sum()
        assert abs(data.sum() + to_unnamed.sum() - placed) < 1e-3 * len(data) + 1e-6 * placed, 'molecules were lost beyond the cut'
    if resolved and distributed:
        was, now = resolved[0][3], distributed[0][3]
        assert (was[:, [0, 3, 4]] == now[:, [0, 3, 4]]).all() and (was[:, 2] == now[:, 1] + now[:, 2]).all(), 'the tallies differ'
        print('distributed / resolved = %.2f (best of each); the tallies agree' % (distributed[2] / resolved[2]), flush=True)


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
    return dt, done.stdout.decode(errors='replace'), [line for line in text.splitlines()
                                                      if line.startswith('[run_many]') or 'molecules (distinct' in line
                                                      or 'resolved to one gene' in line or 'distributed by the EM' in line]


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


def pooled_files(work, pool, tx_offsets):
    """pool_1.fastq, pool_2.fastq, barcodes.fastq (barcode + UMI), whitelist.tsv: the cells of part (a), shuffled"""
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
        pairs, umi = cell_units(rng, pool, tx_offsets, c, molecules)
        mates[0].append(pairs[:, 0]); mates[1].append(pairs[:, 1])
        shifts = 2 * numpy.arange(UMI_LENGTH - 1, -1, -1, dtype=numpy.uint32)
        umis.append(letters[(umi[:, None] >> shifts[None, :]) & 3])
    n_units = args.cells * args.pairs
    shuffle = rng.permutation(n_units)
    mates = [numpy.concatenate(mate)[shuffle] for mate in mates]
    for mate in (0, 1):
        write_fastq(work / ('pool_%d.fastq' % (mate + 1)), mates[mate], args.read_len)
    barcodes = whitelist[shuffle // args.pairs]
    write_fastq(work / 'barcodes.fastq', numpy.concatenate([barcodes, numpy.concatenate(umis)[shuffle]], axis=1),
                args.barcode_len + UMI_LENGTH)
    return molecules


def main():
    from seekmer_amd import index_builder, synth            # (host code only: this process never opens the GPU)
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix='skm_distribute_molecules_'))
    work.mkdir(parents=True, exist_ok=True)
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index_path = pathlib.Path(args.cache) if args.cache else work / 'index.npz'
    if not index_path.exists():
        index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    print('%d cells x %d pairs of 2 x %d bases, %.2f copies a molecule, on %d transcripts; index of %.0f MiB'
          % (args.cells, args.pairs, args.read_len, args.copies, len(ids), index_path.stat().st_size / 2 ** 20), flush=True)
    forward = ['--cells', str(args.cells), '--pairs', str(args.pairs), '--genes', str(args.genes), '--copies', str(args.copies),
               '--read-len', str(args.read_len), '--reps', str(args.reps), '--resident', str(index_path)]
    if args.only:
        forward += ['--only', args.only]
    _, out, _ = step('the calls on the resident set', forward, module=False)
    print(out, end='', flush=True)
    with open(work / 'genes.tsv', 'wb') as f:
        for id_, gene in zip(ids, gene_names(len(ids))):
            if gene:
                f.write(id_ + b'\t' + gene + b'\n')
    pooled_files(work, pool, tx_offsets)
    pooled = ['infer-many', str(index_path), None, str(work / 'pool_1.fastq'), str(work / 'pool_2.fastq'), '--barcodes',
              str(work / 'whitelist.tsv'), '--barcode-file', str(work / 'barcodes.fastq'), '-j', str(args.jobs),
              '--umi-start', str(args.barcode_len), '--umi-length', str(UMI_LENGTH), '--gene-map', str(work / 'genes.tsv'),
              '--matrix-only', '--resolve-molecules']
    took = {}
    for form, extra in (('resolved', []), ('distributed', ['--distribute-molecules'])):
        if args.only in (None, form):
            pooled[2] = str(work / ('out_' + form))
            took[form], _, trace = step('infer-many --matrix-only --resolve-molecules ' + ' '.join(extra), pooled + extra)
            print('infer-many --barcodes --umi-length %d --matrix-only --resolve-molecules%s:   %.2f s'
                  % (UMI_LENGTH, ' --distribute-molecules' if extra else '', took[form]), flush=True)
            print('\n'.join('    ' + line for line in trace), flush=True)
    if len(took) == 2:
        print('with / without --distribute-molecules = %.3f' % (took['distributed'] / took['resolved']), flush=True)
        names = sorted(f.name for f in (work / 'out_resolved' / 'counts').iterdir())
        for name in names:
            assert (work / 'out_resolved' / 'counts' / name).read_bytes() == (work / 'out_distributed' / 'counts' / name).read_bytes(), name
        print('counts/: the %d files of --resolve-molecules are the same bytes in both runs' % len(names), flush=True)


if __name__ == '__main__':
    if args.resident:
        resident_part()
    else:
        main()
