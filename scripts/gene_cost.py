"""What the gene-level tables (--genes) cost: N samples of P read pairs each on the synthetic index of G genes, with
the gene map of the tests (gene = transcript // 4, every tenth gene unnamed)
    device  the four native calls against the numpy statement of tests/gene_reference.py on the same inputs, with
            equality asserted (bit for bit for the sums): skm_gene_sums on the samples' TPM rows, skm_gene_unique_counts
            on the set's exported table, skm_mapper_gene_counts on one sample's resident table,
            skm_sample_set_gene_counts on the set's resident table
    host    `infer-many` on the samples' FASTQ files with `--gene-map` against the same command without it, alternating
            in one process (no file of the existing paths depends on the option, so the second is the time of a build
            without the feature)
    python3 scripts/gene_cost.py --samples 64 --pairs 20000 --genes 100
    python3 scripts/gene_cost.py --samples 64 --pairs 50000 --genes 20000 --cache /tmp/skm_idx.npz
--only device|host runs one part alone.  On a shared GPU machine run every invocation under a time limit of its own
(`timeout -k 10 600 python3 ...`), one per shape.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--samples', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', choices=['device', 'host'], default=None)
ap.add_argument('--cache', default='')
args = ap.parse_args()

import gene_reference as ref                                                        # noqa: E402
from seekmer_amd import __main__ as cli, _native, common, index_builder, infer, mapper, synth   # noqa: E402


def best(call, reps):
    """(result, warm-up ms, best ms of `reps`)"""
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, times[0], min(times[1:])


def line(what, device, numpy_ms, note=''):
    print('%-28s device: warm-up %.2f ms, best %.3f ms; numpy: %.2f ms -> %.1f x%s'
          % (what, device[1], device[2], numpy_ms, numpy_ms / device[2], note), flush=True)


def inputs():
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    if args.cache and os.path.exists(args.cache):
        index = common.KMerIndex.load(args.cache)
    else:
        index = index_builder.build_pooled(ids, pool, tx_offsets)
        if args.cache:
            index.save(args.cache)
    batches = []
    for sample in range(args.samples):
        bases, offsets = synth.reads(100 + sample % 2, pool, tx_offsets, sample * args.pairs, args.pairs, args.read_len, True)
        batches.append(common.ReadBatch(args.pairs, bases, offsets, True))
    gene = np.arange(index.transcripts.size) // 4
    names = np.asarray([b'' if g % 10 == 0 else b'G%07d' % g for g in gene])
    return index, batches, names


def device_part(index, batches, names):
    gene_ids, tx_gene = ref.gene_map_from_ids(names)
    n_genes, n = gene_ids.size, len(batches)
    index.device_handle(0)
    sample_set = mapper.SampleSet(index, True, per_sample_lengths=True)
    for sample, batch in enumerate(batches):
        sample_set.add_batch(sample, 0, batch)
    tpm = sample_set.quantify()
    print('%d transcripts, %d genes; TPM rows %s' % (tx_gene.size, n_genes, tpm.shape), flush=True)

    # (a) sums
    got = best(lambda: infer.gene_sums(tx_gene, n_genes, tpm), args.reps)
    t0 = time.perf_counter()
    want = ref.gene_sums(tx_gene, n_genes, tpm)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    assert got[0].tobytes() == want.tobytes(), 'gene sums differ from numpy.add.at'
    line('skm_gene_sums (%d rows)' % n, got, numpy_ms)

    # (b) the set's table from the host, as one CSR with the classes' samples
    summaries = sample_set.summarize()
    offsets = [np.zeros(1, dtype=np.int64)]
    targets, counts, sample_of = [], [], []
    for k, summary in enumerate(summaries):
        o, t = (summary.class_offsets, summary.class_targets) if summary.class_offsets is not None \
            else infer._csr_from_class_map(summary.class_map, summary.class_count.size)
        offsets.append(np.asarray(o[1:], dtype=np.int64) + offsets[-1][-1])
        targets.append(np.asarray(t, dtype=np.int32))
        counts.append(np.asarray(summary.class_count, dtype=np.int64))
        sample_of.append(np.full(counts[-1].size, k, dtype=np.int32))
    offsets, targets, counts, sample_of = (np.ascontiguousarray(np.concatenate(a)) for a in (offsets, targets, counts, sample_of))
    unique, other = np.zeros((n, n_genes), dtype=np.int64), np.zeros((n, 2), dtype=np.int64)
    p = _native.ptr

    def from_host():
        _native.check(_native.hip().skm_gene_unique_counts(
            0, counts.size, p(offsets, _native.c_i64p), p(targets, _native.c_i32p), p(counts, _native.c_i64p),
            p(sample_of, _native.c_i32p), n, tx_gene.size, n_genes, p(tx_gene, _native.c_i32p), p(unique, _native.c_i64p),
            p(other, _native.c_i64p)))
        return unique.copy(), other.copy()
    got = best(from_host, args.reps)
    t0 = time.perf_counter()
    want = ref.unique_counts_reduceat(offsets, targets, counts, tx_gene, n_genes, sample_of, n)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1]), 'unique counts differ from the reference'
    line('skm_gene_unique_counts', got, numpy_ms, '; %d classes, %d ids' % (counts.size, targets.size))

    # the same where the table lies
    resident = best(lambda: sample_set.gene_unique_counts(tx_gene, n_genes), args.reps)
    assert np.array_equal(resident[0][0], want[0]) and np.array_equal(resident[0][1], want[1])
    line('skm_sample_set_gene_counts', resident, numpy_ms)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(batches[0])
    one = best(lambda: result.gene_unique_counts(tx_gene, n_genes), args.reps)
    first = slice(0, int(np.searchsorted(sample_of, 1)))
    t0 = time.perf_counter()
    want_one = ref.unique_counts_reduceat(np.concatenate([[0], offsets[1:][first]]), targets[:offsets[1:][first][-1]], counts[first],
                                          tx_gene, n_genes)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(one[0][0], want_one[0][0]) and np.array_equal(one[0][1], want_one[1][0])
    line('skm_mapper_gene_counts', one, numpy_ms, '; %d classes' % counts[first].size)
    kinds = want[0].sum(), want[1][:, 0].sum(), want[1][:, 1].sum()
    print('units inside one gene / ambiguous / unnamed: %d / %d / %d' % kinds, flush=True)


def write_fastq(path, batch, mate):
    bases, offsets = batch.bases.tobytes(), batch.offsets
    with open(path, 'wb') as f:
        for u in range(batch.count):
            read = bases[offsets[2 * u + mate]:offsets[2 * u + mate + 1]]
            f.write(b'@u%d\n%s\n+\n%s\n' % (u, read, b'I' * len(read)))


def host_part(index, batches, names):
    folder = tempfile.mkdtemp(prefix='gene_cost_')
    try:
        index_path = os.path.join(folder, 'index.npz')
        index.save(index_path)
        with open(os.path.join(folder, 'genes.tsv'), 'wb') as f:
            for id_, gene in zip(index.transcripts['transcript_id'], names):
                if gene:
                    f.write(id_ + b'\t' + gene + b'\n')
        files = []
        print('writing the FASTQ files of %d samples' % len(batches), flush=True)
        for sample, batch in enumerate(batches):
            for mate in range(2):
                files.append(os.path.join(folder, 's%03d_%d.fastq' % (sample, mate + 1)))
                write_fastq(files[-1], batch, mate)
        commands = {'without': [], 'with --gene-map': ['--gene-map', os.path.join(folder, 'genes.tsv')]}
        times = {name: [] for name in commands}
        for rep in range(args.reps + 1):                 # (the first repetition of each is its warm-up)
            for name, extra in commands.items():
                out = os.path.join(folder, 'out_%d_%d' % (rep, len(extra)))
                t0 = time.perf_counter()
                assert cli.main(['infer-many', index_path, out, *files, *extra]) == 0
                times[name].append(time.perf_counter() - t0)
                print('  infer-many %s, run %d: %.2f s' % (name, rep, times[name][-1]), flush=True)
                shutil.rmtree(out)
        for name, seconds in times.items():
            print('infer-many %-16s warm-up %.2f s; then %s s -> best %.2f ms per sample'
                  % (name, seconds[0], ', '.join('%.2f' % s for s in seconds[1:]), min(seconds[1:]) * 1e3 / len(batches)), flush=True)
        print('with / without = %.3f (best of each)' % (min(times['with --gene-map'][1:]) / min(times['without'][1:])), flush=True)
    finally:
        shutil.rmtree(folder, ignore_errors=True)


def main():
    import logging
    logging.disable(logging.CRITICAL)
    t0 = time.perf_counter()
    index, batches, names = inputs()
    print('%d samples x %d pairs on %d transcripts: index and reads made in %.1f s'
          % (args.samples, args.pairs, index.transcripts.size, time.perf_counter() - t0), flush=True)
    if args.only in (None, 'device'):
        device_part(index, batches, names)
    if args.only in (None, 'host'):
        host_part(index, batches, names)


if __name__ == '__main__':
    main()
