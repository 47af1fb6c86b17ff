"""Host-side native code (libseekmer_host.so) and the Python module surface
that needs no GPU: index builder == oracle bit for bit, FASTQ batching rules,
synthetic generator determinism."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

ARRAYS = ('kmers', 'contigs', 'sequences', 'targets')


def _same_index(product, oracle_index):
    for name in ARRAYS:
        assert getattr(product, name).tobytes() == getattr(oracle_index, name).tobytes(), name


def test_builder_matches_oracle_chr21(native_libs, oracle, chr21, chr21_oracle_index):
    from seekmer_amd import index_builder
    index = index_builder.build(*chr21)
    _same_index(index, chr21_oracle_index)
    assert index.transcripts['length'].tolist() == [float(len(s)) for s in chr21[1]]
    assert index.transcripts['transcript_id'][0] == chr21[0][0]


def test_builder_matches_oracle_with_extra(native_libs, oracle):
    from seekmer_amd import index_builder
    ids, seqs = index_builder.read_transcripts(os.path.join(GOLDEN, 'human.cdna.21.with_extra.fa.gz'))
    o_ids, o_seqs = oracle.read_fasta(os.path.join(GOLDEN, 'human.cdna.21.with_extra.fa.gz'))
    assert (ids, seqs) == (o_ids, o_seqs)
    index = index_builder.build(ids, seqs)
    _same_index(index, oracle.build_index(seqs))
    assert index.transcripts.shape[0] == 3                     # test_index_builder.py:90


@pytest.mark.parametrize('seed,genes', [(1, 100), (2, 37)])
def test_builder_matches_oracle_synthetic(native_libs, oracle, seed, genes):
    from seekmer_amd import index_builder, synth
    ids, pool, offsets = synth.transcriptome(seed, genes)
    index = index_builder.build_pooled(ids, pool, offsets)
    _same_index(index, oracle.build_index(synth.sequences_of(pool, offsets)))


def test_builder_edge_inputs(native_libs, oracle):
    """Short transcripts are skipped, repeats / palindromes / homopolymers and
    lower case + N go through the same code paths as in the oracle."""
    from seekmer_amd import index_builder
    rng = np.random.default_rng(3)
    core = bytes(rng.choice(list(b'ACGT'), 400).astype(np.uint8))
    seqs = [b'ACGT' * 5, core, core[50:300] + core[:80], b'A' * 60, b'AT' * 40,
            core[:100].lower() + b'NNN' + core[100:200], core[::-1], b'']
    ids = [b'T%d' % i for i in range(len(seqs))]
    index = index_builder.build(ids, seqs)
    _same_index(index, oracle.build_index(seqs))


def test_builder_never_leaves_an_occupied_slot_unassigned(native_libs, oracle):
    """SURVEY.md (rows a9, (f)1) records, for the reference's 3-transcript FASTA, one
    occupied k-mer slot whose position was never assigned and a 24-base contig without
    targets: the compiled reference's "no link" value is 0, the number of a slot (SURVEY.md
    section 0, finding 8; tests/test_reference_recordings.py pins that relation).  With a value
    that is no slot number, as our builders have it, neither can come out of _assemble_contigs
    (_index_builder.pyx:428-487): links are
    only ever made between two consecutive NEW k-mers (:283-288), so the graph is a set of
    disjoint simple paths, every path has an end that starts a walk (:436-445), a walk covers its
    whole path (:458-471), and a contig of n k-mers is 25*ceil(n/25) + (n-1)%25 = n + 24 >= 25
    bases long (:466-476).  DESIGN.md section 2 spells the argument out; here it is checked on
    the graph shapes that could break it -- tandem repeats (would-be cycles), hairpins, even
    palindromes (a k-mer followed by its own reverse complement), shared pieces in both
    orientations, low-complexity sequence -- and on the reference's own 3-transcript file."""
    from seekmer_amd import index_builder
    rng = np.random.default_rng(0)
    comp = bytes.maketrans(b'ACGT', b'TGCA')

    def rnd(n):
        return bytes(rng.choice(list(b'ACGT'), n).astype(np.uint8))

    def check(seqs, compare_product):
        ix = oracle.build_index(seqs)
        occupied = ix.kmers['kmer'] != np.uint64(0xFFFFFFFFFFFFFFFF)
        assert (ix.kmers['offset'][occupied] >= 0).all()
        assert (ix.kmers['offset'][~occupied] < 0).all()          # empty slots are (0, -1)
        if ix.contigs.size:
            assert ix.contigs['length'].min() >= 25
            assert (ix.contigs['target_count'] > 0).all()
            # every occupied slot lies on a contig: the lengths add up
            assert occupied.sum() == (ix.contigs['length'] - 24).sum()
        if compare_product:
            index = index_builder.build([b'T%d' % i for i in range(len(seqs))], seqs)
            _same_index(index, ix)

    _, seqs3 = oracle.read_fasta(os.path.join(GOLDEN, 'human.cdna.21.with_extra.fa.gz'))
    check(seqs3, True)
    for trial in range(240):
        kind = trial % 6
        core = rnd(int(rng.integers(30, 200)))
        if kind == 0:
            unit = rnd(int(rng.integers(1, 40)))
            seqs = [unit * int(rng.integers(2, 10)) + rnd(int(rng.integers(0, 30)))]
        elif kind == 1:
            seqs = [core + core.translate(comp)[::-1]]
        elif kind == 2:
            seqs = []
            for _ in range(int(rng.integers(2, 6))):
                a = int(rng.integers(0, len(core) - 26))
                b = int(rng.integers(a + 25, len(core) + 1))
                piece = core[a:b]
                if rng.random() < 0.5:
                    piece = piece.translate(comp)[::-1]
                seqs.append(rnd(int(rng.integers(0, 40))) + piece + rnd(int(rng.integers(0, 40))))
        elif kind == 3:
            half = rnd(12)
            palindrome = half + half.translate(comp)[::-1]
            seqs = [rnd(30) + palindrome + rnd(30), rnd(10) + palindrome + rnd(10), palindrome * 3]
        elif kind == 4:
            seqs = [bytes(rng.choice(list(b'AC'), int(rng.integers(25, 120))).astype(np.uint8))
                    for _ in range(4)]
        else:
            seqs = [core + rnd(5) + core[10:] + core.translate(comp)[::-1][5:], core[::-1]]
        check(seqs, trial < 60)


def test_build_rejects_empty(native_libs):
    from seekmer_amd import index_builder
    with pytest.raises(ValueError):
        index_builder.build([], [])                             # index_builder.py:106-107


def test_index_save_load_roundtrip(native_libs, tmp_path, chr21):
    from seekmer_amd import common, index_builder
    index = index_builder.build(chr21[0][:50], chr21[1][:50])
    path = tmp_path / 'index.npz'
    index.save(path)
    loaded = common.KMerIndex.load(path)
    for name in ARRAYS:
        assert getattr(loaded, name).tobytes() == getattr(index, name).tobytes()
    assert loaded.transcripts['transcript_id'].tolist() == index.transcripts['transcript_id'].tolist()


def test_index_load_maps_the_container(native_libs, tmp_path, chr21):
    """The four big arrays come back as views of the file (no copy through the zip reader); a
    deflated container, which cannot be mapped, still loads through numpy; a wrong version is
    refused like the reference does (seekmer/_common.pyx:303-304)."""
    from seekmer_amd import common, index_builder
    index = index_builder.build(chr21[0][:40], chr21[1][:40])
    path = tmp_path / 'index.npz'
    index.save(path)
    mapped = common._map_npz_members(str(path))
    assert sorted(mapped) == sorted(ARRAYS)
    for name in ARRAYS:
        assert isinstance(mapped[name], np.memmap)
        assert mapped[name].dtype == getattr(index, name).dtype
        assert mapped[name].tobytes() == getattr(index, name).tobytes()
    packed = tmp_path / 'deflated.npz'
    np.savez_compressed(packed, seekmer_version=np.asarray(common._INDEX_VERSION),
                        kmers=index.kmers, contigs=index.contigs, sequences=index.sequences,
                        targets=index.targets, transcripts=np.asarray(index.transcripts),
                        exons=np.asarray(index.exons))
    assert common._map_npz_members(str(packed)) == {}
    loaded = common.KMerIndex.load(packed)
    for name in ARRAYS:
        assert getattr(loaded, name).tobytes() == getattr(index, name).tobytes()
    wrong = tmp_path / 'wrong.npz'
    np.savez(wrong, seekmer_version=np.asarray('0.0.0'), kmers=index.kmers, contigs=index.contigs,
             sequences=index.sequences, targets=index.targets,
             transcripts=np.asarray(index.transcripts), exons=np.asarray(index.exons))
    with pytest.raises(RuntimeError):
        common.KMerIndex.load(wrong)


def test_native_feeder_batches_outlive_the_loop(native_libs, tmp_path):
    """Batches are views of slabs owned by the reader; one kept past the loop (and past the
    reader) must stay intact, and slabs of dropped batches are reused."""
    from seekmer_amd import common
    lines = []
    for i in range(5000):
        lines += [b'@r%d\n' % i, b'ACGT' * 10 + b'%04d' % i + b'\n', b'+\n', b'I' * 44 + b'\n']
    path = tmp_path / 'r.fastq'
    path.write_bytes(b''.join(lines))
    kept = []
    for k, batch in enumerate(common.NativeReadFeeder([path], paired=False, batch_units=512)):
        if k in (0, 3):
            kept.append((k, batch))
    for k, batch in kept:
        reads = batch.reads
        assert len(reads) == 512
        assert reads[0] == b'ACGT' * 10 + b'%04d' % (512 * k) and reads[-1][-4:] == b'%04d' % (512 * k + 511)
        assert batch.names[0] == b'r%d' % (512 * k)


@pytest.mark.timeout(60)
def test_native_feeder_early_exit_on_compressed_input(native_libs, tmp_path):
    """Leaving the loop after one batch of a .gz input (or an exception while mapping) must not
    hang: the native reader's own descriptors of the zcat pipe are closed before the child is
    reaped (round-1 advisor finding: zcat blocked on the full pipe, wait() never returned)."""
    import gzip
    import time
    from seekmer_amd import common
    rng = np.random.default_rng(4)
    seq = bytes(rng.choice(list(b'ACGT'), 100).astype(np.uint8))
    record = b'@r\n' + seq + b'\n+\n' + b'I' * 100 + b'\n'
    path = tmp_path / 'big.fastq.gz'
    with gzip.open(str(path), 'wb', compresslevel=1) as f:
        for _ in range(40):
            f.write(record * 1000)                       # 40 000 reads, ~8 MB of text
    t0 = time.time()
    it = iter(common.NativeReadFeeder([path], paired=False, batch_units=1000))
    first = next(it)
    assert first.count == 1000 and first.reads[0] == seq
    it.close()                                           # GeneratorExit -> finally
    assert time.time() - t0 < 20

    def failing():
        for k, batch in enumerate(common.NativeReadFeeder([path], paired=False, batch_units=1000)):
            if k == 2:
                raise RuntimeError('mapping failed')
    with pytest.raises(RuntimeError):
        failing()
    assert first.reads[-1] == seq                        # the kept batch outlives the reader


# ---- feeders: the reference's TestReadFeeder (seekmer/test/test_mapper.py:20-68)
_BASE_SET = set(b'ACTGNactg')


def _check_batches(batches, count, reads_per_unit):
    seen = 0
    for n, names, reads in batches:
        seen += 1
        assert n == count
        assert len(names) == n
        assert len(reads) == n * reads_per_unit
        for read in reads:
            assert set(read) <= _BASE_SET
    assert seen == 1


@pytest.mark.parametrize('native', [False, True])
def test_feed_single_ended_reads(native_libs, native):
    from seekmer_amd import common
    path = os.path.join(GOLDEN, '20_1.fastq')
    import pathlib
    p = pathlib.Path(path)
    feed = (lambda *ps: common.NativeReadFeeder(ps, paired=False)) if native else common.feed_single_ended_reads
    _check_batches(feed(p), 21, 1)
    _check_batches(feed(p, p), 42, 1)                           # buffer carried across files


@pytest.mark.parametrize('native', [False, True])
def test_feed_pair_ended_reads(native_libs, native):
    import pathlib
    from seekmer_amd import common
    paths = [pathlib.Path(GOLDEN) / '20_1.fastq', pathlib.Path(GOLDEN) / '20_2.fastq']
    feed = (lambda *ps: common.NativeReadFeeder(ps, paired=True)) if native else common.feed_pair_ended_reads
    _check_batches(feed(*paths), 21, 2)
    _check_batches(feed(*(paths * 2)), 42, 2)
    with pytest.raises(ValueError):
        list(feed(paths[0]))                                     # common.py:178-179


def test_native_feeder_equals_python_feeder(native_libs, tmp_path):
    """Same names, same reads, same batch boundaries -- incl. CRLF, blank
    padding, a last line without newline, gzip input and small batches."""
    import gzip
    import pathlib
    from seekmer_amd import common
    rng = np.random.default_rng(9)
    lines1, lines2 = [], []
    for i in range(1000):
        for lines, mate in ((lines1, 1), (lines2, 2)):
            n = int(rng.integers(25, 120))
            seq = bytes(rng.choice(list(b'ACGTNacgt'), n).astype(np.uint8))
            eol = b'\r\n' if i % 7 == 0 else b'\n'
            lines += [b'@read%d/%d extra' % (i, mate) + eol, b'  ' + seq + b' ' + eol, b'+' + eol,
                      b'I' * n + eol]
    lines1[-1] = lines1[-1].rstrip()
    lines2[-1] = lines2[-1].rstrip()
    p1, p2 = tmp_path / 'a_1.fastq', tmp_path / 'a_2.fastq.gz'
    p1.write_bytes(b''.join(lines1))
    with gzip.open(str(p2), 'wb') as f:
        f.write(b''.join(lines2))
    old = common.BUFFER_SIZE
    try:
        common.BUFFER_SIZE = 300
        expected = [(n, list(names), list(reads)) for n, names, reads in
                    common.feed_pair_ended_reads(pathlib.Path(p1), pathlib.Path(p2))]
    finally:
        common.BUFFER_SIZE = old
    got = [(b.count, b.names, b.reads) for b in
           common.NativeReadFeeder([p1, p2], paired=True, batch_units=300)]
    assert got == expected
    assert [g[0] for g in got] == [300, 300, 300, 100]


def test_synth_is_deterministic_and_sliceable(native_libs):
    from seekmer_amd import synth
    ids, pool, offsets = synth.transcriptome(5, 30)
    ids2, pool2, offsets2 = synth.transcriptome(5, 30)
    assert pool.tobytes() == pool2.tobytes() and offsets.tolist() == offsets2.tolist()
    assert set(pool[:-1].tobytes()) <= set(b'ACGT')
    full, _ = synth.reads(5, pool, offsets, 0, 5000, 75, True, n_threads=4)
    part, _ = synth.reads(5, pool, offsets, 1234, 100, 75, True, n_threads=1)
    assert part[:-1].tobytes() == full[1234 * 150:(1234 + 100) * 150].tobytes()
    single, o = synth.reads(5, pool, offsets, 0, 10, 100, False)
    assert o.tolist() == list(range(0, 1001, 100))


# ---- impute: the host-side arithmetic around the kernels (seekmer/impute.py:149-252)
def test_impute_weights_and_blend(native_libs):
    """gene_matrix / cell_weights / blend against the reference's formulae spelled out
    naively: integer truncation of the gene sums, correlation + 2-means cut, and the
    count blend c_j * w_ij * total_i / total_j over the concatenated class tables."""
    import types
    from seekmer_amd import impute
    rng = np.random.default_rng(3)
    n_tx, n_cells = 60, 5
    transcripts = np.zeros(n_tx, dtype=[('transcript_id', 'S8'), ('gene_id', 'S6'), ('length', 'f8')])
    transcripts['gene_id'] = [b'' if t % 11 == 0 else b'G%03d' % (t // 9 if t % 2 else 6 - t // 9) for t in range(n_tx)]
    index = types.SimpleNamespace(transcripts=transcripts)
    profile = rng.gamma(0.5, 200.0, size=(2, n_tx))
    tpm = np.stack([profile[c % 2] * rng.uniform(0.5, 1.5, n_tx) for c in range(n_cells)])
    matrix, genes = impute.gene_matrix(index, tpm)
    all_genes, inverse = np.unique(transcripts['gene_id'], return_inverse=True)
    expected = np.zeros((n_cells, len(all_genes)), dtype='i8')
    for g in range(len(all_genes)):
        expected[:, g] = tpm[:, inverse == g].sum(axis=1)
    np.testing.assert_array_equal(matrix, expected[:, all_genes != b''])
    assert genes.tolist() == all_genes[all_genes != b''].tolist()

    weights = impute.cell_weights(index, tpm, seed=0)
    corr = np.corrcoef(matrix)
    assert weights.shape == (n_cells, n_cells)
    kept = weights != 0
    np.testing.assert_array_equal(weights[kept], corr[kept])      # kept values are the correlations
    assert kept.diagonal().all()                                   # r = 1 sits in the upper cluster
    off = corr[~np.eye(n_cells, dtype=bool)]
    assert corr[kept].min() > off[~kept[~np.eye(n_cells, dtype=bool)]].max()   # a threshold cut

    summaries = []
    for c in range(n_cells):
        n_classes = int(rng.integers(3, 8))
        sizes = rng.integers(1, 4, n_classes)
        class_map = np.vstack([np.repeat(np.arange(n_classes), sizes),
                               rng.integers(0, n_tx, sizes.sum())]).astype(np.int64)
        summaries.append(types.SimpleNamespace(class_map=class_map,
                                               class_count=rng.integers(1, 50, n_classes).astype('f8')))
    offsets, targets, counts = impute.blend(summaries, weights ** 3)
    assert offsets[-1] == targets.size == sum(s.class_map.shape[1] for s in summaries)
    np.testing.assert_array_equal(targets, np.concatenate([s.class_map[1] for s in summaries]))
    np.testing.assert_array_equal(np.diff(offsets),
                                  np.concatenate([np.bincount(s.class_map[0]) for s in summaries]))
    w = weights ** 3
    for i in range(n_cells):
        total_i = summaries[i].class_count.sum()
        naive = np.concatenate([s.class_count * w[i, j] * total_i / s.class_count.sum()
                                for j, s in enumerate(summaries)])
        np.testing.assert_array_equal(counts[i], naive)
    with pytest.raises(ValueError):
        impute.blend(summaries + [types.SimpleNamespace(class_map=np.zeros((2, 0), np.int64),
                                                        class_count=np.zeros(0))], np.ones((6, 6)))



# ---- map_reads / map_multiple_samples: a failing worker must fail the call (device errors are
# real here, unlike in the reference's CPU workers; round-1 advisor finding)
class _StubResult:
    def __init__(self, index, readmap=None, device=0):
        self.readmap = readmap
        self.index = index
        self.batches = 0

    def sync(self):
        pass


@pytest.mark.timeout(60)
@pytest.mark.parametrize('job_count', [1, 3])
def test_map_reads_reraises_a_worker_failure(native_libs, monkeypatch, job_count):
    import threading
    from seekmer_amd import _native, common, mapper
    lock = threading.Lock()

    def map_batch(self, batch):
        with lock:
            self.map_result.batches += 1
            if self.map_result.batches == 2:
                raise _native.NativeError(2, 'skm_mapper_map_batch: GPU out of memory (stub)')
    monkeypatch.setattr(mapper, 'MapResult', _StubResult)
    monkeypatch.setattr(mapper.ReadMapper, 'map_batch_async', map_batch)
    batches = [common.ReadBatch.from_lists(1, [b'r'], [b'ACGT' * 10]) for _ in range(40)]
    with pytest.raises(_native.NativeError):
        mapper.map_reads(object(), iter(batches), job_count=job_count)
    # and without a failure every batch is consumed
    monkeypatch.setattr(mapper.ReadMapper, 'map_batch_async',
                        lambda self, batch: setattr(self.map_result, 'batches', self.map_result.batches + 1))
    done = mapper.map_reads(object(), iter(batches), job_count=1)
    assert done.batches == 40
    with pytest.raises(_native.NativeError):
        monkeypatch.setattr(mapper.ReadMapper, 'map_batch_async', map_batch)
        mapper.map_multiple_samples(object(), [iter(batches[:3]), iter(batches[:1])], job_count=2)


@pytest.mark.timeout(120)
@pytest.mark.parametrize('paired', [True, False])
def test_parallel_fastq_engine_equals_sequential(native_libs, tmp_path, paired):
    """The parallel engine of the native reader (memory-mapped files, newline index, whole
    batches parsed side by side) hands out exactly the batches of the sequential engine --
    ragged read lengths, CRLF, padding blanks, a quality line that starts with '@', several
    files with a batch carried across the file boundary, a last line without newline -- and
    files it cannot split exactly (line count not a multiple of four) fall back silently."""
    from seekmer_amd import common
    rng = np.random.default_rng(12)

    def write(path, n, mate, last_newline=True):
        lines = []
        for i in range(n):
            m = int(rng.integers(25, 160))
            seq = bytes(rng.choice(list(b'ACGTNacgt'), m).astype(np.uint8))
            eol = b'\r\n' if i % 11 == 0 else b'\n'
            qual = (b'@' if i % 5 == 0 else b'I') + b'I' * (m - 1)
            lines += [b'@r%d/%d some text' % (i, mate) + eol, (b' ' if i % 7 == 0 else b'') + seq + eol,
                      b'+' + eol, qual + eol]
        text = b''.join(lines)
        path.write_bytes(text if last_newline else text.rstrip(b'\r\n'))

    counts = (3001, 1777)
    paths = []
    for f, n in enumerate(counts):
        for mate in ((1, 2) if paired else (1,)):
            path = tmp_path / ('s%d_%d.fastq' % (f, mate))
            write(path, n, mate, last_newline=not (f == 1 and mate == 1))
            paths.append(path)
    sequential = [(b.count, b.names, b.reads, b.first_unit) for b in
                  common.NativeReadFeeder(paths, paired=paired, batch_units=700)]
    feeder = common.NativeReadFeeder(paths, paired=paired, batch_units=700, threads=3)
    parallel = [(b.count, b.names, b.reads, b.first_unit) for b in feeder]
    assert feeder.parallel is True
    assert parallel == sequential
    assert all(b.uniform_len is None for b in common.NativeReadFeeder(paths, paired=paired, batch_units=700,
                                                                      threads=3))     # ragged reads
    assert [p[0] for p in parallel] == [700] * 6 + [sum(counts) - 4200]
    assert [p[3] for p in parallel] == [700 * k for k in range(7)]
    # leaving the loop early with workers in flight must not hang or leak
    it = iter(common.NativeReadFeeder(paths, paired=paired, batch_units=100, threads=4))
    assert next(it).count == 100
    it.close()
    # a file with a dangling name line: not splittable exactly -> sequential engine, same result
    width = 2 if paired else 1                      # (zip() stops at the shorter file: both mates dangle)
    others = list(paths)
    for mate in range(width):
        ragged = tmp_path / ('ragged_%d.fastq' % (mate + 1))
        ragged.write_bytes(paths[mate].read_bytes() + b'@dangling\n')
        others[mate] = ragged
    feeder = common.NativeReadFeeder(others, paired=paired, batch_units=700, threads=3)
    got = [(b.count, b.reads) for b in feeder]
    assert feeder.parallel is False
    assert got == [(b.count, b.reads) for b in common.NativeReadFeeder(others, paired=paired, batch_units=700)]


@pytest.mark.parametrize('threads', [0, 3])
def test_sharded_feeders_partition_the_sample(native_libs, tmp_path, threads):
    """shard=(rank, world): the feeders of the ranks hand out disjoint batches whose union, put
    back in first_unit order, is the unsharded sequence of batches (both engines)."""
    from seekmer_amd import common
    lines = []
    for i in range(2300):
        lines += [b'@r%d\n' % i, b'ACGT' * 8 + b'%04d' % i + b'\n', b'+\n', b'I' * 36 + b'\n']
    path = tmp_path / 'r.fastq'
    path.write_bytes(b''.join(lines))
    whole = [(b.first_unit, b.count, b.reads) for b in
             common.NativeReadFeeder([path], paired=False, batch_units=300, threads=threads)]
    assert [w[0] for w in whole] == [300 * k for k in range(8)]
    # every read is 36 bases long: the batches say so (they can be handed over without offsets)
    assert [b.uniform_len for b in common.NativeReadFeeder([path], paired=False, batch_units=300,
                                                           threads=threads)] == [36] * 8
    for world in (2, 3, 9):
        parts = []
        for rank in range(world):
            mine = [(b.first_unit, b.count, b.reads) for b in
                    common.NativeReadFeeder([path], paired=False, batch_units=300, threads=threads,
                                            shard=(rank, world))]
            assert [m[0] // 300 % world for m in mine] == [rank] * len(mine)
            parts += mine
        assert sorted(parts) == whole


def test_infer_chooses_its_reader(tmp_path):
    """infer._feeder: plain files go through the one-pass packed reader (a rank of several: over its
    share of the sample, given the ranks' all-reduce); compressed input and -m (readmap.txt in the
    reference's batches) keep the ASCII reader."""
    import gzip
    from seekmer_amd import common, infer
    plain = [tmp_path / 'a_1.fastq', tmp_path / 'a_2.fastq']
    for path in plain:
        path.write_bytes(b'@r\nACGT\n+\nIIII\n')
    packed = tmp_path / 'b_1.fastq.gz'
    with gzip.open(packed, 'wb') as f:
        f.write(b'@r\nACGT\n+\nIIII\n')
    chosen = infer._feeder(plain, True, None, None, False)
    assert isinstance(chosen, common.PackedReadFeeder) and chosen.paired and 1 <= chosen.threads <= 16
    assert isinstance(infer._feeder(plain, True, 3, (0, 1), False), common.PackedReadFeeder)
    assert isinstance(infer._feeder(plain, True, None, None, True), common.NativeReadFeeder)       # -m
    assert isinstance(infer._feeder(plain, True, None, (1, 2), False), common.NativeReadFeeder)    # a rank of two, no exchange
    shared = infer._feeder(plain, True, None, (1, 2), False, sum_over_ranks=lambda table: table)     # ... with one
    assert isinstance(shared, common.PackedReadFeeder) and shared.shard == (1, 2)
    assert isinstance(infer._feeder([packed, plain[1]], True, None, None, False), common.NativeReadFeeder)
    assert isinstance(infer._feeder(plain, True, 0, None, False), common.NativeReadFeeder)         # --parse-threads 0
    assert common.PackedReadFeeder.eligible(plain) and not common.PackedReadFeeder.eligible([packed])
    # the reader's pieces of this tiny sample: one read per stream
    pieces = [(p.stream, p.first_read, p.n_reads, p.lengths.tolist()) for p in chosen]
    assert sorted(pieces) == [(0, 0, 1, [4]), (1, 0, 1, [4])]
