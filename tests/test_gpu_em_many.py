"""Many EM problems on one class structure (skm_quant_em_many, skm_quant_em_blend; skm_em_batch.hip)
against the same problems run one at a time on the same handle with skm_quant_set_counts +
skm_quant_em: results and step counts bit for bit, whatever the neighbours of a problem in the working
set of eight are and whenever it starts -- and the second round of `impute` on top of it against the
loop over the cells that SKM_IMPUTE_SERIAL=1 keeps."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOTS = 'SKM_EM_MANY_SLOTS'
WHOLE_TABLE = 'SKM_EM_NO_COMPONENTS'
SERIAL = 'SKM_IMPUTE_SERIAL'


@pytest.fixture(autouse=True)
def _switches_off_by_default(monkeypatch):
    for name in (SLOTS, WHOLE_TABLE, SERIAL, 'SKM_BOOTSTRAP_CHUNK'):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope='module')
def mapped_table(native_libs):
    """BASELINE.json configs[0] in size: the 1k-transcript synthetic index, 100k 2x75 pairs mapped on the GPU."""
    from seekmer_amd import common, index_builder, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(1, 100)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 100000
    bases, offsets = synth.reads(1, pool, tx_offsets, 0, n_units, 75, True)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
    summarized = result.summarize()
    class_offsets, class_targets, counts, _, _ = result.export()
    np.testing.assert_array_equal(counts, summarized.class_count)
    l = summarized.effective_lengths.astype('f8')
    x0 = 1.0 / l
    x0 /= x0.sum()
    return len(ids), class_offsets, class_targets, counts.astype('f8'), x0, l, summarized


def _count_vectors(counts, k, seed):
    """The observed counts, then k - 1 vectors of them scaled class by class by random positive factors
    (spread over up to three decades) with 0-60 % of the classes zeroed."""
    rng = np.random.default_rng(seed)
    rows = [counts.astype('f8')]
    for _ in range(k - 1):
        row = counts * rng.uniform(0.05, 20.0, counts.size) ** rng.uniform(0.0, 2.0)
        row[rng.random(counts.size) < rng.uniform(0.0, 0.6)] = 0.0
        rows.append(row)
    return np.asarray(rows)


def _one_by_one(quant, rows, x0, l, own):
    """Today's path: set_counts + em for every row; the handle gets its own counts back."""
    results, steps = [], []
    for row in rows:
        quant.set_counts(row)
        x, it = quant.em(x0, l)
        results.append(x)
        steps.append(it)
    quant.set_counts(own)
    return np.asarray(results).reshape(len(rows), x0.size), np.asarray(steps, dtype=np.int64)


def _check_many(quant, rows, x0, l, expected, steps):
    from seekmer_amd import infer
    out, iters = quant.em_many(rows, x0, l)
    np.testing.assert_array_equal(iters, steps)
    np.testing.assert_array_equal(out, expected)
    tpm, iters_tpm = quant.em_many(rows, x0, l, tpm=True)
    np.testing.assert_array_equal(iters_tpm, steps)
    np.testing.assert_array_equal(tpm, np.asarray([infer._tpm(x.copy()) for x in expected]).reshape(expected.shape))


@pytest.mark.parametrize('k', [1, 7, 8, 9, 29])
def test_many_equals_one_by_one(mapped_table, monkeypatch, k):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l, _ = mapped_table
    rows = _count_vectors(counts, k, 100 + k)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        own, own_steps = quant.em(x0, l)
        expected, steps = _one_by_one(quant, rows, x0, l, counts)
        print('K = %d: steps one by one %s' % (k, steps.tolist()))
        if k > 1:
            assert len(set(steps.tolist())) >= 2             # (else no place is refilled while others run)
        _check_many(quant, rows, x0, l, expected, steps)
        # several groups (a place is refilled across a group's edge: the next group starts afresh)
        monkeypatch.setenv(SLOTS, '3')
        _check_many(quant, rows, x0, l, expected, steps)
        monkeypatch.delenv(SLOTS)
        # the single-problem EM that the tail of a group is handed to steps the whole table
        monkeypatch.setenv(WHOLE_TABLE, '1')
        whole, whole_steps = _one_by_one(quant, rows, x0, l, counts)
        np.testing.assert_array_equal(whole_steps, steps)
        np.testing.assert_array_equal(whole, expected)
        _check_many(quant, rows, x0, l, expected, steps)
        monkeypatch.setenv(SLOTS, '3')
        _check_many(quant, rows, x0, l, expected, steps)
        monkeypatch.delenv(SLOTS)
        monkeypatch.delenv(WHOLE_TABLE)
        # the handle holds its own counts again
        again, again_steps = quant.em(x0, l)
        assert again_steps == own_steps
        np.testing.assert_array_equal(again, own)
        np.testing.assert_array_equal(expected[0], own)       # (row 0: the observed counts)
    finally:
        quant.close()


def test_quantify_many_is_quantify_per_count_vector(mapped_table):
    import copy
    from seekmer_amd import infer
    _, _, _, counts, _, _, summarized = mapped_table
    rows = _count_vectors(counts, 5, 7)
    tpm, iters = infer.quantify_many(summarized, rows, return_iters=True)
    assert tpm.shape == (5, summarized.effective_lengths.size)
    for row, got, it in zip(rows, tpm, iters):
        table = copy.copy(summarized)
        table.class_count = row
        expected, steps = infer.quantify(table, return_iters=True)
        assert steps == it
        np.testing.assert_array_equal(got, expected)
    np.testing.assert_array_equal(infer.quantify_many(summarized, rows[:2]), tpm[:2])


# ------------------------------------------------------------------------------------ impute
N_CELLS = 12


@pytest.fixture(scope='module')
def cells(native_libs, tmp_path_factory):
    """Twelve small cells of two expression profiles: their FASTQ files, an index with gene names and
    the cells' summaries after the histograms have been pooled (what impute.run hands to its second round)."""
    from seekmer_amd import common, impute, index_builder, mapper, synth
    tmp = tmp_path_factory.mktemp('cells')
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    transcripts = np.zeros(len(ids), dtype=[('transcript_id', index.transcripts.dtype['transcript_id']),
                                            ('gene_id', 'S8'), ('length', 'f8')])
    transcripts['transcript_id'] = index.transcripts['transcript_id']
    transcripts['length'] = index.transcripts['length']
    transcripts['gene_id'] = [b'GENE%04d' % (t // 4) for t in range(len(ids))]
    index = common.KMerIndex(index.kmers, index.contigs, index.sequences, index.targets, transcripts, index.exons)
    index_path = tmp / 'index.npz'
    index.save(index_path)
    n_units, read_len, paths, results = 4000, 75, [], []
    for cell in range(N_CELLS):
        bases, offsets = synth.reads(100 + cell % 2, pool, tx_offsets, cell * n_units, n_units, read_len, True)
        reads = bases[:-1].reshape(n_units, 2, read_len)
        for mate in (0, 1):
            path = tmp / ('cell%d_%d.fastq' % (cell, mate + 1))
            path.write_bytes(b''.join(b'@c%d/%d\n%s\n+\n%s\n' % (i, mate + 1, reads[i, mate].tobytes(), b'I' * read_len)
                                      for i in range(n_units)))
            paths.append(path)
        result = mapper.MapResult(index)
        mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
        results.append(result)
    impute.pool_fragment_lengths(results)
    summaries = [result.summarize() for result in results]
    return index_path, paths, summaries


def _weights(n, seed):
    """Ones on the diagonal, zeros between the two profiles (and a few inside them), anything in (0, 1) elsewhere."""
    rng = np.random.default_rng(seed)
    weight = rng.uniform(0.05, 1.0, (n, n)) ** 4
    profile = np.arange(n) % 2
    weight[profile[:, None] != profile[None, :]] = 0.0
    weight[rng.random((n, n)) < 0.1] = 0.0
    weight[np.arange(n), np.arange(n)] = 1.0
    assert (weight == 0).any() and ((weight > 0) & (weight < 1)).any()
    return weight


def test_blended_counts_are_made_on_the_device(cells, monkeypatch):
    from seekmer_amd import impute, infer
    _, _, summaries = cells
    weight = _weights(N_CELLS, 3)
    offsets, targets, counts = impute.blend(summaries, weight)
    counts = np.asarray(counts)
    own, class_cell, cell_total = impute.blend_sources(summaries)
    l = summaries[0].effective_lengths.astype('f8')
    x0 = 1.0 / l
    x0 /= x0.sum()
    quant = infer._QuantHandle.from_csr(l.size, offsets, targets, own)
    try:
        for slots in (None, '5'):
            if slots:
                monkeypatch.setenv(SLOTS, slots)
            out, iters, made = quant.em_blend(class_cell, weight, cell_total, x0, l, want_counts=True)
            assert np.array_equal(made, counts)
            expected, steps = quant.em_many(counts, x0, l)
            np.testing.assert_array_equal(iters, steps)
            np.testing.assert_array_equal(out, expected)
            tpm, iters_tpm, _ = quant.em_blend(class_cell, weight, cell_total, x0, l, tpm=True)
            np.testing.assert_array_equal(iters_tpm, steps)
            np.testing.assert_array_equal(tpm, quant.em_many(counts, x0, l, tpm=True)[0])
        monkeypatch.delenv(SLOTS)
        one_by_one, steps_one = _one_by_one(quant, counts, x0, l, own)
        np.testing.assert_array_equal(steps, steps_one)
        np.testing.assert_array_equal(expected, one_by_one)
        with pytest.raises(ValueError):                            # a class of a cell that does not exist
            quant.em_blend(np.where(np.arange(class_cell.size) == 3, N_CELLS, class_cell), weight, cell_total, x0, l)
    finally:
        quant.close()


def test_impute_second_round_batched_equals_serial(cells, monkeypatch, tmp_path):
    from seekmer_amd import impute
    from seekmer_amd.__main__ import main
    from seekmer_amd import infer
    index_path, paths, summaries = cells
    weight = _weights(N_CELLS, 4)
    # which form ran: every em_blend call and every one-by-one EM is counted
    calls = {'em_blend': 0, 'em': 0}
    real_blend, real_em = infer._QuantHandle.em_blend, infer._QuantHandle.em

    def counted_blend(self, *a, **k):
        calls['em_blend'] += 1
        return real_blend(self, *a, **k)

    def counted_em(self, *a, **k):
        calls['em'] += 1
        return real_em(self, *a, **k)

    monkeypatch.setattr(infer._QuantHandle, 'em_blend', counted_blend)
    monkeypatch.setattr(infer._QuantHandle, 'em', counted_em)
    for other in summaries[1:]:                                   # (after pooling: what the batched path requires)
        np.testing.assert_array_equal(other.effective_lengths, summaries[0].effective_lengths)
    batched = impute.requantify_blend(summaries, weight)
    assert calls == {'em_blend': 1, 'em': 0}
    monkeypatch.setenv(SERIAL, '1')
    serial = impute.requantify_blend(summaries, weight)
    monkeypatch.delenv(SERIAL)
    assert calls == {'em_blend': 1, 'em': N_CELLS}
    assert len(batched) == len(serial) == N_CELLS
    for got, expected in zip(batched, serial):
        assert got.any()
        np.testing.assert_array_equal(got, expected)
    # through the CLI: the same bytes
    arguments = ['impute', str(index_path), None, *map(str, paths), '-p', '4', '--seed', '0']
    arguments[2] = str(tmp_path / 'batched')
    assert main(arguments) == 0
    assert calls['em_blend'] == 2                                  # (the second round of this run was the batched one)
    before = calls['em']
    monkeypatch.setenv(SERIAL, '1')
    arguments[2] = str(tmp_path / 'serial')
    assert main(arguments) == 0
    monkeypatch.delenv(SERIAL)
    assert calls["em_blend"] == 2 and calls["em"] == before + 2 * N_CELLS   # (both rounds one cell at a time)
    one, other = (tmp_path / 'batched' / 'tpm.csv').read_bytes(), (tmp_path / 'serial' / 'tpm.csv').read_bytes()
    assert len(one) > 1000 and one == other
    assert (tmp_path / 'batched' / 'weight.csv').read_bytes() == (tmp_path / 'serial' / 'weight.csv').read_bytes()


# ------------------------------------------------------------------------------------ edges
def test_an_undefined_problem_among_good_ones(mapped_table, monkeypatch):
    from seekmer_amd import _native, infer
    n_tx, offsets, targets, counts, x0, l, _ = mapped_table
    rows = _count_vectors(counts, 11, 5)
    rows[6] = 0.0
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        own, own_steps = quant.em(x0, l)
        for slots in (None, '1', '4'):
            if slots:
                monkeypatch.setenv(SLOTS, slots)
            with pytest.raises(_native.NativeError) as raised:
                quant.em_many(rows, x0, l)
            assert raised.value.code == _native.SKM_ERR_UNDEFINED
            again, again_steps = quant.em(x0, l)                      # its own counts, unchanged bits
            assert again_steps == own_steps
            np.testing.assert_array_equal(again, own)
        monkeypatch.delenv(SLOTS)
        quant.set_counts(rows[6])
        with pytest.raises(_native.NativeError) as raised:            # (as the loop over the vectors would raise there)
            quant.em(x0, l)
        assert raised.value.code == _native.SKM_ERR_UNDEFINED
    finally:
        quant.close()


def test_no_problem_at_all(mapped_table):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l, _ = mapped_table
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        out, iters = quant.em_many(np.zeros((0, counts.size)), x0, l)
        assert out.shape == (0, n_tx) and iters.size == 0
        with pytest.raises(ValueError):
            quant.em_many(np.zeros((2, counts.size + 1)), x0, l)
        hip = infer._native.hip()
        assert hip.skm_quant_em_many(quant.handle, -1, None, None, None, 0.01, 1e-8, 0, None, None) == infer._native.SKM_ERR_ARG
        assert hip.skm_quant_em_many(quant.handle, 0, None, None, None, 0.01, 1e-8, 0, None, None) == infer._native.SKM_OK
        assert hip.skm_quant_em_many(quant.handle, 1, None, None, None, 0.01, 1e-8, 0, None, None) == infer._native.SKM_ERR_ARG
    finally:
        quant.close()


def test_through_a_one_rank_communicator(mapped_table, cells):
    """With a communicator attached the problems go one by one through the single-problem EM and its
    all-reduces (a sum over one rank is the identity): the same bits and step counts.  For em_blend that
    path writes every cell's row straight into the handle's counts, after the cells' own counts were
    taken from there -- and puts the own counts back."""
    from seekmer_amd import _native, impute, infer, parallel
    n_tx, offsets, targets, counts, x0, l, _ = mapped_table
    rows = _count_vectors(counts, 9, 21)
    hip = _native.hip()
    raw = ctypes.create_string_buffer(128)
    _native.check(hip.skm_comm_unique_id(raw))
    comm = parallel.create_comm(0, raw.raw, 0, 1)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        plain, steps = quant.em_many(rows, x0, l)
        plain_tpm, _ = quant.em_many(rows, x0, l, tpm=True)
        _native.check(hip.skm_quant_set_comm(quant.handle, comm))
        through, steps_through = quant.em_many(rows, x0, l)
        through_tpm, _ = quant.em_many(rows, x0, l, tpm=True)
        _native.check(hip.skm_quant_set_comm(quant.handle, None))
        np.testing.assert_array_equal(steps_through, steps)
        np.testing.assert_array_equal(through, plain)
        np.testing.assert_array_equal(through_tpm, plain_tpm)
        # the blended problem
        _, _, summaries = cells
        weight = _weights(N_CELLS, 9)
        blend_offsets, blend_targets, blended = impute.blend(summaries, weight)
        own, class_cell, cell_total = impute.blend_sources(summaries)
        bl = summaries[0].effective_lengths.astype('f8')
        bx0 = 1.0 / bl
        bx0 /= bx0.sum()
        blend_quant = infer._QuantHandle.from_csr(bl.size, blend_offsets, blend_targets, own)
        try:
            plain, steps, _ = blend_quant.em_blend(class_cell, weight, cell_total, bx0, bl)
            own_result, own_steps = blend_quant.em(bx0, bl)
            _native.check(hip.skm_quant_set_comm(blend_quant.handle, comm))
            for _ in range(2):                                     # (the second call starts from restored own counts)
                through, steps_through, made = blend_quant.em_blend(class_cell, weight, cell_total, bx0, bl, want_counts=True)
                np.testing.assert_array_equal(steps_through, steps)
                np.testing.assert_array_equal(through, plain)
                assert np.array_equal(made, np.asarray(blended))
            _native.check(hip.skm_quant_set_comm(blend_quant.handle, None))
            again, again_steps = blend_quant.em(bx0, bl)
            assert again_steps == own_steps
            np.testing.assert_array_equal(again, own_result)
        finally:
            blend_quant.close()
    finally:
        quant.close()
        parallel.destroy_comm(comm)
