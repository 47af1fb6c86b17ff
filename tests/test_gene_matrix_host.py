"""The count matrix without a GPU: the plain-Python reference against the dense gene reference, the refusals of
`infer-many --matrix-only` that come before anything is loaded, and the writer of output/counts/."""
import pathlib

import numpy as np
import pytest

import gene_matrix_reference as mref
import gene_reference as ref


def _random_table(rng, n_classes, n_samples, n_tx, n_genes):
    """(offsets, targets, counts, sample, tx_gene): classes of 0 to 12 ids, most of them inside one gene's
    neighbourhood so that all three kinds occur; some counts are 0"""
    tx_gene = np.sort(np.where(rng.uniform(0, 1, n_tx) < 0.15, -1, rng.integers(0, n_genes, n_tx))).astype(np.int32)
    lengths = rng.integers(0, 13, n_classes)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    targets = np.zeros(offsets[-1], dtype=np.int32)
    for c in range(n_classes):
        near = int(rng.integers(n_tx))
        spread = int(rng.choice([1, 3, 40]))
        targets[offsets[c]:offsets[c + 1]] = np.clip(near + rng.integers(0, spread, lengths[c]), 0, n_tx - 1)
    counts = (rng.integers(0, 1000, n_classes) * (rng.uniform(0, 1, n_classes) > 0.1)).astype(np.int64)
    sample = rng.integers(0, n_samples, n_classes).astype(np.int32)
    return offsets, targets, counts, sample, tx_gene


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_reference_densified_is_the_dense_reference(seed):
    rng = np.random.default_rng(seed)
    n_samples, n_genes = 7, 30
    offsets, targets, counts, sample, tx_gene = _random_table(rng, 600, n_samples, 400, n_genes)
    indptr, indices, data, other = mref.matrix(offsets, targets, counts, tx_gene, sample, n_samples)
    mref.check_csr(indptr, indices, data, n_samples, n_genes)
    want_unique, want_other = ref.unique_counts(offsets, targets, counts, tx_gene, n_genes, sample, n_samples)
    np.testing.assert_array_equal(mref.dense(indptr, indices, data, n_genes), want_unique)
    np.testing.assert_array_equal(other, want_other)
    assert indptr[-1] == np.count_nonzero(want_unique) and 0 < indptr[-1] < want_unique.size
    assert data.sum() + other.sum() == counts.sum() and other.sum(axis=0).min() > 0
    # one sample, no class_sample
    indptr, indices, data, other = mref.matrix(offsets, targets, counts, tx_gene)
    want_unique, want_other = ref.unique_counts(offsets, targets, counts, tx_gene, n_genes)
    np.testing.assert_array_equal(mref.dense(indptr, indices, data, n_genes), want_unique)
    np.testing.assert_array_equal(other, want_other)


@pytest.mark.parametrize('options, word', [(['-b', '2'], '-b N'), (['--bias'], '--bias'), (['--genes'], '--genes')])
def test_matrix_only_refuses_what_needs_the_em_before_anything_is_loaded(tmp_path, options, word):
    """neither the index nor a read file exists: the refusal is the first thing that happens"""
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    missing = [str(tmp_path / name) for name in ('no_index.npz', 'no_1.fastq', 'no_2.fastq')]
    with pytest.raises(ValueError) as refused:
        cli.main(['infer-many', missing[0], str(tmp_path / 'out'), *missing[1:], '--matrix-only', *options])
    assert str(refused.value) == infer.MATRIX_ONLY_NEEDS_EM % word and 'EM' in str(refused.value)
    assert not (tmp_path / 'out').exists()


def test_matrix_only_refusals_through_run_many_and_the_parsed_options(tmp_path):
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    missing = [pathlib.Path(tmp_path / name) for name in ('no_index.npz', 'no_1.fastq', 'no_2.fastq')]
    for keywords in ({'bootstrap': 1}, {'bias': True}, {'genes': True}):
        arguments = dict(job_count=1, single_ended=False, bootstrap=0, debug=False, matrix_only=True)
        arguments.update(keywords)
        with pytest.raises(ValueError, match='needs the EM'):
            infer.run_many(missing[0], tmp_path / 'out', missing[1:], **arguments)
    assert not (tmp_path / 'out').exists()
    # --matrix-only implies --count-matrix; with either, --gene-map serves the matrix and does not imply --genes
    base = ['infer-many', 'index', 'out', 'a_1.fastq', 'a_2.fastq']
    opts = cli.parse_args(base + ['--matrix-only', '--gene-map', 'map.tsv'])
    assert opts['matrix_only'] and opts['count_matrix'] and not opts['genes'] and opts['gene_map'] == pathlib.Path('map.tsv')
    opts = cli.parse_args(base + ['--count-matrix', '--gene-map', 'map.tsv'])
    assert not opts['matrix_only'] and opts['count_matrix'] and not opts['genes']
    opts = cli.parse_args(base + ['--count-matrix', '--genes'])
    assert opts['count_matrix'] and opts['genes']
    opts = cli.parse_args(base + ['--gene-map', 'map.tsv'])
    assert not opts['count_matrix'] and not opts['matrix_only'] and opts['genes']
    # infer and impute take neither option
    for command in (['infer', 'index', 'out', 'a_1.fastq', 'a_2.fastq'],):
        with pytest.raises(SystemExit):
            cli.parse_args(command + ['--count-matrix'])
        with pytest.raises(SystemExit):
            cli.parse_args(command + ['--matrix-only'])


@pytest.mark.parametrize('option', ['--count-matrix', '--matrix-only'])
def test_count_matrix_without_genes_is_refused_before_a_read_file_is_opened(native_libs, tmp_path, monkeypatch, option):
    """An index without genes and no --gene-map: NO_GENES.  Whether an index has genes is known once it is loaded, which
    run_many does after it has named the device to the page-locked allocator; without a GPU that one call fails, so
    its status is let through here.  The read files exist (run_many checks that first) but hold no FASTQ record: a
    run that opened them would fail in another way."""
    from seekmer_amd import __main__ as cli
    from seekmer_amd import index_builder, infer, synth
    index_path = tmp_path / 'index.npz'
    index_builder.build_pooled(*synth.transcriptome(3, 5)).save(index_path)
    reads = [tmp_path / 'a_1.fastq', tmp_path / 'a_2.fastq', tmp_path / 'b_1.fastq', tmp_path / 'b_2.fastq']
    for path in reads:
        path.write_text('not a read file\n')
    monkeypatch.setattr(infer._native, 'check', lambda code: None)
    with pytest.raises(ValueError) as refused:
        cli.main(['infer-many', str(index_path), str(tmp_path / 'out'), *map(str, reads), option])
    assert str(refused.value) == infer.NO_GENES
    assert list((tmp_path / 'out').iterdir()) == []


def test_the_writer_round_trips(tmp_path):
    from seekmer_amd import infer
    rng = np.random.default_rng(11)
    n_samples, n_genes = 6, 70001
    offsets, targets, counts, sample, tx_gene = _random_table(rng, 400, n_samples, 300, 25)
    tx_gene = np.where(tx_gene == 24, n_genes - 1, tx_gene).astype(np.int32)         # (a gene number above 2^16)
    sample[sample == 3] = 2                                                         # (sample 3 has an empty row)
    inside = [c for c in range(counts.size) if offsets[c + 1] > offsets[c]
              and tx_gene[targets[offsets[c]]] >= 0 and len(set(tx_gene[targets[offsets[c]:offsets[c + 1]]].tolist())) == 1]
    counts[inside[0]] = 1 << 40                                                     # (a count that needs 64 bits)
    indptr, indices, data, other = mref.matrix(offsets, targets, counts, tx_gene, sample, n_samples)
    assert indptr[3] == indptr[4] and indices.max() == n_genes - 1 and data.max() >= 1 << 40
    gene_ids = np.asarray([b'G%06d' % g for g in range(n_genes)])
    names = ['cell%d' % s for s in range(n_samples)]
    units = [int(data[indptr[s]:indptr[s + 1]].sum() + other[s].sum()) + 10 * s for s in range(n_samples)]
    infer.output_count_matrix(tmp_path, gene_ids, names, units, indptr, indices, data, other)
    counts_path = tmp_path / 'counts'
    assert sorted(f.name for f in counts_path.iterdir()) == ['cells.tsv', 'genes.tsv', 'matrix.mtx', 'matrix.npz']
    lines = (counts_path / 'matrix.mtx').read_text().splitlines(keepends=True)
    assert lines == mref.mtx_lines(indptr, indices, data, n_genes, infer.COUNT_MATRIX_COMMENT)
    got_genes, comment, got_indptr, got_indices, got_data = mref.parse_mtx(lines)
    assert got_genes == n_genes and '--count-matrix' in comment and 'rows are genes' in comment and 'columns are cells' in comment
    for got, want in ((got_indptr, indptr), (got_indices, indices), (got_data, data)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert (counts_path / 'genes.tsv').read_text().splitlines() == [g.decode() for g in gene_ids]
    cells = (counts_path / 'cells.tsv').read_text().splitlines(keepends=True)
    assert cells == mref.cells_lines(names, units, indptr, data, other)
    for line, total in zip(cells, units):
        fields = line.split('\t')
        assert int(fields[1]) == total and int(fields[3]) + int(fields[4]) + int(fields[5]) == int(fields[2])
    arrays = np.load(counts_path / 'matrix.npz')
    assert sorted(arrays.files) == ['data', 'format', 'indices', 'indptr', 'shape']
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [n_samples, n_genes]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want)
    # the same arrays written again are the same bytes: the container carries no time of day
    again = tmp_path / 'again'
    again.mkdir()
    infer.output_count_matrix(again, gene_ids, names, units, indptr, indices, data, other)
    for f in counts_path.iterdir():
        assert f.read_bytes() == (again / 'counts' / f.name).read_bytes(), f.name
    # rows one by one give the same CSR; arrays that do not fit together are refused
    rows = [(indices[indptr[s]:indptr[s + 1]], data[indptr[s]:indptr[s + 1]]) for s in range(n_samples)]
    for got, want in zip(infer.stack_count_rows(rows), (indptr, indices, data)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    with pytest.raises(ValueError):
        infer.output_count_matrix(again, gene_ids, names, units, indptr[:-1], indices, data, other)
