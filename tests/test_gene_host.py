"""Gene-level tables (--genes / --gene-map) as far as they go without a GPU: the gene map, the command line, the
table and its writer through a stub of gene_sums, the reference against plain Python loops, and the four entry
points' answer on a machine without a GPU."""
import gzip
import logging
import types

import numpy as np
import pytest

import gene_reference as ref


# ------------------------------------------------------------------------------------------------ the gene map
def _sequences(n, rng, length=120):
    return [bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, length)) for _ in range(n)]


def _index(ids, genes=None):
    """what gene_map reads of an index: its transcript table"""
    width = max(len(i) for i in ids)
    transcripts = np.zeros(len(ids), dtype=[('transcript_id', 'S%d' % width), ('gene_id', 'S8'), ('length', 'f8')])
    transcripts['transcript_id'] = ids
    if genes is not None:
        transcripts['gene_id'] = genes
    return types.SimpleNamespace(transcripts=transcripts)


def test_gene_map_from_a_built_index(native_libs):
    from seekmer_amd import index_builder, infer
    rng = np.random.default_rng(5)
    ids = [b'TX%d' % i for i in range(7)]
    exome = np.zeros(6, dtype=[('transcript_id', 'S4'), ('gene_id', 'S5'), ('exon_number', 'i4'), ('chromosome', 'S1'),
                               ('start', 'i4'), ('end', 'i4'), ('strand', '?')])
    exome['transcript_id'] = [b'TX0', b'TX0', b'TX2', b'TX3', b'TX5', b'TX9']       # TX0 twice; TX9 is not in the index
    exome['gene_id'] = [b'GB', b'GB', b'GA', b'GB', b'GC', b'GZ']
    exome['exon_number'] = [1, 2, 1, 1, 1, 1]
    index = index_builder.build(ids, _sequences(7, rng), exome)
    np.testing.assert_array_equal(index.transcripts['gene_id'], [b'GB', b'', b'GA', b'GB', b'', b'GC', b''])
    gene_ids, tx_gene = infer.gene_map(index)
    assert gene_ids.dtype.kind == 'S' and gene_ids.tolist() == [b'GA', b'GB', b'GC']
    assert tx_gene.dtype == np.int32 and tx_gene.tolist() == [1, -1, 0, 1, -1, 2, -1]
    want_ids, want = ref.gene_map_from_ids(index.transcripts['gene_id'])
    np.testing.assert_array_equal(gene_ids, want_ids)
    np.testing.assert_array_equal(tx_gene, want)
    # an index built without an annotation has no genes
    with pytest.raises(ValueError) as error:
        infer.gene_map(index_builder.build(ids, _sequences(7, rng)))
    assert 'GTF' in str(error.value) and '--gene-map' in str(error.value)


MAP_LINES = [b'# transcript\tgene\n', b'TX1.4\tGB\n', b'TX0\tGC\textra column\n', b'\n', b'TX3.1.2\tGA\n', b'NOPE.1\tGQ\n',
             b'#TX2\tGX\n', b'TX1\tGB\r\n', b'ELSE\tGQ\n', b'TX4\tGB\n']


@pytest.mark.parametrize('compressed', [False, True], ids=['plain', 'gzip'])
def test_gene_map_from_a_file(tmp_path, caplog, compressed):
    from seekmer_amd import infer
    ids = [b'TX0', b'TX1', b'TX2', b'TX3', b'TX4']
    index = _index(ids, [b'IGNORED'] * 5)                         # (with a file the index's own genes are not read)
    path = tmp_path / ('genes.tsv.gz' if compressed else 'genes.tsv')
    (gzip.open if compressed else open)(path, 'wb').write(b''.join(MAP_LINES))
    with caplog.at_level(logging.INFO):
        gene_ids, tx_gene = infer.gene_map(index, path)
    assert gene_ids.tolist() == [b'GA', b'GB', b'GC'] and tx_gene.tolist() == [2, 1, -1, 0, 1]
    genes, unknown = ref.parse_gene_map(MAP_LINES, ids)
    assert unknown == 2
    np.testing.assert_array_equal(tx_gene, ref.gene_map_from_ids(np.asarray(genes, dtype='S'))[1])
    said = [record.getMessage() for record in caplog.records if 'does not hold' in record.getMessage()]
    assert len(said) == 1 and ' 2 ' in said[0]                    # one line for both unknown ids


def test_gene_map_refuses_two_genes_for_one_transcript(tmp_path):
    from seekmer_amd import infer
    index = _index([b'TX0', b'TX1'])
    path = tmp_path / 'genes.tsv'
    path.write_bytes(b'TX0\tGA\nTX1.1\tGB\nTX1.2\tGC\n')
    with pytest.raises(ValueError) as error:
        infer.gene_map(index, path)
    assert 'TX1' in str(error.value) and 'GB' in str(error.value) and 'GC' in str(error.value)
    path.write_bytes(b'TX0\tGA\nTX1.1\tGB\nTX1.2\tGB\n')          # the same gene twice is no conflict
    assert infer.gene_map(index, path)[1].tolist() == [0, 1]
    path.write_bytes(b'TX0 GA\n')                                 # no tab
    with pytest.raises(ValueError):
        infer.gene_map(index, path)


def test_no_gene_at_all_is_an_error(tmp_path):
    from seekmer_amd import infer
    index = _index([b'TX0', b'TX1'])
    with pytest.raises(ValueError) as error:
        infer.gene_map(index)
    assert str(error.value) == infer.NO_GENES and 'GTF' in infer.NO_GENES and '--gene-map' in infer.NO_GENES
    path = tmp_path / 'genes.tsv'
    path.write_bytes(b'# nothing\nOTHER\tGA\n')
    with pytest.raises(ValueError) as error:
        infer.gene_map(index, path)
    assert str(error.value) == infer.NO_GENES


def test_a_run_without_genes_fails_before_any_read_file_is_opened(tmp_path, monkeypatch):
    """run_many on an index without genes: the error is gene_map's, and no reader was made."""
    from seekmer_amd import common, infer
    reads, more = tmp_path / 'reads.fastq', tmp_path / 'more.fastq'
    reads.write_bytes(b'')
    more.write_bytes(b'')
    monkeypatch.setattr(common.KMerIndex, 'load', staticmethod(lambda path: _index([b'TX0', b'TX1'])))
    monkeypatch.setattr(infer._native, 'hip', lambda: types.SimpleNamespace(skm_pinned_set_device=lambda device: 0))
    monkeypatch.setattr(infer._native, 'check', lambda code: None)

    def opened(*args, **kwargs):
        raise AssertionError('a read file was opened')
    monkeypatch.setattr(common, 'PackedReadFeeder', opened)
    monkeypatch.setattr(common, 'NativeReadFeeder', opened)
    with pytest.raises(ValueError) as error:
        infer.run_many('index', tmp_path / 'out', [reads, more], 1, True, 0, False, genes=True)
    assert str(error.value) == infer.NO_GENES


# -------------------------------------------------------------------------------------------- the command line
COMMANDS = (['infer', 'ix', 'out', 'a.fq'], ['infer-many', 'ix', 'out', 'a.fq', 'b.fq'])


@pytest.mark.parametrize('command', COMMANDS, ids=[command[0] for command in COMMANDS])
def test_gene_map_implies_genes(command):
    import pathlib
    from seekmer_amd.__main__ import parse_args
    plain = parse_args(command)
    assert plain['genes'] is False and plain['gene_map'] is None
    assert parse_args(command + ['--genes'])['genes'] is True
    mapped = parse_args(command + ['--gene-map', 'genes.tsv'])
    assert mapped['genes'] is True and mapped['gene_map'] == pathlib.Path('genes.tsv')


def test_impute_does_not_take_the_option(capsys):
    from seekmer_amd.__main__ import parse_args
    with pytest.raises(SystemExit):
        parse_args(['impute', 'ix', 'out', 'a.fq', 'b.fq', '--genes'])


def test_several_ranks_refuse_genes(tmp_path):
    from seekmer_amd import infer
    ranks = types.SimpleNamespace(world=2, rank=0, local_rank=0)
    with pytest.raises(ValueError) as error:
        infer._run(ranks, None, 'index', tmp_path / 'out', [], 1, False, False, 0, False, 0, None, None, genes=True)
    assert str(error.value) == infer.GENES_ONE_RANK and not (tmp_path / 'out').exists()


# --------------------------------------------------------------------------------- the table and its writer
def _hand_made():
    """Six transcripts: G1 = {0, 3}, G0 = {1}, G2 = {4, 5} without any tpm, transcript 2 unnamed"""
    gene_ids = np.asarray([b'G0', b'G1', b'G2'])
    tx_gene = np.asarray([1, 0, -1, 1, 2, 2], dtype=np.int32)
    length = np.asarray([1000.0, 500.0, 77.0, 3000.0, 100.0, 301.0])
    effective = np.asarray([800.5, 300.25, 10.0, 2800.125, 1.0, 102.0])
    tpm = np.asarray([250000.0, 1e-3, 600000.0, 149999.999, 0.0, 0.0])
    est = np.asarray([12.5, 1e-7, 99.0, 1234567.0, 0.0, 0.0])
    unique = np.asarray([3, 1 << 33, 0], dtype=np.int64)
    return gene_ids, tx_gene, length, effective, tpm, est, unique


def test_gene_table_through_a_stub_of_gene_sums(tmp_path, monkeypatch):
    from seekmer_amd import infer
    gene_ids, tx_gene, length, effective, tpm, est, unique = _hand_made()
    calls = []

    def stub(tx_gene, n_genes, rows, device=0):
        calls.append(np.asarray(rows).shape)
        return ref.gene_sums(tx_gene, n_genes, rows)
    monkeypatch.setattr(infer, 'gene_sums', stub)
    index = _index([b'T%d' % i for i in range(6)])
    index.transcripts['length'] = length
    results = types.SimpleNamespace(effective_lengths=effective)
    table = infer.gene_table(index, gene_ids, tx_gene, results, tpm, est, unique)
    assert calls == [(4, 6)]                                       # all sums from one call with four rows
    want = ref.gene_table(gene_ids, tx_gene, length, effective, tpm, est, unique)
    assert sorted(table) == sorted(infer.GENE_COLUMNS) == sorted(want)
    for name in infer.GENE_COLUMNS:
        np.testing.assert_array_equal(table[name], want[name], err_msg=name)
    assert table['n_transcripts'].tolist() == [1, 2, 2]
    assert table['tpm'][1] == 250000.0 + 149999.999 and table['tpm'][2] == 0      # the unnamed 600000 is nowhere
    assert table['length'][0] == 500.0
    assert table['length'][1] == (250000.0 * 1000.0 + 149999.999 * 3000.0) / (250000.0 + 149999.999)
    assert table['length'][2] == (100.0 + 301.0) / 2 and table['eff_length'][2] == (1.0 + 102.0) / 2   # no tpm: the plain mean
    infer._output_gene_table(tmp_path, table)
    lines = (tmp_path / 'abundance.genes.tsv').read_text().splitlines(keepends=True)
    assert lines == ref.gene_table_lines(want)
    assert lines[0] == 'gene_id\tn_transcripts\tlength\teff_length\test_count\ttpm\tunique_count\n'
    assert lines[1] == 'G0\t1\t500\t300.25\t1e-07\t0.001\t3\n'                    # floats as %g
    assert lines[2].startswith('G1\t2\t1750\t') and lines[2].endswith('\t1.23458e+06\t400000\t8589934592\n')
    assert lines[3] == 'G2\t2\t200.5\t51.5\t0\t0\t0\n'
    assert len(lines) == 4 and not any('77' in line or '600000' in line for line in lines)


def test_gene_table_on_a_random_table(monkeypatch):
    """500 transcripts, half of the genes without any tpm: every column is the reference's bit for bit"""
    from seekmer_amd import infer
    monkeypatch.setattr(infer, 'gene_sums', lambda tx_gene, n_genes, rows, device=0: ref.gene_sums(tx_gene, n_genes, rows))
    rng = np.random.default_rng(41)
    n_genes = 60
    tx_gene = rng.integers(-1, n_genes - 1, 500).astype(np.int32)           # (the last gene has no transcript)
    gene_ids = np.asarray([b'G%03d' % g for g in range(n_genes)])
    length = rng.integers(30, 9000, 500).astype('f8')
    effective = length * rng.uniform(0.3, 1.0, 500)
    tpm = 10.0 ** rng.uniform(-3, 5, 500) * (tx_gene % 2 == 0)              # genes of odd number have none
    est = tpm * rng.uniform(0.0, 3.0, 500)
    unique = rng.integers(0, 1 << 40, n_genes)
    index = _index([b'T%d' % i for i in range(500)])
    index.transcripts['length'] = length
    table = infer.gene_table(index, gene_ids, tx_gene, types.SimpleNamespace(effective_lengths=effective), tpm, est, unique)
    want = ref.gene_table(gene_ids, tx_gene, length, effective, tpm, est, unique)
    for name in infer.GENE_COLUMNS:
        assert table[name].dtype == want[name].dtype and table[name].tobytes() == want[name].tobytes(), name
    assert (table['tpm'] == 0).sum() > 20 and (table['length'][table['tpm'] == 0] > 0).sum() > 20
    assert table['n_transcripts'][-1] == 0 and table['length'][-1] == 0 and table['eff_length'][-1] == 0


def test_gene_matrix_writer(tmp_path):
    from seekmer_amd import infer
    infer._output_gene_matrix(tmp_path / 'm.tsv', np.asarray([b'G0', b'G1']), ['a', 'b', 'c'],
                              np.asarray([[1.5, 0.0], [1e-7, 2.0], [3e6, 1234567.0]]), '%g')
    assert (tmp_path / 'm.tsv').read_text() == 'gene_id\ta\tb\tc\nG0\t1.5\t1e-07\t3e+06\nG1\t0\t2\t1.23457e+06\n'


def test_run_info_and_arrays_gain_the_gene_entries(tmp_path, monkeypatch):
    import datetime
    import json
    from seekmer_amd import infer
    gene_ids, tx_gene, length, effective, tpm, est, unique = _hand_made()
    monkeypatch.setattr(infer, 'gene_sums', lambda tx_gene, n_genes, rows, device=0: ref.gene_sums(tx_gene, n_genes, rows))
    index = _index([b'T%d' % i for i in range(6)])
    index.transcripts['length'] = length
    aligned = int(unique.sum()) + 7 + 2
    results = types.SimpleNamespace(effective_lengths=effective, class_map=np.asarray([[0, 1], [0, 2]]),
                                    class_count=np.asarray([2.0, 3.0]), total=aligned + 5, aligned=aligned,
                                    fragment_length_frequencies=np.zeros(2000, dtype=np.int64))
    boots = [tpm * 0.5, tpm * 2.0]
    start = datetime.datetime(2020, 1, 1)
    with_genes, without = tmp_path / 'with', tmp_path / 'without'
    with_genes.mkdir(), without.mkdir()
    infer.output_results(with_genes, index, start, results, tpm, boots,
                         genes=(gene_ids, tx_gene, unique, np.asarray([7, 2], dtype=np.int64)))
    infer.output_results(without, index, start, results, tpm, boots)
    assert sorted(f.name for f in without.iterdir()) == ['abundance.npz', 'abundance.tsv', 'run_info.json']
    assert sorted(f.name for f in with_genes.iterdir()) == ['abundance.genes.tsv', 'abundance.npz', 'abundance.tsv', 'run_info.json']
    assert (with_genes / 'abundance.tsv').read_bytes() == (without / 'abundance.tsv').read_bytes()
    info, plain = json.load((with_genes / 'run_info.json').open()), json.load((without / 'run_info.json').open())
    assert info.pop('n_genes') == 3 and info.pop('n_gene_ambiguous') == 7 and info.pop('n_gene_unnamed') == 2
    assert info.pop('n_gene_unique') + 9 == info['n_pseudoaligned'] and info == plain
    a, b = np.load(with_genes / 'abundance.npz'), np.load(without / 'abundance.npz')
    for name in b.files:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), name
    gained = sorted(set(a.files) - set(b.files))
    assert gained == sorted(['genes/ids', 'genes/tpm', 'genes/est_counts', 'genes/lengths', 'genes/eff_lengths',
                             'genes/unique_counts', 'genes/bootstrap/bs0', 'genes/bootstrap/bs1'])
    np.testing.assert_array_equal(a['genes/ids'], gene_ids)
    np.testing.assert_array_equal(a['genes/unique_counts'], unique)
    for i, boot in enumerate(boots):
        np.testing.assert_array_equal(a['genes/bootstrap/bs%d' % i], ref.gene_sums(tx_gene, 3, boot)[0])


# ----------------------------------------------------------------- the reference against plain Python loops
def test_reference_sums_against_a_loop():
    rng = np.random.default_rng(77)
    tx_gene = rng.integers(-1, 40, 700).astype(np.int32)
    rows = rng.uniform(1e-8, 1e6, (3, 700)) * rng.integers(0, 2, (3, 700))
    got, want = ref.gene_sums(tx_gene, 41, rows), ref.gene_sums_loop(tx_gene, 41, rows)
    assert got.shape == (3, 41) and got.tobytes() == want.tobytes()
    assert not got[:, 40].any()                                   # a gene without transcripts


def test_reference_counts_against_a_loop():
    rng = np.random.default_rng(78)
    n_tx, n_genes, n_classes, n_samples = 300, 25, 400, 4
    tx_gene = (np.arange(n_tx) // 12).astype(np.int32)
    tx_gene[rng.integers(0, n_tx, 60)] = -1
    sizes = rng.integers(0, 6, n_classes)                         # (some classes without a transcript)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    starts = rng.integers(0, n_tx - 6, n_classes)
    targets = np.concatenate([(starts[c] + rng.permutation(6)[:sizes[c]]) for c in range(n_classes)]).astype(np.int32)
    counts = rng.integers(1, 1 << 40, n_classes)
    sample = rng.integers(0, n_samples - 1, n_classes).astype(np.int32)       # the last sample owns no class
    for class_sample, samples in ((None, 1), (sample, n_samples)):
        got = ref.unique_counts(offsets, targets, counts, tx_gene, n_genes, class_sample, samples)
        want = ref.unique_counts_loop(offsets, targets, counts, tx_gene, n_genes, class_sample, samples)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        fast = ref.unique_counts_reduceat(offsets, targets, counts, tx_gene, n_genes, class_sample, samples)
        np.testing.assert_array_equal(fast[0], want[0])
        np.testing.assert_array_equal(fast[1], want[1])
        assert got[0].sum() + got[1].sum() == counts.sum()
        assert got[0].sum() > 0 and (got[1].sum(axis=0) > 0).all()         # all three kinds occur
    assert not got[0][n_samples - 1].any() and not got[1][n_samples - 1].any()
    assert got[0].max() > 1 << 32


# ------------------------------------------------------------------------------------------- without a GPU
def test_the_symbols_are_exported_and_fail_without_a_gpu(native_libs):
    hip = native_libs.hip()
    names = ('skm_gene_sums', 'skm_gene_unique_counts', 'skm_mapper_gene_counts', 'skm_sample_set_gene_counts')
    for name in names:
        assert name in native_libs.HIP_SYMBOLS and hasattr(hip, name)
    if native_libs.device_count() > 0:
        return
    p, i32, i64, f64 = native_libs.ptr, native_libs.c_i32p, native_libs.c_i64p, native_libs.c_f64p
    tx_gene = np.asarray([0, 1, -1, 1], dtype=np.int32)
    values, sums = np.ones((2, 4)), np.zeros((2, 2))
    offsets, targets, counts = np.asarray([0, 2, 3], dtype=np.int64), np.asarray([0, 1, 3], dtype=np.int32), np.asarray([5, 6], dtype=np.int64)
    unique, other = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    assert hip.skm_gene_sums(0, 2, 4, 2, p(tx_gene, i32), p(values, f64), p(sums, f64)) == native_libs.SKM_ERR_NO_DEVICE
    assert hip.skm_gene_unique_counts(0, 2, p(offsets, i64), p(targets, i32), p(counts, i64), None, 1, 4, 2, p(tx_gene, i32),
                                      p(unique, i64), p(other, i64)) == native_libs.SKM_ERR_NO_DEVICE
    assert hip.skm_mapper_gene_counts(None, 4, 2, p(tx_gene, i32), p(unique, i64), p(other, i64)) == native_libs.SKM_ERR_NO_DEVICE
    assert hip.skm_sample_set_gene_counts(None, 4, 2, p(tx_gene, i32), 1, p(unique, i64), p(other, i64)) == native_libs.SKM_ERR_NO_DEVICE
    assert b'no HIP device' in hip.skm_last_error()
    assert not sums.any() and not unique.any() and not other.any()
