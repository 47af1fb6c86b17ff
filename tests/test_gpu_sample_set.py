"""Sample sets (mapper.SampleSet / skm_sample_set_*): many samples mapped in shared launches into one
class table whose classes are (sample, tuple).

The contract under test: every per-sample table -- class order, offsets, targets, counts, first-seen
units counted inside the sample, unaligned and total units -- is bit for bit the table a MapResult of
its own gives for the sample's reads, however the samples are interleaved, cut into launches or spread
over threads; the set's one histogram is the sum of the samples'.  All comparisons are array_equal on
integers; the impute check compares files byte for byte."""
import multiprocessing.pool
import os

import numpy as np
import pytest

from conftest import make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 37, 5000, 20000)
RANDOM_CELL, TWIN_A, TWIN_B = 5, 3, 6          # a cell of random reads; two cells with identical reads


def _cell_reads(seqs, rng, n_units, paired, read_len=75):
    """Units of chr21 fragments, one read in eight with a substitution or an N."""
    long_tx = [s.upper() for s in seqs if len(s) > 450]
    reads = []
    for u in range(n_units):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(150, 401))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        mates = [f[:read_len], reverse_complement(f[-read_len:])]
        if rng.integers(2):
            mates.reverse()
        for read in (mates if paired else mates[:1]):
            r = bytearray(read)
            kind = int(rng.integers(16))
            if kind == 0:
                r[int(rng.integers(len(r)))] = b'ACGT'[int(rng.integers(4))]
            elif kind == 1:
                r[int(rng.integers(len(r)))] = ord('N')
            reads.append(bytes(r))
    return reads


def _cells(seqs, paired):
    """The reads of seven cells: SIZES, a cell of random reads (every unit unaligned), and a second copy
    of the 5000-unit cell (the same tuples in two samples)."""
    rng = np.random.default_rng(77 + paired)
    cells = [_cell_reads(seqs, rng, n, paired) for n in SIZES]
    mates = 2 if paired else 1
    cells.append([bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 75)) for _ in range(3000 * mates)])
    cells.append(list(cells[TWIN_A]))
    return cells


def _batch(oracle, reads, paired):
    from seekmer_amd import common
    bases, offsets = oracle.pack_reads(reads) if reads else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    return common.ReadBatch(len(reads) // (2 if paired else 1), bases, offsets, paired)


def _per_cell(oracle, index, cells, paired, strand=None):
    """[(sizes, export)] of a MapResult per cell."""
    from seekmer_amd import mapper
    out = []
    for reads in cells:
        result = mapper.MapResult(index, strand=strand)
        mapper.ReadMapper(index, result).map_batch(_batch(oracle, reads, paired))
        out.append((result.sizes(), result.export()))
    return out


def _add(oracle, sample_set, sample, reads, paired, packed, first_unit=0):
    """One segment: packed (the mates as pieces of their own) or as text."""
    from seekmer_amd import common
    if not packed or not reads:
        sample_set.add_batch(sample, first_unit, _batch(oracle, reads, paired))
        return
    step = 2 if paired else 1
    pieces = [common.PackedReads.from_ascii(*oracle.pack_reads(reads[mate::step]), stream=mate) for mate in range(step)]
    sample_set.add_packed(sample, first_unit, *pieces)


def _assert_same(sample_set, expected):
    sizes = sample_set.sizes()
    tables = sample_set.export()
    assert len(sample_set) == len(expected) == len(tables)
    total_fld = np.zeros(2000, dtype=np.int64)
    for i, (want_sizes, (offsets, targets, counts, first, fld)) in enumerate(expected):
        assert tuple(int(v) for v in sizes[i]) == want_sizes, i
        got = tables[i]
        np.testing.assert_array_equal(got[0], offsets, err_msg='class_offsets of sample %d' % i)
        np.testing.assert_array_equal(got[1], targets, err_msg='class_targets of sample %d' % i)
        np.testing.assert_array_equal(got[2], counts, err_msg='class_counts of sample %d' % i)
        np.testing.assert_array_equal(got[3], first, err_msg='first_seen of sample %d' % i)
        total_fld += fld
    np.testing.assert_array_equal(sample_set.fragment_length_counts, total_fld)


@pytest.fixture(scope='module')
def product_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


@pytest.fixture(scope='module', params=[True, False], ids=['paired', 'single'])
def case(request, oracle, native_libs, chr21, product_index):
    paired = request.param
    cells = _cells(chr21[1], paired)
    return paired, cells, _per_cell(oracle, product_index, cells, paired)


def test_tables_equal_the_per_cell_tables(oracle, product_index, case):
    """Cells of 0, 1, 37, 5000 and 20000 units, one of random reads and two with identical reads, added in
    order -- even samples packed, odd ones as text -- against a MapResult per cell."""
    from seekmer_amd import mapper
    paired, cells, expected = case
    assert expected[RANDOM_CELL][0][:3] == (0, 0, 3000), 'the random cell must be all unaligned'
    assert expected[TWIN_A][0][0] > 100 and expected[TWIN_A][0] == expected[TWIN_B][0]
    sample_set = mapper.SampleSet(product_index, paired)
    for i, reads in enumerate(cells):
        _add(oracle, sample_set, i, reads, paired, packed=i % 2 == 0)
    _assert_same(sample_set, expected)
    # both twins came back whole: same tuples, same counts, separate classes
    tables = sample_set.export()
    for a, b in zip(tables[TWIN_A], tables[TWIN_B]):
        np.testing.assert_array_equal(a, b)
    summaries = sample_set.summarize()
    assert [s.total for s in summaries] == [len(c) // (2 if paired else 1) for c in cells]
    assert all(s.fragment_length_frequencies is summaries[0].fragment_length_frequencies for s in summaries)


@pytest.mark.parametrize('how', ['shuffled', 'threads', 'cut', 'segments'])
def test_tables_do_not_depend_on_submission(oracle, product_index, case, how, monkeypatch):
    """The same cells in shuffled order, from four threads, with launches of at most 1000 units (cells
    cut across launches, many launches), and with a cell added as three in-order segments."""
    from seekmer_amd import mapper
    paired, cells, expected = case
    if how == 'cut':
        monkeypatch.setenv('SKM_SAMPLE_SET_MAX_UNITS', '1000')
    sample_set = mapper.SampleSet(product_index, paired)
    step = 2 if paired else 1
    order = list(range(len(cells)))
    if how != 'segments':
        np.random.default_rng(5).shuffle(order)

    def add(i):
        if how == 'segments' and i == 4:
            for lo, hi in ((0, 1234), (1234, 1235), (1235, len(cells[i]) // step)):
                _add(oracle, sample_set, i, cells[i][lo * step:hi * step], paired, packed=lo == 0, first_unit=lo)
        else:
            _add(oracle, sample_set, i, cells[i], paired, packed=i % 2 == 1)

    if how == 'threads':
        pool = multiprocessing.pool.ThreadPool(4)
        pool.map(add, order)
        pool.close()
        pool.join()
    else:
        for i in order:
            add(i)
    _assert_same(sample_set, expected)


def test_segments_out_of_order_are_refused(oracle, native_libs, product_index, case):
    from seekmer_amd import mapper
    paired, cells, _ = case
    step = 2 if paired else 1
    sample_set = mapper.SampleSet(product_index, paired)
    _add(oracle, sample_set, 0, cells[2][:10 * step], paired, packed=True)
    for first_unit in (20, 5, 0):                     # a gap, an overlap, a repeat
        with pytest.raises(native_libs.NativeError) as error:
            _add(oracle, sample_set, 0, cells[2][10 * step:20 * step], paired, packed=False, first_unit=first_unit)
        assert error.value.code == native_libs.SKM_ERR_STATE
    _add(oracle, sample_set, 0, cells[2][10 * step:20 * step], paired, packed=False, first_unit=10)
    assert sample_set.sizes()[0][3] == 20
    with pytest.raises(native_libs.NativeError) as error:      # the strand mode of a set that holds units
        native_libs.check(native_libs.hip().skm_sample_set_set_strand(sample_set._handle, 1))
    assert error.value.code == native_libs.SKM_ERR_STATE


def test_truth_and_len_wait_for_nothing(oracle, native_libs, product_index, case):
    """A set is a handle: it is true whatever it holds, and len() counts the samples named so far."""
    from seekmer_amd import mapper
    paired, cells, _ = case
    sample_set = mapper.SampleSet(product_index, paired)
    assert sample_set and len(sample_set) == 0 and sample_set.sizes().shape == (0, 4)
    _add(oracle, sample_set, 1, cells[0], paired, packed=False)         # (a cell of no units; sample 0 comes with it)
    assert sample_set and len(sample_set) == 2
    assert sample_set.sizes().tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert [t[2].size for t in sample_set.export()] == [0, 0]


def test_two_cells_against_the_oracle(oracle, chr21_oracle_index, product_index, case):
    """Not only product against product: the 5000-unit cell and its twin's neighbour against the CPU oracle."""
    from seekmer_amd import mapper
    paired, cells, _ = case
    picked = (TWIN_A, 2, TWIN_B)
    sample_set = mapper.SampleSet(product_index, paired)
    for sample, i in enumerate(picked):
        _add(oracle, sample_set, sample, cells[i], paired, packed=sample != 1)
    sizes, tables = sample_set.sizes(), sample_set.export()
    fld_total = np.zeros(2000, dtype=np.int64)
    for sample, i in enumerate(picked):
        batch = _batch(oracle, cells[i], paired)
        fld = np.zeros(2000, dtype=np.int64)
        units = oracle.map_batch(chr21_oracle_index, batch.bases, batch.offsets, batch.count, paired, fld)
        classes = oracle.Classes()
        classes.update(units)
        offsets, ids, counts = classes.export()
        np.testing.assert_array_equal(tables[sample][0], offsets)
        np.testing.assert_array_equal(tables[sample][1], ids)
        np.testing.assert_array_equal(tables[sample][2], counts)
        assert int(sizes[sample][2]) == classes.unaligned and int(sizes[sample][3]) == batch.count
        fld_total += fld
    np.testing.assert_array_equal(sample_set.fragment_length_counts, fld_total)


def test_strand_mode_applies_to_the_whole_set(oracle, product_index, case):
    from seekmer_amd import mapper
    paired, cells, unstranded = case
    picked = [cells[i] for i in (2, TWIN_A, RANDOM_CELL, TWIN_B)]
    expected = _per_cell(oracle, product_index, picked, paired, strand='fr')
    assert expected[1][0] != unstranded[TWIN_A][0], 'the mode must change the table'
    sample_set = mapper.SampleSet(product_index, paired, strand='fr')
    for i, reads in enumerate(picked):
        _add(oracle, sample_set, i, reads, paired, packed=i % 2 == 0)
    _assert_same(sample_set, expected)


def _write_fastq(path, reads, mate):
    path.write_bytes(b''.join(b'@r%d/%d\n%s\n+\n%s\n' % (i, mate, r, b'I' * len(r)) for i, r in enumerate(reads)))


def test_feeders_equal_map_multiple_samples(oracle, native_libs, chr21, product_index, tmp_path):
    """map_sample_set over FASTQ files against map_multiple_samples: a cell of two pairs of files whose
    mate files differ in length (zip(file1, file2) counts the shorter), an empty cell, a compressed cell
    (the text reader), from one thread and from three."""
    import bz2
    from seekmer_amd import common, mapper
    rng = np.random.default_rng(11)
    groups = []
    for cell, (n1, n2, extra) in enumerate(((700, 650, 300), (0, 0, 0), (400, 400, 0), (900, 950, 0))):
        reads = _cell_reads(chr21[1], rng, max(n1, n2), True)
        paths = [tmp_path / ('c%d_1.fastq' % cell), tmp_path / ('c%d_2.fastq' % cell)]
        _write_fastq(paths[0], reads[0:2 * n1:2], 1)
        _write_fastq(paths[1], reads[1:2 * n2:2], 2)
        if extra:
            more = _cell_reads(chr21[1], rng, extra, True)
            paths += [tmp_path / ('c%d_3.fastq' % cell), tmp_path / ('c%d_4.fastq' % cell)]
            _write_fastq(paths[2], more[0::2], 1)
            _write_fastq(paths[3], more[1::2], 2)
        if cell == 2:
            for k, path in enumerate(paths):
                packed = path.with_suffix('.fastq.bz2')
                packed.write_bytes(bz2.compress(path.read_bytes()))
                paths[k] = packed
        groups.append(paths)

    def feeders():
        return [common.PackedReadFeeder(g, paired=True) if common.PackedReadFeeder.eligible(g)
                else common.NativeReadFeeder(g, paired=True) for g in groups]

    results = mapper.map_multiple_samples(product_index, feeders())
    expected = [(r.sizes(), r.export()) for r in results]
    assert [e[0][3] for e in expected] == [950, 0, 400, 900]
    for jobs in (1, 3):
        _assert_same(mapper.map_sample_set(product_index, feeders(), job_count=jobs), expected)


def test_impute_files_do_not_depend_on_the_mapping_path(native_libs, tmp_path, monkeypatch):
    """`seekmer impute` on nine cells written as FASTQ files: tpm.csv, initial_gene_table.csv and weight.csv
    of the default path (the sample set) are byte for byte those of SKM_IMPUTE_PER_CELL=1."""
    from seekmer_amd import common, index_builder, mapper, synth
    from seekmer_amd.__main__ import main
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    transcripts = np.zeros(len(ids), dtype=[('transcript_id', index.transcripts.dtype['transcript_id']),
                                            ('gene_id', 'S8'), ('length', 'f8')])
    transcripts['transcript_id'] = index.transcripts['transcript_id']
    transcripts['length'] = index.transcripts['length']
    transcripts['gene_id'] = [b'GENE%04d' % (t // 4) for t in range(len(ids))]
    index = common.KMerIndex(index.kmers, index.contigs, index.sequences, index.targets, transcripts, index.exons)
    index_path = tmp_path / 'index.npz'
    index.save(index_path)
    read_len, paths = 75, []
    for cell in range(9):
        n_units = 3000 + 500 * cell
        bases, _ = synth.reads(100 + cell % 2, pool, tx_offsets, cell * 8000, n_units, read_len, True)
        reads = bases[:-1].reshape(n_units, 2, read_len)
        for mate in (0, 1):
            path = tmp_path / ('cell%d_%d.fastq' % (cell, mate + 1))
            _write_fastq(path, [reads[i, mate].tobytes() for i in range(n_units)], mate + 1)
            paths.append(path)
    calls = []
    through_set = mapper.map_sample_set
    monkeypatch.setattr(mapper, 'map_sample_set', lambda *a, **k: calls.append('set') or through_set(*a, **k))
    arguments = [str(index_path), None, *map(str, paths), '-p', '4', '--seed', '0', '-j', '3']
    monkeypatch.delenv('SKM_IMPUTE_PER_CELL', raising=False)
    arguments[1] = str(tmp_path / 'out_set')
    assert main(['impute'] + arguments) == 0
    assert calls == ['set'], 'the default path must map through the sample set'
    monkeypatch.setenv('SKM_IMPUTE_PER_CELL', '1')
    arguments[1] = str(tmp_path / 'out_per_cell')
    assert main(['impute'] + arguments) == 0
    assert calls == ['set']
    for name in ('tpm.csv', 'initial_gene_table.csv', 'weight.csv'):
        ours, theirs = (tmp_path / 'out_set' / name).read_bytes(), (tmp_path / 'out_per_cell' / name).read_bytes()
        assert len(ours) > 100 and ours == theirs, name
