"""Sample sets that keep one fragment-length histogram per sample (mapper.SampleSet(per_sample_lengths=True),
skm_sample_set_keep_histograms / _histograms, sample_fld_kernel) and the effective lengths of many histograms in
one call (skm_effective_lengths_many).

The contract under test: row i of sample_fragment_length_counts is the histogram of a MapResult fed sample i's
reads alone, however the samples are interleaved, cut into launches or spread over threads; the rows add up to the
set's pooled histogram; summary i carries the effective lengths of that MapResult.  All comparisons are
array_equal: integers, or doubles made by the same arithmetic in the same order."""
import multiprocessing.pool

import numpy as np
import pytest

from conftest import make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu

# (units, shortest and longest fragment, shortest transcript drawn from); None = random reads, every unit unaligned
CELLS = ((0, 150, 400, 450), (1, 150, 400, 450), (37, 150, 400, 450), (3000, 150, 400, 450), (400, 450, 900, 950),
         (400, 1900, 2500, 2601), None)
PLAIN, MIDDLE, LONG, RANDOM_CELL = 3, 4, 5, 6
FLD_WINDOW = 512                    # the bins below it are counted in LDS, the others straight in HBM


def _cell_reads(seqs, rng, n_units, paired, shortest, longest, min_tx, read_len=75):
    """Units of chr21 fragments of shortest..longest bases, one read in eight with a substitution or an N."""
    long_tx = [s.upper() for s in seqs if len(s) >= min_tx]
    assert long_tx
    reads = []
    for u in range(n_units):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(shortest, longest + 1))
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
    rng = np.random.default_rng(311 + paired)
    mates = 2 if paired else 1
    return [_cell_reads(seqs, rng, cell[0], paired, *cell[1:]) if cell is not None
            else [bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 75)) for _ in range(500 * mates)] for cell in CELLS]


def _batch(oracle, reads, paired):
    from seekmer_amd import common
    bases, offsets = oracle.pack_reads(reads) if reads else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    return common.ReadBatch(len(reads) // (2 if paired else 1), bases, offsets, paired)


def _add(oracle, sample_set, sample, reads, paired, packed, first_unit=0):
    """One segment: packed (the mates as pieces of their own) or as text."""
    from seekmer_amd import common
    if not packed or not reads:
        sample_set.add_batch(sample, first_unit, _batch(oracle, reads, paired))
        return
    step = 2 if paired else 1
    pieces = [common.PackedReads.from_ascii(*oracle.pack_reads(reads[mate::step]), stream=mate) for mate in range(step)]
    sample_set.add_packed(sample, first_unit, *pieces)


@pytest.fixture(scope='module')
def product_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


@pytest.fixture(scope='module', params=[True, False], ids=['paired', 'single'])
def case(request, oracle, native_libs, chr21, product_index):
    """(paired, cells, per cell: (histogram, summary, TPM, EM steps) of a MapResult fed the cell alone), made once.
    A cell too small to quantify (no abundance above the floor: the reference raises there) has TPM None and the
    error's code in place of the steps."""
    from seekmer_amd import infer, mapper
    paired = request.param
    cells = _cells(chr21[1], paired)
    expected = []
    for reads in cells:
        result = mapper.MapResult(product_index)
        mapper.ReadMapper(product_index, result).map_batch(_batch(oracle, reads, paired))
        summary = result.summarize()
        try:
            tpm, steps = infer.quantify(summary, return_iters=True)
            tpm.setflags(write=False)
        except native_libs.NativeError as error:
            tpm, steps = None, error.code
        fld = result.fragment_length_counts
        fld.setflags(write=False)
        expected.append((fld, summary, tpm, steps))
    return paired, cells, expected


def _assert_histograms(sample_set, expected):
    got = sample_set.sample_fragment_length_counts
    assert got.shape == (len(expected), 2000) and got.dtype == np.int64
    for i, want in enumerate(expected):
        np.testing.assert_array_equal(got[i], want[0], err_msg='histogram of sample %d' % i)
    np.testing.assert_array_equal(got.sum(axis=0), sample_set.fragment_length_counts)


def test_histograms_equal_the_per_cell_histograms(oracle, product_index, case):
    """Cells of 0, 1, 37 and 3000 units, one of fragments that reach the bins the kernel counts outside LDS, one
    that reaches the clamp bin and one of random reads, even samples packed and odd ones as text."""
    from seekmer_amd import mapper
    paired, cells, expected = case
    if paired:      # the reference itself must reach what the test is about
        assert expected[PLAIN][0][:FLD_WINDOW].sum() > 1000
        assert expected[MIDDLE][0][FLD_WINDOW:1999].sum() > 20
        assert expected[LONG][0][1999] > 5
        assert expected[RANDOM_CELL][0].sum() == 0
    else:           # (a read's own span: 25 bases, one k-mer, for a read that maps nowhere)
        assert expected[PLAIN][0][25:76].sum() == expected[PLAIN][0].sum() > 1000
        assert expected[RANDOM_CELL][0][25] == expected[RANDOM_CELL][0].sum() > 0
    assert expected[0][0].sum() == 0
    sample_set = mapper.SampleSet(product_index, paired, per_sample_lengths=True)
    for i, reads in enumerate(cells):
        _add(oracle, sample_set, i, reads, paired, packed=i % 2 == 0)
    _assert_histograms(sample_set, expected)


@pytest.mark.parametrize('how', ['shuffled', 'threads', 'cut', 'segments'])
def test_histograms_do_not_depend_on_submission(oracle, product_index, case, how, monkeypatch):
    """The same cells in shuffled order, from four threads, with launches of at most 1000 units (a cell's row is
    added up over many launches), and with a cell added as three in-order segments."""
    from seekmer_amd import mapper
    paired, cells, expected = case
    if how == 'cut':
        monkeypatch.setenv('SKM_SAMPLE_SET_MAX_UNITS', '1000')
    sample_set = mapper.SampleSet(product_index, paired, per_sample_lengths=True)
    step = 2 if paired else 1
    order = list(range(len(cells)))
    if how != 'segments':
        np.random.default_rng(5).shuffle(order)

    def add(i):
        if how == 'segments' and i == PLAIN:
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
    _assert_histograms(sample_set, expected)


def test_many_tiny_samples_in_one_launch(oracle, chr21, chr21_oracle_index, product_index, case):
    """300 samples of 1 to 5 units in one launch: a block and a wave span many segments.  The samples are numbered
    with gaps; the rows nobody named stay zero.  Reference: the CPU oracle per sample."""
    from seekmer_amd import mapper
    paired = case[0]
    rng = np.random.default_rng(99)
    numbers = 3 * np.arange(300) + 1
    want = np.zeros((int(numbers[-1]) + 1, 2000), dtype=np.int64)
    sample_set = mapper.SampleSet(product_index, paired, per_sample_lengths=True)
    for sample in numbers:
        shortest, longest, min_tx = ((150, 400, 450), (450, 900, 950), (1900, 2500, 2601))[int(rng.integers(3))]
        reads = _cell_reads(chr21[1], rng, int(rng.integers(1, 6)), paired, shortest, longest, min_tx)
        batch = _batch(oracle, reads, paired)
        oracle.map_batch(chr21_oracle_index, batch.bases, batch.offsets, batch.count, paired, want[sample])
        sample_set.add_batch(int(sample), 0, batch)
    # (the reference must reach every path of the kernel; about a third of such pairs give a length)
    assert want.sum() > 100 and (not paired or (want[:, FLD_WINDOW:1999].sum() > 10 and want[:, 1999].sum() > 3))
    got = sample_set.sample_fragment_length_counts
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.sum(axis=0), sample_set.fragment_length_counts)


def test_strand_mode_leaves_the_histograms(oracle, product_index, case):
    """The strand filter runs after the map kernel: the histograms are those of the unstranded set, the tables not."""
    from seekmer_amd import mapper
    paired, cells, expected = case
    sets = []
    for strand in (None, 'fr'):
        sample_set = mapper.SampleSet(product_index, paired, strand=strand, per_sample_lengths=True)
        for i, reads in enumerate(cells):
            _add(oracle, sample_set, i, reads, paired, packed=i % 2 == 0)
        sets.append(sample_set)
    _assert_histograms(sets[1], expected)
    assert sets[0].sizes()[PLAIN].tolist() != sets[1].sizes()[PLAIN].tolist(), 'the mode must change the table'


def test_errors_and_the_pooled_default(oracle, native_libs, product_index, case):
    from seekmer_amd import mapper
    paired, cells, expected = case
    pooled = mapper.SampleSet(product_index, paired)
    for i in (2, MIDDLE):
        _add(oracle, pooled, i - 2, cells[i], paired, packed=False)
    with pytest.raises(native_libs.NativeError) as error:      # switched on a set that holds units
        native_libs.check(native_libs.hip().skm_sample_set_keep_histograms(pooled._handle, 1))
    assert error.value.code == native_libs.SKM_ERR_STATE
    room = np.zeros((len(pooled), 2000), dtype=np.int64)
    with pytest.raises(native_libs.NativeError) as error:      # read from a set that keeps none
        native_libs.check(native_libs.hip().skm_sample_set_histograms(pooled._handle, len(room),
                                                                      native_libs.ptr(room, native_libs.c_i64p)))
    assert error.value.code == native_libs.SKM_ERR_STATE
    with pytest.raises(ValueError):
        pooled.sample_fragment_length_counts
    summaries = pooled.summarize()
    assert len(summaries) == 3
    assert all(s.fragment_length_frequencies is summaries[0].fragment_length_frequencies for s in summaries)
    assert all(s.effective_lengths is summaries[0].effective_lengths for s in summaries)
    np.testing.assert_array_equal(summaries[0].fragment_length_frequencies, expected[2][0] + expected[MIDDLE][0])
    kept = mapper.SampleSet(product_index, paired, per_sample_lengths=True)
    _add(oracle, kept, 1, cells[2], paired, packed=True)
    # room for fewer samples than the set names
    assert native_libs.hip().skm_sample_set_histograms(kept._handle, 1, native_libs.ptr(room, native_libs.c_i64p)) \
        == native_libs.SKM_ERR_ARG
    _add(oracle, kept, 40, [], paired, packed=False)           # named, without units: rows the device never held
    got = kept.sample_fragment_length_counts
    assert got.shape == (41, 2000) and got[0].sum() == 0 and got[2:].sum() == 0
    np.testing.assert_array_equal(got[1], expected[2][0])


@pytest.mark.parametrize('n_tx', [1, 257, 1704])
def test_effective_lengths_of_many_histograms(oracle, native_libs, chr21_oracle_index, case, n_tx):
    """An ordinary histogram, a single occupied bin, the clamp bin alone and an empty histogram (a NaN row): every
    row is what skm_effective_lengths gives for it alone, and what the oracle gives."""
    from seekmer_amd import mapper
    paired, _, expected = case
    lengths = np.ascontiguousarray(chr21_oracle_index.lengths[:n_tx], dtype='f8')
    assert lengths.size == n_tx
    fld = np.zeros((4, 2000), dtype=np.int64)
    fld[0] = expected[PLAIN][0] + expected[MIDDLE][0]
    fld[1, 187] = 12
    fld[2, 1999] = 3
    assert np.count_nonzero(fld[0]) > 30
    got = mapper._effective_lengths_many(lengths, fld, 0)
    assert got.shape == (4, n_tx)
    for row in range(4):
        one = mapper._effective_lengths(lengths, fld[row], 0)
        np.testing.assert_array_equal(got[row], one, err_msg='row %d against the single call' % row)
        np.testing.assert_array_equal(got[row], oracle.effective_lengths(fld[row], lengths),
                                      err_msg='row %d against the oracle' % row)
    assert np.isnan(got[3]).all() and not np.isnan(got[:3]).any()
    none = mapper._effective_lengths_many(lengths, fld[:0], 0)
    assert none.shape == (0, n_tx)


@pytest.mark.parametrize('group', [None, 3, 64])
def test_effective_lengths_of_many_rows_and_groups(oracle, chr21_oracle_index, group, monkeypatch):
    """70 distinct histograms (one of them empty): the form for 64 rows and more, and -- with at most 3 and 64 rows
    a group -- the groups after the first, whose rows are read and written at an offset.  Against the oracle."""
    from seekmer_amd import mapper
    if group is None:
        monkeypatch.delenv('SKM_EFF_MANY_GROUP', raising=False)
    else:
        monkeypatch.setenv('SKM_EFF_MANY_GROUP', str(group))
    rng = np.random.default_rng(8)
    lengths = np.ascontiguousarray(chr21_oracle_index.lengths, dtype='f8')
    fld = np.zeros((70, 2000), dtype=np.int64)
    for row in range(70):
        bins = rng.integers(1, 2000, int(rng.integers(1, 300)))
        np.add.at(fld[row], bins, rng.integers(1, 1000, bins.size))
    fld[41] = 0
    got = mapper._effective_lengths_many(lengths, fld, 0)
    for row in range(70):
        np.testing.assert_array_equal(got[row], oracle.effective_lengths(fld[row], lengths), err_msg='row %d' % row)
    assert np.isnan(got[41]).all() and len({got[row].tobytes() for row in range(70)}) == 70


def test_sample_numbers_of_a_set_with_histograms_are_bounded(oracle, native_libs, product_index, case):
    """The histograms are rows by sample number: a number that would ask for more than 1 GiB of them is refused."""
    from seekmer_amd import mapper
    paired, cells, _ = case
    kept = mapper.SampleSet(product_index, paired, per_sample_lengths=True)
    with pytest.raises(ValueError, match='below 65536'):
        _add(oracle, kept, 1 << 16, cells[2], paired, packed=False)
    assert len(kept) == 0
    pooled = mapper.SampleSet(product_index, paired)
    _add(oracle, pooled, 1 << 16, [], paired, packed=False)        # (a pooled set has no such rows)
    assert len(pooled) == (1 << 16) + 1


def test_summaries_carry_their_own_lengths(oracle, native_libs, product_index, case):
    from seekmer_amd import infer, mapper
    paired, cells, expected = case
    sample_set = mapper.SampleSet(product_index, paired, per_sample_lengths=True)
    for i, reads in enumerate(cells):
        _add(oracle, sample_set, i, reads, paired, packed=i % 2 == 1)
    summaries = sample_set.summarize()
    assert len(summaries) == len(cells)
    means = sample_set.harmonic_mean_fragment_lengths()
    for i, (summary, (fld, want, tpm, steps)) in enumerate(zip(summaries, expected)):
        np.testing.assert_array_equal(summary.fragment_length_frequencies, fld, err_msg='histogram %d' % i)
        np.testing.assert_array_equal(summary.effective_lengths, want.effective_lengths, err_msg='lengths %d' % i)
        assert (summary.aligned, summary.unaligned, summary.total) == (want.aligned, want.unaligned, want.total)
        if tpm is None:
            with pytest.raises(native_libs.NativeError) as error:
                infer.quantify(summary)
            assert error.value.code == steps, i
        else:
            got_tpm, got_steps = infer.quantify(summary, return_iters=True)
            assert got_steps == steps, i
            np.testing.assert_array_equal(got_tpm, tpm, err_msg='TPM %d' % i)
        assert means[i] == oracle.harmonic_mean_fragment_length(fld), i
    assert means[0] == 0 and means[RANDOM_CELL] == (0 if paired else 25) and means[PLAIN] > 25
    assert all(expected[i][2] is not None for i in (0, PLAIN, MIDDLE, RANDOM_CELL)), 'cells that must quantify'
    assert np.isnan(summaries[0].effective_lengths).all()
    if paired:      # pooled lengths cannot pass: the cells' lengths differ from each other and from the pooled ones
        pooled = mapper._effective_lengths(np.ascontiguousarray(product_index.transcripts['length'], dtype='f8'),
                                           sample_set.fragment_length_counts, 0)
        plain, middle = summaries[PLAIN].effective_lengths, summaries[MIDDLE].effective_lengths
        assert not np.array_equal(plain, middle)
        assert not np.array_equal(plain, pooled) and not np.array_equal(middle, pooled)


def test_a_sample_without_units_past_the_rows_reads_as_zero(oracle, chr21, product_index):
    """A set that keeps histograms and hexamer counts, two samples of 300 pairs, and sample 40 named by a segment
    without units: no launch held it, so its rows lie past the set's buffers (rows 0 to 1 exist).  Its histogram
    and hexamer rows are zero, its sizes (0, 0, 0, 0); the rows of the two others are those of the same reads
    mapped alone."""
    from seekmer_amd import mapper
    rng = np.random.default_rng(40)
    cells = [_cell_reads(chr21[1], rng, 300, True, 150, 400, 450) for _ in range(2)]
    sample_set = mapper.SampleSet(product_index, True, per_sample_lengths=True, bias=True)
    for i, reads in enumerate(cells):
        _add(oracle, sample_set, i, reads, True, packed=i == 0)
    _add(oracle, sample_set, 40, [], True, packed=False)
    histograms, hexamers, sizes = sample_set.sample_fragment_length_counts, sample_set.bias_observed(), sample_set.sizes()
    assert histograms.shape == (41, 2000) and hexamers.shape == (41, 4096) and sizes.shape == (41, 4)
    assert not histograms[2:].any() and not hexamers[2:].any() and not sizes[2:].any()
    for i, reads in enumerate(cells):
        alone = mapper.MapResult(product_index, bias=True)
        mapper.ReadMapper(product_index, alone).map_batch(_batch(oracle, reads, True))
        assert alone.fragment_length_counts.sum() > 100 and alone.bias_observed().sum() > 100
        np.testing.assert_array_equal(histograms[i], alone.fragment_length_counts, err_msg='histogram of sample %d' % i)
        np.testing.assert_array_equal(hexamers[i], alone.bias_observed(), err_msg='hexamers of sample %d' % i)
        assert tuple(sizes[i]) == alone.sizes(), i
