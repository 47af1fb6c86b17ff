"""Sequence bias (--bias) in sample sets: the observed hexamers counted per sample inside the set's launches, the
correction of many samples in one call, the second pass in shared EM launches, and `infer-many --bias`.

Everything that has a single-sample counterpart on the device is compared with it bit for bit; the comparisons
with tests/bias_reference.py are exact for the integer counts and use test_gpu_bias.py's 1e-9 for E, b and eff'."""
import logging
import os

import numpy as np
import pytest

import bias_reference as ref
from conftest import GOLDEN, make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu

STRANDS = [None, 'fr', 'rf']
EMPTY, UNALIGNED, ODD, LARGE = 3, 4, 5, 2           # the samples of _samples with a case of their own


# ---------------------------------------------------------------------------------------------- inputs
def _fragments(seqs, rng, n_units, read_len=60):
    """[mate 1, mate 2] of n_units chr21 fragments, either mate first"""
    long_tx = [s.upper() for s in seqs if len(s) > 450 and set(s.upper()) <= set(b'ACGT')]
    units = []
    for _ in range(n_units):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(150, 401))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        mates = [bytearray(f[:read_len]), bytearray(reverse_complement(f[-read_len:]))]
        if rng.integers(2):
            mates.reverse()
        units.append(mates)
    return units


def _samples(seqs, paired):
    """Six samples, as lists of reads ([mate 1, mate 2, mate 1, ...] when paired): two of 40 units (a wave's 64
    records hold both, a tile of 256 several samples), one of 600 (whole tiles of one sample), one without units,
    one whose units all fail to align, and one with a read shorter than six bases and reads with N or a
    lower-case letter among the first six."""
    rng = np.random.default_rng(606)
    samples = [_fragments(seqs, rng, 40), _fragments(seqs, rng, 41), _fragments(seqs, rng, 600), []]
    samples.append([[bytearray(bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 60))) for _ in range(2)] for _ in range(50)])
    odd = _fragments(seqs, rng, 36)
    for u, mates in enumerate(odd):
        kind = u % 6
        if kind == 0:
            mates[0][int(rng.integers(6))] = ord('N')
        elif kind == 1:
            q = int(rng.integers(6))
            mates[0][q:q + 1] = bytes(mates[0][q:q + 1]).lower()
        elif kind == 2:
            mates[0][6] = ord('N')                                       # base 7: still counted
        elif kind == 3:
            mates[1][:6] = bytes(mates[1][:6]).lower()                    # mate 2's bases are not what counts
    odd.insert(7, [bytearray(b'ACGTA'), bytearray(odd[0][1])])            # a read of five bases
    odd.insert(20, [bytearray(b'ACGTAC'), bytearray(odd[1][1])])          # six bases: too short to align
    samples.append(odd)
    return [[bytes(r) for mates in units for r in (mates if paired else mates[:1])] for units in samples]


def _batch(oracle, reads, paired):
    from seekmer_amd import common
    bases, offsets = oracle.pack_reads(reads) if reads else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    return common.ReadBatch(len(reads) // (2 if paired else 1), bases, offsets, paired)


def _add(oracle, sample_set, sample, reads, paired, packed, first_unit=0):
    from seekmer_amd import common
    if not packed or not reads:
        sample_set.add_batch(sample, first_unit, _batch(oracle, reads, paired))
        return
    step = 2 if paired else 1
    pieces = [common.PackedReads.from_ascii(*oracle.pack_reads(reads[mate::step]), stream=mate) for mate in range(step)]
    sample_set.add_packed(sample, first_unit, *pieces)


class _Feeder:
    """A sample's reads as text batches of at most `step` units, for mapper.map_sample_set"""

    def __init__(self, oracle, reads, paired, step):
        self.oracle, self.reads, self.paired, self.step = oracle, reads, paired, step

    def __iter__(self):
        width = 2 if self.paired else 1
        for lo in range(0, len(self.reads) // width, self.step):
            yield _batch(self.oracle, self.reads[lo * width:(lo + self.step) * width], self.paired)


@pytest.fixture(scope='module')
def chr21_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


@pytest.fixture(scope='module')
def chr21_windows(chr21_oracle_index):
    ix = chr21_oracle_index
    bases, known = ref.rebuild_transcripts(ix.contigs, ix.sequences, ix.targets, ix.lengths)
    return [ref.windows(b, k) for b, k in zip(bases, known)]


# -------------------------------------------------------------------------------------------- observed
@pytest.mark.parametrize('paired', [True, False], ids=['paired', 'single'])
@pytest.mark.parametrize('strand', STRANDS)
def test_rows_equal_the_samples_mapped_alone(oracle, native_libs, chr21, chr21_index, strand, paired, monkeypatch):
    from seekmer_amd import mapper
    index = chr21_index
    samples = _samples(chr21[1], paired)
    width = 2 if paired else 1
    units = [len(reads) // width for reads in samples]
    assert units == [40, 41, 600, 0, 50, 38]
    # every sample alone: the mapper's own counts, and the counter of the reference on the units it aligned
    want = np.zeros((len(samples), 4096), dtype=np.int64)
    for i, reads in enumerate(samples):
        if not reads:
            continue
        result = mapper.MapResult(index, strand=strand, bias=True)
        rm = mapper.ReadMapper(index, result)
        rm.map_batch(_batch(oracle, reads, paired))
        aligned = rm.last_tuples(units[i])[0] > 0
        want[i] = result.bias_observed()
        np.testing.assert_array_equal(want[i], ref.observed_counts(reads[0::width], aligned), err_msg='sample %d alone' % i)
        if i == ODD:
            firsts = reads[0::width]
            valid = np.asarray([ref.hexamer_code(r[:6]) >= 0 for r in firsts])
            assert len(firsts[7]) == 5 and not aligned[7] and not aligned[20]
            if strand is None:
                assert (aligned & ~valid).any()                                # skipped for its first six bases
        if i == UNALIGNED:
            assert not aligned.any()
    print(strand, 'paired' if paired else 'single', 'counted per sample', want.sum(axis=1).tolist())
    assert not want[UNALIGNED].any() and not want[EMPTY].any()
    assert want[LARGE].sum() > 100 and want[0].sum() > 5 and want[1].sum() > 5 and want[ODD].sum() > 3

    def check(sample_set, how):
        got = sample_set.bias_observed()
        assert got.dtype == np.int64 and got.shape == (len(samples), 4096), how
        np.testing.assert_array_equal(got, want, err_msg=how)

    # in sample order, even samples packed and odd ones as text -- and the same set without counting
    counting = mapper.SampleSet(index, paired, strand=strand, bias=True)
    plain = mapper.SampleSet(index, paired, strand=strand)
    for sample_set in (counting, plain):
        for i, reads in enumerate(samples):
            _add(oracle, sample_set, i, reads, paired, packed=i % 2 == 0)
    check(counting, 'in order')
    np.testing.assert_array_equal(counting.sizes(), plain.sizes())
    for a, b in zip(counting.export(), plain.export()):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(counting.fragment_length_counts, plain.fragment_length_counts)
    with pytest.raises(native_libs.NativeError) as refused:
        plain.bias_observed()
    assert refused.value.code == native_libs.SKM_ERR_STATE
    del counting, plain

    # segments of different samples interleaved, launches of at most 250 units: a border inside the large sample
    monkeypatch.setenv('SKM_SAMPLE_SET_MAX_UNITS', '250')
    sample_set = mapper.SampleSet(index, paired, strand=strand, bias=True)
    cuts = {0: [0, 13, 40], 1: [0, 1, 30, 41], LARGE: [0, 100, 333, 600], UNALIGNED: [0, 50], ODD: [0, 8, 21, 38]}
    turn = 0
    while any(len(c) > 1 for c in cuts.values()):
        for i in sorted(cuts):
            if len(cuts[i]) > 1:
                lo, hi = cuts[i][0], cuts[i][1]
                _add(oracle, sample_set, i, samples[i][lo * width:hi * width], paired, packed=(turn + i) % 2 == 0, first_unit=lo)
                cuts[i].pop(0)
        turn += 1
    sample_set.add_batch(EMPTY, 0, _batch(oracle, [], paired))
    check(sample_set, 'interleaved segments, launches of 250 units')
    del sample_set
    monkeypatch.delenv('SKM_SAMPLE_SET_MAX_UNITS')

    # map_sample_set from feeders, one thread and three
    for job_count in (1, 3):
        feeders = [_Feeder(oracle, reads, paired, 97) for reads in samples]
        check(mapper.map_sample_set(index, feeders, job_count=job_count, strand=strand, bias=True), 'job_count %d' % job_count)


def test_state_rules(oracle, native_libs, chr21_index, pairs21):
    from seekmer_amd import _native, mapper
    hip = _native.hip()
    sample_set = mapper.SampleSet(chr21_index, True)
    h = sample_set._handle
    out = np.zeros((4, 4096), dtype=np.int64)
    p = _native.ptr(out, _native.c_i64p)
    assert hip.skm_sample_set_bias_observed(h, 4, p) == _native.SKM_ERR_STATE       # the set does not count
    assert hip.skm_sample_set_keep_bias(h, 1) == _native.SKM_OK
    assert hip.skm_sample_set_keep_bias(h, 0) == _native.SKM_OK
    assert hip.skm_sample_set_keep_bias(h, 1) == _native.SKM_OK
    assert hip.skm_sample_set_bias_observed(h, 0, None) == _native.SKM_OK           # no samples yet
    sample_set.add_batch(2, 0, _batch(oracle, pairs21, True))
    assert hip.skm_sample_set_keep_bias(h, 0) == _native.SKM_ERR_STATE              # the set holds units
    assert hip.skm_sample_set_keep_bias(h, 1) == _native.SKM_ERR_STATE
    assert hip.skm_sample_set_bias_observed(h, 2, p) == _native.SKM_ERR_ARG         # three samples are named
    assert hip.skm_sample_set_bias_observed(h, 3, None) == _native.SKM_ERR_ARG
    assert hip.skm_sample_set_bias_observed(None, 3, p) == _native.SKM_ERR_ARG
    out[:] = -1
    assert hip.skm_sample_set_bias_observed(h, 4, p) == _native.SKM_OK
    assert not out[:2].any() and out[2].sum() > 0 and (out[3] == -1).all()          # samples 0 and 1 have no units
    alone = mapper.MapResult(chr21_index, bias=True)
    mapper.ReadMapper(chr21_index, alone).map_batch(_batch(oracle, pairs21, True))
    np.testing.assert_array_equal(out[2], alone.bias_observed())
    # rows of 32 KB by sample number within 1 GiB: samples below 2^15
    limit = 1 << 15
    with pytest.raises(ValueError):
        sample_set.add_batch(limit, 0, _batch(oracle, pairs21, True))
    with pytest.raises(ValueError):
        _add(oracle, sample_set, limit + 5, pairs21, True, packed=True)
    assert len(sample_set) == 3
    plain = mapper.SampleSet(chr21_index, True)                                     # (a set that does not count takes it)
    plain.add_batch(limit, 0, _batch(oracle, [], True))
    assert len(plain) == limit + 1


# ------------------------------------------------------------------------------------ correction of many
def _close(got, want, rel):
    got, want = np.asarray(got), np.asarray(want)
    np.testing.assert_array_equal(got[want == 0], 0)
    seen = want != 0
    error = np.abs(got[seen] - want[seen]) / np.abs(want[seen])
    assert error.max() <= rel, error.max()


@pytest.fixture(scope='module')
def first_passes(oracle, native_libs, chr21, chr21_index):
    """Three samples mapped alone on chr21 with counting on: [(summary, TPM of the first pass, observed), ...]"""
    from seekmer_amd import infer, mapper
    out = []
    for i in (0, LARGE, ODD):
        reads = _samples(chr21[1], True)[i]
        result = mapper.MapResult(chr21_index, bias=True)
        mapper.ReadMapper(chr21_index, result).map_batch(_batch(oracle, reads, True))
        summary = result.summarize().detach()
        out.append((summary, infer.quantify(summary), result.bias_observed()))
    return out


def _rows(first_passes, windows):
    """The five rows of the correction tests: (summaries, tpms, observed)"""
    from seekmer_amd import mapper
    summary, tpm, _ = first_passes[1]
    rng = np.random.default_rng(12)
    eff = summary.effective_lengths.astype('f8')
    made_up = rng.integers(0, 400, 4096)
    one = np.zeros(tpm.size)
    one[next(t for t, w in enumerate(windows) if 600 <= w.size <= 1200)] = 1e6
    other_eff = eff * rng.uniform(0.5, 2.0, eff.size)
    tpms = np.vstack([tpm, tpm, one, np.zeros(tpm.size), first_passes[0][1]])
    observed = np.vstack([made_up, np.zeros(4096, dtype=np.int64), made_up, made_up, rng.integers(0, 30, 4096)])
    summaries = [mapper.SummarizedResult(0, 0, 0, None, None, None, e) for e in (eff, eff, eff, eff, other_eff)]
    assert (tpm > 0).sum() > 1 and (first_passes[0][1] > 0).sum() > 1
    return summaries, tpms, observed


def _with_env(name, value, call):
    saved = os.environ.get(name)
    os.environ[name] = value
    try:
        return call()
    finally:
        if saved is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = saved


@pytest.mark.parametrize('strand', STRANDS)
def test_every_row_is_the_single_call(native_libs, chr21_index, chr21_windows, first_passes, strand):
    from seekmer_amd import infer
    summaries, tpms, observed = _rows(first_passes, chr21_windows)
    call = lambda s=slice(None): infer.bias_correct_many(chr21_index, summaries[s], tpms[s], observed[s], strand)   # noqa: E731
    many = call()
    assert [a.shape for a in many] == [(5, tpms.shape[1]), (5, 4096), (5, 4096)]
    for k in range(5):
        single = infer.bias_correct(chr21_index, summaries[k], tpms[k], observed[k], strand)
        for got, want, what in zip(many, single, ("eff'", 'b', 'E')):
            assert got[k].tobytes() == want.tobytes(), (k, what)
    assert (many[1][1] == 1).all() and (many[1][3] == 1).all() and not many[2][3].any()    # nothing observed; nothing expected
    assert many[0][3].tobytes() == summaries[3].effective_lengths.tobytes()
    assert many[1][0].min() < 1 < many[1][0].max() and (many[2][2] == 0).sum() > 1000
    assert many[0][4].tobytes() != many[0][0].tobytes()
    # groups of 2, 2, 1 and other grids: the same bits
    runs = [_with_env('SKM_BIAS_MANY_GROUP', '2', call), _with_env('SKM_BIAS_BLOCKS', '1', call),
            _with_env('SKM_BIAS_BLOCKS', '3', call), _with_env('SKM_BIAS_MANY_GROUP', '1', call), call()]
    for run in runs:
        for got, want in zip(run, many):
            assert got.tobytes() == want.tobytes()
    # row 0 against the reference
    want_e, want_b, want_eff = ref.correct(chr21_windows, observed[0], tpms[0], summaries[0].effective_lengths.astype('f8'), strand)
    _close(many[2][0], want_e, 1e-9)
    _close(many[1][0], want_b, 1e-9)
    _close(many[0][0], want_eff, 1e-9)
    # one row, no row, and every count of rows up to the five (tails of every group width)
    for n in (1, 2, 3, 4):
        for got, want in zip(call(slice(0, n)), many):
            assert got.tobytes() == want[:n].tobytes(), n
    for got, want in zip(call(slice(4, 5)), many):
        assert got.tobytes() == want[4:].tobytes()
    assert [a.shape for a in call(slice(0, 0))] == [(0, tpms.shape[1]), (0, 4096), (0, 4096)]


def test_many_checks_every_row_before_any_device_work(native_libs, chr21_index, chr21_windows, first_passes):
    from seekmer_amd import infer
    summaries, tpms, observed = _rows(first_passes, chr21_windows)
    infer.bias_correct_many(chr21_index, summaries[:1], tpms[:1], observed[:1], None)          # (the pool is built)
    hip, handle, p = native_libs.hip(), chr21_index.device_handle(0), native_libs.ptr
    n_tx = tpms.shape[1]
    eff = np.ascontiguousarray(np.vstack([s.effective_lengths for s in summaries]), dtype='f8')
    out = np.full((5, n_tx), -3.0)
    args = lambda o=observed, t=tpms, strand=0, n=5, width=n_tx: (                              # noqa: E731
        handle, strand, n, p(np.ascontiguousarray(o, dtype=np.int64), native_libs.c_i64p), p(np.ascontiguousarray(t), native_libs.c_f64p),
        p(eff, native_libs.c_f64p), width, None, None, p(out, native_libs.c_f64p))
    for bad in (np.nan, np.inf, -1.0):
        wrong = tpms.copy()
        wrong[4, 7] = bad                                                                      # in the last row
        assert hip.skm_bias_correct_many(*args(t=wrong)) == native_libs.SKM_ERR_ARG
    negative = observed.copy()
    negative[3, 9] = -1
    assert hip.skm_bias_correct_many(*args(o=negative)) == native_libs.SKM_ERR_ARG
    huge = tpms.copy()
    huge[4] = 1e308
    assert hip.skm_bias_correct_many(*args(t=huge)) == native_libs.SKM_ERR_ARG                 # a total that cannot be scaled
    assert hip.skm_bias_correct_many(*args(strand=3)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct_many(*args(n=-1)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct_many(*args(width=n_tx - 1)) == native_libs.SKM_ERR_ARG
    assert (out == -3.0).all()                                                                 # nothing was written
    assert hip.skm_bias_correct_many(*args(n=0)) == native_libs.SKM_OK and (out == -3.0).all()
    assert hip.skm_bias_correct_many(*args()) == native_libs.SKM_OK and (out != -3.0).all()


def test_many_without_a_pool_is_refused(native_libs, oracle):
    ids, seqs = ref.synthetic_transcriptome()
    index = make_product_index(oracle.build_index(seqs, ids), ids)                              # (a handle of its own)
    n_tx = len(seqs)
    observed, tpm, out = np.zeros((2, 4096), dtype=np.int64), np.ones((2, n_tx)), np.zeros((2, n_tx))
    p = native_libs.ptr
    assert native_libs.hip().skm_bias_correct_many(
        index.device_handle(0), 0, 2, p(observed, native_libs.c_i64p), p(tpm, native_libs.c_f64p), p(tpm, native_libs.c_f64p),
        n_tx, None, None, p(out, native_libs.c_f64p)) == native_libs.SKM_ERR_STATE


@pytest.mark.parametrize('strand', STRANDS)
def test_many_on_the_synthetic_transcriptome(native_libs, oracle, strand):
    """Transcripts of 25 and of 10 bases (the latter without a window), three rows."""
    from seekmer_amd import infer, mapper
    ids, seqs = ref.synthetic_transcriptome()
    oindex = oracle.build_index(seqs, ids)
    index = make_product_index(oindex, ids)
    bases, known = ref.rebuild_transcripts(oindex.contigs, oindex.sequences, oindex.targets, oindex.lengths)
    windows = [ref.windows(b, k) for b, k in zip(bases, known)]
    assert windows[5].size == 0 and windows[4].size == 20
    rng = np.random.default_rng(2)
    effs = [rng.uniform(1.0, 300.0, len(seqs)) for _ in range(3)]
    summaries = [mapper.SummarizedResult(0, 0, 0, None, None, None, eff) for eff in effs]
    tpms = rng.uniform(0.001, 1e5, (3, len(seqs)))
    tpms[0, 1] = 0
    tpms[2] = 0                                                                                 # nothing expected: b = 1
    observed = rng.integers(0, 30, (3, 4096))
    many = infer.bias_correct_many(index, summaries, tpms, observed, strand)
    for k in range(3):
        single = infer.bias_correct(index, summaries[k], tpms[k], observed[k], strand)
        for got, want in zip(many, single):
            assert got[k].tobytes() == want.tobytes(), k
        assert many[0][k][5] == effs[k][5]                                                      # n_t = 0 keeps eff_t exactly
    assert many[0][0][4] != effs[0][4] and (many[1][2] == 1).all()
    want_e, want_b, want_eff = ref.correct(windows, observed[1], tpms[1], effs[1], strand)
    _close(many[2][1], want_e, 1e-9)
    _close(many[1][1], want_b, 1e-9)
    _close(many[0][1], want_eff, 1e-9)


# ----------------------------------------------------------------------------------------- second pass
def test_tables_start_from_the_rows_given(native_libs, chr21_index, first_passes):
    from seekmer_amd import infer
    corrected = [infer.bias_pass(chr21_index, summary, tpm, observed, None)[0] for summary, tpm, observed in first_passes]
    firsts = np.vstack([tpm for _, tpm, _ in first_passes])
    out, iters = infer.quantify_tables(corrected, x0s=firsts, return_iters=True)
    default = infer.quantify_tables(corrected)
    for k, summary in enumerate(corrected):
        want, want_iters = infer.quantify(summary, x0=firsts[k], return_iters=True)
        assert out[k].tobytes() == want.tobytes() and int(iters[k]) == want_iters, k
        assert default[k].tobytes() == infer.quantify(summary).tobytes(), k                     # x0s=None: as ever
    assert out.tobytes() != default.tobytes() or (iters != infer.quantify_tables(corrected, return_iters=True)[1]).any()
    # rows that are not normalised are normalised as quantify() does it
    scaled = firsts * np.asarray([[3.0], [0.5], [1e-3]])
    again = infer.quantify_tables(corrected, x0s=scaled)
    for k, summary in enumerate(corrected):
        assert again[k].tobytes() == infer.quantify(summary, x0=scaled[k]).tobytes(), k


@pytest.mark.parametrize('strand', [None, 'rf'])
def test_pass_of_many_equals_the_pass_of_each(native_libs, chr21_index, first_passes, strand, monkeypatch):
    """64 samples (three different ones, repeated) so that the second EM runs in shared launches; then the loop."""
    from seekmer_amd import impute, infer
    n = 64
    picks = [first_passes[k % 3] for k in range(n)]
    summaries = [pick[0] for pick in picks]
    tpms = np.vstack([pick[1] for pick in picks])
    observed = np.vstack([pick[2] for pick in picks])
    singles = [infer.bias_pass(chr21_index, *first_passes[k], strand) for k in range(3)]
    monkeypatch.delenv('SKM_SET_QUANT_SERIAL', raising=False)
    assert impute.use_set_quant(n, tpms.shape[1], sum(s.class_count.size for s in summaries))
    for serial in (False, True):
        if serial:
            monkeypatch.setenv('SKM_SET_QUANT_SERIAL', '1')
            assert not impute.use_set_quant(n, tpms.shape[1], sum(s.class_count.size for s in summaries))
        passed, second = infer.bias_pass_many(chr21_index, summaries, tpms, observed, strand)
        assert len(passed) == n and second.shape == tpms.shape
        for k in range(n):
            want_summary, want = singles[k % 3]
            assert second[k].tobytes() == want.tobytes(), (serial, k)
            assert passed[k].effective_lengths.tobytes() == want_summary.effective_lengths.tobytes()
            assert passed[k].bias_weights.tobytes() == want_summary.bias_weights.tobytes()
            np.testing.assert_array_equal(passed[k].bias_observed, want_summary.bias_observed)
            assert passed[k].class_count is summaries[k].class_count and passed[k].total == summaries[k].total
    # outside the regime (three samples): the loop, the same rows
    monkeypatch.delenv('SKM_SET_QUANT_SERIAL')
    assert not impute.use_set_quant(3, tpms.shape[1], sum(s.class_count.size for s in summaries[:3]))
    passed, second = infer.bias_pass_many(chr21_index, summaries[:3], tpms[:3], observed[:3], strand)
    for k in range(3):
        assert second[k].tobytes() == singles[k][1].tobytes()


# ------------------------------------------------------------------------------------------ end to end
def _write_fastq(path, names, reads):
    with open(path, 'wb') as f:
        for name, read in zip(names, reads):
            f.write(b'@' + name + b'\n' + read + b'\n+\n' + b'I' * len(read) + b'\n')


@pytest.fixture(scope='module')
def index_file(native_libs, tmp_path_factory):
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('set_bias_index')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(path)]) == 0
    return path


def _same_folder(a, b):
    """Two output folders hold the same files with the same bytes, but for the start time and the call."""
    import json
    assert sorted(f.name for f in a.iterdir()) == sorted(f.name for f in b.iterdir())
    for f in a.iterdir():
        if f.name == 'abundance.npz':
            x, y = np.load(f), np.load(b / f.name)
            assert sorted(x.files) == sorted(y.files)
            for name in x.files:
                if name not in ('aux/call', 'aux/start_time'):
                    assert x[name].dtype == y[name].dtype and x[name].tobytes() == y[name].tobytes(), (f.name, name)
        elif f.name == 'run_info.json':
            i, j = json.load(f.open()), json.load((b / f.name).open())
            for info in (i, j):
                info.pop('start_time'), info.pop('call')
            assert i == j
        else:
            assert f.read_bytes() == (b / f.name).read_bytes(), f.name


@pytest.mark.parametrize('options', [[], ['--fr-stranded'], ['-s', '-l', '200', '--sd', '20']],
                         ids=['paired', 'fr-stranded', 'single-ended'])
def test_infer_many_takes_the_set_and_writes_the_same_files(native_libs, chr21, index_file, tmp_path, caplog, monkeypatch,
                                                            options):
    from seekmer_amd import __main__ as cli
    single = '-s' in options
    samples = _samples(chr21[1], True)
    groups = [[os.path.join(GOLDEN, '20_1.fastq'), os.path.join(GOLDEN, '20_2.fastq')]]
    for name, reads in (('large', samples[LARGE]), ('few', samples[UNALIGNED] + samples[0][:24])):   # few: twelve units of 62 can align
        files = [tmp_path / (name + '_1.fastq'), tmp_path / (name + '_2.fastq')]
        for s in range(2):
            _write_fastq(files[s], [b'u%d' % u for u in range(len(reads) // 2)], reads[s::2])
        groups.append([str(f) for f in files])
    if single:
        groups = [group[:1] for group in groups]
    names = ['golden', 'large', 'few']
    common_options = ['--bias', '-b', '2', '--seed', '5', *options]
    fastq = [path for group in groups for path in group]
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    monkeypatch.delenv('SKM_SET_QUANT_SERIAL', raising=False)
    through_set, one_by_one = tmp_path / 'set', tmp_path / 'one_by_one'
    with caplog.at_level(logging.INFO):
        assert cli.main(['infer-many', str(index_file), str(through_set), *fastq, '--names', ','.join(names), *common_options]) == 0
    assert any('Mapping 3 samples in shared launches' in record.getMessage() for record in caplog.records)
    assert sum('Sequence bias:' in record.getMessage() for record in caplog.records) == 3
    caplog.clear()
    monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', '1')
    with caplog.at_level(logging.INFO):
        assert cli.main(['infer-many', str(index_file), str(one_by_one), *fastq, '--names', ','.join(names), *common_options]) == 0
    assert not any('in shared launches' in record.getMessage() for record in caplog.records)
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE')
    assert (through_set / 'samples.tsv').read_bytes() == (one_by_one / 'samples.tsv').read_bytes()
    assert sorted(f.name for f in through_set.iterdir()) == sorted(names + ['samples.tsv'])
    for name, group in zip(names, groups):
        _same_folder(through_set / name, one_by_one / name)
        alone = tmp_path / ('alone_' + name)
        assert cli.main(['infer', str(index_file), str(alone), *group, *common_options]) == 0
        _same_folder(through_set / name, alone)
        arrays = np.load(through_set / name / 'abundance.npz')
        if name == 'large':
            assert arrays['aux/bias_observed'].sum() > 100 and not (arrays['aux/bias_normalized'] == 1).all()
        if name == 'few':
            assert arrays['aux/bias_observed'].sum() <= 12
