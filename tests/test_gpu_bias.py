"""Sequence-bias correction (--bias) on the GPU against tests/bias_reference.py.

Integer outputs (the transcript pool, the observed hexamer counts) are exact.  E / sum E, b and eff' are held to
1e-9 relative, the bound of the EM steps against the oracle: E is accumulated in 96-bit fixed point, whose
error ("Sequence bias") is at most 1 / (2 W_min) per bin, below 1e-14 for the abundances used here.
eff' from the device's own b is held to 1e-12: fixed-order f64 sums of at most 1e5 positive terms."""
import json
import logging
import math
import os

import numpy as np
import pytest

import bias_reference as ref
from conftest import GOLDEN, make_product_index

pytestmark = pytest.mark.gpu

STRANDS = [None, 'fr', 'rf']


# ---------------------------------------------------------------------------------------------- inputs
def _units(seqs, pairs21, n_synthetic=200, read_len=100):
    """The golden 21 pairs, then synthetic pairs of chr21 fragments (either mate may come first) with the
    cases of the counting rule: reads as [mate 1, mate 2, mate 1, ...] and the kind of every unit."""
    rng = np.random.default_rng(314)
    long_tx = [s.upper() for s in seqs if len(s) > 450 and set(s.upper()) <= set(b'ACGT')]
    reads, kinds = list(pairs21), ['golden'] * (len(pairs21) // 2)
    names = ['plain', 'lower6', 'n6', 'n7', 'garbage', 'lower_mate2', 'lower_all', 'plain']
    for u in range(n_synthetic):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(150, 401))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        mates = [bytearray(f[:read_len]), bytearray(ref.reverse_complement(f[-read_len:]))]
        if rng.integers(2):
            mates.reverse()
        kind = names[u % len(names)]
        if kind == 'lower6':                         # a lower-case letter within the first six bases
            q = int(rng.integers(6))
            mates[0][q:q + 1] = bytes(mates[0][q:q + 1]).lower()
        elif kind == 'n6':                           # an N within the first six bases
            mates[0][int(rng.integers(6))] = ord('N')
        elif kind == 'n7':                           # an N at base 7 only
            mates[0][6] = ord('N')
        elif kind == 'garbage':                      # unaligned
            mates = [bytearray(bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, read_len))) for _ in range(2)]
        elif kind == 'lower_mate2':                  # mate 2's first bases are not what counts
            mates[1][:6] = bytes(mates[1][:6]).lower()
        elif kind == 'lower_all':
            mates[0] = bytearray(bytes(mates[0]).lower())
        assert mates[0] != mates[1]
        reads += [bytes(mates[0]), bytes(mates[1])]
        kinds.append(kind)
    return reads, kinds


def _streams_of(common, bases, offsets, n_units, paired):
    """The reads of a flat batch as one packed piece per stream (mate 1 reads, mate 2 reads)."""
    mates = 2 if paired else 1
    lengths = np.diff(offsets)
    pieces = []
    for s in range(mates):
        sel = np.arange(s, mates * n_units, mates)
        sub_offsets = np.zeros(n_units + 1, dtype=np.int64)
        np.cumsum(lengths[sel], out=sub_offsets[1:])
        sub = np.concatenate([bases[offsets[r]:offsets[r + 1]] for r in sel] + [np.zeros(1, np.uint8)])
        pieces.append(common.PackedReads.from_ascii(sub, sub_offsets, stream=s, paired=paired))
    return pieces


def _cut(common, piece, borders):
    codes, lengths = piece.codes, piece.lengths
    exc_reads, exc_masks = piece.exceptions
    out = []
    for lo, hi in zip(borders[:-1], borders[1:]):
        sel = (exc_reads >= lo) & (exc_reads < hi)
        out.append(common.PackedReads.from_arrays(piece.stream, lo, codes[lo:hi], lengths[lo:hi],
                                                  exc_reads[sel] - lo, exc_masks[sel], paired=piece.paired))
    return out


@pytest.fixture(scope='module')
def chr21_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


@pytest.fixture(scope='module')
def chr21_windows(chr21, chr21_oracle_index):
    """(bases, known, h+ of every window) of every chr21 transcript, rebuilt by the reference's rule"""
    ix = chr21_oracle_index
    bases, known = ref.rebuild_transcripts(ix.contigs, ix.sequences, ix.targets, ix.lengths)
    return bases, known, [ref.windows(b, k) for b, k in zip(bases, known)]


@pytest.fixture(scope='module')
def synthetic(oracle):
    ids, seqs = ref.synthetic_transcriptome()
    oindex = oracle.build_index(seqs, ids)
    bases, known = ref.rebuild_transcripts(oindex.contigs, oindex.sequences, oindex.targets, oindex.lengths)
    return ids, seqs, make_product_index(oindex, ids), bases, known, [ref.windows(b, k) for b, k in zip(bases, known)]


@pytest.fixture(scope='module')
def first_pass(oracle, native_libs, chr21, chr21_index, pairs21):
    """The units of _units mapped on chr21 with counting on: (summary, TPM of the first pass, observed)"""
    from seekmer_amd import common, infer, mapper
    reads, _ = _units(chr21[1], pairs21)
    bases, offsets = oracle.pack_reads(reads)
    result = mapper.MapResult(chr21_index, bias=True)
    mapper.ReadMapper(chr21_index, result).map_batch(common.ReadBatch(len(reads) // 2, bases, offsets, True))
    summary = result.summarize().detach()
    return summary, infer.quantify(summary), result.bias_observed()


def _pool(native, index):
    """(bases, known) of the device's transcript pool, transcripts back to back"""
    lengths = np.ascontiguousarray(index.transcripts['length'], dtype='f8')
    handle = index.device_handle(0)
    native.check(native.hip().skm_index_build_transcripts(handle, native.ptr(lengths, native.c_f64p), lengths.size))
    total = int(lengths.sum())
    bases = np.zeros(total, dtype='S1')
    known = np.zeros(total, dtype=np.uint8)
    native.check(native.hip().skm_index_transcript_bases(handle, bases.ctypes.data, known.ctypes.data))
    return bases, known


# ------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize('source', ['chr21', 'synthetic'])
def test_pool_equals_the_fasta(native_libs, chr21, chr21_index, chr21_windows, synthetic, source):
    if source == 'chr21':
        seqs, index, want_bases, want_known = chr21[1], chr21_index, chr21_windows[0], chr21_windows[1]
    else:
        seqs, index, want_bases, want_known = synthetic[1], synthetic[2], synthetic[3], synthetic[4]
    bases, known = _pool(native_libs, index)
    np.testing.assert_array_equal(known.astype(bool), np.concatenate(want_known))
    assert bases.tobytes() == b''.join(bytes(b) for b in want_bases)
    fasta = np.frombuffer(b''.join(s.upper() for s in seqs), dtype='S1')
    mask = known.astype(bool)
    np.testing.assert_array_equal(bases[mask], fasta[mask])
    assert bytes(bases[~mask].tobytes()) == b'N' * int((~mask).sum())
    if source == 'synthetic':
        first = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        assert not mask[first[5]:first[6]].any() and mask[first[4]:first[5]].all()   # 10 bases: unknown; 25: known
        assert mask.sum() == mask.size - 10
    else:
        assert mask.mean() > 0.99


def test_pool_state_and_argument_rules(native_libs, oracle, synthetic):
    ids, seqs = synthetic[0], synthetic[1]
    index = make_product_index(oracle.build_index(seqs, ids), ids)          # (a handle of its own)
    hip, handle = native_libs.hip(), index.device_handle(0)
    lengths = np.ascontiguousarray(index.transcripts['length'], dtype='f8')
    p = native_libs.ptr
    observed, tpm, out = np.zeros(4096, dtype=np.int64), np.ones(lengths.size), np.zeros(lengths.size)
    args = lambda o=observed, t=tpm, n=lengths.size, strand=0: (                       # noqa: E731
        handle, strand, p(o, native_libs.c_i64p), p(t, native_libs.c_f64p), p(lengths, native_libs.c_f64p), n, None, None,
        p(out, native_libs.c_f64p))
    assert hip.skm_index_transcript_bases(handle, None, None) == native_libs.SKM_ERR_STATE
    assert hip.skm_bias_correct(*args()) == native_libs.SKM_ERR_STATE
    short = lengths - 30                                                       # rows leave these lengths
    assert hip.skm_index_build_transcripts(handle, p(short.clip(min=0), native_libs.c_f64p), short.size) == native_libs.SKM_ERR_ARG
    assert hip.skm_index_build_transcripts(handle, p(lengths, native_libs.c_f64p), lengths.size - 1) == native_libs.SKM_ERR_ARG
    assert hip.skm_index_build_transcripts(handle, p(lengths + 0.5, native_libs.c_f64p), lengths.size) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct(*args()) == native_libs.SKM_ERR_STATE          # (a refused build leaves no pool)
    assert hip.skm_index_build_transcripts(handle, p(lengths, native_libs.c_f64p), lengths.size) == native_libs.SKM_OK
    assert hip.skm_index_build_transcripts(handle, p(lengths, native_libs.c_f64p), lengths.size) == native_libs.SKM_OK
    longer = np.concatenate([lengths, [100.0]])
    assert hip.skm_index_build_transcripts(handle, p(longer, native_libs.c_f64p), longer.size) == native_libs.SKM_ERR_STATE
    assert hip.skm_bias_correct(*args()) == native_libs.SKM_OK
    for bad in (np.nan, np.inf, -1.0):
        wrong = tpm.copy()
        wrong[2] = bad
        assert hip.skm_bias_correct(*args(t=wrong)) == native_libs.SKM_ERR_ARG
    negative = observed.copy()
    negative[7] = -1
    assert hip.skm_bias_correct(*args(o=negative)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct(*args(strand=3)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct(*args(n=-1)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct(*args(n=lengths.size - 1)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct(handle, 0, None, p(tpm, native_libs.c_f64p), p(lengths, native_libs.c_f64p), lengths.size,
                                None, None, p(out, native_libs.c_f64p)) == native_libs.SKM_ERR_ARG
    assert hip.skm_bias_correct(handle, 0, p(observed, native_libs.c_i64p), p(tpm, native_libs.c_f64p),
                                p(lengths, native_libs.c_f64p), lengths.size, None, None, None) == native_libs.SKM_ERR_ARG


# -------------------------------------------------------------------------------------------- observed
@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('strand', STRANDS)
def test_observed_counts_equal_a_counter_for_every_input_form(oracle, native_libs, chr21, chr21_index, pairs21, strand, paired):
    from seekmer_amd import _native, common, mapper
    index = chr21_index
    reads, kinds = _units(chr21[1], pairs21)
    if not paired:
        reads = reads[0::2]
    first_reads = reads[0::2] if paired else reads
    mates = 2 if paired else 1
    n_units = len(first_reads)
    assert n_units == 221 and all(len(r) == 100 for r in reads)
    bases, offsets = oracle.pack_reads(reads)

    # the ASCII batch; the units last_batch reports as aligned are the ones to count
    result = mapper.MapResult(index, strand=strand, bias=True)
    rm = mapper.ReadMapper(index, result)
    rm.map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    counts, _ = rm.last_tuples(n_units)
    aligned = counts > 0
    want = ref.observed_counts(first_reads, aligned)
    valid = np.asarray([ref.hexamer_code(r[:6]) >= 0 for r in first_reads])
    kinds = np.asarray(kinds)
    print(strand, 'paired' if paired else 'single', 'aligned', int(aligned.sum()), 'counted', int(want.sum()),
          {k: (int((aligned & (kinds == k)).sum()), int((kinds == k).sum())) for k in sorted(set(kinds))})
    assert want.sum() == (aligned & valid).sum() > 20
    assert (aligned & ~valid).any() and (~aligned & valid).any()          # skipped for its bases / for not aligning
    assert (aligned & (kinds == 'n7')).any() and (aligned & (kinds == 'lower_mate2')).any()
    if strand is None:
        assert (aligned & np.isin(kinds, ['lower6', 'n6', 'lower_all'])).any()
    assert not aligned[kinds == 'garbage'].any()
    got = result.bias_observed()
    assert got.dtype == np.int64 and got.shape == (4096,)
    np.testing.assert_array_equal(got, want)

    result.reset()                                                         # reset zeroes, the setting stays
    assert not result.bias_observed().any()
    # uniform batches, out of order
    for lo, hi in ((77, n_units), (0, 77)):
        piece = common.ReadBatch(hi - lo, bases, offsets[mates * lo:mates * hi + 1], paired, first_unit=lo)
        piece.uniform_len = 100
        rm.map_batch_async(piece)
    np.testing.assert_array_equal(result.bias_observed(), want)
    # packed pieces, cut at two different places
    streams = _streams_of(common, bases, offsets, n_units, paired)
    assert sum(p.raw.n_exceptions for p in streams) > 50
    for borders in ([[0, 1, 60, 61, n_units], [0, 30, 199, n_units]], [[0, 110, n_units], [0, 5, 6, 150, 220, n_units]]):
        result.reset()
        pieces = [p for s, piece in enumerate(streams) for p in _cut(common, piece, borders[s])]
        for k in np.random.default_rng(len(pieces)).permutation(len(pieces)):
            rm.push_packed(pieces[k])
        np.testing.assert_array_equal(result.bias_observed(), want)
        assert result.sizes()[3] == n_units
    result.clear()                                                         # clear keeps the counts, as the histogram
    np.testing.assert_array_equal(result.bias_observed(), want)
    rm.map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    np.testing.assert_array_equal(result.bias_observed(), 2 * want)

    plain = mapper.MapResult(index, strand=strand)                         # a mapper that was not asked to count
    mapper.ReadMapper(index, plain).map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    out = np.zeros(4096, dtype=np.int64)
    assert _native.hip().skm_mapper_bias_observed(plain._handle, _native.ptr(out, _native.c_i64p)) == _native.SKM_ERR_STATE
    with pytest.raises(_native.NativeError):
        plain.bias_observed()


def test_counting_state_rules(oracle, native_libs, chr21, chr21_index, pairs21):
    from seekmer_amd import _native, common, mapper
    hip = _native.hip()
    bases, offsets = oracle.pack_reads(pairs21)
    batch = common.ReadBatch(21, bases, offsets, True)
    result = mapper.MapResult(chr21_index)
    rm = mapper.ReadMapper(chr21_index, result)
    h = result._handle
    assert hip.skm_mapper_set_bias(h, 1) == _native.SKM_OK
    assert hip.skm_mapper_set_bias(h, 0) == _native.SKM_OK
    assert hip.skm_mapper_set_bias(h, 1) == _native.SKM_OK
    rm.map_batch(batch)
    want = ref.observed_counts(pairs21[0::2], rm.last_tuples(21)[0] > 0)
    assert want.sum() > 0
    assert hip.skm_mapper_set_bias(h, 0) == _native.SKM_ERR_STATE           # the handle holds units
    assert hip.skm_mapper_set_bias(h, 1) == _native.SKM_ERR_STATE
    np.testing.assert_array_equal(_observed(result), want)
    # tables merged in add no observations
    other = mapper.MapResult(chr21_index, bias=True)
    mapper.ReadMapper(chr21_index, other).map_batch(batch)
    offs, targets, counts, first, fld = other.export()
    result.merge_table(offs, targets, counts, first, other.sizes()[2], fld)
    result.merge_resident(other)
    np.testing.assert_array_equal(_observed(result), want)
    result.reset()
    assert hip.skm_mapper_set_bias(h, 0) == _native.SKM_OK                  # an empty handle again
    rm.map_batch(batch)
    out = np.zeros(4096, dtype=np.int64)
    assert hip.skm_mapper_bias_observed(h, _native.ptr(out, _native.c_i64p)) == _native.SKM_ERR_STATE
    result.reset()
    rm.map_batch_async(batch)                                              # a queued batch: no change under it
    assert hip.skm_mapper_set_bias(h, 1) == _native.SKM_ERR_STATE
    result.sync()


def _observed(result):
    from seekmer_amd import _native
    out = np.zeros(4096, dtype=np.int64)
    _native.check(_native.hip().skm_mapper_bias_observed(result._handle, _native.ptr(out, _native.c_i64p)))
    return out


# ------------------------------------------------------------------------------------ expected, b, eff'
def _close(got, want, rel):
    got, want = np.asarray(got), np.asarray(want)
    np.testing.assert_array_equal(got[want == 0], 0)
    seen = want != 0
    error = np.abs(got[seen] - want[seen]) / np.abs(want[seen])
    assert error.max() <= rel, error.max()
    return float(error.max())


def _check_correction(index, windows, summary, tpm, observed, strand):
    from seekmer_amd import infer
    eff = summary.effective_lengths.astype('f8')
    corrected, b, expected = infer.bias_correct(index, summary, tpm, observed, strand)
    want_e, want_b, want_eff = ref.correct(windows, observed, tpm, eff, strand)
    total, want_total = math.fsum(expected), math.fsum(want_e)
    errors = {}
    if want_total > 0:
        errors['E/sum E'] = _close(expected / total, want_e / want_total, 1e-9)
        errors['E'] = _close(expected, want_e, 1e-9)
    else:
        assert not expected.any()
    errors['b'] = _close(b, want_b, 1e-9)
    errors["eff'"] = _close(corrected, want_eff, 1e-9)
    errors["eff' from the device's b"] = _close(corrected, ref.corrected_lengths(eff, windows, b, strand), 1e-12)
    print(strand, {k: '%.2e' % v for k, v in errors.items()})
    empty = np.asarray([w.size == 0 for w in windows])
    np.testing.assert_array_equal(corrected[empty], eff[empty])             # n_t = 0 keeps eff_t exactly
    # the same bits on every run and for every grid
    runs = [(corrected, b, expected), infer.bias_correct(index, summary, tpm, observed, strand)]
    saved = os.environ.get('SKM_BIAS_BLOCKS')
    try:
        for blocks in ('1', '3'):
            os.environ['SKM_BIAS_BLOCKS'] = blocks
            runs.append(infer.bias_correct(index, summary, tpm, observed, strand))
    finally:
        if saved is None:
            os.environ.pop('SKM_BIAS_BLOCKS', None)
        else:
            os.environ['SKM_BIAS_BLOCKS'] = saved
    for run in runs[1:]:
        for got, want in zip(run, runs[0]):
            assert got.tobytes() == want.tobytes()
    return corrected, b, expected


@pytest.mark.parametrize('case', ['first pass', 'nothing observed', 'one transcript'])
@pytest.mark.parametrize('strand', STRANDS)
def test_correction_equals_the_reference(native_libs, chr21_index, chr21_windows, first_pass, strand, case):
    summary, tpm, _ = first_pass
    windows = chr21_windows[2]
    observed = np.random.default_rng(12).integers(0, 400, 4096)             # made up
    if case == 'nothing observed':
        observed = np.zeros(4096, dtype=np.int64)
    if case == 'one transcript':
        tpm = np.zeros(tpm.size)
        tpm[next(t for t, w in enumerate(windows) if 600 <= w.size <= 1200)] = 1e6
    assert (tpm > 0).sum() == (1 if case == 'one transcript' else (tpm > 0).sum()) > 0
    corrected, b, expected = _check_correction(chr21_index, windows, summary, tpm, observed, strand)
    if case == 'nothing observed':
        assert (b == 1).all()
    elif case == 'first pass':
        assert b.min() < 1 < b.max()
    else:                                   # (the few hexamers of one transcript hold all of E: b < 1 there)
        assert (expected == 0).sum() > 1000 and (b[expected == 0] == 1).all() and (b[expected > 0] < 1).all()


@pytest.mark.parametrize('strand', STRANDS)
def test_correction_on_the_synthetic_transcriptome(native_libs, synthetic, strand):
    """Transcripts of 25 and of 10 bases (the latter without a window) and both orientations of one segment."""
    from seekmer_amd import mapper
    ids, seqs, index, _, _, windows = synthetic
    assert windows[5].size == 0 and windows[4].size == 20
    rng = np.random.default_rng(2)
    eff = rng.uniform(1.0, 300.0, len(seqs))
    summary = mapper.SummarizedResult(0, 0, 0, None, None, None, eff)
    tpm = rng.uniform(0.001, 1e5, len(seqs))
    tpm[1] = 0
    observed = rng.integers(0, 30, 4096)
    corrected, _, _ = _check_correction(index, windows, summary, tpm, observed, strand)
    assert corrected[5] == eff[5] and corrected[4] != eff[4]
    _check_correction(index, windows, summary, np.zeros(len(seqs)), observed, strand)      # nothing expected: b = 1


# ------------------------------------------------------------------------------------------ end to end
def _digits(field, value, rel):
    """`field`, a number printed with %g, against `value`: within half a unit of its sixth significant digit,
    plus `rel` of the value for what the printed number itself may differ by."""
    value = float(value)
    if value == 0:
        return float(field) == 0
    half_unit = 0.5 * 10.0 ** (math.floor(math.log10(abs(value))) - 5)
    return abs(float(field) - value) <= half_unit * (1 + 1e-9) + rel * abs(value)


def _write_fastq(path, names, reads):
    with open(path, 'wb') as f:
        for name, read in zip(names, reads):
            f.write(b'@' + name + b'\n' + read + b'\n+\n' + b'I' * len(read) + b'\n')


@pytest.fixture(scope='module')
def index_file(native_libs, tmp_path_factory):
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('bias_index')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(path)]) == 0
    return path


def _same_outputs(a, b):
    """Two output folders hold the same results: everything but the start time and the call."""
    assert (a / 'abundance.tsv').read_bytes() == (b / 'abundance.tsv').read_bytes()
    x, y = np.load(a / 'abundance.npz'), np.load(b / 'abundance.npz')
    assert sorted(x.files) == sorted(y.files)
    for name in x.files:
        if name not in ('aux/call', 'aux/start_time'):
            assert x[name].dtype == y[name].dtype and x[name].tobytes() == y[name].tobytes(), name
    i, j = json.load((a / 'run_info.json').open()), json.load((b / 'run_info.json').open())
    for info in (i, j):
        info.pop('start_time'), info.pop('call')
    assert i == j
    return x, i


def test_cli_end_to_end(oracle, native_libs, chr21, chr21_oracle_index, chr21_windows, pairs21, index_file, tmp_path, caplog):
    from seekmer_amd import __main__ as cli
    fastq = [os.path.join(GOLDEN, '20_1.fastq'), os.path.join(GOLDEN, '20_2.fastq')]
    out, plain, default = tmp_path / 'bias', tmp_path / 'plain', tmp_path / 'default'
    with caplog.at_level(logging.INFO):
        assert cli.main(['infer', str(index_file), str(out), *fastq, '--bias']) == 0
    assert any('Sequence bias: 21 observed hexamers' in record.getMessage() for record in caplog.records)
    assert cli.main(['infer', str(index_file), str(plain), *fastq]) == 0

    windows = chr21_windows[2]
    lengths = chr21_oracle_index.lengths
    bases, offsets = oracle.pack_reads(pairs21)
    fld = np.zeros(2000, dtype=np.int64)
    mapped = oracle.map_batch(chr21_oracle_index, bases, offsets, 21, True, fld)
    classes = oracle.Classes()
    classes.update(mapped)
    class_map, class_count = classes.summarize()
    eff = oracle.effective_lengths(fld, lengths)
    first, _ = oracle.quantify(eff, class_map, class_count)
    observed = ref.observed_counts(pairs21[0::2], mapped.count > 0)
    assert observed.sum() == 21
    _, b, corrected = ref.correct(windows, observed, first, eff, None)
    second, _ = oracle.quantify(corrected, class_map, class_count, x0=first)
    assert np.abs(corrected / eff - 1).max() > 0.01 and (second != first).any()      # the option does something

    rows = [line.rstrip('\n').split('\t') for line in (out / 'abundance.tsv').open()]
    assert rows[0] == ['target_id', 'length', 'eff_length', 'est_count', 'tpm'] and len(rows) == 1 + len(chr21[0])
    for i, row in enumerate(rows[1:]):
        assert row[0] == chr21[0][i].decode() and row[1] == '%g' % lengths[i]
        assert _digits(row[2], np.float32(corrected[i]), 1e-9 + 2.0 ** -24), (i, row[2], corrected[i])   # (written as f4)
        assert _digits(row[4], second[i], 1e-9), (i, row[4], second[i])
    arrays = np.load(out / 'abundance.npz')
    assert arrays['aux/bias_observed'].dtype == np.dtype('i4') and arrays['aux/bias_normalized'].dtype == np.dtype('f8')
    np.testing.assert_array_equal(arrays['aux/bias_observed'], observed)
    np.testing.assert_allclose(arrays['aux/bias_normalized'], b, rtol=1e-9, atol=0)
    np.testing.assert_allclose(arrays['aux/eff_lengths'], corrected, rtol=1e-9, atol=0)
    np.testing.assert_array_equal(arrays['aux/fld'], fld.astype('i4'))
    info = json.load((out / 'run_info.json').open())
    assert info['bias'] is True and info['n_pseudoaligned'] == 21

    # without the option: the placeholders, no key, the first pass's numbers -- and the files of a run whose
    # caller does not know the option at all
    from seekmer_amd import infer
    import pathlib
    infer.run(index_file, default, [pathlib.Path(p) for p in fastq], 1, False, False, 0, False)
    arrays, info = _same_outputs(plain, default)
    assert 'bias' not in info
    assert arrays['aux/bias_observed'].tobytes() == np.ones(4096, dtype='i4').tobytes()
    assert arrays['aux/bias_normalized'].tobytes() == np.ones(4096, dtype='f8').tobytes()
    np.testing.assert_array_equal(arrays['aux/eff_lengths'], eff)
    rows = [line.rstrip('\n').split('\t') for line in (plain / 'abundance.tsv').open()]
    for i, row in enumerate(rows[1:]):
        assert row[2] == '%g' % np.float32(eff[i]) and _digits(row[4], first[i], 1e-9)


def test_infer_many_gives_the_files_of_infer(native_libs, chr21, pairs21, index_file, tmp_path):
    from seekmer_amd import __main__ as cli
    reads, _ = _units(chr21[1], pairs21)
    reads = reads[42:]                                                     # the synthetic units
    names = [b'u%d' % u for u in range(len(reads) // 2)]
    files = [tmp_path / 'synthetic_1.fastq', tmp_path / 'synthetic_2.fastq']
    for s in range(2):
        _write_fastq(files[s], names, reads[s::2])
    samples = [[os.path.join(GOLDEN, '20_1.fastq'), os.path.join(GOLDEN, '20_2.fastq')], [str(f) for f in files]]
    many = tmp_path / 'many'
    assert cli.main(['infer-many', str(index_file), str(many), *samples[0], *samples[1], '--bias', '--rf-stranded',
                     '-b', '2', '--seed', '5', '--names', 'golden,synthetic']) == 0
    for name, sample in zip(('golden', 'synthetic'), samples):
        alone = tmp_path / ('alone_' + name)
        assert cli.main(['infer', str(index_file), str(alone), *sample, '--bias', '--rf-stranded', '-b', '2', '--seed', '5']) == 0
        arrays, info = _same_outputs(many / name, alone)
        assert info['bias'] is True and info['n_bootstraps'] == 2
        assert 0 < arrays['aux/bias_observed'].sum() <= info['n_pseudoaligned']
        assert not (arrays['aux/bias_normalized'] == 1).all()


def test_bootstraps_start_from_the_corrected_result(oracle, native_libs, chr21, pairs21, index_file, tmp_path):
    """-b 2 --seed 1 --bias: the replicates are skm_quant_bootstrap_tpm called with eff' and the corrected start."""
    from seekmer_amd import __main__ as cli
    from seekmer_amd import common, infer, mapper
    reads, _ = _units(chr21[1], pairs21)
    names = [b'u%d' % u for u in range(len(reads) // 2)]
    files = [tmp_path / 'r_1.fastq', tmp_path / 'r_2.fastq']
    for s in range(2):
        _write_fastq(files[s], names, reads[s::2])
    out = tmp_path / 'out'
    assert cli.main(['infer', str(index_file), str(out), *map(str, files), '-b', '2', '--seed', '1', '--bias']) == 0
    arrays = np.load(out / 'abundance.npz')

    index = common.KMerIndex.load(index_file)
    bases, offsets = oracle.pack_reads(reads)
    result = mapper.MapResult(index, bias=True)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(len(reads) // 2, bases, offsets, True))
    summary = result.summarize()
    first = infer.quantify(summary)
    corrected_summary, second = infer.bias_pass(index, summary, first, result.bias_observed(), None)
    np.testing.assert_array_equal(arrays['aux/eff_lengths'], corrected_summary.effective_lengths)
    np.testing.assert_array_equal(arrays['aux/bias_observed'], result.bias_observed())
    quant = infer._QuantHandle.from_csr(second.size, summary.class_offsets, summary.class_targets, summary.class_count)
    try:
        x0 = second.copy()
        x0 /= x0.sum()
        replicates, _, _ = quant.bootstrap(2, 1, x0, corrected_summary.effective_lengths.astype('f8'), tpm=True)
        uncorrected, _, _ = quant.bootstrap(2, 1, x0, summary.effective_lengths.astype('f8'), tpm=True)
    finally:
        quant.close()
    for i in range(2):
        assert arrays['bootstrap/bs%d' % i].tobytes() == replicates[i].tobytes()
        assert arrays['bootstrap/bs%d' % i].tobytes() != uncorrected[i].tobytes()
