"""The fragment-length model (--fragment-length MEAN --sd SD) on the GPU: effective_lengths_weights_kernel against
the numpy rule of length_model_reference, then the three device-resident paths that read the model where it lies
in HBM (skm_quant_infer, skm_sample_set_quantify, SampleSet.summarize) and the three commands.

Every comparison is array_equal or byte for byte: the weights are made once, on the host, by the expression the
reference uses, and the device accumulates max(len - i, 1) * p[i] for i = 0..1999 in order with separate
multiplies and adds, as the numpy loop does."""
import ctypes
import json
import os

import numpy as np
import pytest

import length_model_reference as reference
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODEL = (200, 20)
OPTIONS = ['-l', '200', '--sd', '20']
READS_1 = os.path.join(GOLDEN, '20_1.fastq')
READS_2 = os.path.join(GOLDEN, '20_2.fastq')


# ---- the kernel --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rule():
    """{model: (weights, the numpy rule on the 302 test lengths)}, made once and read-only."""
    lengths = reference.transcript_lengths()
    table = {}
    for model in reference.MODELS:
        p = reference.weights(*model)
        eff = reference.effective_lengths(p, lengths)
        p.setflags(write=False)
        eff.setflags(write=False)
        table[model] = (p, eff)
    lengths.setflags(write=False)
    return lengths, table


def _device_rule(native_libs, p, lengths):
    """skm_effective_lengths_weights as it is: (status, out[n, n_tx])"""
    p = np.ascontiguousarray(p, dtype='f8').reshape(-1, 2000)
    lengths = np.ascontiguousarray(lengths, dtype='f8')
    out = np.full((p.shape[0], lengths.size), -1.0)
    f64 = native_libs.c_f64p
    code = native_libs.hip().skm_effective_lengths_weights(0, p.shape[0], native_libs.ptr(p, f64), native_libs.ptr(lengths, f64),
                                                           lengths.size, native_libs.ptr(out, f64))
    return code, out


@pytest.mark.parametrize('n_tx', [302, 1, 257])
@pytest.mark.parametrize('model', reference.MODELS)
def test_one_row_equals_the_numpy_rule(native_libs, rule, model, n_tx):
    """302 lengths are two blocks with a ragged tail, 257 one block and one thread, 1 a single thread."""
    from seekmer_amd import mapper
    lengths, table = rule
    p, eff = table[model]
    np.testing.assert_array_equal(mapper.fragment_length_weights(*model), p)
    code, out = _device_rule(native_libs, p, lengths[:n_tx])
    assert code == native_libs.SKM_OK
    assert np.isfinite(out).all() and (out > 0.0).all()
    np.testing.assert_array_equal(out[0], eff[:n_tx])


def test_the_models_reach_what_they_are_for(rule):
    _, table = rule
    occupied = {model: np.flatnonzero(table[model][0]) for model in reference.MODELS}
    assert occupied[(1.5, 0.4)][0] == 1 and table[(1.5, 0.4)][0][1:3].sum() > 0.99
    assert occupied[(1999, 50)][-1] == 1999 and table[(1999, 50)][0].argmax() == 1999
    assert table[(187.3, 0.05)][0][187] > 0.9999 and occupied[(187.3, 0.05)].size < 8
    assert occupied[(1000, 1e4)].size == 1999                 # the packed list is full


def test_rows_of_different_models(native_libs, rule, monkeypatch):
    """Three rows in one launch; five rows under SKM_EFF_MANY_GROUP=2: launches of 2, 2 and 1 rows."""
    lengths, table = rule
    monkeypatch.delenv('SKM_EFF_MANY_GROUP', raising=False)
    models = reference.MODELS[:3]
    code, out = _device_rule(native_libs, np.stack([table[model][0] for model in models]), lengths)
    assert code == native_libs.SKM_OK
    for row, model in zip(out, models):
        np.testing.assert_array_equal(row, table[model][1], err_msg=str(model))
    monkeypatch.setenv('SKM_EFF_MANY_GROUP', '2')
    code, out = _device_rule(native_libs, np.stack([table[model][0] for model in reference.MODELS]), lengths)
    assert code == native_libs.SKM_OK
    for row, model in zip(out, reference.MODELS):
        np.testing.assert_array_equal(row, table[model][1], err_msg=str(model))


def test_bad_weights_and_empty_calls(native_libs, rule):
    lengths, table = rule
    for bad in (-1e-12, float('nan')):
        p = np.stack([table[MODEL][0]] * 3)
        p[2, 700] = bad
        code, out = _device_rule(native_libs, p, lengths)
        assert code == native_libs.SKM_ERR_ARG and (out == -1.0).all()
    code, out = _device_rule(native_libs, table[MODEL][0], lengths[:0])
    assert code == native_libs.SKM_OK
    f64 = native_libs.c_f64p
    p, out = np.array(table[MODEL][0]), np.full(4, -1.0)
    assert native_libs.hip().skm_effective_lengths_weights(0, 0, native_libs.ptr(p, f64), native_libs.ptr(np.array(lengths), f64), 4,
                                                           native_libs.ptr(out, f64)) == native_libs.SKM_OK
    assert (out == -1.0).all()


# ---- one mapper --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def chr21_index(native_libs, tmp_path_factory):
    """(index path, index, the numpy rule on its transcripts): the chr21 transcriptome through `index -t`."""
    from seekmer_amd import __main__ as cli
    from seekmer_amd import common
    folder = tmp_path_factory.mktemp('length_model_index')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    index_path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(index_path)]) == 0
    index = common.KMerIndex.load(index_path)
    eff = reference.effective_lengths(reference.weights(*MODEL), index.transcripts['length'])
    eff.setflags(write=False)
    return index_path, index, eff


def _batch(reads):
    from seekmer_amd import common
    if not reads:
        return common.ReadBatch(0, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), False)
    return common.ReadBatch.from_lists(len(reads), [b'r%d' % i for i in range(len(reads))], list(reads))


def _mapped(index, reads, **kwargs):
    from seekmer_amd import mapper
    result = mapper.MapResult(index, **kwargs)
    mapper.ReadMapper(index, result).map_batch(_batch(reads))
    return result


@pytest.fixture(scope='module')
def single_reads(oracle):
    """20_1.fastq as 21 single-ended reads"""
    return oracle.read_fastq_pairs(READS_1)


def test_a_mapper_with_a_model(native_libs, chr21_index, single_reads):
    """summarize(), quantify_resident (alone and through a one-rank communicator) and quantify(summary) agree bit
    for bit on the model's lengths; the histogram and the class table do not know about the model; clearing the
    model brings the histogram's lengths back."""
    from seekmer_amd import infer, parallel
    _, index, eff = chr21_index
    plain = _mapped(index, single_reads)
    model = _mapped(index, single_reads, length_model=MODEL)
    assert model.length_model == (200.0, 20.0) and plain.length_model is None
    summary, plain_summary = model.summarize(), plain.summarize()
    assert summary.length_model == (200.0, 20.0) and plain_summary.length_model is None
    np.testing.assert_array_equal(summary.effective_lengths, eff)
    np.testing.assert_array_equal(model.effective_lengths, eff)
    assert not np.array_equal(plain_summary.effective_lengths, eff)
    # what was counted is what is counted without a model
    for ours, theirs in zip(model.export(), plain.export()):
        np.testing.assert_array_equal(ours, theirs)
    assert model.sizes() == plain.sizes() and summary.aligned > 0
    np.testing.assert_array_equal(summary.fragment_length_frequencies, plain_summary.fragment_length_frequencies)
    assert model.harmonic_mean_fragment_length == plain.harmonic_mean_fragment_length
    # the resident path against the summary's
    tpm, steps = infer.quantify(summary, return_iters=True)
    assert steps > 0 and tpm.sum() > 0
    plain_tpm, plain_steps, plain_eff = infer.quantify_resident(plain, return_iters=True, return_effective_lengths=True)
    np.testing.assert_array_equal(plain_eff, plain_summary.effective_lengths)

    def check_resident(comm):
        got_tpm, got_steps, got_eff = infer.quantify_resident(model, comm=comm, return_iters=True, return_effective_lengths=True)
        np.testing.assert_array_equal(got_eff, eff)
        assert got_steps == steps
        np.testing.assert_array_equal(got_tpm, tpm)
        # cleared, the histogram's lengths are back; set again, the model's
        model.set_length_model(None)
        back = infer.quantify_resident(model, comm=comm, return_iters=True, return_effective_lengths=True)
        assert back[1] == plain_steps
        np.testing.assert_array_equal(back[2], plain_eff)
        np.testing.assert_array_equal(back[0], plain_tpm)
        np.testing.assert_array_equal(model.summarize().effective_lengths, plain_eff)
        model.set_length_model(MODEL)

    check_resident(None)
    raw = ctypes.create_string_buffer(128)
    native_libs.check(native_libs.hip().skm_comm_unique_id(raw))
    comm = parallel.create_comm(0, raw.raw, 0, 1)
    try:
        check_resident(comm)
    finally:
        parallel.destroy_comm(comm)
    # the native setter refuses what is no weight and keeps the model it has
    bad = np.array(reference.weights(*MODEL))
    bad[3] = float('nan')
    assert native_libs.hip().skm_mapper_set_length_weights(model._handle, native_libs.ptr(bad, native_libs.c_f64p)) \
        == native_libs.SKM_ERR_ARG
    np.testing.assert_array_equal(infer.quantify_resident(model, return_effective_lengths=True)[1], eff)


# ---- a sample set ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def samples(single_reads):
    """about ten units of the fixture, no unit at all, and units that cannot align"""
    rng = np.random.default_rng(77)
    noise = [bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 75)) for _ in range(12)]
    return [list(single_reads[:10]), [], noise]


def _sample_set(index, samples, **kwargs):
    from seekmer_amd import mapper
    sample_set = mapper.SampleSet(index, False, **kwargs)
    for i, reads in enumerate(samples):
        sample_set.add_batch(i, 0, _batch(reads))
    sample_set.sync()
    return sample_set


@pytest.mark.parametrize('per_sample_lengths', [False, True], ids=['pooled', 'per_sample'])
def test_a_sample_set_with_a_model(native_libs, chr21_index, samples, per_sample_lengths, monkeypatch):
    from seekmer_amd import infer
    _, index, eff = chr21_index
    monkeypatch.setenv('SKM_SET_QUANT_GROUP', '2')
    sample_set = _sample_set(index, samples, per_sample_lengths=per_sample_lengths, length_model=MODEL)
    plain = _sample_set(index, samples, per_sample_lengths=per_sample_lengths)
    summaries = sample_set.summarize()
    assert len(summaries) == 3 and summaries[0].aligned > 0 and summaries[1].total == 0
    assert summaries[2].aligned == 0 and summaries[2].total == 12
    tpm, steps, lengths = sample_set.quantify(return_iters=True, return_effective_lengths=True)
    assert tpm.shape == lengths.shape == (3, eff.size)
    for i, summary in enumerate(summaries):
        assert summary.length_model == (200.0, 20.0)
        np.testing.assert_array_equal(summary.effective_lengths, eff, err_msg='summary %d' % i)
        np.testing.assert_array_equal(lengths[i], eff, err_msg='quantify %d' % i)
        want_tpm, want_steps = infer.quantify(summary, return_iters=True)
        assert steps[i] == want_steps, i
        np.testing.assert_array_equal(tpm[i], want_tpm, err_msg='tpm %d' % i)
    assert steps[0] > 0 and tpm[0].sum() > 0
    # the sample without a unit: finite lengths, nothing to quantify
    assert summaries[1].fragment_length_frequencies.sum() == 0 or not per_sample_lengths
    assert np.isfinite(lengths[1]).all() and steps[1] == 0 and not tpm[1].any()
    assert steps[2] == 0 and not tpm[2].any()
    # the histograms are those of a set without a model
    np.testing.assert_array_equal(sample_set.fragment_length_counts, plain.fragment_length_counts)
    for ours, theirs in zip(summaries, plain.summarize()):
        np.testing.assert_array_equal(ours.fragment_length_frequencies, theirs.fragment_length_frequencies)
        assert theirs.length_model is None
    if per_sample_lengths:
        np.testing.assert_array_equal(sample_set.sample_fragment_length_counts, plain.sample_fragment_length_counts)
        assert sample_set.sample_fragment_length_counts[1].sum() == 0
        assert np.isnan(plain.summarize()[1].effective_lengths).all()       # what the model is for
    # cleared through the native setter, quantify() is the plain set's again
    native_libs.check(native_libs.hip().skm_sample_set_set_length_weights(sample_set._handle, None))
    if not per_sample_lengths:
        back = sample_set.quantify(return_iters=True, return_effective_lengths=True)
        for got, want in zip(back, plain.quantify(return_iters=True, return_effective_lengths=True)):
            np.testing.assert_array_equal(got, want)


def test_summarize_launches_one_row(native_libs, chr21_index, samples, monkeypatch):
    """With a model SampleSet.summarize() makes ONE row for all samples and does not call skm_effective_lengths_many."""
    from seekmer_amd import mapper
    _, index, eff = chr21_index
    calls = []
    weights_rule, many = mapper._effective_lengths_weights, mapper._effective_lengths_many
    monkeypatch.setattr(mapper, '_effective_lengths_weights',
                        lambda lengths, weights, device: calls.append(np.asarray(weights).size // 2000) or weights_rule(lengths, weights, device))
    monkeypatch.setattr(mapper, '_effective_lengths_many', lambda *a: calls.append('many') or many(*a))
    sample_set = _sample_set(index, samples, per_sample_lengths=True, length_model=MODEL)
    summaries = sample_set.summarize()
    assert calls == [1]
    assert all(summary.effective_lengths is summaries[0].effective_lengths for summary in summaries)
    assert not summaries[0].effective_lengths.flags.writeable


# ---- the commands ------------------------------------------------------------------------------------------
def _columns(path):
    rows = [line.rstrip('\n').split('\t') for line in open(path)]
    assert rows[0] == ['target_id', 'length', 'eff_length', 'est_count', 'tpm']
    return rows[1:]


def test_infer_with_a_model(native_libs, chr21_index, single_reads, tmp_path):
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    index_path, index, eff = chr21_index
    out = tmp_path / 'out'
    assert cli.main(['infer', str(index_path), str(out), READS_1, '-s', *OPTIONS, '-b', '3', '--seed', '7']) == 0
    summary = _mapped(index, single_reads, length_model=MODEL).summarize()
    tpm = infer.quantify(summary)
    rows = _columns(out / 'abundance.tsv')
    assert len(rows) == eff.size
    assert [row[2] for row in rows] == ['%g' % float(value) for value in eff.astype('f4')]
    assert [row[4] for row in rows] == ['%g' % float(value) for value in tpm]
    info = json.loads((out / 'run_info.json').read_text())
    assert info['fragment_length_model'] == {'mean': 200.0, 'sd': 20.0} and info['n_bootstraps'] == 3
    assert info['n_processed'] == 21 and info['n_pseudoaligned'] == summary.aligned
    with np.load(out / 'abundance.npz') as arrays:
        np.testing.assert_array_equal(arrays['aux/eff_lengths'], eff)
        np.testing.assert_array_equal(arrays['aux/fld'], summary.fragment_length_frequencies.astype('i4'))   # the observed one
        for i, replicate in enumerate(infer.bootstrap_quantify(summary, tpm, 3, seed=7)):
            np.testing.assert_array_equal(arrays['bootstrap/bs%d' % i], replicate)
    # without the options nothing names a model
    plain = tmp_path / 'plain'
    assert cli.main(['infer', str(index_path), str(plain), READS_1, '-s']) == 0
    assert 'fragment_length_model' not in json.loads((plain / 'run_info.json').read_text())
    assert [row[2] for row in _columns(plain / 'abundance.tsv')] != [row[2] for row in rows]


def _set_regime(monkeypatch):
    """The calls of SampleSet.quantify, recorded; the rule's constants lowered so that a handful of samples take it."""
    from seekmer_amd import impute, mapper
    calls = []
    set_quantify = mapper.SampleSet.quantify
    monkeypatch.setattr(mapper.SampleSet, 'quantify', lambda self, *a, **k: calls.append('set') or set_quantify(self, *a, **k))
    monkeypatch.setattr(impute, 'SET_QUANT_MIN_SAMPLES', 2)
    monkeypatch.setattr(impute, 'SET_QUANT_LARGE_MIN_SAMPLES', 2)
    for bound in ('SET_QUANT_SMALL_TRANSCRIPTS', 'SET_QUANT_SMALL_CLASSES', 'SET_QUANT_MAX_TRANSCRIPTS', 'SET_QUANT_MAX_CLASSES'):
        monkeypatch.setattr(impute, bound, 1 << 40)
    return calls


SWITCHES = ('SKM_INFER_MANY_PER_SAMPLE', 'SKM_SET_QUANT_SERIAL', 'SKM_IMPUTE_SERIAL', 'SKM_IMPUTE_PER_CELL')


def test_infer_many_with_a_model(native_libs, chr21_index, tmp_path, monkeypatch):
    """Two single-ended samples (the fixture's two files): every abundance.tsv is that of `infer -s` on the sample
    alone with the same options -- through the set and its shared EM launches, with the set quantified sample by
    sample, and with a mapper per sample."""
    from seekmer_amd import __main__ as cli
    index_path, _, eff = chr21_index
    calls = _set_regime(monkeypatch)
    for switch in SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    alone = {}
    for name, path in (('20_1', READS_1), ('20_2', READS_2)):
        assert cli.main(['infer', str(index_path), str(tmp_path / 'alone' / name), path, '-s', *OPTIONS]) == 0
        alone[name] = (tmp_path / 'alone' / name / 'abundance.tsv').read_bytes()
        assert [row[2] for row in _columns(tmp_path / 'alone' / name / 'abundance.tsv')] == ['%g' % float(v) for v in eff.astype('f4')]
    assert alone['20_1'] != alone['20_2']
    for form, switch, expected_calls in (('set', None, ['set']), ('per_sample', 'SKM_INFER_MANY_PER_SAMPLE', []),
                                         ('serial', 'SKM_SET_QUANT_SERIAL', [])):
        if switch:
            monkeypatch.setenv(switch, '1')
        del calls[:]
        out = tmp_path / form
        assert cli.main(['infer-many', str(index_path), str(out), READS_1, READS_2, '-s', *OPTIONS]) == 0
        assert calls == expected_calls, form
        for name in alone:
            assert (out / name / 'abundance.tsv').read_bytes() == alone[name], (form, name)
            assert json.loads((out / name / 'run_info.json').read_text())['fragment_length_model'] == {'mean': 200.0, 'sd': 20.0}
        if switch:
            monkeypatch.delenv(switch)


def test_impute_with_a_model(native_libs, chr21_index, tmp_path, monkeypatch):
    """Nine cells cut from the fixture's 42 reads (18 reads each, three further on from cell to cell), four
    transcripts a gene: tpm.csv byte for byte through the set with both rounds in shared launches, one cell at a
    time (SKM_IMPUTE_SERIAL=1) and with a mapper per cell (SKM_IMPUTE_PER_CELL=1)."""
    from seekmer_amd import __main__ as cli
    from seekmer_amd import common
    _, index, _ = chr21_index
    transcripts = np.zeros(index.transcripts.size, dtype=[('transcript_id', index.transcripts.dtype['transcript_id']),
                                                          ('gene_id', 'S8'), ('length', 'f8')])
    transcripts['transcript_id'] = index.transcripts['transcript_id']
    transcripts['length'] = index.transcripts['length']
    transcripts['gene_id'] = [b'G%05d' % (t // 4) for t in range(transcripts.size)]
    index_path = tmp_path / 'genes.npz'
    common.KMerIndex(index.kmers, index.contigs, index.sequences, index.targets, transcripts, index.exons).save(index_path)
    records = []
    for path in (READS_1, READS_2):
        lines = open(path, 'rb').read().splitlines(keepends=True)
        records += [b''.join(lines[i:i + 4]) for i in range(0, len(lines), 4)]
    assert len(records) == 42
    paths = []
    for cell in range(9):
        paths.append(tmp_path / ('cell%d.fastq' % cell))
        paths[-1].write_bytes(b''.join(records[3 * cell:3 * cell + 18]))
    calls = _set_regime(monkeypatch)
    for switch in SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    tables = {}
    for form, switch, expected_calls in (('default', None, ['set']), ('serial', 'SKM_IMPUTE_SERIAL', []),
                                         ('per_cell', 'SKM_IMPUTE_PER_CELL', [])):
        if switch:
            monkeypatch.setenv(switch, '1')
        del calls[:]
        out = tmp_path / form
        assert cli.main(['impute', str(index_path), str(out), *map(str, paths), '-s', *OPTIONS, '--seed', '0']) == 0
        assert calls == expected_calls, form
        tables[form] = (out / 'tpm.csv').read_bytes()
        if switch:
            monkeypatch.delenv(switch)
    assert len(tables['default']) > 10000
    assert tables['serial'] == tables['default'] and tables['per_cell'] == tables['default']
