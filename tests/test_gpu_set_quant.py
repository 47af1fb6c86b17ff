"""Many class tables over the same transcripts in shared EM launches (skm_em_set.hip): the samples of a sample
set (mapper.SampleSet.quantify, skm_sample_set_quantify) and K tables of the caller's (infer.quantify_tables,
skm_quant_em_tables) against infer.quantify() on every table alone.  Every comparison is array_equal on the TPM
plus equality of the EM step counts: each table runs its own iteration, with its own total, to its own stopping
rule, and is frozen from then on while the others go on."""
import types

import numpy as np
import pytest

from conftest import make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu

GROUP = 'SKM_SET_QUANT_GROUP'
SERIAL = 'SKM_SET_QUANT_SERIAL'

# (units, shortest and longest fragment, shortest transcript drawn from); None = 500 units of random reads, none aligned
CELLS = (None, (1, 150, 400, 450), (37, 150, 400, 450), (3000, 150, 400, 450), (400, 450, 900, 950), (1200, 150, 400, 450),
         (150, 1900, 2500, 2601))
RANDOM_CELL, SINGLE_UNIT, LARGEST = 0, 1, 3


@pytest.fixture(autouse=True)
def _switches_off_by_default(monkeypatch):
    for name in (GROUP, SERIAL, 'SKM_IMPUTE_SERIAL', 'SKM_IMPUTE_PER_CELL', 'SKM_INFER_MANY_PER_SAMPLE', 'SKM_SAMPLE_SET_MAX_UNITS'):
        monkeypatch.delenv(name, raising=False)


def _cell_reads(seqs, rng, n_units, paired, shortest, longest, min_tx, read_len=75):
    """Units of chr21 fragments of shortest..longest bases; in cells of more than one unit one read in eight
    carries a substitution or an N."""
    long_tx = [s.upper() for s in seqs if len(s) >= min_tx]
    assert long_tx
    reads = []
    for _ in range(n_units):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(shortest, longest + 1))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        mates = [f[:read_len], reverse_complement(f[-read_len:])]
        if rng.integers(2):
            mates.reverse()
        for read in (mates if paired else mates[:1]):
            r = bytearray(read)
            kind = int(rng.integers(16)) if n_units > 1 else 15
            if kind == 0:
                r[int(rng.integers(len(r)))] = b'ACGT'[int(rng.integers(4))]
            elif kind == 1:
                r[int(rng.integers(len(r)))] = ord('N')
            reads.append(bytes(r))
    return reads


def _cells(seqs, paired):
    rng = np.random.default_rng(911 + paired)
    mates = 2 if paired else 1
    return [_cell_reads(seqs, rng, cell[0], paired, *cell[1:]) if cell is not None
            else [bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 75)) for _ in range(500 * mates)] for cell in CELLS]


def _add(oracle, sample_set, sample, reads, paired, first_unit=0):
    from seekmer_amd import common
    bases, offsets = oracle.pack_reads(reads) if reads else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    sample_set.add_batch(sample, first_unit, common.ReadBatch(len(reads) // (2 if paired else 1), bases, offsets, paired))


def _feed_shuffled(oracle, sample_set, cells, paired, which):
    """The cells `which` in shuffled order, the largest one as three segments with other cells in between."""
    step = 2 if paired else 1
    order = list(which)
    np.random.default_rng(17).shuffle(order)
    cuts = ((0, 1234), (1234, 1235), (1235, len(cells[LARGEST]) // step))
    pending = list(cuts) if LARGEST in which else []
    number = {cell: sample for sample, cell in enumerate(which)}
    for cell in order:
        if cell == LARGEST:
            continue
        if pending:
            lo, hi = pending.pop(0)
            _add(oracle, sample_set, number[LARGEST], cells[LARGEST][lo * step:hi * step], paired, first_unit=lo)
        _add(oracle, sample_set, number[cell], cells[cell], paired)
    for lo, hi in pending:
        _add(oracle, sample_set, number[LARGEST], cells[LARGEST][lo * step:hi * step], paired, first_unit=lo)


@pytest.fixture(scope='module')
def product_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


@pytest.fixture(scope='module')
def cells_by_layout(chr21):
    return {paired: _cells(chr21[1], paired) for paired in (True, False)}


def _loop(summaries):
    """Today's first round: quantify() summary by summary."""
    from seekmer_amd import infer
    results = [infer.quantify(summary, return_iters=True) for summary in summaries]
    return np.asarray([tpm for tpm, _ in results]), np.asarray([steps for _, steps in results], dtype=np.int64)


def _assert_set_equals_loop(sample_set, want_tpm, want_steps, summaries=None):
    tpm, steps, lengths = sample_set.quantify(return_iters=True, return_effective_lengths=True)
    assert tpm.shape == want_tpm.shape and tpm.dtype == np.float64
    np.testing.assert_array_equal(steps, want_steps)
    assert np.array_equal(tpm, want_tpm)
    for i, summary in enumerate(summaries or []):
        # (assert_array_equal: a sample without a fragment length has NaN lengths, in both)
        np.testing.assert_array_equal(lengths[i], summary.effective_lengths, err_msg='effective lengths of sample %d' % i)
    assert np.array_equal(sample_set.quantify(), want_tpm)


@pytest.mark.parametrize('paired, per_sample, strand', [(True, True, None), (True, False, None), (False, True, None),
                                                        (False, False, None), (True, True, 'fr')],
                         ids=['paired-own', 'paired-pooled', 'single-own', 'single-pooled', 'paired-own-fr'])
def test_set_equals_the_loop(oracle, product_index, cells_by_layout, paired, per_sample, strand):
    """Seven cells from no aligned unit and a single unit to 3000 units, fed in shuffled order with one cell in
    segments: TPM, steps and effective lengths of every sample are those of quantify() on its summary."""
    from seekmer_amd import mapper
    cells = cells_by_layout[paired]
    sample_set = mapper.SampleSet(product_index, paired, strand=strand, per_sample_lengths=per_sample)
    _feed_shuffled(oracle, sample_set, cells, paired, range(len(cells)))
    summaries = sample_set.summarize()
    assert [s.total for s in summaries] == [500] + [cell[0] for cell in CELLS[1:]]
    # (the single unit: aligned, unless the library's orientation filters its one pair out)
    assert summaries[RANDOM_CELL].aligned == 0 and summaries[SINGLE_UNIT].aligned == (1 if strand is None else summaries[SINGLE_UNIT].aligned) <= 1
    want_tpm, want_steps = _loop(summaries)
    print('steps of the loop: %s' % want_steps.tolist())
    assert want_steps[RANDOM_CELL] == 0 and not want_tpm[RANDOM_CELL].any()
    assert len(set(want_steps.tolist())) >= 3, 'the cells must stop at different steps, or nothing is frozen while others run'
    _assert_set_equals_loop(sample_set, want_tpm, want_steps, summaries)


@pytest.mark.parametrize('group', [1, 2, 4])
def test_groups(oracle, product_index, cells_by_layout, monkeypatch, group):
    """Six cells in groups of at most 1, 2 and 4: a group of one, a remainder group, buffers reused by the next."""
    from seekmer_amd import mapper
    cells = cells_by_layout[True]
    which = (3, 0, 1, 5, 2, 4)
    sample_set = mapper.SampleSet(product_index, True, per_sample_lengths=True)
    _feed_shuffled(oracle, sample_set, cells, True, which)
    summaries = sample_set.summarize()
    assert [s.total for s in summaries] == [500 if CELLS[cell] is None else CELLS[cell][0] for cell in which]
    want_tpm, want_steps = _loop(summaries)
    assert len(set(want_steps.tolist())) >= 3
    monkeypatch.setenv(GROUP, str(group))
    _assert_set_equals_loop(sample_set, want_tpm, want_steps, summaries)
    from seekmer_amd import infer
    tpm, steps = infer.quantify_tables(summaries, return_iters=True)
    np.testing.assert_array_equal(steps, want_steps)
    assert np.array_equal(tpm, want_tpm)


def _table(n_tx, tuples, counts, lengths):
    """A stand-in for mapper.SummarizedResult: what quantify() and quantify_tables() read of one."""
    sizes = [len(t) for t in tuples]
    if sum(sizes):
        class_map = np.vstack([np.repeat(np.arange(len(tuples)), sizes), np.concatenate([np.asarray(t) for t in tuples])]).astype(np.int64)
    else:
        class_map = np.asarray([]).T
    return types.SimpleNamespace(class_map=class_map, class_count=np.asarray(counts, dtype='f8'), effective_lengths=lengths)


def _hand_made_tables(n_tx, k, seed):
    """k tables: [0] one transcript in 1300 classes (three rows: the arrivals path) beside other classes, [1] one
    class, the middle one without a class, the others random -- with tuples of 1, 4 and 5 entries where n_tx
    allows -- on their own effective lengths."""
    rng = np.random.default_rng(seed)
    wide = min(n_tx, 5)
    tables = []
    for i in range(k):
        lengths = rng.uniform(150.0, 4000.0, n_tx)
        if i == k // 2 and k > 2:
            tables.append(_table(n_tx, [], [], lengths))
            continue
        if i == 0:
            hub = int(rng.integers(n_tx))
            tuples = [[hub] + rng.choice(n_tx, int(rng.integers(0, wide)), replace=False).tolist() for _ in range(1300)]
            tuples = [list(dict.fromkeys(t)) for t in tuples]
        elif i == 1:
            tuples = [rng.choice(n_tx, min(wide, 4), replace=False).tolist()]
        else:
            sizes = [1, min(wide, 4), wide] + rng.integers(1, wide + 1, int(rng.integers(1, 60))).tolist()
            tuples = [rng.choice(n_tx, size, replace=False).tolist() for size in sizes]
        counts = rng.integers(1, 10 ** int(rng.integers(1, 5)), len(tuples))
        tables.append(_table(n_tx, tuples, counts, lengths))
    return tables


@pytest.mark.parametrize('k, n_tx', [(1, 257), (9, 1), (9, 257), (9, 1704)])
def test_hand_made_tables(native_libs, k, n_tx):
    from seekmer_amd import infer
    tables = _hand_made_tables(n_tx, k, 40 + k + n_tx)
    if n_tx >= 5:
        assert {1, 4, 5} <= {int(n) for t in tables if t.class_map.size for n in np.bincount(t.class_map[0])}
    assert np.bincount(tables[0].class_map[1]).max() == 1300
    want_tpm, want_steps = _loop(tables)
    print('steps of the loop: %s' % want_steps.tolist())
    if k > 1:
        assert want_steps[k // 2] == 0 and not want_tpm[k // 2].any()
        if n_tx > 1:
            assert len(set(want_steps[want_steps > 0].tolist())) >= 2
    tpm, steps = infer.quantify_tables(tables, return_iters=True)
    np.testing.assert_array_equal(steps, want_steps)
    assert np.array_equal(tpm, want_tpm)
    assert np.array_equal(infer.quantify_tables(tables), want_tpm)


def test_classes_without_a_tuple_entry(native_libs, monkeypatch):
    """A class that class_map never names (an empty tuple) counts in its table's total and in nothing else.  In
    tables that are not the last -- the one of 1300 classes, the one of a single class, which stops first, and a
    random one, at the front, in the middle and at the end of their class lists -- it must not move any later
    table's class range: every table as quantify() gives it alone."""
    from seekmer_amd import infer
    plain = _hand_made_tables(257, 5, 11)
    tables = list(plain)
    for at, places in ((0, (0, 700)), (1, (1,)), (3, (0, 2, None))):
        sizes = np.bincount(plain[at].class_map[0])
        tuples = np.split(plain[at].class_map[1], np.cumsum(sizes)[:-1])
        counts = plain[at].class_count.tolist()
        for place in places:
            place = len(tuples) if place is None else place
            tuples.insert(place, [])
            counts.insert(place, 7.0)
        tables[at] = _table(257, tuples, counts, plain[at].effective_lengths)
        assert tables[at].class_count.size == plain[at].class_count.size + len(places) == np.unique(tables[at].class_map[0]).size + len(places)
    want_tpm, want_steps = _loop(tables)
    print('steps of the loop: %s' % want_steps.tolist())
    assert len(set(want_steps[want_steps > 0].tolist())) >= 3          # (tables frozen while later ones run)
    for group in (None, '2'):
        if group:
            monkeypatch.setenv(GROUP, group)
        tpm, steps = infer.quantify_tables(tables, return_iters=True)
        np.testing.assert_array_equal(steps, want_steps)
        assert np.array_equal(tpm, want_tpm)


def test_too_few_rows_for_the_samples_of_a_set(oracle, product_index, cells_by_layout, native_libs):
    """cap_samples below the samples of the set: SKM_ERR_ARG with the count reported and nothing written, which is
    what SampleSet.quantify() retries on when a sample was added meanwhile; with room, the same call succeeds."""
    import ctypes
    from seekmer_amd import infer, mapper
    cells = cells_by_layout[True]
    sample_set = mapper.SampleSet(product_index, True)
    for sample, cell in enumerate((2, 4, 1)):
        _add(oracle, sample_set, sample, cells[cell], True)
    assert len(sample_set) == 3
    lengths = np.ascontiguousarray(product_index.transcripts['length'], dtype='f8')
    tpm = np.full((3, lengths.size), -1.0)
    steps = np.full(3, -1, dtype=np.int64)

    def call(cap):
        n = ctypes.c_int64(-5)
        code = native_libs.hip().skm_sample_set_quantify(
            sample_set._handle, native_libs.ptr(lengths, native_libs.c_f64p), lengths.size, infer.REL_TOL, infer.X_FLOOR, 0, cap,
            ctypes.byref(n), native_libs.ptr(tpm, native_libs.c_f64p), None, native_libs.ptr(steps, native_libs.c_i64p))
        return code, n.value

    for cap in (2, 0):
        assert call(cap) == (native_libs.SKM_ERR_ARG, 3)
        assert (tpm == -1.0).all() and (steps == -1).all()
    assert call(3) == (native_libs.SKM_OK, 3)
    want_tpm, want_steps = _loop(sample_set.summarize())
    np.testing.assert_array_equal(steps, want_steps)
    assert np.array_equal(tpm, want_tpm)


def test_an_undefined_table_among_good_ones(native_libs):
    """All-zero counts leave no abundance above the floor: the call fails as quantify() does at that table, names
    it, and the next call in the process is right."""
    from seekmer_amd import infer
    tables = _hand_made_tables(257, 5, 3)
    want_tpm, want_steps = _loop(tables)
    bad = list(tables)
    for at in (3, 1):
        bad[at] = types.SimpleNamespace(class_map=tables[at].class_map, class_count=np.zeros_like(tables[at].class_count),
                                        effective_lengths=tables[at].effective_lengths)
    with pytest.raises(native_libs.NativeError) as alone:
        infer.quantify(bad[1])
    assert alone.value.code == native_libs.SKM_ERR_UNDEFINED
    with pytest.raises(native_libs.NativeError) as error:
        infer.quantify_tables(bad)
    assert error.value.code == native_libs.SKM_ERR_UNDEFINED and 'table 1:' in str(error.value)
    tpm, steps = infer.quantify_tables(tables, return_iters=True)
    np.testing.assert_array_equal(steps, want_steps)
    assert np.array_equal(tpm, want_tpm)


# ---- the product: impute and infer-many with the first round in shared launches and with the loop
@pytest.fixture(scope='module')
def synthetic(native_libs, tmp_path_factory):
    from seekmer_amd import common, index_builder, synth
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    # (impute weighs the cells by gene: four transcripts a gene)
    transcripts = np.zeros(len(ids), dtype=[('transcript_id', index.transcripts.dtype['transcript_id']),
                                            ('gene_id', 'S8'), ('length', 'f8')])
    transcripts['transcript_id'] = index.transcripts['transcript_id']
    transcripts['length'] = index.transcripts['length']
    transcripts['gene_id'] = [b'GENE%04d' % (t // 4) for t in range(len(ids))]
    index = common.KMerIndex(index.kmers, index.contigs, index.sequences, index.targets, transcripts, index.exons)
    index_path = tmp_path_factory.mktemp('set_quant_index') / 'index.npz'
    index.save(index_path)
    return index_path, pool, tx_offsets


def _write_samples(folder, pool, tx_offsets, units):
    from seekmer_amd import synth
    paths = []
    for sample, n_units in enumerate(units):
        bases, _ = synth.reads(100 + sample % 2, pool, tx_offsets, sample * 8000, n_units, 75, True)
        names = [folder / ('s%d_%d.fastq' % (sample, mate + 1)) for mate in range(2)]
        synth.write_fastq(bases, n_units, 75, True, *names)
        paths += names
    return paths


def _routes(monkeypatch):
    """Calls of the shared-launch forms, recorded; the rule's constants lowered so that small runs take them."""
    from seekmer_amd import impute, infer, mapper
    calls = []
    set_quantify, tables = mapper.SampleSet.quantify, infer.quantify_tables
    monkeypatch.setattr(mapper.SampleSet, 'quantify', lambda self, *a, **k: calls.append('set') or set_quantify(self, *a, **k))
    monkeypatch.setattr(infer, 'quantify_tables', lambda *a, **k: calls.append('tables') or tables(*a, **k))
    monkeypatch.setattr(impute, 'SET_QUANT_MIN_SAMPLES', 2)
    monkeypatch.setattr(impute, 'SET_QUANT_LARGE_MIN_SAMPLES', 2)
    for bound in ('SET_QUANT_SMALL_TRANSCRIPTS', 'SET_QUANT_SMALL_CLASSES', 'SET_QUANT_MAX_TRANSCRIPTS', 'SET_QUANT_MAX_CLASSES'):
        monkeypatch.setattr(impute, bound, 1 << 40)
    return calls


def test_impute_writes_the_same_files_either_way(synthetic, tmp_path, monkeypatch):
    """12 small cells: tpm.csv, initial_gene_table.csv and weight.csv byte for byte with the first round in shared
    launches (from the set, and from the summaries of a mapper per cell), with SKM_SET_QUANT_SERIAL=1, and with
    SKM_IMPUTE_SERIAL=1, which keeps both rounds one cell at a time."""
    from seekmer_amd.__main__ import main
    index_path, pool, tx_offsets = synthetic
    paths = _write_samples(tmp_path, pool, tx_offsets, tuple(1000 + 250 * ((5 * cell) % 12) for cell in range(12)))
    calls = _routes(monkeypatch)
    outputs = {}
    for name, serial, per_cell, all_serial in (('set', None, None, None), ('tables', None, '1', None), ('loop', '1', None, None),
                                              ('both_serial', None, None, '1')):
        for switch, value in ((SERIAL, serial), ('SKM_IMPUTE_PER_CELL', per_cell), ('SKM_IMPUTE_SERIAL', all_serial)):
            monkeypatch.setenv(switch, value) if value else monkeypatch.delenv(switch, raising=False)
        del calls[:]
        assert main(['impute', str(index_path), str(tmp_path / name), *map(str, paths), '-p', '4', '--seed', '0']) == 0
        assert calls == {'set': ['set'], 'tables': ['tables'], 'loop': [], 'both_serial': []}[name]
        outputs[name] = {f: (tmp_path / name / f).read_bytes() for f in ('tpm.csv', 'initial_gene_table.csv', 'weight.csv')}
        assert all(len(data) > 100 for data in outputs[name].values())
    assert outputs['set'] == outputs['loop'] and outputs['tables'] == outputs['loop'] and outputs['both_serial'] == outputs['loop']


def test_infer_many_writes_the_same_files_either_way(synthetic, tmp_path, monkeypatch):
    from seekmer_amd.__main__ import main
    index_path, pool, tx_offsets = synthetic
    units = (2000, 3500, 4000, 2500, 3000)
    paths = _write_samples(tmp_path, pool, tx_offsets, units)
    calls = _routes(monkeypatch)
    for name, serial in (('set', None), ('loop', '1')):
        monkeypatch.setenv(SERIAL, serial) if serial else monkeypatch.delenv(SERIAL, raising=False)
        del calls[:]
        assert main(['infer-many', str(index_path), str(tmp_path / name), *map(str, paths), '-b', '1', '--seed', '7']) == 0
        assert calls == (['set'] if name == 'set' else [])
    for sample in range(len(units)):
        one = (tmp_path / 'set' / ('s%d_1' % sample) / 'abundance.tsv').read_bytes()
        assert len(one) > 1000 and one == (tmp_path / 'loop' / ('s%d_1' % sample) / 'abundance.tsv').read_bytes()
    assert (tmp_path / 'set' / 'samples.tsv').read_bytes() == (tmp_path / 'loop' / 'samples.tsv').read_bytes()
