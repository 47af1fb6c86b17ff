"""The class table's growth, deferral and collision paths (csrc/skm_classes.hip; map_batch_resident,
table_grow, skm_mapper_merge, skm_mapper_merge_device in csrc/skm_abi.hip), each against a plain
reference: the oracle's Counter, the table of a mapper that never had to grow, a Python dict.

Every comparison is exact.  SKM_TEST_CLASS_SLOTS (README.md) starts a mapper's table at a few slots,
so a batch of a few thousand units defers units past the bounded probe, grows the table four-fold with
units in flight and retries, several times over; MapResult.timing()['deferred_grows']
(skm_mapper_timing, stats[7]) says that it did.  clear() and reset() keep a grown table, so every
hooked case makes its mapper fresh."""
import numpy as np
import pytest

import class_table_reference as ref
from conftest import make_product_index
from strand_reference import filter_result
from test_gpu_parity import _adversarial_reads, _compare_tables, _streams_of
from test_gpu_sample_set import _assert_same

pytestmark = pytest.mark.gpu

CUTS = (0, 2500, 2501)                  # (and the end of the batch)


@pytest.fixture(scope='module')
def product_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


class _Batch:
    pass


def _make_batch(oracle, chr21, chr21_oracle_index, product_index, paired):
    import os
    from seekmer_amd import common, mapper
    assert 'SKM_TEST_CLASS_SLOTS' not in os.environ
    b = _Batch()
    rng = np.random.default_rng(41)
    b.reads = _adversarial_reads(chr21[1], rng, 2 * 6000, 100)
    b.paired = paired
    b.n_units = 6000 if paired else 12000
    b.cuts = CUTS + (b.n_units,)
    b.bases, b.offsets = oracle.pack_reads(b.reads)
    b.fld = np.zeros(2000, dtype=np.int64)
    b.expected = oracle.map_batch(chr21_oracle_index, b.bases, b.offsets, b.n_units, paired, b.fld)
    classes = oracle.Classes()
    classes.update(b.expected)
    b.n_classes = int(classes.export()[2].size)
    b.plain = {}
    for strand in (None, 'rf'):
        result = mapper.MapResult(product_index, strand=strand)
        mapper.ReadMapper(product_index, result).map_batch(common.ReadBatch(b.n_units, b.bases, b.offsets, paired))
        assert result.timing()['deferred_grows'] == 0
        b.plain[strand] = result
    _compare_tables(oracle, b.expected, b.fld, b.plain[None])
    return b


@pytest.fixture(scope='module')
def batch(oracle, native_libs, chr21, chr21_oracle_index, product_index):
    """The 12 000 adversarial reads of test_tables_merge_on_the_device as 12 000 single-ended units
    (2989 classes), the oracle's result, and the table of a mapper made WITHOUT the hook (nothing has
    set it when this fixture runs)."""
    b = _make_batch(oracle, chr21, chr21_oracle_index, product_index, False)
    assert b.n_classes >= 2048
    return b


@pytest.fixture(scope='module')
def pairs(oracle, native_libs, chr21, chr21_oracle_index, product_index):
    """The same reads as the 6000 pairs of that test.  Their mates come from transcripts drawn
    independently, so all but a handful of pairs are unaligned: the batch has 5 classes."""
    b = _make_batch(oracle, chr21, chr21_oracle_index, product_index, True)
    assert b.n_classes == 5
    return b


def _largest_slots(n_classes):
    """The largest power of two N with 16 N <= n_classes: even then two four-fold growths leave fewer
    slots than the batch has classes."""
    n = 2
    while 32 * n <= n_classes:
        n *= 2
    assert 16 * n <= n_classes
    return n


def _slots(which, n_classes):
    return 4 if which == 'four' else _largest_slots(n_classes)


def _map(index, result, b, how):
    from seekmer_amd import _native, common, mapper
    rm = mapper.ReadMapper(index, result)
    if how == 'one':
        rm.map_batch(common.ReadBatch(b.n_units, b.bases, b.offsets, b.paired))
    elif how == 'three':
        mates = 2 if b.paired else 1
        for lo, hi in zip(b.cuts[:-1], b.cuts[1:]):
            sub = np.ascontiguousarray(b.offsets[mates * lo:mates * hi + 1])
            rm.map_batch_async(common.ReadBatch(hi - lo, b.bases, sub, b.paired, first_unit=lo))
        result.sync()
    else:
        assert how == 'packed'
        _native.check(_native.hip().skm_mapper_expect_units(result._handle, b.n_units))
        for piece in _streams_of(common, b.bases, b.offsets, b.n_units, b.paired):
            rm.push_packed(piece)
        result.sync()


def _same_table(result, plain):
    for got, want in zip(result.export(), plain.export()):     # offsets, ids, counts, first-seen values, histogram
        np.testing.assert_array_equal(got, want)
    assert result.sizes() == plain.sizes()


def _deferred(oracle, index, b, how, n_slots, least_grows, monkeypatch):
    from seekmer_amd import mapper
    monkeypatch.setenv('SKM_TEST_CLASS_SLOTS', str(n_slots))
    result = mapper.MapResult(index)
    _map(index, result, b, how)
    grows = result.timing()['deferred_grows']
    print('%s, %d slots, %d classes: %d growths with units in flight' % (how, n_slots, b.n_classes, grows))
    assert grows >= least_grows
    _compare_tables(oracle, b.expected, b.fld, result)
    _same_table(result, b.plain[None])
    assert b.plain[None].timing()['deferred_grows'] == 0


@pytest.mark.parametrize('slots', ['four', 'largest'])
@pytest.mark.parametrize('how', ['one', 'three', 'packed'])
def test_units_deferred_under_a_growing_table(oracle, product_index, batch, how, slots, monkeypatch):
    """A table of N slots under 12 000 units with 2989 classes: units past the bounded probe are
    deferred, the populated table grows with the batch's unit -> slot map in flight, the deferred
    units are retried -- at least twice, for 16 N <= classes -- and the table is the oracle's and,
    first-seen values included, that of a mapper that never grew.  As one batch, as three batches
    placed with first_unit (cut at 0 / 2500 / 2501 / the end), and packed after expect_units.

    The units are single-ended because the 6000 PAIRS these reads make have 5 classes (their mates
    are drawn independently), which one growth of a 4-slot table holds: see the test below."""
    n_slots = _slots(slots, batch.n_classes)
    assert batch.n_classes >= 16 * n_slots
    _deferred(oracle, product_index, batch, how, n_slots, 2, monkeypatch)


@pytest.mark.parametrize('how', ['one', 'three', 'packed'])
def test_pairs_on_a_table_of_four_slots(oracle, product_index, pairs, how, monkeypatch):
    """The paired form of the batch: 6000 pairs, 5 classes, 4 slots.  As one batch the fifth class
    finds no slot, so its units are deferred and the table grows once under the batch; 16 slots then
    hold all five, and no second growth can happen (with 5 classes there is no N >= 2 with
    16 N <= classes).  Cut into several batches the table may grow between them instead, to keep its
    load below 0.5, with nothing in flight: there only the tables are checked."""
    _deferred(oracle, product_index, pairs, how, 4, 1 if how == 'one' else 0, monkeypatch)


def test_stranded_units_deferred_under_a_growing_table(oracle, product_index, batch, monkeypatch):
    """The same with strand='rf': the strand filter rewrites the records' keys before they are counted."""
    from seekmer_amd import mapper
    filtered = filter_result(batch.expected, 'rf')
    _compare_tables(oracle, filtered, batch.fld, batch.plain['rf'])
    assert batch.plain['rf'].sizes()[0] >= 64           # two four-fold growths of 4 slots do not hold them
    monkeypatch.setenv('SKM_TEST_CLASS_SLOTS', '4')
    result = mapper.MapResult(product_index, strand='rf')
    _map(product_index, result, batch, 'one')
    assert result.timing()['deferred_grows'] >= 2
    _compare_tables(oracle, filtered, batch.fld, result)
    _same_table(result, batch.plain['rf'])


class _Feeder(list):
    paired = False


def test_a_sample_set_on_a_growing_table(oracle, product_index, batch, monkeypatch):
    """map_sample_set with three samples cut from the same reads: classes are (sample, tuple) in one
    table, which starts at 4 slots.  Every sample's table against a MapResult of its own and against
    the set that never grew (the comparison of test_gpu_sample_set.py)."""
    from seekmer_amd import common, mapper

    def feeders():
        out = []
        for lo, hi in zip(batch.cuts[:-1], batch.cuts[1:]):
            bases, offsets = oracle.pack_reads(batch.reads[lo:hi])
            out.append(_Feeder([common.ReadBatch(hi - lo, bases, offsets, False)]))
        return out

    expected = []
    for feeder in feeders():
        result = mapper.MapResult(product_index)
        mapper.ReadMapper(product_index, result).map_batch(feeder[0])
        expected.append((result.sizes(), result.export()))
    plain = mapper.map_sample_set(product_index, feeders())
    _assert_same(plain, expected)
    monkeypatch.setenv('SKM_TEST_CLASS_SLOTS', '4')
    hooked = mapper.map_sample_set(product_index, feeders())
    _assert_same(hooked, expected)
    np.testing.assert_array_equal(hooked.sizes(), plain.sizes())
    for got, want in zip(hooked.export(), plain.export()):
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_the_em_reads_the_remapped_registry(product_index, batch, monkeypatch):
    """skm_quant_create_from_mapper walks the class registry, which every growth redirects: the EM on
    the grown table gives the vector and the step count of the EM on the table that never grew, bit for bit."""
    from seekmer_amd import infer, mapper
    monkeypatch.setenv('SKM_TEST_CLASS_SLOTS', '4')
    result = mapper.MapResult(product_index)
    _map(product_index, result, batch, 'one')
    assert result.timing()['deferred_grows'] >= 2
    eff = batch.plain[None].summarize().effective_lengths
    x0 = np.ones(eff.size) / eff
    x0 /= x0.sum()
    runs = []
    for held in (batch.plain[None], result):
        quant = infer._QuantHandle.from_map_result(held, eff.size)
        runs.append(quant.em(x0, eff))
        quant.close()
    assert runs[0][1] == runs[1][1] and runs[0][1] > 1
    np.testing.assert_array_equal(runs[1][0], runs[0][0])


# ---- merges of synthetic tuples against a dict -----------------------------------------------------

@pytest.fixture(scope='module')
def merge_sets():
    return ref.merge_classes()


def _check(result, reference):
    assert result.sizes() == reference.sizes()
    for got, want in zip(result.export(), reference.export()):
        np.testing.assert_array_equal(got, want)
    assert result.timing()['deferred_grows'] == 0          # merges probe without a bound: nothing is deferred


def _holding(index, *class_sets):
    from seekmer_amd import mapper
    result = mapper.MapResult(index)
    for class_set in class_sets:
        class_set.merge_into(result)
    return result


def test_merges_against_a_dict(native_libs, product_index, merge_sets):
    """skm_mapper_merge on a mapper without the hook: 40 000 classes into an empty table (2^16 ->
    2^17 slots), 100 000 on top -- every tuple of A again, with other counts and first-seen values
    below and above A's, and 60 000 new ones: the populated table grows 2^17 -> 2^19, rehash and
    registry remap -- then a single class, then no class at all with only unaligned units and a
    histogram.  (A set of 100 000 DISTINCT tuples cannot hold 50 000 of A's 40 000: it holds all of
    them.)  sizes() and export() against the dict after every step."""
    from seekmer_amd import mapper
    result = mapper.MapResult(product_index)
    reference = ref.CounterReference()
    for class_set in merge_sets:
        class_set.merge_into(result)
        reference.merge(class_set)
        _check(result, reference)
    assert reference.sizes()[0] == 100001


def test_resident_merges_in_both_directions(native_libs, product_index, merge_sets):
    """A and B held by two mappers and joined with merge_resident (class_merge_kernel<double> over the
    other mapper's arrays in HBM), B into A and A into B: the dict's totals either way."""
    a, b, _, _ = merge_sets
    reference = ref.CounterReference().merge(a).merge(b)
    into_a, held_b = _holding(product_index, a), _holding(product_index, b)
    into_a.merge_resident(held_b)
    _check(into_a, reference)
    _check(held_b, ref.CounterReference().merge(b))        # (the giver is unchanged)
    held_b.merge_resident(_holding(product_index, a))
    _check(held_b, reference)


@pytest.mark.parametrize('n_classes', [1, 63, 64, 65, 257])
def test_merges_of_partial_waves_and_blocks(native_libs, product_index, merge_sets, n_classes):
    """The wave-aggregated allocation of registry entries and arena space with a single lane, a wave
    short of one lane, a full wave, a wave and a lane, a block and a lane -- from host arrays and
    from another mapper's table."""
    part = merge_sets[0].head(n_classes)
    reference = ref.CounterReference().merge(part)
    held = _holding(product_index, part)
    _check(held, reference)
    resident = _holding(product_index)
    resident.merge_resident(held)
    _check(resident, reference)
    resident.merge_resident(held)                           # every class found, none made
    _check(resident, ref.CounterReference().merge(part).merge(part))


def test_one_long_probe_chain(native_libs, product_index, merge_sets):
    """300 single-id tuples whose keys share their low 16 bits: one home slot in the 2^16-slot table
    of a fresh mapper, a probe chain of 300 -- past CLASS_PROBE_LIMIT, which binds batches, not
    merges.  All 300 come back with their counts; 40 000 classes merged on top grow the table, the
    chain is rehashed, and the 300 are still exact."""
    chain = ref.probe_chain()
    reference = ref.CounterReference().merge(chain)
    result = _holding(product_index, chain)
    _check(result, reference)
    merge_sets[0].merge_into(result)
    _check(result, reference.merge(merge_sets[0]))
    assert reference.sizes()[0] == 40300
    by_tuple = dict(zip(chain.tuples, chain.counts.tolist()))
    offsets, targets, counts, _, _ = result.export()
    singles = np.flatnonzero(np.diff(offsets) == 1)
    got = {(int(targets[offsets[k]]),): int(counts[k]) for k in singles}
    assert all(got[t] == n for t, n in by_tuple.items())


# ---- a constructed 64-bit key collision -----------------------------------------------------------------

def _colliding_sets(merge_sets):
    """[(A, B, A and B in one set)]: single-class sets of two different tuples with one key, with
    unaligned units and a histogram of their own, so that a merge that went through shows in the totals."""
    rng = np.random.default_rng(5)
    out = []
    first = 1 << 21
    for one, two in ref.collision_pairs(3):
        assert one != two and ref.tuple_key(one) == ref.tuple_key(two)
        one, two = (tuple(ref.as_int32(i) for i in t) for t in (one, two))
        assert min(one + two) < 0             # an id with its top bit set, passed as the negative int32
        sets = [ref.ClassSet([t], [int(rng.integers(1, 1000))], [first + k], int(rng.integers(1, 1000)),
                             ref._random_fld(rng)) for k, t in enumerate((one, two))]
        both = ref.ClassSet([one, two], [3, 5], [first + 2, first + 3], 7, ref._random_fld(rng))
        out.append(sets + [both])
        first += 4
    return out


def _refused(call):
    from seekmer_amd import _native
    with pytest.raises(_native.NativeError) as caught:
        call()
    assert caught.value.code == _native.SKM_ERR_COLLISION


@pytest.mark.parametrize('how', ['two calls', 'one call', 'resident'])
def test_a_key_collision_fails_the_merge(native_libs, product_index, merge_sets, how):
    """Two different tuples with the same 64-bit key (class_table_reference.collision_pairs) must
    never share a class: the merge that brings the second one -- in a later skm_mapper_merge call, in
    the same call, or from another mapper's table through skm_mapper_merge_device -- fails with
    SKM_ERR_COLLISION and leaves the unit totals and the histogram as they were; after reset() the
    handle is as good as new.

    Out of scope: class_insert / class_verify cannot be driven into their collision exit by this
    construction.  One id of every such pair is >= 2^31 and no transcript id is, so no mapped read can
    carry one of the tuples."""
    bystanders = merge_sets[0].head(257)
    for first, second, both in _colliding_sets(merge_sets):
        held = _holding(product_index, bystanders) if how == 'one call' else _holding(product_index, bystanders, first)
        sizes, fld = held.sizes(), held.fragment_length_counts
        if how == 'two calls':
            _refused(lambda: second.merge_into(held))
        elif how == 'one call':
            _refused(lambda: both.merge_into(held))
        else:
            other = _holding(product_index, second)
            _refused(lambda: held.merge_resident(other))
        assert held.sizes()[2:] == sizes[2:]
        np.testing.assert_array_equal(held.fragment_length_counts, fld)
        held.reset()
        first.merge_into(held)
        _check(held, ref.CounterReference().merge(first))
