"""The map kernel's long target lists, the refill of its unit contexts and the relaunch after an entry-arena
overflow, against the CPU oracle on the constructed transcriptome of tests/target_list_reference.py (what that
input reaches is asserted, on the oracle alone, by tests/test_target_lists.py).

Every comparison is exact: per unit the count, the signed entries, begin, end and the anchor; per table the
classes in first-seen order, the histogram and the unaligned count.  What is pinned here and nowhere else:
  * lists of 17 to 300 entries with chosen positions left -- bits 7/8, 15/16, 63/64, 127/128, 191/192 of the
    keep-mask, its extension words in the HBM workspace and their staging copy (TSet, filter_on_contig,
    intersect, the emission loop), read forwards and mirrored, a five-word list against a four-word one;
  * a unit context that has held a long list and is given the next unit (SKM_TEST_MAP_BLOCKS: one or two blocks
    map the whole batch, every context is refilled several times, the block drains its tail);
  * a batch whose ids outgrow the entry arena, alone and inside a sample set (skm_mapper_map_relaunches);
  * the strand filter on runs of 129 to 300 ids."""
import numpy as np
import pytest

import target_list_reference as lists
from conftest import make_product_index
from strand_reference import filter_result, mixed_units
from test_gpu_parity import _adversarial_reads, _compare_tables, _compare_units
from test_gpu_strand import _same_table

pytestmark = pytest.mark.gpu

CONTEXTS = 480                       # unit contexts of a block of the map kernel (skm_kernels.h: MAP_CONTEXTS)


class World:
    """The fixture, its index (built by the product's builder) with the oracle on the same arrays, and per layout
    the batch and what the oracle makes of it -- computed once, read by every test, changed by none."""

    def __init__(self, oracle):
        from seekmer_amd import index_builder
        self.fixture = lists.fixture()
        ids, pool, tx_offsets = self.fixture.pooled()
        self.built = index_builder.build_pooled(ids, pool, tx_offsets)
        self.oindex = oracle.OracleIndex(self.built.kmers, self.built.contigs, self.built.sequences,
                                         self.built.targets, lengths=np.diff(tx_offsets))
        met = lists.check_list_positions(self.fixture, self.built.contigs, self.built.targets)
        assert set(lists.SIZES) <= met and max(met) == 300
        self.batches = {}
        for paired, units in ((False, self.fixture.singles), (True, self.fixture.pairs)):
            bases, offsets = oracle.pack_reads(lists.reads_of(units))
            self.batches[paired] = self.expect(oracle, bases, offsets, len(units), paired)

    def expect(self, oracle, bases, offsets, n_units, paired):
        fld = np.zeros(2000, dtype=np.int64)
        stats = oracle.Stats()
        expected = oracle.map_batch(self.oindex, bases, offsets, n_units, paired, fld, stats=stats)
        for array in (bases, offsets, fld, expected.count, expected.entries, expected.begin, expected.end):
            array.setflags(write=False)
        return bases, offsets, n_units, expected, fld, stats

    def index(self):
        """A product index of its own on the shared arrays: its device copy is made under the environment of the
        test that asks (the successor hooks are read at upload)."""
        from seekmer_amd import common
        b = self.built
        return common.KMerIndex(b.kmers, b.contigs, b.sequences, b.targets, b.transcripts, b.exons)


@pytest.fixture(scope='module')
def world(oracle, native_libs):
    return World(oracle)


@pytest.fixture(scope='module')
def plain_index(world):
    return world.index()


def _map(index, bases, offsets, n_units, paired, stats=False, strand=None):
    from seekmer_amd import common, mapper
    result = mapper.MapResult(index, keep_spans=True, strand=strand)
    if stats:
        result.set_stats(True)
    rm = mapper.ReadMapper(index, result)
    rm.map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    return result, rm


def _check(oracle, world, index, paired, stats=False):
    bases, offsets, n_units, expected, fld, ostats = world.batches[paired]
    result, rm = _map(index, bases, offsets, n_units, paired, stats=stats)
    _compare_units(expected, rm.last_batch(n_units))
    _compare_tables(oracle, expected, fld, result)
    return result, ostats


@pytest.mark.parametrize('paired', [True, False])
def test_long_lists_equal_the_oracles(oracle, world, plain_index, paired):
    """Case 1: the production kernel.  The oracle's own result says what the batch reaches: final lists of every
    size of SIZES (single-ended), lists in the fourth extension word, and lists of every form side by side."""
    expected = world.batches[paired][3]
    if paired:
        assert int(expected.count.max()) == 292 and ((expected.count > 16) & (expected.count <= 64)).any()
    else:
        assert set(lists.SIZES) <= set(int(c) for c in expected.count)
    assert (expected.count > 256).any() and (expected.count <= 8).any() and (expected.count == 0).any()
    assert plain_index.device_info()['max_target_count'] == 300
    # (lists this long outgrow an arena sized for 8 ids a unit: this batch is mapped twice as well, see
    # test_arena_relaunch for the path itself)
    _check(oracle, world, plain_index, paired)


@pytest.mark.parametrize('paired', [True, False])
def test_the_counting_build_on_long_lists(oracle, world, plain_index, paired):
    """Case 2: map_units_kernel<true, false> takes the two-pointer walks for the short lists too; its results are
    the oracle's and every access counter equals oracle.Stats."""
    result, ostats = _check(oracle, world, plain_index, paired, stats=True)
    counted = result.access_stats()
    for name, value in ostats.as_dict().items():
        assert counted[name] == value, (name, counted[name], value)


@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('hook', ['SKM_TEST_SUCC_LOOKUP', 'SKM_NO_SUCCESSORS'])
def test_long_lists_when_hops_look_their_junction_up(oracle, world, paired, hook, monkeypatch):
    """Case 3: every successor marked "look it up" at upload, and no successors at all: no merge is settled by a
    contig record's mask, every one runs filter_on_contig."""
    monkeypatch.setenv(hook, '1')
    index = world.index()
    assert index.device_info()['successors'] == (1 if hook == 'SKM_TEST_SUCC_LOOKUP' else 0)
    _check(oracle, world, index, paired)


@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('blocks', [1, 2])
def test_refilled_contexts(oracle, world, plain_index, paired, blocks, monkeypatch):
    """Case 4: one block, then two, map the whole batch.  Every context (pair slot) takes several units one after
    the other -- long-list and short-list units alternate in the batch -- so whatever a finished unit leaves behind
    (the high mask word, the read's edges, the extension words, the pair slot's count) meets the next one; the last
    units leave fewer units than contexts, short queues and a draining block."""
    monkeypatch.setenv('SKM_TEST_MAP_BLOCKS', str(blocks))
    n_units = world.batches[paired][2]
    per_block = -(-n_units // blocks)
    assert per_block > (CONTEXTS // 2 if paired else CONTEXTS)
    _check(oracle, world, plain_index, paired)


@pytest.mark.parametrize('paired', [True, False])
def test_chr21_in_one_block(oracle, chr21, chr21_oracle_index, paired, monkeypatch):
    """The reads of test_chr21_adversarial through one block: 3000 pairs over 240 pair slots, 6000 reads over 480
    contexts."""
    monkeypatch.setenv('SKM_TEST_MAP_BLOCKS', '1')
    rng = np.random.default_rng(7)
    reads = _adversarial_reads(chr21[1], rng, 6000, 100)
    index = make_product_index(chr21_oracle_index, chr21[0])
    bases, offsets = oracle.pack_reads(reads)
    n_units = len(reads) // 2 if paired else len(reads)
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(chr21_oracle_index, bases, offsets, n_units, paired, fld)
    result, rm = _map(index, bases, offsets, n_units, paired)
    _compare_units(expected, rm.last_batch(n_units))
    _compare_tables(oracle, expected, fld, result)


@pytest.mark.parametrize('value', ['0', '-3', 'many'])
def test_the_block_cap_refuses_less_than_one(plain_index, value, monkeypatch):
    from seekmer_amd import mapper
    monkeypatch.setenv('SKM_TEST_MAP_BLOCKS', value)
    with pytest.raises(ValueError, match='SKM_TEST_MAP_BLOCKS'):         # (SKM_ERR_ARG)
        mapper.MapResult(plain_index)


@pytest.mark.parametrize('blocks', [None, 1])
@pytest.mark.parametrize('size', [128, 300])
def test_arena_relaunch(oracle, world, plain_index, size, blocks, monkeypatch):
    """Case 5: 2000 units that each keep a whole list of `size` entries, on a fresh mapper: 256 000 and 600 000
    ids where the arena holds 8 a unit plus 2048 a wave.  The launch is repeated (once: the test does not retry
    and the call does not fail), units and tables are the oracle's, and an ordinary batch behind it on the same
    mapper accumulates as one big batch would (test_batches_accumulate's rule)."""
    from seekmer_amd import common
    if blocks is None:
        monkeypatch.delenv('SKM_TEST_MAP_BLOCKS', raising=False)
    else:
        monkeypatch.setenv('SKM_TEST_MAP_BLOCKS', str(blocks))
    units = world.fixture.whole_list_units(size, 2000, seed=size)
    first = lists.reads_of(units)
    second = lists.reads_of(world.fixture.singles)
    bases, offsets = oracle.pack_reads(first)
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(world.oindex, bases, offsets, len(first), False, fld)
    assert (expected.count == size).all()
    granted = 8 * len(first) + (1 if blocks else -(-len(first) // CONTEXTS)) * 4 * 2048 + 4096
    assert int(expected.count.sum()) > 2 * granted                # (the pool rounds a buffer up by an eighth at most)
    result, rm = _map(plain_index, bases, offsets, len(first), False)
    relaunches = result.timing()['map_relaunches']
    print('map kernel relaunches:', relaunches)
    assert relaunches == 1
    _compare_units(expected, rm.last_batch(len(first)))
    _compare_tables(oracle, expected, fld, result)
    # the ordinary batch behind it: per unit its own, the tables those of both batches as one
    s_bases, s_offsets, s_units, s_expected = world.batches[False][:4]
    rm.map_batch(common.ReadBatch(s_units, s_bases, s_offsets, False))
    _compare_units(s_expected, rm.last_batch(s_units))
    assert result.timing()['map_relaunches'] == 1                 # (the arena has grown: nothing to repeat)
    both_bases, both_offsets = oracle.pack_reads(first + second)
    both_fld = np.zeros(2000, dtype=np.int64)
    both = oracle.map_batch(world.oindex, both_bases, both_offsets, len(first) + len(second), False, both_fld)
    _compare_tables(oracle, both, both_fld, result)


def test_arena_relaunch_in_a_sample_set(oracle, world, plain_index):
    """Case 6: two samples in one sample set that keeps a histogram per sample; the set's first launch overflows the
    arena.  The spans of the launch that stood feed the histograms: per sample they, the table and the unaligned
    count are those of the sample mapped alone, and the oracle's."""
    from seekmer_amd import common, mapper
    fixture = world.fixture
    samples = [lists.reads_of(fixture.whole_list_units(300, 1000, seed=61) + fixture.singles[::2]),
               lists.reads_of(fixture.singles[1::3] + fixture.whole_list_units(128, 1000, seed=62))]
    sample_set = mapper.SampleSet(plain_index, False, per_sample_lengths=True)
    batches = []
    for i, reads in enumerate(samples):
        bases, offsets = oracle.pack_reads(reads)
        batches.append((bases, offsets, len(reads)))
        sample_set.add_batch(i, 0, common.ReadBatch(len(reads), bases, offsets, False))
    relaunches = sample_set.map_relaunches()
    print('map kernel relaunches of the set:', relaunches)
    assert relaunches >= 1
    tables = sample_set.export()
    sizes = sample_set.sizes()
    histograms = sample_set.sample_fragment_length_counts
    assert len(tables) == 2
    for i, (bases, offsets, n_units) in enumerate(batches):
        fld = np.zeros(2000, dtype=np.int64)
        expected = oracle.map_batch(world.oindex, bases, offsets, n_units, False, fld)
        classes = oracle.Classes()
        classes.update(expected)
        offs, ids, counts = classes.export()
        alone, _ = _map(plain_index, bases, offsets, n_units, False)
        _compare_tables(oracle, expected, fld, alone)
        a_offs, a_ids, a_counts, a_first, a_fld = alone.export()
        got_offs, got_ids, got_counts, got_first = tables[i]
        np.testing.assert_array_equal(got_offs, offs, err_msg='class_offsets of sample %d' % i)
        np.testing.assert_array_equal(got_ids, ids, err_msg='class_targets of sample %d' % i)
        np.testing.assert_array_equal(got_counts, counts, err_msg='class_counts of sample %d' % i)
        np.testing.assert_array_equal(got_first, a_first, err_msg='first_seen of sample %d' % i)
        np.testing.assert_array_equal(histograms[i], fld, err_msg='histogram of sample %d' % i)
        np.testing.assert_array_equal(histograms[i], a_fld)
        assert tuple(int(v) for v in sizes[i]) == tuple(int(v) for v in alone.sizes())
        assert int(sizes[i][2]) == classes.unaligned and int(sizes[i][3]) == n_units
    np.testing.assert_array_equal(histograms.sum(axis=0), sample_set.fragment_length_counts)


@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('mode', ['fr', 'rf'])
def test_the_strand_filter_on_long_runs(oracle, world, plain_index, mode, paired):
    """Case 7: strand_filter_kernel compacts a unit's run of ids in place and rekeys it.  Runs of 129 ids of both
    signs (the mixed family: 64 or 65 stay), runs of up to 300 of one sign (all stay, or the unit is emptied)."""
    bases, offsets, n_units, expected, fld, _ = world.batches[paired]
    filtered = filter_result(expected, mode)
    mixed = mixed_units(expected)
    assert (mixed & (expected.count == 129)).any() == (not paired)      # (a pair keeps the pattern: 43 of both signs)
    assert (mixed & (expected.count == 43)).any()
    assert ((filtered.count >= 192) & ~mixed).any() and ((filtered.count == 0) & (expected.count >= 192)).any()
    result, rm = _map(plain_index, bases, offsets, n_units, paired, strand=mode)
    begin, end, a_entry, a_offset, counts, entries = rm.last_batch(n_units)
    np.testing.assert_array_equal(counts, filtered.count)
    np.testing.assert_array_equal(entries, filtered.entries)
    np.testing.assert_array_equal(begin, expected.begin)
    np.testing.assert_array_equal(end, expected.end)
    np.testing.assert_array_equal(a_entry, expected.anchor_entry)
    np.testing.assert_array_equal(a_offset, expected.anchor_offset)
    _same_table(oracle, result, filtered, fld)
