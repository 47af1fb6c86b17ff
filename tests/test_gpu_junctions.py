"""The junction words successor_build_kernel writes into every contig record at upload (skm_device.h: DevSide::succ,
DevSide::kept), downloaded with skm_index_junctions and compared, word for word, with the host reference of
tests/junction_reference.py; the hooks and fall-backs that change or drop them; and reads made to go through
merge_by_record of the map kernel -- with the whole list of the contig they leave, and with a proper part of it
under a mask -- against the CPU oracle per unit.  What the reference itself is worth is checked without a GPU by
tests/test_junction_reference.py."""
import numpy as np
import pytest

import junction_reference as jr
from conftest import make_product_index
from test_gpu_parity import _compare_units, _run_gpu
from test_junction_reference import Case

pytestmark = pytest.mark.gpu

FLAGS = jr.WHOLE | jr.MASKED


@pytest.fixture(scope='module')
def cases(oracle, native_libs, chr21):
    return {'chr21': Case(oracle, chr21[1]),
            'segment chains': Case(oracle, jr.segment_chain_transcripts(np.random.default_rng(2024))),
            'boundaries': Case(oracle, jr.boundary_families()[0]),
            'one k-mer': Case(oracle, jr.single_kmer_transcripts())}


def _words(index):
    succ, kept = index.device_junctions()
    assert succ.shape == kept.shape == (index.contigs.size, 2, 4)
    return succ, kept


# ---- a. every word ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['chr21', 'segment chains', 'boundaries', 'one k-mer'])
def test_every_word_is_the_references(cases, name):
    case = cases[name]
    index = make_product_index(case.oindex)
    info = index.device_info()
    assert info['successors'] == 1 and info['sorted_targets'] == 1 and info['bucketed'] == 1
    got = _words(index)
    difference = jr.first_difference(case.ix, got, case.words)
    assert difference is None, difference
    # and the claim merge_by_record rests on, on the device's own words
    walks = jr.check_soundness(case.ix, got)
    assert (walks > 0) == (name != 'one k-mer')
    assert jr.census(case.ix, got) == case.census


def test_the_words_of_an_index_made_by_the_products_builder(cases, oracle):
    """The same transcriptome through index_builder (the arrays the product itself uploads)."""
    from seekmer_amd import index_builder
    transcripts = cases['segment chains'].transcripts
    ids = [b'R%04d' % i for i in range(len(transcripts))]
    tx_offsets = np.concatenate([[0], np.cumsum([len(t) for t in transcripts])]).astype(np.int64)
    pool = np.frombuffer(b''.join(transcripts) + b'\0', dtype=np.uint8).copy()
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    ix = jr.from_arrays(index)
    want = jr.expected_words(ix)
    got = _words(index)
    difference = jr.first_difference(ix, got, want)
    assert difference is None, difference
    assert jr.check_soundness(ix, got) > 0


# ---- b. hooks and fall-backs -----------------------------------------------------------------------------------
def test_every_successor_marked_look_it_up(cases, monkeypatch):
    monkeypatch.setenv('SKM_TEST_SUCC_LOOKUP', '1')
    case = cases['chr21']
    succ, kept = _words(make_product_index(case.oindex))
    absent = (case.words[0] & 3) == jr.ABSENT
    assert 0 < absent.sum() < absent.size
    assert (succ[absent] == jr.ABSENT).all()               # (word 0: unchanged)
    assert (succ[~absent] == jr.LOOKUP).all()              # kind LOOKUP, entry bits 0, no flag
    assert (kept == 0).all()


def test_no_successors_no_download(cases, native_libs, monkeypatch):
    monkeypatch.setenv('SKM_NO_SUCCESSORS', '1')
    index = make_product_index(cases['segment chains'].oindex)
    assert index.device_info()['successors'] == 0 and index.device_info()['bucketed'] == 1
    with pytest.raises(native_libs.NativeError) as refused:
        index.device_junctions()
    assert refused.value.code == native_libs.SKM_ERR_STATE


def test_one_slice_out_of_order_drops_every_flag(cases, oracle):
    case = cases['chr21']
    targets = case.oindex.targets.copy()
    contigs = case.oindex.contigs
    for c in range(contigs.size):
        first, n = int(contigs['target_offset'][c]), int(contigs['target_count'][c])
        if n >= 2 and targets['entry'][first] != targets['entry'][first + n - 1]:
            targets[[first, first + n - 1]] = targets[[first + n - 1, first]]
            break
    else:
        raise AssertionError('no slice of two distinct entries')
    shuffled = oracle.OracleIndex(case.oindex.kmers, contigs, case.oindex.sequences, targets, lengths=case.oindex.lengths)
    index = make_product_index(shuffled)
    assert index.device_info()['sorted_targets'] == 0 and index.device_info()['successors'] == 1
    succ, kept = _words(index)
    assert (succ & FLAGS == 0).all() and (kept == 0).all()
    assert (case.words[0] & FLAGS != 0).sum() > 10000
    np.testing.assert_array_equal(succ, case.words[0] & ~FLAGS)          # kinds and entries as they were


def test_no_buckets_no_words_and_the_reads_still_map(cases, oracle, native_libs, chr21, monkeypatch):
    """Without the bucket table the successors are never built: the record words stay as the upload zeroed them,
    nothing may read them, and reads map as the oracle maps them."""
    monkeypatch.setenv('SKM_NO_BUCKETS', '1')
    case = cases['chr21']
    index = make_product_index(case.oindex)
    info = index.device_info()
    assert info['bucketed'] == 0 and info['successors'] == 0
    with pytest.raises(native_libs.NativeError) as refused:
        index.device_junctions()
    assert refused.value.code == native_libs.SKM_ERR_STATE
    rng = np.random.default_rng(11)
    long_tx = [s for s in chr21[1] if len(s) > 200]
    reads = []
    for _ in range(200):
        t = long_tx[int(rng.integers(len(long_tx)))]
        at = int(rng.integers(0, len(t) - 100))
        reads.append(t[at:at + 100] if rng.random() < 0.5 else jr.reverse_complement_bases(t[at:at + 100]))
    bases, offsets = oracle.pack_reads(reads)
    expected = oracle.map_batch(case.oindex, bases, offsets, len(reads), False, np.zeros(2000, dtype=np.int64))
    assert (expected.count > 0).mean() > 0.9
    _, units = _run_gpu(index, bases, offsets, len(reads), False)
    _compare_units(expected, units)


# ---- c. directed reads through merge_by_record -----------------------------------------------------------------
class Directed:
    """The two batches, chosen with the reference alone, and what the oracle makes of them."""

    def __init__(self, oracle, case):
        ix, words = case.ix, case.words
        given = case.transcripts
        mirrored = [jr.reverse_complement_bases(s) for s in given]
        # whole list at the hop: every class of slot a transcript's path crosses, on either strand
        self.whole_reads, self.whole_classes = [], []
        # (a path enters a contig at an end and shares a transcript with the contig before: it crosses neither a
        # LOOKUP slot nor a mask that keeps nothing; every other class of the census it does, on either strand)
        crossable = {name for name in jr.placed_classes() if name[3] != 'masked, nothing kept'}
        for sequences in (given, mirrored):
            reads, names, crossed = jr.whole_list_reads(ix, words, sequences, per_class=20)      # (40 a class)
            assert set(crossed) == crossable == set(names), set(crossed) ^ crossable
            self.whole_reads += reads
            self.whole_classes += names
        lookups = jr.lookup_reads(ix, words)
        assert len(lookups) == case.census[('lookup',)] > 0
        self.whole_reads += lookups
        self.whole_classes += [('lookup',)] * len(lookups)
        assert 400 <= len(self.whole_reads) <= 1100 and all(len(r) <= 60 for r in self.whole_reads)
        # a proper part of the list at a hop that is not kept whole
        self.part_reads, self.part_j, self.part_size = [], [], []
        for strand, sequences in enumerate((given[:1200], mirrored[:1200])):
            reads, js, sizes = jr.sublist_reads(ix, words, sequences, cap=1000)
            assert len(reads) >= 200, (strand, len(reads))
            self.part_reads += reads
            self.part_j += js
            self.part_size += sizes
        assert set(self.part_j) == {3, 12} and 59 <= min(map(len, self.part_reads)) and max(map(len, self.part_reads)) <= 166
        self.batches = []
        for reads in (self.whole_reads, self.part_reads):
            bases, offsets = oracle.pack_reads(reads)
            expected = oracle.map_batch(case.oindex, bases, offsets, len(reads), False, np.zeros(2000, dtype=np.int64))
            for array in (bases, offsets, expected.count, expected.entries, expected.begin, expected.end):
                array.setflags(write=False)
            self.batches.append((bases, offsets, len(reads), expected))
        # the left walk has gone past the N into the contig before, and the list that leaves c0 is a proper part
        part = self.batches[1][3]
        assert (part.begin < np.asarray(self.part_j)).all()
        assert ((part.count > 0) & (part.count < np.asarray(self.part_size))).all()
        whole = self.batches[0][3]
        assert (whole.count > 0).mean() > 0.9


@pytest.fixture(scope='module')
def directed(oracle, cases):
    return Directed(oracle, cases['chr21'])


@pytest.mark.parametrize('hook', [None, 'SKM_TEST_SUCC_LOOKUP', 'SKM_NO_SUCCESSORS'])
def test_directed_reads_equal_the_oracles(cases, directed, hook, monkeypatch):
    """As uploaded (the flags settle the merges), with every successor marked "look it up", and without successors
    (filter_on_contig settles them all): the oracle's units every time."""
    if hook:
        monkeypatch.setenv(hook, '1')
    index = make_product_index(cases['chr21'].oindex)
    assert index.device_info()['successors'] == (0 if hook == 'SKM_NO_SUCCESSORS' else 1)
    for which, (bases, offsets, n_units, expected) in zip(('whole list', 'proper part'), directed.batches):
        _, units = _run_gpu(index, bases, offsets, n_units, False)
        try:
            _compare_units(expected, units)
        except AssertionError as error:
            raise AssertionError('%s reads, %s: %s' % (which, hook or 'as uploaded', error)) from None


@pytest.mark.parametrize('name', ['chr21', 'segment chains'])
def test_a_contig_met_again_the_other_way_round(oracle, cases, name):
    """merge_by_record's `set.forward != forward`: a read that first hits a contig, walks on, meets the same contig
    reverse complemented (hairpins on chr21, a segment and its reverse complement in one chain) and leaves it
    through a masked slot.  Its list is a part of that contig's slice in the orientation of the FIRST visit; the
    mask describes the list as the anchor of the second visit would read it, so this hop must merge."""
    case = cases[name]
    reads = []
    for sequences in (case.transcripts, [jr.reverse_complement_bases(s) for s in case.transcripts]):
        reads += jr.mirrored_visit_reads(case.ix, case.words, sequences)
    assert len(reads) >= 10
    bases, offsets = oracle.pack_reads(reads)
    expected = oracle.map_batch(case.oindex, bases, offsets, len(reads), False, np.zeros(2000, dtype=np.int64))
    assert (expected.begin == 0).all() and (expected.count > 0).all()
    _, units = _run_gpu(make_product_index(case.oindex), bases, offsets, len(reads), False)
    _compare_units(expected, units)
