"""The host reference of the junction words (tests/junction_reference.py) on its own, where nobody has a GPU:
the words it expects of four indexes are sound -- every flag it sets is what _filter_on_contig really does, for
every running list a read can arrive with -- and between them the indexes hold every class of slot there is.
tests/test_gpu_junctions.py compares the device's words with these."""
import numpy as np
import pytest

import junction_reference as jr


class Case:
    def __init__(self, oracle, transcripts):
        self.transcripts = transcripts
        self.oindex = oracle.build_index(transcripts)
        self.ix = jr.from_arrays(self.oindex)
        self.words = jr.expected_words(self.ix)
        self.census = jr.census(self.ix, self.words)
        for array in self.words:
            array.setflags(write=False)


@pytest.fixture(scope='module')
def chr21_case(oracle, chr21):
    return Case(oracle, chr21[1])


@pytest.fixture(scope='module')
def chain_case(oracle):
    return Case(oracle, jr.segment_chain_transcripts(np.random.default_rng(2024)))


@pytest.fixture(scope='module')
def boundary_case(oracle):
    case = Case(oracle, jr.boundary_families()[0])
    case.families = jr.boundary_families()[1]
    return case


@pytest.fixture(scope='module')
def single_case(oracle):
    return Case(oracle, jr.single_kmer_transcripts())


def _consistent(case):
    """What holds of any set of expected words: a slot per (contig, side, base), flags only where an entry is
    placed, a mask only under SUCC_MASKED."""
    succ, kept = case.words
    assert sum(case.census.values()) == 8 * case.ix.n_contigs
    placed = np.isin(succ & 3, (jr.AT_START, jr.AT_END))
    assert ((succ[~placed] & ~3) == 0).all() and (kept[(succ & jr.MASKED) == 0] == 0).all()
    assert case.ix.sorted_targets


def test_the_primitives_agree_with_one_another(oracle, chr21_case):
    """The array forms against the scalar ones, and both against the oracle's k-mer arithmetic."""
    rng = np.random.default_rng(3)
    kmers = rng.integers(0, 1 << 50, 2000, dtype=np.uint64)
    flipped = jr.reverse_complements(kmers)
    for kmer, rc in zip(kmers.tolist()[:300], flipped.tolist()):
        assert jr.reverse_complement(kmer) == rc == oracle.kmer_reverse_complement(kmer)
        assert jr.append(kmer, 2) == oracle.kmer_append(kmer, b'G') and jr.prepend(kmer, 3) == oracle.kmer_prepend(kmer, b'T')
    seq = b'ACGTNacgtTTGACCAGTAGGATCCAAGTTTACGN'
    assert jr.kmers_of(seq).tolist() == [oracle.kmer_encode(seq, i) for i in range(len(seq) - 24)]
    assert jr.encode(seq, 3) == oracle.kmer_encode(seq, 3)
    ix = chr21_case.ix
    stored = ix.stored_kmers[::997]
    queries = np.concatenate([stored, jr.reverse_complements(stored), kmers])
    found, entry, offset = ix.map_kmers(queries)
    assert found[:2 * stored.size].all() and not found[2 * stored.size:].any()
    for q, f, e, o in zip(queries.tolist(), found.tolist(), entry.tolist(), offset.tolist()):
        assert ix.map_kmer(q) == ((e, o) if f else None)
    # the walk with and without the bisection, on lists that ascend and lists that do not
    for trial in range(300):
        landing = rng.integers(-6, 12, int(rng.integers(1, 30))).tolist()
        if trial % 2:
            landing.sort()
        running = sorted(rng.integers(-6, 12, int(rng.integers(1, 9))).tolist())
        ix._oriented[10 ** 9] = (landing, False)
        plain = ix.filter_on_contig(running, 10 ** 9)
        ix._oriented[10 ** 9] = (landing, all(a <= b for a, b in zip(landing, landing[1:])))
        assert ix.filter_on_contig(running, 10 ** 9) == plain
    del ix._oriented[10 ** 9]


def test_chr21_holds_every_class_and_its_flags_are_sound(chr21_case):
    case = chr21_case
    _consistent(case)
    print('census of chr21:', sorted(case.census.items()))
    outcomes = _by_outcome(case.census)
    print('by outcome:', outcomes)
    assert case.census[('absent',)] >= 1 and case.census[('lookup',)] > 0
    for name in jr.placed_classes():
        assert case.census[name] >= 1, name
    walks = jr.check_soundness(case.ix, case.words)
    print('walks:', walks)
    assert walks > 500000


def _by_outcome(census):
    out = {}
    for name, n in census.items():
        key = name[-1]
        out[key] = out.get(key, 0) + n
    return out


def test_the_lookup_slots_of_chr21_land_inside_contigs(chr21_case):
    """The junction k-mers that are in the table at an offset that is neither 0 nor length - k: the only natural
    cover of the hop that looks its k-mer up."""
    ix = chr21_case.ix
    succ = chr21_case.words[0]
    inside = 0
    for c, side, b in zip(*np.nonzero((succ & 3) == jr.LOOKUP)):
        entry, offset = ix.map_kmer(ix.junction_kmer(int(c), int(side), int(b)))
        landing = entry if entry >= 0 else ~entry
        assert 0 < offset < ix.length[landing] - jr.K and succ[c, side, b] == jr.LOOKUP
        inside += 1
    assert inside == chr21_case.census[('lookup',)] > 0


def test_the_segment_chains(chain_case):
    """Transcripts listed twice by a contig, landings in both orientations, lists past the inline eight."""
    case = chain_case
    _consistent(case)
    print('census of the segment chains:', sorted(case.census.items()))
    outcomes = _by_outcome(case.census)
    for outcome in ('whole', 'masked', 'merge', 'merge, duplicate'):
        assert outcomes.get(outcome, 0) >= 1, outcome
    assert any(name[1:3] == ('reverse', 'long') for name in case.census if len(name) == 4)
    assert jr.check_soundness(case.ix, case.words) > 0


def _hop_onto_tail(case, family):
    """The last hop of the family's first member (which begins with P) before the contig of A: (the contig it
    leaves, side, base, the contig of A).  Among 4096 random prefixes the last bases before A repeat, so in the two
    large families the members reach A through a tree of contigs that they share with more and more others; the
    last of them holds about a quarter of the family.  In the small ones the contig of P runs up to A."""
    first, members, shared, prefix, tail = family
    ix = case.ix
    found, entry, offset = ix.path(case.transcripts[first])
    assert found.all()
    at = len(prefix)                                         # the k-mer that is A's first 25 bases
    c, d = _contig(int(entry[at - 1])), _contig(int(entry[at]))
    # (A's first k-mer is where a walk to the right enters its contig, stored as the transcripts read or mirrored)
    assert offset[at] == (0 if entry[at] >= 0 else ix.length[d] - jr.K) and c != d
    assert sorted(_contig(e) for e in ix.lists[d]) == list(range(first, first + members))
    assert set(range(first, first + shared)) <= {_contig(e) for e in ix.lists[c]}
    if members < 100:
        assert len(ix.lists[c]) == shared
    slots = [(side, b) for side in (0, 1) for b in range(4) if ix.junction(c, side, b)[0] in (jr.AT_START, jr.AT_END)
             and _contig(ix.junction(c, side, b)[1]) == d]
    assert len(slots) == 1
    return c, slots[0][0], slots[0][1], d


def test_the_boundaries_of_both_flags(boundary_case):
    """n_to = 4096 against 4097 (the longest landing list the upload walks) and n_from = 8 against 9 (the longest
    list a mask describes)."""
    case = boundary_case
    _consistent(case)
    print('census of the boundary families:', sorted(case.census.items()))
    succ, kept = case.words
    ix = case.ix
    flags, back = [], []
    for family in case.families:
        c, side, b, d = _hop_onto_tail(case, family)
        word = int(succ[c, side, b])
        assert (word & 3) in (jr.AT_START, jr.AT_END) and _contig(jr.entry_of(word)) == d
        flags.append(word & (jr.WHOLE | jr.MASKED))
        # every hop that lands on the contig of A leaves a part of its list: all of them as this one
        onto = [int(succ[c2, s2, b2]) & (jr.WHOLE | jr.MASKED)
                for c2, s2, b2 in zip(*np.nonzero(np.isin(succ & 3, (jr.AT_START, jr.AT_END))))
                if _contig(jr.entry_of(succ[c2, s2, b2])) == d]
        assert len(onto) >= 1 + (family[1] > family[2]) and set(onto) == {flags[-1]}
        # the way back, from the contig of A: a list of `members` entries against a part of them
        slots = [(s2, b2) for s2 in (0, 1) for b2 in range(4)
                 if (succ[d, s2, b2] & 3) in (jr.AT_START, jr.AT_END) and _contig(jr.entry_of(succ[d, s2, b2])) == c]
        assert len(slots) == 1
        back.append((int(succ[d][slots[0]]) & (jr.WHOLE | jr.MASKED), int(kept[d][slots[0]])))
    assert flags == [jr.WHOLE, 0, jr.WHOLE, jr.WHOLE, jr.WHOLE]
    # (4096, 4097, 9 and 10 entries: no mask; the 8 entries of the last family: a mask that keeps the five of P)
    assert back[:4] == [(0, 0), (0, 0), (0, 0), (0, 0)]
    assert back[4][0] == jr.MASKED and bin(back[4][1]).count('1') == 5
    # and wherever a hop of this index is not kept whole: a mask for every list of up to eight entries, none for a
    # longer one
    by_length = {}
    for c, side, b in zip(*np.nonzero(np.isin(succ & 3, (jr.AT_START, jr.AT_END)) & ((succ & jr.WHOLE) == 0))):
        if len(ix.lists[_contig(jr.entry_of(succ[c, side, b]))]) <= jr.LONGEST_LANDING:
            by_length.setdefault(len(ix.lists[c]), set()).add(int(succ[c, side, b]) & jr.MASKED)
    assert by_length[8] == {jr.MASKED} and by_length[9] == {0} and by_length[10] == {0}
    assert all(found == ({jr.MASKED} if n <= jr.INLINE_TARGETS else {0}) for n, found in by_length.items())
    assert jr.check_soundness(case.ix, case.words) > 0


def _contig(entry):
    return entry if entry >= 0 else ~entry


def test_a_contig_of_exactly_k_bases(single_case):
    """One transcript of 25 bases: one contig, whose tail k-mer at the end is first_kmer; nothing follows it."""
    case = single_case
    _consistent(case)
    ix = case.ix
    assert ix.n_contigs == 1 and ix.length[0] == jr.K
    assert [ix.junction_kmer(0, jr.SIDE_END, b) for b in range(4)] == [jr.append(ix.first_kmer[0], b) for b in range(4)]
    assert case.census == {('absent',): 8}
    assert jr.check_soundness(case.ix, case.words) == 0
