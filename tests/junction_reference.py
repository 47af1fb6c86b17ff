"""Host reference of the junction words of the contig records (seekmer_amd/csrc/skm_device.h: DevSide::succ,
DevSide::kept; successor_build_kernel in skm_map.hip) and of the claim the map kernel's merge_by_record rests on.

Plain Python and numpy over the four index arrays (kmers, contigs, sequences, targets in the reference's
layout); nothing of the product or of the oracle is imported.  The pieces:

  Index.map_kmer          KMerIndex.map_kmer (seekmer/_common.pyx:54-97) as a dict of the stored k-mers
  Index.filter_on_contig  KMerIndex._filter_on_contig (_common.pyx:185-235) on lists of signed entries
  expected_words          succ / kept of every record by the documented rule
  check_soundness         "flag => what _filter_on_contig really does", whatever computed the flags
  census                  how many slots of each class a set of words has
  and what the directed reads of tests/test_gpu_junctions.py are chosen with (paths, the four test transcriptomes).
"""
import bisect
import collections
import itertools

import numpy as np

K = 25
KMER_MASK = (1 << (2 * K)) - 1
KMER_INVALID = 0xFFFFFFFFFFFFFFFF
INLINE_TARGETS = 8                  # CONTIG_INLINE_TARGETS: the longest list a mask (one byte) describes
LONGEST_LANDING = 4096              # the longest landing list successor_build_kernel walks
ABSENT, AT_START, AT_END, LOOKUP = 0, 1, 2, 3
WHOLE, MASKED = 4, 8
ENTRY_SHIFT = 4
SIDE_END, SIDE_START = 0, 1

_CODES = np.zeros(256, dtype=np.uint8)           # _kmer.pxd:253-273: everything but ACGT/acgt encodes as A
for _i, _c in enumerate(b'ACGT'):
    _CODES[_c] = _CODES[_c + 32] = _i
COMPLEMENT = bytes.maketrans(b'ACGT', b'TGCA')


def reverse_complement_bases(seq):
    return bytes(seq).translate(COMPLEMENT)[::-1]


def encode(seq, at=0):
    kmer = 0
    for c in bytes(seq[at:at + K]):
        kmer = (kmer << 2) | int(_CODES[c])
    return kmer


def reverse_complement(kmer):
    out = 0
    for _ in range(K):
        out = (out << 2) | (3 - (kmer & 3))
        kmer >>= 2
    return out


def append(kmer, b):
    return ((kmer << 2) | b) & KMER_MASK


def prepend(kmer, b):
    return (kmer >> 2) | (b << (2 * K - 2))


def kmers_of(seq):
    """Every k-mer of a sequence, in order, as uint64."""
    codes = _CODES[np.frombuffer(bytes(seq), dtype=np.uint8)].astype(np.uint64)
    n = codes.size - K + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    out = np.zeros(n, dtype=np.uint64)
    for i in range(K):
        out |= codes[i:i + n] << np.uint64(2 * (K - 1 - i))
    return out


def reverse_complements(kmers):
    """reverse_complement of an array (the 2-bit groups of the word reversed, shifted down, complemented)."""
    k = np.asarray(kmers, dtype=np.uint64)
    three, nibble = np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
    k = ((k >> np.uint64(2)) & three) | ((k & three) << np.uint64(2))
    k = ((k >> np.uint64(4)) & nibble) | ((k & nibble) << np.uint64(4))
    k = k.byteswap() >> np.uint64(64 - 2 * K)
    return ~k & np.uint64(KMER_MASK)


def _field(array, i):
    return array[array.dtype.names[i]]


class Index:
    """The four arrays as Python lists and a dict."""

    def __init__(self, kmers, contigs, sequences, targets):
        stored = _field(kmers, 0) != np.uint64(KMER_INVALID)
        self.stored_kmers = _field(kmers, 0)[stored]
        self.stored_entry = _field(kmers, 1)[stored].astype(np.int32)
        self.stored_offset = _field(kmers, 2)[stored].astype(np.int32)
        self.table = dict(zip(self.stored_kmers.tolist(), zip(self.stored_entry.tolist(), self.stored_offset.tolist())))
        assert len(self.table) == self.stored_kmers.size, 'a k-mer is stored twice: not a built index'
        order = np.argsort(self.stored_kmers)
        self._sorted = (self.stored_kmers[order], self.stored_entry[order], self.stored_offset[order])
        self.n_contigs = int(contigs.size)
        self.pooled = bytes(np.ascontiguousarray(sequences).view(np.uint8))
        self.contig_offset = _field(contigs, 0).tolist()
        self.length = _field(contigs, 1).tolist()
        self.first_kmer = _field(contigs, 2).tolist()
        self.last_kmer = _field(contigs, 3).tolist()
        entries = _field(targets, 0).tolist()
        self.lists = [entries[a:a + n] for a, n in zip(_field(contigs, 4).tolist(), _field(contigs, 5).tolist())]
        # skm_index_info[7]: every slice ascends by signed entry
        self.sorted_targets = all(all(a <= b for a, b in zip(l, l[1:])) for l in self.lists)
        self._oriented = {}
        self._counted = {}
        self.hops_of = {}

    # ---- KMerIndex.map_kmer
    def map_kmer(self, kmer):
        """(entry, offset) of a k-mer of the table, the entry complemented when the table stores the reverse
        complement; None when neither is stored."""
        at = self.table.get(kmer)
        if at is not None:
            return at
        at = self.table.get(reverse_complement(kmer))
        if at is not None:
            return (~at[0], at[1])
        return None

    def map_kmers(self, kmers):
        """map_kmer of an array: (found, entry, offset); (0, -1) where not found, as the invalid coordinate."""
        kmers = np.asarray(kmers, dtype=np.uint64)
        keys, entry, offset = self._sorted
        found = np.zeros(kmers.size, dtype=bool)
        out_entry = np.zeros(kmers.size, dtype=np.int32)
        out_offset = np.full(kmers.size, -1, dtype=np.int32)
        if keys.size == 0:
            return found, out_entry, out_offset
        for query, flip in ((reverse_complements(kmers), True), (kmers, False)):     # (the k-mer itself wins)
            at = np.minimum(np.searchsorted(keys, query), keys.size - 1)
            hit = keys[at] == query
            out_entry[hit] = ~entry[at[hit]] if flip else entry[at[hit]]
            out_offset[hit] = offset[at[hit]]
            found |= hit
        return found, out_entry, out_offset

    # ---- KMerIndex.map_contig / _filter_on_contig
    def oriented_list(self, entry):
        """map_contig: the list of the contig as an anchor of this sign reads it."""
        got = self._oriented.get(entry)
        if got is None:
            got = self.lists[entry] if entry >= 0 else [~e for e in reversed(self.lists[~entry])]
            ascending = all(a <= b for a, b in zip(got, got[1:]))
            got = self._oriented[entry] = (got, ascending)
        return got[0]

    def filter_on_contig(self, running, landing_entry):
        """The two-pointer walk of _filter_on_contig: the positions of `running` it keeps.  (Where the landing
        list ascends, the steps that only advance its pointer are taken together: the same pointer, found by
        bisection.)"""
        landing = self.oriented_list(landing_entry)
        ascending = self._oriented[landing_entry][1]
        kept = []
        r = t = 0
        n, m = len(running), len(landing)
        while r != n and t != m:
            a, b = running[r], landing[t]
            if a == b:
                kept.append(r)
                r += 1
                t += 1
            elif a < b:
                r += 1
            elif ascending:
                t = bisect.bisect_left(landing, a, t + 1)
            else:
                t += 1
        return kept

    def counted_list(self, entry):
        got = self._counted.get(entry)
        if got is None:
            got = self._counted[entry] = collections.Counter(self.oriented_list(entry))
        return got

    # ---- the junction k-mers
    def junction_kmer(self, contig, side, b):
        """END: append(tail k-mer, b), the tail k-mer of a contig of exactly k bases being first_kmer
        (get_tail_kmer tells the two by offset == 0); START: prepend(first_kmer, b)."""
        if side == SIDE_END:
            tail = self.first_kmer[contig] if self.length[contig] == K else self.last_kmer[contig]
            return append(tail, b)
        return prepend(self.first_kmer[contig], b)

    def junction(self, contig, side, b):
        """(kind, landing entry or None) of a slot."""
        at = self.map_kmer(self.junction_kmer(contig, side, b))
        if at is None:
            return ABSENT, None
        entry, offset = at
        if offset < 0:
            return LOOKUP, entry
        landing = entry if entry >= 0 else ~entry
        if offset == 0:
            return AT_START, entry
        if offset == self.length[landing] - K:
            return AT_END, entry
        return LOOKUP, entry

    def contig_bases(self, contig):
        return self.pooled[self.contig_offset[contig]:self.contig_offset[contig] + self.length[contig]]

    def path(self, seq):
        """The k-mers of a sequence through the table: (found bool[n], entry int32[n], offset int32[n])."""
        return self.map_kmers(kmers_of(seq))


def from_arrays(index):
    """Index of anything that has .kmers, .contigs, .sequences, .targets."""
    return Index(index.kmers, index.contigs, index.sequences, index.targets)


def word_of(kind, entry=0, flags=0):
    word = (((entry << ENTRY_SHIFT) | flags | kind) if kind in (AT_START, AT_END) else kind) & 0xFFFFFFFF
    return word - (1 << 32) if word >= (1 << 31) else word


def entry_of(word):
    return int(word) >> ENTRY_SHIFT


def expected_words(ix):
    """succ int32[n_contigs, 2, 4] and kept uint8[n_contigs, 2, 4] by the rule of skm_device.h."""
    succ = np.zeros((ix.n_contigs, 2, 4), dtype=np.int32)
    kept = np.zeros((ix.n_contigs, 2, 4), dtype=np.uint8)
    for c in range(ix.n_contigs):
        leaving = ix.lists[c]
        n_from = len(leaving)
        distinct = len(set(leaving)) == n_from
        for side in (SIDE_END, SIDE_START):
            for b in range(4):
                kind, entry = ix.junction(c, side, b)
                if kind not in (AT_START, AT_END):
                    succ[c, side, b] = word_of(kind)
                    continue
                flags = 0
                n_to = len(ix.lists[entry if entry >= 0 else ~entry])
                if ix.sorted_targets and n_to <= LONGEST_LANDING:
                    counted = ix.counted_list(entry)
                    # as multisets, in the orientation the hop arrives in
                    if n_from <= n_to and all(counted[e] >= n for e, n in collections.Counter(leaving).items()):
                        flags = WHOLE
                    elif n_from <= INLINE_TARGETS and distinct:
                        flags = MASKED
                        kept[c, side, b] = sum(1 << i for i in ix.filter_on_contig(leaving, entry))
                succ[c, side, b] = word_of(kind, entry, flags)
    return succ, kept


def sublists(n):
    """The position sets a running list is checked with: all of them for a list that a mask can describe; the
    whole list, every single entry, the even and the odd positions for a longer one."""
    if n <= INLINE_TARGETS:
        for size in range(1, n + 1):
            yield from itertools.combinations(range(n), size)
        return
    yield tuple(range(n))
    for i in range(n):
        yield (i,)
    yield tuple(range(0, n, 2))
    yield tuple(range(1, n, 2))


def check_soundness(ix, words):
    """Every slot of `words` that carries WHOLE or MASKED: with a running list made of the positions S of the
    leaving contig's list, in either read orientation (in the reverse one both lists are reversed and
    complemented), _filter_on_contig on the landing contig keeps exactly S (WHOLE) or S and `kept` (MASKED).
    Returns the number of walks."""
    succ, kept = words
    walks = 0
    for c, side, b in zip(*np.nonzero(succ & (WHOLE | MASKED))):
        word = int(succ[c, side, b])
        assert (word & 3) in (AT_START, AT_END), ('a flag on a slot that places no entry', c, side, b, word)
        assert (word & (WHOLE | MASKED)) != (WHOLE | MASKED), ('both flags', c, side, b, word)
        entry = entry_of(word)
        leaving = ix.lists[c]
        n = len(leaving)
        assert 0 <= (entry if entry >= 0 else ~entry) < ix.n_contigs, ('no such contig', c, side, b, word)
        if word & MASKED:
            assert n <= INLINE_TARGETS and int(kept[c, side, b]) >> n == 0, ('a mask wider than its list', c, side, b)
        else:
            assert kept[c, side, b] == 0, ('a mask without SUCC_MASKED', c, side, b)
        mask = set(range(n)) if word & WHOLE else {i for i in range(n) if (int(kept[c, side, b]) >> i) & 1}
        for positions in sublists(n):
            want = [i for i in positions if i in mask]
            forward = ix.filter_on_contig([leaving[i] for i in positions], entry)
            got = [positions[r] for r in forward]
            assert got == want, ('forward', int(c), int(side), int(b), word, positions, got, want, leaving,
                                 ix.oriented_list(entry))
            mirrored = positions[::-1]
            reverse = ix.filter_on_contig([~leaving[i] for i in mirrored], ~entry)
            got = sorted(mirrored[r] for r in reverse)
            assert got == want, ('reverse', int(c), int(side), int(b), word, positions, got, want, leaving,
                                 ix.oriented_list(~entry))
            walks += 2
    return walks


KIND_NAMES = {ABSENT: 'absent', AT_START: 'start', AT_END: 'end', LOOKUP: 'lookup'}


def slot_class(ix, words, c, side, b):
    """('absent',) / ('lookup',) / (kind, sign of the landing entry, leaving list short or long, outcome)."""
    succ, kept = words
    word = int(succ[c, side, b])
    kind = word & 3
    if kind in (ABSENT, LOOKUP):
        return (KIND_NAMES[kind],)
    leaving = ix.lists[c]
    if word & WHOLE:
        outcome = 'whole'
    elif word & MASKED:
        outcome = 'masked' if kept[c, side, b] else 'masked, nothing kept'
    else:
        outcome = 'merge' if len(set(leaving)) == len(leaving) else 'merge, duplicate'
    return (KIND_NAMES[kind], 'forward' if entry_of(word) >= 0 else 'reverse',
            'short' if len(leaving) <= INLINE_TARGETS else 'long', outcome)


def census(ix, words):
    counts = collections.Counter()
    for c in range(ix.n_contigs):
        for side in (SIDE_END, SIDE_START):
            for b in range(4):
                counts[slot_class(ix, words, c, side, b)] += 1
    return counts


def placed_classes():
    """Every class a slot that places an entry can be of when no landing list is longer than LONGEST_LANDING: a
    mask describes short lists only, and a short list that is not kept whole goes without one only for a transcript
    listed twice."""
    out = []
    for kind in ('start', 'end'):
        for sign in ('forward', 'reverse'):
            for outcome in ('whole', 'masked', 'masked, nothing kept', 'merge, duplicate'):
                out.append((kind, sign, 'short', outcome))
            for outcome in ('whole', 'merge', 'merge, duplicate'):
                out.append((kind, sign, 'long', outcome))
    return out


def first_difference(ix, got, want):
    """None, or a description of the first slot where two sets of words differ."""
    differ = np.argwhere((got[0] != want[0]) | (got[1] != want[1]))
    if differ.size == 0:
        return None
    c, side, b = (int(v) for v in differ[0])
    kind, entry = ix.junction(c, side, b)
    landing = None if entry is None else ix.oriented_list(entry)
    return ('%d slots differ; first: contig %d side %d base %d: word %#x kept %#x, expected word %#x kept %#x; '
            'leaving list %r, landing %s entry %r list %r'
            % (len(differ), c, side, b, int(got[0][c, side, b]) & 0xFFFFFFFF, int(got[1][c, side, b]),
               int(want[0][c, side, b]) & 0xFFFFFFFF, int(want[1][c, side, b]), ix.lists[c], KIND_NAMES[kind], entry,
               landing))


# ---- the transcriptomes the words are pinned on (besides the reference's chr21) --------------------------------
def _random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), n))


def segment_chain_transcripts(rng):
    """Chains of segments drawn from a small pool, any segment forwards or reverse complemented and possibly
    several times in one transcript: contigs that list a transcript twice, hops that land in the other
    orientation, lists that are supersets and lists that are not at nearly every junction, lists longer than
    the eight inline targets.  Draws from `rng`, which the caller goes on using."""
    segments = [_random_bases(rng, int(rng.integers(26, 140))) for _ in range(40)]
    transcripts = []
    for _ in range(90):
        parts = []
        for _ in range(int(rng.integers(3, 10))):
            seg = segments[int(rng.integers(len(segments)))]
            parts.append(seg.translate(COMPLEMENT)[::-1] if rng.random() < 0.35 else seg)
        if rng.random() < 0.5:                      # a segment twice in the same transcript, some way apart
            parts.insert(int(rng.integers(len(parts) + 1)), parts[0])
        transcripts.append(b''.join(parts))
    return transcripts


def boundary_families(seed=4096):
    """Families of transcripts X + A: A is 40 bases shared by the family; X is a 40-base prefix P shared by the
    first `shared` members and 30 bases of the member's own for the rest.  The junction P -> A leaves a list of
    `shared` entries for one of `members`: (4096, 5) and (4097, 5) sit on either side of the longest landing list
    the upload walks; (9, 8) and (10, 9) leave 8 and 9 entries for a list that holds them all.  The way back, from
    the contig of A onto the contig of P, leaves `members` entries for `shared` of them: (8, 5) and (9, 8) sit on
    either side of the longest list a mask describes.
    Returns (transcripts, [(first transcript, members, shared, P, A)])."""
    rng = np.random.default_rng(seed)
    transcripts, families = [], []
    for members, shared in ((4096, 5), (4097, 5), (9, 8), (10, 9), (8, 5)):
        tail, prefix = _random_bases(rng, 40), _random_bases(rng, 40)
        families.append((len(transcripts), members, shared, prefix, tail))
        for i in range(members):
            own = bytearray(_random_bases(rng, 30))
            if members - shared <= 3:               # (a small family: no member's own bases end as P or as another's do)
                own[-1] = b'ACGT'[(b'ACGT'.index(prefix[-1:]) + 1 + i - shared) % 4]
            transcripts.append((prefix if i < shared else bytes(own)) + tail)
    return transcripts, families


def single_kmer_transcripts(seed=25):
    """One transcript of exactly k bases: its contig's tail k-mer is first_kmer."""
    return [_random_bases(np.random.default_rng(seed), K)]


# ---- reads that cross chosen junctions (tests/test_gpu_junctions.py) -------------------------------------------
def stretches(found, entry, offset):
    """A path cut where it changes contig: (first, last) k-mer of every run of consecutive k-mers that lie side by
    side in one contig, in walking order.  Runs of k-mers that are not in the table are left out."""
    n = found.size
    if n == 0:
        return []
    step = np.where(entry[1:] >= 0, 1, -1)
    joined = found[1:] & found[:-1] & (entry[1:] == entry[:-1]) & (offset[1:] - offset[:-1] == step)
    firsts = np.flatnonzero(np.concatenate([[True], ~joined]))
    lasts = np.concatenate([firsts[1:] - 1, [n - 1]])
    return [(int(a), int(b)) for a, b in zip(firsts, lasts) if found[a]]


def leaving_slot(ix, entry, offset, next_base):
    """The slot a walk to the right reads when its anchor (entry, offset) is the last k-mer of its contig in read
    direction and the read goes on with `next_base` (a code): (contig, side, b); None when the k-mer is not at that
    end of its contig."""
    contig = entry if entry >= 0 else ~entry
    if offset != (ix.length[contig] - K if entry >= 0 else 0):
        return None
    return (contig, SIDE_END, next_base) if entry >= 0 else (contig, SIDE_START, 3 - next_base)


def _hops(ix, seq):
    """Every place where the path of a sequence goes from one stretch straight on into the next:
    (index of the stretch it leaves, slot, first k-mer of the next stretch), and the stretches."""
    if seq in ix.hops_of:
        return ix.hops_of[seq]
    found, entry, offset = ix.path(seq)
    runs = stretches(found, entry, offset)
    out = []
    for i in range(len(runs) - 1):
        last, q = runs[i][1], runs[i + 1][0]
        if last + 1 != q:
            continue
        slot = leaving_slot(ix, int(entry[last]), int(offset[last]), int(_CODES[seq[q + K - 1]]))
        if slot is not None:
            out.append((i, slot, q))
    ix.hops_of[seq] = out, runs, entry
    return out, runs, entry


def whole_list_reads(ix, words, sequences, per_class=40, before=35):
    """One read of before + k bases per chosen hop: `before` bases in front of the first k-mer of the stretch the hop
    lands on and that k-mer.  Up to per_class hops of every class of slot (slot_class) that the paths of the
    sequences cross, those first where the read begins on the contig it leaves (its whole list arrives at the hop).
    Returns (reads, class of each, classes crossed with their counts)."""
    crossed = collections.Counter()
    first_choice, second_choice = collections.defaultdict(list), collections.defaultdict(list)
    for seq in sequences:
        hops, runs, _ = _hops(ix, seq)
        for i, slot, q in hops:
            name = slot_class(ix, words, *slot)
            crossed[name] += 1
            if q < before:
                continue
            pile = first_choice if runs[i][0] <= q - before else second_choice
            if len(pile[name]) < per_class:
                pile[name].append(bytes(seq[q - before:q + K]))
    reads, names = [], []
    for name in sorted(crossed):
        for read in (first_choice[name] + second_choice[name])[:per_class]:
            reads.append(read)
            names.append(name)
    return reads, names, crossed


def sublist_reads(ix, words, sequences, before=(3, 12), beyond=54, cap=1000):
    """Reads that leave a contig through a slot that is not SUCC_WHOLE with a proper part of its list.  For stretches
    l, c0, r that follow one another, c0 of 2 to 100 k-mers with a list of up to eight distinct entries of which l
    shares some but not all: the sequence from j bases before c0's first k-mer to `beyond` bases past r's first,
    with N at read position j (c0's first base, which is not A: N encodes as A -- and not the base behind it either:
    the alignment step of the walk to the left compares c0's first eight bases with the read from the N on, and
    over a run of one base it can settle one base off, which sends the hop elsewhere).  By the dict, k-mers 0..j are not
    in the table and k-mer j + 1 -- c0's second -- is: the first hit, at a position > 0, walks left into l, which
    narrows the list, then right out of c0.  Returns (reads, j of each, length of c0's list for each)."""
    reads, js, sizes = [], [], []
    for seq in sequences:
        hops, runs, entry = _hops(ix, seq)
        leaves = {i: (slot, q) for i, slot, q in hops}
        for i in sorted(leaves):
            if i - 1 not in leaves:
                continue
            (c0, side, b), q = leaves[i]
            first, last = runs[i]
            mine = ix.oriented_list(int(entry[first]))
            theirs = set(ix.oriented_list(int(entry[runs[i - 1][1]])))
            shared = sum(1 for e in mine if e in theirs)
            if not (len(mine) <= INLINE_TARGETS and len(set(mine)) == len(mine) and 2 <= last - first + 1 <= 100
                    and 0 < shared < len(mine) and (int(words[0][c0, side, b]) & WHOLE) == 0
                    and seq[first:first + 1] in (b'C', b'G', b'T') and seq[first] != seq[first + 1]):
                continue
            for j in before:
                if first - j < 0 or q + beyond > len(seq):
                    continue
                read = bytearray(seq[first - j:q + beyond])
                read[j] = ord('N')
                hit = ix.map_kmers(kmers_of(read)[:j + 2])[0]
                if hit[:j + 1].any() or not hit[j + 1]:
                    continue
                reads.append(bytes(read))
                js.append(j)
                sizes.append(len(mine))
                if len(reads) >= cap:
                    return reads, js, sizes
    return reads, js, sizes


def lookup_reads(ix, words, before=35):
    """No transcript's path crosses a slot of kind LOOKUP (its k-mer lies inside another contig, which a path
    enters at an end), so the reads are made from the contig itself: up to `before` + k - 1 bases at the end the
    slot belongs to and the slot's base, read in the direction that walks out of that end."""
    reads = []
    for c, side, b in zip(*np.nonzero((words[0] & 3) == LOOKUP)):
        bases = ix.contig_bases(int(c))
        if side == SIDE_END:
            reads.append(bases[-(before + K - 1):] + b'ACGT'[b:b + 1])
        else:
            reads.append(reverse_complement_bases(b'ACGT'[b:b + 1] + bases[:before + K - 1]))
    return reads


def mirrored_visit_reads(ix, words, sequences, longest=1000, beyond=30):
    """Reads that begin on the first k-mer of a stretch on a contig with a list of up to eight distinct entries and
    run on until their path has come back to the SAME contig the other way round (a transcript that holds a segment
    and, further on, its reverse complement) and left it through a slot with SUCC_MASKED, `beyond` bases past the
    landing k-mer.  The running list is still a part of that contig's slice, but in the orientation of the first
    hit, not of the anchor: the stored mask does not describe it, and the hop has to merge."""
    reads = []
    for seq in sequences:
        hops, runs, entry = _hops(ix, seq)
        leaves = {i: (slot, q) for i, slot, q in hops}
        for i, (first, _) in enumerate(runs):
            e = int(entry[first])
            mine = ix.oriented_list(e)
            if len(mine) > INLINE_TARGETS or len(set(mine)) != len(mine):
                continue
            for k in range(i + 1, len(runs)):
                if runs[k][0] - first > longest:
                    break
                if runs[k - 1][1] + 1 != runs[k][0]:
                    break                               # (k-mers that are not in the table: the walk ends there)
                if int(entry[runs[k][0]]) != ~e or k not in leaves:
                    continue
                (c, side, b), q = leaves[k]
                if (int(words[0][c, side, b]) & MASKED) and q + K + beyond <= len(seq):
                    reads.append(bytes(seq[first:q + K + beyond]))
    return reads
