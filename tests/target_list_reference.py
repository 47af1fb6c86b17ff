"""A constructed transcriptome whose reads put the mapper's running target list at chosen sizes and
leave chosen list positions set (tests/test_target_lists.py, tests/test_gpu_target_lists.py).

The map kernel keeps the running list of a read as a slice of the index's target array plus a
keep-mask (skm_map.hip, TSet): lists of at most 8 entries settle on a byte of the contig record,
lists of at most 16 run on registers, longer ones take the two-pointer walks over a 64-bit mask, and
lists of more than 64 entries keep mask words 1.. in an HBM workspace with a staging copy.  The
reference's own test data hardly leaves the first two forms, so this fixture is built to order.

FAMILIES of N transcripts with consecutive ids, N in SIZES.  Member m of a family is list position m
of the family's contigs (the builder sorts a slice by signed entry; check_list_positions asserts it).
A family has PATTERNS, subsets of its member indices: the first member, the last, the even ones, and
around every edge E of EDGES below N the members below E, from E on, and the two at the edge.  For
every pattern k every member carries

    core_k   80 random bases shared by all N members, and directly behind it
    seg_k    60 random bases shared by the pattern's members (60 bases of its own for a non-member),

with 30 random bases of the member's own between such blocks and at both ends.  The contig of core_k
lists N transcripts; a read that runs from core_k into seg_k narrows the list to the pattern, i.e. to
chosen bit positions of the mask.  Every read is used as it is and reverse complemented, which
mirrors the list positions.

Beside the sized families: a family whose odd members carry core + seg reverse complemented (a list
of both signs), families whose members hold a core twice (every transcript listed twice by one
contig), and reads that belong nowhere -- chimeras of two families, pairs with a mate from each, Ns.

Everything is seeded; nothing here touches the product or the oracle."""
import numpy as np

from strand_reference import reverse_complement

SEED = 5
SIZES = (1, 8, 9, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 300)
EDGES = (8, 16, 64, 128, 192)
MIXED_SIZE = 129
TWICE_SIZES = (5, 8, 9, 40)
CORE, SEG, OWN = 80, 60, 30
# windows of core + seg (140 bases): the first two stay inside the core and keep the whole list, the
# others run into the segment and keep the pattern ([55:140] begins at the core's last k-mer)
WHOLE_WINDOWS = ((0, 80), (10, 70))
PATTERN_WINDOWS = ((30, 130), (50, 140), (55, 140))
# pairs from the fragment (core + seg)[0:140]: (mate 1 window, mate 2 window; mate 2 is reverse complemented).
# In the first two a mate stays on one contig: the long list and the short one meet in the intersection alone.
# In the third both mates cross the junction, so either mate's context merges a long list before that.
PAIR_WINDOWS = (((0, 70), (85, 140)), ((10, 80), (80, 140)), ((30, 130), (60, 140)))


_LETTERS = np.frombuffer(b'ACGT', dtype=np.uint8)


def _random_bases(rng, n):
    return _LETTERS[rng.integers(0, 4, n)].tobytes()


def patterns_of(n):
    """name -> sorted member indices, in a fixed order."""
    out = {'first': [0], 'last': [n - 1], 'even': list(range(0, n, 2))}
    for edge in EDGES:
        if n > edge:
            out['lo_%d' % edge] = list(range(edge))
            out['hi_%d' % edge] = list(range(edge, n))
            out['at_%d' % edge] = [edge - 1, edge]
    return out


class Family:
    """kind: 'sized', 'mixed' (odd members reverse complemented), 'twice' (the core twice), 'other'."""

    def __init__(self, kind, first_id, size, patterns):
        self.kind = kind
        self.first_id = first_id
        self.size = size
        self.patterns = patterns            # name -> member indices
        self.core = {}                      # name -> bytes
        self.seg = {}

    def ids(self, members=None):
        members = range(self.size) if members is None else members
        return tuple(self.first_id + m for m in members)


class Unit:
    """One unit of a batch: its reads (one or two) and what it was made to reach.
    targets: the transcripts the unit must keep, ascending (None: whatever the reference makes of it);
    listed: the number of list entries that stands for (twice the transcripts in a 'twice' family)."""

    def __init__(self, reads, family, pattern, targets, listed=None, note=''):
        self.reads = tuple(reads)
        self.family = family
        self.pattern = pattern
        self.targets = targets
        self.listed = listed if listed is not None else (None if targets is None else len(targets))
        self.note = note


class Fixture:
    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        self.sequences = []
        self.families = []
        for size in SIZES:
            self._add_family(rng, 'sized', size, patterns_of(size))
        self.sized_bases = sum(len(s) for s in self.sequences)
        self.mixed = self._add_family(rng, 'mixed', MIXED_SIZE, {'third': list(range(0, MIXED_SIZE, 3))})
        self.twice = [self._add_family(rng, 'twice', size, {'even': list(range(0, size, 2))}) for size in TWICE_SIZES]
        self.other = self._add_family(rng, 'other', 20, {'even': list(range(0, 20, 2))})
        self.ids = [b'L%05d' % i for i in range(len(self.sequences))]
        self.singles = self._single_units(rng)
        self.pairs = self._pair_units(rng)
        # long-list and short-list units alternate: a wave's lanes then hold lists of every form at once
        rng.shuffle(self.singles)
        rng.shuffle(self.pairs)

    # ------------------------------------------------------------------ transcripts
    def _add_family(self, rng, kind, size, patterns):
        family = Family(kind, len(self.sequences), size, patterns)
        members = [[_random_bases(rng, OWN)] for _ in range(size)]
        for name, chosen in patterns.items():
            core, seg = _random_bases(rng, CORE), _random_bases(rng, SEG)
            family.core[name], family.seg[name] = core, seg
            inside = set(chosen)
            for m in range(size):
                block = core + (seg if m in inside else _random_bases(rng, SEG))
                if kind == 'mixed' and m % 2 == 1:
                    block = reverse_complement(block)
                members[m] += [block, _random_bases(rng, OWN)]
                if kind == 'twice':                     # the core a second time, nothing shared behind it
                    members[m] += [core, _random_bases(rng, OWN)]
        self.sequences += [b''.join(parts) for parts in members]
        self.families.append(family)
        return family

    def pooled(self):
        """(ids, pool, tx_offsets) as index_builder.build_pooled takes them."""
        offsets = np.zeros(len(self.sequences) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.sequences], out=offsets[1:])
        pool = np.frombuffer(b''.join(self.sequences) + b'\0', dtype=np.uint8).copy()
        return self.ids, pool, offsets

    # ------------------------------------------------------------------------ reads
    def _single_units(self, rng):
        units = []
        for family in self.families:
            if family.kind == 'other':
                continue
            copies = 2 if family.kind == 'twice' else 1
            for name, chosen in family.patterns.items():
                block = family.core[name] + family.seg[name]
                whole, part = family.ids(), family.ids(chosen)
                for windows, targets, listed in ((WHOLE_WINDOWS, whole, copies * len(whole)),
                                                 (PATTERN_WINDOWS, part, len(part))):
                    for lo, hi in windows:
                        read = block[lo:hi]
                        units.append(Unit([read], family, name, targets, listed, 'forward'))
                        units.append(Unit([reverse_complement(read)], family, name, targets, listed, 'reverse'))
        # reads that belong nowhere: chimeras of two unrelated cores, and Ns inside a core
        a, b = self.families[len(SIZES) - 1], self.other        # the family of 300 and the unrelated one
        for name in ('first', 'even', 'hi_64'):
            chimera = a.core[name][:50] + b.core['even'][20:70]
            for read in (chimera, reverse_complement(chimera), b.core['even'][20:70] + a.core[name][:50]):
                units.append(Unit([read], a, name, None, note='chimera'))
        core = bytearray(a.core['lo_128'])
        core[40:45] = b'NNNNN'
        units.append(Unit([bytes(core)], a, 'lo_128', None, note='Ns'))
        units.append(Unit([reverse_complement(bytes(core))], a, 'lo_128', None, note='Ns'))
        return units

    def _pair_units(self, rng):
        units = []
        for family in self.families:
            if family.kind == 'other':
                continue
            for name, chosen in family.patterns.items():
                block = family.core[name] + family.seg[name]
                part = family.ids(chosen)
                for (lo1, hi1), (lo2, hi2) in PAIR_WINDOWS:
                    mate1, mate2 = block[lo1:hi1], reverse_complement(block[lo2:hi2])
                    # both orders: the intersection sees the long list on either side
                    units.append(Unit([mate1, mate2], family, name, part, note='long list first'))
                    units.append(Unit([mate2, mate1], family, name, part, note='long list second'))
        # mates of different families have no transcript in common
        b = self.other
        for family in self.families[len(SIZES) - 4:len(SIZES)]:
            mate1, mate2 = family.core['even'][0:70], reverse_complement(b.core['even'][10:80])
            units.append(Unit([mate1, mate2], family, 'even', (), note='mates of two families'))
            units.append(Unit([mate2, mate1], family, 'even', (), note='mates of two families'))
        return units

    def whole_list_units(self, size, n_units, seed):
        """`n_units` single-ended units that each keep the whole list of the sized family of `size`
        members: windows of 40 to 80 bases inside its cores, either strand."""
        rng = np.random.default_rng(seed)
        family = self.families[SIZES.index(size)]
        names = list(family.patterns)
        units = []
        for _ in range(n_units):
            name = names[int(rng.integers(len(names)))]
            lo = int(rng.integers(0, 41))
            hi = int(rng.integers(lo + 40, CORE + 1))
            read = family.core[name][lo:hi]
            if rng.integers(2):
                read = reverse_complement(read)
            units.append(Unit([read], family, name, family.ids()))
        return units


_made = {}


def fixture(seed=SEED):
    """The fixture of `seed`, made once per process (read-only by convention)."""
    if seed not in _made:
        _made[seed] = Fixture(seed)
    return _made[seed]


def wanted_entries(unit):
    """The transcripts of the unit's final list, ascending, each as often as the list holds it."""
    if not unit.targets:
        return ()
    return tuple(sorted(unit.targets * (unit.listed // len(unit.targets))))


def reads_of(units):
    """The reads of `units`, back to back (the mates of a pair adjacent)."""
    return [read for unit in units for read in unit.reads]


def check_list_positions(fixture, contigs, targets):
    """On a built index: every slice ascends by signed entry; every family's core contigs list the
    family's members with one sign (a contig stored in the transcripts' orientation lists member m at
    position m, one stored reverse complemented lists ~m descending, and a read of the other strand
    mirrors either), a 'twice' family's each member twice.  Returns the set of target_count values."""
    counts = contigs['target_count']
    starts = contigs['target_offset']
    entries = targets[targets.dtype.names[0]].astype(np.int64)
    lists = {}
    for c in range(counts.size):
        n, a = int(counts[c]), int(starts[c])
        got = entries[a:a + n]
        assert (np.diff(got) >= 0).all(), c
        plain = np.where(got < 0, ~got, got)
        lists.setdefault((int(plain.min()), n), []).append(got)
    for family in fixture.families:
        if family.kind in ('mixed', 'other'):
            continue
        copies = 2 if family.kind == 'twice' else 1
        want = np.repeat(np.asarray(family.ids(), dtype=np.int64), copies)
        found = lists.get((family.first_id, copies * family.size), [])
        # one contig per core at the least (the one transcript of a family of one is one contig)
        assert len(found) >= (len(family.patterns) if family.size > 1 else 1), (family.kind, family.size, len(found))
        for got in found:
            assert (got >= 0).all() or (got < 0).all()
            np.testing.assert_array_equal(got if got[0] >= 0 else (~got)[::-1], want)
    return set(int(n) for n in counts)
