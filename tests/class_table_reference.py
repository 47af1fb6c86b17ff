"""Plain numpy / Python oracles for the class table tests (test_gpu_class_table.py): the 64-bit
tuple key restated in Python integers, synthetic class sets with a dict as the Counter they must
merge into, one long probe chain, and constructed pairs of different tuples that share a key.
Nothing here touches the GPU; test_class_table_host.py checks the generators themselves."""
import itertools

import numpy as np

MASK64 = (1 << 64) - 1
KEY_MULTIPLIER = 0x9E3779B97F4A7C15
KEY_SEED = 0x243F6A8885A308D3
MAX_FRAGMENT_LENGTH = 2000
TUPLE_LENGTHS = (1, 2, 3, 7, 64, 65, 300)
# (short tuples are the common ones, as in a real table; every length is drawn thousands of times)
TUPLE_LENGTH_WEIGHTS = (0.30, 0.25, 0.20, 0.15, 0.04, 0.04, 0.02)


def tuple_key_seed(n):
    return KEY_SEED ^ n


def tuple_key_step(h, unsigned_id):
    h ^= unsigned_id
    h = (h * KEY_MULTIPLIER) & MASK64
    return h ^ (h >> 32)


def tuple_key(ids):
    """The table's key of an id tuple (skm_kernels.h: tuple_key_seed, tuple_key_step; ids as the
    unsigned 32-bit values the kernels hash; a key of 0 is stored as 1)."""
    h = tuple_key_seed(len(ids))
    for i in ids:
        h = tuple_key_step(h, int(i) & 0xffffffff)
    return h or 1


def single_id_keys(n):
    """tuple_key((i,)) for every i < n, in numpy (uint64 arithmetic wraps as the kernels' does)."""
    h = np.arange(n, dtype=np.uint64) ^ np.uint64(tuple_key_seed(1))
    h *= np.uint64(KEY_MULTIPLIER)
    h ^= h >> np.uint64(32)
    h[h == 0] = 1
    return h


def as_int32(unsigned_id):
    """An id with its top bit set goes through the int32 arrays of the C ABI as the negative number
    with the same 32 bits."""
    return unsigned_id - (1 << 32) if unsigned_id >= (1 << 31) else unsigned_id


class ClassSet:
    """Classes as skm_mapper_merge takes them: CSR offsets, int32 ids, counts, first-seen values, and
    the totals that travel with them."""

    def __init__(self, tuples, counts, first_seen, unaligned=0, fld=None):
        self.tuples = list(tuples)
        self.counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        self.first_seen = np.asarray(first_seen, dtype=np.int64).reshape(-1)
        assert len(self.tuples) == self.counts.size == self.first_seen.size
        self.unaligned = int(unaligned)
        self.fld = np.zeros(MAX_FRAGMENT_LENGTH, dtype=np.int64) if fld is None else np.asarray(fld, dtype=np.int64)
        self.offsets = np.zeros(len(self.tuples) + 1, dtype=np.int64)
        np.cumsum(np.asarray([len(t) for t in self.tuples], dtype=np.int64), out=self.offsets[1:])
        self.targets = np.fromiter(itertools.chain.from_iterable(self.tuples), dtype=np.int64,
                                   count=int(self.offsets[-1])).astype(np.int32)

    def __len__(self):
        return len(self.tuples)

    def head(self, n):
        """The first n classes as a set of their own (same totals)."""
        return ClassSet(self.tuples[:n], self.counts[:n], self.first_seen[:n], self.unaligned, self.fld)

    def merge_into(self, map_result):
        map_result.merge_table(self.offsets, self.targets, self.counts, self.first_seen, self.unaligned, self.fld)


class CounterReference:
    """What a table must hold after merges: dict tuple -> [sum of counts, min first_seen], with the
    sums of unaligned, units and the histogram; listed by first-seen as skm_mapper_export lists."""

    def __init__(self):
        self.classes = {}
        self.unaligned = 0
        self.units = 0
        self.fld = np.zeros(MAX_FRAGMENT_LENGTH, dtype=np.int64)

    def merge(self, class_set):
        for t, count, first in zip(class_set.tuples, class_set.counts.tolist(), class_set.first_seen.tolist()):
            held = self.classes.get(t)
            if held is None:
                self.classes[t] = [count, first]
            else:
                held[0] += count
                held[1] = min(held[1], first)
        self.unaligned += class_set.unaligned
        self.units += class_set.unaligned + int(class_set.counts.sum())
        self.fld = self.fld + class_set.fld
        return self

    def sizes(self):
        return (len(self.classes), sum(len(t) for t in self.classes), self.unaligned, self.units)

    def export(self):
        """(class_offsets, class_targets, class_counts, first_seen, fld) as MapResult.export()."""
        listed = sorted(self.classes.items(), key=lambda item: item[1][1])
        firsts = [value[1] for _, value in listed]
        assert len(set(firsts)) == len(firsts), 'tied first-seen values: the export order is not defined'
        made = ClassSet([t for t, _ in listed], [value[0] for _, value in listed], firsts)
        return made.offsets, made.targets, made.counts, made.first_seen, self.fld


def _random_fld(rng):
    fld = rng.integers(0, 50, MAX_FRAGMENT_LENGTH).astype(np.int64)
    fld[0] = 0
    return fld


def merge_classes(seed=20250607, n_a=40000, n_b=100000):
    """The class sets of the merge tests: A (n_a classes), B (n_b classes: every tuple of A again with
    another count -- as many tuples of A as a set of distinct tuples can repeat -- and new tuples for
    the rest), one single class, and a set without classes that carries only unaligned units and a
    histogram.  Ids lie in [0, 2^31), tuple lengths come from TUPLE_LENGTHS.  Deliberate near-misses:
    tuples and their proper prefixes, the same ids in another order, (x,) next to (x, x).  All
    first-seen values are cut from ONE permutation, so no two entries ever share one, whichever sets
    they are in."""
    rng = np.random.default_rng(seed)
    seen = set()
    tuples = []

    def take(t):
        if t in seen or not t:
            return False
        seen.add(t)
        tuples.append(t)
        return True

    # near-misses first (they are spread over A and B by the shuffle below)
    for _ in range(200):
        x = int(rng.integers(0, 1 << 31))
        take((x,))
        take((x, x))
        take((x, x, x))
    for n in (2, 3, 7, 64, 65, 300):
        for _ in range(40):
            base = tuple(int(v) for v in rng.integers(0, 1 << 31, n))
            take(base)
            take(base[:-1])                                   # a proper prefix
            take(base[::-1])                                  # the same ids in another order
            take(base[1:] + base[:1])
            if n > 2:
                take(base[:n // 2])
    lengths = rng.choice(TUPLE_LENGTHS, size=n_b + 1, p=TUPLE_LENGTH_WEIGHTS)   # (more than needed)
    for n in lengths.tolist():
        if len(tuples) == n_b + 1:
            break
        take(tuple(rng.integers(0, 1 << 31, n).tolist()))
    assert len(tuples) == n_b + 1
    order = rng.permutation(n_b + 1)
    tuples = [tuples[k] for k in order.tolist()]
    single, tuples = tuples[0], tuples[1:]
    a_tuples = tuples[:n_a]
    b_order = rng.permutation(n_b)
    b_tuples = [tuples[k] for k in b_order.tolist()]                  # A's tuples scattered among the new ones
    first = rng.permutation(4 * (n_a + n_b + 1))                      # one global permutation
    a = ClassSet(a_tuples, rng.integers(1, 1000, n_a), first[:n_a], int(rng.integers(1, 1000)), _random_fld(rng))
    b = ClassSet(b_tuples, rng.integers(1, 1000, n_b), first[n_a:n_a + n_b], int(rng.integers(1, 1000)),
                 _random_fld(rng))
    one = ClassSet([single], [int(rng.integers(1, 1000))], first[n_a + n_b:n_a + n_b + 1], 0, _random_fld(rng))
    none = ClassSet([], [], [], int(rng.integers(1, 1000)), _random_fld(rng))
    return a, b, one, none


def probe_chain(n=300, id_bound=1 << 25, slots_log2=16, first_seen_base=1 << 20):
    """n single-id tuples whose keys share their low `slots_log2` bits: one home slot in a table of
    2^slots_log2 slots, i.e. one probe chain of n.  The ids are the n smallest of the fullest home
    slot among the ids below id_bound.  First-seen values start at first_seen_base, above every value
    of merge_classes()."""
    keys = single_id_keys(id_bound)
    home = (keys & np.uint64((1 << slots_log2) - 1)).astype(np.int64)
    fullest = int(np.bincount(home, minlength=1 << slots_log2).argmax())
    ids = np.flatnonzero(home == fullest)[:n]
    assert ids.size == n, 'no home slot with %d ids below %d' % (n, id_bound)
    rng = np.random.default_rng(300)
    return ClassSet([(int(i),) for i in ids], rng.integers(1, 1000, n), first_seen_base + rng.permutation(n))


COLLISION_DELTA = 2971215073            # a Fibonacci number: DELTA * KEY_MULTIPLIER = -50920843 (mod 2^64)


def collision_pairs(n=4, seed=11):
    """n pairs of DIFFERENT two-id tuples with the SAME 64-bit key, ids as unsigned 32-bit numbers.

    The state after the first id is (seed(2) ^ a) * M folded by h ^= h >> 32.  With a = u ^ s and
    a' = (u - DELTA) ^ s (s = low word of seed(2)) the two products differ by DELTA * M = -50920843
    (mod 2^64), so for most u they share their high word, and the fold leaves the two states
    different in the low word only: d = state ^ state' fits in 32 bits.  A second id b on one side
    and b ^ d on the other makes the states, and so the keys, equal."""
    assert (COLLISION_DELTA * KEY_MULTIPLIER) & MASK64 == MASK64 + 1 - 50920843
    s = tuple_key_seed(2) & 0xffffffff
    rng = np.random.default_rng(seed)
    pairs = []
    while len(pairs) < n:
        u = int(rng.integers(COLLISION_DELTA, 1 << 32))
        b = int(rng.integers(0, 1 << 31))
        a, a2 = u ^ s, (u - COLLISION_DELTA) ^ s
        d = tuple_key_step(tuple_key_seed(2), a) ^ tuple_key_step(tuple_key_seed(2), a2)
        if d >> 32:
            continue                    # (the high words differ: about one draw in a hundred)
        pairs.append(((a, b), (a2, b ^ d)))
    return pairs
