"""The generators behind test_gpu_class_table.py, checked where there is no GPU: the oracles of the
GPU tests are plain numpy and Python, and a wrong one would pin the kernels to the wrong answer."""
import numpy as np

import class_table_reference as ref


def test_the_restated_key_is_the_documented_one():
    """The worked example of the collision construction: two different tuples, one key."""
    assert ref.tuple_key((0x47e8f50a, 0x1e240)) == 0x2d4557f8a4f7a985
    assert ref.tuple_key((0x9491d02b, 0x0df6e035)) == 0x2d4557f8a4f7a985
    # the vectorised form agrees with the scalar one
    keys = ref.single_id_keys(1000)
    assert [int(k) for k in keys] == [ref.tuple_key((i,)) for i in range(1000)]
    # the length is part of the key: (x,) and (x, x) and a prefix differ
    assert len({ref.tuple_key(t) for t in [(5,), (5, 5), (5, 5, 5), (5, 6), (6, 5)]}) == 5


def test_collision_pairs_differ_and_share_a_key():
    pairs = ref.collision_pairs(8)
    assert len(pairs) == 8
    for one, two in pairs:
        assert one != two and len(one) == len(two) == 2
        assert all(0 <= i < (1 << 32) for i in one + two)
        assert ref.tuple_key(one) == ref.tuple_key(two)
        # one id of every pair has its top bit set: no such tuple can come from mapped reads
        assert max(one + two) >= (1 << 31)
        for i in one + two:
            assert np.int32(ref.as_int32(i)).astype(np.uint32) == i
    assert len({ref.tuple_key(one) for one, _ in pairs}) == 8
    assert pairs == ref.collision_pairs(8)          # a fixed seed


def test_the_chain_shares_one_home_slot():
    chain = ref.probe_chain()
    assert len(chain) == 300
    keys = [ref.tuple_key(t) for t in chain.tuples]
    assert len(set(keys)) == 300 and len(set(chain.tuples)) == 300
    assert len({k & 0xffff for k in keys}) == 1
    assert all(len(t) == 1 and 0 <= t[0] < (1 << 25) for t in chain.tuples)
    assert np.unique(chain.first_seen).size == 300


def test_merge_classes_never_tie_and_hold_what_they_promise():
    a, b, one, none = ref.merge_classes()
    assert (len(a), len(b), len(one), len(none)) == (40000, 100000, 1, 0)
    chain = ref.probe_chain()
    every = np.concatenate([s.first_seen for s in (a, b, one, chain)])
    assert np.unique(every).size == every.size and every.min() >= 0
    for s in (a, b, one):
        assert len(set(s.tuples)) == len(s)         # a merge call's classes are distinct
        assert s.counts.min() >= 1
        assert s.targets.min() >= 0                 # ids in [0, 2^31)
        assert {len(t) for t in s.tuples} <= set(ref.TUPLE_LENGTHS) | {1, 2, 3, 6, 32, 63, 64, 150, 299}
    assert {len(t) for t in a.tuples} >= set(ref.TUPLE_LENGTHS)
    assert {len(t) for t in b.tuples} >= set(ref.TUPLE_LENGTHS)
    in_a = {t: k for k, t in enumerate(a.tuples)}
    again = [(in_a[t], k) for k, t in enumerate(b.tuples) if t in in_a]
    assert len(again) == len(a)                     # every tuple of A comes again in B ...
    ka, kb = (np.asarray(v) for v in zip(*again))
    assert (a.counts[ka] != b.counts[kb]).mean() > 0.99           # ... with another count
    below = b.first_seen[kb] < a.first_seen[ka]
    assert 0.3 < below.mean() < 0.7                 # first-seen values below and above A's
    assert one.tuples[0] not in in_a and one.tuples[0] not in set(b.tuples)
    assert not set(chain.tuples) & (set(a.tuples) | set(b.tuples))
    assert none.unaligned > 0 and none.fld.sum() > 0
    # the near-misses are there: prefixes, reorderings, (x,) against (x, x)
    union = set(a.tuples) | set(b.tuples) | set(one.tuples)
    assert sum(1 for t in union if len(t) > 1 and t[:-1] in union) >= 100
    assert sum(1 for t in union if len(t) > 1 and t[::-1] != t and t[::-1] in union) >= 100
    assert sum(1 for t in union if len(t) == 1 and t * 2 in union) >= 100
    # all keys differ (the constructed collisions are a set of their own)
    keys = {ref.tuple_key(t) for t in list(union)[:20000]}
    assert len(keys) == 20000


def test_the_counter_reference_is_a_counter():
    a = ref.ClassSet([(1, 2), (3,), (2, 1)], [5, 7, 11], [30, 10, 20], unaligned=2)
    b = ref.ClassSet([(3,), (3, 3)], [100, 1], [40, 5], unaligned=1, fld=np.arange(2000))
    held = ref.CounterReference().merge(a).merge(b)
    assert held.sizes() == (4, 7, 3, 5 + 7 + 11 + 100 + 1 + 3)
    offsets, targets, counts, first, fld = held.export()
    np.testing.assert_array_equal(offsets, [0, 2, 3, 5, 7])
    np.testing.assert_array_equal(targets, [3, 3, 3, 2, 1, 1, 2])
    np.testing.assert_array_equal(counts, [1, 107, 11, 5])
    np.testing.assert_array_equal(first, [5, 10, 20, 30])
    np.testing.assert_array_equal(fld, np.arange(2000))
    empty = ref.ClassSet([], [], [], unaligned=4)
    assert empty.offsets.tolist() == [0] and empty.targets.size == 0
    assert ref.CounterReference().merge(empty).sizes() == (0, 0, 4, 4)
