"""The lookups the junction words and the mapper are built from, asked one k-mer at a time (skm_index_probe) and
compared with a plain dictionary of the stored k-mers (tests/junction_reference.py): map_kmer over the reference's
layout, the bucket table's chain with and without the home bucket's positions fetched up front, and the signature
table that must turn away no k-mer of the table.  And the first-hit roll of the map kernel, whose windows of
minimizer hashes are written differently from kmer_min_hash, with reads made to stop it at every position."""
import numpy as np
import pytest

import junction_reference as jr
from conftest import make_product_index
from test_gpu_parity import _compare_units, _run_gpu

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


def _bucket_hash(canonical):
    """skm_device.h: bucket_hash -- used here to CHOOSE inputs only; what a lookup must return comes from the dict."""
    h = ((canonical & M32) * 0x9E3779B1) & M32
    h = ((h ^ (h >> 16)) + (((canonical >> 32) & M32) * 0x85EBCA77)) & M32
    return (h * 0xC2B2AE3D) & M32


def _substitutions(kmers):
    """Every k-mer one base away from each of `kmers`: 75 a k-mer."""
    kmers = np.asarray(kmers, dtype=np.uint64)
    out = [kmers ^ (np.uint64(d) << np.uint64(2 * at)) for at in range(jr.K) for d in (1, 2, 3)]
    return np.concatenate(out)


def _check_modes(index, ix, queries, modes=(0, 1, 2), expected=None):
    found, entry, offset = expected or ix.map_kmers(queries)
    for mode in modes:
        got_entry, got_offset = index.device_probe(mode, queries)
        wrong = np.flatnonzero((got_entry != entry) | (got_offset != offset))
        assert wrong.size == 0, ('mode %d: %d of %d queries differ; first: k-mer %#x gives (%d, %d), the dict (%d, %d)'
                                 % (mode, wrong.size, queries.size, int(queries[wrong[0]]), got_entry[wrong[0]],
                                    got_offset[wrong[0]], entry[wrong[0]], offset[wrong[0]]))
    return found


@pytest.fixture(scope='module')
def world(oracle, native_libs, chr21_oracle_index, chr21):
    ix = jr.from_arrays(chr21_oracle_index)
    index = make_product_index(chr21_oracle_index, chr21[0])
    rng = np.random.default_rng(5)
    stored = ix.stored_kmers
    some = stored[rng.choice(stored.size, 20000, replace=False)]
    queries = np.concatenate([stored, jr.reverse_complements(stored), _substitutions(some),
                              rng.integers(0, 1 << 50, 200000, dtype=np.uint64)])
    expected = ix.map_kmers(queries)                # (once: four million bisections)
    for array in (queries,) + expected:
        array.setflags(write=False)
    return ix, index, queries, expected


def test_the_three_lookups_equal_the_dict(world):
    ix, index, queries, expected = world
    info = index.device_info()
    assert info['bucketed'] == 1 and info['bucket_kmers'] == ix.stored_kmers.size == 1155426
    found = _check_modes(index, ix, queries, expected=expected)
    n = ix.stored_kmers.size
    assert found[:2 * n].all() and 0.5 < (~found[2 * n:]).mean() < 1.0
    # (k-mers stored without a position, offset < 0: a built index has none; the tampered tables of
    # test_gpu_parity.py::test_unassigned_slots_are_misses drive that branch)
    assert (ix.stored_offset >= 0).all()


def test_the_signatures_turn_away_no_stored_kmer(world):
    ix, index, queries, expected = world
    assert index.device_info()['signature_slots'] > 0
    verdict, zero = index.device_probe(3, queries)
    assert set(np.unique(verdict).tolist()) <= {0, 1} and (zero == 0).all()
    found = expected[0]
    assert (verdict[found] == 1).all(), '%d stored k-mers turned away' % int((verdict[found] == 0).sum())
    absent = ~found
    n = ix.stored_kmers.size
    neighbours = slice(2 * n, 2 * n + 75 * 20000)
    print('signatures turn away %.1f %% of %d absent queries (%.1f %% of the one-base neighbours of stored k-mers, '
          '%.1f %% of the random ones)'
          % (100.0 * (verdict[absent] == 0).mean(), int(absent.sum()),
             100.0 * (verdict[neighbours][absent[neighbours]] == 0).mean(),
             100.0 * (verdict[2 * n + 75 * 20000:][absent[2 * n + 75 * 20000:]] == 0).mean()))
    assert (verdict[absent] == 0).any()


def test_what_a_mode_needs_must_be_there(world, native_libs, chr21_oracle_index, monkeypatch):
    ix, index, queries, _ = world
    few = queries[:1000]
    with pytest.raises(ValueError):
        index.device_probe(4, few)
    with pytest.raises(ValueError):
        index.device_probe(0, np.array([1 << 50], dtype=np.uint64))
    monkeypatch.setenv('SKM_NO_SIGNATURES', '1')
    plain = make_product_index(chr21_oracle_index)
    with pytest.raises(native_libs.NativeError) as refused:
        plain.device_probe(3, few)
    assert refused.value.code == native_libs.SKM_ERR_STATE
    _check_modes(plain, ix, few)
    monkeypatch.setenv('SKM_NO_BUCKETS', '1')
    bare = make_product_index(chr21_oracle_index)
    for mode in (1, 2, 3):
        with pytest.raises(native_libs.NativeError) as refused:
            bare.device_probe(mode, few)
        assert refused.value.code == native_libs.SKM_ERR_STATE
    _check_modes(bare, ix, few, modes=(0,))
    assert bare.device_probe(0, few[:0])[0].size == 0


def test_a_chain_that_wraps_from_the_last_bucket_to_the_first(oracle, native_libs):
    """A table of 16 buckets of which the last is the home of five k-mers or more: the fifth is placed in bucket 0."""
    for attempt in range(20000):
        transcript = bytes(np.random.default_rng(attempt).choice(np.frombuffer(b'ACGT', dtype=np.uint8), 40))
        kmers = jr.kmers_of(transcript)
        canonical = np.minimum(kmers, jr.reverse_complements(kmers))
        if sum(_bucket_hash(int(k)) >> 28 == 15 for k in canonical.tolist()) >= 5 and np.unique(canonical).size == 16:
            break
    else:
        raise AssertionError('no such transcript')
    oindex = oracle.build_index([transcript])
    ix = jr.from_arrays(oindex)
    assert ix.stored_kmers.size <= 16
    index = make_product_index(oindex)
    info = index.device_info()
    assert info['bucketed'] == 1 and info['buckets'] == 16 and info['bucket_overflowed'] > 0
    stored = ix.stored_kmers
    queries = np.concatenate([stored, jr.reverse_complements(stored), _substitutions(stored),
                              _substitutions(jr.reverse_complements(stored))])
    found = _check_modes(index, ix, queries)
    assert found[:2 * stored.size].all()
    verdict, _ = index.device_probe(3, queries)
    assert (verdict[found] == 1).all()


class Roll:
    """For every first-hit position e in 1..48: 20 windows of 100 bases of chr21 with a substitution at e - 1 (and
    at e - 26 when e > 25), so that by the dict k-mers 0..e-1 are not in the table and k-mer e is; each read and
    its reverse complement."""

    def __init__(self, oracle, ix, oindex, transcripts):
        rng = np.random.default_rng(48)
        long_tx = [s for s in transcripts if len(s) > 300]
        self.reads, self.first_hit = [], []
        for e in range(1, 49):
            made = 0
            for _ in range(2000):
                if made == 20:
                    break
                t = long_tx[int(rng.integers(len(long_tx)))]
                at = int(rng.integers(0, len(t) - 100))
                read = bytearray(t[at:at + 100].upper())
                for spot in ([e - 1, e - 26] if e > 25 else [e - 1]):
                    if bytes(read[spot:spot + 1]) not in (b'A', b'C', b'G', b'T'):
                        break
                    read[spot] = b'ACGT'[(b'ACGT'.index(bytes(read[spot:spot + 1])) + 1 + int(rng.integers(3))) % 4]
                else:
                    hit = ix.map_kmers(jr.kmers_of(bytes(read))[:e + 1])[0]
                    if not hit[:e].any() and hit[e]:
                        self.reads += [bytes(read), jr.reverse_complement_bases(read)]
                        self.first_hit += [e, -1]
                        made += 1
            assert made == 20, e
        assert len(self.reads) == 1920
        self.bases, self.offsets = oracle.pack_reads(self.reads)
        self.expected = oracle.map_batch(oindex, self.bases, self.offsets, len(self.reads), False,
                                         np.zeros(2000, dtype=np.int64))
        # (the oracle's first hit is where the dict says: it only ever moves `begin` to the left of it)
        first_hit = np.asarray(self.first_hit)
        forward = first_hit > 0
        assert (self.expected.begin[forward] <= first_hit[forward]).all() and (self.expected.count[forward] > 0).mean() > 0.9


@pytest.fixture(scope='module')
def roll(oracle, world, chr21_oracle_index, chr21):
    return Roll(oracle, world[0], chr21_oracle_index, chr21[1])


@pytest.mark.parametrize('signatures', [True, False])
def test_the_roll_stops_where_the_dict_says(roll, chr21_oracle_index, signatures, monkeypatch):
    if not signatures:
        monkeypatch.setenv('SKM_NO_SIGNATURES', '1')
    index = make_product_index(chr21_oracle_index)
    assert (index.device_info()['signature_slots'] > 0) == signatures
    _, units = _run_gpu(index, roll.bases, roll.offsets, len(roll.reads), False)
    _compare_units(roll.expected, units)
