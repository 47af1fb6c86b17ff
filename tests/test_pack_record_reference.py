"""tests/pack_record_reference.py against the host packer (skm_pack_reads) on the inputs of
tests/test_gpu_pack_records.py: the code words are equal, and so are the bases that are not upper-case
ACGT.  The host packer states the latter as the mask rows of its exception reads, in which a SET bit
means "upper-case ACGT", exactly as in the record's flag words (include/seekmer_hip.h: skm_packed_reads);
a read without an exception entry has all of its bases flagged.  So the reference is pinned without a GPU."""
import ctypes

import numpy as np
import pytest

import pack_record_reference as ref


def _host_pack(native_libs, bases, offsets):
    """(codes uint64[n][cw], lengths, flags uint32[n][cw]) of skm_pack_reads"""
    n = offsets.size - 1
    longest = int(np.diff(offsets).max()) if n else 0
    cw = max(1, (longest + 31) // 32)
    codes = np.zeros((n, cw), dtype=np.uint64)
    lengths = np.zeros(n, dtype=np.uint32)
    exc_reads = np.zeros(n + 1, dtype=np.uint32)
    exc_masks = np.zeros((n + 1, cw), dtype=np.uint32)
    n_exc = ctypes.c_int64()
    held = np.ascontiguousarray(bases) if bases.size else np.zeros(1, dtype=np.uint8)
    code = native_libs.host().skm_pack_reads(held.ctypes.data, native_libs.ptr(offsets, native_libs.c_i64p), n, cw,
                                             codes.ctypes.data, lengths.ctypes.data, exc_reads.ctypes.data,
                                             exc_masks.ctypes.data, n + 1, ctypes.byref(n_exc), -1)
    assert code == 0
    at = np.arange(32 * cw).reshape(cw, 32)
    flags = np.zeros((n, cw), dtype=np.uint32)
    for r in range(n):                                    # no exception entry: every base of the read is flagged
        inside = (at < int(lengths[r])).astype(np.uint64)
        flags[r] = (inside << (31 - (at & 31)).astype(np.uint64)).sum(axis=1).astype(np.uint32)
    listed = exc_reads[:n_exc.value]
    assert np.all(np.diff(listed.astype(np.int64)) > 0)
    flags[listed] = exc_masks[:n_exc.value]
    return codes, lengths, flags, set(int(r) for r in listed)


def _check(native_libs, bases, offsets):
    want = ref.records(bases, offsets)
    n = offsets.size - 1
    words = ref.words_per_read(int(np.diff(offsets).max()) if n else 0)
    assert want.shape == (n, ref.record_words(words)) and want.shape[1] % 16 == 0
    codes, lengths, flags, listed = _host_pack(native_libs, bases, offsets)
    cw = codes.shape[1]
    assert cw in (words - 1, words)                      # (a batch of empty reads: the packer takes one word at the least)
    np.testing.assert_array_equal(ref.code_words_of(want, words)[:, :cw], codes)
    np.testing.assert_array_equal(ref.flag_words_of(want, words)[:, :cw], flags)
    np.testing.assert_array_equal(~ref.flag_words_of(want, words)[:, :cw], ~flags)      # the exceptions themselves
    np.testing.assert_array_equal(want[:, 3 * words], lengths)
    # the pad word, and everything behind the length, is zero
    if cw < words:
        assert not ref.code_words_of(want, words)[:, cw:].any() and not ref.flag_words_of(want, words)[:, cw:].any()
    assert not want[:, 3 * words + 1:].any()
    # a read is an exception of the packer exactly when the reference leaves one of its bases unflagged
    full = np.array([bin(int(v)).count('1') for v in ref.flag_words_of(want, words).reshape(-1)]).reshape(n, words).sum(axis=1)
    assert listed == set(int(r) for r in np.flatnonzero(full != np.diff(offsets)))


@pytest.mark.parametrize('name,lengths', list(ref.length_cases()), ids=[c[0] for c in ref.length_cases()])
def test_reference_equals_the_host_packer_by_length(native_libs, name, lengths):
    _check(native_libs, *ref.batch_of(lengths, seed=len(lengths) + sum(lengths)))


@pytest.mark.parametrize('length', [100, 150, 250])
def test_reference_equals_the_host_packer_around_the_block(native_libs, length):
    reads = ctypes.c_int32()
    assert native_libs.hip().skm_pack_stage_reads(ref.words_per_read(length), ctypes.byref(reads)) == 0
    assert 16 <= reads.value <= 128
    for name, lengths in ref.block_cases(reads.value, length):
        _check(native_libs, *ref.batch_of(lengths, seed=len(lengths)))


def test_the_fallback_case_is_beyond_the_stage(native_libs):
    reads = ctypes.c_int32(-1)
    hip = native_libs.hip()
    assert hip.skm_pack_stage_reads(ref.words_per_read(ref.FALLBACK_LENGTH), ctypes.byref(reads)) == 0
    assert reads.value == 0
    assert hip.skm_pack_stage_reads(ref.words_per_read(250), ctypes.byref(reads)) == 0 and reads.value > 0
    assert hip.skm_pack_stage_reads(0, ctypes.byref(reads)) == native_libs.SKM_ERR_ARG


@pytest.mark.parametrize('byte', ref.ODD_BYTES, ids=[repr(b) for b in ref.ODD_BYTES])
def test_reference_equals_the_host_packer_on_odd_bytes(native_libs, byte):
    bases, offsets = ref.odd_byte_batch(byte)
    _check(native_libs, bases, offsets)
    want = ref.records(bases, offsets)
    words = ref.words_per_read(100)
    for r in (0, 20, 39):                                 # the byte is where it was put, unflagged, in the record
        length = int(offsets[r + 1] - offsets[r])
        for p in (0, 15, 16, 31, 32, length - 1):
            assert not (int(want[r, 2 * words + (p >> 5)]) >> (31 - (p & 31))) & 1
            code = (int(ref.code_words_of(want[r:r + 1], words)[0, p >> 5]) >> (62 - 2 * (p & 31))) & 3
            assert code == (b'ACGT'.index(byte.upper()) if byte.upper() in b'ACGT' else 0)


def test_benchmark_shape(native_libs):
    """3000 pairs of 2 x 100 bases, one base in a hundred damaged"""
    rng = np.random.default_rng(11)
    bases, offsets = ref.random_reads(rng, [100] * 6000)
    _check(native_libs, ref.damage(bases, rng, 0.01), offsets)
