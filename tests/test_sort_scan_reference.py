"""tests/sort_scan_reference.py, the numpy statement of the scan and the radix sort that tests/test_gpu_scan_sort.py
holds the kernels to, against plain Python at small sizes: itertools.accumulate and sorted() with the masked key.
And the two probe entry points without a GPU: they refuse, they do not fall back."""
import itertools

import numpy as np
import pytest

import sort_scan_reference as ref

SIZES = (0, 1, 2, 63, 64, 300)
WIDTHS = {np.dtype(np.uint32): 32, np.dtype(np.uint64): 64, np.dtype(np.int32): 32}


@pytest.mark.parametrize('n', SIZES)
def test_scan_is_accumulate(n):
    rng = np.random.default_rng(n)
    for values in (rng.integers(0, 1 << 40, n), np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)):
        got = ref.scan(values)
        assert got.dtype == np.int64 and got.shape == (n + 1,)
        assert got.tolist() == [0] + list(itertools.accumulate(int(v) for v in values))


def test_passes_and_masks():
    assert [ref.passes(b) for b in (0, 1, 9, 10, 18, 19, 27, 28, 32, 36, 37, 54, 55, 63, 64)] \
        == [1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 6, 7, 7, 8]
    assert ref.sort_mask(0, 32) == 0x1ff and ref.sort_mask(1, 64) == 0x1ff and ref.sort_mask(9, 32) == 0x1ff
    assert ref.sort_mask(10, 32) == 0x3ffff and ref.sort_mask(18, 32) == 0x3ffff
    assert ref.sort_mask(28, 32) == 0xffffffff and ref.sort_mask(32, 32) == 0xffffffff       # (36 bits, cut at the width)
    assert ref.sort_mask(32, 64) == (1 << 36) - 1 and ref.sort_mask(64, 64) == (1 << 64) - 1


@pytest.mark.parametrize('end_bit', [0, 1, 9, 10, 64])
@pytest.mark.parametrize('dtype', [np.uint32, np.uint64, np.int32])
def test_sort_is_sorted_by_the_masked_key(dtype, end_bit):
    width = WIDTHS[np.dtype(dtype)]                 # (end_bit 64 on a 32-bit key: every pass the key has, the whole key)
    top = 31 if dtype is np.int32 else width
    mask = ref.sort_mask(end_bit, width)
    for n in SIZES:
        rng = np.random.default_rng(n * 100 + end_bit)
        few = rng.integers(0, 3, n)                                             # many ties: the order among them shows
        full = rng.integers(0, 1 << top, n, dtype=np.uint64)                    # bits above the mask set
        above = full & np.uint64(((1 << top) - 1) & ~mask)                      # ... and nothing but ties below it
        for keys in (few.astype(dtype), full.astype(dtype), (above | few.astype(np.uint64)).astype(dtype)):
            vals = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
            order = sorted(range(n), key=lambda i: int(keys[i]) & mask)         # (sorted() is stable)
            got_keys, got_vals = ref.sort_pairs(keys, vals, end_bit, width)
            assert got_keys.dtype == keys.dtype and got_vals.dtype == np.int32
            assert got_keys.tolist() == [int(keys[i]) for i in order]
            assert got_vals.tolist() == [int(vals[i]) for i in order]
        if n == 300 and mask < (1 << top) - 1:                                  # (the last pattern)
            assert np.any(np.diff(got_keys.astype(np.float64)) < 0)             # carried whole: not sorted as numbers


def test_the_probes_refuse_without_a_gpu(native_libs):
    if native_libs.device_count() > 0:
        pytest.skip('a GPU is present')
    hip = native_libs.hip()
    values = np.arange(5, dtype=np.int64)
    out = np.full(6, -7, dtype=np.int64)
    for in_place in (0, 1):
        assert hip.skm_device_scan_probe(0, native_libs.ptr(values, native_libs.c_i64p), 5, in_place,
                                         native_libs.ptr(out, native_libs.c_i64p)) == native_libs.SKM_ERR_NO_DEVICE
    assert b'no HIP device' in hip.skm_last_error()
    # (before every other check: a bad argument is SKM_ERR_NO_DEVICE too, as with skm_units_group)
    assert hip.skm_device_scan_probe(0, None, -1, 0, None) == native_libs.SKM_ERR_NO_DEVICE
    assert (out == -7).all()
    vals = np.arange(5, dtype=np.int32)
    vals_out = np.full(5, -7, dtype=np.int32)
    for kind, dtype in enumerate((np.uint32, np.uint64, np.int32)):
        keys = np.arange(5).astype(dtype)
        keys_out = np.full(5, 7, dtype=dtype)
        assert hip.skm_device_sort_probe(0, kind, keys.ctypes.data, native_libs.ptr(vals, native_libs.c_i32p), 5, 9,
                                         keys_out.ctypes.data, native_libs.ptr(vals_out, native_libs.c_i32p)) \
            == native_libs.SKM_ERR_NO_DEVICE
        assert (keys_out == 7).all() and (vals_out == -7).all()
    assert hip.skm_device_sort_probe(0, 5, None, None, 0, 99, None, None) == native_libs.SKM_ERR_NO_DEVICE
