"""The hand-written prefix sum and stable radix sort of skm_quant_setup.hip (exclusive_scan_with_total, sort_pairs<K>)
run on their own through skm_device_scan_probe / skm_device_sort_probe and held to numpy bit for bit
(tests/sort_scan_reference.py): every size at which a lane, a wave, a tile or the single block over the tile sums
changes its share; the scan in place; partial sums above 2^32; all three key types of the sort at one to eight passes,
both parities of the ping-pong between the scratch arrays and the caller's, shifts up to 63; the carry loop of the
per-digit scan (more than 1024 tiles); key patterns that put a whole tile, or a whole 64-pair chunk, into one digit;
and the order by WHOLE 9-bit passes that localize's 0xffffffff key relies on.  Integers only: no tolerances."""
import numpy as np
import pytest

import sort_scan_reference as ref

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048                    # values per block of the scan
SORT_TILE = 4096                    # pairs per block of the sort
# key_kind of skm_device_sort_probe -> (dtype, width of the key, bits a key may use: int32 keys are non-negative)
KINDS = {0: (np.uint32, 32, 32), 1: (np.uint64, 64, 64), 2: (np.int32, 32, 31)}
END_BITS_32 = (1, 8, 9, 10, 18, 19, 27, 28, 32)
END_BITS_64 = END_BITS_32 + (33, 36, 37, 45, 54, 55, 63, 64)


def _scan(native, values, in_place):
    values = np.ascontiguousarray(values, dtype=np.int64)
    out = np.full(values.size + 1, -12345, dtype=np.int64)
    native.check(native.hip().skm_device_scan_probe(0, native.ptr(values, native.c_i64p), values.size, int(in_place),
                                                    native.ptr(out, native.c_i64p)))
    return out


def _sort(native, kind, keys, vals, end_bit):
    keys = np.ascontiguousarray(keys, dtype=KINDS[kind][0])
    vals = np.ascontiguousarray(vals, dtype=np.int32)
    assert keys.shape == vals.shape
    keys_out = np.full(keys.size, 0x5a5a5a5a, dtype=keys.dtype)
    vals_out = np.full(keys.size, 0x5a5a5a5a, dtype=np.int32)
    native.check(native.hip().skm_device_sort_probe(0, kind, keys.ctypes.data, native.ptr(vals, native.c_i32p), keys.size,
                                                    end_bit, keys_out.ctypes.data, native.ptr(vals_out, native.c_i32p)))
    return keys_out, vals_out


def _check_sort(native, kind, keys, vals, end_bit, what=''):
    keys = np.asarray(keys).astype(KINDS[kind][0])
    want_keys, want_vals = ref.sort_pairs(keys, vals, end_bit, KINDS[kind][1])
    got_keys, got_vals = _sort(native, kind, keys, vals, end_bit)
    note = 'kind %d, n = %d, end_bit %d (%d passes) %s' % (kind, keys.size, end_bit, ref.passes(end_bit), what)
    np.testing.assert_array_equal(got_keys, want_keys, err_msg=note)
    np.testing.assert_array_equal(got_vals, want_vals, err_msg=note)


def _values(rng, n):
    """int32 values with repeats and negatives, nothing like iota: they are carried, not recomputed"""
    return rng.integers(-max(n, 2) // 2, max(n, 2) // 2, n).astype(np.int32)


def _uniform(rng, n, bits):
    if bits >= 64:
        return rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    return rng.integers(0, 1 << bits, n, dtype=np.uint64)


# ---- scan -----------------------------------------------------------------------------------------------------------
SCAN_SIZES = (0, 1, 7, 8, 9,                                    # one lane's eight values
              511, 512, 513,                                    # a wave
              2047, 2048, 2049, 4096, 3 * SCAN_TILE + 5,        # tiles
              1024 * SCAN_TILE, 1024 * SCAN_TILE + 1,           # 1025 tiles: two sums a lane of the block over the sums,
              2048 * SCAN_TILE + 1)                             # the lanes past 513 own nothing; 2049 tiles: three a lane


@pytest.fixture(scope='module')
def scan_cases():
    """n -> (values, their scan), made once and shared by the two ways to run a size"""
    made = {}

    def case(n):
        if n not in made:
            values = np.random.default_rng(1000 + n).integers(0, 1 << 40, n)
            want = ref.scan(values)
            assert n < 4096 or (1 << 32) < want[n] < (1 << 62)
            values.setflags(write=False)
            want.setflags(write=False)
            made[n] = values, want
        return made[n]
    return case


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('n', SCAN_SIZES)
def test_scan_equals_cumsum(native_libs, scan_cases, n, in_place):
    values, want = scan_cases(n)
    got = _scan(native_libs, values, in_place)
    np.testing.assert_array_equal(got, want)
    assert got[n] == int(values.sum(dtype=np.int64))            # out[n] is the total


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('n', [2049, 1024 * SCAN_TILE + 1])
def test_scan_of_zeros_and_of_ones(native_libs, n, in_place):
    np.testing.assert_array_equal(_scan(native_libs, np.zeros(n, dtype=np.int64), in_place), np.zeros(n + 1, dtype=np.int64))
    np.testing.assert_array_equal(_scan(native_libs, np.ones(n, dtype=np.int64), in_place), np.arange(n + 1, dtype=np.int64))


# ---- sort -----------------------------------------------------------------------------------------------------------
SORT_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025,               # a chunk of 64 pairs; a wave's quarter of a tile
              4095, 4096, 4097, 8192, 3 * SORT_TILE + 5)        # tiles
SIZES_AND_PASSES = [(kind, end_bit) for kind in KINDS for end_bit in (END_BITS_64 if kind == 1 else END_BITS_32)
                    if end_bit <= KINDS[kind][2]] + [(2, 31)]


def test_every_pass_count_and_both_parities_are_run():
    assert sorted({ref.passes(b) for k, b in SIZES_AND_PASSES if k == 1}) == [1, 2, 3, 4, 5, 6, 7, 8]
    for kind in (0, 2):
        assert sorted({ref.passes(b) for k, b in SIZES_AND_PASSES if k == kind}) == [1, 2, 3, 4]
    assert max(9 * (ref.passes(b) - 1) for k, b in SIZES_AND_PASSES) == 63           # the last pass's shift


@pytest.mark.parametrize('kind,end_bit', SIZES_AND_PASSES)
def test_sort_sizes_and_pass_counts(native_libs, kind, end_bit):
    for n in SORT_SIZES:
        rng = np.random.default_rng((kind * 100 + end_bit) * 100000 + n)
        _check_sort(native_libs, kind, _uniform(rng, n, end_bit), _values(rng, n), end_bit)


PATTERN_END_BITS = {0: (9, 18, 27, 32), 1: (9, 18, 27, 36, 45, 64), 2: (9, 18, 27, 31)}


def _pattern(name, rng, n, kind, end_bit):
    """keys of the named pattern as uint64, or None where the pattern does not exist at this end_bit"""
    i = np.arange(n, dtype=np.uint64)
    top = KINDS[kind][2]
    if name == 'uniform':
        return _uniform(rng, n, end_bit)
    if name == 'three keys':        # stability across lanes, chunks, waves and tiles (distinct: their low two bits are)
        three = _uniform(np.random.default_rng(end_bit), 3, end_bit) & ~np.uint64(3) | np.asarray([0, 1, 2], dtype=np.uint64)
        return three[rng.integers(0, 3, n)]
    if name == 'all equal':         # one digit takes a whole tile
        return np.full(n, int(_uniform(rng, 1, end_bit)[0]), dtype=np.uint64)
    if name == 'sorted':
        return np.sort(_uniform(rng, n, end_bit))
    if name == 'reversed':
        return np.sort(_uniform(rng, n, end_bit))[::-1]
    if name == 'i % 512':
        return i % np.uint64(512)
    if name == '(i // 64) % 512':   # a chunk of one digit
        return (i // np.uint64(64)) % np.uint64(512)
    if name == 'bits above':        # random bits above the last pass: ignored by the order, carried in the keys
        if 9 * ref.passes(end_bit) >= top:
            return None
        keys = _uniform(rng, n, top)
        assert (keys >> np.uint64(9 * ref.passes(end_bit))).any()
        return keys
    raise KeyError(name)


@pytest.mark.parametrize('name', ['uniform', 'three keys', 'all equal', 'sorted', 'reversed', 'i % 512', '(i // 64) % 512',
                                  'bits above'])
@pytest.mark.parametrize('n', [4097, 3 * SORT_TILE + 5])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_sort_key_patterns(native_libs, kind, n, name):
    ran = 0
    for end_bit in PATTERN_END_BITS[kind]:
        rng = np.random.default_rng(kind * 1000 + end_bit + n)
        keys = _pattern(name, rng, n, kind, end_bit)
        if keys is None:
            continue
        _check_sort(native_libs, kind, keys, _values(rng, n), end_bit, name)
        ran += 1
    assert ran >= 3


@pytest.mark.parametrize('n', [4097, 3 * SORT_TILE + 5])
def test_sort_puts_all_ones_keys_last(native_libs, n):
    """localize: an empty class has the key 0xffffffff and 18 key bits are asked for -- two whole passes, and the
    key is all ones in both, so these classes come out last and in their input order"""
    rng = np.random.default_rng(n)
    keys = rng.integers(0, (1 << 18) - 1, n, dtype=np.uint64).astype(np.uint32)
    empty = rng.random(n) < 0.1
    keys[empty] = 0xffffffff
    vals = _values(rng, n)
    _check_sort(native_libs, 0, keys, vals, 18, 'a tenth 0xffffffff')
    got_keys, got_vals = _sort(native_libs, 0, keys, vals, 18)
    n_empty = int(empty.sum())
    assert 0 < n_empty < n
    assert (got_keys[n - n_empty:] == 0xffffffff).all() and (got_keys[:n - n_empty] < (1 << 18) - 1).all()
    np.testing.assert_array_equal(got_vals[n - n_empty:], vals[empty])
    assert (np.diff(got_keys[:n - n_empty].astype(np.int64)) >= 0).all()


@pytest.mark.parametrize('n', [1024 * SORT_TILE, 1024 * SORT_TILE + 1])      # 1025 tiles: the carry loop's second round
@pytest.mark.parametrize('kind,end_bit,three', [(0, 18, False), (1, 64, False), (2, 27, True)])
def test_sort_big(native_libs, kind, end_bit, three, n):
    rng = np.random.default_rng(kind + n)
    if three:                       # (they differ in each of the three digits)
        keys = np.asarray([5, (1 << 26) + (1 << 13) + 7, (1 << 20) + 3], dtype=np.uint64)[rng.integers(0, 3, n)]
    else:
        keys = _uniform(rng, n, end_bit)
    _check_sort(native_libs, kind, keys, _values(rng, n), end_bit)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_empty_inputs(native_libs):
    hip = native_libs.hip()
    out = np.full(1, -1, dtype=np.int64)
    for in_place in (0, 1):
        out[0] = -1
        assert hip.skm_device_scan_probe(0, None, 0, in_place, native_libs.ptr(out, native_libs.c_i64p)) == native_libs.SKM_OK
        assert out[0] == 0
    for kind in KINDS:
        assert hip.skm_device_sort_probe(0, kind, None, None, 0, 9, None, None) == native_libs.SKM_OK


def test_refusals_write_nothing(native_libs):
    hip, ARG = native_libs.hip(), native_libs.SKM_ERR_ARG
    n_dev = native_libs.device_count()
    values = np.arange(8, dtype=np.int64)
    out = np.full(9, -7, dtype=np.int64)
    p_in, p_out = native_libs.ptr(values, native_libs.c_i64p), native_libs.ptr(out, native_libs.c_i64p)
    for device, a, n, b in ((0, p_in, -1, p_out), (0, p_in, 1 << 31, p_out), (0, None, 8, p_out), (0, p_in, 8, None),
                            (0, None, 0, None), (n_dev, p_in, 8, p_out), (-1, p_in, 8, p_out)):
        for in_place in (0, 1):
            assert hip.skm_device_scan_probe(device, a, n, in_place, b) == ARG, (device, n)
            assert hip.skm_last_error()
    assert (out == -7).all() and (values == np.arange(8)).all()

    vals = np.arange(8, dtype=np.int32)
    vals_out = np.full(8, -7, dtype=np.int32)
    p_vals, p_vals_out = native_libs.ptr(vals, native_libs.c_i32p), native_libs.ptr(vals_out, native_libs.c_i32p)
    for kind, (dtype, width, _) in KINDS.items():
        keys = np.arange(8).astype(dtype)
        keys_out = np.full(8, 7, dtype=dtype)
        k, ko = keys.ctypes.data, keys_out.ctypes.data
        for device, kd, a, b, n, end_bit, c, d in (
                (0, kind, k, p_vals, -1, 9, ko, p_vals_out), (0, kind, k, p_vals, 1 << 31, 9, ko, p_vals_out),
                (0, kind, None, p_vals, 8, 9, ko, p_vals_out), (0, kind, k, None, 8, 9, ko, p_vals_out),
                (0, kind, k, p_vals, 8, 9, None, p_vals_out), (0, kind, k, p_vals, 8, 9, ko, None),
                (0, kind, k, p_vals, 8, -1, ko, p_vals_out), (0, kind, k, p_vals, 8, width + 1, ko, p_vals_out),
                (0, kind, k, p_vals, 0, width + 1, ko, p_vals_out),
                (0, -1, k, p_vals, 8, 9, ko, p_vals_out), (0, 3, k, p_vals, 8, 9, ko, p_vals_out),
                (n_dev, kind, k, p_vals, 8, 9, ko, p_vals_out), (-1, kind, k, p_vals, 8, 9, ko, p_vals_out)):
            assert hip.skm_device_sort_probe(device, kd, a, b, n, end_bit, c, d) == ARG, (device, kd, n, end_bit)
            assert hip.skm_last_error()
        assert (keys_out == 7).all() and (vals_out == -7).all()
        # end_bit 0 and the key's width are taken, and the call after a refusal works
        for end_bit in (0, width if kind != 2 else 31):
            _check_sort(native_libs, kind, keys[::-1].copy(), vals, end_bit)
    np.testing.assert_array_equal(_scan(native_libs, values, True), ref.scan(values))
