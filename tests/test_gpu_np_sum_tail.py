"""numpy.sum on the device (skm_em.hip: np_sum_blocks_kernel) for arrays whose last block of 8192 is partial: the
block's own pairwise tree, walked by name with eight lanes per leaf, must give numpy's bits for every length --
below eight elements, one leaf with and without a remainder, a first split, the benchmark's 1986, the deepest
trees -- alone and behind 1 or 23 full blocks.  Through skm_device_np_sum_probe."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAILS = (1, 7, 8, 9, 127, 128, 129, 1986, 4095, 8191)


def _device_sum(native, values):
    values = np.ascontiguousarray(values, dtype='f8')
    out = np.full(1, np.nan)
    native.check(native.hip().skm_device_np_sum_probe(0, native.ptr(values, native.c_f64p), values.size,
                                                      native.ptr(out, native.c_f64p)))
    return out[0]


def _values(rng, n):
    """Doubles of mixed sign over sixteen orders of magnitude: any other association of the additions shows."""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 10.0 ** rng.integers(-8, 9, n)


@pytest.mark.parametrize('full_blocks', [0, 1, 23])
def test_partial_last_block_equals_numpy_bit_for_bit(native_libs, full_blocks):
    rng = np.random.default_rng(100 + full_blocks)
    for tail in TAILS:
        values = _values(rng, 8192 * full_blocks + tail)
        got, want = _device_sum(native_libs, values), values.sum()
        assert got.tobytes() == np.float64(want).tobytes(), (full_blocks, tail, got, want)


def test_positive_values_of_one_scale(native_libs):
    """The start vector's kind of input: reciprocals of lengths."""
    rng = np.random.default_rng(3)
    for n in (1986, 8192 * 23 + 1986):
        values = 1.0 / rng.uniform(100, 3000, n)
        assert _device_sum(native_libs, values).tobytes() == np.float64(values.sum()).tobytes()


def test_empty_and_refusals(native_libs):
    out = np.full(1, 7.0)
    p_out = native_libs.ptr(out, native_libs.c_f64p)
    assert native_libs.hip().skm_device_np_sum_probe(0, None, 0, p_out) == native_libs.SKM_OK and out[0] == 0.0
    values = np.ones(4)
    p_in = native_libs.ptr(values, native_libs.c_f64p)
    out[0] = 7.0
    for device, a, n, b in ((0, p_in, -1, p_out), (0, None, 4, p_out), (0, p_in, 4, None), (0, p_in, 1 << 31, p_out),
                            (-1, p_in, 4, p_out)):
        assert native_libs.hip().skm_device_np_sum_probe(device, a, n, b) == native_libs.SKM_ERR_ARG
    assert out[0] == 7.0
