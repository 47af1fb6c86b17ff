"""Sequence bias for sample sets, the host's side (no GPU): the fixed-point weights of the expected counts against
exact arithmetic, the argument checks of the new Python entry points, and the header function under
AddressSanitizer + UBSan in a program of its own."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'seekmer_amd', 'csrc')


def _fixed_weights(native, tpm, windows):
    tpm = np.ascontiguousarray(tpm, dtype='f8')
    windows = np.ascontiguousarray(windows, dtype=np.int32)
    limbs = np.full((3, tpm.size), 7, dtype=np.uint64)
    total = np.zeros(1)
    code = native.host().skm_bias_fixed_weights(
        native.ptr(tpm, native.c_f64p), native.ptr(windows, native.c_i32p), tpm.size,
        native.ptr(limbs, native.c_u64p), native.ptr(total, native.c_f64p))
    return code, limbs, float(total[0])


def _exact_weights(tpm, windows):
    """The contract in Python ints and fractions: the total added in transcript order as doubles, the scale and
    the product as the doubles they are, then round-half-up, the clamp below 2^95 and the cut into limbs exactly."""
    total = 0.0
    for a, n in zip(tpm, windows):
        total += float(a) * float(n)
    limbs = np.zeros((3, len(tpm)), dtype=np.uint64)
    if total > 0:
        scale = 2.0 ** 94 / total
        for t, (a, n) in enumerate(zip(tpm, windows)):
            if n == 0:
                continue
            w = Fraction(float(a) * scale)                      # (the double product, held exactly)
            fixed = int(w + Fraction(1, 2)) if w < 2 ** 52 else int(w)
            fixed = min(fixed, 2 ** 95 - 1)
            for k in range(3):
                limbs[k, t] = (fixed >> (32 * k)) & 0xffffffff
    return limbs, total


def _value(limbs, t):
    return sum(int(limbs[k, t]) << (32 * k) for k in range(3))


def test_fixed_weights_equal_exact_arithmetic(native_libs):
    rng = np.random.default_rng(94)
    n_tx = 500
    tpm = np.exp(rng.uniform(np.log(1e-3), np.log(1e6), n_tx))
    tpm[rng.integers(0, n_tx, 40)] = 0.0
    windows = rng.integers(1, 5000, n_tx).astype(np.int32)
    windows[[3, 77, 400]] = 0                                   # transcripts without windows
    tpm[77] = 1e6
    code, limbs, total = _fixed_weights(native_libs, tpm, windows)
    want, want_total = _exact_weights(tpm, windows)
    assert code == native_libs.SKM_OK and total == want_total
    np.testing.assert_array_equal(limbs, want)
    assert (limbs < 2 ** 32).all()
    assert not limbs[:, [3, 77, 400]].any()                     # no window: limbs 0, whatever the abundance
    # W_t is tpm_t 2^94 / sum tpm n within the roundings of the doubles on the way: n_tx additions, one
    # division, one product (each 2^-53 relative; the bound below allows twice their sum for the second-order
    # terms) and half a unit of the last place of the fixed point
    exact_total = sum(Fraction(float(a)) * int(n) for a, n in zip(tpm, windows))
    for t in range(n_tx):
        if windows[t] == 0 or tpm[t] == 0:
            assert _value(limbs, t) == 0
            continue
        exact = Fraction(float(tpm[t])) * 2 ** 94 / exact_total
        assert abs(_value(limbs, t) - exact) <= exact * (n_tx + 4) * Fraction(1, 2 ** 52) + Fraction(1, 2)
    # the sum over the windows of the weights is one in fixed point, within the same bound
    one = sum(_value(limbs, t) * int(windows[t]) for t in range(n_tx))
    assert abs(Fraction(one, 2 ** 94) - 1) < Fraction(n_tx + 2, 2 ** 52)


def test_fixed_weights_edge_cases(native_libs):
    windows = np.asarray([10, 0, 250, 7], dtype=np.int32)
    code, limbs, total = _fixed_weights(native_libs, np.zeros(4), windows)          # nothing expressed
    assert code == native_libs.SKM_OK and total == 0.0 and not limbs.any()
    code, limbs, total = _fixed_weights(native_libs, [0.0, 5.0, 0.0, 0.0], windows)  # ... but in a transcript without windows
    assert code == native_libs.SKM_OK and total == 0.0 and not limbs.any()
    # one transcript with one window holds everything: 2^94 itself, and under a scale that rounds up, the clamp
    for a in (1.0, 3.0, 1e6, 0.1, 1e-3):
        code, limbs, total = _fixed_weights(native_libs, [0.0, 0.0, 0.0, a], np.asarray([10, 0, 250, 1], dtype=np.int32))
        want, _ = _exact_weights([0.0, 0.0, 0.0, a], [10, 0, 250, 1])
        assert code == native_libs.SKM_OK
        np.testing.assert_array_equal(limbs, want)
        assert 2 ** 94 - 2 ** 42 <= _value(limbs, 3) <= 2 ** 95 - 1 and not limbs[:, :3].any()
    # the smallest total whose scale (2^1023) is still finite: the weight stays below 2^95
    tiny = 2.0 ** -929
    code, limbs, total = _fixed_weights(native_libs, [tiny, 0, 0, 0], np.asarray([1, 0, 0, 0], dtype=np.int32))
    assert code == native_libs.SKM_OK and _value(limbs, 0) <= 2 ** 95 - 1
    np.testing.assert_array_equal(limbs, _exact_weights([tiny, 0, 0, 0], [1, 0, 0, 0])[0])
    # totals that cannot be scaled: 2^94 / total overflows, or the total does
    for tpm in ([5e-324, 0, 0, 0], [1e308, 0, 1e308, 0]):
        code, limbs, _ = _fixed_weights(native_libs, tpm, windows)
        assert code == native_libs.SKM_ERR_ARG
        assert (limbs == 7).all()                                # nothing written
    for bad in (np.nan, np.inf, -1.0):
        assert _fixed_weights(native_libs, [1.0, bad, 1.0, 1.0], windows)[0] == native_libs.SKM_ERR_ARG
    assert _fixed_weights(native_libs, np.ones(4), np.asarray([1, -1, 1, 1], dtype=np.int32))[0] == native_libs.SKM_ERR_ARG
    total = np.zeros(1)
    assert native_libs.host().skm_bias_fixed_weights(None, None, 0, None, native_libs.ptr(total, native_libs.c_f64p)) == native_libs.SKM_OK
    assert native_libs.host().skm_bias_fixed_weights(None, None, 2, None, native_libs.ptr(total, native_libs.c_f64p)) == native_libs.SKM_ERR_ARG


class _NoDevice:
    """An index that must not be asked for a device handle."""

    def __init__(self, n_tx):
        self.transcripts = np.zeros(n_tx, dtype=[('length', 'f8')])
        self.transcripts['length'] = 100.0

    def device_handle(self, device):
        raise AssertionError('the device was touched')


def _summary(n_tx, n_classes=2):
    from seekmer_amd import mapper
    class_map = np.vstack([np.arange(n_classes, dtype=np.int64), np.arange(n_classes, dtype=np.int64) % n_tx])
    return mapper.SummarizedResult(n_classes, 0, n_classes, class_map, np.ones(n_classes), None, np.full(n_tx, 50.0))


def test_quantify_tables_checks_its_start_vectors_before_any_native_call(native_libs, monkeypatch):
    from seekmer_amd import _native, infer

    def no_native():
        raise AssertionError('a native call was made')
    monkeypatch.setattr(_native, 'hip', no_native)
    tables = [_summary(6), _summary(6), _summary(6)]
    for x0s in (np.ones((2, 6)), np.ones((4, 6)), np.ones((3, 5)), np.ones((3, 7)), np.ones(6), np.ones((3, 6, 1))):
        with pytest.raises(ValueError, match='x0s must be'):
            infer.quantify_tables(tables, x0s=x0s)
    with pytest.raises(ValueError, match='x0s must be'):
        infer.quantify_tables([], x0s=np.ones((1, 6)))
    assert infer.quantify_tables([], x0s=np.zeros((0, 6))).shape == (0, 0)


def test_bias_correct_many_checks_its_shapes_before_any_native_call(native_libs, monkeypatch):
    from seekmer_amd import _native, infer

    def no_native():
        raise AssertionError('a native call was made')
    monkeypatch.setattr(_native, 'hip', no_native)
    index = _NoDevice(6)
    two = [_summary(6), _summary(6)]
    good_tpm, good_observed = np.ones((2, 6)), np.zeros((2, 4096), dtype=np.int64)
    cases = [(two, np.ones((3, 6)), good_observed), (two, np.ones((2, 5)), good_observed), (two, np.ones(6), good_observed),
             (two, good_tpm, np.zeros((2, 4095), dtype=np.int64)), (two, good_tpm, np.zeros((1, 4096), dtype=np.int64)),
             (two, good_tpm, np.zeros(4096, dtype=np.int64)), ([_summary(6), _summary(5)], good_tpm, good_observed)]
    for summaries, tpms, observed in cases:
        with pytest.raises(ValueError, match='bias_correct_many takes'):
            infer.bias_correct_many(index, summaries, tpms, observed, None)
        with pytest.raises(ValueError, match='bias_correct_many takes'):
            infer.bias_pass_many(index, summaries, tpms, observed, None)
    with pytest.raises(ValueError):
        infer.bias_correct_many(index, two, good_tpm, good_observed, 'sideways')


def test_the_new_options_default_to_off_and_impute_takes_none():
    from seekmer_amd import __main__ as cli
    assert 'bias' not in cli.parse_args(['impute', 'index', 'out', 'a.fq', 'b.fq'])
    from seekmer_amd import mapper
    import inspect
    assert inspect.signature(mapper.SampleSet.__init__).parameters['bias'].default is False
    assert inspect.signature(mapper.map_sample_set).parameters['bias'].default is False


PROGRAM = r'''
#include "skm_bias_weights.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

// the header function on heap arrays of exactly the sizes its contract names, so that a word read or written
// outside them is an AddressSanitizer report
static unsigned long long value_ok(const std::vector<unsigned long long> &limbs, size_t n_tx)
{
    unsigned long long worst = 0;
    for (size_t i = 0; i < 3 * n_tx; ++i) worst = limbs[i] > worst ? limbs[i] : worst;
    return worst;
}

int main()
{
    unsigned long long state = 88172645463325252ULL;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (size_t n_tx : {0, 1, 2, 63, 1000}) {
        std::vector<double> tpm(n_tx);
        std::vector<int32_t> windows(n_tx);
        for (size_t t = 0; t < n_tx; ++t) {
            tpm[t] = (double)(next() % 1000000) * 1e-3;
            windows[t] = (int32_t)(next() % 3000);
        }
        for (int round = 0; round < 4; ++round) {
            if (round == 1) for (auto &a : tpm) a = 0.0;                       // nothing expressed
            if (round == 2 && n_tx) { tpm[n_tx - 1] = 1e6; windows[n_tx - 1] = 1; }   // one transcript holds everything
            if (round == 3 && n_tx) {                                          // a total that cannot be scaled
                for (auto &a : tpm) a = 0.0;
                tpm[0] = 5e-324; windows[0] = 1;
            }
            std::vector<unsigned long long> limbs(3 * n_tx, 9);
            double total = -1.0;
            const bool ok = skm::bias_fixed_weights(tpm.data(), windows.data(), (int64_t)n_tx, limbs.data(), &total);
            if (ok && value_ok(limbs, n_tx) >= (1ULL << 32)) { std::printf("limb above 2^32\n"); return 1; }
            if (round == 1 && (!ok || value_ok(limbs, n_tx) != 0 || total != 0.0)) { std::printf("zeros\n"); return 1; }
            if (round == 2 && n_tx && (!ok || limbs[2 * n_tx + n_tx - 1] < (1u << 29))) { std::printf("one transcript\n"); return 1; }
            if (round == 3 && n_tx && ok) { std::printf("unscalable total accepted\n"); return 1; }
        }
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_header_function_is_clean_under_asan_ubsan(tmp_path):
    """A program of its own (nothing is preloaded): the header function, compiled with both sanitizers."""
    source = tmp_path / 'fixed_weights_main.cpp'
    source.write_text(PROGRAM)
    binary = tmp_path / 'fixed_weights_main'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                           '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan', '-I', CSRC, str(source), '-o', str(binary)])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    proc = subprocess.run([str(binary)], env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    assert proc.stdout.strip().endswith('ok')
    assert 'runtime error' not in proc.stderr and 'AddressSanitizer' not in proc.stderr, proc.stderr[-3000:]
