"""The numpy references of quant_reference.py against first principles: SplitMix64's
published outputs, the multinomial distribution, a brute-force sort and a float64 EM step.
The GPU tests (test_gpu_quant_edges.py) hold the kernels against these references."""
import numpy as np

from quant_reference import (_uniform_draws, check_multinomial_dispersion, draw_counts, em_step_ld,
                             internal_order, mix64, multinomial_tile)
from test_oracle_quant import _numpy_em_step


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63


def test_mix64_is_splitmix64():
    # SplitMix64 seeded with 0: its state advances by 0x9E3779B97F4A7C15 and each output is mix64(state)
    assert mix64(0x9E3779B97F4A7C15) == 0xe220a8397b1dcdaf
    assert mix64(2 * 0x9E3779B97F4A7C15) == 0x6e789e6aa1b965f4
    states = np.array([0x9E3779B97F4A7C15, (2 * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)], dtype=np.uint64)
    assert mix64(states).tolist() == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4]


def test_multinomial_tile():
    assert [multinomial_tile(c) for c in (1, 4096, 4097, 8192, 8193, 300_000, 8_388_608, 8_388_609)] \
        == [1, 1, 2, 2, 4, 128, 2048, 4096]
    assert multinomial_tile(4096 ** 2 + 1) > 4096


def test_draw_counts_is_a_multinomial_sampler():
    rng = np.random.default_rng(11)
    for n_classes in (700, 9000):                            # tiles of one class; tiles of four
        class_count = rng.integers(0, 60, n_classes)
        class_count[:40] = 0                              # zero-count runs: at the start, at the end,
        class_count[-35:] = 0                             # and over whole tiles
        class_count[1000:1100] = 0
        class_count[rng.integers(0, n_classes, 10)] = rng.integers(1000, 5000, 10)
        cum = np.cumsum(class_count)
        n = int(cum[-1])
        draws, redraws = zip(*(draw_counts(cum, n, 99, b) for b in range(200)))
        counts = np.array(draws)
        assert (counts.sum(axis=1) == n).all()
        assert (counts[:, class_count == 0] == 0).all()
        assert len({c.tobytes() for c in counts}) == counts.shape[0]
        mean = counts.mean(axis=0)
        p = class_count / n
        assert (np.abs(mean - n * p) < 6 * np.sqrt(n * p * (1 - p) / counts.shape[0]) + 1).all()
        check_multinomial_dispersion(counts, class_count.astype('f8'))
        assert sum(redraws) > 0 or n < 1000
    # seeds and replicate numbers both move the draw; one seed and number give one draw
    cum = np.cumsum(np.full(50, 3))
    a, _ = draw_counts(cum, 150, 0, 0)
    assert not np.array_equal(a, draw_counts(cum, 150, 1, 0)[0])
    assert not np.array_equal(a, draw_counts(cum, 150, 0, 1)[0])
    assert np.array_equal(a, draw_counts(cum, 150, 0, 0)[0])
    assert draw_counts(cum, 150, (1 << 64) - 1, 0)[0].sum() == 150


def test_uniform_draws_redraw_rejected_words():
    # range 2^31 + 1: 2^32 mod range = 2^31 - 1, so nearly every other word is rejected, and the
    # redraws leave the draw uniform (mean and variance of U[0, range) within 6 sigma)
    range_ = (1 << 31) + 1
    r, _, redraws = _uniform_draws(20001, range_, 5, 0, 0)
    assert r.size == 20001 and (r < range_).all() and 15000 < redraws < 25000
    u = r.astype('f8') / range_
    assert abs(u.mean() - 0.5) < 6 * np.sqrt(1 / 12 / u.size)
    assert abs(u.var() - 1 / 12) < 6 * np.sqrt(1 / 180 / u.size)
    # a range that divides 2^32 rejects nothing
    assert _uniform_draws(999, 1 << 20, 5, 0, 0)[2] == 0


def test_internal_order_matches_brute_force():
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 6, 500)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    targets = rng.integers(0, 60, offsets[-1]).astype(np.int32)
    order = internal_order(offsets, targets)
    keys = [min(targets[offsets[c]:offsets[c + 1]].tolist()) for c in range(lens.size)]
    brute = sorted(range(lens.size), key=lambda c: (keys[c], c))
    assert order.tolist() == brute


def test_em_step_ld_agrees_with_float64_within_its_bound():
    rng = np.random.default_rng(4)
    n_tx, n_classes = 400, 3000
    lens = rng.integers(1, 9, n_classes)
    lens[:3] = (64, 1000, 700)
    cls = np.repeat(np.arange(n_classes), lens)
    tx = rng.integers(0, n_tx - 10, cls.size)               # the last ten transcripts are in no class
    tx[rng.random(cls.size) < 0.2] = 5                       # a heavy transcript
    counts = rng.integers(1, 50, n_classes).astype('f8')
    counts[10:20] = 0
    l = rng.uniform(50, 3000, n_tx)
    x = rng.uniform(0.5, 2, n_tx) / n_tx
    x[[7, 8]] = 0
    offsets = np.concatenate([[0], np.cumsum(lens)])
    tx[offsets[30]:offsets[31]] = 7                         # a class whose sum is zero: NaN -> 0
    ref, bound = em_step_ld(x, l, offsets, tx, counts)
    got = _numpy_em_step(x, l, np.vstack([cls, tx]).astype(np.int64), counts, counts.sum())
    assert ref.dtype == np.longdouble
    assert ((got == 0) == (ref == 0)).all() and ref[n_tx - 10:].max() == 0 and ref[7] == 0
    live = ref > 0
    rel = np.abs(got[live].astype(np.longdouble) - ref[live]) / ref[live]
    assert (rel <= bound[live]).all()
    assert rel.max() > 0                                     # float64 did round somewhere
