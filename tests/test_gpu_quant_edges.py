"""The quantification kernels (skm_em.hip, skm_em_batch.hip, skm_quant_setup.hip) against
exact host references (quant_reference.py) at the shapes where they could go wrong: tile
boundaries of the bootstrap draw, the class views' three-pass radix sorts, EM row and tuple
edges, every leaf shape of numpy's pairwise sum, adversarial fragment-length histograms."""
import numpy as np
import pytest

from quant_reference import draw_counts, em_step_ld, internal_order

pytestmark = pytest.mark.gpu

SEEDS = (0, (1 << 64) - 1, 0x5EED_2026_0BAD_F00D)
DEGREES = (1, 7, 8, 9, 16, 17, 511, 512, 513, 1024, 1025, 4097, 100_003)


def _check_table(n_tx, offsets, targets, counts=None):
    """What skm_mapper_merge and skm_quant_create_from_mapper do not check, checked here."""
    assert offsets[0] == 0 and (np.diff(offsets) > 0).all() and offsets[-1] == targets.size
    assert targets.min() >= 0 and targets.max() < n_tx
    if counts is not None:
        assert counts.size == offsets.size - 1 and (counts >= 0).all()


def _em_inputs(n_tx, rng):
    l = rng.uniform(100, 3000, n_tx)
    x0 = 1.0 / l
    return x0 / x0.sum(), l


# ---------------------------------------------------------------- the bootstrap draw, count for count

def _scattered_singletons(n_classes, n_tx):
    """Classes of one transcript each, ids scattered so that the locality order is a real permutation."""
    offsets = np.arange(n_classes + 1, dtype=np.int64)
    targets = ((np.arange(n_classes, dtype=np.int64) * 7919 + 13) % n_tx).astype(np.int32)
    return offsets, targets


def _random_tuples(n_classes, n_tx, rng, longest=5):
    lens = rng.integers(1, longest + 1, n_classes)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offsets, rng.integers(0, n_tx, offsets[-1]).astype(np.int32)


def _pattern(n_classes, kind, rng, total=None):
    """Class counts in INTERNAL (draw) order."""
    tile = 1
    while (n_classes + tile - 1) // tile > 4096:
        tile <<= 1
    c = rng.integers(0, 40, n_classes).astype(np.int64)
    if kind == 'runs':                                   # zero runs: at the start, at the end, over a whole tile
        c[:min(37, n_classes // 3)] = 0
        c[n_classes - min(29, n_classes // 3):] = 0
        if n_classes > 3 * tile:
            c[tile:3 * tile] = 0
        c[rng.integers(0, n_classes, 3)] += 500
    elif kind == 'heavy':                                # one class holds more than 99 % of the mass
        c[:] = rng.integers(0, 2, n_classes)
        c[n_classes // 2] = 200 * (c.sum() + 1)
    if total is not None:                                # thinned to about `total` draws
        c = rng.binomial(c, total / max(c.sum(), 1)).astype(np.int64)
    if c.sum() == 0:
        c[-1] = 1
    return c


def _caller(order, internal):
    out = np.empty_like(internal)
    out[order] = internal
    return out


def _expected_draw(order, counts, seed, number):
    cum = np.cumsum(counts[order])
    got, redraws = draw_counts(cum, int(cum[-1]), seed, number)
    return _caller(order, got), redraws


def _draw_and_compare(quant, offsets, targets, counts, seeds, n_boot, x0, l):
    order = internal_order(offsets, targets)
    redraws = 0
    results = {}
    for seed in seeds:
        out, drawn, iters = quant.bootstrap(n_boot, seed, x0, l, want_counts=True)
        for b in range(n_boot):
            expected, more = _expected_draw(order, counts, seed, b)
            redraws += more
            assert drawn[b].sum() == counts.sum()
            np.testing.assert_array_equal(drawn[b], expected, err_msg='seed %d replicate %d' % (seed, b))
        results[seed] = (out, drawn, iters)
    return redraws, results


def test_bootstrap_draw_equals_restatement(native_libs):
    from seekmer_amd import infer
    rng = np.random.default_rng(20)
    redraws = 0
    cases = [  # (classes, transcripts, count pattern, seeds, replicates)
        (1, 3, 'plain', SEEDS, 3), (2, 3, 'runs', SEEDS, 3),
        (4095, 700, 'runs', SEEDS, 2), (4096, 700, 'heavy', SEEDS, 2), (4097, 700, 'runs', SEEDS, 2),
        (8193, 900, 'runs', SEEDS[:2], 2), (8193, 900, 'heavy', SEEDS[2:], 1),
        (300_007, 5000, 'runs', SEEDS[1:2], 1), (300_007, 5000, 'heavy', SEEDS[:1], 1),
        (8_388_609, 1000, 'runs', SEEDS[2:], 1),
    ]
    for n_classes, n_tx, kind, seeds, n_boot in cases:
        offsets, targets = _scattered_singletons(n_classes, n_tx)
        order = internal_order(offsets, targets)
        total = 1_500_000 if n_classes > 1_000_000 else None
        internal = _pattern(n_classes, kind, rng, total) if n_classes > 2 else np.array([7, 4][:n_classes])
        counts = _caller(order, internal)
        if n_classes == 2:
            counts = np.array([0, 10])                  # a zero class first, an even total
        _check_table(n_tx, offsets, targets, counts)
        x0, l = _em_inputs(n_tx, rng)
        quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts.astype('f8'))
        try:
            more, _ = _draw_and_compare(quant, offsets, targets, counts, seeds, n_boot, x0, l)
        finally:
            quant.close()
        redraws += more
    assert redraws > 0                                   # the keyed redraw path was taken and restated


@pytest.mark.parametrize('n_classes,n_tx', [(4097, 500), (300_007, 20_000)])
def test_exact_draws_give_exact_em(native_libs, n_classes, n_tx):
    """The drawn counts, restated on the host and set with set_counts, give the replicate's EM
    bit for bit and step for step: through the one-by-one path and the batched one."""
    from seekmer_amd import infer
    rng = np.random.default_rng(n_classes)
    offsets, targets = _random_tuples(n_classes, n_tx, rng)
    order = internal_order(offsets, targets)
    counts = _caller(order, _pattern(n_classes, 'runs', rng))
    _check_table(n_tx, offsets, targets, counts)
    x0, l = _em_inputs(n_tx, rng)
    seed = SEEDS[2]
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts.astype('f8'))
    try:
        _, results = _draw_and_compare(quant, offsets, targets, counts, (seed,), 3, x0, l)
        out, _, iters = results[seed]
        batched, _, iters_b = quant.bootstrap(3, seed, x0, l)
        np.testing.assert_array_equal(batched, out)
        np.testing.assert_array_equal(iters_b, iters)
        for b in range(3):
            quant.set_counts(_expected_draw(order, counts, seed, b)[0].astype('f8'))
            x, it = quant.em(x0, l)
            assert it == iters[b]
            np.testing.assert_array_equal(x, out[b])
    finally:
        quant.close()


def test_bootstrap_draw_on_a_mapped_table(native_libs):
    """configs[4] in shape: paired reads mapped on the GPU, the table resampled where it lies."""
    from seekmer_amd import common, index_builder, infer, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(4, 60)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 100_000
    bases, offsets = synth.reads(4, pool, tx_offsets, 0, n_units, 100, True)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
    n_tx = len(ids)
    class_offsets, class_targets, counts, _, _ = result.export()
    assert counts.size > 200
    x0, l = _em_inputs(n_tx, np.random.default_rng(4))
    quant = infer._QuantHandle.from_map_result(result, n_tx)
    try:
        _draw_and_compare(quant, class_offsets, class_targets, counts, SEEDS, 2, x0, l)
    finally:
        quant.close()


def test_refused_draws_leave_the_handle_usable(native_libs):
    from seekmer_amd import _native, infer
    rng = np.random.default_rng(21)
    for n_classes, n_tx, counts in ((2, 5, np.array([(1 << 32) - 5, 5.0])),              # 2^32 units
                                    (4096 ** 2 + 1, 1000, np.ones(4096 ** 2 + 1))):     # tile > 4096
        offsets, targets = _scattered_singletons(n_classes, n_tx)
        _check_table(n_tx, offsets, targets, counts)
        x0, l = _em_inputs(n_tx, rng)
        quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
        try:
            before, it_before = quant.em(x0, l)
            for want_counts in (True, False):
                with pytest.raises(_native.NativeError) as raised:
                    quant.bootstrap(1, 5, x0, l, want_counts=want_counts)
                assert raised.value.code == _native.SKM_ERR_STATE
                after, it_after = quant.em(x0, l)
                assert it_after == it_before
                np.testing.assert_array_equal(after, before)
        finally:
            quant.close()


# ---------------------------------------------------------------- EM against extended precision

def _edge_table(n_tx, seed):
    """Classes in caller order: one transcript at each degree of DEGREES (its first class holds it
    twice), tuples of 1-9, 64, 1000 and 20 000 ids with duplicates, four transcripts in no class,
    two transcripts that start at zero and share a class (its sum is zero: NaN -> 0), zero counts.
    Tuples are distinct when n_tx exceeds the largest degree.  Returns (offsets, targets, counts,
    zeroed transcripts)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n_tx)
    special, orphans, zeroed, pool = ids[:13], ids[13:17], ids[17:19], ids[19:]
    tuples = []
    for t, d in zip(special, DEGREES):
        partners = pool[rng.permutation(pool.size)[:d]] if d <= pool.size else pool[rng.integers(0, pool.size, d)]
        for i in range(d - (1 if d >= 2 else 0)):
            extra = rng.integers(0, pool.size, int(rng.integers(0, 3)))
            tup = [t] * (2 if i == 0 and d >= 2 else 1) + [partners[i]] + pool[extra].tolist()
            if d == 1:
                tup = [t]
            rng.shuffle(tup)
            tuples.append(tup)
    background = {}
    for size in list(rng.integers(1, 10, 20_000)) + [64, 1000, 20_000]:
        tup = pool[rng.integers(0, pool.size, size)]
        background.setdefault(tup.tobytes(), tup.tolist())
    tuples += list(background.values())
    tuples += [[zeroed[0], zeroed[1]], [zeroed[1]]]
    counts = rng.integers(1, 30, len(tuples)).astype(np.int64)
    counts[rng.integers(0, len(tuples), 50)] = 0
    counts[len(DEGREES) + 5] = 0                        # (a class of the degree-9 transcript)
    counts[-1] = 0                                      # zero count and zero sum
    order = rng.permutation(len(tuples))
    tuples = [tuples[k] for k in order]
    counts = counts[order]
    lens = np.array([len(t) for t in tuples])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    targets = np.concatenate([np.asarray(t) for t in tuples]).astype(np.int32)
    assert not np.isin(orphans, targets).any()
    assert np.bincount(targets, minlength=n_tx)[special].tolist() == list(DEGREES)
    return offsets, targets, counts, zeroed


def _edge_start(n_tx, zeroed, seed):
    rng = np.random.default_rng(seed + 1)
    x0, l = _em_inputs(n_tx, rng)
    x0[zeroed] = 0
    return x0 / x0.sum(), l


def _check_steps(quant, x0, l, offsets, targets, counts):
    """Three single steps, each from the GPU's previous result, within em_step_ld's bound."""
    x = x0
    for _ in range(3):
        got, it = quant.em(x, l, fixed_iters=1)
        assert it == 1
        ref, bound = em_step_ld(x, l, offsets, targets, counts)
        zero = ref == 0
        assert zero.any() and (got[zero] == 0).all()
        rel = np.abs(got[~zero].astype(np.longdouble) - ref[~zero]) / ref[~zero]
        worst = np.argmax(rel / bound[~zero])
        assert (rel <= bound[~zero]).all(), (float(rel[worst]), float(bound[~zero][worst]))
        x = got


def _class_map(offsets, targets):
    return np.vstack([np.repeat(np.arange(offsets.size - 1), np.diff(offsets)), targets]).astype(np.int64)


def _check_converged(quant, x0, l, class_map, counts, oracle):
    x, it = quant.em(x0, l)
    x_ref, it_ref = oracle.em(x0, l, class_map, counts.astype('f8'))
    assert it == it_ref
    np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
    return x, it


@pytest.mark.parametrize('n_tx', [300, (1 << 18) + 3])
def test_em_row_and_tuple_edges_against_extended_precision(oracle, native_libs, n_tx):
    from seekmer_amd import infer
    offsets, targets, counts, zeroed = _edge_table(n_tx, n_tx)
    _check_table(n_tx, offsets, targets, counts)
    x0, l = _edge_start(n_tx, zeroed, n_tx)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts.astype('f8'))
    try:
        _check_steps(quant, x0, l, offsets, targets, counts)
        x, it = _check_converged(quant, x0, l, _class_map(offsets, targets), counts, oracle)
        again, it_again = quant.em(x0, l)
        assert it_again == it
        np.testing.assert_array_equal(again, x)
    finally:
        quant.close()


_UNFUSED_CHILD = '''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from seekmer_amd import infer
d = np.load(sys.argv[2])
quant = infer._QuantHandle.from_csr(int(d['n_tx']), d['offsets'], d['targets'], d['counts'])
try:
    x, it = quant.em(d['x0'], d['l'])
    x3, it3 = quant.em(d['x0'], d['l'], fixed_iters=3)
    boot, _, boot_it = quant.bootstrap(9, int(d['seed']), d['x0'], d['l'])
finally:
    quant.close()
np.savez(sys.argv[3], x=x, it=it, x3=x3, it3=it3, boot=boot, boot_it=boot_it)
'''


def test_unfused_em_equals_fused(native_libs, tmp_path):
    """SKM_EM_UNFUSED=1 (read once per process: a fresh child) runs rows and finalize as two launches,
    single-problem and batched, with the whole-table kernels only: bit for bit and step for step what
    this process computes with the fused and tile kernels."""
    import os
    import subprocess
    import sys
    from seekmer_amd import infer
    n_tx = 300
    offsets, targets, counts, zeroed = _edge_table(n_tx, n_tx)
    x0, l = _edge_start(n_tx, zeroed, n_tx)
    given, got = str(tmp_path / 'given.npz'), str(tmp_path / 'unfused.npz')
    np.savez(given, n_tx=n_tx, offsets=offsets, targets=targets, counts=counts.astype('f8'), x0=x0, l=l,
             seed=np.uint64(SEEDS[2]))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run(['timeout', '-k', '10', '120', sys.executable, '-c', _UNFUSED_CHILD, root, given, got],
                          env=dict(os.environ, SKM_EM_UNFUSED='1'), capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    child = np.load(got)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts.astype('f8'))
    try:
        x, it = quant.em(x0, l)
        x3, it3 = quant.em(x0, l, fixed_iters=3)
        boot, _, boot_it = quant.bootstrap(9, SEEDS[2], x0, l)
    finally:
        quant.close()
    assert it3 == 3
    np.testing.assert_array_equal(child['it'], it)
    np.testing.assert_array_equal(child['it3'], it3)
    np.testing.assert_array_equal(child['boot_it'], boot_it)
    np.testing.assert_array_equal(child['x'], x)
    np.testing.assert_array_equal(child['x3'], x3)
    np.testing.assert_array_equal(child['boot'], boot)


def test_em_single_transcript(oracle, native_libs):
    from seekmer_amd import infer
    offsets = np.array([0, 1, 3, 6], dtype=np.int64)
    targets = np.zeros(6, dtype=np.int32)
    counts = np.array([3, 0, 5], dtype=np.int64)
    x0, l = np.ones(1), np.array([250.0])
    quant = infer._QuantHandle.from_csr(1, offsets, targets, counts.astype('f8'))
    try:
        _check_steps_single(quant, x0, l, offsets, targets, counts)
        _check_converged(quant, x0, l, _class_map(offsets, targets), counts, oracle)
    finally:
        quant.close()


def _check_steps_single(quant, x0, l, offsets, targets, counts):
    x = x0
    for _ in range(3):
        got, it = quant.em(x, l, fixed_iters=1)
        ref, bound = em_step_ld(x, l, offsets, targets, counts)
        assert it == 1 and ref[0] > 0
        assert abs(got[0] - ref[0]) <= bound[0] * ref[0]
        x = got


def test_em_three_pass_sorts_three_ways(oracle, native_libs):
    """2^18 + 3 transcripts: the class views' radix sorts take three 9-bit passes.  The same
    classes from the caller's CSR (localize), from a mapper's table with distinct first-seen
    values (ranked by bitmap) and with shared ones (the first-seen sort, then localize)."""
    from seekmer_amd import index_builder, infer, mapper, synth
    n_tx = (1 << 18) + 3
    offsets, targets, counts, zeroed = _edge_table(n_tx, 7)
    _check_table(n_tx, offsets, targets, counts)
    keys = {targets[offsets[c]:offsets[c + 1]].tobytes() for c in range(counts.size)}
    assert len(keys) == counts.size                    # a mapper merges classes by their tuple
    assert targets.max() >= (1 << 18)
    x0, l = _edge_start(n_tx, zeroed, 7)
    class_map = _class_map(offsets, targets)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts.astype('f8'))
    try:
        x_csr, it_csr = _check_converged(quant, x0, l, class_map, counts, oracle)
        one, _, iters_one = quant.bootstrap(9, SEEDS[2], x0, l, want_counts=True)
        batched, _, iters_b = quant.bootstrap(9, SEEDS[2], x0, l)
        np.testing.assert_array_equal(iters_b, iters_one)
        np.testing.assert_array_equal(batched, one)
    finally:
        quant.close()
    ids, pool, tx_offsets = synth.transcriptome(3, 20)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    first = np.cumsum(np.random.default_rng(8).integers(2, 12, counts.size)).astype(np.int64)
    assert first[-1] // 3 >= (1 << 18) and np.unique(first // 3).size < first.size
    for first_seen, ranked in ((first, True), (first // 3, False)):
        result = mapper.MapResult(index)
        result.merge_table(offsets, targets, counts, first_seen, 0, np.zeros(2000, dtype=np.int64))
        exported = result.export()
        if ranked:                                     # first-seen order is the caller's order
            np.testing.assert_array_equal(exported[0], offsets)
            np.testing.assert_array_equal(exported[1], targets)
            np.testing.assert_array_equal(exported[2], counts)
        quant = infer._QuantHandle.from_map_result(result, n_tx)
        try:
            if ranked:                                 # the same caller order and internal order: the same bits
                x, it = quant.em(x0, l)
                assert it == it_csr
                np.testing.assert_array_equal(x, x_csr)
            else:                                      # ties may reorder classes: held to the bound
                _check_steps(quant, x0, l, offsets, targets, counts)
                _check_converged(quant, x0, l, class_map, counts, oracle)
        finally:
            quant.close()
        del result


# ---------------------------------------------------------------- numpy's sums restated on the device

TPM_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 255, 256, 257, 1000, 8191, 8192, 8193,
             16384, 16391, 3 * 8192 + 129, 190_001)


def _tpm_problem(n_tx, rng):
    offsets = np.arange(n_tx + 1, dtype=np.int64)
    targets = rng.permutation(n_tx).astype(np.int32)
    counts = rng.integers(1, 50, n_tx).astype(np.int64)
    counts[np.flatnonzero(targets == 0)[0]] = counts.sum()   # (x_0 above the EM's floor in every replicate)
    l = 10.0 ** rng.uniform(0, 12, n_tx)
    l[0] = 1.0
    x0 = 1.0 / l
    return offsets, targets, counts, x0 / x0.sum(), l


@pytest.mark.parametrize('n_tx,n_boot', [(n, 16 if n < 128 else 4) for n in TPM_SIZES] + [(3, 40_000)])
def test_tpm_scaling_every_shape(native_libs, n_tx, n_boot):
    from seekmer_amd import infer
    rng = np.random.default_rng(n_tx)
    offsets, targets, counts, x0, l = _tpm_problem(n_tx, rng)
    _check_table(n_tx, offsets, targets, counts)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts.astype('f8'))
    try:
        tpm, _, iters_tpm = quant.bootstrap(n_boot, 31, x0, l, tpm=True)
        raw, _, iters = quant.bootstrap(n_boot, 31, x0, l)
    finally:
        quant.close()
    np.testing.assert_array_equal(iters_tpm, iters)
    for b in range(n_boot):
        np.testing.assert_array_equal(tpm[b], infer._tpm(raw[b].copy()), err_msg='replicate %d' % b)
    if n_tx >= 9:                                       # numpy's blocked pairwise sum, not a left-to-right one
        assert any(np.cumsum(raw[b])[-1] != raw[b].sum() for b in range(n_boot))
    assert (raw > 0).sum() > (tpm > 0).sum() or n_tx < 100   # the 0.001 cut removed something


# ---------------------------------------------------------------- effective lengths

def _effective_lengths_ref(fld, lengths):
    """mapper.py:134-141 literally, evaluated once per distinct length."""
    values, inverse = np.unique(lengths, return_inverse=True)
    expected = np.zeros(values.shape, dtype='f8')
    with np.errstate(invalid='ignore'):
        p = fld / fld.sum()
    for i in range(p.size):
        expected += (values - i).clip(min=1) * p[i]
    return expected[inverse]


def _histograms(rng):
    out = {}
    out['all bins'] = rng.integers(1, 1000, 2000)
    h = np.zeros(2000, dtype=np.int64)
    h[[0, 1999]] = (3, 5)
    out['bins 0 and 1999'] = h
    h = np.zeros(2000, dtype=np.int64)
    h[777] = 42
    out['one bin'] = h
    h = np.zeros(2000, dtype=np.int64)
    h[1500:] = rng.integers(0, 50, 500)
    h[1500] = 9
    out['bins >= 1500'] = h
    h = np.zeros(2000, dtype=np.int64)
    h[[0, 5, 10, 300, 1999]] = (1, 3, (1 << 53) + 1, 1 << 60, 7)
    out['2^53 + 1 and 2^60'] = h
    out['empty'] = np.zeros(2000, dtype=np.int64)
    return out


def test_effective_lengths_adversarial(native_libs):
    from seekmer_amd import _native
    hip = _native.hip()
    rng = np.random.default_rng(22)
    special = np.array([0.5, 1, 1.5, 1999, 2000, 2001, 1e12])
    big = np.concatenate([special, rng.integers(1, 5000, 1_000_003 - special.size).astype('f8')])
    rng.shuffle(big)
    assert (big <= 1500).any()
    for name, fld in _histograms(rng).items():
        fld = np.ascontiguousarray(fld, dtype=np.int64)
        assert fld.sum() < (1 << 63)
        for lengths in (np.zeros(0), special[[int(rng.integers(0, special.size))]], big):
            lengths = np.ascontiguousarray(lengths, dtype='f8')
            out = np.full(lengths.size, -1.0)
            _native.check(hip.skm_effective_lengths(0, _native.ptr(fld, _native.c_i64p),
                                                    _native.ptr(lengths, _native.c_f64p), lengths.size,
                                                    _native.ptr(out, _native.c_f64p)))
            if lengths.size == 0:
                continue
            expected = _effective_lengths_ref(fld, lengths)
            if name == 'empty':
                assert np.isnan(expected).all()
            np.testing.assert_array_equal(out, expected, err_msg=name)
    # every special length against the histograms, one transcript at a time
    for name, fld in _histograms(np.random.default_rng(23)).items():
        fld = np.ascontiguousarray(fld, dtype=np.int64)
        out = np.empty(special.size)
        _native.check(hip.skm_effective_lengths(0, _native.ptr(fld, _native.c_i64p),
                                                _native.ptr(special, _native.c_f64p), special.size,
                                                _native.ptr(out, _native.c_f64p)))
        np.testing.assert_array_equal(out, _effective_lengths_ref(fld, special), err_msg=name)
