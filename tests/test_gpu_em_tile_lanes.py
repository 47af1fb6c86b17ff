"""The lanes of the tile EM (skm_em.hip: em_local_chunk_kernel): class tuples taken in batches of
EM_TILE_CLASS_BATCH entries, a tile's classes listed by their number of batches (skm_quant_setup.hip),
and the stop without a replayed chunk -- every step's abundances are kept, and the launch that finds the
EM stopped copies the tiles' entries of that step.  As in test_gpu_em_components.py every comparison is
the tile run against the SKM_EM_NO_COMPONENTS=1 run on the same handle, bit for bit and step for step;
one run per table is compared with the oracle."""
import numpy as np
import pytest

from test_gpu_em_components import (_both, _check_packing, _class_map, _csr, _em_inputs, _mixed_table,
                                    _switch_off_by_default, _whole_table)   # noqa: F401 (the fixture is autouse)

pytestmark = pytest.mark.gpu

BATCH_EDGE_LENGTHS = {40: 3, 17: 5, 16: 5, 15: 5, 9: 10, 8: 10, 7: 10, 5: 30, 4: 40, 3: 50, 2: 60, 1: 60}


def _tuple_length_table(seed=17):
    """One tile: a component of 60 transcripts in 288 classes (two passes of the 256 lanes) whose tuple
    lengths lie around the batch width, a component that starts at zero abundance, a transcript in no
    class; some classes of count 0; the caller's class order shuffled."""
    rng = np.random.default_rng(seed)
    members = np.arange(60)
    classes = []
    for length, n in BATCH_EDGE_LENGTHS.items():
        for k in range(n):
            if length == 2 and k < 59:
                classes.append(np.array([k, k + 1]))               # (a chain: one component for certain)
            else:
                classes.append(rng.permutation(members)[:length])
    zero_from = 60
    classes += [np.array([60, 61]), np.array([61, 62])]
    n_tx = 64                                                      # transcript 63: in no class
    counts = rng.integers(1, 40, len(classes)).astype('f8')
    counts[rng.integers(0, len(classes) - 2, 25)] = 0.0
    order = rng.permutation(len(classes))
    offsets, targets = _csr([classes[i] for i in order])
    x0, l = _em_inputs(n_tx, rng)
    x0[zero_from:zero_from + 3] = 0.0
    return n_tx, offsets, targets, counts[order], x0, l


def _row_length_table(seed=23):
    """One tile: transcripts 0..6 lie in 1, 7, 8, 9, 16, 17 and 60 classes (the eight lanes of a row take
    one, two, three and eight turns), each class shared with at most one of the transcripts 7..39."""
    rng = np.random.default_rng(seed)
    degrees = (1, 7, 8, 9, 16, 17, 60)
    classes = []
    for t, degree in enumerate(degrees):
        for k in range(degree):
            other = int(rng.integers(7, 40))
            classes.append([np.array([t]), np.array([t, other]), np.array([other, t])][k % 3])
    classes += [np.array([i, i + 1]) for i in range(7, 39)]
    n_tx = 40
    counts = rng.integers(0, 40, len(classes)).astype('f8')
    order = rng.permutation(len(classes))
    offsets, targets = _csr([classes[i] for i in order])
    x0, l = _em_inputs(n_tx, rng)
    return n_tx, offsets, targets, counts[order], x0, l, degrees


def _slow_pairs_table(seed=5):
    """test_stopping_on_a_chunk_edge's table: 200 pairs of transcripts told apart by few units and shared
    by many (slow, steady convergence); 400 transcripts, tiles alone."""
    rng = np.random.default_rng(seed)
    classes, counts = [], []
    for g in range(200):
        classes += [[2 * g], [2 * g + 1], [2 * g, 2 * g + 1]]
        counts += [int(rng.integers(1, 6)), int(rng.integers(1, 6)), int(rng.integers(50, 500))]
    offsets, targets = _csr(classes)
    x0, l = _em_inputs(400, rng)
    return 400, offsets, targets, np.array(counts, dtype='f8'), x0, l


def test_tuple_lengths_around_the_batch_width(oracle, native_libs):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l = _tuple_length_table()
    assert set(np.diff(offsets)) == set(BATCH_EDGE_LENGTHS)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        # (the packing as the set-up left it: listing the classes by length moved none to another tile)
        info, label, tile = _check_packing(quant, n_tx, offsets, targets.astype(np.int64), True, False)
        assert info['tiles'] == 1 and offsets.size - 1 > 256           # one tile, two passes over its classes
        assert np.unique(label).size == 3                              # the 60, the one that starts at zero, no class
        for fixed in (1, 2):
            assert _both(quant, x0, l, fixed_iters=fixed)[1] == fixed
        x, it = _both(quant, x0, l)
        assert it > 2 and (x[60:] == 0).all()
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts)
        assert it == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
    finally:
        quant.close()


def test_rows_around_the_lane_group(oracle, native_libs):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l, degrees = _row_length_table()
    np.testing.assert_array_equal(np.bincount(targets, minlength=n_tx)[:len(degrees)], degrees)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, _, _ = _check_packing(quant, n_tx, offsets, targets.astype(np.int64), True, False)
        assert info['tiles'] == 1
        for fixed in (1, 2):
            assert _both(quant, x0, l, fixed_iters=fixed)[1] == fixed
        x, it = _both(quant, x0, l)
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts)
        assert it == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
    finally:
        quant.close()


def _stop_table(mixed):
    return _mixed_table(21, True) if mixed else _slow_pairs_table()


def _again_with_other_counts(quant, infer, table, other, **kw):
    """The same run after set_counts(other) against a handle that has never run anything: the snapshots of
    the run before must not show; the first counts are put back."""
    n_tx, offsets, targets, counts, x0, l = table
    quant.set_counts(other)
    x, it = _both(quant, x0, l, **kw)
    fresh = infer._QuantHandle.from_csr(n_tx, offsets, targets, other)
    try:
        x_fresh, it_fresh = fresh.em(x0, l, **kw)
    finally:
        fresh.close()
    assert it == it_fresh, (kw, it, it_fresh)
    np.testing.assert_array_equal(x, x_fresh, err_msg=str(kw))
    quant.set_counts(counts)


@pytest.mark.parametrize('mixed', [False, True])
def test_max_iters_at_every_place_of_a_chunk(oracle, native_libs, mixed):
    from seekmer_amd import infer
    table = _stop_table(mixed)
    n_tx, offsets, targets, counts, x0, l = table
    other = np.random.default_rng(77).integers(0, 60, counts.size).astype('f8')
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info = quant.components(arrays=False)[0]
        assert info['em_uses_tiles'] and (info['oversize'] > 0) == mixed
        x, unbounded = _both(quant, x0, l)
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts)
        assert unbounded == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
        for k in range(1, 35):
            assert _both(quant, x0, l, max_iters=k)[1] == min(k, unbounded)
            _again_with_other_counts(quant, infer, table, other, max_iters=k)
    finally:
        quant.close()


@pytest.mark.parametrize('mixed', [False, True])
def test_rel_tol_stops_inside_a_chunk(native_libs, mixed):
    """rel_tol between consecutive maxima of the relative change, so that the rule is first met 5, 21 and
    30 steps in: inside the first and the second chunk, never on a chunk's edge."""
    from seekmer_amd import infer
    table = _stop_table(mixed)
    n_tx, offsets, targets, counts, x0, l = table
    other = np.random.default_rng(78).integers(0, 60, counts.size).astype('f8')
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        with _whole_table():
            xs = [np.array(x0)] + [quant.em(x0, l, fixed_iters=k)[0] for k in range(1, 32)]
        biggest = []
        for k in range(1, 32):
            keep = xs[k] > 1e-8
            biggest.append((np.abs(xs[k] - xs[k - 1])[keep] / xs[k][keep]).max())
        isolated = 0
        for steps in (5, 21, 30):
            earlier = min(biggest[:steps - 1])
            if not biggest[steps - 1] < earlier:
                continue                                               # (no tolerance stops exactly here)
            isolated += 1
            tol = 0.5 * (biggest[steps - 1] + earlier)
            assert _both(quant, x0, l, rel_tol=tol)[1] == steps
            _again_with_other_counts(quant, infer, table, other, rel_tol=tol)
        assert isolated > 0
    finally:
        quant.close()
