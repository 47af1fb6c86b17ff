"""The schedule of the tile EM's launches (skm_em.hip: em_local_chunk_kernel): the tiles launched largest
first (skm_quant_setup.hip: tile_order_kernel; SKM_EM_TILE_ORDER=identity|reverse are the other orders),
and a chunk of tiles alone judged by the chunk launch itself -- the workgroup that arrives last applies
the stopping rule to the chunk's steps (em_tile_arrive, em_tiles_judge).  As in
test_gpu_em_components.py every comparison is the tile run against the SKM_EM_NO_COMPONENTS=1 run on the
same handle, bit for bit and step for step; one run per table is compared with the oracle."""
import os

import numpy as np
import pytest

from test_gpu_em_components import (_both, _check_packing, _class_map, _csr, _em_inputs,
                                    _switch_off_by_default, _whole_table)   # noqa: F401 (the fixture is autouse)
from test_gpu_em_tile_lanes import _slow_pairs_table

pytestmark = pytest.mark.gpu

ORDER = 'SKM_EM_TILE_ORDER'


class _order:
    """Inside: the tiles are launched in this order (None: the set-up's; looked up at every run)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.before = os.environ.pop(ORDER, None)
        if self.form is not None:
            os.environ[ORDER] = self.form

    def __exit__(self, *exc):
        os.environ.pop(ORDER, None)
        if self.before is not None:
            os.environ[ORDER] = self.before


def _tiles_alone(quant):
    info = quant.components(arrays=False)[0]
    assert info['em_uses_tiles'] and info['oversize'] == 0 and info['tiles'] > 0
    return info


def _pair_components(first, n, rng):
    """n components of two transcripts from id `first` on: a class of its own for each and one for both."""
    classes = []
    for g in range(n):
        a = first + 2 * g
        classes += [[a], [a + 1], [a, a + 1]]
    return classes, list(rng.integers(1, 60, 3 * n))


def _sized_tiles_table(seed=41):
    """Four runs of 256 ids and one id more.  Run 0: a component of 100 transcripts and 2028 pairs (a chain
    and 366 classes of five), then 78 components of two; runs 1 and 2: 128 components of two each -- two
    tiles of 256 pairs a run, all four of one size; run 3: 254 transcripts in no class and one component of
    two -- a tile without a pair and one of four pairs; the last id: in no class, a tile by itself."""
    rng = np.random.default_rng(seed)
    members = np.arange(100)
    classes = [[i, i + 1] for i in range(99)] + [rng.permutation(members)[:5] for _ in range(366)]
    counts = list(rng.integers(1, 40, len(classes)))
    for first, n in ((100, 78), (256, 128), (512, 128), (1022, 1)):
        more, more_counts = _pair_components(first, n, rng)
        classes += more
        counts += more_counts
    n_tx = 4 * 256 + 1
    order = rng.permutation(len(classes))                          # caller's class order: shuffled
    offsets, targets = _csr([classes[i] for i in order])
    x0, l = _em_inputs(n_tx, rng)
    return n_tx, offsets, targets, np.array(counts, dtype='f8')[order], x0, l


def test_results_do_not_depend_on_the_launch_order(oracle, native_libs):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l = _sized_tiles_table()
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, _, tile = _check_packing(quant, n_tx, offsets, targets.astype(np.int64), True, False)
        _, _, _, class_tile = quant.components()
        n_tiles, cap_pairs = info['tiles'], info['capacity'][0]
        pairs = np.bincount(class_tile, weights=np.diff(offsets), minlength=n_tiles).astype(np.int64)
        tx = np.bincount(tile, minlength=n_tiles)
        print('pairs of the tiles:', pairs.tolist(), 'transcripts:', tx.tolist())
        assert n_tiles >= 5
        assert pairs.max() >= 0.95 * cap_pairs                          # one near the pair capacity
        assert ((pairs > 0) & (pairs <= 8)).any()                       # one of a few pairs
        assert pairs[tile[n_tx - 1]] == 0 and tx[tile[n_tx - 1]] == 1   # one that is a transcript in no class
        sizes, times = np.unique(pairs[pairs > 0], return_counts=True)
        assert (times >= 2).any()                                       # a tie
        assert sizes.size >= 4                                          # clearly different sizes
        for kw in ({}, {'fixed_iters': 17}, {'max_iters': 20}):
            x, it = _both(quant, x0, l, **kw)                           # (the set-up's order, and the whole table)
            for form in ('identity', 'reverse'):
                with _order(form):
                    x_form, it_form = quant.em(x0, l, **kw)
                assert it_form == it, (form, kw)
                np.testing.assert_array_equal(x_form, x, err_msg='%s %s' % (form, kw))
        x, it = _both(quant, x0, l)
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts)
        assert it == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
        with _order('largest'), pytest.raises(ValueError):              # (not one of the two names)
            quant.em(x0, l)
        _both(quant, x0, l, fixed_iters=3)
    finally:
        quant.close()


def test_chunk_edges_through_the_judge_in_the_chunk_launch(oracle, native_libs):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l = _slow_pairs_table()
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        _tiles_alone(quant)
        for fixed in (1, 15, 16, 17, 32, 33):                           # (33: three chunks, the words used a third time)
            assert _both(quant, x0, l, fixed_iters=fixed)[1] == fixed
        x, it = _both(quant, x0, l)                                     # the free-running stop
        assert it > 33
        for cut in (16, 17):
            assert _both(quant, x0, l, max_iters=cut)[1] == cut
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts)
        assert it == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
        # one launch a chunk and none beside it: the chunks that step, and the one that copies the result
        before = quant.timing()['launches']
        quant.em(x0, l, fixed_iters=33)
        assert quant.timing()['launches'] - before == 4
    finally:
        quant.close()


def _fading_table(seed=9):
    """200 components of two transcripts of one length, most units shared; the start favours the one with
    fewer units of its own, which loses its share slowly: the largest abundance falls with every step."""
    rng = np.random.default_rng(seed)
    classes, counts, l = [], [], []
    for g in range(200):
        classes += [[2 * g], [2 * g + 1], [2 * g, 2 * g + 1]]
        counts += [int(rng.integers(1, 4)), int(rng.integers(6, 11)), int(rng.integers(1500, 2500))]
        l += [float(rng.uniform(500, 3000))] * 2
    offsets, targets = _csr(classes)
    x0 = np.tile([9.0, 1.0], 200)
    return 400, offsets, targets, np.array(counts, dtype='f8'), x0 / x0.sum(), np.array(l)


def test_no_abundance_above_the_floor_raises_as_the_whole_table_does(native_libs):
    """x_floor between the largest abundances of steps k - 1 and k: step k is the first without an abundance
    above it -- the first step of a chunk (1, 17) and later ones (7, 20)."""
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l = _fading_table()
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        _tiles_alone(quant)
        with _whole_table():
            tops = [float(x0.max())] + [float(quant.em(x0, l, fixed_iters=k)[0].max()) for k in range(1, 21)]
        assert all(after < before for before, after in zip(tops[1:], tops[2:]))     # (else no floor isolates a step)
        for k in (1, 7, 17, 20):
            floor = 2.0 * tops[1] if k == 1 else 0.5 * (tops[k - 1] + tops[k])
            kw = dict(x_floor=floor, rel_tol=1e-30)
            if k > 1:
                assert _both(quant, x0, l, max_iters=k - 1, **kw)[1] == k - 1       # (defined up to the step before)
            for whole in (True, False):
                with pytest.raises(native_libs.NativeError) as raised:
                    if whole:
                        with _whole_table():
                            quant.em(x0, l, **kw)
                    else:
                        quant.em(x0, l, **kw)
                assert raised.value.code == native_libs.SKM_ERR_UNDEFINED, (k, whole)
            _both(quant, x0, l, fixed_iters=18)                                     # (nothing is left behind)
    finally:
        quant.close()


def test_one_handle_several_runs(native_libs):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l = _slow_pairs_table()
    runs = (dict(max_iters=21), dict(), dict(fixed_iters=1), dict(max_iters=40))     # (21: stops inside a chunk)
    fresh_results = []
    for kw in runs:
        fresh = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
        try:
            fresh_results.append(fresh.em(x0, l, **kw))
        finally:
            fresh.close()
    assert fresh_results[0][1] == 21 and fresh_results[2][1] == 1
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        _tiles_alone(quant)
        for kw, (x_fresh, it_fresh) in zip(runs, fresh_results):
            x, it = _both(quant, x0, l, **kw)
            assert it == it_fresh, kw
            np.testing.assert_array_equal(x, x_fresh, err_msg=str(kw))
    finally:
        quant.close()


def test_more_tiles_than_are_resident_at_once(oracle, native_libs):
    """2048 runs of 256 ids, in each a chain of six transcripts and 250 in no class: two tiles a run, 4096
    in all against the 7 x 256 = 1792 workgroups a launch has resident -- the last to arrive comes from a
    later round."""
    from seekmer_amd import infer
    rng = np.random.default_rng(12)
    runs = 2048
    n_tx = runs * 256
    first = np.arange(runs, dtype=np.int64) * 256 + rng.integers(0, 250, runs)
    link = first[:, None] + np.arange(5)[None, :]                      # classes (t, t + 1): 5 a run
    targets = np.stack([link, link + 1], axis=2).reshape(-1).astype(np.int32)
    offsets = np.arange(0, targets.size + 1, 2, dtype=np.int64)
    counts = rng.integers(1, 50, offsets.size - 1).astype('f8')
    x0, l = _em_inputs(n_tx, rng)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info = _tiles_alone(quant)
        assert info['tiles'] > 1792
        x, it = _both(quant, x0, l, fixed_iters=17)
        assert it == 17
        with _order('reverse'):
            x_reverse, it_reverse = quant.em(x0, l, fixed_iters=17)
        assert it_reverse == 17
        np.testing.assert_array_equal(x_reverse, x)
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts, fixed_iters=17)
        assert it_ref == 17
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
    finally:
        quant.close()
