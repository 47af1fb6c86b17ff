"""The EM of independent components (skm_em.hip: em_local_chunk_kernel; skm_quant_setup.hip: the
components and their tiles) against the whole-table EM on the same handle: with SKM_EM_NO_COMPONENTS
set an EM run steps the whole table with two launches per step, as before the tiles existed.  Every
comparison between the two forms is bit for bit and step for step."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = 'SKM_EM_NO_COMPONENTS'


class _whole_table:
    """Inside: EM runs ignore the tiles (the switch is looked up at every run)."""

    def __enter__(self):
        self.before = os.environ.get(SWITCH)
        os.environ[SWITCH] = '1'

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.before


@pytest.fixture(autouse=True)
def _switch_off_by_default():
    before = os.environ.pop(SWITCH, None)
    yield
    if before is not None:
        os.environ[SWITCH] = before


def _both(quant, x0, l, **kw):
    x, it = quant.em(x0, l, **kw)
    with _whole_table():
        x_ref, it_ref = quant.em(x0, l, **kw)
    assert it == it_ref, (kw, it, it_ref)
    np.testing.assert_array_equal(x, x_ref, err_msg=str(kw))
    return x, it


def _em_inputs(n_tx, rng):
    l = rng.uniform(100, 3000, n_tx)
    x0 = 1.0 / l
    return x0 / x0.sum(), l


def _class_map(offsets, targets):
    return np.vstack([np.repeat(np.arange(offsets.size - 1), np.diff(offsets)), targets]).astype(np.int64)


def _csr(classes):
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int64)
    return offsets, np.concatenate([np.asarray(c, dtype=np.int32) for c in classes]).astype(np.int32)


def _labels(n_tx, offsets, targets):
    """Smallest transcript id of every transcript's component (min-label propagation to a fixed point)."""
    label = np.arange(n_tx, dtype=np.int64)
    cls = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    while True:
        low = np.full(offsets.size - 1, n_tx, dtype=np.int64)
        np.minimum.at(low, cls, label[targets])
        new = label.copy()
        np.minimum.at(new, targets, low[cls])
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def _check_packing(quant, n_tx, offsets, targets, expect_tiles, expect_residual):
    """The packing rule, from what the set-up left on the device."""
    info, label, tile, class_tile = quant.components()
    assert info['built']
    cap_pairs, cap_classes, cap_tx = info['capacity']
    np.testing.assert_array_equal(label, _labels(n_tx, offsets, targets))
    n_tiles = info['tiles']
    lens = np.diff(offsets)
    cls = np.repeat(np.arange(offsets.size - 1), lens)
    # a class lies where its transcripts lie, all of them
    np.testing.assert_array_equal(tile[targets], class_tile[cls])
    # no component is split: one tile (or the residual, n_tx) per label
    first_tile = np.full(n_tx, -1, dtype=np.int64)
    first_tile[label] = tile
    np.testing.assert_array_equal(first_tile[label], tile)
    in_tile = tile < n_tx
    assert ((tile >= 0) & ((tile < n_tiles) | (tile == n_tx))).all()
    # no tile above the capacity; every tile in use
    tx_per_tile = np.bincount(tile[in_tile], minlength=n_tiles)
    assert tx_per_tile.size == n_tiles and (tx_per_tile >= 1).all() and tx_per_tile.max(initial=0) <= cap_tx
    cls_in_tile = class_tile < n_tx
    assert np.bincount(class_tile[cls_in_tile], minlength=n_tiles).max(initial=0) <= cap_classes
    assert np.bincount(class_tile[cls_in_tile], weights=lens[cls_in_tile], minlength=n_tiles).max(initial=0) <= cap_pairs
    # in the residual: exactly the components that exceed a capacity by themselves
    comp_tx = np.bincount(label, minlength=n_tx)
    comp_cls = np.bincount(label[targets[offsets[:-1]]], minlength=n_tx)
    comp_pairs = np.bincount(label[targets[offsets[:-1]]], weights=lens, minlength=n_tx)
    oversize = (comp_tx > cap_tx) | (comp_cls > cap_classes) | (comp_pairs > cap_pairs)
    np.testing.assert_array_equal(tile == n_tx, oversize[label])
    assert info['oversize'] == int(oversize.sum())
    assert (n_tiles > 0) == expect_tiles and (info['oversize'] > 0) == expect_residual
    assert info['em_uses_tiles'] == (n_tiles > 0)
    return info, label, tile


def _genes(rng, n_genes, first_tx, scatter=None):
    """Small ambiguous components: 2-6 transcripts each, 3-10 classes of random subsets."""
    classes, t = [], first_tx
    for _ in range(n_genes):
        n = int(rng.integers(2, 7))
        members = np.arange(t, t + n)
        t += n
        for _ in range(int(rng.integers(3, 11))):
            k = int(rng.integers(1, n + 1))
            classes.append(rng.permutation(members)[:k])
        classes.append(members[:2])
    if scatter is not None:
        classes = [scatter[c] for c in classes]
    return classes, t


def _hub(first_tx, n, shared):
    """One component of n transcripts: a class of its own for each and `shared` classes over all of them."""
    members = np.arange(first_tx, first_tx + n)
    return [[m] for m in members] + [members.copy() for _ in range(shared)], first_tx + n


def _mixed_table(seed, residual_decides):
    """Many small components, one above the tile capacity (200 transcripts), a transcript in no class, a
    class of count 0 and a component that starts from zero abundance (class sums 0: NaN -> 0)."""
    rng = np.random.default_rng(seed)
    if residual_decides:
        # the small ones settle at once (a class of its own per transcript), the large one is ambiguous
        small, t = [], 0
        for _ in range(300):
            small += [[t], [t + 1], [t, t + 1]]
            t += 2
        big = []
        members = np.arange(t, t + 200)
        for _ in range(900):
            big.append(rng.permutation(members)[:int(rng.integers(2, 6))])
        big += [members[i:i + 2] for i in range(199)]              # (a chain: one component for certain)
        t += 200
        counts_small = rng.integers(50, 500, len(small)).astype('f8')
        counts_small[2::3] = 0.0                                   # the shared classes: count 0
        counts_big = rng.integers(1, 40, len(big)).astype('f8')
    else:
        small, t = _genes(rng, 300, 0)
        big, t = _hub(t, 200, 1)
        counts_small = rng.integers(1, 40, len(small)).astype('f8')
        counts_small[rng.integers(0, len(small), 20)] = 0.0        # classes of count 0
        counts_big = np.concatenate([rng.integers(5000, 9000, 200), [1]]).astype('f8')
    zero_from = t                                                  # a component of zero abundance
    zero = [[t, t + 1], [t + 1, t + 2]]
    t += 3
    n_tx = t + 2                                                   # the last two transcripts: in no class
    classes = small + big + zero
    counts = np.concatenate([counts_small, counts_big, [7.0, 3.0]])
    order = rng.permutation(len(classes))                          # caller's class order: shuffled
    offsets, targets = _csr([classes[i] for i in order])
    x0, l = _em_inputs(n_tx, rng)
    x0[zero_from:zero_from + 3] = 0.0
    return n_tx, offsets, targets, counts[order], x0, l


def _deciding_transcript(quant, x0, l, steps, x_floor=1e-8):
    """Where the maximum relative change of the last step lies (whole-table EM, two fixed-step runs)."""
    with _whole_table():
        before, _ = quant.em(x0, l, fixed_iters=steps - 1) if steps > 1 else (np.array(x0), 0)
        after, _ = quant.em(x0, l, fixed_iters=steps)
    change = np.where(after > x_floor, np.abs(after - before) / np.where(after > 0, after, 1.0), -1.0)
    return int(np.argmax(change))


def test_mapped_table_runs_in_tiles_alone(oracle, native_libs):
    from seekmer_amd import common, index_builder, infer, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(4, 60)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 100_000
    bases, offsets = synth.reads(4, pool, tx_offsets, 0, n_units, 100, True)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
    n_tx = len(ids)
    class_offsets, class_targets, counts, _, _ = result.export()
    x0, l = _em_inputs(n_tx, np.random.default_rng(4))
    quant = infer._QuantHandle.from_map_result(result, n_tx)
    try:
        info, _, _ = _check_packing(quant, n_tx, class_offsets, class_targets.astype(np.int64), True, False)
        assert info['oversize'] == 0 and info['em_uses_tiles']        # (else the new kernel is not what runs below)
        x, it = _both(quant, x0, l)
        for fixed in (1, 15, 16, 17, 33):
            assert _both(quant, x0, l, fixed_iters=fixed)[1] == fixed
        assert _both(quant, x0, l, max_iters=40)[1] == min(it, 40)
        x_ref, it_ref = oracle.em(x0, l, _class_map(class_offsets, class_targets), counts.astype('f8'))
        assert it == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
    finally:
        quant.close()


@pytest.mark.parametrize('residual_decides', [False, True])
def test_tiles_and_residual_together(oracle, native_libs, residual_decides):
    from seekmer_amd import infer
    n_tx, offsets, targets, counts, x0, l = _mixed_table(11 + residual_decides, residual_decides)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, label, tile = _check_packing(quant, n_tx, offsets, targets.astype(np.int64), True, True)
        assert info['oversize'] == 1
        x, it = _both(quant, x0, l)
        assert it > 2
        decider = _deciding_transcript(quant, x0, l, it)
        assert (tile[decider] == n_tx) == residual_decides          # the last step's maximum: in the residual / in a tile
        assert (x[-2:] == 0).all() and (x[-5:-2] == 0).all()        # no class; zero class sums (NaN -> 0)
        for fixed in (1, 15, 16, 17, 33):
            assert _both(quant, x0, l, fixed_iters=fixed)[1] == fixed
        cut = max(1, it - 3)
        assert _both(quant, x0, l, max_iters=cut)[1] == cut
        x_ref, it_ref = oracle.em(x0, l, _class_map(offsets, targets), counts)
        assert it == it_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-9, atol=1e-300)
    finally:
        quant.close()


@pytest.mark.parametrize('degree', [513, 1025])
def test_transcript_in_many_classes(native_libs, degree):
    """A transcript in 513 / 1025 classes (two / three rows) is above the tile capacity in classes:
    its component is the residual, the small components beside it run in tiles."""
    from seekmer_amd import infer
    rng = np.random.default_rng(degree)
    small, t = _genes(rng, 40, 0)
    hub = t
    others = np.arange(t + 1, t + 31)
    big = [np.concatenate([[hub], rng.permutation(others)[:int(rng.integers(0, 3))]]) for _ in range(degree)]
    n_tx = t + 31
    classes = small + big
    order = rng.permutation(len(classes))
    offsets, targets = _csr([classes[i] for i in order])
    counts = rng.integers(0, 30, len(classes)).astype('f8')
    x0, l = _em_inputs(n_tx, rng)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, label, tile = _check_packing(quant, n_tx, offsets, targets.astype(np.int64), True, True)
        assert tile[hub] == n_tx
        _both(quant, x0, l)
        for fixed in (1, 16, 17):
            _both(quant, x0, l, fixed_iters=fixed)
    finally:
        quant.close()


def test_one_component_keeps_the_whole_table_em(native_libs):
    from seekmer_amd import infer
    rng = np.random.default_rng(3)
    n_tx = 300
    classes = [[i, i + 1] for i in range(n_tx - 1)] + [rng.permutation(n_tx)[:4] for _ in range(500)]
    offsets, targets = _csr(classes)
    counts = rng.integers(1, 30, len(classes)).astype('f8')
    x0, l = _em_inputs(n_tx, rng)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, _, _ = _check_packing(quant, n_tx, offsets, targets.astype(np.int64), False, True)
        assert info['tiles'] == 0 and not info['em_uses_tiles']
        before = quant.timing()['launches']
        _, it = quant.em(x0, l)
        launches = quant.timing()['launches'] - before
        with _whole_table():
            before = quant.timing()['launches']
            _, it_ref = quant.em(x0, l)
            assert quant.timing()['launches'] - before == launches   # launch for launch
        assert it == it_ref
        _both(quant, x0, l)
    finally:
        quant.close()


@pytest.mark.parametrize('mixed', [False, True])
def test_stopping_on_a_chunk_edge(native_libs, mixed):
    """rel_tol chosen so that the rule is first met on the last step of a chunk (16, 32) and on the
    first step of one (17): the step counts and the results of both forms agree."""
    from seekmer_amd import infer
    rng = np.random.default_rng(5)
    if mixed:
        n_tx, offsets, targets, counts, x0, l = _mixed_table(21, True)
    else:
        # pairs of transcripts told apart by few units and shared by many: slow, steady convergence
        classes, counts = [], []
        for g in range(200):
            classes += [[2 * g], [2 * g + 1], [2 * g, 2 * g + 1]]
            counts += [int(rng.integers(1, 6)), int(rng.integers(1, 6)), int(rng.integers(50, 500))]
        n_tx = 400
        offsets, targets = _csr(classes)
        counts = np.array(counts, dtype='f8')
        x0, l = _em_inputs(n_tx, rng)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        assert quant.components(arrays=False)[0]['em_uses_tiles']
        assert (quant.components(arrays=False)[0]['oversize'] > 0) == mixed
        with _whole_table():
            xs = [np.array(x0)] + [quant.em(x0, l, fixed_iters=k)[0] for k in range(1, 34)]
        biggest = []
        for k in range(1, 34):
            keep = xs[k] > 1e-8
            biggest.append((np.abs(xs[k] - xs[k - 1])[keep] / xs[k][keep]).max())
        for steps in (16, 17, 32):
            earlier = min(biggest[:steps - 1])
            assert biggest[steps - 1] < earlier                      # (else no tolerance stops exactly here)
            tol = 0.5 * (biggest[steps - 1] + earlier)
            assert _both(quant, x0, l, rel_tol=tol)[1] == steps
    finally:
        quant.close()


@pytest.mark.parametrize('mixed', [False, True])
def test_set_counts_then_em_equals_a_fresh_handle(native_libs, mixed):
    from seekmer_amd import infer
    rng = np.random.default_rng(8)
    if mixed:
        n_tx, offsets, targets, counts, x0, l = _mixed_table(31, False)
    else:
        classes, n_tx = _genes(rng, 150, 0, scatter=rng.permutation(1200))
        n_tx = 1200
        offsets, targets = _csr(classes)
        counts = rng.integers(1, 40, len(classes)).astype('f8')
        x0, l = _em_inputs(n_tx, rng)
    other = rng.integers(0, 60, counts.size).astype('f8')
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    fresh = infer._QuantHandle.from_csr(n_tx, offsets, targets, other)
    try:
        assert quant.components(arrays=False)[0]['em_uses_tiles']
        _both(quant, x0, l)
        quant.set_counts(other)
        x, it = _both(quant, x0, l)
        x_fresh, it_fresh = fresh.em(x0, l)
        assert it == it_fresh
        np.testing.assert_array_equal(x, x_fresh)
    finally:
        quant.close()
        fresh.close()
