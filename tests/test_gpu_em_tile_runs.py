"""The tiles of the tile EM as the set-up packs them (skm_quant_setup.hip: tile_pack_kernel, one wave per
run of transcript ids) against the packing rule restated in plain Python (tile_pack_reference.py).  The
run length and the capacities are the library's (skm_quant_components), and the hand-made tables are laid
out from them (a table that the built values leave no room for says so by an assertion of its own); every
comparison of tiles is exact."""
import numpy as np
import pytest

from test_gpu_em_components import _both, _csr, _em_inputs, _switch_off_by_default   # noqa: F401 (the fixture is autouse)
from tile_pack_reference import component_sizes, labels, tile_table

pytestmark = pytest.mark.gpu


def _exported(quant, n_tx, offsets):
    """(info, tx_tile, the tiles' starts in transcripts, classes and pairs) from what the set-up left on the device."""
    info, _, tile, class_tile = quant.components()
    assert info['built'] and info['segment'] > 0
    n_tiles = info['tiles']
    tile, class_tile = tile.astype(np.int64), class_tile.astype(np.int64)
    assert ((tile >= 0) & ((tile < n_tiles) | (tile == n_tx))).all()
    assert ((class_tile >= 0) & ((class_tile < n_tiles) | (class_tile == n_tx))).all()
    lens = np.diff(offsets)

    def starts(of, weights=None):
        inside = of < n_tx
        per_tile = np.bincount(of[inside], weights=None if weights is None else weights[inside], minlength=n_tiles)
        return np.concatenate([[0], np.cumsum(per_tile.astype(np.int64))])

    return info, tile, starts(tile), starts(class_tile), starts(class_tile, lens)


def _check_tiles(quant, n_tx, offsets, targets):
    """Exact equality of the device's tiles with the rule's; returns (info, the rule's cuts)."""
    info, tile, tx_start, cls_start, pair_start = _exported(quant, n_tx, offsets)
    want_tile, want_tx, want_cls, want_pairs, want_oversize, cuts = tile_table(
        n_tx, offsets, targets, info['segment'], info['capacity'])
    np.testing.assert_array_equal(tile, want_tile)
    assert info['tiles'] == want_tx.size - 1 and info['oversize'] == want_oversize
    np.testing.assert_array_equal(tx_start, want_tx)
    np.testing.assert_array_equal(cls_start, want_cls)
    np.testing.assert_array_equal(pair_start, want_pairs)
    return info, cuts


@pytest.mark.parametrize('seed,genes,n_tx', [(7, 63, 604), (4, 26, 256)])
def test_tiles_of_a_mapped_table_equal_the_serial_rule(native_libs, seed, genes, n_tx):
    """604 transcripts: runs of 256 ids with a partial last run; 256: one run, full to its last id."""
    from seekmer_amd import common, index_builder, infer, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(seed, genes)
    assert len(ids) == n_tx
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 500 * genes
    bases, offsets = synth.reads(seed, pool, tx_offsets, 0, n_units, 100, True)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
    class_offsets, class_targets, _, _, _ = result.export()
    quant = infer._QuantHandle.from_map_result(result, n_tx)
    try:
        info, cuts = _check_tiles(quant, n_tx, class_offsets, class_targets.astype(np.int64))
        assert info['em_uses_tiles'] and info['oversize'] == 0
        assert info['tiles'] >= -(-n_tx // info['segment'])             # (a tile does not cross runs)
        x0, l = _em_inputs(n_tx, np.random.default_rng(seed))
        _both(quant, x0, l)
    finally:
        quant.close()


def _built_for(infer):
    """(ids per packing run, capacity) of the library in use."""
    quant = infer._QuantHandle.from_csr(2, *_csr([[0, 1]]), np.ones(1))
    try:
        info = quant.components(arrays=False)[0]
    finally:
        quant.close()
    return info['segment'], info['capacity']


def _chain(first, n):
    """One component of n transcripts in n - 1 classes of two."""
    return [[t, t + 1] for t in range(first, first + n - 1)] if n > 1 else [[first]]


def _every_cut_table(segment, capacity, seed=41):
    """Run 0 holds, in id order: four chains of which three fill a tile in transcripts (a cut by
    transcripts); components of two transcripts in many one-entry classes (a cut by classes); components
    whose few classes name all their transcripts (a cut by pairs); a transcript in cap_pairs + 1 classes
    of its own (above the capacity: the residual); the ids left are one chain.  Run 1: chains of cap_tx
    transcripts, a chain of cap_tx - 1 brought to cap_classes - 12 classes, and as the run's last id a
    transcript in 13 classes: the run's last tile holds it alone.  Run 2: small random components and, last, three
    transcripts in no class."""
    cap_pairs, cap_classes, cap_tx = capacity
    rng = np.random.default_rng(seed)
    classes, t = [], 0
    a = cap_tx * 5 // 16                                  # 3 a <= cap_tx < 4 a
    for _ in range(4):
        classes += _chain(t, a)
        t += a
    m = cap_classes * 25 // 64                            # (a - 1) + 2 m <= cap_classes < (a - 1) + 3 m
    for _ in range(3):
        classes += [[t, t + 1]] + [[t]] * ((m - 1) // 2) + [[t + 1]] * (m - 1 - (m - 1) // 2)
        t += 2
    q = cap_pairs * 75 // 256                             # (m + 1) + 3 q <= cap_pairs < (m + 1) + 4 q
    u = min(20, (segment - t - 4) // 4)                   # transcripts of such a component: all four lie in run 0
    assert u >= 2
    for _ in range(4):
        members = list(range(t, t + u))
        classes += [members] * (q // u)
        t += u
    hub = t
    classes += [[hub]] * (cap_pairs + 1)
    t += 1
    assert t < segment
    classes += _chain(t, segment - t)
    t = segment
    w = min(cap_tx - 1, segment - 1)
    assert w >= 2 and w - 1 <= cap_classes - 12
    while t < 2 * segment - 1 - w:
        n = min(cap_tx, 2 * segment - 1 - w - t)
        classes += _chain(t, n)
        t += n
    classes += _chain(t, w) + [[t]] * (cap_classes - 12 - (w - 1))
    t += w
    alone = t
    assert alone == 2 * segment - 1
    classes += [[alone]] * 13
    t += 1
    while t < 2 * segment + 180:
        n = int(rng.integers(2, 7))
        members = np.arange(t, t + n)
        classes += [list(rng.permutation(members)[:int(rng.integers(1, n + 1))]) for _ in range(int(rng.integers(3, 11)))]
        classes += _chain(t, n)
        t += n
    n_tx = t + 3
    counts = rng.integers(1, 40, len(classes)).astype('f8')
    order = rng.permutation(len(classes))
    offsets, targets = _csr([classes[i] for i in order])
    x0, l = _em_inputs(n_tx, rng)
    return n_tx, offsets, targets, counts[order], x0, l, hub, alone


def test_a_run_with_every_kind_of_cut(native_libs):
    from seekmer_amd import infer
    segment, capacity = _built_for(infer)
    n_tx, offsets, targets, counts, x0, l, hub, alone = _every_cut_table(segment, capacity)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, cuts = _check_tiles(quant, n_tx, offsets, targets.astype(np.int64))
        _, tile, tx_start, cls_start, pair_start = _exported(quant, n_tx, offsets)
        assert info['em_uses_tiles'] and info['oversize'] == 1 and tile[hub] == n_tx
        # the cuts counted from the exported tiles: tile k ends on a capacity when its fill and the first
        # component of tile k + 1 (of the same run) together exceed it
        label_of = {}
        for t in range(n_tx):
            if tile[t] < n_tx:
                label_of.setdefault(int(tile[t]), t)                 # (a component's smallest id comes first)
        kinds = {'pairs': 0, 'classes': 0, 'tx': 0}
        in_run_0, counted = set(), []
        cap_pairs, cap_classes, cap_tx = info['capacity']
        label = labels(n_tx, offsets, targets)
        c_tx, c_pairs, c_classes = component_sizes(n_tx, offsets, targets, label)
        for k in range(info['tiles'] - 1):
            first = label_of[k + 1]
            if first // info['segment'] != label_of[k] // info['segment']:
                continue                                             # (tile k + 1 begins a run)
            found = set()
            if pair_start[k + 1] - pair_start[k] + c_pairs[first] > cap_pairs:
                found.add('pairs')
            if cls_start[k + 1] - cls_start[k] + c_classes[first] > cap_classes:
                found.add('classes')
            if tx_start[k + 1] - tx_start[k] + c_tx[first] > cap_tx:
                found.add('tx')
            assert found
            counted.append((k + 1, found))
            for kind in found:
                kinds[kind] += 1
            if first < info['segment'] and len(found) == 1:
                in_run_0 |= found
        assert min(kinds.values()) >= 1, kinds
        assert in_run_0 == {'pairs', 'classes', 'tx'}                # each kind by itself within one run
        assert counted == [(at, found) for _, at, found in cuts]     # (what the rule itself says of every cut)
        # the last tile of run 1 holds one transcript
        assert (tile == tile[alone]).sum() == 1 and tile[alone] + 1 == tile[alone + 1]
        # the EM in tiles + residual against the whole-table EM: abundances and step count bit for bit
        x, it = _both(quant, x0, l)
        assert it > 2
        for fixed in (1, 16, 17):
            assert _both(quant, x0, l, fixed_iters=fixed)[1] == fixed
    finally:
        quant.close()


@pytest.mark.parametrize('last_run', [64, 65, 128, 129])
def test_last_run_ends_at_a_wave_border(native_libs, last_run):
    """The ids of the last run fill one / two waves of the walk exactly, or one more; components of 1-6
    transcripts in 1 % to 12 % of cap_classes classes, so that tiles end (on classes, mostly) every 50 ids
    or so, anywhere in a wave."""
    from seekmer_amd import infer
    segment, (_, cap_classes, _) = _built_for(infer)
    n_tx = segment + last_run
    rng = np.random.default_rng(last_run)
    classes, t = [], 0
    while t < n_tx:
        n = min(int(rng.integers(1, 7)), n_tx - t)
        members = np.arange(t, t + n)
        classes += _chain(t, n)
        classes += [list(rng.permutation(members)[:int(rng.integers(1, n + 1))]) for _ in range(int(rng.integers(cap_classes // 100, cap_classes // 8 - 3)))]
        t += n
    counts = rng.integers(1, 40, len(classes)).astype('f8')
    order = rng.permutation(len(classes))
    offsets, targets = _csr([classes[i] for i in order])
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, cuts = _check_tiles(quant, n_tx, offsets, targets.astype(np.int64))
        assert info['em_uses_tiles'] and info['oversize'] == 0
        assert any(run == 1 for run, _, _ in cuts)                     # (the last run holds more than one tile)
        x0, l = _em_inputs(n_tx, rng)
        assert _both(quant, x0, l, fixed_iters=17)[1] == 17
    finally:
        quant.close()
