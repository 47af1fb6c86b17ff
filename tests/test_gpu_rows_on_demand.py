"""The whole table's transcript-major rows are built when a reader first asks (skm_abi_quant.hip: QuantRowsHolder),
not with the class views: the tile set-up makes a tile's views from the tile's own classes (tile_build_kernel) and
the tile EM reads no row.  skm_quant_rows_built says whether a handle holds them.  Here: which handles build them
and when; a table whose classes name a transcript more than once, every tile array against the reference; and on
a mapped table the batched drivers as the first reader of the rows against a handle that had them already."""
import os

import numpy as np
import pytest

import repeated_members_reference as M
import tile_list_reference as R
from test_gpu_em_components import SWITCH, _both, _em_inputs, _switch_off_by_default, _whole_table   # noqa: F401 (the fixture is autouse)
from test_gpu_em_tile_runs import _built_for
from test_gpu_tile_build import _check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(R.TABLES))
def test_rows_are_built_by_their_first_reader(native_libs, name):
    from seekmer_amd import infer
    segment, capacity = _built_for(infer)
    n_tx, offsets, targets, counts = R.TABLES[name](segment, capacity)
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info = quant.components(arrays=False)[0]
        tiles_alone = info['tiles'] > 0 and info['oversize'] == 0
        assert tiles_alone == (name not in ('oversize', 'one_oversize_component'))
        # (a residual is cut out of the rows at the set-up; a table without tiles has them from its first EM)
        assert quant.rows_built() == (name == 'oversize')
        x0, l = _em_inputs(n_tx, np.random.default_rng(3))
        x, it = quant.em(x0, l)
        assert info['em_uses_tiles'] == (name != 'one_oversize_component')
        assert quant.rows_built() == (not tiles_alone)
        x_both, it_both = _both(quant, x0, l)                # (the whole-table EM on the same handle: bit for bit)
        assert quant.rows_built()
        assert it_both == it
        np.testing.assert_array_equal(x_both, x)
        x_again, it_again = quant.em(x0, l)                  # the tiles again, beside rows that are there now
        assert it_again == it
        np.testing.assert_array_equal(x_again, x)
    finally:
        quant.close()


def test_repeated_member(native_libs):
    """Classes that name a transcript twice and three times: the transcript's degree counts every naming, its row
    holds the class as often, in tuple order.  tile_list_reference.py states repeated members (CPU:
    test_repeated_members_reference.py), so every tile array is compared, and the tile EM against the whole-table EM,
    whose rows cut transcript 0's 520 pairs in two."""
    from seekmer_amd import infer
    n_tx, offsets, targets, counts = M.repeated_member_table()
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
    try:
        info, got, ref = _check(native_libs, quant, n_tx, offsets, targets.astype(np.int64))
        assert info['tiles'] == 1 and info['oversize'] == 0 and info['em_uses_tiles']
        assert info['capacity'][0] >= 783 and info['capacity'][1] >= 261 and info['capacity'][2] >= 101
        assert ref['degree'][0] == 520 > M.ROW_CAP and got['tx_list'][0] == 0
        assert not quant.rows_built()
        x0, l = _em_inputs(n_tx, np.random.default_rng(9))
        _both(quant, x0, l)
        assert _both(quant, x0, l, fixed_iters=17)[1] == 17
        assert quant.rows_built()
    finally:
        quant.close()


@pytest.fixture(scope='module')
def mapped():
    from seekmer_amd import common, index_builder, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(7, 63)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 500 * 63
    bases, offsets = synth.reads(7, pool, tx_offsets, 0, n_units, 100, True)
    result = mapper.MapResult(index)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_units, bases, offsets, True))
    return result, len(ids)


def _first_use_against_built(result, n_tx, use):
    """use(quant) on a fresh handle, where it is the first reader of the rows, and on a handle whose whole-table EM
    ran before."""
    from seekmer_amd import infer
    x0, l = _em_inputs(n_tx, np.random.default_rng(11))
    fresh = infer._QuantHandle.from_map_result(result, n_tx)
    try:
        assert fresh.components(arrays=False)[0]['em_uses_tiles'] and not fresh.rows_built()
        first = use(fresh, x0, l)
        assert fresh.rows_built()
    finally:
        fresh.close()
    built = infer._QuantHandle.from_map_result(result, n_tx)
    try:
        with _whole_table():
            built.em(x0, l)
        assert built.rows_built()
        second = use(built, x0, l)
    finally:
        built.close()
    assert len(first) == len(second)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)


def test_bootstrap_as_the_first_reader(native_libs, mapped):
    result, n_tx = mapped

    def use(quant, x0, l):
        out, _, iters = quant.bootstrap(3, 5, x0, l)
        return out, iters
    _first_use_against_built(result, n_tx, use)


def test_em_many_as_the_first_reader(native_libs, mapped):
    result, n_tx = mapped
    n_classes = result.sizes()[0]
    counts = np.random.default_rng(13).integers(0, 40, (3, n_classes)).astype('f8')

    def use(quant, x0, l):
        return quant.em_many(counts, x0, l)
    _first_use_against_built(result, n_tx, use)


def test_resident_quantification_with_and_without_tiles(native_libs, mapped):
    from seekmer_amd import infer
    result, _ = mapped
    tpm, iters = infer.quantify_resident(result, return_iters=True)
    os.environ[SWITCH] = '1'
    try:
        tpm_whole, iters_whole = infer.quantify_resident(result, return_iters=True)
    finally:
        del os.environ[SWITCH]
    assert iters == iters_whole and iters > 0
    assert tpm.tobytes() == tpm_whole.tobytes()
