"""The host side of the many-problems EM (skm_quant_em_many, skm_quant_em_blend): what needs no GPU."""
import ctypes
import types

import numpy as np
import pytest


def _summaries(n_cells, n_tx, seed):
    """Stand-ins for mapper.SummarizedResult: what blend() and requantify_blend read of one."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cells):
        n_classes = int(rng.integers(3, 40))
        sizes = rng.integers(1, 5, n_classes)
        class_map = np.vstack([np.repeat(np.arange(n_classes), sizes), rng.integers(0, n_tx, int(sizes.sum()))]).astype(np.int64)
        out.append(types.SimpleNamespace(class_map=class_map, class_count=rng.integers(1, 5000, n_classes).astype('f8'),
                                         effective_lengths=np.linspace(100.0, 900.0, n_tx)))
    return out


def test_blend_sources_reproduce_blend():
    """((own * weight[i, cell]) * total[i]) / total[cell] -- the formula the device kernel evaluates -- in
    numpy, from the (class_cell, cell_total) that requantify_blend hands over: blend()'s vectors, bit for bit."""
    from seekmer_amd import impute
    summaries = _summaries(13, 50, 1)
    rng = np.random.default_rng(2)
    weight = rng.uniform(0.0, 1.0, (13, 13)) ** 16
    weight[rng.random((13, 13)) < 0.3] = 0.0
    weight[np.arange(13), np.arange(13)] = 1.0
    offsets, targets, counts = impute.blend(summaries, weight)
    own, class_cell, cell_total = impute.blend_sources(summaries)
    assert own.dtype == np.float64 and class_cell.dtype == np.int32 and cell_total.dtype == np.float64
    assert own.size == class_cell.size == offsets.size - 1 and targets.size == offsets[-1]
    assert class_cell.min() == 0 and class_cell.max() == 12 and (np.diff(class_cell) >= 0).all()
    np.testing.assert_array_equal(np.bincount(class_cell), [s.class_count.size for s in summaries])
    for i in range(13):
        made = ((own * weight[i, class_cell]) * cell_total[i]) / cell_total[class_cell]
        assert np.array_equal(made, counts[i])
    structure = impute.blend_structure(summaries)
    np.testing.assert_array_equal(structure[0], offsets)
    np.testing.assert_array_equal(structure[1], targets)


def test_new_entry_points_check_their_arguments(native_libs):
    hip = native_libs.hip()
    one = np.ones(4)
    cell = np.zeros(4, dtype=np.int32)
    f, i32 = native_libs.c_f64p, native_libs.c_i32p
    p = native_libs.ptr
    assert hip.skm_quant_em_many(None, 1, p(one, f), p(one, f), p(one, f), 0.01, 1e-8, 0, p(one, f), None) == native_libs.SKM_ERR_ARG
    assert hip.skm_quant_em_blend(None, 1, p(cell, i32), p(one, f), p(one, f), p(one, f), p(one, f), 0.01, 1e-8, 0,
                                  p(one, f), None, None) == native_libs.SKM_ERR_ARG
    # (a stand-in for a handle: the NULL checks come before anything looks inside it)
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    for missing in range(4):
        args = [p(one, f)] * 4
        args[missing] = None
        assert hip.skm_quant_em_many(fake, 1, args[0], args[1], args[2], 0.01, 1e-8, 0, args[3], None) == native_libs.SKM_ERR_ARG
    for missing in range(6):
        args = [p(cell, i32)] + [p(one, f)] * 5
        args[missing] = None
        assert hip.skm_quant_em_blend(fake, 1, args[0], args[1], args[2], args[3], args[4], 0.01, 1e-8, 0, args[5],
                                      None, None) == native_libs.SKM_ERR_ARG
    assert hip.skm_quant_em_many(fake, -1, p(one, f), p(one, f), p(one, f), 0.01, 1e-8, 0, p(one, f), None) == native_libs.SKM_ERR_ARG
    assert hip.skm_quant_em_blend(fake, -1, p(cell, i32), p(one, f), p(one, f), p(one, f), p(one, f), 0.01, 1e-8, 0,
                                  p(one, f), None, None) == native_libs.SKM_ERR_ARG
    assert b'argument' in hip.skm_last_error()
    # no problem at all: nothing is done, and nothing is asked of a GPU
    assert hip.skm_quant_em_many(fake, 0, None, None, None, 0.01, 1e-8, 0, None, None) == native_libs.SKM_OK
    assert hip.skm_quant_em_blend(fake, 0, None, None, None, None, None, 0.01, 1e-8, 0, None, None, None) == native_libs.SKM_OK


def test_new_entry_points_fail_loudly_without_a_gpu(native_libs):
    if native_libs.device_count() > 0:
        pytest.skip('a GPU is present')
    hip = native_libs.hip()
    one = np.ones(4)
    cell = np.zeros(4, dtype=np.int32)
    f, i32 = native_libs.c_f64p, native_libs.c_i32p
    p = native_libs.ptr
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    assert hip.skm_quant_em_many(fake, 1, p(one, f), p(one, f), p(one, f), 0.01, 1e-8, 0, p(one, f), None) == native_libs.SKM_ERR_NO_DEVICE
    assert b'no HIP device' in hip.skm_last_error()
    assert hip.skm_quant_em_blend(fake, 1, p(cell, i32), p(one, f), p(one, f), p(one, f), p(one, f), 0.01, 1e-8, 0,
                                  p(one, f), None, None) == native_libs.SKM_ERR_NO_DEVICE


def test_quantify_many_without_classes(native_libs):
    from seekmer_amd import infer
    empty = types.SimpleNamespace(class_map=np.asarray([]).T, class_count=np.zeros(0), effective_lengths=np.full(7, 200.0))
    tpm, iters = infer.quantify_many(empty, np.zeros((3, 0)), return_iters=True)
    assert tpm.shape == (3, 7) and not tpm.any() and tpm.dtype == np.float64
    assert iters.shape == (3,) and not iters.any()
    assert infer.quantify_many(empty, np.zeros((0, 0))).shape == (0, 7)
    with pytest.raises(ValueError):
        infer.quantify_many(empty, np.zeros(3))


def test_requantify_blend_keeps_the_loop_when_asked_or_needed(monkeypatch):
    """SKM_IMPUTE_SERIAL=1, cells whose effective lengths differ and shapes outside the measured regime
    (few cells, a large blended structure, many transcripts) take the loop over the cells."""
    from seekmer_amd import impute
    taken = []
    monkeypatch.setattr(impute, '_requantify_blend_serial', lambda *a, **k: taken.append('serial') or [])
    monkeypatch.setattr(impute.infer._QuantHandle, 'from_csr',
                        classmethod(lambda cls, *a, **k: (_ for _ in ()).throw(RuntimeError('batched'))))
    summaries = _summaries(impute.BATCH_MIN_CELLS + 2, 20, 3)
    weight = np.eye(len(summaries))
    monkeypatch.delenv('SKM_IMPUTE_SERIAL', raising=False)
    with pytest.raises(RuntimeError, match='batched'):
        impute.requantify_blend(summaries, weight)
    monkeypatch.setenv('SKM_IMPUTE_SERIAL', '0')                    # (only '1' switches)
    with pytest.raises(RuntimeError, match='batched'):
        impute.requantify_blend(summaries, weight)
    monkeypatch.setenv('SKM_IMPUTE_SERIAL', '1')
    impute.requantify_blend(summaries, weight)
    monkeypatch.delenv('SKM_IMPUTE_SERIAL')
    monkeypatch.setattr(impute, 'BATCH_MAX_CLASSES', sum(s.class_count.size for s in summaries) - 1)
    impute.requantify_blend(summaries, weight)
    monkeypatch.setattr(impute, 'BATCH_MAX_CLASSES', 1 << 40)
    monkeypatch.setattr(impute, 'BATCH_MAX_TRANSCRIPTS', 19)
    impute.requantify_blend(summaries, weight)
    monkeypatch.setattr(impute, 'BATCH_MAX_TRANSCRIPTS', 20)
    impute.requantify_blend(summaries[:impute.BATCH_MIN_CELLS - 1], weight[:impute.BATCH_MIN_CELLS - 1, :impute.BATCH_MIN_CELLS - 1])
    summaries[4].effective_lengths = summaries[4].effective_lengths + 1.0
    impute.requantify_blend(summaries, weight)
    assert taken == ['serial'] * 5
