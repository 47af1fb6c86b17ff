"""The host side of the quantification of many class tables in shared EM launches (skm_quant_em_tables,
skm_sample_set_quantify, skm_set_quant_groups; infer.quantify_tables): what needs no GPU."""
import ctypes
import types

import numpy as np
import pytest


def _tables_call(lib, n_tx=4, n_tables=1, table_offsets=(0, 1), class_offsets=(0, 2), targets=(0, 3), counts=(5.0,),
                 x0=True, l=True, out=True, device=0):
    """skm_quant_em_tables on one small table, every argument replaceable (None = NULL)."""
    p = lib.ptr
    keep = []

    def arr(values, dtype, ctype):
        if values is None:
            return None
        a = np.ascontiguousarray(values, dtype=dtype)
        keep.append(a)
        return p(a, ctype)

    room = max(n_tables, 1) * max(n_tx, 1)
    return lib.hip().skm_quant_em_tables(
        device, n_tx, n_tables, arr(table_offsets, np.int64, lib.c_i64p), arr(class_offsets, np.int64, lib.c_i64p),
        arr(targets, np.int32, lib.c_i32p), arr(counts, 'f8', lib.c_f64p),
        arr(np.full(room, 0.25) if x0 else None, 'f8', lib.c_f64p), arr(np.full(room, 200.0) if l else None, 'f8', lib.c_f64p),
        0.01, 1e-8, 0, 1, arr(np.zeros(room) if out else None, 'f8', lib.c_f64p), None)


def test_em_tables_checks_its_arguments(native_libs):
    bad = native_libs.SKM_ERR_ARG
    assert _tables_call(native_libs, n_tables=-1) == bad
    assert _tables_call(native_libs, n_tx=0) == bad
    assert _tables_call(native_libs, n_tx=-3) == bad
    assert _tables_call(native_libs, table_offsets=None) == bad
    assert _tables_call(native_libs, class_offsets=None) == bad
    assert _tables_call(native_libs, targets=None) == bad
    assert _tables_call(native_libs, counts=None) == bad
    assert _tables_call(native_libs, x0=False) == bad
    assert _tables_call(native_libs, l=False) == bad
    assert _tables_call(native_libs, out=False) == bad
    assert b'argument' in native_libs.hip().skm_last_error() or b'NULL' in native_libs.hip().skm_last_error()
    assert _tables_call(native_libs, n_tables=2, table_offsets=(0, 1, 0)) == bad         # tables that step backwards
    assert _tables_call(native_libs, table_offsets=(-1, 0)) == bad
    assert _tables_call(native_libs, class_offsets=(2, 0)) == bad                        # classes that step backwards
    assert b'monotone' in native_libs.hip().skm_last_error()
    assert _tables_call(native_libs, targets=(0, 4)) == bad                              # a target outside [0, n_tx)
    assert b'outside' in native_libs.hip().skm_last_error()
    assert _tables_call(native_libs, targets=(-1, 3)) == bad
    # a table whose classes all lack a tuple entry (one such class beside others is left to the device: the GPU tests)
    assert _tables_call(native_libs, table_offsets=(0, 2), class_offsets=(0, 0, 0), counts=(5.0, 1.0)) == bad
    assert b'names a transcript' in native_libs.hip().skm_last_error()
    # no table at all: nothing is done, and nothing is asked of a GPU
    assert _tables_call(native_libs, n_tables=0, table_offsets=None, class_offsets=None, targets=None, counts=None,
                        x0=False, l=False, out=False) == native_libs.SKM_OK
    # good arguments get as far as the device
    code = _tables_call(native_libs)
    assert code == (native_libs.SKM_OK if native_libs.device_count() > 0 else native_libs.SKM_ERR_NO_DEVICE)
    if native_libs.device_count() > 0:
        assert _tables_call(native_libs, device=native_libs.device_count()) == bad


def test_sample_set_quantify_checks_its_arguments(native_libs):
    hip = native_libs.hip()
    p, f, i64 = native_libs.ptr, native_libs.c_f64p, native_libs.c_i64p
    one = np.ones(4)
    n = ctypes.c_int64()
    # (a stand-in for a handle: these checks come before anything looks inside it)
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    bad = native_libs.SKM_ERR_ARG
    assert hip.skm_sample_set_quantify(None, p(one, f), 4, 0.01, 1e-8, 0, 1, ctypes.byref(n), p(one, f), None, None) == bad
    assert hip.skm_sample_set_quantify(fake, None, 4, 0.01, 1e-8, 0, 1, ctypes.byref(n), p(one, f), None, None) == bad
    assert hip.skm_sample_set_quantify(fake, p(one, f), 0, 0.01, 1e-8, 0, 1, ctypes.byref(n), p(one, f), None, None) == bad
    assert hip.skm_sample_set_quantify(fake, p(one, f), -4, 0.01, 1e-8, 0, 1, ctypes.byref(n), p(one, f), None, None) == bad
    assert hip.skm_sample_set_quantify(fake, p(one, f), 4, 0.01, 1e-8, 0, -1, ctypes.byref(n), p(one, f), None, None) == bad
    assert hip.skm_sample_set_quantify(fake, p(one, f), 4, 0.01, 1e-8, 0, 1, None, p(one, f), None, None) == bad
    assert hip.skm_sample_set_quantify(fake, p(one, f), 4, 0.01, 1e-8, 0, 1, ctypes.byref(n), None, None, None) == bad
    assert b'argument' in hip.skm_last_error()


def _brute_force_groups(n_tx, classes, ids, max_slots):
    """The documented rule (include/seekmer_hip.h, skm_set_quant_groups), table by table."""
    first, n, c, m = [0], 0, 0, 0
    for i in range(len(classes)):
        n1, c1, m1 = n + 1, c + int(classes[i]), m + int(ids[i])
        fits = (n1 <= min(max_slots, 32768) and n1 * n_tx < 2 ** 31 and c1 < 2 ** 31 and m1 < 2 ** 31
                and n1 * n_tx * 96 + c1 * 64 + m1 * 24 <= 2 ** 31)
        if n and not fits:
            first.append(i)
            n1, c1, m1 = 1, int(classes[i]), int(ids[i])
        n, c, m = n1, c1, m1
    if len(classes):
        first.append(len(classes))
    return first


@pytest.mark.parametrize('n_tx, max_slots, scale, min_groups', [
    (1700, 4, 1, 75), (1700, 1, 1, 300), (1700, 1 << 20, 1, 1), (190000, 1 << 20, 1, 2), (190000, 1 << 20, 4000, 3),
    (40000000, 1 << 20, 1, 300), (3, 40000, 1, 2)])
def test_group_cut_against_brute_force(native_libs, n_tx, max_slots, scale, min_groups):
    """A slot cap of 4 and of 1, no cut at all, the byte bound reached by the transcripts (190 k: about a hundred
    tables a group) and by the classes (scaled tables, one of them a group of its own above the bound), tables
    that each exceed the bound (40 M transcripts), and the grid's 32768 rows (50 000 tiny tables)."""
    rng = np.random.default_rng(n_tx + max_slots + scale)
    n_tables = 50000 if n_tx == 3 else 300
    classes = rng.integers(0, 5 if n_tx == 3 else 5000, n_tables).astype(np.int64) * scale
    classes[rng.integers(0, n_tables, 10)] = 0
    ids = classes * rng.integers(1, 6, n_tables)
    if scale > 1:
        classes[7], ids[7] = 30000000, 90000000          # alone above the byte bound: a group of its own
    first = np.zeros(n_tables + 1, dtype=np.int64)
    n_groups = ctypes.c_int64()
    p, i64 = native_libs.ptr, native_libs.c_i64p
    assert native_libs.hip().skm_set_quant_groups(n_tables, n_tx, p(classes, i64), p(ids, i64), max_slots,
                                                  ctypes.byref(n_groups), p(first, i64)) == native_libs.SKM_OK
    want = _brute_force_groups(n_tx, classes, ids, max_slots)
    assert first[:n_groups.value + 1].tolist() == want
    sizes = np.diff(want)
    assert sizes.min() >= 1 and sizes.max() <= min(max_slots, 32768) and sizes.sum() == n_tables
    assert len(want) - 1 >= min_groups and (min_groups > 1 or len(want) == 2)
    if n_tx == 3:
        assert sizes[0] == 32768
    if scale > 1:
        assert 7 in want and 8 in want


def test_group_cut_checks_its_arguments(native_libs):
    hip = native_libs.hip()
    p, i64 = native_libs.ptr, native_libs.c_i64p
    two = np.asarray([1, 2], dtype=np.int64)
    first = np.zeros(3, dtype=np.int64)
    n = ctypes.c_int64(-1)
    bad = native_libs.SKM_ERR_ARG
    assert hip.skm_set_quant_groups(-1, 5, p(two, i64), p(two, i64), 4, ctypes.byref(n), p(first, i64)) == bad
    assert hip.skm_set_quant_groups(2, 0, p(two, i64), p(two, i64), 4, ctypes.byref(n), p(first, i64)) == bad
    assert hip.skm_set_quant_groups(2, 5, p(two, i64), p(two, i64), 0, ctypes.byref(n), p(first, i64)) == bad
    assert hip.skm_set_quant_groups(2, 5, None, p(two, i64), 4, ctypes.byref(n), p(first, i64)) == bad
    assert hip.skm_set_quant_groups(2, 5, p(two, i64), p(two, i64), 4, None, p(first, i64)) == bad
    assert hip.skm_set_quant_groups(2, 5, p(two, i64), p(-two, i64), 4, ctypes.byref(n), p(first, i64)) == bad
    assert hip.skm_set_quant_groups(0, 5, None, None, 4, ctypes.byref(n), None) == native_libs.SKM_OK and n.value == 0


def test_quantify_tables_without_tables_and_with_mixed_transcripts(native_libs):
    from seekmer_amd import infer
    none = infer.quantify_tables([])
    assert none.size == 0 and none.dtype == np.float64
    tpm, iters = infer.quantify_tables([], return_iters=True)
    assert tpm.size == 0 and iters.shape == (0,)

    def table(n_tx):
        return types.SimpleNamespace(class_map=np.asarray([[0, 0], [0, 1]], dtype=np.int64), class_count=np.asarray([3.0]),
                                     effective_lengths=np.full(n_tx, 200.0))
    with pytest.raises(ValueError, match='n_tx'):
        infer.quantify_tables([table(7), table(8)])


def test_quantify_tables_fails_loudly_without_a_gpu(native_libs):
    """(tables, even ones without classes, are the device's business: there is no host fall-back)"""
    if native_libs.device_count() > 0:
        pytest.skip('a GPU is present')
    from seekmer_amd import infer
    empty = types.SimpleNamespace(class_map=np.asarray([]).T, class_count=np.zeros(0), effective_lengths=np.full(7, 200.0))
    with pytest.raises(native_libs.NativeError) as error:
        infer.quantify_tables([empty, empty])
    assert error.value.code == native_libs.SKM_ERR_NO_DEVICE


def test_first_round_routing(monkeypatch):
    """impute.first_round takes the shared launches inside the measured regime only, from the set when there is
    one; SKM_SET_QUANT_SERIAL=1 and SKM_IMPUTE_SERIAL=1 (exactly that value) both keep the loop over the cells."""
    from seekmer_amd import impute
    for name in ('SKM_SET_QUANT_SERIAL', 'SKM_IMPUTE_SERIAL'):
        monkeypatch.delenv(name, raising=False)
    n = impute.SET_QUANT_MIN_SAMPLES
    summaries = [types.SimpleNamespace(class_count=np.ones(3), effective_lengths=np.full(5, 200.0)) for _ in range(n)]
    taken = []
    monkeypatch.setattr(impute.infer, 'quantify', lambda summary: taken.append('loop') or np.zeros(5))
    monkeypatch.setattr(impute.infer, 'quantify_tables', lambda tables, device=0: taken.append('tables') or np.zeros((len(tables), 5)))
    sample_set = types.SimpleNamespace(quantify=lambda: taken.append('set') or np.zeros((n, 5)))

    def route(cells=summaries, through=None):
        del taken[:]
        assert impute.first_round(cells, through).shape == (len(cells), 5)
        return taken[:]

    assert route() == ['tables'] and route(through=sample_set) == ['set']
    assert route(summaries[:-1], sample_set) == ['loop'] * (n - 1)      # (below the smallest count measured ahead)
    for switch in ('SKM_SET_QUANT_SERIAL', 'SKM_IMPUTE_SERIAL'):
        monkeypatch.setenv(switch, '1')
        assert route() == ['loop'] * n and route(through=sample_set) == ['loop'] * n
        monkeypatch.setenv(switch, '0')                                 # (only '1' switches)
        assert route() == ['tables']
        monkeypatch.delenv(switch)
    # the two measured regimes: small tables from SET_QUANT_MIN_SAMPLES, larger ones only from SET_QUANT_LARGE_MIN_SAMPLES
    monkeypatch.setattr(impute, 'SET_QUANT_SMALL_TRANSCRIPTS', 4)
    assert route() == ['loop'] * n
    monkeypatch.setattr(impute, 'SET_QUANT_LARGE_MIN_SAMPLES', n)
    assert route() == ['tables']
    monkeypatch.setattr(impute, 'SET_QUANT_MAX_TRANSCRIPTS', 4)
    assert route() == ['loop'] * n
    monkeypatch.setattr(impute, 'SET_QUANT_MAX_TRANSCRIPTS', 5)
    monkeypatch.setattr(impute, 'SET_QUANT_MAX_CLASSES', 3 * n - 1)
    assert route() == ['loop'] * n
    monkeypatch.setattr(impute, 'SET_QUANT_MAX_CLASSES', 3 * n)
    assert route() == ['tables']
    monkeypatch.setattr(impute, 'SET_QUANT_LARGE_MIN_SAMPLES', n + 1)
    monkeypatch.setattr(impute, 'SET_QUANT_SMALL_TRANSCRIPTS', 5)
    monkeypatch.setattr(impute, 'SET_QUANT_SMALL_CLASSES', 3 * n - 1)
    assert route() == ['loop'] * n
    monkeypatch.setattr(impute, 'SET_QUANT_SMALL_CLASSES', 3 * n)
    assert route() == ['tables']


def test_the_rule_holds_the_measured_shapes_and_no_more():
    """use_set_quant at the shapes of profiles/set_quant_ab.log (samples, transcripts, classes in all) and next to them."""
    from seekmer_amd import impute
    rule = impute.use_set_quant
    assert rule(8, 944, 27765) and rule(64, 944, 221741) and rule(512, 944, 1773517) and rule(64, 190402, 2629763)
    assert not rule(2, 944, 6984) and not rule(7, 944, 27765)               # (level at 2 cells; 3 to 7 not run)
    assert not rule(8, 190402, 330000) and not rule(63, 190402, 2629763)     # (fewer than 64 cells on the large table: not run)
    assert not rule(64, 190403, 2629763) and not rule(64, 190402, 2629764) and not rule(8, 945, 27765)
    assert not rule(513, 944, 2629764)
