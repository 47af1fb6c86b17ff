"""Distributed molecules on the device ("Distributed molecules") against
tests/molecule_em_reference.py, exactly -- integers equal, doubles equal as bits: the EM alone through
skm_gene_em_cells at the edges of its eight-lane order and of its two paths; host classes and molecules through
skm_gene_matrix_from_molecule_sets; a sample set's resident state through SampleSet.gene_distributed_matrix, with the
classes taken from the oracle, also under umi_mismatches=1; and `infer-many --distribute-molecules` on pooled files."""
import ctypes
import os

import numpy as np
import pytest

import molecule_em_reference as emref
import molecule_resolve_reference as mres
import umi_mismatch_reference as near_ref
import umi_reference as ref
from conftest import GOLDEN, make_product_index
from test_gpu_molecule_resolve import (_add_sample, _chosen_pairs, _classes, _csr_of, _hook, _pairs, _two_fragments,
                                       _write_fastq)

pytestmark = pytest.mark.gpu

READ_LEN = 75
NAMES = ('indptr', 'indices', 'data', 'tally', 'to_unnamed')
LDS_ROWS = 4096                   # GENE_EM_LDS_ROWS of skm_kernels.h


def _same_bits(got, want, names):
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (name, a, b)


# ---- the EM alone -------------------------------------------------------------------------------------------------
class Cells:
    """the CSR arrays of skm_gene_em_cells, a cell (u, sets of cell-local rows) at a time"""

    def __init__(self):
        self.cell_row_start, self.cell_set_start, self.u, self.set_start, self.set_rows = [0], [0], [], [0], []

    def add(self, u, sets):
        self.u += [int(v) for v in u]
        for rows in sets:
            self.set_rows += [int(r) for r in rows]
            self.set_start.append(len(self.set_rows))
        self.cell_row_start.append(len(self.u))
        self.cell_set_start.append(len(self.set_start) - 1)
        return self

    def arrays(self):
        return (np.asarray(self.cell_row_start, dtype=np.int64), np.asarray(self.u, dtype=np.int64),
                np.asarray(self.cell_set_start, dtype=np.int64), np.asarray(self.set_start, dtype=np.int64),
                np.asarray(self.set_rows, dtype=np.int32))


def _em(cells, max_steps=1000):
    """the device's (x, steps, capped), equal to the reference's"""
    from seekmer_amd import mapper
    got = mapper.gene_em_cells(*cells.arrays(), max_steps=max_steps)
    _same_bits(got, emref.em_cells(*cells.arrays(), max_steps=max_steps), ('x', 'steps', 'capped'))
    return got


def _edge_cell():
    """rows 0..6 lie in 0, 1, 7, 8, 9, 17 and 1000 sets of two rows (the other row one of 7..11), rows 12..27 form one
    set of 16 rows, twice"""
    counts = [0, 1, 7, 8, 9, 17, 1000]
    sets = [[r, 7 + (i + r) % 5] for r, k in enumerate(counts) for i in range(k)]
    sets = [sets[i] for i in np.random.default_rng(5).permutation(len(sets))] + [list(range(12, 28))] * 2
    u = [3, 0, 2, 0, 1, 40, 5, 0, 1, 0, 7, 2] + [k % 3 for k in range(16)]
    return u, sets


def _small_cells(n_cells, seed):
    """random cells of 0 to 12 rows and 0 to 20 sets of 2 to min(rows, 16) rows; every fifth cell is empty"""
    rng = np.random.default_rng(seed)
    cells = Cells()
    for c in range(n_cells):
        rows = 0 if c % 5 == 2 else int(rng.integers(1, 13))
        n_sets = 0 if rows < 2 else int(rng.integers(0, 21))
        sets = [sorted(rng.choice(rows, size=int(rng.integers(2, min(rows, 16) + 1)), replace=False)) for _ in range(n_sets)]
        cells.add(rng.integers(0, 6, rows), sets)
    return cells


def test_rows_at_the_edges_of_the_eight_lane_order(native_libs):
    u, sets = _edge_cell()
    holds = np.bincount([r for rows in sets for r in rows], minlength=len(u))
    assert holds[:7].tolist() == [0, 1, 7, 8, 9, 17, 1000] and {len(rows) for rows in sets} == {2, 16}
    x, steps, capped = _em(Cells().add(u, sets))
    assert x[0] == 3.0 and steps[0] >= 2 and not capped[0]
    total = sum(u) + len(sets)
    assert abs(x.sum() - total) < 1e-9 * total


def test_a_cell_of_one_row_and_cells_without_sets(native_libs):
    x, steps, capped = _em(Cells().add([4], []))
    assert x.tolist() == [4.0] and steps.tolist() == [0] and capped.tolist() == [0]
    x, steps, capped = _em(Cells().add([], []).add([1, 0, 7], []).add([], []))
    assert x.tolist() == [1.0, 0.0, 7.0] and steps.tolist() == [0, 0, 0]
    x, steps, capped = _em(Cells())            # no cell at all
    assert x.size == 0 and steps.size == 0


def test_300_cells_in_one_call(native_libs):
    cells = _small_cells(300, 11)
    starts = np.asarray(cells.cell_row_start)
    assert (np.diff(starts) == 0).sum() >= 60 and (np.diff(cells.cell_set_start) == 0).sum() > 60
    x, steps, capped = _em(cells)
    assert steps.max() >= 2 and not capped.any()


def _slow_cell():
    """50 sets over a row of 100 molecules and a row of none: the second row decays by a constant factor a step"""
    return [100, 0], [[0, 1]] * 50


def test_a_slow_cell_is_capped(native_libs):
    u, sets = _slow_cell()
    _, steps, capped = emref.em(u, sets)
    assert steps > 3 and not capped
    x, steps, capped = _em(Cells().add(u, sets).add([1, 1], [[0, 1]]), max_steps=3)
    assert steps.tolist() == [3, 1] and capped.tolist() == [1, 0]
    x, steps, capped = _em(Cells().add(u, sets), max_steps=1)
    assert steps.tolist() == [1] and capped.tolist() == [1]


def test_the_global_path_gives_the_bits_of_the_lds_path(native_libs, monkeypatch):
    """a cell of LDS_ROWS + 1 rows beside one of LDS_ROWS; and the small cases with the cap lowered to 4 rows"""
    monkeypatch.delenv('SKM_TEST_GENE_EM_LDS_ROWS', raising=False)
    rng = np.random.default_rng(23)
    cells = Cells()
    for rows in (LDS_ROWS + 1, LDS_ROWS):
        sets = [sorted(rng.choice(rows, size=int(rng.integers(2, 17)), replace=False)) for _ in range(3000)]
        sets.append([0, rows - 1])             # (the last row is in a set)
        cells.add(rng.integers(0, 3, rows), sets)
    x, steps, capped = _em(cells)
    assert steps.min() >= 1
    small = [Cells().add(*_edge_cell()), _small_cells(300, 11), Cells().add(*_slow_cell())]
    in_lds = [_em(c) for c in small]
    monkeypatch.setenv('SKM_TEST_GENE_EM_LDS_ROWS', '4')
    for c, want in zip(small, in_lds):
        _same_bits(_em(c), want, ('x', 'steps', 'capped'))
    _same_bits(_em(small[2], max_steps=3), emref.em_cells(*small[2].arrays(), max_steps=3), ('x', 'steps', 'capped'))


def test_the_em_refuses_bad_cells(native_libs):
    from seekmer_amd import mapper
    good = dict(cell_row_start=[0, 3], u=[1, 0, 2], cell_set_start=[0, 2], set_start=[0, 2, 5], set_rows=[0, 1, 0, 1, 2])
    assert mapper.gene_em_cells(**good)[1].tolist() == [emref.em([1, 0, 2], [[0, 1], [0, 1, 2]])[1]]
    bad = [dict(set_rows=[0, 3, 0, 1, 2]), dict(set_rows=[0, -1, 0, 1, 2]),          # a row outside its cell
           dict(set_start=[0, 1, 5], set_rows=[0, 0, 1, 2, 2]),                      # a set of one row
           dict(cell_row_start=[0, 20], u=[1] * 20, set_start=[0, 2, 19], set_rows=[0, 1] + list(range(17))),   # 17 rows
           dict(set_rows=[1, 0, 0, 1, 2]), dict(set_rows=[0, 1, 0, 1, 1]),          # unsorted, repeated
           dict(u=[1, -1, 2]), dict(max_steps=0)]
    for change in bad:
        with pytest.raises(ValueError):           # (SKM_ERR_ARG)
            mapper.gene_em_cells(**dict(good, **change))
    # a second cell whose set names a row of the first cell's range: outside ITS cell
    with pytest.raises(ValueError):
        mapper.gene_em_cells([0, 3, 5], [1, 0, 2, 1, 1], [0, 0, 1], [0, 2], [1, 2])


# ---- the host door ------------------------------------------------------------------------------------------------
def _door(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes, max_steps=1000):
    """the device's five arrays, equal to the reference's, and the identities that follow from the rule"""
    from seekmer_amd import mapper
    got = mapper.distributed_molecule_matrix(*_csr_of(class_tuples), class_sample, mol_class, mol_umi, tx_gene, n_samples,
                                             n_genes, max_steps=max_steps)
    emref.check_csr(*got[:3], n_samples, n_genes)
    want = emref.matrix_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes, max_steps)
    _same_bits(got, want, NAMES)
    tally = got[3]
    resolved = mres.matrix_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples)[3]
    np.testing.assert_array_equal(tally[:, [emref.RESOLVED, emref.UNNAMED, emref.COLLISION]],
                                  resolved[:, [mres.RESOLVED, mres.UNNAMED, mres.COLLISION]])
    np.testing.assert_array_equal(tally[:, emref.DISTRIBUTED] + tally[:, emref.WIDE], resolved[:, mres.MULTI])
    return got


def _random_case(n, seed=2000):
    """about 48 classes over 120 transcripts, 36 genes of three and twelve transcripts without a gene, 5 cells and an
    empty sixth, 12 UMIs; every (cell, UMI) draws from a pool of 1 to 3 of the cell's classes.  The classes of a cell
    share a base of 20 genes' transcripts now and then, so that intersections of more than 16 genes occur"""
    rng = np.random.default_rng(seed + n)
    tx_gene = (np.arange(120) // 3).astype(np.int32)
    tx_gene[tx_gene >= 36] = -1
    class_tuples, class_sample = [], []
    for k in range(48):
        cell, shape = k % 5, k // 5
        block = lambda g: rng.permutation(np.flatnonzero(np.arange(120) // 3 == g))
        strangers = lambda low, high: rng.integers(0, 108, int(rng.integers(low, high)))
        base = np.arange(20) * 3 + 15 + cell % 3
        if shape == 0:                        # inside the cell's block
            t = block(cell)[:int(rng.integers(1, 4))]
        elif shape in (1, 2, 3):              # one or two of the block and a few strangers, or many
            t = np.concatenate([block(cell)[:1 + shape % 2], strangers(1, 4) if shape < 3 else strangers(6, 11)])
        elif shape == 4:                      # another block and strangers
            t = np.concatenate([block(cell + 5)[:2], strangers(1, 4)])
        elif shape in (5, 6):                 # wide: the base of 20 genes and strangers
            t = np.concatenate([rng.permutation(base), strangers(0, 5)])
        elif shape == 7:                      # the block, a neighbour and an unnamed transcript
            t = np.concatenate([block(cell)[:1], block(cell + 1)[:1], [110 + cell]])
        else:                                 # unnamed transcripts, with company in the last
            t = np.concatenate([[112, 113][:int(rng.integers(1, 3))], strangers(0, 1) if shape == 8 else strangers(1, 2)])
        class_tuples.append(tuple(int(x) for x in dict.fromkeys(int(x) for x in t)))
        class_sample.append(cell)
    class_sample = np.asarray(class_sample, dtype=np.int32)
    pools = []
    for cell in range(5):
        mine = np.flatnonzero(class_sample == cell)
        for umi in range(12):
            pools.append((umi, rng.choice(mine, size=int(rng.integers(1, 4)))))
    group = rng.integers(0, len(pools), n)
    mol_class = np.asarray([int(rng.choice(pools[g][1])) for g in group], dtype=np.int32)
    mol_umi = np.asarray([pools[g][0] for g in group], dtype=np.uint32)
    return class_tuples, class_sample, mol_class, mol_umi, tx_gene


def test_the_random_case_is_not_trivial():
    """the reference alone: every outcome, a cell of at least two steps and no capped cell at n = 3000"""
    class_tuples, class_sample, mol_class, mol_umi, tx_gene = _random_case(3000)
    tally = emref.matrix_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene, 6, 36)[3]
    print('resolved, distributed, wide, unnamed, collision: %r; steps %r' % (tally[:, :5].sum(axis=0).tolist(), tally[:, 6].tolist()))
    assert (tally[:, :5].sum(axis=0) > 0).all() and tally[:, emref.STEPS].max() >= 2 and not tally[:, emref.CAPPED].any()
    assert tally[:5, emref.DISTRIBUTED].min() > 0 and not tally[5].any()


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 3000])
def test_random_molecules(native_libs, n):
    class_tuples, class_sample, mol_class, mol_umi, tx_gene = _random_case(n)
    got = _door(class_tuples, class_sample, mol_class, mol_umi, tx_gene, 6, 36)
    assert got[0][5] == got[0][6] and not got[3][5].any()               # (sample 5 is empty)
    order = np.random.default_rng(n).permutation(n)                     # the same molecules in another order
    _same_bits(_door(class_tuples, class_sample, mol_class[order], mol_umi[order], tx_gene, 6, 36), got, NAMES)


@pytest.mark.parametrize('k', [2, 15, 16, 17, 70])
def test_intersections_of_k_genes(native_libs, k):
    """every gene has two transcripts; the pivot holds the k genes' first transcripts at its head, strangers, and the
    genes' second transcripts astride place 64 (k = 70: the first astride 64, the second astride 128) -- the genes are
    repeated on both sides of a 64-candidate chunk's boundary"""
    n_genes = 600
    tx_gene = np.concatenate([np.arange(n_genes), np.arange(n_genes)]).astype(np.int32)
    first, second = list(range(k)), list(range(n_genes, n_genes + k))
    pivot = first + list(range(200, 200 + max(0, 64 - (k + 1) // 2 - k))) + second
    member = second[::-1] + first + list(range(300, 300 + len(pivot)))
    assert len(member) > len(pivot) > 64 and (k > 64 or pivot.index(second[0]) < 64 <= pivot.index(second[-1]))
    # beside it in the cell: a molecule inside gene 598 and one inside gene 599
    got = _door([tuple(pivot), tuple(member), (598,), (599,)], np.zeros(4, dtype=np.int32), [1, 0, 2, 3], [5, 5, 6, 7], tx_gene, 1, n_genes)
    wide = k > 16
    assert got[3][0, :5].tolist() == [2, 0 if wide else 1, 1 if wide else 0, 0, 0]
    assert got[3][0, emref.ROWS] == (2 if wide else k + 2)
    if not wide:
        assert got[1].tolist() == list(range(k)) + [598, 599] and abs(got[2].sum() - 3.0) < 1e-12


def test_an_intersection_that_holds_no_gene(native_libs):
    #          transcripts 0 1 in gene 0, 2 3 in gene 1, 4 5 unnamed
    tx_gene = np.asarray([0, 0, 1, 1, -1, -1], dtype=np.int32)
    got = _door([(0, 4, 2), (5, 1, 3), (0,), (4,)], np.zeros(4, dtype=np.int32), [0, 1, 2, 2, 3], [9, 9, 1, 2, 3], tx_gene, 1, 2)
    assert got[3][0, :6].tolist() == [2, 1, 0, 1, 0, 3]                 # rows: gene 0, gene 1 and the sink, which is last
    assert got[1][0] == 0 and got[2][0] > 2.0 and got[4][0] > 1.0       # to_unnamed: its own molecule and a share
    assert 4.0 - 0.001 < got[2].sum() + got[4][0] < 4.0 + 1e-12         # (gene 1 has no molecule of its own: it may fall below the cut)
    # the sink alone in a set with one gene, and no other molecule: half each at the start, and it stays
    got = _door([(0, 4)], np.zeros(1, dtype=np.int32), [0], [9], tx_gene, 1, 2)
    assert got[2].tolist() == [0.5] and got[4].tolist() == [0.5] and got[3][0].tolist() == [0, 1, 0, 0, 0, 2, 1, 0]


def test_one_ambiguous_class_and_several_members_make_the_same_set(native_libs):
    tx_gene = np.arange(8, dtype=np.int32)
    class_tuples = [(1, 0), (0, 1, 2), (3, 1, 0), (0,), (1,), (0, 1, 2), (3, 1, 0), (1, 0), (0,), (1,)]
    class_sample = np.asarray([0, 1, 1, 0, 0, 2, 2, 2, 1, 1], dtype=np.int32)
    #   cell 0: the class {0, 1} alone;  cell 1: two classes that meet in {0, 1};  cell 2: all three under one UMI;
    #   cells 0 and 1 with two molecules inside gene 0 and one inside gene 1 beside it
    mol_class = [0, 3, 3, 4, 1, 2, 8, 8, 9, 5, 6, 7]
    mol_umi = [4, 5, 6, 7, 4, 4, 5, 6, 7, 4, 4, 4]
    got = _door(class_tuples, class_sample, mol_class, mol_umi, tx_gene, 3, 8)
    assert got[3][:2, :6].tolist() == [[3, 1, 0, 0, 0, 2]] * 2 and got[3][2, :6].tolist() == [0, 1, 0, 0, 0, 2]
    assert got[2][:2].tobytes() == got[2][2:4].tobytes() and got[1].tolist() == [0, 1] * 3 and got[2][4:].tolist() == [0.5, 0.5]
    assert got[2][0] > 2.5 and got[3][0, emref.STEPS] >= 2


def test_groups_across_a_wave_and_across_a_block(native_libs):
    """a 3-class group at sorted places 63..65 and another at 255..257, single-class groups of smaller keys ahead"""
    tx_gene = np.arange(20, dtype=np.int32)
    class_tuples = [(0,), (1, 2), (2, 1, 3), (1, 4, 2, 5)]
    mol_class, mol_umi = [], []
    for umi in range(252):
        if umi == 63:
            mol_class += [1, 2, 3]; mol_umi += [1000] * 3
        mol_class.append(0); mol_umi.append(umi if umi < 63 else 1000 + umi)
    mol_class += [3, 2, 1]; mol_umi += [5000] * 3
    assert len(mol_umi) == 258 and sorted(mol_umi).index(1000) == 63 and sorted(mol_umi).index(5000) == 255
    got = _door(class_tuples, np.zeros(4, dtype=np.int32), mol_class, mol_umi, tx_gene, 1, 20)
    assert got[1].tolist() == [0, 1, 2] and got[2].tolist() == [252.0, 1.0, 1.0] and got[3][0, :6].tolist() == [252, 2, 0, 0, 0, 3]


def test_a_cell_of_resolved_groups_alone_is_the_resolved_matrix(native_libs):
    from seekmer_amd import mapper
    tx_gene = np.asarray([0, 0, 0, 1, 1, -1, -1, 2], dtype=np.int32)
    class_tuples = [(0, 1, 7), (2, 3, 4, 5), (0, 1, 2), (1, 3, 4, 7), (5,), (3,), (7,)]
    mol_class, mol_umi = [0, 1, 2, 3, 4, 5, 5, 6, 2], [1, 1, 2, 2, 3, 4, 5, 6, 7]
    sample = np.zeros(len(class_tuples), dtype=np.int32)
    got = _door(class_tuples, sample, mol_class, mol_umi, tx_gene, 1, 3)
    counts = mapper.resolved_molecule_matrix(*_csr_of(class_tuples), sample, mol_class, mol_umi, tx_gene, 1, 3)
    assert got[3][0].tolist() == [6, 0, 0, 1, 0, 4, 0, 0] and got[4].tolist() == [1.0]
    np.testing.assert_array_equal(got[0], counts[0]); np.testing.assert_array_equal(got[1], counts[1])
    assert got[2].tobytes() == counts[2].astype(np.float64).tobytes()


def test_bad_input_gives_no_handle(native_libs):
    hip = native_libs.hip()
    good = dict(offsets=[0, 2, 3], targets=[0, 1, 2], sample=[0, 1], mol_class=[0, 1], n_tx=3, max_steps=1000)
    bad = [dict(mol_class=[0, 2]), dict(mol_class=[-1, 0]), dict(sample=[0, 2]), dict(sample=[-1, 0]), dict(targets=[0, 3, 2]),
           dict(targets=[0, -1, 2]), dict(offsets=[0, 3, 3]), dict(n_tx=2), dict(max_steps=0)]
    for n_bad, change in enumerate([{}] + bad):
        case = dict(good, **change)
        offsets = np.asarray(case['offsets'], dtype=np.int64)
        targets, sample, mol_class = (np.asarray(case[k], dtype=np.int32) for k in ('targets', 'sample', 'mol_class'))
        umi, tx_gene = np.asarray([1, 2], dtype=np.uint32), np.asarray([0, 0, 1][:case['n_tx']], dtype=np.int32)
        handle = ctypes.c_void_p(1)
        code = hip.skm_gene_matrix_from_molecule_sets(
            0, 2, native_libs.ptr(offsets, native_libs.c_i64p), native_libs.ptr(targets, native_libs.c_i32p),
            native_libs.ptr(sample, native_libs.c_i32p), 2, native_libs.ptr(mol_class, native_libs.c_i32p),
            native_libs.ptr(umi, native_libs.c_u32p), 2, case['n_tx'], 2, native_libs.ptr(tx_gene, native_libs.c_i32p),
            case['max_steps'], ctypes.byref(handle))
        if n_bad == 0:
            assert code == 0 and handle.value
            # the counts of a handle that holds weights, and its resolved tally
            words = np.zeros(16, dtype=np.int64)
            assert hip.skm_gene_matrix_read(handle, None, None, native_libs.ptr(words, native_libs.c_i64p), None) == native_libs.SKM_ERR_STATE
            assert hip.skm_gene_matrix_read_tally(handle, native_libs.ptr(words, native_libs.c_i64p)) == native_libs.SKM_ERR_STATE
            hip.skm_gene_matrix_destroy(handle)
        else:
            assert code == native_libs.SKM_ERR_ARG and handle.value is None, change
    assert hip.skm_sample_set_distributed_matrix(None, 0, 0, None, None) == native_libs.SKM_ERR_ARG
    # the weights and the EM's tally of a handle that holds a resolved matrix
    offsets, targets = np.asarray(good['offsets'], dtype=np.int64), np.asarray(good['targets'], dtype=np.int32)
    sample = mol_class = np.asarray([0, 1], dtype=np.int32)
    umi, tx_gene = np.asarray([1, 2], dtype=np.uint32), np.asarray([0, 0, 1], dtype=np.int32)
    handle = ctypes.c_void_p()
    assert hip.skm_gene_matrix_from_molecule_classes(
        0, 2, native_libs.ptr(offsets, native_libs.c_i64p), native_libs.ptr(targets, native_libs.c_i32p),
        native_libs.ptr(sample, native_libs.c_i32p), 2, native_libs.ptr(mol_class, native_libs.c_i32p),
        native_libs.ptr(umi, native_libs.c_u32p), 2, 3, 2, native_libs.ptr(tx_gene, native_libs.c_i32p), ctypes.byref(handle)) == 0
    words, weights = np.zeros(16, dtype=np.int64), np.zeros(16, dtype=np.float64)
    try:
        assert hip.skm_gene_matrix_read_weights(handle, native_libs.ptr(weights, native_libs.c_f64p)) == native_libs.SKM_ERR_STATE
        assert hip.skm_gene_matrix_read_em(handle, native_libs.ptr(words, native_libs.c_i64p),
                                           native_libs.ptr(weights, native_libs.c_f64p)) == native_libs.SKM_ERR_STATE
    finally:
        hip.skm_gene_matrix_destroy(handle)


# ---- the set, directly (fixtures of its own, smaller than tests/test_gpu_molecule_resolve.py's) ------------------
N_SYNTH_GENES = 400
DISTINCT = 1500                   # distinct pairs a cell
N_CELLS = 3


@pytest.fixture(scope='module')
def transcriptome(oracle, native_libs):
    """(pool, tx_offsets, oracle index, product index, tx_gene, n_genes, block): transcripts that some class of 30 000
    oracle-mapped pairs holds together form a block; a block is a gene, but in every fifth block every transcript is a
    gene of its own (a split block: classes inside it are multi-gene), and every tenth block is unnamed"""
    from seekmer_amd import synth
    ids, pool, tx_offsets = synth.transcriptome(9, N_SYNTH_GENES)
    oindex = oracle.build_index(synth.sequences_of(pool, tx_offsets), ids)
    n_tx = len(ids)
    parent = list(range(n_tx))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    probe = synth.reads(3, pool, tx_offsets, 700000, 30000, READ_LEN, True)
    for t in set(oracle.map_batch(oindex, probe[0], probe[1], 30000, True).tuples()):
        for x in t[1:]:
            parent[find(x)] = find(t[0])
    roots = {}
    block = np.asarray([roots.setdefault(find(t), len(roots)) for t in range(n_tx)])
    tx_gene = block.copy()
    n_genes = len(roots)
    for t in np.flatnonzero(block % 5 == 0):
        tx_gene[t] = n_genes
        n_genes += 1
    tx_gene[block % 10 == 0] = -1
    return pool, tx_offsets, oindex, make_product_index(oindex, ids), tx_gene.astype(np.int32), n_genes, block


@pytest.fixture(scope='module')
def cells(oracle, transcriptome):
    """N_CELLS cells of units (pair, UMI): every distinct pair one to three times under a UMI of its own, but the chosen
    pairs of pairs (tests/test_gpu_molecule_resolve.py's choice) under one.  Cell 0 begins with units that under
    umi_mismatches=1 take the first class away from five of its multi-gene groups."""
    pool, tx_offsets, oindex, index, tx_gene, n_genes, block = transcriptome
    rng = np.random.default_rng(29)
    samples = []
    for s in range(N_CELLS):
        distinct = _pairs(pool, tx_offsets, 80 + s, s * 40000, DISTINCT)
        chosen = _chosen_pairs(_classes(oracle, oindex, distinct), block)
        umi_of = {}
        for pairs in chosen.values():
            for i, j in pairs:
                umi_of[i] = umi_of[j] = int(rng.integers(1000, 2 ** 32 - 1)) & ~1
        units = []
        for i, pair in enumerate(distinct):
            units += [(pair, umi_of.get(i, int(rng.integers(1000, 2 ** 32 - 1))))] * int(rng.choice([1, 2, 3], p=[.5, .3, .2]))
        units = [units[i] for i in rng.permutation(len(units))]
        if s == 0:
            units = [(distinct[i], umi_of[i] ^ 1) for i, _ in chosen['multi'][:5]] + units
        samples.append(units)
    reads = [read for units in samples for pair, _ in units for read in pair]
    sample = np.repeat(np.arange(N_CELLS), [len(units) for units in samples]).astype(np.int32)
    umi = np.asarray([m for units in samples for _, m in units], dtype=np.uint32)
    tuples = oracle.map_batch(oindex, *oracle.pack_reads(reads), sample.size, True).tuples()
    stay = {0: ref.survivors(sample, umi, tuples), 1: near_ref.survivors(sample, umi, tuples, 16, 1)}
    want = {k: emref.matrix(sample, umi, tuples, stay[k], tx_gene, N_CELLS, n_genes) for k in stay}
    resolved = {k: mres.matrix(sample, umi, tuples, stay[k], tx_gene, N_CELLS)[3] for k in stay}
    return dict(samples=samples, want=want, resolved=resolved, index=index, tx_gene=tx_gene, n_genes=n_genes)


def test_the_cells_are_not_trivial(cells):
    """the reference alone: every cell has sets and takes steps, none is capped; unnamed and collisions occur"""
    for mismatches in (0, 1):
        tally = cells['want'][mismatches][3]
        print('umi_mismatches=%d: %r' % (mismatches, tally.tolist()))
        assert tally[:, emref.DISTRIBUTED].min() >= 20 and tally[:, emref.STEPS].min() >= 1 and not tally[:, emref.CAPPED].any()
        assert tally[:, [emref.RESOLVED, emref.UNNAMED, emref.COLLISION]].min() >= 5
    assert cells['want'][0][3].tobytes() != cells['want'][1][3].tobytes()
    data = cells['want'][0][2]
    assert (data != np.round(data)).sum() >= 20                          # shares, not counts alone


@pytest.mark.parametrize('mismatches,hook', [(0, None), (1, None), (1, ('SKM_TEST_UMI_SLOTS=2', 'SKM_SAMPLE_SET_MAX_UNITS=500'))])
def test_the_distributed_matrix_of_a_set_is_the_reference(cells, monkeypatch, mismatches, hook):
    """2 slots and launches of 500 units: the molecule set grows after the launch that marked molecules dropped"""
    from seekmer_amd import mapper
    _hook(monkeypatch, hook)
    sample_set = mapper.SampleSet(cells['index'], True, per_sample_lengths=True, umi_bases=16, umi_mismatches=mismatches)
    for s in (1, 0, 2):                       # (the samples in any order)
        units = cells['samples'][s]
        _add_sample(sample_set, s, units, umis=[m for _, m in units], cuts=(2, 700) if hook and s == 0 else ())
    tx_gene, n_genes = cells['tx_gene'], cells['n_genes']
    before = sample_set.gene_resolved_matrix(tx_gene, n_genes)
    got = sample_set.gene_distributed_matrix(tx_gene, n_genes)
    emref.check_csr(*got[:3], N_CELLS, n_genes)
    print('entries %d, tally %r, to_unnamed %r' % (got[2].size, got[3].sum(axis=0).tolist(), got[4].tolist()))
    _same_bits(got, cells['want'][mismatches], NAMES)
    _same_bits(sample_set.gene_distributed_matrix(tx_gene, n_genes), got, NAMES)      # (the set is read, not used up)
    after = sample_set.gene_resolved_matrix(tx_gene, n_genes)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    # the tally identities against the resolved matrix of the same set, which is the reference's
    np.testing.assert_array_equal(after[3], cells['resolved'][mismatches])
    np.testing.assert_array_equal(got[3][:, [emref.RESOLVED, emref.UNNAMED, emref.COLLISION]],
                                  after[3][:, [mres.RESOLVED, mres.UNNAMED, mres.COLLISION]])
    np.testing.assert_array_equal(got[3][:, emref.DISTRIBUTED] + got[3][:, emref.WIDE], after[3][:, mres.MULTI])


def test_a_set_without_umis_or_without_units(cells, native_libs):
    from seekmer_amd import mapper
    tx_gene, n_genes = cells['tx_gene'], cells['n_genes']
    plain = mapper.SampleSet(cells['index'], True, per_sample_lengths=True)
    _add_sample(plain, 0, cells['samples'][2][:50])
    with pytest.raises(native_libs.NativeError) as error:
        plain.gene_distributed_matrix(tx_gene, n_genes)
    assert error.value.code == native_libs.SKM_ERR_STATE
    handle = ctypes.c_void_p(1)
    assert native_libs.hip().skm_sample_set_distributed_matrix(plain._handle, tx_gene.size, n_genes,
                                                               native_libs.ptr(tx_gene, native_libs.c_i32p),
                                                               ctypes.byref(handle)) == native_libs.SKM_ERR_STATE
    assert handle.value is None
    empty = mapper.SampleSet(cells['index'], True, per_sample_lengths=True, umi_bases=16)
    indptr, indices, data, tally, to_unnamed = empty.gene_distributed_matrix(tx_gene, n_genes)
    assert indptr.tolist() == [0] and indices.size == 0 and data.size == 0 and tally.shape == (0, 8) and to_unnamed.size == 0


# ---- command line -------------------------------------------------------------------------------------------------
BARCODES = [b'ACGTACGTAC', b'TTGCAAGGCT', b'GGATCCTTAG']
CELLS = ['cell0', 'cell1', 'cell2']
EM_FILES = ['molecules.em.mtx', 'molecules.em.npz', 'molecules.em.tsv']


@pytest.fixture(scope='module')
def cli_inputs(oracle, native_libs, chr21, chr21_oracle_index, tmp_path_factory):
    """A pooled run of three cells in the style of tests/test_gpu_molecule_resolve.py's: every molecule is two different
    fragments of one transcript under one UMI of 8 bases, each written once or twice; genes of TWO transcripts, every
    tenth unnamed, so that the classes of a molecule's fragments often span genes."""
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('distribute_cli')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    index_path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(index_path)]) == 0
    ids = [id_.split()[0].split(b'.')[0] for id_ in chr21[0]]
    map_path = folder / 'genes.tsv'
    gene_name = [b'G%05d' % (t // 2) if (t // 2) % 10 else b'' for t in range(len(ids))]
    with open(map_path, 'wb') as f:
        for id_, name in zip(ids, gene_name):
            if name:
                f.write(id_ + b'\t' + name + b'\n')
    (folder / 'whitelist.tsv').write_bytes(b''.join(b'%s\t%s\n' % (code, name.encode()) for code, name in zip(BARCODES, CELLS)))
    rng = np.random.default_rng(1213)
    mates, tags, cell = ([], []), [], []
    for c, n_molecules in enumerate((200, 120, 160)):
        for _ in range(n_molecules):
            umi = bytes(b'ACGT'[int(k)] for k in rng.integers(0, 4, 8))
            for pair in _two_fragments(chr21[1], rng):
                for _ in range(int(rng.integers(1, 3))):
                    mates[0].append(pair[0]), mates[1].append(pair[1]), tags.append(BARCODES[c] + umi + b'TTTT'), cell.append(c)
    order = rng.permutation(len(tags))
    pooled = [folder / 'pool_1.fastq', folder / 'pool_2.fastq', folder / 'pool_barcodes.fastq']
    reads = [[mates[0][u] for u in order], [mates[1][u] for u in order]]
    _write_fastq(pooled[0], reads[0])
    _write_fastq(pooled[1], reads[1])
    _write_fastq(pooled[2], [tags[u] for u in order])
    cell = np.asarray(cell)[order]
    umi, readable = ref.windows([tags[u].decode() for u in order], 10, 8)
    assert readable.all()
    tuples = oracle.map_batch(chr21_oracle_index, *oracle.pack_reads([m for pair in zip(*reads) for m in pair]), len(order), True).tuples()
    return dict(index=index_path, map=map_path, files=[str(f) for f in pooled], whitelist=str(folder / 'whitelist.tsv'),
                cell=cell, umi=umi, tuples=tuples, stay=ref.survivors(cell, umi, tuples), gene_name=gene_name)


def _pooled_run(cli_inputs, out, *options):
    from seekmer_amd import __main__ as cli
    mate1, mate2, barcode_file = cli_inputs['files']
    assert cli.main(['infer-many', str(cli_inputs['index']), str(out), mate1, mate2, '--barcodes', cli_inputs['whitelist'],
                     '--barcode-file', barcode_file, '--umi-start', '10', '--umi-length', '8', '--gene-map', str(cli_inputs['map']),
                     *options]) == 0
    return out


def test_distribute_molecules_on_pooled_files(cli_inputs, tmp_path):
    from seekmer_amd import infer
    os.environ.pop('SKM_INFER_MANY_PER_SAMPLE', None)
    ours = _pooled_run(cli_inputs, tmp_path / 'with', '--matrix-only', '--distribute-molecules')
    without = _pooled_run(cli_inputs, tmp_path / 'without', '--matrix-only', '--resolve-molecules')
    assert sorted(f.name for f in ours.iterdir()) == sorted(f.name for f in without.iterdir())
    others = sorted(f.name for f in (without / 'counts').iterdir())
    assert sorted(f.name for f in (ours / 'counts').iterdir()) == sorted(others + EM_FILES) and 'molecules.resolved.mtx' in others
    for name in others:
        assert (ours / 'counts' / name).read_bytes() == (without / 'counts' / name).read_bytes(), name
    for name in ('barcodes.json', 'barcodes.tsv', 'samples.tsv'):
        assert (ours / name).read_bytes() == (without / name).read_bytes(), name
    # the reference, from the oracle's classes of the pooled reads and the genes in the order of genes.tsv
    genes = (ours / 'counts' / 'genes.tsv').read_bytes().splitlines()
    number = {name: g for g, name in enumerate(genes)}
    tx_gene = np.asarray([number[name] if name else -1 for name in cli_inputs['gene_name']], dtype=np.int32)
    cell, umi, tuples, stay = (cli_inputs[k] for k in ('cell', 'umi', 'tuples', 'stay'))
    indptr, indices, data, tally, to_unnamed = emref.matrix(cell, umi, tuples, stay, tx_gene, 3, len(genes))
    print('tally %r, to_unnamed %r' % (tally.tolist(), to_unnamed.tolist()))
    lines = (ours / 'counts' / 'molecules.em.mtx').read_text().splitlines(keepends=True)
    assert lines[0] == '%%MatrixMarket matrix coordinate real general\n' and lines[1] == infer.DISTRIBUTED_MATRIX_COMMENT + '\n'
    assert lines[2] == '%d 3 %d\n' % (len(genes), data.size)
    sample_of = np.repeat(np.arange(3), np.diff(indptr))
    assert lines[3:] == ['%d %d %r\n' % (g + 1, s + 1, float(v)) for s, g, v in zip(sample_of, indices, data)]
    arrays = np.load(ours / 'counts' / 'molecules.em.npz')
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [3, len(genes)]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and arrays[name].tobytes() == want.tobytes(), name
    rows = [line.split('\t') for line in (ours / 'counts' / 'molecules.em.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == CELLS
    for s, row in enumerate(rows):
        assert [int(v) for v in row[1:11]] == [int(tally[s, :5].sum())] + tally[s].tolist() + [int(indptr[s + 1] - indptr[s])]
        assert row[11] == repr(float(to_unnamed[s]))
    # what the fixture is for: sets in every cell, shares among the weights
    assert tally[:, emref.DISTRIBUTED].min() >= 5 and (data != np.round(data)).any()
    # with the cells' own folders (no --matrix-only): they are what they are without the option
    from test_gpu_genes import _same_folder
    full = _pooled_run(cli_inputs, tmp_path / 'full', '--distribute-molecules')
    plain = _pooled_run(cli_inputs, tmp_path / 'plain', '--resolve-molecules')
    for name in CELLS:
        _same_folder(full / name, plain / name)
    for name in EM_FILES:
        assert (full / 'counts' / name).read_bytes() == (ours / 'counts' / name).read_bytes(), name
