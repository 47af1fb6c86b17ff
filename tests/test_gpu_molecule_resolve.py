"""Resolved molecules on the device ("Resolved molecules") against
tests/molecule_resolve_reference.py, exactly: host classes and molecules through
skm_gene_matrix_from_molecule_classes (the sort, group, resolve and fill steps at their edges); a sample set's resident
state through SampleSet.gene_resolved_matrix, with the classes the reference intersects taken from the oracle, never
from the code under test; the same under umi_mismatches=1 (survivors of tests/umi_mismatch_reference.py); and
`infer-many --resolve-molecules` on pooled files."""
import ctypes
import os

import numpy as np
import pytest

import gene_matrix_reference as mref
import molecule_reference as mol
import molecule_resolve_reference as mres
import umi_mismatch_reference as near_ref
import umi_reference as ref
from conftest import GOLDEN, make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu

READ_LEN = 75
UMI_ZERO, UMI_ONES = 0, 2 ** 32 - 1
NAMES = ('indptr', 'indices', 'data', 'tally')


# ---- the host door ------------------------------------------------------------------------------------------------
def _csr_of(class_tuples):
    offsets = np.zeros(len(class_tuples) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(t) for t in class_tuples])
    targets = np.asarray([x for t in class_tuples for x in t], dtype=np.int32)
    return offsets, targets


def _door(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes):
    """the device's four arrays, equal to the reference's"""
    from seekmer_amd import mapper
    got = mapper.resolved_molecule_matrix(*_csr_of(class_tuples), class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes)
    mref.check_csr(*got[:3], n_samples, n_genes)
    want = mres.matrix_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples)
    for name, a, b in zip(NAMES, got, want):
        np.testing.assert_array_equal(a, b, err_msg=name)
    tally = got[3]
    assert tally.shape == (n_samples, 5) and tally.dtype == np.int64
    distinct = np.zeros(n_samples, dtype=np.int64)
    for s, _ in {(int(class_sample[int(k)]), int(m)) for k, m in zip(mol_class, mol_umi)}:
        distinct[s] += 1
    np.testing.assert_array_equal(tally[:, [0, 2, 3, 4]].sum(axis=1), distinct)
    assert (tally[:, 1] <= tally[:, 0]).all()
    resolved = np.zeros(n_samples, dtype=np.int64)
    np.add.at(resolved, np.repeat(np.arange(n_samples), np.diff(got[0])), got[2])
    np.testing.assert_array_equal(resolved, tally[:, 0])
    return got


def _random_case(n):
    """about 40 classes of 1 to 12 ids over 30 transcripts, 9 genes and some -1, 5 cells and an empty sixth, 9 UMIs;
    every (cell, UMI) draws from a pool of 1 to 6 of the cell's classes"""
    rng = np.random.default_rng(1000 + n)
    tx_gene = (np.arange(30) // 3).astype(np.int32)
    tx_gene[tx_gene == 9] = -1
    tx_gene[[4, 13]] = -1
    class_tuples, class_sample = [], []
    for k in range(40):
        cell, shape = k % 5, k // 5
        block = lambda g: rng.permutation(np.flatnonzero(np.arange(30) // 3 == g))
        strangers = lambda low, high: rng.integers(0, 27, int(rng.integers(low, high)))
        if shape == 0:                        # inside the cell's block of three transcripts
            t = block(cell)[:int(rng.integers(1, 4))]
        elif shape in (1, 2, 3):              # one or two of the block and a few strangers, or many
            t = np.concatenate([block(cell)[:1 + shape % 2], strangers(1, 4) if shape < 3 else strangers(6, 11)])
        elif shape == 4:                      # another block and strangers
            t = np.concatenate([block(cell + 5)[:2], strangers(1, 4)])
        elif shape == 5:                      # wide
            t = strangers(6, 13)
        else:                                 # unnamed transcripts, with company in the last
            t = np.concatenate([[27, 28][:int(rng.integers(1, 3))], strangers(0, 1) if shape == 6 else strangers(1, 2)])
        class_tuples.append(tuple(int(x) for x in dict.fromkeys(int(x) for x in t)))
        class_sample.append(cell)
    class_sample = np.asarray(class_sample, dtype=np.int32)
    pools = []
    for cell in range(5):
        mine = np.flatnonzero(class_sample == cell)
        for umi in range(9):
            pools.append((umi, rng.choice(mine, size=int(rng.integers(1, 7)))))
    group = rng.integers(0, len(pools), n)
    mol_class = np.asarray([int(rng.choice(pools[g][1])) for g in group], dtype=np.int32)
    mol_umi = np.asarray([pools[g][0] for g in group], dtype=np.uint32)
    return class_tuples, class_sample, mol_class, mol_umi, tx_gene


def test_the_random_case_is_not_trivial():
    """the reference alone: all five outcomes and a rescued group occur at n = 3000, in groups of several classes"""
    class_tuples, class_sample, mol_class, mol_umi, tx_gene = _random_case(3000)
    _, tally = mres.from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene)
    total = np.asarray(list(tally.values())).sum(axis=0)
    print('resolved %d, rescued %d, multi-gene %d, unnamed %d, collision %d' % tuple(total))
    assert (total > 0).all()
    sizes = {}
    for k, m in zip(mol_class, mol_umi):
        sizes.setdefault((int(class_sample[k]), int(m)), set()).add(int(k))
    assert {len(v) for v in sizes.values()} >= {1, 2, 3, 4} and len(sizes) == 45


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 3000])
def test_random_molecules(native_libs, n):
    class_tuples, class_sample, mol_class, mol_umi, tx_gene = _random_case(n)
    got = _door(class_tuples, class_sample, mol_class, mol_umi, tx_gene, 6, 9)
    assert got[0][5] == got[0][6] and not got[3][5].any()               # (sample 5 is empty)
    # the same molecules in another order: identical arrays
    order = np.random.default_rng(n).permutation(n)
    again = _door(class_tuples, class_sample, mol_class[order], mol_umi[order], tx_gene, 6, 9)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def _own_genes(n_tx):
    """every transcript a gene of its own: a class's gene set is its ids"""
    return np.arange(n_tx, dtype=np.int32)


def test_groups_across_a_wave_and_across_a_block(native_libs):
    """a 3-class group at sorted places 63..65 and another at 255..257, single-class groups of smaller keys ahead"""
    tx_gene = _own_genes(20)
    class_tuples = [(0,), (1, 2), (1, 3), (1, 4, 5)]
    mol_class, mol_umi = [], []
    for umi in range(252):                   # places 0..62, then 66..254: one class each
        if umi == 63:
            mol_class += [1, 2, 3]; mol_umi += [1000] * 3
        mol_class.append(0); mol_umi.append(umi if umi < 63 else 1000 + umi)
    mol_class += [3, 2, 1]; mol_umi += [5000] * 3
    assert len(mol_umi) == 258 and sorted(mol_umi).index(1000) == 63 and sorted(mol_umi).index(5000) == 255
    got = _door(class_tuples, np.zeros(4, dtype=np.int32), mol_class, mol_umi, tx_gene, 1, 20)
    assert got[1].tolist() == [0, 1] and got[2].tolist() == [252, 2] and got[3].tolist() == [[254, 2, 0, 0, 0]]


@pytest.mark.parametrize('lacking', [False, True])
def test_groups_of_130_and_of_1000_classes(native_libs, lacking):
    """all classes of a group hold transcript 0 beside one of their own -- or all but one do"""
    n_tx = 1200
    tx_gene = (1 + np.arange(n_tx) % 50).astype(np.int32)
    tx_gene[0] = 0
    class_tuples = [(1 + k, 0) if k % 2 else (0, 1 + k) for k in range(1130)]
    if lacking:
        class_tuples[77] = (78,)
        class_tuples[130 + 999] = (1130,)
    class_sample = np.asarray([0] * 130 + [1] * 1000, dtype=np.int32)
    order = np.random.default_rng(3).permutation(1130)
    got = _door(class_tuples, class_sample, np.arange(1130)[order], np.full(1130, 7), tx_gene, 2, 51)
    if lacking:
        assert got[2].size == 0 and got[3][:, 0].tolist() == [0, 0] and got[3][:, [2, 4]].sum(axis=1).tolist() == [1, 1]
    else:
        assert got[1].tolist() == [0, 0] and got[2].tolist() == [1, 1] and got[3].tolist() == [[1, 1, 0, 0, 0]] * 2


LENGTHS = [8, 9, 64, 65, 200]


def test_tuple_lengths_as_pivot_and_as_member(native_libs):
    """every pair of lengths, the two classes sharing their first id alone; and every length alone"""
    tx_gene = _own_genes(5000)
    class_tuples, mol_class, mol_umi, fresh = [], [], [], 100
    for a in LENGTHS:
        for b in LENGTHS:
            shared = len(class_tuples) // 2
            for length in (a, b):
                class_tuples.append((shared,) + tuple(range(fresh, fresh + length - 1)))
                fresh += length - 1
                mol_class.append(len(class_tuples) - 1); mol_umi.append(shared)
    for length in LENGTHS:                   # single-class groups: multi-gene, by the lane or by the wave
        class_tuples.append(tuple(range(fresh, fresh + length)))
        fresh += length
        mol_class.append(len(class_tuples) - 1); mol_umi.append(10000 + length)
    assert fresh <= 5000
    got = _door(class_tuples, np.zeros(len(class_tuples), dtype=np.int32), mol_class, mol_umi, tx_gene, 1, 5000)
    assert got[1].tolist() == list(range(25)) and got[3].tolist() == [[25, 25, 5, 0, 0]]


@pytest.mark.parametrize('at', [0, 8, 63, 64, 127, 199])
def test_the_surviving_gene_at_any_place(native_libs, at):
    """two classes of 200 and 230 ids: the shared one at place `at` of the pivot, at the mirrored place of the member"""
    tx_gene = _own_genes(1000)
    pivot = list(range(100, 300))
    member = list(range(400, 630))
    pivot[at] = member[229 - at] = 7
    single = tuple(range(700, 900)) + (7,)                  # and a long class inside no gene alone: multi-gene
    got = _door([tuple(pivot), tuple(member), single], np.zeros(3, dtype=np.int32), [1, 0, 2], [5, 5, 6], tx_gene, 1, 1000)
    assert got[1].tolist() == [7] and got[3].tolist() == [[1, 1, 1, 0, 0]]
    # a long class inside one gene, the last id included, beside it: resolved, not rescued
    tx_gene = np.zeros(1000, dtype=np.int32)
    tx_gene[400:] = np.arange(600) + 1
    got = _door([tuple(range(200)), (at,) + tuple(range(400, 600))], np.zeros(2, dtype=np.int32), [0, 1], [5, 5], tx_gene, 1, 601)
    assert got[1].tolist() == [0] and got[3].tolist() == [[1, 0, 0, 0, 0]]


def test_named_intersections(native_libs):
    #          transcripts 0 1 2 in gene 0, 3 4 in gene 1, 5 6 unnamed, 7 in gene 2
    tx_gene = np.asarray([0, 0, 0, 1, 1, -1, -1, 2], dtype=np.int32)
    cases = [                                                 # (classes of one group, [resolved, rescued, multi, unnamed, collision], gene)
        ([(0, 1, 7), (2, 3, 4, 5)], [1, 1, 0, 0, 0], 0),      # a pivot that holds the gene several times
        ([(0, 1, 2), (1, 3, 4, 7)], [1, 0, 0, 0, 0], 0),      # ... and nothing else: a class inside the gene
        ([(0, 1, 3), (2, 0, 7), (1, 2, 7, 5)], [1, 1, 0, 0, 0], 0),
        ([(0, 3, 7), (4, 1)], [0, 0, 1, 0, 0], None),         # {g, h}
        ([(0, 5), (6, 1, 7)], [0, 0, 1, 0, 0], None),         # {g, -1}
        ([(5, 0), (6, 3)], [0, 0, 0, 1, 0], None),            # {-1}
        ([(5,), (6,)], [0, 0, 0, 1, 0], None),
        ([(0, 1), (3,)], [0, 0, 0, 0, 1], None),              # empty
        ([(0, 3), (3, 7), (7, 0)], [0, 0, 0, 0, 1], None),    # empty, every two of the three meet
        ([(0, 1), (2, 3)], [1, 0, 0, 0, 0], 0),               # a class inside the gene among them: not rescued
    ]
    for classes, tally, gene in cases:
        got = _door(classes, np.zeros(len(classes), dtype=np.int32), np.arange(len(classes)), np.full(len(classes), 9), tx_gene, 1, 3)
        assert got[3].tolist() == [tally] and got[1].tolist() == ([] if gene is None else [gene]), classes
    # all of them at once, a group per UMI
    class_tuples = [t for classes, _, _ in cases for t in classes]
    mol_umi = [u for u, (classes, _, _) in enumerate(cases) for _ in classes]
    got = _door(class_tuples, np.zeros(len(class_tuples), dtype=np.int32), np.arange(len(class_tuples)), mol_umi, tx_gene, 1, 3)
    assert got[3].tolist() == [np.asarray([tally for _, tally, _ in cases]).sum(axis=0).tolist()]


def test_named_molecules(native_libs):
    tx_gene = np.asarray([0, 0, 1, 1], dtype=np.int32)
    class_tuples = [(0, 2), (1, 3), (0, 1), (2,), (0, 2)]
    class_sample = np.asarray([0, 0, 0, 0, 1], dtype=np.int32)
    # duplicate (class, UMI) molecules count as one: a group of one class, three times over, is a group of one class
    got = _door(class_tuples, class_sample, [2, 2, 2, 0, 0], [4, 4, 4, 5, 5], tx_gene, 2, 2)
    assert got[3].tolist() == [[1, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    # the same UMI in two cells: two groups
    got = _door(class_tuples, class_sample, [2, 4], [4, 4], tx_gene, 2, 2)
    assert got[3].tolist() == [[1, 0, 0, 0, 0], [0, 0, 1, 0, 0]]
    # UMI 0 and UMI 2^32 - 1, a group of two classes each, in one cell and in its neighbour
    got = _door(class_tuples, class_sample, [0, 2, 0, 3, 4], [UMI_ZERO, UMI_ZERO, UMI_ONES, UMI_ONES, UMI_ONES], tx_gene, 2, 2)
    assert got[1].tolist() == [0, 1] and got[3].tolist() == [[2, 0, 0, 0, 0], [0, 0, 1, 0, 0]]
    # the last sample of 65 536 and the last gene of 70 001
    tx_gene = np.asarray([70000, 70000, 0, 5], dtype=np.int32)
    class_sample = np.asarray([65535, 65535, 65535, 0, 65535], dtype=np.int32)
    got = _door(class_tuples, class_sample, [0, 1, 2, 3, 4], [1, 1, 2, 1, 1], tx_gene, 65536, 70001)
    assert got[0][-1] == 2 and got[0][1] == 1 and got[1].tolist() == [0, 70000] and got[2].tolist() == [1, 2]
    assert got[3][65535].tolist() == [2, 1, 0, 0, 0] and got[3][0].tolist() == [1, 0, 0, 0, 0]


def test_bad_input_gives_no_handle(native_libs):
    hip = native_libs.hip()
    good = dict(offsets=[0, 2, 3], targets=[0, 1, 2], sample=[0, 1], mol_class=[0, 1], n_tx=3)
    bad = [dict(mol_class=[0, 2]), dict(mol_class=[-1, 0]), dict(sample=[0, 2]), dict(sample=[-1, 0]), dict(targets=[0, 3, 2]),
           dict(targets=[0, -1, 2]), dict(offsets=[0, 3, 3]), dict(n_tx=2)]
    for n_bad, change in enumerate([{}] + bad):
        case = dict(good, **change)
        offsets = np.asarray(case['offsets'], dtype=np.int64)
        targets, sample, mol_class = (np.asarray(case[k], dtype=np.int32) for k in ('targets', 'sample', 'mol_class'))
        umi, tx_gene = np.asarray([1, 2], dtype=np.uint32), np.asarray([0, 0, 1][:case['n_tx']], dtype=np.int32)
        handle = ctypes.c_void_p(1)
        code = hip.skm_gene_matrix_from_molecule_classes(
            0, 2, native_libs.ptr(offsets, native_libs.c_i64p), native_libs.ptr(targets, native_libs.c_i32p),
            native_libs.ptr(sample, native_libs.c_i32p), 2, native_libs.ptr(mol_class, native_libs.c_i32p),
            native_libs.ptr(umi, native_libs.c_u32p), 2, case['n_tx'], 2, native_libs.ptr(tx_gene, native_libs.c_i32p),
            ctypes.byref(handle))
        if n_bad == 0:
            assert code == 0 and handle.value
            hip.skm_gene_matrix_destroy(handle)
        else:
            assert code == native_libs.SKM_ERR_ARG and handle.value is None, change
    assert hip.skm_sample_set_resolved_matrix(None, 0, 0, None, None) == native_libs.SKM_ERR_ARG
    # the tally of a handle that holds a count matrix
    arrays = [np.asarray([0, 1], dtype=np.int32), np.asarray([0, 0], dtype=np.int32), np.asarray([1, 2], dtype=np.uint32)]
    handle = ctypes.c_void_p()
    assert hip.skm_gene_matrix_from_molecules(0, 2, native_libs.ptr(arrays[0], native_libs.c_i32p),
                                              native_libs.ptr(arrays[1], native_libs.c_i32p),
                                              native_libs.ptr(arrays[2], native_libs.c_u32p), 3, 5, ctypes.byref(handle)) == 0
    tally = np.zeros((3, 5), dtype=np.int64)
    try:
        assert hip.skm_gene_matrix_read_tally(handle, native_libs.ptr(tally, native_libs.c_i64p)) == native_libs.SKM_ERR_STATE
    finally:
        hip.skm_gene_matrix_destroy(handle)


# ---- the set, directly (helpers: copies of tests/test_gpu_molecule_matrix.py's, which is free to change) -----------
N_SYNTH_GENES = 600
DISTINCT = 2500                   # distinct pairs a cell
N_CELLS = 4


@pytest.fixture(scope='module')
def transcriptome(oracle, native_libs):
    """(ids, pool, tx_offsets, oracle index, product index over the same arrays, tx_gene, n_genes, block).  tx_gene is
    the test's own: transcripts that some class of 40 000 oracle-mapped pairs holds together form a block, numbered in
    the order of their first transcript, and a block is a gene -- but in every fifth block every transcript is a gene
    of its own (a split block), and every tenth block is unnamed."""
    from seekmer_amd import synth
    ids, pool, tx_offsets = synth.transcriptome(5, N_SYNTH_GENES)
    oindex = oracle.build_index(synth.sequences_of(pool, tx_offsets), ids)
    n_tx = len(ids)
    parent = list(range(n_tx))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    probe = synth.reads(7, pool, tx_offsets, 900000, 40000, READ_LEN, True)
    for t in set(oracle.map_batch(oindex, probe[0], probe[1], 40000, True).tuples()):
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
    return ids, pool, tx_offsets, oindex, make_product_index(oindex, ids), tx_gene.astype(np.int32), n_genes, block


def _pairs(pool, tx_offsets, seed, first, n):
    from seekmer_amd import synth
    raw = synth.reads(seed, pool, tx_offsets, first, n, READ_LEN, True)[0][:-1].tobytes()
    return [(raw[2 * u * READ_LEN:(2 * u + 1) * READ_LEN], raw[(2 * u + 1) * READ_LEN:(2 * u + 2) * READ_LEN]) for u in range(n)]


def _classes(oracle, oindex, pairs):
    return oracle.map_batch(oindex, *oracle.pack_reads([read for pair in pairs for read in pair]), len(pairs), True).tuples()


def _chosen_pairs(classes, block):
    """places (i, j) of two distinct pairs of the cell that get one UMI, every place in one pair at most: in the split
    blocks two classes that cross -- in one transcript (both of several: rescued; one of them that transcript alone:
    resolved, not rescued), or in two or more (multi-gene) --, and two classes of neighbouring named blocks (collision)"""
    by_block = {}
    for i, t in enumerate(classes):
        if t:
            by_block.setdefault(int(block[t[0]]), {}).setdefault(t, i)
    used, out = set(), dict(rescued=[], resolved=[], multi=[], collision=[])
    for b in sorted(by_block):
        if b % 10 != 5:
            continue
        items = sorted(by_block[b].items())
        for x, (ta, i) in enumerate(items):
            for tb, j in items[x + 1:]:
                if i in used or j in used:
                    continue
                shared = len(set(ta) & set(tb))
                if shared == 1 and len(ta) > 1 and len(tb) > 1:
                    kind = 'rescued'
                elif shared == 1:
                    kind = 'resolved'
                elif shared >= 2:
                    kind = 'multi'
                else:
                    continue
                if len(out[kind]) > min(len(v) for k, v in out.items() if k != 'collision') + 5:
                    continue              # (the kinds share the places of the split blocks: none takes them all)
                out[kind].append((i, j))
                used |= {i, j}
    named = [b for b in sorted(by_block) if b % 10 not in (0, 5)]
    for a, b in zip(named[0:60:2], named[1:60:2]):
        out['collision'].append((min(by_block[a].values()), min(by_block[b].values())))
    return out


@pytest.fixture(scope='module')
def cells(oracle, transcriptome):
    """N_CELLS cells of units (pair, UMI): every distinct pair one to three times under a UMI of its own, but the
    chosen pairs of pairs under one.  Cell 0 begins with units that under umi_mismatches=1 take the first class away
    from five of its rescued groups: the same pair under a UMI one substitution away."""
    ids, pool, tx_offsets, oindex, index, tx_gene, n_genes, block = transcriptome
    rng = np.random.default_rng(17)
    samples = []
    for s in range(N_CELLS):
        distinct = _pairs(pool, tx_offsets, 60 + s, s * 50000, DISTINCT)
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
            units = [(distinct[i], umi_of[i] ^ 1) for i, _ in chosen['rescued'][:5]] + units
        samples.append(units)
    reads = [read for units in samples for pair, _ in units for read in pair]
    sample = np.repeat(np.arange(N_CELLS), [len(units) for units in samples]).astype(np.int32)
    umi = np.asarray([m for units in samples for _, m in units], dtype=np.uint32)
    tuples = oracle.map_batch(oindex, *oracle.pack_reads(reads), sample.size, True).tuples()
    stay = {0: ref.survivors(sample, umi, tuples), 1: near_ref.survivors(sample, umi, tuples, 16, 1)}
    want = {k: mres.matrix(sample, umi, tuples, stay[k], tx_gene, N_CELLS) for k in stay}
    return dict(samples=samples, sample=sample, umi=umi, tuples=tuples, stay=stay, want=want, index=index, tx_gene=tx_gene,
                n_genes=n_genes)


def _kinds(cells, mismatches):
    """the groups of several classes by kind, and the unnamed groups: from the reference's verdicts"""
    groups = {}
    for c, m, t, keep in zip(cells['sample'], cells['umi'], cells['tuples'], cells['stay'][mismatches]):
        if keep and t:
            groups.setdefault((int(c), int(m)), set()).add(t)
    count = dict(rescued=0, resolved=0, multi=0, collision=0, unnamed=0, several=0)
    for classes in groups.values():
        outcome, _, rescued = mres.verdict([mres.gene_set(t, cells['tx_gene']) for t in classes])
        count['unnamed'] += outcome == mres.UNNAMED
        if len(classes) > 1:
            count['several'] += 1
            count['rescued'] += bool(rescued)
            count['resolved'] += outcome == mres.RESOLVED and not rescued
            count['multi'] += outcome == mres.MULTI
            count['collision'] += outcome == mres.COLLISION
    return count


def test_the_cells_are_not_trivial(cells):
    """the reference alone, before the device is asked: at least 20 groups of each of the four kinds, 20 unnamed"""
    for mismatches in (0, 1):
        count = _kinds(cells, mismatches)
        print('umi_mismatches=%d: %r' % (mismatches, count))
        assert min(count[k] for k in ('rescued', 'resolved', 'multi', 'collision', 'unnamed')) >= 20, count
    # what the five leading units of cell 0 change under umi_mismatches=1
    assert _kinds(cells, 1)['rescued'] <= _kinds(cells, 0)['rescued'] - 3
    assert (cells['stay'][0] & ~cells['stay'][1]).sum() >= 5 and (~cells['stay'][0]).sum() > 1000
    # a pattern of its own: entries the molecule matrix lacks, and the other way round
    resolved = set(mres.resolve(cells['sample'], cells['umi'], cells['tuples'], cells['stay'][0], cells['tx_gene'])[0])
    counted = set(mol.entries(cells['sample'], cells['umi'], cells['tuples'], cells['stay'][0], cells['tx_gene'])[0])
    assert resolved - counted and counted - resolved


def _add_sample(sample_set, s, units, umis=None, cuts=()):
    """the units (pair, umi) of sample s as packed segments cut at `cuts`"""
    from seekmer_amd import common
    from oracle import oracle
    bounds = [0] + list(cuts) + [len(units)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        pieces = [common.PackedReads.from_ascii(*oracle.pack_reads([pair[mate] for pair, _ in units[lo:hi]]), stream=mate)
                  for mate in (0, 1)]
        if umis is None:
            sample_set.add_packed(s, lo, *pieces)
        else:
            sample_set.add_packed(s, lo, *pieces, umis=np.asarray(umis[lo:hi], dtype=np.uint32))


def _hook(monkeypatch, hook):
    for name in ('SKM_SAMPLE_SET_MAX_UNITS', 'SKM_TEST_UMI_SLOTS', 'SKM_TEST_MAP_BLOCKS'):
        monkeypatch.delenv(name, raising=False)
    for pair in hook or ():
        monkeypatch.setenv(*pair.split('='))


@pytest.mark.parametrize('mismatches,hook', [(0, None), (1, None), (1, ('SKM_TEST_UMI_SLOTS=2', 'SKM_SAMPLE_SET_MAX_UNITS=500'))])
def test_the_resolved_matrix_of_a_set_is_the_reference(cells, monkeypatch, mismatches, hook):
    """2 slots and launches of 500 units: the molecule set grows after the launch that marked molecules dropped"""
    from seekmer_amd import mapper
    _hook(monkeypatch, hook)
    sample_set = mapper.SampleSet(cells['index'], True, per_sample_lengths=True, umi_bases=16, umi_mismatches=mismatches)
    for s in (1, 0, 3, 2):                    # (the samples in any order)
        units = cells['samples'][s]
        _add_sample(sample_set, s, units, umis=[m for _, m in units], cuts=(2, 700) if hook and s == 0 else ())
    tx_gene, n_genes = cells['tx_gene'], cells['n_genes']
    before = sample_set.gene_molecule_matrix(tx_gene, n_genes), sample_set.gene_count_matrix(tx_gene, n_genes)
    got = sample_set.gene_resolved_matrix(tx_gene, n_genes)
    mref.check_csr(*got[:3], N_CELLS, n_genes)
    print('entries %d, tally %r' % (got[2].size, got[3].sum(axis=0).tolist()))
    for name, a, b in zip(NAMES, got, cells['want'][mismatches]):
        np.testing.assert_array_equal(a, b, err_msg=name)
    again = sample_set.gene_resolved_matrix(tx_gene, n_genes)             # (the set is read, not used up)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    after = sample_set.gene_molecule_matrix(tx_gene, n_genes), sample_set.gene_count_matrix(tx_gene, n_genes)
    for was, now in zip(before, after):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(was, now))
    # and the molecule matrix is the reference's still: the same population
    want = mol.matrix(cells['sample'], cells['umi'], cells['tuples'], cells['stay'][mismatches], tx_gene, N_CELLS)
    for a, b in zip(after[0], want):
        np.testing.assert_array_equal(a, b)


def test_a_set_without_umis_or_without_units(cells, native_libs):
    from seekmer_amd import mapper
    tx_gene, n_genes = cells['tx_gene'], cells['n_genes']
    plain = mapper.SampleSet(cells['index'], True, per_sample_lengths=True)
    _add_sample(plain, 0, cells['samples'][2][:50])
    with pytest.raises(native_libs.NativeError) as error:
        plain.gene_resolved_matrix(tx_gene, n_genes)
    assert error.value.code == native_libs.SKM_ERR_STATE
    handle = ctypes.c_void_p(1)
    assert native_libs.hip().skm_sample_set_resolved_matrix(plain._handle, tx_gene.size, n_genes,
                                                            native_libs.ptr(tx_gene, native_libs.c_i32p),
                                                            ctypes.byref(handle)) == native_libs.SKM_ERR_STATE
    assert handle.value is None
    empty = mapper.SampleSet(cells['index'], True, per_sample_lengths=True, umi_bases=16)
    indptr, indices, data, tally = empty.gene_resolved_matrix(tx_gene, n_genes)
    assert indptr.tolist() == [0] and indices.size == 0 and data.size == 0 and tally.shape == (0, 5)
    with pytest.raises(ValueError):           # a gene map that does not cover the index's transcripts
        empty.gene_resolved_matrix(tx_gene[:-1], n_genes)


# ---- command line -------------------------------------------------------------------------------------------------
BARCODES = [b'ACGTACGTAC', b'TTGCAAGGCT', b'GGATCCTTAG']
CELLS = ['cell0', 'cell1', 'cell2']
COUNT_FILES = ['cells.tsv', 'genes.tsv', 'matrix.mtx', 'matrix.npz', 'molecules.mtx', 'molecules.npz']
RESOLVED_FILES = ['molecules.resolved.mtx', 'molecules.resolved.npz', 'molecules.resolved.tsv']


def _write_fastq(path, reads):
    with open(path, 'wb') as f:
        for u, read in enumerate(reads):
            f.write(b'@u%d\n' % u + read + b'\n+\n' + b'I' * len(read) + b'\n')


def _two_fragments(seqs, rng, read_len=60):
    """two different fragments of one transcript, either mate first"""
    long_tx = [s.upper() for s in seqs if len(s) > 450 and set(s.upper()) <= set(b'ACGT')]
    s = long_tx[int(rng.integers(len(long_tx)))]
    out = []
    for _ in range(2):
        frag = int(rng.integers(150, 401))
        at = int(rng.integers(0, len(s) - frag + 1))
        f = s[at:at + frag]
        mates = [bytes(f[:read_len]), bytes(reverse_complement(f[-read_len:]))]
        if rng.integers(2):
            mates.reverse()
        out.append(mates)
    return out


@pytest.fixture(scope='module')
def cli_inputs(oracle, native_libs, chr21, chr21_oracle_index, tmp_path_factory):
    """A pooled run of three cells in the style of tests/test_gpu_molecule_matrix.py's: every molecule is two different
    fragments of one transcript under one UMI of 8 bases, each written once or twice; genes of TWO transcripts, every
    tenth unnamed, so that the classes of a molecule's fragments often span genes.  With it the reference: cell, UMI
    and the oracle's class of every pooled unit."""
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('resolve_cli')
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
    rng = np.random.default_rng(711)
    mates, tags, cell = ([], []), [], []
    for c, n_molecules in enumerate((250, 150, 200)):
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


def test_resolve_molecules_on_pooled_files(cli_inputs, tmp_path):
    from seekmer_amd import infer
    from test_gpu_genes import _same_folder
    os.environ.pop('SKM_INFER_MANY_PER_SAMPLE', None)
    ours = _pooled_run(cli_inputs, tmp_path / 'with', '--resolve-molecules')
    without = _pooled_run(cli_inputs, tmp_path / 'without', '--count-molecules')
    only = _pooled_run(cli_inputs, tmp_path / 'only', '--matrix-only', '--resolve-molecules')
    top = sorted(CELLS + ['barcodes.json', 'barcodes.tsv', 'counts', 'samples.tsv'])
    assert sorted(f.name for f in ours.iterdir()) == top == sorted(f.name for f in without.iterdir())
    assert sorted(f.name for f in (without / 'counts').iterdir()) == COUNT_FILES
    assert sorted(f.name for f in (ours / 'counts').iterdir()) == sorted(COUNT_FILES + RESOLVED_FILES)
    for name in COUNT_FILES:
        assert (ours / 'counts' / name).read_bytes() == (without / 'counts' / name).read_bytes(), name
    for name in ('barcodes.json', 'barcodes.tsv', 'samples.tsv'):
        assert (ours / name).read_bytes() == (without / name).read_bytes(), name
    for name in CELLS:
        _same_folder(ours / name, without / name)
    # --matrix-only: the same counts/
    assert sorted(f.name for f in only.iterdir()) == ['barcodes.json', 'barcodes.tsv', 'counts', 'samples.tsv']
    assert sorted(f.name for f in (only / 'counts').iterdir()) == sorted(COUNT_FILES + RESOLVED_FILES)
    for name in COUNT_FILES + RESOLVED_FILES:
        assert (only / 'counts' / name).read_bytes() == (ours / 'counts' / name).read_bytes(), name
    # the reference, from the oracle's classes of the pooled reads and the genes in the order of genes.tsv
    genes = (ours / 'counts' / 'genes.tsv').read_bytes().splitlines()
    number = {name: g for g, name in enumerate(genes)}
    tx_gene = np.asarray([number[name] if name else -1 for name in cli_inputs['gene_name']], dtype=np.int32)
    cell, umi, tuples, stay = (cli_inputs[k] for k in ('cell', 'umi', 'tuples', 'stay'))
    indptr, indices, data, tally = mres.matrix(cell, umi, tuples, stay, tx_gene, 3)
    print('tally %r' % tally.tolist())
    lines = (ours / 'counts' / 'molecules.resolved.mtx').read_text().splitlines(keepends=True)
    assert lines == mref.mtx_lines(indptr, indices, data, len(genes), infer.RESOLVED_MATRIX_COMMENT)
    arrays = np.load(ours / 'counts' / 'molecules.resolved.npz')
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [3, len(genes)]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want), name
    rows = [line.split('\t') for line in (ours / 'counts' / 'molecules.resolved.tsv').read_text().splitlines()]
    names = [line.split('\t')[0] for line in (ours / 'samples.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == names == CELLS
    for s, row in enumerate(rows):
        resolved, rescued, multi, unnamed, collisions = tally[s].tolist()
        assert [int(v) for v in row[1:]] == [resolved + multi + unnamed + collisions, resolved, rescued, multi, unnamed,
                                             collisions, int(indptr[s + 1] - indptr[s])]
    # what the fixture is for: groups of two classes, rescued ones among them
    assert tally[:, 1].sum() >= 5 and tally[:, 0].sum() >= 100
