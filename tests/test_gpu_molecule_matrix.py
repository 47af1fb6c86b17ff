"""The molecule matrix on the device ("Molecule matrix") against tests/molecule_reference.py,
exactly: host triples through skm_gene_matrix_from_molecules (the sort, head and fill steps at their edges); a sample
set's resident state through SampleSet.gene_molecule_matrix, with the classes the reference counts by taken from the
oracle, never from the code under test; the same under umi_mismatches=1 (survivors of tests/umi_mismatch_reference.py);
and `infer-many --count-molecules` on pooled files.

The set's fixture uses synth.transcriptome(5, 600), not the (5, 30) of tests/test_gpu_umi.py: its non-triviality
check asks every sample for 100 entries with fewer molecules than units and 100 with as many, and 30 synthetic genes
give a sample 30 entries at the most."""
import ctypes
import os

import numpy as np
import pytest

import gene_matrix_reference as mref
import molecule_reference as mol
import umi_mismatch_reference as near_ref
import umi_reference as ref
from conftest import GOLDEN, make_product_index
from strand_reference import filter_result, reverse_complement

pytestmark = pytest.mark.gpu

READ_LEN = 75
UMI_ZERO, UMI_ONES = 0, 2 ** 32 - 1


# ---- triples ------------------------------------------------------------------------------------------------------
def _assert_triples(sample, gene, umi, n_samples, n_genes):
    from seekmer_amd import mapper
    indptr, indices, data, other = mapper.molecule_matrix(sample, gene, umi, n_samples, n_genes)
    mref.check_csr(indptr, indices, data, n_samples, n_genes)
    want = mref.csr(mol.from_triples(sample, gene, umi), n_samples)
    for got, expected, name in zip((indptr, indices, data), want, ('indptr', 'indices', 'data')):
        np.testing.assert_array_equal(got, expected, err_msg=name)
    assert other.shape == (n_samples, 2) and other.dtype == np.int64 and not other.any()
    return indptr, indices, data


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 3000])
def test_random_triples(native_libs, n):
    """few samples, genes and UMIs: every (sample, gene) run holds repeated UMIs"""
    rng = np.random.default_rng(n)
    sample, gene, umi = rng.integers(0, 5, n), rng.integers(0, 7, n), rng.integers(0, 9, n)
    indptr, indices, data = _assert_triples(sample, gene, umi, 6, 7)
    assert indptr[-1] == len(set(zip(sample.tolist(), gene.tolist()))) and indptr[5] == indptr[6]     # (sample 5 is empty)
    # the same triples in another order: identical arrays
    order = rng.permutation(n)
    again = _assert_triples(sample[order], gene[order], umi[order], 6, 7)
    for a, b in zip((indptr, indices, data), again):
        assert a.tobytes() == b.tobytes()


def test_named_triples(native_libs):
    n = 3000
    indptr, indices, data = _assert_triples(np.full(n, 2), np.full(n, 4), np.full(n, 77), 3, 5)      # all identical
    assert indptr.tolist() == [0, 0, 0, 1] and indices.tolist() == [4] and data.tolist() == [1]
    # one (sample, gene) run of 1000 distinct UMIs, crossing waves and blocks, between two other runs
    sample = np.concatenate([np.zeros(300), np.ones(1000), np.full(300, 2)]).astype(np.int64)
    gene = np.concatenate([np.full(300, 1), np.full(1000, 3), np.full(300, 0)]).astype(np.int64)
    umi = np.concatenate([np.arange(300) % 7, np.arange(1000) * 4099, np.arange(300) % 5])
    indptr, indices, data = _assert_triples(sample, gene, umi, 3, 4)
    assert data.tolist() == [7, 1000, 5]
    # two copies of one triple more than 1024 places apart, among distinct ones
    sample, gene, umi = np.zeros(2500, dtype=np.int64), np.arange(2500) % 3, np.arange(2500) + 10
    umi[[5, 2400]], gene[[5, 2400]] = 9, 1
    _, _, data = _assert_triples(sample, gene, umi, 1, 3)
    assert data.sum() == 2499
    # UMI 0 and 2^32 - 1, each twice, in one run and in neighbouring runs
    _, _, data = _assert_triples([0, 0, 0, 0, 1, 1], [2, 2, 2, 2, 2, 2], [UMI_ZERO, UMI_ONES, UMI_ZERO, UMI_ONES, UMI_ONES, UMI_ZERO], 2, 3)
    assert data.tolist() == [2, 2]
    # the last sample of 65 536 and the last gene of 70 001
    indptr, indices, data = _assert_triples([65535, 0, 65535, 65535], [70000, 70000, 70000, 0], [1, 1, 2, 1], 65536, 70001)
    assert indptr[-1] == 3 and indices.tolist() == [70000, 0, 70000] and data.tolist() == [1, 1, 2]


def test_bad_triples_give_no_handle(native_libs):
    hip = native_libs.hip()
    for sample, gene in (([0, 3], [0, 0]), ([0, -1], [0, 0]), ([0, 1], [0, 5]), ([0, 1], [-1, 0])):
        arrays = [np.asarray(sample, dtype=np.int32), np.asarray(gene, dtype=np.int32), np.asarray([1, 2], dtype=np.uint32)]
        handle = ctypes.c_void_p(1)
        code = hip.skm_gene_matrix_from_molecules(0, 2, native_libs.ptr(arrays[0], native_libs.c_i32p),
                                                  native_libs.ptr(arrays[1], native_libs.c_i32p),
                                                  native_libs.ptr(arrays[2], native_libs.c_u32p), 3, 5, ctypes.byref(handle))
        assert code == native_libs.SKM_ERR_ARG and handle.value is None
    assert hip.skm_gene_matrix_from_molecules(0, 0, None, None, None, 3, 5, None) == native_libs.SKM_ERR_ARG
    assert hip.skm_sample_set_molecule_matrix(None, 0, 0, None, None) == native_libs.SKM_ERR_ARG


# ---- the set, directly (helpers: copies of tests/test_gpu_umi.py's, which is free to change) -----------------------
N_SYNTH_GENES = 600
DISTINCT = 2500                   # distinct pairs a sample


@pytest.fixture(scope='module')
def transcriptome(oracle, native_libs):
    """(ids, pool, tx_offsets, oracle index, product index over the same arrays, tx_gene, n_genes).  tx_gene is the
    test's own: transcripts that some class of 40 000 oracle-mapped pairs holds together form a gene, numbered in the
    order of their first transcript; every tenth gene is unnamed; in every seventh the last transcript belongs to the
    next gene instead, so that classes across genes exist."""
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
    for g in range(3, len(roots) - 1, 7):
        tx_gene[np.flatnonzero(block == g)[-1]] = g + 1
    tx_gene[block % 10 == 0] = -1
    return ids, pool, tx_offsets, oindex, make_product_index(oindex, ids), tx_gene.astype(np.int32), len(roots)


def _pairs(pool, tx_offsets, seed, first, n):
    from seekmer_amd import synth
    raw = synth.reads(seed, pool, tx_offsets, first, n, READ_LEN, True)[0][:-1].tobytes()
    return [(raw[2 * u * READ_LEN:(2 * u + 1) * READ_LEN], raw[(2 * u + 1) * READ_LEN:(2 * u + 2) * READ_LEN]) for u in range(n)]


def _classes(oracle, oindex, pairs):
    return oracle.map_batch(oindex, *oracle.pack_reads([read for pair in pairs for read in pair]), len(pairs), True).tuples()


def _by_gene(classes, tx_gene):
    """{gene: {class: [places]}} of the classes inside one gene"""
    out = {}
    for i, t in enumerate(classes):
        if t and mol.kind(t, tx_gene) >= 0:
            out.setdefault(mol.kind(t, tx_gene), {}).setdefault(t, []).append(i)
    return out


def _sample_units(rng, distinct, classes, tx_gene, taken):
    """the filler of a sample: every distinct pair not in `taken` 1 to 4 times with one UMI.  In every second gene that
    has two classes, two pairs of different classes share their UMI: that gene's entry has fewer molecules than units."""
    umi_of = {}
    for k, (g, of) in enumerate(sorted(_by_gene(classes, tx_gene).items())):
        free = [[i for i in places if i not in taken] for _, places in sorted(of.items())]
        free = [places for places in free if places]
        if k % 2 == 0 and len(free) >= 2:
            umi_of[free[0][0]] = umi_of[free[1][0]] = int(rng.integers(1000, 2 ** 32 - 1))
    filler = []
    for i, pair in enumerate(distinct):
        if i not in taken:
            umi = umi_of.get(i, int(rng.integers(1000, 2 ** 32 - 1)))
            filler += [(pair, umi)] * int(rng.choice([1, 2, 3, 4], p=[.4, .3, .2, .1]))
    return [filler[i] for i in rng.permutation(len(filler))]


@pytest.fixture(scope='module')
def molecules(oracle, transcriptome):
    """Three samples of units (pair, UMI) and the oracle's classes.  Named, in samples 0 and 1 (by the oracle's classes):
      A  one UMI (11) on three units of three classes of one gene; the same pairs and UMI in sample 1
      B  one UMI (12) on a unit in each of two genes
      C  one UMI (13) on a unit of a class inside a gene and on a unit of an ambiguous class
      D  one UMI (14) on two units of two classes of one gene more than 1024 units apart (and a verbatim copy later)
      G  UMI 0 and UMI 2^32 - 1, each on two classes of one gene"""
    ids, pool, tx_offsets, oindex, index, tx_gene, n_genes = transcriptome
    rng = np.random.default_rng(99)
    samples, named = [], None
    for s in range(3):
        distinct = _pairs(pool, tx_offsets, 40 + s, s * 50000, DISTINCT)
        classes = _classes(oracle, oindex, distinct)
        if s == 0:
            genes = sorted(_by_gene(classes, tx_gene).items())
            three = [list(of.values()) for g, of in genes if len(of) >= 3]
            two = [list(of.values()) for g, of in genes if len(of) == 2]
            ambiguous = next(i for i, t in enumerate(classes) if t and mol.kind(t, tx_gene) == -2)
            a = [places[0] for places in three[0][:3]]
            b = [three[1][0][0], three[2][0][0]]
            c = [three[3][0][0], ambiguous]
            d = [two[0][0][0], two[0][1][0]]
            g0, g1 = [two[1][0][0], two[1][1][0]], [two[2][0][0], two[2][1][0]]
            taken = set(a + b + c + d + g0 + g1)
            named = dict(a=[distinct[i] for i in a], b=[distinct[i] for i in b], c=[distinct[i] for i in c],
                         d=[distinct[i] for i in d], g0=[distinct[i] for i in g0], g1=[distinct[i] for i in g1])
        filler = _sample_units(rng, distinct, classes, tx_gene, taken if s == 0 else set())
        if s == 2:
            samples.append(filler)
            continue
        p = named
        units = [(p['a'][0], 11), (p['d'][0], 14), (p['a'][1], 11), (p['b'][0], 12), (p['c'][0], 13)] + filler[:40]
        units += [(p['a'][2], 11), (p['b'][1], 12), (p['c'][1], 13), (p['g0'][0], UMI_ZERO), (p['g1'][0], UMI_ONES)] + filler[40:1300]
        units += [(p['d'][1], 14), (p['g0'][1], UMI_ZERO), (p['g1'][1], UMI_ONES), (p['g1'][1], UMI_ONES)] + filler[1300:] + [(p['d'][0], 14)]
        samples.append(units)
    reads = [read for units in samples for pair, _ in units for read in pair]
    sample = np.repeat(np.arange(3), [len(units) for units in samples]).astype(np.int32)
    umi = np.asarray([m for units in samples for _, m in units], dtype=np.uint32)
    bases, offsets = oracle.pack_reads(reads)
    mapped = oracle.map_batch(oindex, bases, offsets, sample.size, True)
    tuples = {None: mapped.tuples(), 'rf': filter_result(mapped, 'rf').tuples()}
    stay = {strand: ref.survivors(sample, umi, t) for strand, t in tuples.items()}
    want = {strand: mol.matrix(sample, umi, tuples[strand], stay[strand], tx_gene, 3) for strand in tuples}
    return dict(samples=samples, sample=sample, umi=umi, tuples=tuples, stay=stay, want=want, index=index, named=named,
                tx_gene=tx_gene, n_genes=n_genes)


def test_the_molecules_are_not_trivial(molecules):
    """the reference alone, before anything runs on a GPU: what the set is asked is in the input"""
    samples, sample, umi, tx_gene = (molecules[k] for k in ('samples', 'sample', 'umi', 'tx_gene'))
    tuples, stay = molecules['tuples'][None], molecules['stay'][None]
    counted, other = mol.entries(sample, umi, tuples, stay, tx_gene)
    units = mol.unit_entries(sample, tuples, stay, tx_gene)
    assert sorted(counted) == sorted(units)
    for s in range(3):
        below = sum(1 for key in counted if key[0] == s and counted[key] < units[key])
        equal = sum(1 for key in counted if key[0] == s and counted[key] == units[key])
        print('sample %d: %d entries with fewer molecules than units, %d with as many' % (s, below, equal))
        assert below >= 100 and equal >= 100, (s, below, equal)
        assert other[s][0] >= 100 and other[s][1] >= 10, 'ambiguous and unnamed classes'
    assert (~stay).sum() > 1000, 'collapse removes units'
    p = molecules['named']
    for s in (0, 1):
        first, base = samples[s], int(np.flatnonzero(sample == s)[0])
        at = lambda pair, m: base + next(u for u, item in enumerate(first) if item == (pair, m))
        klass = lambda pair, m: tuples[at(pair, m)]
        gene = lambda pair, m: mol.kind(klass(pair, m), tx_gene)
        a = [(pair, 11) for pair in p['a']]
        assert len({klass(*x) for x in a}) == 3 and len({gene(*x) for x in a}) == 1 and gene(*a[0]) >= 0 and all(stay[at(*x)] for x in a)
        others = [u for u in np.flatnonzero((sample == s) & stay) if tuples[u] and mol.kind(tuples[u], tx_gene) == gene(*a[0]) and umi[u] != 11]
        assert counted[(s, gene(*a[0]))] == 1 + len({int(umi[u]) for u in others}) and units[(s, gene(*a[0]))] == 3 + len(others)
        b = [(pair, 12) for pair in p['b']]
        assert gene(*b[0]) >= 0 and gene(*b[1]) >= 0 and gene(*b[0]) != gene(*b[1]) and all(stay[at(*x)] for x in b)
        c = [(pair, 13) for pair in p['c']]
        assert gene(*c[0]) >= 0 and gene(*c[1]) == -2 and all(stay[at(*x)] for x in c)
        d = [(pair, 14) for pair in p['d']]
        assert gene(*d[0]) == gene(*d[1]) >= 0 and klass(*d[0]) != klass(*d[1]) and at(*d[1]) - at(*d[0]) > 1024
        copies = [u for u, item in enumerate(first) if item == d[0]]
        assert len(copies) == 2 and stay[base + copies[0]] and not stay[base + copies[1]] and copies[1] - copies[0] > 1024
        for pairs, m in ((p['g0'], UMI_ZERO), (p['g1'], UMI_ONES)):
            assert gene(pairs[0], m) == gene(pairs[1], m) >= 0 and klass(pairs[0], m) != klass(pairs[1], m)
    # under the rf library other classes, and still entries of both kinds
    rf_counted, _ = mol.entries(sample, umi, molecules['tuples']['rf'], molecules['stay']['rf'], tx_gene)
    rf_units = mol.unit_entries(sample, molecules['tuples']['rf'], molecules['stay']['rf'], tx_gene)
    assert any(a != b for a, b in zip(tuples, molecules['tuples']['rf']))
    assert sum(rf_counted[key] < rf_units[key] for key in rf_counted) >= 10 and sum(rf_counted[key] == rf_units[key] for key in rf_counted) >= 10


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


def _assert_set(fixture, strand=None, cuts=(), **how):
    from seekmer_amd import mapper
    sample_set = mapper.SampleSet(fixture['index'], True, strand=strand, per_sample_lengths=True, umi_bases=16, **how)
    for s in [1, 0, 2] if len(fixture['samples']) == 3 else range(len(fixture['samples'])):      # (the samples in any order)
        units = fixture['samples'][s]
        _add_sample(sample_set, s, units, umis=[m for _, m in units], cuts=cuts if s == 0 else ())
    n_samples, n_genes = len(fixture['samples']), fixture['n_genes']
    got = sample_set.gene_molecule_matrix(fixture['tx_gene'], n_genes)
    mref.check_csr(*got[:3], n_samples, n_genes)
    unit_matrix = sample_set.gene_count_matrix(fixture['tx_gene'], n_genes)
    print('entries %d, molecules %d, units inside one gene %d' % (got[2].size, got[2].sum(), unit_matrix[2].sum()))
    for name, a, b in zip(('indptr', 'indices', 'data', 'other'), got, fixture['want'][strand]):
        np.testing.assert_array_equal(a, b, err_msg=name)
    for k in (0, 1, 3):
        np.testing.assert_array_equal(got[k], unit_matrix[k])
    assert (got[2] >= 1).all() and (got[2] <= unit_matrix[2]).all()
    again = sample_set.gene_molecule_matrix(fixture['tx_gene'], n_genes)              # (the set is read, not used up)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    return got


def _hook(monkeypatch, hook):
    for name in ('SKM_SAMPLE_SET_MAX_UNITS', 'SKM_TEST_UMI_SLOTS', 'SKM_TEST_MAP_BLOCKS'):
        monkeypatch.delenv(name, raising=False)
    for pair in hook or ():
        monkeypatch.setenv(*pair.split('='))


@pytest.mark.parametrize('hook', [None, ('SKM_SAMPLE_SET_MAX_UNITS=500',), ('SKM_TEST_UMI_SLOTS=2',), ('SKM_TEST_MAP_BLOCKS=1',)])
def test_the_molecule_matrix_of_a_set_is_the_reference(molecules, monkeypatch, hook):
    _hook(monkeypatch, hook)
    _assert_set(molecules, cuts=(2, 700) if hook else ())           # (a cut between the units of A, and between those of D)


def test_molecules_follow_the_strand_filter(molecules, monkeypatch):
    _hook(monkeypatch, ('SKM_SAMPLE_SET_MAX_UNITS=500',))
    _assert_set(molecules, strand='rf')


def test_a_set_without_umis_or_without_units(molecules, native_libs):
    from seekmer_amd import mapper
    plain = mapper.SampleSet(molecules['index'], True, per_sample_lengths=True)
    _add_sample(plain, 0, molecules['samples'][2][:50])
    with pytest.raises(native_libs.NativeError) as error:
        plain.gene_molecule_matrix(molecules['tx_gene'], molecules['n_genes'])
    assert error.value.code == native_libs.SKM_ERR_STATE
    handle = ctypes.c_void_p(1)
    tx_gene = molecules['tx_gene']
    assert native_libs.hip().skm_sample_set_molecule_matrix(plain._handle, tx_gene.size, molecules['n_genes'],
                                                            native_libs.ptr(tx_gene, native_libs.c_i32p),
                                                            ctypes.byref(handle)) == native_libs.SKM_ERR_STATE
    assert handle.value is None
    empty = mapper.SampleSet(molecules['index'], True, per_sample_lengths=True, umi_bases=16)
    indptr, indices, data, other = empty.gene_molecule_matrix(tx_gene, molecules['n_genes'])
    assert indptr.tolist() == [0] and indices.size == 0 and data.size == 0 and other.shape == (0, 2)
    with pytest.raises(ValueError):           # a gene map that does not cover the index's transcripts
        empty.gene_molecule_matrix(tx_gene[:-1], molecules['n_genes'])


# ---- umi_mismatches = 1 -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def near(oracle, transcriptome, molecules):
    """One sample.  X: a molecule (class x1, UMI u) whose first unit follows a unit of (x1, u ^ 1) and is removed for
    it, u nowhere else in the gene: not counted.  Y: the same with UMI v, which a surviving unit of another class of
    the gene carries too: counted once.  Then filler, so that launches and growth of the set follow."""
    ids, pool, tx_offsets, oindex, index, tx_gene, n_genes = transcriptome
    p = molecules['named']
    x1, x2 = p['d']
    y1, y2 = p['g0']
    u, v = 0x12345678, 0x0BADCAFE
    units = [(x1, u ^ 1), (y1, v ^ (2 << 10)), (x1, u), (y1, v), (y2, v), (x1, u), (x2, 5)]
    units += [unit for unit in molecules['samples'][2] if unit[0] not in (x1, x2, y1, y2)][:3000]
    sample = np.zeros(len(units), dtype=np.int32)
    umi = np.asarray([m for _, m in units], dtype=np.uint32)
    tuples = oracle.map_batch(oindex, *oracle.pack_reads([read for pair, _ in units for read in pair]), len(units), True).tuples()
    stay = near_ref.survivors(sample, umi, tuples, 16, 1)
    exact = ref.survivors(sample, umi, tuples)
    return dict(samples=[units], sample=sample, umi=umi, tuples=tuples, stay={None: stay}, exact=exact, index=index,
                tx_gene=tx_gene, n_genes=n_genes, want={None: mol.matrix(sample, umi, tuples, stay, tx_gene, 1)}, u=u, v=v)


def test_the_neighbours_are_not_trivial(near):
    """the reference alone"""
    tuples, stay, exact, umi, tx_gene = near['tuples'], near['stay'][None], near['exact'], near['umi'], near['tx_gene']
    assert stay[:7].tolist() == [True, True, False, False, True, False, True] and exact[:7].tolist() == [True, True, True, True, True, False, True]
    gx, gy = mol.kind(tuples[0], tx_gene), mol.kind(tuples[1], tx_gene)
    assert gx >= 0 and gy >= 0 and gx != gy and tuples[0] == tuples[2] != tuples[6] and tuples[1] == tuples[3] != tuples[4]
    assert mol.kind(tuples[6], tx_gene) == gx and mol.kind(tuples[4], tx_gene) == gy
    in_gene = lambda g, mask: {int(umi[k]) for k in np.flatnonzero(mask) if tuples[k] and mol.kind(tuples[k], tx_gene) == g}
    assert near['u'] not in in_gene(gx, stay) and near['u'] in in_gene(gx, exact)      # X: gone, and a molecule of the exact rule
    assert near['v'] in in_gene(gy, stay)                                                # Y: counted, once
    counted, _ = mol.entries(near['sample'], umi, tuples, stay, tx_gene)
    counted_exact, _ = mol.entries(near['sample'], umi, tuples, exact, tx_gene)
    assert counted[(0, gx)] == counted_exact[(0, gx)] - 1 and counted[(0, gy)] == counted_exact[(0, gy)]
    assert (exact & ~stay).sum() >= 2


@pytest.mark.parametrize('hook', [None, ('SKM_TEST_UMI_SLOTS=2', 'SKM_SAMPLE_SET_MAX_UNITS=500')])
def test_a_molecule_removed_for_a_neighbour_is_not_counted(near, monkeypatch, hook):
    """2 slots and launches of 500 units: the set is rehashed after the launch that marked X and Y's first molecules"""
    _hook(monkeypatch, hook)
    _assert_set(near, umi_mismatches=1)


# ---- command line -------------------------------------------------------------------------------------------------
BARCODES = [b'ACGTACGTAC', b'TTGCAAGGCT', b'GGATCCTTAG']
CELLS = ['cell0', 'cell1', 'cell2']
COUNT_FILES = ['cells.tsv', 'genes.tsv', 'matrix.mtx', 'matrix.npz']
MOLECULE_FILES = ['molecules.mtx', 'molecules.npz']


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
    """A pooled run of three cells in the style of tests/test_gpu_gene_matrix.py's: every molecule is two different
    fragments of one transcript under one UMI of 8 bases, each written once or twice; genes of four transcripts, every
    tenth unnamed.  With it the reference: cell, UMI and the oracle's class of every pooled unit."""
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('molecule_cli')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    index_path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(index_path)]) == 0
    ids = [id_.split()[0].split(b'.')[0] for id_ in chr21[0]]
    map_path = folder / 'genes.tsv'
    gene_name = [b'G%05d' % (t // 4) if (t // 4) % 10 else b'' for t in range(len(ids))]
    with open(map_path, 'wb') as f:
        for id_, name in zip(ids, gene_name):
            if name:
                f.write(id_ + b'\t' + name + b'\n')
    (folder / 'whitelist.tsv').write_bytes(b''.join(b'%s\t%s\n' % (code, name.encode()) for code, name in zip(BARCODES, CELLS)))
    rng = np.random.default_rng(709)
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


@pytest.fixture(scope='module')
def runs(cli_inputs, tmp_path_factory):
    os.environ.pop('SKM_INFER_MANY_PER_SAMPLE', None)
    folder = tmp_path_factory.mktemp('molecule_runs')
    return (_pooled_run(cli_inputs, folder / 'with', '--count-matrix', '--count-molecules'),
            _pooled_run(cli_inputs, folder / 'without', '--count-matrix'))


def test_count_molecules_writes_the_reference_and_changes_no_other_file(cli_inputs, runs):
    from seekmer_amd import infer
    from test_gpu_genes import _same_folder
    ours, without = runs
    top = sorted(CELLS + ['barcodes.json', 'barcodes.tsv', 'counts', 'samples.tsv'])
    assert sorted(f.name for f in ours.iterdir()) == top == sorted(f.name for f in without.iterdir())
    assert sorted(f.name for f in (without / 'counts').iterdir()) == COUNT_FILES
    assert sorted(f.name for f in (ours / 'counts').iterdir()) == sorted(COUNT_FILES + MOLECULE_FILES)
    for name in COUNT_FILES:
        assert (ours / 'counts' / name).read_bytes() == (without / 'counts' / name).read_bytes(), name
    for name in ('barcodes.json', 'barcodes.tsv', 'samples.tsv'):
        assert (ours / name).read_bytes() == (without / name).read_bytes(), name
    for name in CELLS:
        _same_folder(ours / name, without / name)
    # the reference, from the oracle's classes of the pooled reads and the genes in the order of genes.tsv
    genes = (ours / 'counts' / 'genes.tsv').read_bytes().splitlines()
    number = {name: g for g, name in enumerate(genes)}
    tx_gene = np.asarray([number[name] if name else -1 for name in cli_inputs['gene_name']], dtype=np.int32)
    cell, umi, tuples, stay = (cli_inputs[k] for k in ('cell', 'umi', 'tuples', 'stay'))
    indptr, indices, data, other = mol.matrix(cell, umi, tuples, stay, tx_gene, 3)
    lines = (ours / 'counts' / 'molecules.mtx').read_text().splitlines(keepends=True)
    assert lines == mref.mtx_lines(indptr, indices, data, len(genes), infer.MOLECULE_MATRIX_COMMENT)
    arrays = np.load(ours / 'counts' / 'molecules.npz')
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [3, len(genes)]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want), name
    # the pattern of matrix.mtx, and fewer counts in total: fragments of one molecule fell into different classes
    _, _, u_indptr, u_indices, u_data = mref.parse_mtx((ours / 'counts' / 'matrix.mtx').read_text().splitlines(keepends=True))
    assert np.array_equal(u_indptr, indptr) and np.array_equal(u_indices, indices)
    units = mref.csr(mol.unit_entries(cell, tuples, stay, tx_gene), 3)[2]
    assert np.array_equal(u_data, units) and (data <= u_data).all() and (data >= 1).all()
    print('units inside one gene %d, molecules %d' % (u_data.sum(), data.sum()))
    assert data.sum() < u_data.sum() and (data < u_data).sum() >= 10 and (data == u_data).sum() >= 50
    cells = [line.split('\t') for line in (ours / 'counts' / 'cells.tsv').read_text().splitlines()]
    assert [[int(row[4]), int(row[5])] for row in cells] == other.tolist()


def test_count_molecules_with_matrix_only(cli_inputs, runs, tmp_path):
    ours, _ = runs
    only = _pooled_run(cli_inputs, tmp_path / 'only', '--matrix-only', '--count-molecules')
    assert sorted(f.name for f in only.iterdir()) == ['barcodes.json', 'barcodes.tsv', 'counts', 'samples.tsv']
    assert sorted(f.name for f in (only / 'counts').iterdir()) == sorted(COUNT_FILES + MOLECULE_FILES)
    for name in COUNT_FILES + MOLECULE_FILES:
        assert (only / 'counts' / name).read_bytes() == (ours / 'counts' / name).read_bytes(), name
    for name in ('barcodes.json', 'barcodes.tsv', 'samples.tsv'):
        assert (only / name).read_bytes() == (ours / name).read_bytes(), name


def test_count_molecules_refusals(cli_inputs, tmp_path):
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    mate1, mate2, barcode_file = cli_inputs['files']
    index, genes = str(cli_inputs['index']), ['--gene-map', str(cli_inputs['map'])]
    pooled = ['--barcodes', cli_inputs['whitelist'], '--barcode-file', barcode_file]
    for n, options in enumerate((pooled, [])):                        # pooled without --umi-length; not pooled
        out = tmp_path / ('refused%d' % n)
        with pytest.raises(ValueError) as refused:
            cli.main(['infer-many', index, str(out), mate1, mate2, *options, *genes, '--count-molecules'])
        assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS and not out.exists()
    with pytest.raises(SystemExit):
        cli.main(['infer', index, str(tmp_path / 'infer'), mate1, mate2, '--count-molecules'])
    assert not (tmp_path / 'infer').exists()
