"""The count matrix on the device: hand-made class tables through skm_gene_matrix_from_classes, exact against
tests/gene_matrix_reference.py; a sample set's resident table against its own dense rows; and the command line
(`infer-many --count-matrix`, `--matrix-only`, plain samples and one pooled run)."""
import ctypes
import os

import numpy as np
import pytest

import gene_matrix_reference as mref
import gene_reference as ref
from conftest import GOLDEN, make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------- hand-made class tables
def _native_matrix(native_libs, offsets, targets, counts, sample, n_samples, tx_gene, n_genes, n_tx=None):
    """(code, (indptr, indices, data, other) or None) of skm_gene_matrix_from_classes; the handle is read and destroyed"""
    p, i32, i64 = native_libs.ptr, native_libs.c_i32p, native_libs.c_i64p
    hip = native_libs.hip()
    handle = ctypes.c_void_p(0xdead)                              # (a failed call leaves NULL here)
    code = hip.skm_gene_matrix_from_classes(
        0, counts.size, p(offsets, i64), p(targets, i32) if targets.size else None, p(counts, i64) if counts.size else None,
        p(sample, i32) if sample is not None else None, n_samples, tx_gene.size if n_tx is None else n_tx, n_genes,
        p(tx_gene, i32), ctypes.byref(handle))
    if code != native_libs.SKM_OK:
        assert not handle.value
        return code, None
    shape = [ctypes.c_int64(-1) for _ in range(3)]
    assert hip.skm_gene_matrix_shape(handle, *[ctypes.byref(word) for word in shape]) == native_libs.SKM_OK
    assert (shape[0].value, shape[1].value) == (n_samples, n_genes)
    nnz = shape[2].value
    indptr = np.full(n_samples + 1, -7, dtype=np.int64)
    indices = np.full(nnz + 1, -7, dtype=np.int32)
    data = np.full(nnz + 1, -7, dtype=np.int64)
    other = np.full((n_samples + 1, 2), -7, dtype=np.int64)
    assert hip.skm_gene_matrix_read(handle, p(indptr, i64), None, None, None) == native_libs.SKM_OK     # (any one alone)
    assert hip.skm_gene_matrix_read(handle, p(indptr, i64), p(indices, i32), p(data, i64), p(other, i64)) == native_libs.SKM_OK
    assert hip.skm_gene_matrix_destroy(handle) == native_libs.SKM_OK
    assert indices[nnz] == -7 and data[nnz] == -7 and (other[n_samples] == -7).all()                   # (nothing past the end)
    return code, (indptr, indices[:nnz], data[:nnz], other[:n_samples])


def _table(classes, counts, samples):
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int64)
    targets = np.concatenate([np.asarray(c, dtype=np.int32) for c in classes] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return offsets, targets, np.asarray(counts, dtype=np.int64), np.asarray(samples, dtype=np.int32)


def _assert_matrix(native_libs, table, n_samples, tx_gene, n_genes, with_sample=True):
    offsets, targets, counts, sample = table
    want = mref.matrix(offsets, targets, counts, tx_gene, sample if with_sample else None, n_samples)
    code, got = _native_matrix(native_libs, offsets, targets, counts, sample if with_sample else None, n_samples, tx_gene, n_genes)
    assert code == native_libs.SKM_OK
    mref.check_csr(*got[:3], n_samples, n_genes)
    for name, a, b in zip(('indptr', 'indices', 'data', 'other'), got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)
    return got


WIDE_GENES = 70001                    # gene numbers above 2^16
# transcripts [0, 150): gene 0; [150, 300): the last gene; [300, 310): gene 5; [310, 400): unnamed
WIDE_TX_GENE = np.concatenate([np.zeros(150), np.full(150, WIDE_GENES - 1), np.full(10, 5), np.full(90, -1)]).astype(np.int32)
EDGE_LENGTHS = (1, 8, 9, 72, 73, 137)     # around GENE_HEAD = 8 and the 64-wide walk of the rest: 8 + 64, 8 + 2 x 64 + 1


def _edge_table():
    """n_samples = 6, samples 0, 3 and 5 own no class.  Returns (table, what the test states about it)"""
    rng = np.random.default_rng(12)
    classes, counts, samples = [], [], []

    def add(ids, count, sample):
        classes.append(list(ids)), counts.append(count), samples.append(sample)
    for n in EDGE_LENGTHS:
        for sample, first in ((1, 0), (2, 150)):                 # all in gene 0 / all in the last gene
            plain = first + rng.permutation(150)[:n]
            add(plain, int(rng.integers(1, 1000)), sample)
            odd = plain.copy()
            odd[-1] = (150 - first) + int(rng.integers(150))      # only its last id in the other gene
            add(odd, int(rng.integers(1, 1000)), sample)
    add([], 11, 1)                                                # a class with no ids: ambiguous
    add(310 + rng.permutation(90)[:5], 13, 1)                     # all unnamed
    add(310 + rng.permutation(90)[:80], 17, 4)                    # all unnamed, long
    add([3, 320], 19, 2)                                          # named and unnamed
    add(list(range(20)) + [399], 23, 4)                           # named and unnamed, past the head
    add([300, 301, 302], 0, 4)                                    # inside gene 5 with count 0: no entry
    add([303], 29, 2), add([304, 305], 31, 2)                     # two classes of one sample in one gene: one entry
    add([306], 37, 4)                                             # ... and gene 5 in another sample too: its own entry
    add([1], 1 << 40, 4), add([2, 3], 1 << 40, 4), add([4], (1 << 40) + 5, 4)     # sums that need 64 bits
    order = rng.permutation(len(classes))
    return _table([classes[k] for k in order], [counts[k] for k in order], [samples[k] for k in order])


def test_edges_of_the_walk_and_of_the_rows(native_libs):
    table = _edge_table()
    assert sorted(set(np.diff(table[0]).tolist()) & set(EDGE_LENGTHS)) == list(EDGE_LENGTHS)
    indptr, indices, data, other = _assert_matrix(native_libs, table, 6, WIDE_TX_GENE, WIDE_GENES)
    # what the table was made to show, stated on the result itself
    # empty rows first, in the middle and last; a class of one id "with its last id in the other gene" lies in that gene
    assert np.diff(indptr).tolist() == [0, 2, 3, 0, 2, 0]
    assert indices.tolist() == [0, WIDE_GENES - 1, 0, 5, WIDE_GENES - 1, 0, 5]
    rows = {s: dict(zip(indices[indptr[s]:indptr[s + 1]].tolist(), data[indptr[s]:indptr[s + 1]].tolist())) for s in range(6)}
    assert rows[2][5] == 29 + 31 and 5 not in rows[1]
    assert rows[4] == {0: 3 * (1 << 40) + 5, 5: 37}                                # (the count-0 class adds nothing to 37)
    assert other[1].tolist()[1] == 13 and other[4, 1] == 17 and other[2, 0] >= 19 and other[1, 0] >= 11
    assert not other[[0, 3, 5]].any()
    # the same classes as ONE sample without class_sample
    one = (table[0], table[1], table[2], np.zeros(table[2].size, dtype=np.int32))
    _assert_matrix(native_libs, one, 1, WIDE_TX_GENE, WIDE_GENES, with_sample=False)


def test_the_last_sample_of_65536_and_the_last_gene_of_70001(native_libs):
    n_samples = 65536
    classes = [[0], [150, 151], [149], [299], [0, 150], [310], [5, 6, 7]]
    samples = [65535, 65535, 0, 0, 65535, 65535, 32768]
    counts = [3, 4, 5, 6, 7, 8, 9]
    indptr, indices, data, other = _assert_matrix(native_libs, _table(classes, counts, samples), n_samples, WIDE_TX_GENE, WIDE_GENES)
    assert indptr[-1] == 5 and indptr[1] == 2 and indptr[32768] == 2 and indptr[32769] == 3 and indptr[65535] == 3
    assert indices.tolist() == [0, WIDE_GENES - 1, 0, 0, WIDE_GENES - 1] and data.tolist() == [5, 6, 9, 3, 4]
    assert other[65535].tolist() == [7, 8] and other[:65535].sum() == 0


def test_a_run_across_waves_and_blocks(native_libs):
    """700 classes of one (sample, gene), among others: after the sort the run covers eleven waves and three blocks"""
    rng = np.random.default_rng(13)
    classes = [[300 + int(rng.integers(10))] for _ in range(700)] + [[int(rng.integers(150))] for _ in range(300)] \
        + [[150 + int(rng.integers(150))] for _ in range(200)]
    counts = rng.integers(1, 1 << 40, len(classes)).tolist()
    samples = [2] * 700 + rng.integers(0, 4, 500).tolist()
    order = rng.permutation(len(classes))
    table = _table([classes[k] for k in order], [counts[k] for k in order], [samples[k] for k in order])
    indptr, indices, data, _ = _assert_matrix(native_libs, table, 4, WIDE_TX_GENE, WIDE_GENES)
    row = dict(zip(indices[indptr[2]:indptr[3]].tolist(), data[indptr[2]:indptr[3]].tolist()))
    assert row[5] == sum(counts[:700]) > 1 << 45


def test_an_empty_table_and_a_table_without_a_class_inside_one_gene(native_libs):
    none = _table([], [], [])
    for n_samples in (0, 1, 3):
        indptr, indices, data, other = _assert_matrix(native_libs, none, n_samples, WIDE_TX_GENE, WIDE_GENES)
        assert not indptr.any() and indices.size == 0 and other.shape == (n_samples, 2) and not other.any()
    classes = [[0, 150], [310, 311], [], [5, 320], [300, 301]]
    indptr, indices, data, other = _assert_matrix(native_libs, _table(classes, [1, 2, 3, 4, 0], [0, 1, 1, 2, 2]), 3,
                                                  WIDE_TX_GENE, WIDE_GENES)
    assert not indptr.any() and indices.size == 0 and data.size == 0                 # nnz = 0
    assert other.tolist() == [[1, 0], [3, 2], [4, 0]]


def test_a_random_table(native_libs):
    rng = np.random.default_rng(14)
    n_classes, n_samples, n_genes, n_tx = 5000, 37, 50, 900
    tx_gene = np.sort(np.where(rng.uniform(0, 1, n_tx) < 0.1, -1, rng.integers(0, n_genes, n_tx))).astype(np.int32)
    lengths = rng.choice([0, 1, 2, 3, 7, 8, 9, 20, 70, 100], n_classes, p=[.02, .3, .2, .2, .1, .05, .05, .04, .02, .02])
    classes = []
    for n in lengths:
        near, spread = int(rng.integers(n_tx)), int(rng.choice([1, 6, 60]))
        classes.append(np.clip(near + rng.integers(0, spread, n), 0, n_tx - 1))
    counts = rng.integers(0, 500, n_classes) * (rng.uniform(0, 1, n_classes) > 0.05)
    table = _table(classes, counts, rng.integers(0, n_samples, n_classes))
    indptr, indices, data, other = _assert_matrix(native_libs, table, n_samples, tx_gene, n_genes)
    want_unique, want_other = ref.unique_counts(*table[:3], tx_gene, n_genes, table[3], n_samples)
    np.testing.assert_array_equal(mref.dense(indptr, indices, data, n_genes), want_unique)
    assert 500 < indptr[-1] < n_samples * n_genes and other.sum(axis=0).min() > 0 and (np.diff(indptr) > 0).all()


def test_bad_tables_give_no_handle(native_libs):
    table = _edge_table()
    offsets, targets, counts, sample = table
    err = native_libs.SKM_ERR_ARG
    short = int(targets.max())                                    # a target not below n_tx
    assert _native_matrix(native_libs, offsets, targets, counts, sample, 6, WIDE_TX_GENE[:short].copy(), WIDE_GENES, n_tx=short) == (err, None)
    assert _native_matrix(native_libs, offsets, targets, counts, sample, 4, WIDE_TX_GENE, WIDE_GENES) == (err, None)    # sample 4 of 4
    assert _native_matrix(native_libs, offsets, targets, counts, sample, 6, WIDE_TX_GENE, WIDE_GENES - 1) == (err, None)  # gene n_genes
    wrong = WIDE_TX_GENE.copy()
    wrong[0] = -2
    assert _native_matrix(native_libs, offsets, targets, counts, sample, 6, wrong, WIDE_GENES) == (err, None)
    negative = counts.copy()
    negative[3] = -1
    assert _native_matrix(native_libs, offsets, targets, negative, sample, 6, WIDE_TX_GENE, WIDE_GENES) == (err, None)
    assert _native_matrix(native_libs, offsets, targets, counts, None, 6, WIDE_TX_GENE, WIDE_GENES) == (err, None)      # no class_sample
    # more samples than a key can number: refused with a message, never wrapped
    assert _native_matrix(native_libs, offsets, targets, counts, sample, (1 << 31) - 1, WIDE_TX_GENE, WIDE_GENES) == (err, None)
    assert b'samples' in native_libs.hip().skm_last_error()
    # NULL handles
    assert native_libs.hip().skm_gene_matrix_shape(None, None, None, None) == err
    assert native_libs.hip().skm_gene_matrix_read(None, None, None, None, None) == err
    assert native_libs.hip().skm_gene_matrix_destroy(None) == native_libs.SKM_OK


# ------------------------------------------------------------------------------------ chr21: the inputs
# (the helpers of tests/test_gpu_genes.py)
def _fragments(seqs, rng, n_units, read_len=60):
    """[mate 1, mate 2] of n_units chr21 fragments, either mate first"""
    long_tx = [s.upper() for s in seqs if len(s) > 450 and set(s.upper()) <= set(b'ACGT')]
    units = []
    for _ in range(n_units):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(150, 401))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        mates = [bytes(f[:read_len]), bytes(reverse_complement(f[-read_len:]))]
        if rng.integers(2):
            mates.reverse()
        units.append(mates)
    return units


def _reads(units):
    return [read for mates in units for read in mates]


def _batch(oracle, reads):
    from seekmer_amd import common
    bases, offsets = oracle.pack_reads(reads) if reads else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    return common.ReadBatch(len(reads) // 2, bases, offsets, True)


def _chr21_genes(n_tx):
    """gene = t // 4, the genes with gene % 10 == 0 unnamed"""
    gene = np.arange(n_tx) // 4
    names = np.asarray([b'' if g % 10 == 0 else b'G%05d' % g for g in gene])
    return ref.gene_map_from_ids(names)


@pytest.fixture(scope='module')
def chr21_index(chr21, chr21_oracle_index):
    return make_product_index(chr21_oracle_index, chr21[0])


@pytest.fixture(scope='module')
def set_samples(chr21):
    """samples of 40, 41 and 600 units, one without units, one whose units all fail to align"""
    rng = np.random.default_rng(707)
    samples = [_reads(_fragments(chr21[1], rng, n)) for n in (40, 41, 600)]
    samples.append([])
    samples.append([bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 60)) for _ in range(100)])
    return samples


# -------------------------------------------------------------------------------------------- sample set
@pytest.mark.parametrize('packed', [False, True], ids=['text', 'packed'])
def test_sample_set_matrix_is_its_dense_rows(oracle, native_libs, chr21_index, set_samples, monkeypatch, packed):
    from seekmer_amd import common, infer, mapper
    gene_ids, tx_gene = _chr21_genes(chr21_index.transcripts.size)
    n_genes = gene_ids.size
    monkeypatch.setenv('SKM_SAMPLE_SET_MAX_UNITS', '256')
    monkeypatch.delenv('SKM_GENE_GROUP', raising=False)
    sample_set = mapper.SampleSet(chr21_index, True)
    indptr, indices, data, other = sample_set.gene_count_matrix(tx_gene, n_genes)
    assert indptr.tolist() == [0] and indices.size == 0 and data.size == 0 and other.shape == (0, 2)     # no samples yet
    for i, reads in enumerate(set_samples):
        if packed and reads:
            pieces = [common.PackedReads.from_ascii(*oracle.pack_reads(reads[mate::2]), stream=mate) for mate in range(2)]
            sample_set.add_packed(i, 0, *pieces)
        else:
            sample_set.add_batch(i, 0, _batch(oracle, reads))
    indptr, indices, data, other = sample_set.gene_count_matrix(tx_gene, n_genes)
    mref.check_csr(indptr, indices, data, 5, n_genes)
    unique, dense_other = sample_set.gene_unique_counts(tx_gene, n_genes)
    np.testing.assert_array_equal(mref.dense(indptr, indices, data, n_genes), unique)
    np.testing.assert_array_equal(other, dense_other)
    assert other.dtype == np.int64 and other.shape == (5, 2)
    assert (np.diff(indptr)[:3] > 0).all() and not np.diff(indptr)[3:].any() and indptr[-1] == np.count_nonzero(unique)
    sizes = sample_set.sizes()
    inside = np.asarray([data[indptr[s]:indptr[s + 1]].sum() for s in range(5)])
    np.testing.assert_array_equal(inside + other.sum(axis=1), sizes[:, 3] - sizes[:, 2])
    # the same rows from the samples' summaries, stacked and passed through the device once
    stacked = infer.gene_count_matrix(sample_set.summarize(), tx_gene, n_genes)
    for got, want in zip(stacked, (indptr, indices, data, other)):
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    # a gene map that does not cover the index's transcripts is refused, not read past
    with pytest.raises(ValueError):
        sample_set.gene_count_matrix(tx_gene[:-1], n_genes)


# ------------------------------------------------------------------------------------------ command line
def _write_fastq(path, reads):
    with open(path, 'wb') as f:
        for u, read in enumerate(reads):
            f.write(b'@u%d\n' % u + read + b'\n+\n' + b'I' * len(read) + b'\n')


@pytest.fixture(scope='module')
def cli_inputs(native_libs, chr21, tmp_path_factory):
    """(index file without genes, gene-map file, {name: [mate 1 file, mate 2 file]}, the pooled run's files)"""
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('gene_matrix_cli')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    index_path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(index_path)]) == 0
    ids = [id_.split()[0].split(b'.')[0] for id_ in chr21[0]]
    map_path = folder / 'genes.tsv'
    with open(map_path, 'wb') as f:
        for t, id_ in enumerate(ids):
            if (t // 4) % 10:
                f.write(id_ + b'\tG%05d\n' % (t // 4))
    rng = np.random.default_rng(708)
    groups = {}
    for name, n_units in (('small', 300), ('tiny', 45), ('mid', 120)):
        reads = _reads(_fragments(chr21[1], rng, n_units))
        files = [folder / (name + '_1.fastq'), folder / (name + '_2.fastq')]
        for mate in range(2):
            _write_fastq(files[mate], reads[mate::2])
        groups[name] = [str(f) for f in files]
    # one pooled run: three cells of a few hundred units, every unit written once or twice with one UMI of 8 bases
    barcodes = [b'ACGTACGTAC', b'TTGCAAGGCT', b'GGATCCTTAG']
    (folder / 'whitelist.tsv').write_bytes(b''.join(b'%s\tcell%d\n' % (code, c) for c, code in enumerate(barcodes)))
    mates, tags = ([], []), []
    for c, n_units in enumerate((300, 200, 250)):
        for pair in _fragments(chr21[1], rng, n_units):
            umi = bytes(b'ACGT'[int(k)] for k in rng.integers(0, 4, 8))
            for _ in range(int(rng.integers(1, 3))):
                mates[0].append(pair[0]), mates[1].append(pair[1]), tags.append(barcodes[c] + umi + b'TTTT')
    order = rng.permutation(len(tags))
    pooled = [folder / 'pool_1.fastq', folder / 'pool_2.fastq', folder / 'pool_barcodes.fastq']
    _write_fastq(pooled[0], [mates[0][u] for u in order])
    _write_fastq(pooled[1], [mates[1][u] for u in order])
    _write_fastq(pooled[2], [tags[u] for u in order])
    return index_path, map_path, groups, [str(f) for f in pooled] + [str(folder / 'whitelist.tsv')]


NAMES = ['small', 'tiny', 'mid']
COUNT_FILES = ['cells.tsv', 'genes.tsv', 'matrix.mtx', 'matrix.npz']


def _many(cli_inputs, out, *options):
    from seekmer_amd import __main__ as cli
    index_path, _, groups, _ = cli_inputs
    fastq = [path for name in NAMES for path in groups[name]]
    assert cli.main(['infer-many', str(index_path), str(out), *fastq, '--names', ','.join(NAMES), *options]) == 0
    return out


@pytest.fixture(scope='module')
def full_run(cli_inputs, tmp_path_factory):
    """`infer-many --genes --gene-map FILE --count-matrix` through the set"""
    os.environ.pop('SKM_INFER_MANY_PER_SAMPLE', None)
    return _many(cli_inputs, tmp_path_factory.mktemp('gene_matrix_full') / 'out', '--genes', '--gene-map', str(cli_inputs[1]),
                 '--count-matrix')


def _same_counts(a, b):
    assert sorted(f.name for f in (a / 'counts').iterdir()) == COUNT_FILES == sorted(f.name for f in (b / 'counts').iterdir())
    for name in COUNT_FILES:
        assert (a / 'counts' / name).read_bytes() == (b / 'counts' / name).read_bytes(), name


def test_count_matrix_is_the_dense_table_and_changes_no_other_file(cli_inputs, full_run, tmp_path, monkeypatch):
    from seekmer_amd import infer
    from test_gpu_genes import _same_folder
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    without = _many(cli_inputs, tmp_path / 'without', '--genes', '--gene-map', str(cli_inputs[1]))
    top = sorted(NAMES + ['samples.tsv', 'genes.tpm.tsv', 'genes.unique_counts.tsv'])
    assert sorted(f.name for f in without.iterdir()) == top and sorted(f.name for f in full_run.iterdir()) == sorted(top + ['counts'])
    for name in ('samples.tsv', 'genes.tpm.tsv', 'genes.unique_counts.tsv'):
        assert (without / name).read_bytes() == (full_run / name).read_bytes(), name
    for name in NAMES:
        _same_folder(without / name, full_run / name)
    # matrix.mtx densified is genes.unique_counts.tsv
    lines = (full_run / 'counts' / 'matrix.mtx').read_text().splitlines(keepends=True)
    n_genes, comment, indptr, indices, data = mref.parse_mtx(lines)
    assert comment == infer.COUNT_MATRIX_COMMENT
    mref.check_csr(indptr, indices, data, len(NAMES), n_genes)
    rows = [line.split('\t') for line in (full_run / 'genes.unique_counts.tsv').read_text().splitlines()]
    assert rows[0] == ['gene_id'] + NAMES
    dense = np.asarray([[int(v) for v in row[1:]] for row in rows[1:]], dtype=np.int64).T
    np.testing.assert_array_equal(mref.dense(indptr, indices, data, n_genes), dense)
    assert (np.diff(indptr) > 0).all() and indptr[-1] == np.count_nonzero(dense)
    assert (full_run / 'counts' / 'genes.tsv').read_text().splitlines() == [row[0] for row in rows[1:]]
    arrays = np.load(full_run / 'counts' / 'matrix.npz')
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [len(NAMES), n_genes]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want)
    # cells.tsv: the units and aligned units of samples.tsv, and columns 4 to 6 add up to column 3
    cells = [line.split('\t') for line in (full_run / 'counts' / 'cells.tsv').read_text().splitlines()]
    samples = [line.split('\t') for line in (full_run / 'samples.tsv').read_text().splitlines()]
    assert [row[:3] for row in cells] == [row[:3] for row in samples] and [row[0] for row in cells] == NAMES
    for s, row in enumerate(cells):
        assert int(row[3]) + int(row[4]) + int(row[5]) == int(row[2]) and int(row[3]) == dense[s].sum()
        assert int(row[6]) == indptr[s + 1] - indptr[s] and min(int(v) for v in row[3:6]) > 0


def test_count_matrix_alone_writes_no_gene_tables_and_sample_by_sample_the_same_counts(cli_inputs, full_run, tmp_path, monkeypatch):
    monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', '1')
    one_by_one = _many(cli_inputs, tmp_path / 'one_by_one', '--gene-map', str(cli_inputs[1]), '--count-matrix')
    assert sorted(f.name for f in one_by_one.iterdir()) == sorted(NAMES + ['samples.tsv', 'counts'])
    _same_counts(one_by_one, full_run)
    assert (one_by_one / 'samples.tsv').read_bytes() == (full_run / 'samples.tsv').read_bytes()
    assert 'abundance.genes.tsv' not in [f.name for f in (one_by_one / 'small').iterdir()]


@pytest.mark.parametrize('per_sample', [None, '1'], ids=['set', 'one by one'])
def test_matrix_only_stops_before_the_em(cli_inputs, full_run, tmp_path, monkeypatch, per_sample):
    from seekmer_amd import infer, mapper
    called = []
    for module, name in ((infer, 'quantify'), (mapper.SampleSet, 'summarize'), (mapper.SampleSet, 'quantify'),
                         (mapper.MapResult, 'summarize'), (infer, 'output_results')):
        monkeypatch.setattr(module, name, lambda *a, _name=name, **k: called.append(_name) or pytest.fail(_name + ' was called'))
    if per_sample:
        monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', per_sample)
    else:
        monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    out = _many(cli_inputs, tmp_path / 'matrix_only', '--gene-map', str(cli_inputs[1]), '--matrix-only')
    assert called == []
    assert sorted(f.name for f in out.iterdir()) == ['counts', 'samples.tsv']              # no folder per sample
    _same_counts(out, full_run)
    assert (out / 'samples.tsv').read_bytes() == (full_run / 'samples.tsv').read_bytes()


def test_count_matrix_needs_genes(cli_inputs, tmp_path):
    """the index has no genes and no --gene-map is given: NO_GENES, and nothing of the run is written"""
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    index_path, _, groups, _ = cli_inputs
    for option in ('--count-matrix', '--matrix-only'):
        out = tmp_path / option.strip('-')
        with pytest.raises(ValueError) as refused:
            cli.main(['infer-many', str(index_path), str(out), *groups['small'], *groups['tiny'], option])
        assert str(refused.value) == infer.NO_GENES
        assert not out.exists() or list(out.iterdir()) == []


def test_matrix_only_of_a_pooled_run(cli_inputs, tmp_path, monkeypatch):
    from seekmer_amd import __main__ as cli
    index_path, map_path, _, (mate1, mate2, barcode_file, whitelist) = cli_inputs
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    options = ['--barcodes', whitelist, '--barcode-file', barcode_file, '--umi-start', '10', '--umi-length', '8',
               '--gene-map', str(map_path)]
    full, only = tmp_path / 'full', tmp_path / 'only'
    assert cli.main(['infer-many', str(index_path), str(full), mate1, mate2, *options, '--count-matrix']) == 0
    assert cli.main(['infer-many', str(index_path), str(only), mate1, mate2, *options, '--matrix-only']) == 0
    cells = ['cell0', 'cell1', 'cell2']
    assert sorted(f.name for f in full.iterdir()) == sorted(cells + ['barcodes.json', 'barcodes.tsv', 'counts', 'samples.tsv'])
    assert sorted(f.name for f in only.iterdir()) == ['barcodes.json', 'barcodes.tsv', 'counts', 'samples.tsv']
    _same_counts(only, full)
    for name in ('barcodes.tsv', 'barcodes.json', 'samples.tsv'):
        assert (only / name).read_bytes() == (full / name).read_bytes(), name
    rows = [line.split('\t') for line in (full / 'counts' / 'cells.tsv').read_text().splitlines()]
    codes = [line.split('\t') for line in (full / 'barcodes.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == cells
    # UMI collapse came first: a cell's units are what is left of its 300, 200 and 250 fragments written once or twice
    assert [int(row[1]) for row in rows] == [int(code[5]) for code in codes]
    for row, fragments, code in zip(rows, (300, 200, 250), codes):
        assert int(row[1]) < int(code[4]) and fragments < int(code[4])
        assert int(row[3]) + int(row[4]) + int(row[5]) == int(row[2]) > 0
