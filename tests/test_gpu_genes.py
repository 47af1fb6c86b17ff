"""Gene-level tables on the device: gene sums bit for bit against numpy.add.at, gene-unique counts exact against
tests/gene_reference.py -- on hand-made tables, on a mapper's resident table and on a sample set's -- and the
command line (`infer --genes`, `infer-many --genes`)."""
import json
import os

import numpy as np
import pytest

import gene_reference as ref
from conftest import GOLDEN, make_product_index
from strand_reference import reverse_complement

pytestmark = pytest.mark.gpu


def _env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


# ------------------------------------------------------------------------------------------------ gene sums
def _interleaved_genes(rng):
    """tx_gene[1000]: genes of 0, 1, 2, 63, 64, 65 and 300 transcripts (gene 0 has none), interleaved, the rest unnamed"""
    sizes = [0, 1, 2, 63, 64, 65, 300]
    tx_gene = np.full(1000, -1, dtype=np.int32)
    places = rng.permutation(1000)[:sum(sizes)]
    tx_gene[places] = np.repeat(np.arange(len(sizes)), sizes)
    assert np.bincount(tx_gene[tx_gene >= 0], minlength=7).tolist() == sizes and (tx_gene == -1).sum() == 505
    return tx_gene, len(sizes)


@pytest.mark.parametrize('group', [None, '2'], ids=['one group', 'groups of 2'])
@pytest.mark.parametrize('n_rows', [1, 4, 9])
def test_gene_sums_are_numpy_add_at_bit_for_bit(native_libs, monkeypatch, n_rows, group):
    from seekmer_amd import infer
    rng = np.random.default_rng(1000 + n_rows)
    tx_gene, n_genes = _interleaved_genes(rng)
    # 1e-8 .. 1e6 with zeros: the order of the additions decides the last bits
    rows = 10.0 ** rng.uniform(-8, 6, (n_rows, 1000)) * (rng.uniform(0, 1, (n_rows, 1000)) > 0.1)
    want = ref.gene_sums(tx_gene, n_genes, rows)
    shuffled = np.zeros_like(want)                                 # (the same values added in another order differ)
    order = rng.permutation(1000)
    for r in range(n_rows):
        np.add.at(shuffled[r], tx_gene[order][tx_gene[order] >= 0], rows[r][order][tx_gene[order] >= 0])
    assert shuffled.tobytes() != want.tobytes()
    _env(monkeypatch, 'SKM_GENE_GROUP', group)
    got = infer.gene_sums(tx_gene, n_genes, rows)
    assert got.shape == (n_rows, n_genes) and got.dtype == np.float64
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes()
    assert not got[:, 0].any()
    # one gene for everything that is named, and a single row given as a vector
    one = np.where(tx_gene >= 0, 0, -1).astype(np.int32)
    got = infer.gene_sums(one, 1, rows)
    assert got.shape == (n_rows, 1) and np.array_equal(got, ref.gene_sums(one, 1, rows))
    assert np.array_equal(infer.gene_sums(tx_gene, n_genes, rows[0]), want[0])
    with pytest.raises(ValueError):                                # (SKM_ERR_ARG: a gene number of n_genes)
        infer.gene_sums(np.where(tx_gene == 6, 7, tx_gene), n_genes, rows)


# ---------------------------------------------------------------------------------- hand-made class tables
N_TX = 17000
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 5000]


def _hand_made_genes():
    """[0, 5500) gene 0, [5500, 11000) gene 1, [11000, 16500) unnamed, [16500, 17000) gene 2; gene 3 has no transcript"""
    tx_gene = np.full(N_TX, -1, dtype=np.int32)
    tx_gene[:5500], tx_gene[5500:11000], tx_gene[16500:] = 0, 1, 2
    return tx_gene, 4


def _hand_made_table():
    """(offsets, targets, counts): for every length of LENGTHS the cases of a class: all of one gene; the odd id first;
    last; at offsets 64 and 256 where the class is long enough; all unnamed; one gene plus one unnamed id"""
    rng = np.random.default_rng(99)
    first = {0: 0, 1: 5500, -1: 11000}
    classes = []
    for n in LENGTHS:
        for gene in (0, 1):
            plain = first[gene] + rng.permutation(5500)[:n]
            classes.append(plain)
            for at in (0, n - 1, 64, 256):
                if at < n and n > 1 or at == 0:
                    odd = plain.copy()
                    odd[at] = first[1 - gene] + int(rng.integers(5500))
                    classes.append(odd)
            if n > 1:
                mixed = plain.copy()
                mixed[int(rng.integers(n))] = first[-1] + int(rng.integers(5500))
                classes.append(mixed)
        classes.append(first[-1] + rng.permutation(5500)[:n])
        classes.append(16500 + rng.integers(0, 500, n))           # (the small gene, ids repeated)
    order = rng.permutation(len(classes))
    classes = [classes[k] for k in order]
    offsets = np.concatenate([[0], np.cumsum([c.size for c in classes])]).astype(np.int64)
    targets = np.concatenate(classes).astype(np.int32)
    counts = rng.integers(1, 1 << 40, len(classes)).astype(np.int64)
    return offsets, targets, counts


def _native_counts(native_libs, offsets, targets, counts, sample, n_samples, tx_gene, n_genes, n_tx=None):
    p, i32, i64 = native_libs.ptr, native_libs.c_i32p, native_libs.c_i64p
    unique = np.full((n_samples, n_genes), -7, dtype=np.int64)
    other = np.full((n_samples, 2), -7, dtype=np.int64)
    code = native_libs.hip().skm_gene_unique_counts(
        0, counts.size, p(offsets, i64), p(targets, i32) if targets.size else None, p(counts, i64) if counts.size else None,
        p(sample, i32) if sample is not None else None, n_samples, tx_gene.size if n_tx is None else n_tx, n_genes,
        p(tx_gene, i32), p(unique, i64), p(other, i64))
    return code, unique, other


@pytest.mark.parametrize('group', [None, '2'], ids=['one range', 'ranges of 2'])
def test_unique_counts_of_hand_made_tables(native_libs, monkeypatch, group):
    tx_gene, n_genes = _hand_made_genes()
    offsets, targets, counts = _hand_made_table()
    assert sorted(set(np.diff(offsets).tolist())) == LENGTHS
    _env(monkeypatch, 'SKM_GENE_GROUP', group)
    # one sample
    want_unique, want_other = ref.unique_counts(offsets, targets, counts, tx_gene, n_genes)
    assert want_unique[0, :3].min() > 1 << 32 and want_unique[0, 3] == 0 and want_other.min() > 1 << 32
    code, unique, other = _native_counts(native_libs, offsets, targets, counts, None, 1, tx_gene, n_genes)
    assert code == native_libs.SKM_OK
    np.testing.assert_array_equal(unique, want_unique)
    np.testing.assert_array_equal(other, want_other)
    assert unique.sum() + other.sum() == counts.sum()
    # five samples, sample 3 owns no class
    sample = np.asarray([0, 1, 2, 4], dtype=np.int32)[np.arange(counts.size) % 4]
    want_unique, want_other = ref.unique_counts(offsets, targets, counts, tx_gene, n_genes, sample, 5)
    code, unique, other = _native_counts(native_libs, offsets, targets, counts, sample, 5, tx_gene, n_genes)
    assert code == native_libs.SKM_OK
    np.testing.assert_array_equal(unique, want_unique)
    np.testing.assert_array_equal(other, want_other)
    assert not unique[3].any() and not other[3].any() and unique[[0, 1, 2, 4]].any(axis=1).all()


def test_unique_counts_of_an_empty_table_and_bad_gene_maps(native_libs):
    tx_gene, n_genes = _hand_made_genes()
    offsets, targets, counts = _hand_made_table()
    none = np.zeros(0, dtype=np.int64)
    code, unique, other = _native_counts(native_libs, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), none, None, 3,
                                         tx_gene, n_genes)
    assert code == native_libs.SKM_OK and not unique.any() and not other.any()
    # a gene number of n_genes; a gene number below -1; a tx_gene shorter than the ids of the table
    for bad in (n_genes, -2):
        wrong = tx_gene.copy()
        wrong[N_TX - 1] = bad
        code, unique, other = _native_counts(native_libs, offsets, targets, counts, None, 1, wrong, n_genes)
        assert code == native_libs.SKM_ERR_ARG and (unique == -7).all() and (other == -7).all()
    short = int(targets.max())                                    # (the largest id is then not below n_tx)
    code, unique, other = _native_counts(native_libs, offsets, targets, counts, None, 1, tx_gene[:short].copy(), n_genes, n_tx=short)
    assert code == native_libs.SKM_ERR_ARG and (unique == -7).all()
    # a class of a sample that is not there
    sample = np.zeros(counts.size, dtype=np.int32)
    sample[5] = 2
    assert _native_counts(native_libs, offsets, targets, counts, sample, 2, tx_gene, n_genes)[0] == native_libs.SKM_ERR_ARG


# ------------------------------------------------------------------------------------ chr21: the inputs
def _fragments(seqs, rng, n_units, read_len=60):
    """[mate 1, mate 2] of n_units chr21 fragments, either mate first (the recipe of test_gpu_set_bias.py)"""
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
def fragments2000(chr21):
    return _reads(_fragments(chr21[1], np.random.default_rng(606), 2000))


# --------------------------------------------------------------------------------------- resident mapper
@pytest.mark.parametrize('strand', [None, 'fr'])
def test_mapper_counts_on_the_resident_table(oracle, native_libs, chr21_index, fragments2000, strand):
    from seekmer_amd import infer, mapper
    index = chr21_index
    gene_ids, tx_gene = _chr21_genes(index.transcripts.size)
    n_genes = gene_ids.size
    result = mapper.MapResult(index, strand=strand)
    empty_unique, empty_other = result.gene_unique_counts(tx_gene, n_genes)
    assert empty_unique.shape == (n_genes,) and not empty_unique.any() and not empty_other.any()     # no classes yet
    mapper.ReadMapper(index, result).map_batch(_batch(oracle, fragments2000))
    unique, other = result.gene_unique_counts(tx_gene, n_genes)
    assert unique.dtype == np.int64 and unique.shape == (n_genes,) and other.shape == (2,)
    offsets, targets, counts, _, _ = result.export()
    want_unique, want_other = ref.unique_counts(offsets, targets, counts, tx_gene, n_genes)
    np.testing.assert_array_equal(unique, want_unique[0])
    np.testing.assert_array_equal(other, want_other[0])
    from_summary = infer.gene_unique_counts(result.summarize(), tx_gene, n_genes)
    np.testing.assert_array_equal(from_summary[0], unique)
    np.testing.assert_array_equal(from_summary[1], other)
    _, _, unaligned, total = result.sizes()
    aligned = total - unaligned
    print(strand, 'unique / ambiguous / unnamed of', aligned, ':', int(unique.sum()), int(other[0]), int(other[1]))
    assert total == 2000 and unique.sum() + other.sum() == aligned
    for kind in (unique.sum(), other[0], other[1]):
        assert kind >= 0.02 * aligned
    # a gene map that does not cover the index's transcripts is refused, not read past
    with pytest.raises(ValueError):
        result.gene_unique_counts(tx_gene[:-1], n_genes)
    p, i32, i64 = native_libs.ptr, native_libs.c_i32p, native_libs.c_i64p
    few = int(targets.max())
    assert native_libs.hip().skm_mapper_gene_counts(result._handle, few, n_genes, p(tx_gene, i32), p(unique.copy(), i64),
                                                    p(other.copy(), i64)) == native_libs.SKM_ERR_ARG


# -------------------------------------------------------------------------------------------- sample set
@pytest.fixture(scope='module')
def set_samples(chr21):
    """samples of 40, 41 and 600 units, one without units, one whose units all fail to align"""
    rng = np.random.default_rng(607)
    samples = [_reads(_fragments(chr21[1], rng, n)) for n in (40, 41, 600)]
    samples.append([])
    samples.append([bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, 60)) for _ in range(100)])
    return samples


@pytest.fixture(scope='module')
def set_samples_alone(oracle, native_libs, chr21_index, set_samples):
    """every sample through a mapper of its own: (unique[5][n_genes], other[5][2])"""
    from seekmer_amd import mapper
    gene_ids, tx_gene = _chr21_genes(chr21_index.transcripts.size)
    unique = np.zeros((len(set_samples), gene_ids.size), dtype=np.int64)
    other = np.zeros((len(set_samples), 2), dtype=np.int64)
    for i, reads in enumerate(set_samples):
        if reads:
            result = mapper.MapResult(chr21_index)
            mapper.ReadMapper(chr21_index, result).map_batch(_batch(oracle, reads))
            unique[i], other[i] = result.gene_unique_counts(tx_gene, gene_ids.size)
    assert unique[:3].any(axis=1).all() and other[:3].any(axis=1).all() and not unique[3:].any() and not other[3:].any()
    return unique, other


@pytest.mark.parametrize('group', [None, '2'], ids=['one range', 'ranges of 2'])
@pytest.mark.parametrize('packed', [False, True], ids=['text', 'packed'])
def test_sample_set_rows_are_the_samples_mapped_alone(oracle, native_libs, chr21_index, set_samples, set_samples_alone,
                                                      monkeypatch, packed, group):
    from seekmer_amd import common, mapper
    gene_ids, tx_gene = _chr21_genes(chr21_index.transcripts.size)
    n_genes = gene_ids.size
    monkeypatch.setenv('SKM_SAMPLE_SET_MAX_UNITS', '256')
    _env(monkeypatch, 'SKM_GENE_GROUP', group)
    sample_set = mapper.SampleSet(chr21_index, True)
    unique, other = sample_set.gene_unique_counts(tx_gene, n_genes)
    assert unique.shape == (0, n_genes) and other.shape == (0, 2)                  # no samples yet
    for i, reads in enumerate(set_samples):
        if packed and reads:
            pieces = [common.PackedReads.from_ascii(*oracle.pack_reads(reads[mate::2]), stream=mate) for mate in range(2)]
            sample_set.add_packed(i, 0, *pieces)
        else:
            sample_set.add_batch(i, 0, _batch(oracle, reads))
    unique, other = sample_set.gene_unique_counts(tx_gene, n_genes)
    assert unique.shape == (5, n_genes) and other.shape == (5, 2) and unique.dtype == np.int64
    np.testing.assert_array_equal(unique, set_samples_alone[0])
    np.testing.assert_array_equal(other, set_samples_alone[1])
    sizes = sample_set.sizes()
    np.testing.assert_array_equal(unique.sum(axis=1) + other.sum(axis=1), sizes[:, 3] - sizes[:, 2])
    assert sizes[:, 3].tolist() == [40, 41, 600, 0, 50] and sizes[4, 2] == 50
    # room for fewer samples than the set names
    p, i32, i64 = native_libs.ptr, native_libs.c_i32p, native_libs.c_i64p
    room = np.zeros((4, n_genes), dtype=np.int64)
    assert native_libs.hip().skm_sample_set_gene_counts(sample_set._handle, tx_gene.size, n_genes, p(tx_gene, i32), 4, p(room, i64),
                                                        p(other.copy(), i64)) == native_libs.SKM_ERR_ARG
    assert not room.any()
    # a sample added afterwards: the next call sees it, the rows before it stay
    sample_set.add_batch(5, 0, _batch(oracle, set_samples[0]))
    again_unique, again_other = sample_set.gene_unique_counts(tx_gene, n_genes)
    np.testing.assert_array_equal(again_unique[:5], unique)
    np.testing.assert_array_equal(again_unique[5], unique[0])
    np.testing.assert_array_equal(again_other[5], other[0])


# ------------------------------------------------------------------------------------------ command line
def _write_fastq(path, reads):
    with open(path, 'wb') as f:
        for u, read in enumerate(reads):
            f.write(b'@u%d\n' % u + read + b'\n+\n' + b'I' * len(read) + b'\n')


@pytest.fixture(scope='module')
def cli_inputs(native_libs, chr21, tmp_path_factory):
    """(index file, gene-map file, {name: [mate 1 file, mate 2 file]})"""
    from seekmer_amd import __main__ as cli
    folder = tmp_path_factory.mktemp('genes_cli')
    gtf = folder / 'empty.gtf'
    gtf.write_text('')
    index_path = folder / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(index_path)]) == 0
    ids = [id_.split()[0].split(b'.')[0] for id_ in chr21[0]]
    map_path = folder / 'genes.tsv'
    with open(map_path, 'wb') as f:
        f.write(b'# transcript\tgene\n')
        for t, id_ in enumerate(ids):
            if (t // 4) % 10:
                f.write(id_ + b'.7\tG%05d\n' % (t // 4))
        f.write(b'NOT_THERE\tG00001\n')
    groups = {'golden': [os.path.join(GOLDEN, '20_1.fastq'), os.path.join(GOLDEN, '20_2.fastq')]}
    rng = np.random.default_rng(608)
    for name, n_units in (('small', 300), ('tiny', 45)):
        reads = _reads(_fragments(chr21[1], rng, n_units))
        files = [folder / (name + '_1.fastq'), folder / (name + '_2.fastq')]
        for mate in range(2):
            _write_fastq(files[mate], reads[mate::2])
        groups[name] = [str(f) for f in files]
    return index_path, map_path, groups


def _spy_on_outputs(monkeypatch):
    """what output_results was given, by output folder name"""
    from seekmer_amd import infer
    seen = {}
    original = infer.output_results

    def spy(output_path, index, start_time, results, main_abundance, bootstrapped_abundance, genes=None, device=0):
        seen[output_path.name] = (index, results, np.array(main_abundance), [np.array(b) for b in bootstrapped_abundance], genes)
        return original(output_path, index, start_time, results, main_abundance, bootstrapped_abundance, genes=genes, device=device)
    monkeypatch.setattr(infer, 'output_results', spy)
    return seen


def _same_folder(a, b):
    """Two output folders hold the same files with the same bytes, but for the start time and the call."""
    assert sorted(f.name for f in a.iterdir()) == sorted(f.name for f in b.iterdir())
    for f in a.iterdir():
        if f.name == 'abundance.npz':
            x, y = np.load(f), np.load(b / f.name)
            assert sorted(x.files) == sorted(y.files)
            for name in x.files:
                if name not in ('aux/call', 'aux/start_time'):
                    assert x[name].dtype == y[name].dtype and x[name].tobytes() == y[name].tobytes(), (f.name, name)
        elif f.name == 'run_info.json':
            i, j = json.load(f.open()), json.load((b / f.name).open())
            for info in (i, j):
                info.pop('start_time'), info.pop('call')
            assert i == j
        else:
            assert f.read_bytes() == (b / f.name).read_bytes(), f.name


def _check_gene_outputs(folder, seen, bootstraps):
    """the gene files of one sample's folder against the reference on what output_results was given"""
    from seekmer_amd import infer
    index, results, tpm, boots, genes = seen
    gene_ids, tx_gene, unique, other = genes
    offsets, targets = (results.class_offsets, results.class_targets) if results.class_offsets is not None \
        else infer._csr_from_class_map(results.class_map, results.class_count.size)
    want_unique, want_other = ref.unique_counts(offsets, targets, np.asarray(results.class_count, dtype=np.int64), tx_gene, gene_ids.size)
    np.testing.assert_array_equal(unique, want_unique[0])
    np.testing.assert_array_equal(other, want_other[0])
    est = infer._infer_est_counts(index, results, tpm)
    table = ref.gene_table(gene_ids, tx_gene, index.transcripts['length'], results.effective_lengths.astype('f8'), tpm, est, unique)
    assert (folder / 'abundance.genes.tsv').read_text().splitlines(keepends=True) == ref.gene_table_lines(table)
    arrays = np.load(folder / 'abundance.npz')
    for name, column in (('genes/ids', 'gene_id'), ('genes/tpm', 'tpm'), ('genes/est_counts', 'est_count'), ('genes/lengths', 'length'),
                         ('genes/eff_lengths', 'eff_length'), ('genes/unique_counts', 'unique_count')):
        assert arrays[name].dtype == table[column].dtype and arrays[name].tobytes() == table[column].tobytes(), name
    assert len(boots) == bootstraps
    for i in range(bootstraps):
        assert arrays['bootstrap/bs%d' % i].tobytes() == boots[i].tobytes()
        assert arrays['genes/bootstrap/bs%d' % i].tobytes() == ref.gene_sums(tx_gene, gene_ids.size, arrays['bootstrap/bs%d' % i])[0].tobytes()
    assert 'genes/bootstrap/bs%d' % bootstraps not in arrays.files
    info = json.load((folder / 'run_info.json').open())
    assert info['n_genes'] == gene_ids.size
    assert (info['n_gene_unique'], info['n_gene_ambiguous'], info['n_gene_unnamed']) == (int(unique.sum()), int(other[0]), int(other[1]))
    assert info['n_gene_unique'] + info['n_gene_ambiguous'] + info['n_gene_unnamed'] == info['n_pseudoaligned']
    return info


def test_infer_genes(native_libs, cli_inputs, tmp_path, monkeypatch):
    from seekmer_amd import __main__ as cli
    index_path, map_path, groups = cli_inputs
    seen = _spy_on_outputs(monkeypatch)
    options = ['-b', '3', '--seed', '7']
    for name in ('golden', 'small'):
        plain, with_genes = tmp_path / (name + '_plain'), tmp_path / (name + '_genes')
        assert cli.main(['infer', str(index_path), str(plain), *groups[name], *options]) == 0
        assert cli.main(['infer', str(index_path), str(with_genes), *groups[name], *options, '--gene-map', str(map_path)]) == 0
        # nothing that was written before changes
        assert sorted(f.name for f in plain.iterdir()) == ['abundance.npz', 'abundance.tsv', 'run_info.json']
        assert sorted(f.name for f in with_genes.iterdir()) == ['abundance.genes.tsv', 'abundance.npz', 'abundance.tsv', 'run_info.json']
        assert (plain / 'abundance.tsv').read_bytes() == (with_genes / 'abundance.tsv').read_bytes()
        a, b = np.load(plain / 'abundance.npz'), np.load(with_genes / 'abundance.npz')
        for dataset in a.files:
            if dataset not in ('aux/call', 'aux/start_time'):
                assert a[dataset].dtype == b[dataset].dtype and a[dataset].tobytes() == b[dataset].tobytes(), dataset
        assert all(dataset.startswith('genes/') for dataset in set(b.files) - set(a.files))
        info, before = json.load((with_genes / 'run_info.json').open()), json.load((plain / 'run_info.json').open())
        assert seen[plain.name][4] is None
        assert {key: info[key] for key in before if key not in ('start_time', 'call')} == \
            {key: before[key] for key in before if key not in ('start_time', 'call')}
        assert sorted(set(info) - set(before)) == ['n_gene_ambiguous', 'n_gene_unique', 'n_gene_unnamed', 'n_genes']
        info = _check_gene_outputs(with_genes, seen[with_genes.name], 3)
        if name == 'small':
            assert min(info['n_gene_unique'], info['n_gene_ambiguous'], info['n_gene_unnamed']) > 0
    # an index without genes and no --gene-map: refused
    with pytest.raises(ValueError) as refused:
        cli.main(['infer', str(index_path), str(tmp_path / 'refused'), *groups['golden'], '--genes'])
    assert '--gene-map' in str(refused.value) and not (tmp_path / 'refused').exists()


def test_infer_many_genes(native_libs, cli_inputs, tmp_path, monkeypatch, caplog):
    import logging
    from seekmer_amd import __main__ as cli
    index_path, map_path, groups = cli_inputs
    names = ['golden', 'small', 'tiny']
    fastq = [path for name in names for path in groups[name]]
    options = ['-b', '2', '--seed', '5', '--gene-map', str(map_path)]
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    through_set, one_by_one = tmp_path / 'set', tmp_path / 'one_by_one'
    with caplog.at_level(logging.INFO):
        assert cli.main(['infer-many', str(index_path), str(through_set), *fastq, '--names', ','.join(names), *options]) == 0
    assert any('Mapping 3 samples in shared launches' in record.getMessage() for record in caplog.records)
    caplog.clear()
    monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', '1')
    with caplog.at_level(logging.INFO):
        assert cli.main(['infer-many', str(index_path), str(one_by_one), *fastq, '--names', ','.join(names), *options]) == 0
    assert not any('in shared launches' in record.getMessage() for record in caplog.records)
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE')
    top = sorted(names + ['samples.tsv', 'genes.tpm.tsv', 'genes.unique_counts.tsv'])
    assert sorted(f.name for f in through_set.iterdir()) == top == sorted(f.name for f in one_by_one.iterdir())
    for name in ('samples.tsv', 'genes.tpm.tsv', 'genes.unique_counts.tsv'):
        assert (through_set / name).read_bytes() == (one_by_one / name).read_bytes(), name
    columns = {}
    for name in names:
        _same_folder(through_set / name, one_by_one / name)
        alone = tmp_path / ('alone_' + name)
        assert cli.main(['infer', str(index_path), str(alone), *groups[name], *options]) == 0
        _same_folder(through_set / name, alone)
        lines = [line.split('\t') for line in (alone / 'abundance.genes.tsv').read_text().splitlines()[1:]]
        columns[name] = ([line[0] for line in lines], [line[5] for line in lines], [line[6] for line in lines])
    # the two matrices: genes as rows, the folders' columns in sample order
    for file_name, which in (('genes.tpm.tsv', 1), ('genes.unique_counts.tsv', 2)):
        rows = [line.split('\t') for line in (through_set / file_name).read_text().splitlines()]
        assert rows[0] == ['gene_id'] + names
        assert [row[0] for row in rows[1:]] == columns['golden'][0]
        for k, name in enumerate(names):
            assert [row[1 + k] for row in rows[1:]] == columns[name][which], (file_name, name)


def test_genes_with_bias_come_from_the_corrected_result(native_libs, cli_inputs, tmp_path, monkeypatch):
    from seekmer_amd import __main__ as cli
    index_path, map_path, groups = cli_inputs
    seen = _spy_on_outputs(monkeypatch)
    plain, biased = tmp_path / 'plain', tmp_path / 'biased'
    assert cli.main(['infer', str(index_path), str(plain), *groups['small'], '--gene-map', str(map_path)]) == 0
    assert cli.main(['infer', str(index_path), str(biased), *groups['small'], '--gene-map', str(map_path), '--bias']) == 0
    _, results, tpm, _, genes = seen['biased']
    assert results.bias_weights is not None and tpm.tobytes() != seen['plain'][2].tobytes()
    _check_gene_outputs(biased, seen['biased'], 0)
    got = np.load(biased / 'abundance.npz')['genes/tpm']
    assert got.tobytes() == ref.gene_sums(genes[1], genes[0].size, tpm)[0].tobytes()
    assert got.tobytes() != np.load(plain / 'abundance.npz')['genes/tpm'].tobytes()
    np.testing.assert_array_equal(genes[2], seen['plain'][4][2])             # (the counts do not depend on the correction)
