"""The molecule matrix without a GPU: the rule of DESIGN.md section 4, "Molecule matrix", on hand-made cases (one per
sentence of the rule), what follows from it against the unit matrix on a random table, the option checks of
`infer-many --count-molecules` that need no device, and the writer of molecules.mtx / molecules.npz."""
import pathlib

import numpy as np
import pytest

import gene_matrix_reference as mref
import molecule_reference as mol

#          transcripts 0 1 2 in gene 0, 3 4 in gene 1, 5 unnamed, 6 in gene 2
TX_GENE = np.asarray([0, 0, 0, 1, 1, -1, 2], dtype=np.int32)


def _entries(units, stay=None):
    """units: (cell, umi, tuple)"""
    cell, umi, tuples = zip(*units)
    return mol.entries(cell, umi, tuples, [True] * len(units) if stay is None else stay, TX_GENE)


def test_distinct_umis_of_the_classes_inside_a_gene():
    # one molecule, three fragments, three classes of gene 0: one
    assert _entries([(0, 7, (0,)), (0, 7, (0, 1)), (0, 7, (1, 2))]) == ({(0, 0): 1}, {})
    # two UMIs in one class, a third in another class of the gene: three
    assert _entries([(0, 7, (0,)), (0, 8, (0,)), (0, 9, (1, 2))]) == ({(0, 0): 3}, {})


def test_inside_a_gene_is_the_gene_rule():
    counted, other = _entries([(0, 1, (0, 3)), (0, 2, (5,)), (0, 3, (0, 5)), (0, 4, (6,))])
    assert counted == {(0, 2): 1}
    assert other == {0: [2, 1]}             # (0, 3) and (0, 5) are ambiguous; (5,) is unnamed


def test_only_surviving_units_count():
    units = [(0, 7, (0,)), (0, 8, (0, 1)), (0, 9, (3,))]
    assert _entries(units, stay=[True, False, False]) == ({(0, 0): 1}, {})
    assert _entries(units, stay=[False, False, False]) == ({}, {})
    assert _entries([(-1, 7, (0,)), (0, 7, ())]) == ({}, {})           # no cell; unaligned


def test_umis_are_compared_letter_for_letter():
    # one substitution apart (the last base), in two classes of gene 0: two molecules
    assert _entries([(0, 0b0100, (0,)), (0, 0b0101, (0, 1))]) == ({(0, 0): 2}, {})


def test_the_same_umi_in_two_cells_and_in_two_genes():
    assert _entries([(0, 7, (0,)), (1, 7, (0, 1))]) == ({(0, 0): 1, (1, 0): 1}, {})
    assert _entries([(0, 7, (0,)), (0, 7, (3, 4))]) == ({(0, 0): 1, (0, 1): 1}, {})


def test_a_umi_in_a_unique_and_in_an_ambiguous_class_counts_once_for_the_unique_one():
    counted, other = _entries([(0, 7, (0, 1)), (0, 7, (0, 3))])
    assert counted == {(0, 0): 1} and other == {0: [1, 0]}


def test_other_is_the_unit_matrix_s():
    """every survivor is one (cell, class, UMI) molecule: the ambiguous and unnamed words count units"""
    units = [(0, 1, (0, 3)), (0, 1, (0, 4)), (0, 2, (5,)), (1, 2, (5,)), (1, 9, (1, 3))]
    _, other = _entries(units)
    cell, umi, tuples = zip(*units)
    indptr, indices, data, rows = mol.matrix(cell, umi, tuples, [True] * 5, TX_GENE, 2)
    assert other == {0: [2, 1], 1: [1, 1]} and rows.tolist() == [[2, 1], [1, 1]] and data.size == 0


def test_from_triples():
    assert mol.from_triples([0, 0, 0, 1, 0], [4, 4, 4, 4, 2], [9, 9, 8, 9, 9]) == {(0, 4): 2, (1, 4): 1, (0, 2): 1}
    assert mol.from_triples([], [], []) == {}


def test_what_follows_against_the_unit_matrix_on_a_random_table():
    """same pattern, 1 <= molecules <= units, and equality exactly where no UMI of the cell occurs in two classes of
    the gene -- on survivors made by the exact collapse rule"""
    import umi_reference
    rng = np.random.default_rng(5)
    n_tx, n_genes, n_cells, n = 60, 12, 4, 6000
    tx_gene = (np.arange(n_tx) // 5).astype(np.int32)
    tx_gene[rng.random(n_tx) < 0.1] = -1
    classes = [()]
    for _ in range(80):
        g = int(rng.integers(n_genes))
        inside = rng.random() < 0.8
        pick = np.flatnonzero(np.arange(n_tx) // 5 == g) if inside else np.arange(n_tx)
        classes.append(tuple(sorted(set(int(t) for t in rng.choice(pick, size=int(rng.integers(1, 4)))))))
    tuples = [classes[int(k)] for k in rng.integers(len(classes), size=n)]
    cell = rng.integers(-1, n_cells, size=n)
    umi = np.where(cell < 2, rng.integers(0, 40, size=n), rng.integers(0, 2 ** 32, size=n))       # (cells 2 and 3: hardly a UMI twice)
    stay = umi_reference.survivors(cell, umi, tuples)
    molecules, other = mol.entries(cell, umi, tuples, stay, tx_gene)
    units = mol.unit_entries(cell, tuples, stay, tx_gene)
    assert sorted(molecules) == sorted(units) and len(units) > 30
    shared = {}
    for c, m, t, keep in zip(cell, umi, tuples, stay):
        if keep and c >= 0 and t and mol.kind(t, tx_gene) >= 0:
            shared.setdefault((int(c), mol.kind(t, tx_gene)), {}).setdefault(int(m), set()).add(t)
    below = equal = 0
    for key, count in molecules.items():
        assert 1 <= count <= units[key]
        in_two = any(len(of) > 1 for of in shared[key].values())
        assert (count == units[key]) == (not in_two), key
        below, equal = below + (count < units[key]), equal + (count == units[key])
    assert below >= 5 and equal >= 5
    # and the CSR of both has one pattern
    a, b = mref.csr(molecules, n_cells), mref.csr(units, n_cells)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[2] <= b[2]).all()
    rows = mol.matrix(cell, umi, tuples, stay, tx_gene, n_cells)[3]
    assert rows.sum() == sum(1 for c, t, keep in zip(cell, tuples, stay) if keep and c >= 0 and t and mol.kind(t, tx_gene) < 0)


def test_count_molecules_refusals_that_need_no_gpu(tmp_path):
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    missing = [pathlib.Path(tmp_path / name) for name in ('no_index.npz', 'no_1.fastq', 'no_2.fastq')]
    base = dict(job_count=1, single_ended=False, bootstrap=0, debug=False, count_molecules=True)
    pooled = dict(barcodes=tmp_path / 'no_whitelist.tsv', barcode_file=tmp_path / 'no_barcodes.fastq')
    for keywords in ({}, pooled, dict(pooled, matrix_only=True), dict(discover_cells=10, barcode_length=12, barcode_file=tmp_path / 'b.fastq')):
        with pytest.raises(ValueError) as refused:                    # no --umi-length: pooled or not
            infer.run_many(missing[0], tmp_path / 'out', missing[1:], **base, **keywords)
        assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS
    assert not (tmp_path / 'out').exists()
    # with UMIs the option passes its own check: what refuses next is the whitelist that does not exist
    with pytest.raises(Exception) as refused:
        infer.run_many(missing[0], tmp_path / 'out', missing[1:], **base, **pooled, umi_length=8)
    assert str(refused.value) != infer.COUNT_MOLECULES_NEEDS_UMIS and not (tmp_path / 'out').exists()
    # the command line: --count-molecules implies --count-matrix, and a gene map then serves the matrices
    many = ['infer-many', 'index', 'out', 'a_1.fastq', 'a_2.fastq']
    opts = cli.parse_args(many + ['--count-molecules', '--gene-map', 'map.tsv', '--barcodes', 'w.tsv', '--barcode-file', 'b.fastq',
                                  '--umi-length', '8'])
    assert opts['count_molecules'] and opts['count_matrix'] and not opts['matrix_only'] and not opts['genes']
    opts = cli.parse_args(many + ['--count-matrix'])
    assert not opts['count_molecules']
    with pytest.raises(ValueError) as refused:                        # not pooled, through the command line
        cli.main(many + ['--count-molecules'])
    assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS
    for command in (['infer', 'index', 'out', 'a_1.fastq', 'a_2.fastq'], ['impute', 'index', 'out', 'a_1.fastq', 'a_2.fastq']):
        with pytest.raises(SystemExit):
            cli.parse_args(command + ['--count-molecules'])


def test_the_writer_of_the_molecule_files(tmp_path):
    from seekmer_amd import infer
    counted = {(0, 3): 2, (0, 70000): 1, (2, 0): 5}
    indptr, indices, data = mref.csr(counted, 3)
    infer.output_molecule_matrix(tmp_path, 70001, 3, indptr, indices, data)
    assert sorted(f.name for f in (tmp_path / 'counts').iterdir()) == ['molecules.mtx', 'molecules.npz']
    lines = (tmp_path / 'counts' / 'molecules.mtx').read_text().splitlines(keepends=True)
    assert lines == mref.mtx_lines(indptr, indices, data, 70001, infer.MOLECULE_MATRIX_COMMENT)
    assert infer.MOLECULE_MATRIX_COMMENT != infer.COUNT_MATRIX_COMMENT and infer.MOLECULE_MATRIX_COMMENT.startswith('%')
    arrays = np.load(tmp_path / 'counts' / 'molecules.npz')
    assert sorted(arrays.files) == ['data', 'format', 'indices', 'indptr', 'shape']
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [3, 70001]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want)
    first = (tmp_path / 'counts' / 'molecules.npz').read_bytes()
    infer.output_molecule_matrix(tmp_path, 70001, 3, indptr, indices, data)
    assert (tmp_path / 'counts' / 'molecules.npz').read_bytes() == first
    with pytest.raises(ValueError):
        infer.output_molecule_matrix(tmp_path, 70001, 3, indptr[:-1], indices, data)
