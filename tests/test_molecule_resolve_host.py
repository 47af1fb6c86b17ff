"""Resolved molecules without a GPU: the rule of DESIGN.md section 4, "Resolved molecules", on hand-made cases (one per
outcome), what follows from it against the molecule matrix on random inputs, the option checks of
`infer-many --resolve-molecules` that need no device, the writer of the molecules.resolved.* files, and the compiler's
resource remarks for the kernels of skm_molecule_resolve.hip."""
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

import gene_matrix_reference as mref
import molecule_reference as mol
import molecule_resolve_reference as mres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#          transcripts 0 1 2 in gene 0, 3 4 in gene 1, 5 6 unnamed, 7 in gene 2
TX_GENE = np.asarray([0, 0, 0, 1, 1, -1, -1, 2], dtype=np.int32)


def _resolve(units, stay=None):
    """units: (cell, umi, tuple)"""
    cell, umi, tuples = zip(*units)
    return mres.resolve(cell, umi, tuples, [True] * len(units) if stay is None else stay, TX_GENE)


def test_resolved_and_rescued():
    # two classes across genes 0/1 and 0/2 under one UMI: only gene 0 is in both, and neither names it alone
    assert _resolve([(0, 7, (0, 3)), (0, 7, (1, 7))]) == ({(0, 0): 1}, {0: [1, 1, 0, 0, 0]})
    # a class inside the gene among them: resolved, not rescued
    assert _resolve([(0, 7, (0, 3)), (0, 7, (1, 2))]) == ({(0, 0): 1}, {0: [1, 0, 0, 0, 0]})
    # a group of one class resolves exactly when the class lies inside one gene
    assert _resolve([(0, 7, (0, 1))]) == ({(0, 0): 1}, {0: [1, 0, 0, 0, 0]})
    assert _resolve([(0, 7, (0, 3))]) == ({}, {0: [0, 0, 1, 0, 0]})
    # three classes, every two of which share more than the three do
    assert _resolve([(0, 7, (0, 3, 7)), (0, 7, (1, 4, 5)), (0, 7, (2, 7, 6))]) == ({(0, 0): 1}, {0: [1, 1, 0, 0, 0]})


def test_multi_gene():
    assert _resolve([(0, 7, (0, 3, 7)), (0, 7, (1, 4))]) == ({}, {0: [0, 0, 1, 0, 0]})
    # "no gene" is an element like any other: {g, -1}
    assert _resolve([(0, 7, (0, 5)), (0, 7, (6, 1, 7))]) == ({}, {0: [0, 0, 1, 0, 0]})


def test_unnamed():
    assert _resolve([(0, 7, (5,))]) == ({}, {0: [0, 0, 0, 1, 0]})
    assert _resolve([(0, 7, (5, 0)), (0, 7, (6, 3))]) == ({}, {0: [0, 0, 0, 1, 0]})


def test_collision():
    # the same UMI on molecules of two genes: molecules.mtx counts it once in each, here it is tallied
    assert _resolve([(0, 7, (0,)), (0, 7, (3, 4))]) == ({}, {0: [0, 0, 0, 0, 1]})
    assert mol.entries([0, 0], [7, 7], [(0,), (3, 4)], [True, True], TX_GENE)[0] == {(0, 0): 1, (0, 1): 1}
    assert _resolve([(0, 7, (0, 3)), (0, 7, (3, 7)), (0, 7, (7, 0))]) == ({}, {0: [0, 0, 0, 0, 1]})


def test_groups_are_per_cell_and_umi_over_the_live_molecules():
    units = [(0, 7, (0, 3)), (1, 7, (1, 7)), (0, 8, (1, 7)), (0, 7, (0, 3)), (-1, 7, (1, 7)), (0, 7, ())]
    assert _resolve(units) == ({}, {0: [0, 0, 2, 0, 0], 1: [0, 0, 1, 0, 0]})
    # a unit that does not stay takes its class out of the group -- unless another unit of the molecule stays
    units = [(0, 7, (0, 3)), (0, 7, (1, 7)), (0, 7, (1, 7))]
    assert _resolve(units, stay=[True, True, False]) == ({(0, 0): 1}, {0: [1, 1, 0, 0, 0]})
    assert _resolve(units, stay=[True, False, False]) == ({}, {0: [0, 0, 1, 0, 0]})
    assert _resolve(units, stay=[False, False, False]) == ({}, {})
    # UMIs are compared letter for letter
    assert _resolve([(0, 0b0100, (0, 3)), (0, 0b0101, (1, 7))]) == ({}, {0: [0, 0, 2, 0, 0]})


def test_from_classes_and_the_arrays():
    class_tuples = [(0, 3), (1, 7), (5,), (0, 3)]
    counted, tally = mres.from_classes(class_tuples, [0, 0, 1, 2], [0, 1, 1, 2, 3, 0], [7, 7, 7, 9, 7, 7], TX_GENE)
    assert counted == {(0, 0): 1} and tally == {0: [1, 1, 0, 0, 0], 1: [0, 0, 0, 1, 0], 2: [0, 0, 1, 0, 0]}
    indptr, indices, data, rows = mres.matrix_from_classes(class_tuples, [0, 0, 1, 2], [0, 1, 1, 2, 3, 0], [7, 7, 7, 9, 7, 7], TX_GENE, 4)
    assert indptr.tolist() == [0, 1, 1, 1, 1] and indices.tolist() == [0] and data.tolist() == [1]
    assert rows.tolist() == [[1, 1, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0] * 5] and rows.dtype == np.int64
    assert mres.other(rows).tolist() == [[0, 0], [0, 1], [1, 0], [0, 0]]


def _random_units(rng, n, n_umis):
    n_tx, n_genes, n_cells = 60, 12, 4
    tx_gene = (np.arange(n_tx) // 5).astype(np.int32)
    tx_gene[rng.random(n_tx) < 0.1] = -1
    classes = [()]
    for _ in range(80):
        g = int(rng.integers(n_genes))
        pick = np.flatnonzero(np.arange(n_tx) // 5 == g) if rng.random() < 0.6 else np.arange(n_tx)
        classes.append(tuple(sorted(set(int(t) for t in rng.choice(pick, size=int(rng.integers(1, 5)))))))
    tuples = [classes[int(k)] for k in rng.integers(len(classes), size=n)]
    return rng.integers(-1, n_cells, size=n), rng.integers(0, n_umis, size=n), tuples, tx_gene, n_cells


def test_the_sum_identity_on_random_inputs():
    """per cell: resolved + multi-gene + unnamed + collision = the distinct UMIs among the live molecules, rescued a
    part of resolved, and the matrix adds up to resolved"""
    import umi_reference
    rng = np.random.default_rng(11)
    seen = np.zeros(5, dtype=np.int64)
    for n_umis in (40, 400, 2 ** 32):
        cell, umi, tuples, tx_gene, n_cells = _random_units(rng, 4000, n_umis)
        stay = umi_reference.survivors(cell, umi, tuples)
        indptr, indices, data, tally = mres.matrix(cell, umi, tuples, stay, tx_gene, n_cells)
        distinct = [len({int(m) for c, m, t, keep in zip(cell, umi, tuples, stay) if keep and c == s and t}) for s in range(n_cells)]
        assert tally[:, [0, 2, 3, 4]].sum(axis=1).tolist() == distinct and (tally[:, 1] <= tally[:, 0]).all()
        assert [int(data[indptr[s]:indptr[s + 1]].sum()) for s in range(n_cells)] == tally[:, 0].tolist()
        mref.check_csr(indptr, indices, data, n_cells, 12)
        seen += tally.sum(axis=0)
    assert (seen >= 10).all(), seen


def test_groups_of_one_class_give_the_molecule_matrix_and_the_unit_matrix():
    """UMIs that hardly occur twice: every group has one class, and the three matrices are one"""
    import umi_reference
    rng = np.random.default_rng(12)
    cell, umi, tuples, tx_gene, n_cells = _random_units(rng, 3000, 2 ** 32)
    stay = umi_reference.survivors(cell, umi, tuples)
    assert len(set(zip(cell.tolist(), umi.tolist()))) == 3000
    counted, tally = mres.resolve(cell, umi, tuples, stay, tx_gene)
    assert counted == mol.entries(cell, umi, tuples, stay, tx_gene)[0] == mol.unit_entries(cell, tuples, stay, tx_gene)
    assert len(counted) > 20 and not any(row[1] or row[4] for row in tally.values())
    # and with UMIs that recur, the pattern is the matrix's own
    cell, umi, tuples, tx_gene, n_cells = _random_units(rng, 3000, 40)
    stay = umi_reference.survivors(cell, umi, tuples)
    resolved, counted = set(mres.resolve(cell, umi, tuples, stay, tx_gene)[0]), set(mol.entries(cell, umi, tuples, stay, tx_gene)[0])
    assert counted - resolved, 'a collision removes an entry'


def test_a_rescued_group_makes_an_entry_the_count_matrix_lacks():
    units = [(0, 7, (0, 3)), (0, 7, (1, 7))]
    cell, umi, tuples = zip(*units)
    assert mol.entries(cell, umi, tuples, [True, True], TX_GENE)[0] == {} and _resolve(units)[0] == {(0, 0): 1}


def test_resolve_molecules_refusals_that_need_no_gpu(tmp_path):
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    missing = [pathlib.Path(tmp_path / name) for name in ('no_index.npz', 'no_1.fastq', 'no_2.fastq')]
    base = dict(job_count=1, single_ended=False, bootstrap=0, debug=False, resolve_molecules=True)
    pooled = dict(barcodes=tmp_path / 'no_whitelist.tsv', barcode_file=tmp_path / 'no_barcodes.fastq')
    for keywords in ({}, pooled, dict(pooled, matrix_only=True), dict(discover_cells=10, barcode_length=12, barcode_file=tmp_path / 'b.fastq')):
        with pytest.raises(ValueError) as refused:                    # no --umi-length: pooled or not, before the index is opened
            infer.run_many(missing[0], tmp_path / 'out', missing[1:], **base, **keywords)
        assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS
    assert not (tmp_path / 'out').exists()
    # with UMIs the option passes its own check: what refuses next is the whitelist that does not exist
    with pytest.raises(Exception) as refused:
        infer.run_many(missing[0], tmp_path / 'out', missing[1:], **base, **pooled, umi_length=8, umi_mismatches=1, strand='rf')
    assert str(refused.value) != infer.COUNT_MOLECULES_NEEDS_UMIS and not (tmp_path / 'out').exists()
    # the command line: --resolve-molecules implies --count-molecules and so --count-matrix
    many = ['infer-many', 'index', 'out', 'a_1.fastq', 'a_2.fastq']
    opts = cli.parse_args(many + ['--resolve-molecules', '--gene-map', 'map.tsv', '--barcodes', 'w.tsv', '--barcode-file', 'b.fastq',
                                  '--umi-length', '8'])
    assert opts['resolve_molecules'] and opts['count_molecules'] and opts['count_matrix'] and not opts['matrix_only'] and not opts['genes']
    opts = cli.parse_args(many + ['--count-molecules'])
    assert not opts['resolve_molecules'] and opts['count_molecules']
    with pytest.raises(ValueError) as refused:                        # not pooled, through the command line
        cli.main(many + ['--resolve-molecules'])
    assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS
    for command in (['infer', 'index', 'out', 'a_1.fastq', 'a_2.fastq'], ['impute', 'index', 'out', 'a_1.fastq', 'a_2.fastq']):
        with pytest.raises(SystemExit):
            cli.parse_args(command + ['--resolve-molecules'])


def test_the_writer_of_the_resolved_files(tmp_path):
    from seekmer_amd import infer
    counted = {(0, 3): 2, (0, 70000): 1, (2, 0): 5}
    indptr, indices, data = mref.csr(counted, 3)
    tally = [[3, 1, 2, 0, 4], [0, 0, 0, 7, 0], [5, 5, 0, 0, 0]]
    names = ['cellA', 'cellB', 'cellC']
    infer.output_resolved_matrix(tmp_path, 70001, names, indptr, indices, data, tally)
    assert sorted(f.name for f in (tmp_path / 'counts').iterdir()) == ['molecules.resolved.mtx', 'molecules.resolved.npz', 'molecules.resolved.tsv']
    lines = (tmp_path / 'counts' / 'molecules.resolved.mtx').read_text().splitlines(keepends=True)
    assert lines == mref.mtx_lines(indptr, indices, data, 70001, infer.RESOLVED_MATRIX_COMMENT)
    assert infer.RESOLVED_MATRIX_COMMENT not in (infer.COUNT_MATRIX_COMMENT, infer.MOLECULE_MATRIX_COMMENT)
    assert infer.RESOLVED_MATRIX_COMMENT.startswith('%') and '\n' not in infer.RESOLVED_MATRIX_COMMENT
    arrays = np.load(tmp_path / 'counts' / 'molecules.resolved.npz')
    assert sorted(arrays.files) == ['data', 'format', 'indices', 'indptr', 'shape']
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [3, 70001]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want)
    assert (tmp_path / 'counts' / 'molecules.resolved.tsv').read_text() == (
        'cellA\t9\t3\t1\t2\t0\t4\t2\n' 'cellB\t7\t0\t0\t0\t7\t0\t0\n' 'cellC\t5\t5\t5\t0\t0\t0\t1\n')
    for row in (tmp_path / 'counts' / 'molecules.resolved.tsv').read_text().splitlines():
        words = [int(v) for v in row.split('\t')[1:]]
        assert len(words) == 7 and words[1] + words[3] + words[4] + words[5] == words[0]
    first = (tmp_path / 'counts' / 'molecules.resolved.npz').read_bytes()
    infer.output_resolved_matrix(tmp_path, 70001, names, indptr, indices, data, tally)
    assert (tmp_path / 'counts' / 'molecules.resolved.npz').read_bytes() == first
    with pytest.raises(ValueError):
        infer.output_resolved_matrix(tmp_path, 70001, names, indptr[:-1], indices, data, tally)
    with pytest.raises(ValueError):
        infer.output_resolved_matrix(tmp_path, 70001, names, indptr, indices, data, tally[:2])


def test_the_kernels_use_no_scratch_and_spill_nothing():
    """every kernel of the new unit, from the remarks the build keeps beside the object"""
    remarks = os.path.join(ROOT, 'seekmer_amd', 'csrc', 'build', 'skm_molecule_resolve.remarks')
    if not os.path.exists(remarks):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'seekmer_amd', 'csrc'), 'ARCH=gfx950'])
    text = open(remarks).read()
    kernels = re.split(r'remark: Function Name: ', text)[1:]
    names = [block.split()[0] for block in kernels]
    for wanted in ('resolve_class_slots_kernel', 'resolve_keys_kernel', 'resolve_pairs_kernel', 'resolve_heads_kernel',
                   'molecule_resolve_kernel', 'resolve_other_kernel'):
        assert sum(wanted in name for name in names) == 1, (wanted, names)
    for name, block in zip(names, kernels):
        assert re.search(r'ScratchSize \[bytes/lane\]: 0\b', block), name
        assert re.search(r'VGPRs Spill: 0\b', block) and re.search(r'SGPRs Spill: 0\b', block), name
        assert re.search(r'LDS Size \[bytes/block\]: 0\b', block), name
