"""Distributed molecules without a device ("Distributed molecules"): the refusals and implications
of `infer-many --distribute-molecules`, the writer of the molecules.em.* files fed from the reference's arrays, and
the compiler's resource remarks for the kernels of skm_molecule_em.hip."""
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

import molecule_em_reference as emref
from conftest import ROOT


def test_distribute_molecules_refusals_that_need_no_gpu(tmp_path):
    from seekmer_amd import __main__ as cli
    from seekmer_amd import infer
    missing = [pathlib.Path(tmp_path / name) for name in ('no_index.npz', 'no_1.fastq', 'no_2.fastq')]
    base = dict(job_count=1, single_ended=False, bootstrap=0, debug=False, distribute_molecules=True)
    pooled = dict(barcodes=tmp_path / 'no_whitelist.tsv', barcode_file=tmp_path / 'no_barcodes.fastq')
    for keywords in ({}, pooled, dict(pooled, matrix_only=True), dict(discover_cells=10, barcode_length=12, barcode_file=tmp_path / 'b.fastq')):
        with pytest.raises(ValueError) as refused:                    # no --umi-length: pooled or not, before the index is opened
            infer.run_many(missing[0], tmp_path / 'out', missing[1:], **base, **keywords)
        assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS
    assert not (tmp_path / 'out').exists()
    # with UMIs the option passes its own check, with the options it goes with: what refuses next is the missing whitelist
    for more in (dict(umi_mismatches=1, strand='rf'), dict(matrix_only=True, strand='fr'),
                 dict(discover_cells=10, barcode_length=12, barcodes=None)):
        with pytest.raises(Exception) as refused:
            infer.run_many(missing[0], tmp_path / 'out', missing[1:], **dict(base, **pooled, umi_length=8, **more))
        assert str(refused.value) != infer.COUNT_MOLECULES_NEEDS_UMIS and not (tmp_path / 'out').exists()
    # the command line: --distribute-molecules implies --resolve-molecules, and so --count-molecules and --count-matrix
    many = ['infer-many', 'index', 'out', 'a_1.fastq', 'a_2.fastq']
    opts = cli.parse_args(many + ['--distribute-molecules', '--gene-map', 'map.tsv', '--barcodes', 'w.tsv', '--barcode-file', 'b.fastq',
                                  '--umi-length', '8'])
    assert opts['distribute_molecules'] and opts['resolve_molecules'] and opts['count_molecules'] and opts['count_matrix']
    assert not opts['matrix_only'] and not opts['genes']
    opts = cli.parse_args(many + ['--resolve-molecules'])
    assert not opts['distribute_molecules'] and opts['resolve_molecules']
    with pytest.raises(ValueError) as refused:                        # not pooled, through the command line
        cli.main(many + ['--distribute-molecules'])
    assert str(refused.value) == infer.COUNT_MOLECULES_NEEDS_UMIS
    for command in (['infer', 'index', 'out', 'a_1.fastq', 'a_2.fastq'], ['impute', 'index', 'out', 'a_1.fastq', 'a_2.fastq']):
        with pytest.raises(SystemExit):
            cli.parse_args(command + ['--distribute-molecules'])


def test_the_writer_of_the_em_files(tmp_path):
    from seekmer_amd import infer
    # three cells from the reference: two genes that share two sets, a cell without any molecule, a cell with a sink
    groups = {(0, 1): [frozenset([3])], (0, 2): [frozenset([3, 70000])], (0, 3): [frozenset([3, 70000, 5]), frozenset([70000, 3])],
              (0, 4): [frozenset([70000])], (0, 5): [frozenset([70000])], (0, 6): [frozenset([1]), frozenset([2])],
              (2, 9): [frozenset([0, -1])], (2, 8): [frozenset([-1])], (2, 7): [frozenset(range(20))], (2, 6): [frozenset([0])]}
    indptr, indices, data, tally, to_unnamed = emref.distribute(groups, 3, 70001)
    assert indices.tolist() == [3, 70000, 0] and tally[:, :5].tolist() == [[3, 2, 0, 0, 1], [0] * 5, [1, 1, 1, 1, 0]]
    assert (data != np.round(data)).all() and to_unnamed[2] > 1.0
    names = ['cellA', 'cellB', 'cellC']
    infer.output_distributed_matrix(tmp_path, 70001, names, indptr, indices, data, tally, to_unnamed)
    assert sorted(f.name for f in (tmp_path / 'counts').iterdir()) == ['molecules.em.mtx', 'molecules.em.npz', 'molecules.em.tsv']
    lines = (tmp_path / 'counts' / 'molecules.em.mtx').read_text().splitlines()
    assert lines[:3] == ['%%MatrixMarket matrix coordinate real general', infer.DISTRIBUTED_MATRIX_COMMENT, '70001 3 3']
    assert [line.split()[:2] for line in lines[3:]] == [['4', '1'], ['70001', '1'], ['1', '3']]
    assert [float(line.split()[2]).hex() for line in lines[3:]] == [float(v).hex() for v in data]      # (repr: bit for bit)
    assert [line.split()[2] for line in lines[3:]] == [repr(float(v)) for v in data]
    assert infer.DISTRIBUTED_MATRIX_COMMENT not in (infer.COUNT_MATRIX_COMMENT, infer.MOLECULE_MATRIX_COMMENT, infer.RESOLVED_MATRIX_COMMENT)
    assert infer.DISTRIBUTED_MATRIX_COMMENT.startswith('%') and '\n' not in infer.DISTRIBUTED_MATRIX_COMMENT
    arrays = np.load(tmp_path / 'counts' / 'molecules.em.npz')
    assert sorted(arrays.files) == ['data', 'format', 'indices', 'indptr', 'shape']
    assert arrays['format'].item() == b'csr' and arrays['shape'].tolist() == [3, 70001]
    for name, want in (('indptr', indptr), ('indices', indices), ('data', data)):
        assert arrays[name].dtype == want.dtype and arrays[name].tobytes() == want.tobytes()
    assert arrays['data'].dtype == np.float64
    rows = [line.split('\t') for line in (tmp_path / 'counts' / 'molecules.em.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == names and all(len(row) == 12 for row in rows)
    for s, row in enumerate(rows):
        words = [int(v) for v in row[1:11]]
        assert words[0] == sum(words[1:6]) and words[1:9] == tally[s].tolist() and words[9] == indptr[s + 1] - indptr[s]
        assert words[8] in (0, 1) and float(row[11]).hex() == float(to_unnamed[s]).hex()
    assert rows[1][1:] == ['0'] * 10 + ['0.0']
    first = (tmp_path / 'counts' / 'molecules.em.npz').read_bytes()
    infer.output_distributed_matrix(tmp_path, 70001, names, indptr, indices, data, tally, to_unnamed)
    assert (tmp_path / 'counts' / 'molecules.em.npz').read_bytes() == first
    for change in (dict(indptr=indptr[:-1]), dict(tally=tally[:2]), dict(to_unnamed=to_unnamed[:2]), dict(data=data[:-1])):
        arguments = dict(indptr=indptr, indices=indices, data=data, tally=tally, to_unnamed=to_unnamed)
        arguments.update(change)
        with pytest.raises(ValueError):
            infer.output_distributed_matrix(tmp_path, 70001, names, **arguments)


def test_the_kernels_use_no_scratch_and_the_em_fits_its_lds():
    """every kernel of the new unit, from the remarks the build keeps beside the object"""
    remarks = os.path.join(ROOT, 'seekmer_amd', 'csrc', 'build', 'skm_molecule_em.remarks')
    if not os.path.exists(remarks):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'seekmer_amd', 'csrc'), 'ARCH=gfx950'])
    text = open(remarks).read()
    kernels = re.split(r'remark: Function Name: ', text)[1:]
    names = [block.split()[0] for block in kernels]
    for wanted in ('molecule_sets_single_kernel', 'molecule_sets_kernel', 'gene_sets_sizes_kernel', 'gene_sets_elements_kernel',
                   'gene_rows_heads_kernel', 'gene_rows_kernel', 'gene_rows_transpose_kernel', 'gene_cell_sets_kernel',
                   'gene_em_kernel', 'gene_em_keep_kernel', 'gene_em_entries_kernel', 'gene_em_cells_kernel'):
        assert sum(wanted + 'E' in name for name in names) == 1, wanted
    assert len(kernels) == 12
    for name, block in zip(names, kernels):
        assert re.search(r'ScratchSize \[bytes/lane\]: 0\b', block), name
        assert re.search(r'VGPRs Spill: 0\b', block) and re.search(r'SGPRs Spill: 0\b', block), name
        lds = int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1))
        if 'gene_em_kernelE' in name:
            assert 32768 <= lds < 65536, lds        # x of GENE_EM_LDS_ROWS = 4096 rows, and the verdict's slots
        else:
            assert lds == 0, name
