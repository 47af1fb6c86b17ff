"""Abundance inference -- the `seekmer.infer` surface (reference:
seekmer/infer.py:1-353) over the MI355X engine: `run`, `quantify`, `em`,
`output_results`, `add_subcommand_parser` keep their signatures; the EM loop
and the bootstrap resampling run as HIP kernels behind the C ABI.
"""
import ctypes
import datetime
import io
import json
import logging
import os
import pathlib
import shlex
import sys
import time
import types
import zipfile

import numpy

from . import _native
from . import common
from . import mapper

__all__ = ['run', 'run_many', 'gene_map', 'gene_sums', 'gene_unique_counts', 'gene_table', 'bias_correct', 'bias_pass', 'bias_correct_many', 'bias_pass_many', 'quantify', 'quantify_many', 'quantify_tables', 'quantify_resident', 'em', 'output_results', 'bootstrap_quantify',
           'bootstrap_ranks']

_LOG = logging.getLogger(__name__)

REL_TOL = 0.01          # seekmer/infer.py:160
X_FLOOR = 1e-8          # seekmer/infer.py:160


def run(index_path, output_path, fastq_paths, job_count, save_readmap,
        single_ended, bootstrap, debug, device=0, seed=None, parse_threads=None, strand=None, length_model=None,
        bias=False, genes=False, gene_map=None, **__):
    """The entrypoint of the inference module (seekmer/infer.py:27-85).

    Started as one process per GPU (`python -m torch.distributed.run --nproc-per-node N -m
    seekmer_amd infer ...`; experimental: no multi-GPU node has run it yet) the sample is shared out
    batch by batch: every rank maps its batches on its own GPU against its own replica of the
    index, the EM runs over the rank-local class tables with one RCCL all-reduce per step, rank 0
    merges the ranks' tables on its GPU, the `-b N` replicates are shared out over the ranks again
    (the merged table on every rank, no collective while they run), and rank 0 writes the outputs
    of the whole sample.  A rank that fails ends the job (parallel.Ranks.fail).

    strand: None, 'fr' (--fr-stranded) or 'rf' (--rf-stranded): every rank's mapper keeps only the
    targets that lie in the library's orientation (mapper.MapResult).

    length_model: None, or (mean, sd) of --fragment-length / --sd: the effective lengths come from that
    model (mapper.fragment_length_weights) instead of the observed histogram, on every rank's mapper, so
    whichever rank quantifies holds it.  The histogram is still counted, logged and written.

    bias: --bias, the sequence-bias correction (bias_correct): the mapper also counts the hexamer every aligned
    unit starts with; after the first quantification the effective lengths are rescaled by the hexamer
    weights that follow from the counts and that estimate, and the EM runs once more from it.  One rank only.

    genes / gene_map: --genes / --gene-map FILE (which implies --genes), the gene-level tables (gene_table):
    abundance.genes.tsv, the genes/ datasets of abundance.npz and the gene counts of run_info.json, from the result
    that is written (the corrected one with bias).  The genes are the index's, or those of the two-column file.
    One rank only."""
    from . import parallel
    start_time = datetime.datetime.utcnow()
    ranks = parallel.Ranks.from_env()
    try:
        _run(ranks, start_time, index_path, output_path, fastq_paths, job_count, save_readmap, single_ended,
             bootstrap, debug, device, seed, parse_threads, strand=strand, length_model=length_model, bias=bias,
             genes=genes or gene_map is not None, gene_map_path=gene_map)
    except BaseException as error:          # noqa: B902 -- one rank: re-raised as it is
        ranks.fail(error)
    ranks.close()


def _run(ranks, start_time, index_path, output_path, fastq_paths, job_count, save_readmap, single_ended,
         bootstrap, debug, device, seed, parse_threads, strand=None, length_model=None, bias=False, genes=False,
         gene_map_path=None):
    from . import parallel
    mapper.strand_mode(strand)              # (an unknown mode fails before any file is touched)
    length_model, _ = mapper.length_model_weights(length_model)      # (and so does a model that cannot be)
    if bias and ranks.world > 1:
        raise ValueError(BIAS_ONE_RANK)
    if genes and ranks.world > 1:
        raise ValueError(GENES_ONE_RANK)
    index, gene_names = None, None
    if genes:                               # (an index without genes fails before any read file is opened)
        index = common.KMerIndex.load(index_path)
        gene_names = gene_map(index, gene_map_path)
    if ranks.world > 1:
        device = ranks.local_rank
        if save_readmap:
            raise ValueError('-m/--save-readmap needs the reads of the whole sample in one process: run it on one GPU')
    if ranks.rank == 0:
        try:
            output_path.mkdir(parents=True)
        except FileExistsError:
            _LOG.warning('The output folder exists. Overriding...')
    ranks.barrier()
    readmap = (output_path / 'readmap.txt').open('wt') if save_readmap else None
    _LOG.info('Inferring transcript abundance')
    _log_length_model(length_model, single_ended)
    # (the readers' threads page-lock against THIS GPU; their arena is page-locked by a helper thread
    # from here on, under the index load and upload)
    _native.check(_native.hip().skm_pinned_set_device(device))
    read_feeder = _feeder(fastq_paths, not single_ended, parse_threads, ranks.shard, save_readmap,
                          sum_over_ranks=ranks.sum_int64)
    one_pass = isinstance(read_feeder, common.PackedReadFeeder)
    if one_pass and ranks.world > 1:
        read_feeder.locate_share()          # (a collective: every rank counts its share of the newlines, here)
    # (the one-pass reader maps the text: its page tables are set up by helper threads while the index loads)
    ahead = common.Prefault(fastq_paths if one_pass and ranks.world == 1 else [], threads=4)
    try:
        if index is None:
            index = common.KMerIndex.load(index_path)
        index.device_handle(device)
        _LOG.info('Mapping all reads')
        map_result = mapper.map_reads(index, read_feeder, job_count=job_count,
                                      readmap=readmap, debug=debug, device=device, strand=strand,
                                      length_model=length_model, bias=bias)
    finally:
        ahead.finish()
    _LOG.info('Mapped all reads')
    if bootstrap > 0:
        _check_resample_limit(map_result, ranks)
    comm = parallel.make_comm(ranks, device)
    try:
        summarized_results, main_result = finish(map_result, ranks,
                                                 lambda result: quantify_resident(result, comm=comm), comm=comm)
    finally:
        parallel.destroy_comm(comm)
    if ranks.rank == 0:
        _LOG.info('Estimated fragment length: %.2f', map_result.harmonic_mean_fragment_length)
        _LOG.info('Aligned %d reads (%.2f%%)', summarized_results.aligned,
                  100.0 * summarized_results.aligned / summarized_results.total)
        _LOG.info('Quantified transcripts')
    if bias:
        summarized_results, main_result = bias_pass(index, summarized_results, main_result, map_result.bias_observed(),
                                                    strand, device=device)
    bootstrapped_results = bootstrap_ranks(summarized_results, main_result, bootstrap, ranks, seed=seed, device=device)
    if ranks.rank == 0:
        gene_results = None
        if genes:                           # (one rank: the mapper's table is the sample's, and still in HBM)
            gene_results = gene_names + map_result.gene_unique_counts(gene_names[1], gene_names[0].size)
        output_results(output_path, index, start_time, summarized_results,
                       main_result, bootstrapped_results, genes=gene_results, device=device)
        _LOG.info('Wrote results to %s', output_path)


BIAS_ONE_RANK = ('--bias runs in one process on one GPU: the hexamer counts of several ranks are not merged '
                 '(start it without a launcher)')


GENES_ONE_RANK = ('--genes runs in one process on one GPU: the gene-level pass reads one resident class table '
                  '(start it without a launcher)')
NO_GENES = ('no transcript has a gene: build the index with a GTF annotation, or name the genes with '
            '--gene-map FILE (transcript id, tab, gene id)')


def gene_map(index, path=None):
    """(gene_ids, tx_gene) for the gene-level tables: gene_ids the sorted distinct non-empty gene ids (an S array,
    numpy.unique's order), tx_gene int32[T] the gene number of every transcript of the index, -1 for a transcript
    without a gene.  The genes are index.transcripts['gene_id'] (from the GTF the index was built with) or, with
    `path`, those of a two-column tab-separated file, transcript id then gene id: lines that begin with '#' are
    comments, transcript ids are cut at the first '.' as index_builder.read_transcripts cuts them, a transcript
    the file does not name has no gene, ids the index does not hold are counted and reported in one log line,
    and one transcript given two different genes raises ValueError, as does a map that leaves no transcript with
    a gene (NO_GENES).  The file may be compressed (common.decompress_and_open)."""
    transcript_ids = numpy.asarray(index.transcripts['transcript_id'])
    if path is None:
        genes = numpy.asarray(index.transcripts['gene_id'])
    else:
        rows = {}
        for row, id_ in enumerate(transcript_ids.tolist()):
            rows.setdefault(id_, []).append(row)
        named = [b''] * transcript_ids.size
        unknown = 0
        with common.decompress_and_open(path) as f:
            for number, line in enumerate(f, 1):
                line = line.rstrip(b'\r\n')
                if not line.strip() or line.startswith(b'#'):
                    continue
                fields = line.split(b'\t')
                if len(fields) < 2 or not fields[0].strip() or not fields[1].strip():
                    raise ValueError('%s, line %d: expected a transcript id, a tab and a gene id' % (path, number))
                id_, gene = fields[0].strip().split(b'.')[0], fields[1].strip()
                if id_ not in rows:
                    unknown += 1
                    continue
                for row in rows[id_]:
                    if named[row] not in (b'', gene):
                        raise ValueError('%s, line %d: transcript %s has the genes %s and %s'
                                         % (path, number, id_.decode(), named[row].decode(), gene.decode()))
                    named[row] = gene
        if unknown:
            _LOG.warning('%s names %d transcripts that the index does not hold', path, unknown)
        genes = numpy.asarray(named, dtype='S') if named else numpy.zeros(0, dtype='S1')
    has_gene = genes != b''
    if not has_gene.any():
        raise ValueError(NO_GENES)
    gene_ids = numpy.unique(genes[has_gene])
    tx_gene = numpy.full(genes.size, -1, dtype=numpy.int32)
    tx_gene[has_gene] = numpy.searchsorted(gene_ids, genes[has_gene])
    return gene_ids, tx_gene


_gene_map = gene_map           # (run and run_many take the file's path as `gene_map`, the option's name)


def gene_sums(tx_gene, n_genes, rows, device=0):
    """f8[R, n_genes]: out[r][g] = the sum of rows[r][t] over the transcripts t with tx_gene[t] == g, added in
    ascending t, one after the other, from +0.0 -- numpy.add.at(out[r], tx_gene[named], rows[r][named]) bit for
    bit, on the device (skm_gene_sums).  rows f8[R, T] (one row: f8[T] gives f8[n_genes])."""
    rows = numpy.ascontiguousarray(rows, dtype='f8')
    one = rows.ndim == 1
    if one:
        rows = rows[None, :]
    if rows.ndim != 2:
        raise ValueError('gene_sums takes rows[R, T]')
    tx_gene = mapper.gene_numbers(tx_gene, rows.shape[1])
    n_genes = int(n_genes)
    out = numpy.zeros((rows.shape[0], max(n_genes, 1)), dtype='f8')
    _native.check(_native.hip().skm_gene_sums(
        device, rows.shape[0], rows.shape[1], n_genes, _native.ptr(tx_gene, _native.c_i32p),
        _native.ptr(rows, _native.c_f64p) if rows.size else None, _native.ptr(out, _native.c_f64p)))
    out = out[:, :n_genes]
    return out[0] if one else out


def gene_unique_counts(results, tx_gene, n_genes, device=0):
    """(unique int64[n_genes], other int64[2]) of any SummarizedResult's class table (skm_gene_unique_counts): a
    class whose transcripts all lie in one named gene adds its count to unique[gene]; one whose transcripts are all
    unnamed adds to other[1]; every other class adds to other[0] (ambiguous between genes).  The three add up to
    results.aligned.  MapResult.gene_unique_counts gives the same from the table where it lies in HBM."""
    class_count = numpy.ascontiguousarray(results.class_count, dtype=numpy.int64)
    if getattr(results, 'class_offsets', None) is not None:
        offsets, targets = results.class_offsets, results.class_targets
    else:
        offsets, targets = _csr_from_class_map(results.class_map, class_count.size)
    offsets = numpy.ascontiguousarray(offsets, dtype=numpy.int64)
    targets = numpy.ascontiguousarray(targets, dtype=numpy.int32)
    tx_gene = mapper.gene_numbers(tx_gene, numpy.size(results.effective_lengths))
    n_genes = int(n_genes)
    unique = numpy.zeros(max(n_genes, 1), dtype=numpy.int64)
    other = numpy.zeros(2, dtype=numpy.int64)
    _native.check(_native.hip().skm_gene_unique_counts(
        device, class_count.size, _native.ptr(offsets, _native.c_i64p),
        _native.ptr(targets, _native.c_i32p) if targets.size else None,
        _native.ptr(class_count, _native.c_i64p) if class_count.size else None, None, 1, tx_gene.size, n_genes,
        _native.ptr(tx_gene, _native.c_i32p), _native.ptr(unique, _native.c_i64p), _native.ptr(other, _native.c_i64p)))
    return unique[:n_genes], other


def gene_count_matrix(results_list, tx_gene, n_genes, device=0):
    """(indptr int64[K + 1], indices int32[nnz], data int64[nnz], other int64[K, 2]) for K SummarizedResults over the
    same transcripts: row i of the CSR holds the nonzeros of gene_unique_counts(results_list[i]), genes ascending, and
    other[i] its second value.  The tables are stacked with a sample per class and pass through the device once
    (skm_gene_matrix_from_classes; DESIGN.md section 4, "Count matrix"): no dense row is made."""
    results_list = list(results_list)
    tables = [_table_csr(results) for results in results_list]
    sizes = [counts.size for _, _, counts in tables]
    class_sample = numpy.repeat(numpy.arange(len(tables), dtype=numpy.int32), sizes)
    offsets = numpy.zeros(sum(sizes) + 1, dtype=numpy.int64)
    at, ids = 0, 0
    for (table_offsets, table_targets, counts) in tables:
        offsets[at + 1:at + counts.size + 1] = table_offsets[1:] + ids
        at, ids = at + counts.size, ids + table_targets.size
    targets = numpy.ascontiguousarray(numpy.concatenate([t for _, t, _ in tables] or [numpy.zeros(0, dtype=numpy.int32)]),
                                      dtype=numpy.int32)
    class_count = numpy.ascontiguousarray(numpy.concatenate([c for _, _, c in tables] or [numpy.zeros(0)]), dtype=numpy.int64)
    n_tx = numpy.size(results_list[0].effective_lengths) if results_list else numpy.size(tx_gene)
    tx_gene = mapper.gene_numbers(tx_gene, n_tx)
    handle = ctypes.c_void_p()
    _native.check(_native.hip().skm_gene_matrix_from_classes(
        device, class_count.size, _native.ptr(offsets, _native.c_i64p),
        _native.ptr(targets, _native.c_i32p) if targets.size else None,
        _native.ptr(class_count, _native.c_i64p) if class_count.size else None,
        _native.ptr(class_sample, _native.c_i32p) if class_sample.size else None, len(tables), tx_gene.size, int(n_genes),
        _native.ptr(tx_gene, _native.c_i32p), ctypes.byref(handle)))
    return mapper.read_gene_matrix(handle)


def stack_count_rows(rows):
    """The CSR (indptr, indices, data) of rows given one by one as (indices, data) pairs."""
    rows = list(rows)
    indptr = numpy.zeros(len(rows) + 1, dtype=numpy.int64)
    indptr[1:] = numpy.cumsum([len(indices) for indices, _ in rows])
    indices = numpy.concatenate([numpy.asarray(i, dtype=numpy.int32) for i, _ in rows] or [numpy.zeros(0, dtype=numpy.int32)])
    data = numpy.concatenate([numpy.asarray(d, dtype=numpy.int64) for _, d in rows] or [numpy.zeros(0, dtype=numpy.int64)])
    return indptr, indices.astype(numpy.int32, copy=False), data.astype(numpy.int64, copy=False)


COUNT_MATRIX_COMMENT = ('% infer-many --count-matrix: rows are genes (genes.tsv), columns are cells/samples (cells.tsv); '
                        'a value is the units of the cell that lie inside that one gene')


def output_count_matrix(output_path, gene_ids, names, units, indptr, indices, data, other):
    """output/counts/ of `infer-many --count-matrix`: matrix.mtx (MatrixMarket coordinate integer general; genes as
    rows, samples as columns, 1-based, samples ascending and genes ascending inside a sample), genes.tsv (one gene id
    per line), cells.tsv (per sample: name, units, aligned units, units inside one gene, ambiguous between genes,
    units of unnamed transcripts, genes with a count -- columns 4 to 6 add up to column 3) and matrix.npz (indptr,
    indices, data, shape = (n_samples, n_genes), format = b'csr': the keys scipy.sparse.load_npz reads).
    units int64[n_samples]: every sample's units; (indptr, indices, data) the CSR over samples; other[n_samples, 2]."""
    indptr = numpy.asarray(indptr, dtype=numpy.int64)
    indices = numpy.asarray(indices, dtype=numpy.int32)
    data = numpy.asarray(data, dtype=numpy.int64)
    other = numpy.asarray(other, dtype=numpy.int64).reshape(-1, 2)
    n_samples, n_genes = len(names), len(gene_ids)
    if indptr.shape != (n_samples + 1,) or indices.shape != data.shape or indptr[-1] != data.size or len(other) != n_samples:
        raise ValueError('a count matrix of %d samples needs indptr[%d], as many indices as data, and other[%d, 2]'
                         % (n_samples, n_samples + 1, n_samples))
    counts_path = output_path / 'counts'
    counts_path.mkdir(exist_ok=True)
    sample_of = numpy.repeat(numpy.arange(n_samples, dtype=numpy.int64), numpy.diff(indptr))
    _write_mtx(counts_path / 'matrix.mtx', COUNT_MATRIX_COMMENT, n_genes, n_samples, sample_of, indices, data)
    with (counts_path / 'genes.tsv').open('w') as f:
        f.writelines(gene.decode() + '\n' for gene in numpy.asarray(gene_ids).tolist())
    inside = numpy.zeros(n_samples, dtype=numpy.int64)
    numpy.add.at(inside, sample_of, data)
    with (counts_path / 'cells.tsv').open('w') as f:
        for i, name in enumerate(names):
            aligned = int(inside[i] + other[i, 0] + other[i, 1])
            f.write('%s\t%d\t%d\t%d\t%d\t%d\t%d\n' % (name, units[i], aligned, inside[i], other[i, 0], other[i, 1],
                                                      indptr[i + 1] - indptr[i]))
    _write_csr_npz(counts_path / 'matrix.npz', n_samples, n_genes, indptr, indices, data)


def _write_mtx(path, comment, n_genes, n_samples, sample_of, indices, data):
    """A MatrixMarket coordinate file of a CSR over samples: genes as rows, samples as columns, 1-based, in CSR order."""
    with path.open('w') as f:
        f.write('%%MatrixMarket matrix coordinate integer general\n')
        f.write(comment + '\n')
        f.write('%d %d %d\n' % (n_genes, n_samples, data.size))
        for begin in range(0, data.size, 1 << 16):
            chunk = slice(begin, begin + (1 << 16))
            f.writelines('%d %d %d\n' % entry for entry in zip((indices[chunk].astype(numpy.int64) + 1).tolist(),
                                                               (sample_of[chunk] + 1).tolist(), data[chunk].tolist()))


def _write_csr_npz(path, n_samples, n_genes, indptr, indices, data):
    """The keys scipy.sparse.load_npz reads.  numpy.savez stamps every member with the time of day; this container
    holds the same members without one, so that two runs with the same counts write the same bytes."""
    arrays = {'indptr': indptr, 'indices': indices, 'data': data,
              'shape': numpy.asarray([n_samples, n_genes], dtype=numpy.int64), 'format': numpy.asarray(b'csr')}
    with zipfile.ZipFile(str(path), 'w', zipfile.ZIP_STORED, allowZip64=True) as container:
        for key, array in arrays.items():
            member = io.BytesIO()
            numpy.lib.format.write_array(member, numpy.ascontiguousarray(array), allow_pickle=False)
            container.writestr(zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())


MOLECULE_MATRIX_COMMENT = ('% infer-many --count-molecules: rows are genes (genes.tsv), columns are cells/samples (cells.tsv); '
                           'a value is the distinct UMIs among the units of the cell that lie inside that one gene')
COUNT_MOLECULES_NEEDS_UMIS = ('--count-molecules counts distinct UMIs: it needs --umi-length L, and with it a pooled run '
                              '(--barcodes or --discover-cells)')


def output_molecule_matrix(output_path, n_genes, n_samples, indptr, indices, data):
    """What `infer-many --count-molecules` adds to output/counts/: molecules.mtx (the layout of matrix.mtx, rows and
    columns those of genes.tsv and cells.tsv) and molecules.npz (the keys of matrix.npz).  (indptr, indices, data) is
    the CSR over samples of the molecule counts, with the pattern of the count matrix."""
    indptr = numpy.asarray(indptr, dtype=numpy.int64)
    indices = numpy.asarray(indices, dtype=numpy.int32)
    data = numpy.asarray(data, dtype=numpy.int64)
    if indptr.shape != (n_samples + 1,) or indices.shape != data.shape or indptr[-1] != data.size:
        raise ValueError('a molecule matrix of %d samples needs indptr[%d] and as many indices as data' % (n_samples, n_samples + 1))
    counts_path = output_path / 'counts'
    counts_path.mkdir(exist_ok=True)
    sample_of = numpy.repeat(numpy.arange(n_samples, dtype=numpy.int64), numpy.diff(indptr))
    _write_mtx(counts_path / 'molecules.mtx', MOLECULE_MATRIX_COMMENT, n_genes, n_samples, sample_of, indices, data)
    _write_csr_npz(counts_path / 'molecules.npz', n_samples, n_genes, indptr, indices, data)


RESOLVED_MATRIX_COMMENT = ('% infer-many --resolve-molecules: rows are genes (genes.tsv), columns are cells/samples (cells.tsv); '
                           'a value is the UMIs of the cell whose classes\' gene sets intersect in that one gene')
RESOLVED_TALLY = ('resolved', 'rescued', 'multi-gene', 'unnamed', 'collisions')


def output_resolved_matrix(output_path, n_genes, names, indptr, indices, data, tally):
    """What `infer-many --resolve-molecules` adds to output/counts/: molecules.resolved.mtx (the layout of matrix.mtx
    under a comment line of its own, rows and columns those of genes.tsv and cells.tsv), molecules.resolved.npz (the
    keys of matrix.npz) and molecules.resolved.tsv -- per sample: name, distinct UMIs, resolved, rescued, multi-gene,
    unnamed, collisions, genes with a count; columns 3 + 5 + 6 + 7 add up to column 2, rescued is a part of resolved.
    (indptr, indices, data) is the CSR over samples of the resolved molecules, a pattern of its own;
    tally[n_samples, 5] in the order of RESOLVED_TALLY."""
    indptr = numpy.asarray(indptr, dtype=numpy.int64)
    indices = numpy.asarray(indices, dtype=numpy.int32)
    data = numpy.asarray(data, dtype=numpy.int64)
    tally = numpy.asarray(tally, dtype=numpy.int64).reshape(-1, len(RESOLVED_TALLY))
    n_samples = len(names)
    if indptr.shape != (n_samples + 1,) or indices.shape != data.shape or indptr[-1] != data.size or len(tally) != n_samples:
        raise ValueError('a resolved matrix of %d samples needs indptr[%d], as many indices as data, and tally[%d, %d]'
                         % (n_samples, n_samples + 1, n_samples, len(RESOLVED_TALLY)))
    counts_path = output_path / 'counts'
    counts_path.mkdir(exist_ok=True)
    sample_of = numpy.repeat(numpy.arange(n_samples, dtype=numpy.int64), numpy.diff(indptr))
    _write_mtx(counts_path / 'molecules.resolved.mtx', RESOLVED_MATRIX_COMMENT, n_genes, n_samples, sample_of, indices, data)
    _write_csr_npz(counts_path / 'molecules.resolved.npz', n_samples, n_genes, indptr, indices, data)
    with (counts_path / 'molecules.resolved.tsv').open('w') as f:
        for i, name in enumerate(names):
            resolved, rescued, multi, unnamed, collisions = (int(v) for v in tally[i])
            f.write('%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n' % (name, resolved + multi + unnamed + collisions, resolved, rescued,
                                                          multi, unnamed, collisions, indptr[i + 1] - indptr[i]))


DISTRIBUTED_MATRIX_COMMENT = ('% infer-many --distribute-molecules: rows are genes (genes.tsv), columns are cells/samples (cells.tsv); '
                              'a value is the cell\'s UMIs inside that gene plus its share of the multi-gene UMIs, in molecules')
DISTRIBUTED_TALLY = ('resolved', 'distributed', 'wide', 'unnamed', 'collisions', 'rows', 'steps', 'capped')


def output_distributed_matrix(output_path, n_genes, names, indptr, indices, data, tally, to_unnamed):
    """What `infer-many --distribute-molecules` adds to output/counts/: molecules.em.mtx (a real MatrixMarket file in the
    layout and order of matrix.mtx under a comment line of its own, every value written with repr(float): the double
    comes back bit for bit), molecules.em.npz (the keys of matrix.npz, data as float64) and molecules.em.tsv -- per
    sample: name, distinct UMIs, resolved, distributed, wide, unnamed, collisions, rows and steps of its EM, capped 0/1,
    genes with a weight, to_unnamed (what the EM gave to "no gene"); columns 3 to 7 add up to column 2.
    (indptr, indices, data) is the CSR over samples of SampleSet.gene_distributed_matrix; tally[n_samples, 8] in the
    order of DISTRIBUTED_TALLY."""
    indptr = numpy.asarray(indptr, dtype=numpy.int64)
    indices = numpy.asarray(indices, dtype=numpy.int32)
    data = numpy.asarray(data, dtype=numpy.float64)
    tally = numpy.asarray(tally, dtype=numpy.int64).reshape(-1, len(DISTRIBUTED_TALLY))
    to_unnamed = numpy.asarray(to_unnamed, dtype=numpy.float64).reshape(-1)
    n_samples = len(names)
    if (indptr.shape != (n_samples + 1,) or indices.shape != data.shape or indptr[-1] != data.size or len(tally) != n_samples
            or len(to_unnamed) != n_samples):
        raise ValueError('a distributed matrix of %d samples needs indptr[%d], as many indices as data, tally[%d, %d] and '
                         'to_unnamed[%d]' % (n_samples, n_samples + 1, n_samples, len(DISTRIBUTED_TALLY), n_samples))
    counts_path = output_path / 'counts'
    counts_path.mkdir(exist_ok=True)
    sample_of = numpy.repeat(numpy.arange(n_samples, dtype=numpy.int64), numpy.diff(indptr))
    with (counts_path / 'molecules.em.mtx').open('w') as f:
        f.write('%%MatrixMarket matrix coordinate real general\n')
        f.write(DISTRIBUTED_MATRIX_COMMENT + '\n')
        f.write('%d %d %d\n' % (n_genes, n_samples, data.size))
        for begin in range(0, data.size, 1 << 16):
            chunk = slice(begin, begin + (1 << 16))
            f.writelines('%d %d %r\n' % entry for entry in zip((indices[chunk].astype(numpy.int64) + 1).tolist(),
                                                               (sample_of[chunk] + 1).tolist(), data[chunk].tolist()))
    _write_csr_npz(counts_path / 'molecules.em.npz', n_samples, n_genes, indptr, indices, data)
    with (counts_path / 'molecules.em.tsv').open('w') as f:
        for i, name in enumerate(names):
            words = [int(v) for v in tally[i]]
            f.write('%s\t%d\t%s\t%d\t%r\n' % (name, sum(words[:5]), '\t'.join('%d' % v for v in words),
                                               indptr[i + 1] - indptr[i], float(to_unnamed[i])))


MATRIX_ONLY_NEEDS_EM = ('--matrix-only stops before the EM: %s needs the EM (take --count-matrix, which writes the '
                        'count matrix beside the full run)')


GENE_COLUMNS =('gene_id', 'n_transcripts', 'length', 'eff_length', 'est_count', 'tpm', 'unique_count')


def gene_table(index, gene_ids, tx_gene, results, tpm, est_counts, unique, device=0):
    """The columns of abundance.genes.tsv (GENE_COLUMNS) as a dict of arrays, one entry per gene of gene_ids, over
    the gene's transcripts: tpm = sum of tpm; est_count = sum of est_count; length = sum of tpm x length / sum of
    tpm where the gene has any tpm, otherwise the plain mean of its transcripts' lengths; eff_length the same from
    the effective lengths; n_transcripts; unique_count = `unique` (gene_unique_counts).  The products are formed in
    numpy; the sums are ONE gene_sums call with four rows (the plain means of the genes without tpm are numpy's,
    in the same order).  Transcripts without a gene appear nowhere."""
    tx_gene = numpy.asarray(tx_gene, dtype=numpy.int32)
    n_genes = len(gene_ids)
    tpm = numpy.asarray(tpm, dtype='f8')
    length = numpy.asarray(index.transcripts['length'], dtype='f8')
    effective = numpy.asarray(results.effective_lengths, dtype='f8')
    sums = gene_sums(tx_gene, n_genes, numpy.stack([tpm, numpy.asarray(est_counts, dtype='f8'), tpm * length,
                                                    tpm * effective]), device=device)
    named = tx_gene >= 0
    n_transcripts = numpy.bincount(tx_gene[named], minlength=n_genes).astype(numpy.int64)
    columns = {'gene_id': numpy.asarray(gene_ids), 'n_transcripts': n_transcripts, 'est_count': sums[1], 'tpm': sums[0],
               'unique_count': numpy.asarray(unique, dtype=numpy.int64)}
    expressed = sums[0] > 0
    for name, values, weighted in (('length', length, sums[2]), ('eff_length', effective, sums[3])):
        plain = numpy.zeros(n_genes, dtype='f8')
        numpy.add.at(plain, tx_gene[named], values[named])
        columns[name] = numpy.where(expressed, weighted / numpy.where(expressed, sums[0], 1.0),
                                    plain / numpy.maximum(n_transcripts, 1))
    return columns


def bias_correct(index, summarized, tpm, observed, strand, device=0):
    """The sequence-bias correction of the effective lengths ("Sequence bias";
    skm_bias_correct): (eff', b, E) from the summary's effective lengths, the first pass's TPM, the observed
    hexamer counts int64[4096] (MapResult.bias_observed) and the strand mode (None, 'fr', 'rf').  b f8[4096] are
    the hexamer weights, E f8[4096] the expected counts.  The transcripts' sequences are rebuilt on the device
    from the index, once per index handle (skm_index_build_transcripts)."""
    mode = mapper.strand_mode(strand)
    handle = index.device_handle(device)
    lengths = numpy.ascontiguousarray(index.transcripts['length'], dtype='f8')
    tpm = numpy.ascontiguousarray(tpm, dtype='f8')
    eff = numpy.ascontiguousarray(summarized.effective_lengths, dtype='f8')
    observed = numpy.ascontiguousarray(observed, dtype=numpy.int64)
    if observed.shape != (4096,) or tpm.shape != lengths.shape or eff.shape != lengths.shape:
        raise ValueError('bias_correct takes observed[4096] and one abundance and one effective length per transcript')
    _native.check(_native.hip().skm_index_build_transcripts(handle, _native.ptr(lengths, _native.c_f64p), lengths.size))
    corrected = numpy.zeros(lengths.size, dtype='f8')
    weights = numpy.zeros(4096, dtype='f8')
    expected = numpy.zeros(4096, dtype='f8')
    _native.check(_native.hip().skm_bias_correct(
        handle, mode, _native.ptr(observed, _native.c_i64p), _native.ptr(tpm, _native.c_f64p), _native.ptr(eff, _native.c_f64p),
        lengths.size, _native.ptr(expected, _native.c_f64p), _native.ptr(weights, _native.c_f64p),
        _native.ptr(corrected, _native.c_f64p)))
    return corrected, weights, expected


def bias_pass(index, summarized, tpm, observed, strand, device=0):
    """The second pass of --bias: (summary with eff', the observed counts and the weights; corrected TPM).  The EM
    is the one of the first pass (quantify), with l = eff' and started from the first result; the bootstraps
    of the caller then start from the corrected result and use eff', as they read both from what is returned."""
    corrected, weights, _ = bias_correct(index, summarized, tpm, observed, strand, device=device)
    _LOG.info('Sequence bias: %d observed hexamers, weights from %g to %g', int(observed.sum()), weights.min(), weights.max())
    summary = mapper.SummarizedResult(
        summarized.aligned, summarized.unaligned, summarized.total, summarized.class_map, summarized.class_count,
        summarized.fragment_length_frequencies, corrected, class_offsets=summarized.class_offsets,
        class_targets=summarized.class_targets, length_model=summarized.length_model, bias_observed=observed,
        bias_weights=weights)
    return summary, quantify(summary, x0=numpy.asarray(tpm, dtype='f8'), device=device)


def bias_correct_many(index, summaries, tpms, observed, strand, device=0):
    """bias_correct for S samples in one device call (skm_bias_correct_many): (eff'[S, n_tx], b[S, 4096], E[S, 4096])
    from the summaries' effective lengths, the first pass's TPM rows [S, n_tx] and the observed counts int64[S, 4096]
    (SampleSet.bias_observed).  Row s is bit for bit bias_correct on sample s.  Shapes that do not fit raise
    ValueError before the device is touched."""
    mode = mapper.strand_mode(strand)
    summaries = list(summaries)
    n = len(summaries)
    lengths = numpy.ascontiguousarray(index.transcripts['length'], dtype='f8')
    if any(numpy.shape(summary.effective_lengths) != lengths.shape for summary in summaries):
        raise ValueError('bias_correct_many takes one effective length per transcript from every summary')
    tpms = numpy.ascontiguousarray(tpms, dtype='f8').reshape(-1, lengths.size) if n == 0 else numpy.ascontiguousarray(tpms, dtype='f8')
    observed = numpy.ascontiguousarray(observed, dtype=numpy.int64).reshape(-1, 4096) if n == 0 \
        else numpy.ascontiguousarray(observed, dtype=numpy.int64)
    if observed.shape != (n, 4096) or tpms.shape != (n, lengths.size):
        raise ValueError('bias_correct_many takes observed[S, 4096] and tpms[S, n_tx] for its S = %d summaries, not %s and %s'
                         % (n, observed.shape, tpms.shape))
    eff = numpy.zeros((n, lengths.size), dtype='f8')
    for k, summary in enumerate(summaries):
        eff[k] = summary.effective_lengths
    handle = index.device_handle(device)
    _native.check(_native.hip().skm_index_build_transcripts(handle, _native.ptr(lengths, _native.c_f64p), lengths.size))
    corrected = numpy.zeros((n, lengths.size), dtype='f8')
    weights = numpy.zeros((n, 4096), dtype='f8')
    expected = numpy.zeros((n, 4096), dtype='f8')
    if n:
        _native.check(_native.hip().skm_bias_correct_many(
            handle, mode, n, _native.ptr(observed, _native.c_i64p), _native.ptr(tpms, _native.c_f64p),
            _native.ptr(eff, _native.c_f64p), lengths.size, _native.ptr(expected, _native.c_f64p),
            _native.ptr(weights, _native.c_f64p), _native.ptr(corrected, _native.c_f64p)))
    return corrected, weights, expected


def bias_pass_many(index, summaries, tpms, observed, strand, device=0):
    """bias_pass for S samples: ([summary with eff', O and b, ...], corrected TPM [S, n_tx]), row k bit for bit
    bias_pass on sample k.  The correction is one device call (bias_correct_many).  Inside the regime of
    impute.use_set_quant the second EM of all samples runs in shared launches (quantify_tables started from the
    first results); outside it, or under SKM_SET_QUANT_SERIAL=1, sample by sample."""
    from . import impute
    summaries = list(summaries)
    tpms = numpy.ascontiguousarray(tpms, dtype='f8')
    observed = numpy.ascontiguousarray(observed, dtype=numpy.int64)
    corrected, weights, _ = bias_correct_many(index, summaries, tpms, observed, strand, device=device)
    passed = []
    for k, summarized in enumerate(summaries):
        _LOG.info('Sequence bias: %d observed hexamers, weights from %g to %g', int(observed[k].sum()), weights[k].min(),
                  weights[k].max())
        passed.append(mapper.SummarizedResult(
            summarized.aligned, summarized.unaligned, summarized.total, summarized.class_map, summarized.class_count,
            summarized.fragment_length_frequencies, corrected[k], class_offsets=summarized.class_offsets,
            class_targets=summarized.class_targets, length_model=summarized.length_model, bias_observed=observed[k],
            bias_weights=weights[k]))
    n_tx = index.transcripts.size
    if passed and impute.use_set_quant(len(passed), n_tx, sum(summary.class_count.size for summary in passed)):
        second = quantify_tables(passed, device=device, x0s=tpms)
    else:
        second = numpy.zeros((len(passed), n_tx), dtype='f8')
        for k, summary in enumerate(passed):
            second[k] = quantify(summary, x0=tpms[k], device=device)
    return passed, second


def _log_length_model(length_model, single_ended):
    if length_model is None:
        return
    _LOG.info('Effective lengths from the fragment-length model: mean %g, sd %g', *length_model)
    if not single_ended:
        _LOG.info('The model overrides the observed fragment-length histogram of the paired reads')


def sample_groups(fastq_paths, single_ended):
    """The samples of infer-many: every two files are one (with single_ended every file), impute's convention --
    but a file left over (an odd number of files for paired samples) raises ValueError: every file named must
    end up in a sample's folder."""
    width = 1 if single_ended else 2
    if len(fastq_paths) % width:
        raise ValueError('%d files for paired samples: every two files are one sample (use -s for single-ended reads)'
                         % len(fastq_paths))
    return [tuple(fastq_paths[i:i + width]) for i in range(0, len(fastq_paths), width)]


def sample_names(groups, names=None):
    """One name per sample: its first file's name up to the first '.', or the matching entry of `names`
    (a list, or one string with commas).  A list of the wrong length and names that are not unique (or
    cannot name a folder) raise ValueError; no file is looked at."""
    if names is None:
        names = [pathlib.Path(group[0]).name.split('.')[0] for group in groups]
    else:
        names = names.split(',') if isinstance(names, str) else [str(name) for name in names]
        if len(names) != len(groups):
            raise ValueError('%d names for %d samples' % (len(names), len(groups)))
    for name in names:
        if name in ('', '.', '..') or '/' in name:
            raise ValueError('%r cannot name a sample\'s output folder' % (name,))
    repeated = sorted({name for name in names if names.count(name) > 1})
    if repeated:
        raise ValueError('sample names are not unique: %s (name them with --names)' % ', '.join(repeated))
    return names


def sample_set_members(sizes, max_bytes, per_sample=None):
    """The routing rule of run_many as a function of the samples' text sizes (impute.cell_text_bytes):
    the indices of the samples that go through one sample set -- those of at most `max_bytes`, when
    there are at least two of them; every other sample is mapped by itself.  per_sample: the
    switch SKM_INFER_MANY_PER_SAMPLE=1 (None = looked up in the environment now)."""
    if per_sample is None:
        per_sample = os.environ.get('SKM_INFER_MANY_PER_SAMPLE') == '1'
    small = [i for i, size in enumerate(sizes) if size <= max_bytes]
    return small if len(small) >= 2 and not per_sample else []


def run_many(index_path, output_path, fastq_paths, job_count, single_ended, bootstrap, debug, device=0, seed=None,
             strand=None, names=None, length_model=None, bias=False, genes=False, gene_map=None, barcodes=None,
             barcode_file=None, barcode_start=0, barcode_mismatches=1, min_units=1, umi_start=0, umi_length=0,
             discover_cells=None, barcode_length=None, discover_keep_neighbours=False, umi_mismatches=0,
             count_matrix=False, matrix_only=False, count_molecules=False, resolve_molecules=False,
             distribute_molecules=False, **__):
    """`infer-many`: run() for many samples against ONE resident index.  output/<name>/ holds exactly
    the files `infer` writes for that sample alone (same bits but for the start time and the call), and
    output/samples.tsv one line per sample: name, units, aligned units, harmonic mean fragment length.

    Small samples (impute.SAMPLE_SET_MAX_CELL_BYTES of text at most, two of them at least) share
    launches in one mapper.SampleSet that keeps a fragment-length histogram per sample; every other
    sample is mapped by itself on the same index handle.  SKM_INFER_MANY_PER_SAMPLE=1 maps every
    sample by itself.  `seed` is used for every sample, so a sample's `-b N` replicates are those of
    `infer -b N --seed S` on it.  One process, one GPU; no readmap (a set has none).

    Inside the regime of impute.use_set_quant the main estimates of the samples that went through the set
    come from SampleSet.quantify() -- shared EM launches on the set's resident table, the bits of the loop;
    SKM_SET_QUANT_SERIAL=1 keeps quantify() sample by sample.  `-b N` stays per sample.  SKM_TRACE_INFER
    prints the host wall time per phase on stderr.

    length_model: None or (mean, sd), as run(): every sample's effective lengths come from the model, in the
    set and for the samples mapped by themselves; samples.tsv keeps the observed harmonic means.

    bias: --bias, as run().  The samples that go through the set are mapped in a set that also counts every
    sample's first hexamers (SampleSet(bias=True)) and get the second pass together, before the bootstraps and the
    writing (bias_pass_many: one correction call, and inside the regime of impute.use_set_quant one shared second
    EM); every other sample, and every sample under SKM_INFER_MANY_PER_SAMPLE=1, counts in a mapper of its own and
    gets bias_pass.  The files are the same either way.

    genes / gene_map: --genes / --gene-map, as run(): every folder gets what `infer --genes` writes for the sample,
    and output/genes.tpm.tsv and output/genes.unique_counts.tsv hold genes as rows and samples as columns.  The
    samples of the set get their gene-unique counts from ONE pass over the set's resident table
    (SampleSet.gene_unique_counts), every other sample from its mapper's (MapResult.gene_unique_counts); the TPM
    rows of all samples are summed per gene in one gene_sums call.  The files are the same either way.

    barcodes: --barcodes WHITELIST.  The FASTQ files are then ONE pooled sample (one file with single_ended, two
    otherwise) and `barcode_file` holds one barcode read per unit; the samples are the whitelist's cells with at
    least `min_units` assigned units, named by the whitelist (mapper.map_barcoded: the barcodes are matched and the
    units grouped on the GPU, bases [barcode_start, barcode_start + L) of a barcode read with at most
    `barcode_mismatches` (0 or 1) substitutions).  All cells go through one sample set; every folder holds what
    it would for a FASTQ pair of the cell's reads alone.  output/barcodes.tsv lists every whitelist entry
    (barcode, name, assigned units, kept 0/1) and output/barcodes.json the demultiplexing summary.  Plain FASTQ
    files only; `names` is refused.

    umi_length: --umi-length L (1..16, with barcodes only).  The UMI of a unit is bases [umi_start, umi_start + L) of
    its barcode read; a unit without a readable one belongs to no cell, and inside a cell every unit whose UMI and
    class an earlier unit has shown is removed on the GPU as if it had never been in the files (mapper.SampleSet with
    umi_bases; DESIGN.md section 4, "UMI collapse").  Every folder then holds what it would for a FASTQ pair of the
    cell's surviving units; barcodes.tsv gains two columns (units with a readable UMI, units left after collapse) and
    barcodes.json the keys umi_start, umi_length, umi_unreadable, umi_duplicates.

    umi_mismatches: --umi-mismatches 0 or 1 (1 with umi_length only).  0, the default, collapses UMIs that are equal
    letter for letter.  With 1 a unit is also removed when an EARLIER unit of its cell has the same class and a UMI
    one substitution away, whether or not that earlier unit stayed ("UMI mismatches": an
    arrival-ordered rule, neither Cell Ranger's nor UMI-tools' "directional" one).  barcodes.json then gains
    "umi_mismatches": 1 and "umi_near_duplicates" (the units that only a neighbour removed; umi_duplicates stays the
    total), and the last column of barcodes.tsv counts what is left after both kinds of removal.

    discover_cells: --discover-cells N with barcode_length L (1..32), instead of barcodes: there is no whitelist, the
    cells are found in the barcode reads (mapper.discover_barcodes; DESIGN.md section 4, "Cell discovery": an exact
    count of every distinct clean window on the GPU, a tenth of the count at rank ceil(N / 100) as threshold, and --
    unless discover_keep_neighbours -- no candidate one substitution away from an earlier one).  The picked barcodes
    go to output/barcodes.discovered.txt, a valid whitelist, every candidate to output/barcodes.census.tsv (barcode,
    count, picked 0/1), and barcodes.json gains the key "discovery".  From there the run is `barcodes` on that list,
    which reads the barcode file a second time.

    count_matrix: --count-matrix.  output/counts/ then holds the sparse gene x cell count matrix (output_count_matrix:
    matrix.mtx, genes.tsv, cells.tsv, matrix.npz) of the units that lie inside one gene -- the numbers of
    genes.unique_counts.tsv without its zeros.  It needs genes as `genes` does, from the index or from `gene_map`
    (NO_GENES before any read file is opened), but does not switch the gene-level tables on: with it, `gene_map`
    alone no longer implies `genes`.  The samples of the set get their rows from ONE SampleSet.gene_count_matrix call
    on the resident table ("Count matrix"), every other sample from the nonzeros of its mapper's
    MapResult.gene_unique_counts; the files are the same either way, and every other file of the run is what it is
    without the option.

    matrix_only: --matrix-only, which implies count_matrix.  The run stops after mapping (and demultiplexing and UMI
    collapse): no summarize(), no EM, no folder per sample; it writes counts/, samples.tsv and the barcodes.* files,
    each byte for byte that of the full run.  bootstrap, bias and genes need the EM and are refused here, before the
    index is loaded (MATRIX_ONLY_NEEDS_EM).

    count_molecules: --count-molecules, which implies count_matrix and needs umi_length, hence a pooled run
    (COUNT_MOLECULES_NEEDS_UMIS before the index is loaded).  counts/ gains molecules.mtx and molecules.npz: entry
    (gene, cell) is the number of DISTINCT UMIs among the cell's surviving units whose class lies inside the gene,
    UMIs compared letter for letter (SampleSet.gene_molecule_matrix: one pass over the molecule set and the class
    table where they lie; DESIGN.md section 4, "Molecule matrix") -- matrix.mtx counts such a molecule once per class
    its reads fell into.  Same rows, columns and pattern as matrix.mtx; every other file of the run is what it is
    without the option.  Goes with matrix_only, umi_mismatches and strand.

    resolve_molecules: --resolve-molecules, which implies count_molecules (and so count_matrix, with its refusal
    without umi_length).  counts/ gains molecules.resolved.mtx, molecules.resolved.npz and molecules.resolved.tsv
    (output_resolved_matrix): the classes among a cell's live molecules with one UMI form a group, and the
    intersection of their gene sets names the group's gene -- or makes it multi-gene, unnamed or a collision, which are
    tallied only (SampleSet.gene_resolved_matrix; DESIGN.md section 4, "Resolved molecules").  The matrix has a
    pattern of its own; every other file of the run, molecules.mtx among them, is what it is without the option.

    distribute_molecules: --distribute-molecules, which implies resolve_molecules (and so the refusal without
    umi_length).  counts/ gains molecules.em.mtx, molecules.em.npz and molecules.em.tsv (output_distributed_matrix): the
    groups that resolve_molecules tallies as multi-gene are shared out among the genes of their intersection, 16 at
    most, by a small EM per cell (SampleSet.gene_distributed_matrix; DESIGN.md section 4, "Distributed molecules");
    values are doubles, in molecules.  Every other file of the run is what it is without the option.  Parity with
    alevin or bustools is not claimed."""
    # what the phases below share: every option under its own name (locals(): this stays the first statement, so that a
    # new option needs no second list), and with them the index, the genes and the trace's clock
    job = types.SimpleNamespace(**locals(), paired=not single_ended, pooled=barcodes is not None or discover_cells is not None,
                                index=None, gene_names=None, start_time=datetime.datetime.utcnow(), trace=_phase_trace())
    from . import impute
    from . import parallel
    groups, names, whitelist = _check_many_options(job, names)
    ranks = parallel.Ranks.from_env()
    if ranks.world > 1:
        ranks.close()
        raise ValueError('infer-many runs in one process on one GPU: start it without a launcher')
    _open_run(job, len(groups), whitelist)
    _native.check(_native.hip().skm_pinned_set_device(device))
    job.index = common.KMerIndex.load(index_path)
    job.genes = genes or (gene_map is not None and not job.count_matrix)
    if job.genes or job.count_matrix:       # (fails before any read file is opened)
        job.gene_names = _gene_map(job.index, gene_map)
    job.index.device_handle(device)
    if not job.pooled:                      # the records are made once: here, or by _map_pooled when the cells are known
        sizes = [impute.cell_text_bytes(group) for group in groups]
        in_set = set(sample_set_members(sizes, impute.SAMPLE_SET_MAX_CELL_BYTES))
        samples = [_Sample(name, group, i in in_set) for i, (name, group) in enumerate(zip(names, groups))]
    job.trace('index load')
    if job.pooled:
        sample_set, samples = _map_pooled(job, whitelist)
    else:
        sample_set = _map_set(job, [sample for sample in samples if sample.in_set])
    if sample_set is not None:
        _take_from_set(job, sample_set, [sample for sample in samples if sample.in_set])
        del sample_set                      # (the set ends here, before any sample gets a mapper of its own)
    for sample in samples:
        if not sample.in_set:
            _map_alone(job, sample)         # (the sample's MapResult ends in there, before the next is made)
    _LOG.info('Mapped all reads')
    job.trace('mapping (one by one)')
    _finish(job, samples)


class _Sample:
    """What run_many keeps of one sample -- a file group, or a cell of a pooled run -- from the mapping to the files:
    name (the folder's) and group (its FASTQ files; () for a cell); in_set, mapped through the sample set and not by a
    mapper of its own; summary (SummarizedResult) or, with matrix_only, sizes (the sizes() row of its table); mean, the
    observed harmonic mean fragment length; observed, its hexamer counts (bias); gene_counts, (unique, other) of
    gene_unique_counts (genes); matrix_row, (gene indices, counts) of the count matrix, and the matrix_other pair that
    goes with it; molecule_row, the molecule matrix's counts for the genes of matrix_row (count_molecules);
    resolved_row, (gene indices, counts) of the resolved matrix, and the resolved_tally that goes with it (resolve_molecules);
    distributed_row, (gene indices, weights) of the distributed matrix, with its distributed_tally and to_unnamed
    (distribute_molecules);
    set_estimate, the first-pass TPM where the set or the shared bias pass made one; corrected, (summary, TPM) of the
    set's shared bias pass; estimate, the TPM it was written with.  What was not made is None.  Host values only: a
    record never holds the SampleSet or a MapResult, whose device memory ends where run_many says."""
    __slots__ = ('name', 'group', 'in_set', 'summary', 'sizes', 'mean', 'observed', 'gene_counts', 'matrix_row',
                 'matrix_other', 'molecule_row', 'resolved_row', 'resolved_tally', 'distributed_row', 'distributed_tally', 'to_unnamed',
                 'set_estimate', 'corrected', 'estimate')

    def __init__(self, name, group, in_set):
        self.name, self.group, self.in_set = name, group, in_set
        for field in self.__slots__[3:]:
            setattr(self, field, None)

    def units(self):
        """(units, aligned units): the summary's, or without one (matrix_only) from the count-matrix row, `other`
        and the sizes row -- units = unaligned + the units of the classes, which row and `other` hold between them."""
        if self.summary is not None:
            return self.summary.total, self.summary.aligned
        aligned = int(self.matrix_row[1].sum() + self.matrix_other.sum())
        return aligned + int(self.sizes[2]), aligned


def _check_many_options(job, names):
    """run_many's checks that need no file and no GPU, in the order in which they refuse.  Settles job.length_model,
    job.umi_mismatches and job.count_matrix and returns the plan (groups, names, whitelist): the samples' file groups
    and names with whitelist None -- or, for a pooled run, its one group, names None and the whitelist of
    barcode_options (None: the cells are to be discovered)."""
    mapper.strand_mode(job.strand)
    job.length_model, _ = mapper.length_model_weights(job.length_model)
    job.umi_mismatches = mapper.check_umi_mismatches(job.umi_mismatches, job.umi_length)
    job.resolve_molecules = bool(job.resolve_molecules) or bool(job.distribute_molecules)
    job.count_molecules = bool(job.count_molecules) or bool(job.resolve_molecules)
    job.count_matrix = bool(job.count_matrix) or bool(job.matrix_only) or bool(job.count_molecules)
    if job.count_molecules and not (job.umi_length and job.pooled):
        raise ValueError(COUNT_MOLECULES_NEEDS_UMIS)
    if job.matrix_only:
        for given, flag in ((job.bootstrap and job.bootstrap > 0, '-b N'), (job.bias, '--bias'), (job.genes, '--genes')):
            if given:
                raise ValueError(MATRIX_ONLY_NEEDS_EM % flag)
    if job.pooled:
        whitelist = barcode_options(job.fastq_paths, job.single_ended, names, job.barcodes, job.barcode_file,
                                    job.barcode_start, job.barcode_mismatches, job.min_units, job.umi_start,
                                    job.umi_length, discover_cells=job.discover_cells, barcode_length=job.barcode_length,
                                    discover_keep_neighbours=job.discover_keep_neighbours)
        return [tuple(job.fastq_paths)], None, whitelist
    if job.barcode_file is not None:
        raise ValueError('--barcode-file goes with --barcodes')
    if job.umi_length or job.umi_start:
        raise ValueError('--umi-length and --umi-start go with --barcodes')
    if job.barcode_length is not None:
        raise ValueError('--barcode-length goes with --discover-cells')
    if job.discover_keep_neighbours:
        raise ValueError('--discover-keep-neighbours goes with --discover-cells')
    groups = sample_groups(job.fastq_paths, job.single_ended)
    if not groups:
        raise ValueError('no samples: infer-many takes %s' % ('a file per sample' if job.single_ended else 'two files per sample'))
    return groups, sample_names(groups, names), None


def _open_run(job, n_samples, whitelist):
    """The last checks before the GPU is touched -- every read file exists, and a pooled run's are plain FASTQ --,
    then the output folder and the log lines that say what the run is."""
    for path in list(job.fastq_paths) + ([job.barcode_file] if job.pooled else []):
        if not pathlib.Path(path).exists():
            raise ValueError(f'invalid FastQ file: {path}')
        if job.pooled and not common.PackedReadFeeder.eligible([path]):
            raise ValueError('%s reads plain FASTQ files: decompress %s first'
                             % ('--barcodes' if job.barcodes is not None else '--discover-cells', path))
    try:
        job.output_path.mkdir(parents=True)
    except FileExistsError:
        _LOG.warning('The output folder exists. Overriding...')
    if not job.pooled:
        _LOG.info('Inferring transcript abundance of %d samples', n_samples)
    elif whitelist is None:
        _LOG.info('Inferring transcript abundance of the cells of one pooled run (about %d cells, found in the barcode reads)',
                  job.discover_cells)
    else:
        _LOG.info('Inferring transcript abundance of the cells of one pooled run (%d barcodes)', len(whitelist[0]))
    _log_length_model(job.length_model, job.single_ended)


def _map_pooled(job, whitelist):
    """The pooled route: the cells of the pooled run are the samples, all of them in one set.  Finds the cells where
    there is no whitelist, demultiplexes and maps (mapper.map_barcoded) and writes the barcodes.* files -> (the
    SampleSet, the records of the cells that are kept)."""
    parse_threads = 0 if job.debug or job.job_count <= 1 else min(int(job.job_count), 8)     # (one large file: -j parses it)
    discovery = None
    if whitelist is None:
        # no whitelist: the census of the barcode reads gives one (the barcode file is read again below)
        n_units = min(mapper.fastq_records(path) for path in [job.barcode_file] + list(job.fastq_paths))
        picked, _, found = mapper.discover_barcodes(
            common.PackedReadFeeder([job.barcode_file], paired=False, threads=parse_threads), job.barcode_length,
            job.discover_cells, start=job.barcode_start, drop_neighbours=not job.discover_keep_neighbours,
            device=job.device, n_units=n_units)
        discovery = _output_discovery(job.output_path, picked, found, job.discover_cells, job.barcode_length,
                                      job.barcode_start, job.discover_keep_neighbours)
        _LOG.info('Barcodes of %d units: %d counted, %d short, %d unreadable, %d distinct; rank %d has %d, threshold %d: '
                  '%d candidates, %d dropped as neighbours, %d picked', found['units'], found['counted'], found['short'],
                  found['unreadable'], found['distinct'], found['rank'], found['rank_count'], found['threshold'],
                  found['candidates'], found['dropped'], found['picked'])
        whitelist = mapper.check_whitelist(picked)
        job.trace('cell discovery')
    table = mapper.BarcodeTable(*whitelist, device=job.device)
    sample_set, kept, demux = mapper.map_barcoded(
        job.index, table, common.PackedReadFeeder([job.barcode_file], paired=False, threads=parse_threads),
        common.PackedReadFeeder(list(job.fastq_paths), paired=job.paired, threads=parse_threads), job.paired,
        start=job.barcode_start, mismatches=job.barcode_mismatches, min_units=job.min_units, device=job.device,
        strand=job.strand, per_sample_lengths=True, length_model=job.length_model, bias=job.bias, umi_start=job.umi_start,
        umi_length=job.umi_length, umi_mismatches=job.umi_mismatches)
    _LOG.info('Barcodes of %d units: %d exact, %d corrected, %d ambiguous, %d without a match, %d short or unreadable',
              demux['units'], *[demux[name] for name in mapper.BARCODE_STATS])
    if job.umi_length and job.umi_mismatches:
        _LOG.info('UMIs of %d bases: %d units without a readable one, %d duplicates removed, %d of them only for a UMI '
                  'one substitution away', job.umi_length, demux['umi_unreadable'], demux['umi_duplicates'],
                  demux['umi_near_duplicates'])
    elif job.umi_length:
        _LOG.info('UMIs of %d bases: %d units without a readable one, %d duplicates removed', job.umi_length,
                  demux['umi_unreadable'], demux['umi_duplicates'])
    _output_barcodes(job.output_path, table, kept, demux, job.barcode_start, job.barcode_mismatches, job.min_units,
                     job.umi_start, job.umi_length, discovery=discovery, umi_mismatches=job.umi_mismatches)
    if not kept.size:
        raise ValueError('no cell has %d units or more (see %s)' % (job.min_units, job.output_path / 'barcodes.tsv'))
    samples = [_Sample(table.names[c], (), True) for c in kept]
    _LOG.info('%d cells have %d units or more', len(samples), job.min_units)
    job.trace('demultiplexing')
    return sample_set, samples


def _map_set(job, members):
    """The set route: the samples that share launches, through one mapper.SampleSet -> the set, or None when no
    sample goes that way."""
    if not members:
        return None
    _LOG.info('Mapping %d samples in shared launches', len(members))
    feeders = [common.PackedReadFeeder(list(sample.group), paired=job.paired) if common.PackedReadFeeder.eligible(sample.group)
               else common.NativeReadFeeder(list(sample.group), paired=job.paired) for sample in members]
    return mapper.map_sample_set(job.index, feeders, job_count=1 if job.debug else max(1, job.job_count), device=job.device,
                                 strand=job.strand, per_sample_lengths=True, length_model=job.length_model, bias=job.bias)


def _take_from_set(job, sample_set, members):
    """Fills the records of the set's samples, `members` in the set's order, with what the run needs of the set:
    count-matrix rows, then sizes (matrix_only) or summaries with hexamer rows, gene counts and -- inside the regime of
    impute.use_set_quant -- the main estimates from shared EM launches on the table where it lies."""
    from . import impute
    n_genes = None if job.gene_names is None else job.gene_names[0].size
    if job.count_matrix:                    # (one pass over the set's table where it lies: no dense row)
        indptr, indices, data, other = sample_set.gene_count_matrix(job.gene_names[1], n_genes)
        for k, sample in enumerate(members):
            sample.matrix_row = (indices[indptr[k]:indptr[k + 1]], data[indptr[k]:indptr[k + 1]])
            sample.matrix_other = other[k]
    if job.count_molecules:                 # (a pass over the molecule set and the table where they lie)
        m_indptr, m_indices, m_data, m_other = sample_set.gene_molecule_matrix(job.gene_names[1], n_genes)
        if not (numpy.array_equal(m_indptr, indptr) and numpy.array_equal(m_indices, indices) and numpy.array_equal(m_other, other)):
            raise RuntimeError('the molecule matrix does not have the entries of the count matrix')
        for k, sample in enumerate(members):
            sample.molecule_row = m_data[indptr[k]:indptr[k + 1]]
    if job.resolve_molecules:               # (one more pass over the same two: the classes of a UMI, intersected)
        r_indptr, r_indices, r_data, r_tally = sample_set.gene_resolved_matrix(job.gene_names[1], n_genes)
        for k, sample in enumerate(members):
            sample.resolved_row = (r_indices[r_indptr[k]:r_indptr[k + 1]], r_data[r_indptr[k]:r_indptr[k + 1]])
            sample.resolved_tally = r_tally[k]
    if job.distribute_molecules:            # (and one more: the multi-gene groups among them, shared out by an EM per cell)
        d_indptr, d_indices, d_data, d_tally, d_unnamed = sample_set.gene_distributed_matrix(job.gene_names[1], n_genes)
        for k, sample in enumerate(members):
            sample.distributed_row = (d_indices[d_indptr[k]:d_indptr[k + 1]], d_data[d_indptr[k]:d_indptr[k + 1]])
            sample.distributed_tally, sample.to_unnamed = d_tally[k], d_unnamed[k]
    if job.matrix_only:
        for sample, row, mean in zip(members, sample_set.sizes(), sample_set.harmonic_mean_fragment_lengths()):
            sample.sizes, sample.mean = row, mean
        job.trace('mapping (set)')
        return
    for sample, summary, mean in zip(members, sample_set.summarize(), sample_set.harmonic_mean_fragment_lengths()):
        sample.summary, sample.mean = summary, mean
    if job.bias:
        for sample, row in zip(members, sample_set.bias_observed()):
            sample.observed = row
    if job.genes:                           # (one pass over the set's table where it lies)
        for sample, unique, other in zip(members, *sample_set.gene_unique_counts(job.gene_names[1], n_genes)):
            sample.gene_counts = (unique, other)
    job.trace('mapping (set)')
    if all(sample.summary.total for sample in members) and impute.use_set_quant(
            len(members), job.index.transcripts.size, sum(sample.summary.class_count.size for sample in members)):
        try:
            for sample, estimate in zip(members, sample_set.quantify()):
                sample.set_estimate = estimate
        except _native.NativeError as error:
            # (a sample that leaves no abundance above the floor: _finish writes the samples before it and raises
            # at that one, as it always has)
            if error.code != _native.SKM_ERR_UNDEFINED:
                raise
        job.trace('quantification (set)')


def _map_alone(job, sample):
    """The one-by-one route: fills one record from a mapper of its own on the resident index.  The MapResult, and
    with it the sample's table in device memory, ends when this returns."""
    _LOG.info('Mapping sample %s', sample.name)
    map_result = mapper.map_reads(job.index, _feeder(list(sample.group), job.paired, None, None, False),
                                  job_count=job.job_count, debug=job.debug, device=job.device, strand=job.strand,
                                  length_model=job.length_model, bias=job.bias)
    if job.matrix_only:
        sample.sizes, sample.mean = map_result.sizes(), map_result.harmonic_mean_fragment_length
    else:
        sample.summary, sample.mean = map_result.summarize().detach(), map_result.harmonic_mean_fragment_length
    if job.bias:
        sample.observed = map_result.bias_observed()
    if job.genes or job.count_matrix:       # (one dense row of the mapper's own table)
        unique, other = map_result.gene_unique_counts(job.gene_names[1], job.gene_names[0].size)
        sample.gene_counts = (unique, other)
        sample.matrix_row, sample.matrix_other = (numpy.flatnonzero(unique), unique[unique != 0]), other


def _finish(job, samples):
    """Both endings: the refusals that need the units, before anything of a sample is written; unless matrix_only the
    estimates, folders and gene tables (_quantify_samples); then output/counts/ and output/samples.tsv."""
    units = [sample.units() for sample in samples]
    for sample, (total, aligned) in zip(samples, units):
        if total == 0:
            raise ValueError('sample %s has no reads' % sample.name)
        if not job.matrix_only and job.bootstrap > 0 and aligned > RESAMPLE_LIMIT:
            raise ValueError('-b/--bootstrap resamples at most %d aligned units per replicate; sample %s has %d'
                             % (RESAMPLE_LIMIT, sample.name, aligned))
    if not job.matrix_only:
        _quantify_samples(job, samples)
    if job.count_matrix:
        output_count_matrix(job.output_path, job.gene_names[0], [sample.name for sample in samples],
                            [total for total, _ in units], *stack_count_rows(sample.matrix_row for sample in samples),
                            [sample.matrix_other for sample in samples])
    if job.count_molecules:
        indptr, indices, _ = stack_count_rows(sample.matrix_row for sample in samples)
        molecules = numpy.concatenate([numpy.asarray(sample.molecule_row, dtype=numpy.int64) for sample in samples])
        output_molecule_matrix(job.output_path, job.gene_names[0].size, len(samples), indptr, indices, molecules)
        inside = int(sum(int(sample.matrix_row[1].sum()) for sample in samples))
        _LOG.info('Units inside one gene: %d; molecules (distinct UMIs per cell and gene): %d; %.3f units a molecule',
                  inside, int(molecules.sum()), inside / max(int(molecules.sum()), 1))
    if job.resolve_molecules:
        tally = numpy.asarray([sample.resolved_tally for sample in samples], dtype=numpy.int64).reshape(-1, len(RESOLVED_TALLY))
        output_resolved_matrix(job.output_path, job.gene_names[0].size, [sample.name for sample in samples],
                               *stack_count_rows(sample.resolved_row for sample in samples), tally)
        totals = [int(v) for v in tally.sum(axis=0)]
        _LOG.info('Distinct UMIs per cell: %d; resolved to one gene: %d (%d of them rescued), multi-gene: %d, unnamed: %d, '
                  'collisions: %d', totals[0] + totals[2] + totals[3] + totals[4], *totals)
    if job.distribute_molecules:
        tally = numpy.asarray([sample.distributed_tally for sample in samples], dtype=numpy.int64).reshape(-1, len(DISTRIBUTED_TALLY))
        indptr = numpy.concatenate([[0], numpy.cumsum([len(sample.distributed_row[0]) for sample in samples])]).astype(numpy.int64)
        indices = numpy.concatenate([numpy.asarray(sample.distributed_row[0], dtype=numpy.int32) for sample in samples]
                                 or [numpy.zeros(0, dtype=numpy.int32)])
        weights = numpy.concatenate([numpy.asarray(sample.distributed_row[1], dtype=numpy.float64) for sample in samples]
                                 or [numpy.zeros(0, dtype=numpy.float64)])
        output_distributed_matrix(job.output_path, job.gene_names[0].size, [sample.name for sample in samples], indptr, indices,
                                  weights, tally, [sample.to_unnamed for sample in samples])
        totals = [int(v) for v in tally.sum(axis=0)]
        _LOG.info('Distinct UMIs per cell: %d; resolved: %d, distributed by the EM: %d, wide: %d, unnamed: %d, collisions: %d; '
                  'EM steps per cell: %d at most, %d cells capped; weight in genes: %.3f, to no gene: %.3f',
                  sum(totals[:5]), *totals[:5], int(tally[:, 6].max()) if len(tally) else 0, totals[7], float(weights.sum()),
                  float(sum(sample.to_unnamed for sample in samples)))
    with (job.output_path / 'samples.tsv').open('w') as f:
        for sample, (total, aligned) in zip(samples, units):
            f.write('%s\t%d\t%d\t%.2f\n' % (sample.name, total, aligned, sample.mean))
    job.trace('writing', pause=True)
    job.trace(None)
    if job.matrix_only:
        _LOG.info('Wrote the count matrix to %s', job.output_path / 'counts')
    else:
        _LOG.info('Wrote results to %s', job.output_path)


def _quantify_samples(job, samples):
    """What the full ending has over matrix_only: the shared bias pass of the set's samples, every sample's estimate,
    bootstraps and folder in the order of the samples, and the gene tables of the run."""
    members = [sample for sample in samples if sample.in_set]
    if job.bias and members:
        _bias_pass_set(job, members)
    for sample in samples:
        _quantify_and_write(job, sample)
    if job.genes:
        gene_ids, tx_gene = job.gene_names
        names, estimates = [sample.name for sample in samples], numpy.stack([sample.estimate for sample in samples])
        _output_gene_matrix(job.output_path / 'genes.tpm.tsv', gene_ids, names,
                            gene_sums(tx_gene, gene_ids.size, estimates, device=job.device), '%g')
        _output_gene_matrix(job.output_path / 'genes.unique_counts.tsv', gene_ids, names,
                            numpy.stack([sample.gene_counts[0] for sample in samples]), '%d')


def _bias_pass_set(job, members):
    """The second pass of the set's samples together (bias_pass_many) -> their `corrected`.  A sample that leaves no
    abundance above the floor, in either pass, leaves them all without: _quantify_and_write then takes them one by
    one, writes the samples before that one and raises there."""
    try:
        for sample in members:
            if sample.set_estimate is None:
                sample.set_estimate = quantify(sample.summary, device=job.device)
        passed, second = bias_pass_many(job.index, [sample.summary for sample in members],
                                        [sample.set_estimate for sample in members],
                                        [sample.observed for sample in members], job.strand, device=job.device)
        for k, sample in enumerate(members):
            sample.corrected = (passed[k], second[k])
    except _native.NativeError as error:
        if error.code != _native.SKM_ERR_UNDEFINED:
            raise
    job.trace('sequence bias (set)')


def _quantify_and_write(job, sample):
    """One sample's estimate (the set's, or quantify() and bias_pass here), its bootstraps and its folder."""
    _LOG.info('Quantifying sample %s', sample.name)
    if sample.corrected is not None:
        summary, main_result = sample.corrected
    else:
        summary = sample.summary
        main_result = sample.set_estimate if sample.set_estimate is not None else quantify(summary, device=job.device)
        if job.bias:
            summary, main_result = bias_pass(job.index, summary, main_result, sample.observed, job.strand, device=job.device)
    job.trace('quantification', pause=True)
    bootstrapped_results = bootstrap_quantify(summary, main_result, job.bootstrap, seed=job.seed, device=job.device)
    job.trace('bootstraps', pause=True)
    sample_path = job.output_path / sample.name
    sample_path.mkdir(exist_ok=True)
    output_results(sample_path, job.index, job.start_time, summary, main_result, bootstrapped_results,
                   genes=job.gene_names + sample.gene_counts if job.genes else None, device=job.device)
    sample.estimate = main_result
    job.trace('writing', pause=True)


def barcode_options(fastq_paths, single_ended, names, barcodes, barcode_file, barcode_start, barcode_mismatches,
                    min_units, umi_start=0, umi_length=0, discover_cells=None, barcode_length=None,
                    discover_keep_neighbours=False):
    """The checks of `infer-many --barcodes` and `infer-many --discover-cells` that need no read file -> the whitelist
    (barcodes, names) of mapper.read_whitelist, or None where the cells are to be discovered.  ValueError for a
    combination that cannot be and for a malformed whitelist."""
    if barcodes is not None and discover_cells is not None:
        raise ValueError('one of --barcodes and --discover-cells: a whitelist, or cells found in the barcode reads')
    flag = '--barcodes' if discover_cells is None else '--discover-cells'
    if discover_cells is None:
        if barcode_length is not None:
            raise ValueError('--barcode-length does not go with --barcodes: the whitelist gives the length')
        if discover_keep_neighbours:
            raise ValueError('--discover-keep-neighbours goes with --discover-cells')
    else:
        if int(discover_cells) < 1:
            raise ValueError('--discover-cells must be 1 or more, not %r' % (discover_cells,))
        if barcode_length is None:
            raise ValueError('--discover-cells needs the length of a barcode: --barcode-length L')
        if not 1 <= int(barcode_length) <= mapper.MAX_BARCODE_LENGTH:
            raise ValueError('--barcode-length must be 1 to %d, not %r' % (mapper.MAX_BARCODE_LENGTH, barcode_length))
    if barcode_file is None:
        raise ValueError('%s needs the barcode reads: --barcode-file FASTQ' % flag)
    if names is not None:
        raise ValueError('--names does not go with %s: the cells are named by %s'
                         % (flag, 'the whitelist' if discover_cells is None else 'their barcodes'))
    if len(fastq_paths) != (1 if single_ended else 2):
        raise ValueError('%s takes ONE pooled sample: %s, not %d'
                         % (flag, 'one FASTQ file with -s' if single_ended else 'two FASTQ files (one with -s)', len(fastq_paths)))
    if int(barcode_start) < 0:
        raise ValueError('--barcode-start must be 0 or more, not %r' % (barcode_start,))
    if barcode_mismatches not in (0, 1):
        raise ValueError('--barcode-mismatches must be 0 or 1, not %r' % (barcode_mismatches,))
    if int(min_units) < 1:
        raise ValueError('--min-units must be 1 or more, not %r' % (min_units,))
    if int(umi_length) and not 1 <= int(umi_length) <= mapper.MAX_UMI_LENGTH:
        raise ValueError('--umi-length must be 1 to %d, not %r' % (mapper.MAX_UMI_LENGTH, umi_length))
    if int(umi_start) < 0:
        raise ValueError('--umi-start must be 0 or more, not %r' % (umi_start,))
    if int(umi_start) and not int(umi_length):
        raise ValueError('--umi-start goes with --umi-length')
    return mapper.read_whitelist(barcodes) if discover_cells is None else None


def _output_discovery(output_path, picked, found, expect_cells, length, start, keep_neighbours):
    """output/barcodes.discovered.txt: the picked barcodes in ranked order under '#' lines that say how they were
    found -- a whitelist as `--barcodes` reads it; output/barcodes.census.tsv: barcode, count, picked 0/1 of every
    candidate in ranked order.  Returns the "discovery" entry of barcodes.json."""
    with (output_path / 'barcodes.discovered.txt').open('w') as f:
        f.write('# cells discovered from the barcode reads: --discover-cells %d --barcode-length %d --barcode-start %d%s\n'
                % (expect_cells, length, start, ' --discover-keep-neighbours' if keep_neighbours else ''))
        f.write('# threshold %d (a tenth of the count %d at rank %d)\n' % (found['threshold'], found['rank_count'], found['rank']))
        f.write('# distinct %d, candidates %d, dropped %d\n' % (found['distinct'], found['candidates'], found['dropped']))
        for barcode in picked:
            f.write(barcode + '\n')
    stays = set(picked)
    with (output_path / 'barcodes.census.tsv').open('w') as f:
        for barcode, count in zip(found['candidate_barcodes'], found['candidate_counts']):
            f.write('%s\t%d\t%d\n' % (barcode, count, barcode in stays))
    return dict(expect_cells=int(expect_cells), barcode_length=int(length), units_counted=found['counted'], short=found['short'],
                unreadable=found['unreadable'], distinct=found['distinct'], rank=found['rank'], rank_count=found['rank_count'],
                threshold=found['threshold'], candidates=found['candidates'], dropped_neighbours=found['dropped'],
                picked=found['picked'], keep_neighbours=bool(keep_neighbours))


def _output_barcodes(output_path, table, kept, demux, start, mismatches, min_units, umi_start=0, umi_length=0, discovery=None,
                     umi_mismatches=0):
    """output/barcodes.tsv: barcode, name, assigned units, kept 0/1 per whitelist entry -- with UMIs also the units
    with a readable UMI (what `kept` looks at) and the units left after collapse (with umi_mismatches=1: after both
    kinds of removal); output/barcodes.json: the demultiplexing summary, with umi_mismatches=1 also that key and
    umi_near_duplicates."""
    is_kept = numpy.zeros(len(table), dtype=bool)
    is_kept[kept] = True
    with (output_path / 'barcodes.tsv').open('w') as f:
        if umi_length:
            for row in zip(table.barcodes, table.names, demux['cell_assigned'], is_kept, demux['cell_units'],
                           demux['cell_survivors']):
                f.write('%s\t%s\t%d\t%d\t%d\t%d\n' % row)
        else:
            for barcode, name, units, flag in zip(table.barcodes, table.names, demux['cell_units'], is_kept):
                f.write('%s\t%s\t%d\t%d\n' % (barcode, name, units, flag))
    summary = {name: demux[name] for name in mapper.BARCODE_STATS}
    summary.update(units=demux['units'], records=demux['records'], whitelist=len(table), barcode_length=table.length,
                   barcode_start=int(start), barcode_mismatches=int(mismatches), min_units=int(min_units),
                   cells=int(len(kept)), assigned=int(demux['exact'] + demux['corrected']))
    if umi_length:
        summary.update(umi_start=int(umi_start), umi_length=int(umi_length), umi_unreadable=demux['umi_unreadable'],
                       umi_duplicates=demux['umi_duplicates'])
        if umi_mismatches:
            summary.update(umi_mismatches=int(umi_mismatches), umi_near_duplicates=demux['umi_near_duplicates'])
    if discovery is not None:
        summary.update(discovery=discovery)
    with (output_path / 'barcodes.json').open('w') as f:
        json.dump(summary, f, indent=4)
        f.write('\n')


def _phase_trace():
    """SKM_TRACE_INFER (set to anything): run_many's host wall time per phase on stderr.  trace(phase) closes the
    lap since the last call and prints it; with pause=True the lap is added to the phase's sum instead, and
    trace(None) prints the sums.  Without the switch the calls do nothing."""
    if os.environ.get('SKM_TRACE_INFER') is None:
        return lambda phase, pause=False: None
    state = {'last': time.perf_counter(), 'sums': {}}

    def trace(phase, pause=False):
        now = time.perf_counter()
        lap, state['last'] = now - state['last'], now
        if phase is None:
            for name, total in state['sums'].items():
                print('[run_many] %-24s %10.1f ms' % (name, total * 1e3), file=sys.stderr)
        elif pause:
            state['sums'][phase] = state['sums'].get(phase, 0.0) + lap
        else:
            print('[run_many] %-24s %10.1f ms' % (phase, lap * 1e3), file=sys.stderr)
    return trace


RESAMPLE_LIMIT = 2 ** 32 - 1        # units one multinomial draw can resample (skm_quant_bootstrap*)


def _check_resample_limit(map_result, ranks):
    """`-b N` draws n = class_count.sum() units per replicate (seekmer/infer.py:108-111); the device
    draw counts them in 32 bits.  Said now, before the EM, not after it."""
    _, _, unaligned, total = map_result.sizes()
    aligned = total - unaligned
    if ranks.world > 1:
        aligned = sum(ranks.gather_to_root(aligned) or [0])
    if ranks.rank == 0 and aligned > RESAMPLE_LIMIT:
        raise ValueError('-b/--bootstrap resamples at most %d aligned units per replicate; this sample has %d'
                         % (RESAMPLE_LIMIT, aligned))


def _feeder(fastq_paths, paired, parse_threads, shard, keep_reference_batches, sum_over_ranks=None):
    """The native readers as run() uses them.

    Plain files: the one-pass reader (common.PackedReadFeeder) -- the text is parsed straight to the
    mapper's 2-bit read codes by `parse_threads` workers (None = up to 16, the cores this process may
    use less one) and drained into the mapper natively; a third of the bytes of the ASCII batches
    cross PCIe.  Several ranks: each reads a contiguous run of the sample's units, found from
    newline counts that the ranks add up (`sum_over_ranks`; PackedReadFeeder.locate_share).
    Compressed inputs (every rank then takes every world-th batch of the sample off the two-pass
    reader's line index) and `-m` (readmap.txt is written batch by batch in the reference's batches
    of 65 536, seekmer/common.py:17) go through common.NativeReadFeeder: plain files parsed by up to 8 threads, into page-locked slabs when
    there is enough text (> 4 GiB) to pay for pinning them, in batches of 2^18 units (2^20 above
    16 GiB of text); parse_threads 0 = its sequential engine."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    total = 0
    for path in fastq_paths:
        try:
            total += os.path.getsize(str(path))
        except OSError:
            pass
    one_rank = shard is None or shard[1] <= 1
    if (one_rank or sum_over_ranks is not None) and not keep_reference_batches and parse_threads != 0 \
            and common.PackedReadFeeder.eligible(fastq_paths):
        threads = parse_threads if parse_threads else max(1, min(16, cores - 1))
        world = 1 if one_rank else shard[1]
        return common.PackedReadFeeder(fastq_paths, paired, threads=threads, pinned=total > (1 << 30) * world,
                                       shard=None if one_rank else shard, sum_over_ranks=sum_over_ranks)
    if parse_threads is None:
        parse_threads = 0 if keep_reference_batches else min(8, cores)
    if parse_threads <= 0:
        return common.NativeReadFeeder(fastq_paths, paired=paired, shard=shard)
    return common.NativeReadFeeder(fastq_paths, paired=paired, batch_units=1 << (20 if total > (16 << 30) else 18),
                                   threads=parse_threads, pinned=total > (4 << 30), shard=shard)


def finish(map_result, ranks, quantify_ranks, comm=None):
    """From the ranks' tables to the sample's results.  One rank: summarize + quantify as the
    reference does (seekmer/infer.py:66-78).  Several: `quantify_ranks(map_result)` runs the EM
    over the rank-local tables (collectives inside; every rank gets the TPM of the whole sample),
    THEN the other ranks' tables go to rank 0 and are merged into its own, whose summary is the
    whole sample's: (SummarizedResult, TPM) on rank 0, (None, TPM) elsewhere.  The tables travel as
    numpy arrays through the process group (host copy, rank 0 merges on its GPU) -- or, with
    SKM_HANDOVER=rccl and a communicator, from GPU to GPU as they lie in HBM
    (parallel.hand_over_device: ncclSend / ncclRecv + merge by key; experimental, no multi-GPU
    node has run it yet)."""
    from . import parallel
    if ranks.world == 1:
        summarized = map_result.summarize()
        _LOG.info('Quantifying transcripts')
        return summarized, quantify(summarized)
    _LOG.info('Quantifying transcripts')
    tpm = quantify_ranks(map_result)
    if comm and os.environ.get('SKM_HANDOVER') == 'rccl':
        parallel.hand_over_device(map_result, comm, ranks)
        return (map_result.summarize() if ranks.rank == 0 else None), tpm
    tables = ranks.gather_arrays_to_root(parallel.rank_table(map_result) if ranks.rank else {})
    if ranks.rank != 0:
        return None, tpm
    parallel.merge_into(map_result, tables[1:])
    return map_result.summarize(), tpm


# ------------------------------------------------------------- device tables
class _QuantHandle:
    """skm_quant* for one class table."""

    def __init__(self, handle, n_tx, n_classes):
        self.handle = handle
        self.n_tx = n_tx
        self.n_classes = n_classes

    @classmethod
    def from_csr(cls, n_tx, offsets, targets, counts, device=0):
        offsets = numpy.ascontiguousarray(offsets, dtype=numpy.int64)
        targets = numpy.ascontiguousarray(targets if len(targets) else [0], dtype=numpy.int32)
        counts = numpy.ascontiguousarray(counts if len(counts) else [0.0], dtype='f8')
        out = ctypes.c_void_p()
        _native.check(_native.hip().skm_quant_create(
            device, n_tx, offsets.size - 1, _native.ptr(offsets, _native.c_i64p),
            _native.ptr(targets, _native.c_i32p), _native.ptr(counts, _native.c_f64p),
            ctypes.byref(out)))
        return cls(out, n_tx, offsets.size - 1)

    @classmethod
    def from_map_result(cls, map_result, n_tx):
        out = ctypes.c_void_p()
        _native.check(_native.hip().skm_quant_create_from_mapper(
            map_result._handle, n_tx, ctypes.byref(out)))
        return cls(out, n_tx, map_result.sizes()[0])

    def em(self, x, l, fixed_iters=0, max_iters=0, rel_tol=REL_TOL, x_floor=X_FLOOR):
        x = numpy.array(x, dtype='f8', copy=True, order='C')
        l = numpy.ascontiguousarray(l, dtype='f8')
        iters = ctypes.c_int64()
        _native.check(_native.hip().skm_quant_em(
            self.handle, _native.ptr(x, _native.c_f64p), _native.ptr(l, _native.c_f64p),
            rel_tol, x_floor, max_iters, fixed_iters, ctypes.byref(iters)))
        return x, iters.value

    def components(self, arrays=True):
        """The connected components of the class table and the tiles the one-GPU EM steps them in:
        (info, tx_label, tx_tile, class_tile); info as skm_quant_components documents it."""
        raw = numpy.zeros(8, dtype=numpy.int64)
        _native.check(_native.hip().skm_quant_components(self.handle, _native.ptr(raw, _native.c_i64p),
                                                         None, None, None))
        info = {'built': bool(raw[0]), 'tiles': int(raw[1]), 'oversize': int(raw[2]), 'em_uses_tiles': bool(raw[3]),
                'capacity': (int(raw[4]), int(raw[5]), int(raw[6])), 'segment': int(raw[7])}
        if not arrays or not info['built']:
            return info, None, None, None
        label = numpy.zeros(self.n_tx, dtype=numpy.int32)
        tile = numpy.zeros(self.n_tx, dtype=numpy.int32)
        class_tile = numpy.zeros(max(self.n_classes, 1), dtype=numpy.int32)
        _native.check(_native.hip().skm_quant_components(
            self.handle, _native.ptr(raw, _native.c_i64p), _native.ptr(label, _native.c_i32p),
            _native.ptr(tile, _native.c_i32p), _native.ptr(class_tile, _native.c_i32p)))
        return info, label, tile, class_tile[:self.n_classes]

    def rows_built(self):
        """Whether the handle holds the whole table's transcript-major rows (skm_quant_rows_built)."""
        built = ctypes.c_int()
        _native.check(_native.hip().skm_quant_rows_built(self.handle, ctypes.byref(built)))
        return bool(built.value)

    def set_counts(self, counts):
        counts = numpy.ascontiguousarray(counts, dtype='f8')
        _native.check(_native.hip().skm_quant_set_counts(self.handle,
                                                         _native.ptr(counts, _native.c_f64p)))

    def bootstrap(self, n_boot, seed, x0, l, want_counts=False, tpm=False):
        """(results [n_boot, n_tx], resampled counts or None, EM steps per replicate); tpm: the
        results already scaled as quantify() scales them (seekmer/infer.py:127-129)."""
        x0 = numpy.ascontiguousarray(x0, dtype='f8')
        l = numpy.ascontiguousarray(l, dtype='f8')
        out = numpy.zeros((n_boot, self.n_tx), dtype='f8')
        if tpm and not want_counts:
            iters = numpy.zeros(max(n_boot, 1), dtype=numpy.int64)
            _native.check(_native.hip().skm_quant_bootstrap_tpm(
                self.handle, n_boot, seed, _native.ptr(x0, _native.c_f64p),
                _native.ptr(l, _native.c_f64p), REL_TOL, X_FLOOR, 0,
                _native.ptr(out, _native.c_f64p), _native.ptr(iters, _native.c_i64p)))
            return out, None, iters[:n_boot]
        counts = numpy.zeros((n_boot, max(self.n_classes, 1)), dtype=numpy.int64) if want_counts else None
        iters = numpy.zeros(max(n_boot, 1), dtype=numpy.int64)
        _native.check(_native.hip().skm_quant_bootstrap(
            self.handle, n_boot, seed, _native.ptr(x0, _native.c_f64p),
            _native.ptr(l, _native.c_f64p), REL_TOL, X_FLOOR, 0,
            _native.ptr(out, _native.c_f64p),
            _native.ptr(counts, _native.c_i64p) if want_counts else None,
            _native.ptr(iters, _native.c_i64p)))
        return out, counts, iters[:n_boot]

    def em_many(self, counts, x0, l, tpm=False):
        """The EM on this handle's class structure for every row of counts [K, C] (the caller's class
        order), all from x0: (results [K, n_tx], EM steps per row) -- what set_counts(row) + em(x0, l)
        give, row by row and bit for bit, with eight rows side by side on the device; tpm: the results
        already scaled as quantify() scales them (seekmer/infer.py:127-129).  The handle keeps its own counts."""
        counts = numpy.ascontiguousarray(counts, dtype='f8')
        if counts.ndim != 2 or counts.shape[1] != self.n_classes:
            raise ValueError('counts must be [K, %d]' % self.n_classes)
        x0 = numpy.ascontiguousarray(x0, dtype='f8')
        l = numpy.ascontiguousarray(l, dtype='f8')
        n = counts.shape[0]
        out = numpy.zeros((n, self.n_tx), dtype='f8')
        iters = numpy.zeros(max(n, 1), dtype=numpy.int64)
        _native.check(_native.hip().skm_quant_em_many(
            self.handle, n, _native.ptr(counts, _native.c_f64p), _native.ptr(x0, _native.c_f64p),
            _native.ptr(l, _native.c_f64p), REL_TOL, X_FLOOR, int(bool(tpm)), _native.ptr(out, _native.c_f64p),
            _native.ptr(iters, _native.c_i64p)))
        return out, iters[:n]

    def em_blend(self, class_cell, weight, cell_total, x0, l, tpm=False, want_counts=False):
        """The second round of impute on a handle that holds all cells' classes with their own counts:
        problem i is the table blended for cell i (skm_quant_em_blend; the counts are made on the device).
        (results [n, n_tx], EM steps per cell, blended counts [n, C] or None)."""
        class_cell = numpy.ascontiguousarray(class_cell, dtype=numpy.int32)
        weight = numpy.ascontiguousarray(weight, dtype='f8')
        cell_total = numpy.ascontiguousarray(cell_total, dtype='f8')
        n = cell_total.size
        if weight.shape != (n, n) or class_cell.size != self.n_classes:
            raise ValueError('weight must be [n, n] and class_cell [C] for n = len(cell_total) cells')
        x0 = numpy.ascontiguousarray(x0, dtype='f8')
        l = numpy.ascontiguousarray(l, dtype='f8')
        out = numpy.zeros((n, self.n_tx), dtype='f8')
        iters = numpy.zeros(max(n, 1), dtype=numpy.int64)
        counts = numpy.zeros((n, max(self.n_classes, 1)), dtype='f8') if want_counts else None
        _native.check(_native.hip().skm_quant_em_blend(
            self.handle, n, _native.ptr(class_cell, _native.c_i32p), _native.ptr(weight, _native.c_f64p),
            _native.ptr(cell_total, _native.c_f64p), _native.ptr(x0, _native.c_f64p), _native.ptr(l, _native.c_f64p),
            REL_TOL, X_FLOOR, int(bool(tpm)), _native.ptr(out, _native.c_f64p), _native.ptr(iters, _native.c_i64p),
            _native.ptr(counts, _native.c_f64p) if want_counts else None))
        return out, iters[:n], (counts[:, :self.n_classes] if want_counts else None)

    def timing(self):
        out = (ctypes.c_double * 4)()
        _native.check(_native.hip().skm_quant_timing(self.handle, out))
        return {'em_ns': out[0], 'iterations': int(out[1]), 'launches': int(out[2])}

    def close(self):
        if self.handle:
            _native.hip().skm_quant_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _csr_from_class_map(class_map, n_classes):
    """class_map int64[2, M] (seekmer/mapper.py:93) -> CSR keeping the pair
    order inside every class."""
    class_ids = numpy.asarray(class_map[0], dtype=numpy.int64)
    targets = numpy.asarray(class_map[1], dtype=numpy.int64)
    if class_ids.size > 1 and (numpy.diff(class_ids) < 0).any():
        order = numpy.argsort(class_ids, kind='stable')
        class_ids, targets = class_ids[order], targets[order]
    offsets = numpy.zeros(n_classes + 1, dtype=numpy.int64)
    numpy.cumsum(numpy.bincount(class_ids, minlength=n_classes), out=offsets[1:])
    return offsets, targets.astype(numpy.int32)


def _tpm(x):
    """seekmer/infer.py:127-129"""
    x /= x.sum() / 1000000
    x[x < 0.001] = 0
    x /= x.sum() / 1000000
    return x


def _quant_for(results, device=0):
    cached = getattr(results, '_quant', None) if hasattr(results, '__dict__') else None
    if cached is not None:
        return cached, False
    n_tx = results.effective_lengths.size
    offsets = getattr(results, 'class_offsets', None)
    targets = getattr(results, 'class_targets', None)
    if offsets is None or targets is None:
        offsets, targets = _csr_from_class_map(results.class_map, results.class_count.size)
    return _QuantHandle.from_csr(n_tx, offsets, targets, results.class_count, device), True


def quantify(results, x0=None, bootstrap=False, seed=None, fixed_iters=0, return_iters=False, device=0):
    """Estimate the transcript abundance (seekmer/infer.py:88-130) on GPU `device`."""
    transcript_length = results.effective_lengths.astype('f8')
    if results.class_map.size == 0:
        zeros = numpy.zeros(results.effective_lengths.size).astype('f8')
        return (zeros, 0) if return_iters else zeros
    if x0 is None:
        x = numpy.ones(transcript_length.size, dtype='f8') / transcript_length
    else:
        x = x0.copy()
    x /= x.sum()
    quant, owned = _quant_for(results, device)
    try:
        if bootstrap:
            if seed is None:
                seed = int.from_bytes(__import__('os').urandom(8), 'little')
            out, _, iters = quant.bootstrap(1, seed, x, transcript_length)
            x, iters = out[0], int(iters[0])
        else:
            x, iters = quant.em(x, transcript_length, fixed_iters=fixed_iters)
    finally:
        if owned:
            quant.close()
    x = _tpm(x)
    return (x, iters) if return_iters else x


def quantify_many(results, class_counts, device=0, return_iters=False):
    """quantify() for K count vectors on ONE class table: `results` supplies the class structure and
    the effective lengths, class_counts is [K, C] in the order of results.class_count.  Returns the K
    TPM vectors ([K, n_tx]) that quantify() gives for a table with those counts -- every problem starts
    from 1 / effective length as quantify() does (seekmer/infer.py:116-119) --, with the EM steps of each
    when return_iters is set.  The problems run eight at a time on the device (skm_quant_em_many)."""
    transcript_length = results.effective_lengths.astype('f8')
    class_counts = numpy.asarray(class_counts, dtype='f8')
    if class_counts.ndim != 2:
        raise ValueError('class_counts must be [K, C]')
    n = class_counts.shape[0]
    if results.class_map.size == 0:
        zeros = numpy.zeros((n, transcript_length.size), dtype='f8')
        return (zeros, numpy.zeros(n, dtype=numpy.int64)) if return_iters else zeros
    x = numpy.ones(transcript_length.size, dtype='f8') / transcript_length
    x /= x.sum()
    quant, owned = _quant_for(results, device)
    try:
        out, iters = quant.em_many(class_counts, x, transcript_length, tpm=True)
    finally:
        if owned:
            quant.close()
    return (out, iters) if return_iters else out


def _table_csr(results):
    """(class offsets, class targets, class counts) of a summary; a summary without class tuples has
    no classes here (quantify() returns zeros for it before it looks at the counts)."""
    if results.class_map.size == 0:
        return numpy.zeros(1, dtype=numpy.int64), numpy.zeros(0, dtype=numpy.int32), numpy.zeros(0, dtype='f8')
    offsets = getattr(results, 'class_offsets', None)
    targets = getattr(results, 'class_targets', None)
    if offsets is None or targets is None:
        offsets, targets = _csr_from_class_map(results.class_map, results.class_count.size)
    offsets = numpy.asarray(offsets, dtype=numpy.int64)
    return offsets - offsets[0], numpy.asarray(targets, dtype=numpy.int32)[offsets[0]:offsets[-1]], \
        numpy.asarray(results.class_count, dtype='f8')


def quantify_tables(results_list, device=0, return_iters=False, x0s=None):
    """quantify() for K DIFFERENT class tables over the same transcripts (the companion of quantify_many,
    which runs K count vectors on one table): [K, n_tx] TPM, row k what quantify(results_list[k]) returns
    bit for bit -- every table starts from 1 / its effective lengths as quantify() does
    (seekmer/infer.py:116-119) --, with the EM steps of each when return_iters is set.  The tables are
    stacked into one block-diagonal problem and stepped in shared launches, each to its own stopping
    rule (skm_quant_em_tables).  Tables of different n_tx raise ValueError.

    x0s: None, or [K, n_tx] start vectors: table k then starts from row k normalised as quantify() normalises its
    x0 (a copy, x /= x.sum()), and row k of the result is quantify(results_list[k], x0=x0s[k]) bit for bit (a table
    without class tuples gives zeros whatever its row holds, as quantify()).  A wrong number of rows or a wrong
    width raises ValueError."""
    results_list = list(results_list)
    n = len(results_list)
    sizes = {results.effective_lengths.size for results in results_list}
    if len(sizes) > 1:
        raise ValueError('the tables must share their transcripts: n_tx = %s' % sorted(sizes))
    n_tx = sizes.pop() if sizes else 0
    if x0s is not None:
        x0s = numpy.asarray(x0s, dtype='f8')
        if x0s.ndim != 2 or x0s.shape[0] != n or (n and x0s.shape[1] != n_tx):
            raise ValueError('x0s must be [%d, %d]: one start vector per table, not %s' % (n, n_tx, x0s.shape))
    out = numpy.zeros((n, n_tx), dtype='f8')
    iters = numpy.zeros(max(n, 1), dtype=numpy.int64)
    if n and n_tx:
        lengths = numpy.zeros((n, n_tx), dtype='f8')
        start = numpy.zeros((n, n_tx), dtype='f8')
        table_offsets = numpy.zeros(n + 1, dtype=numpy.int64)
        offsets, targets, counts = [numpy.zeros(1, dtype=numpy.int64)], [], []
        n_ids = 0
        for k, results in enumerate(results_list):
            lengths[k] = results.effective_lengths.astype('f8')
            if x0s is None or results.class_map.size == 0:
                x = numpy.ones(n_tx, dtype='f8') / lengths[k]
            else:
                x = x0s[k].copy()
            x /= x.sum()
            start[k] = x
            table = _table_csr(results)
            offsets.append(table[0][1:] + n_ids)
            targets.append(table[1])
            counts.append(table[2])
            n_ids += int(table[0][-1])
            table_offsets[k + 1] = table_offsets[k] + table[2].size
        offsets = numpy.ascontiguousarray(numpy.concatenate(offsets), dtype=numpy.int64)
        targets = numpy.ascontiguousarray(numpy.concatenate(targets + [numpy.zeros(1, dtype=numpy.int32)]), dtype=numpy.int32)
        counts = numpy.ascontiguousarray(numpy.concatenate(counts + [numpy.zeros(1, dtype='f8')]), dtype='f8')
        _native.check(_native.hip().skm_quant_em_tables(
            device, n_tx, n, _native.ptr(table_offsets, _native.c_i64p), _native.ptr(offsets, _native.c_i64p),
            _native.ptr(targets, _native.c_i32p), _native.ptr(counts, _native.c_f64p), _native.ptr(start, _native.c_f64p),
            _native.ptr(lengths, _native.c_f64p), REL_TOL, X_FLOOR, 0, 1, _native.ptr(out, _native.c_f64p),
            _native.ptr(iters, _native.c_i64p)))
    return (out, iters[:n]) if return_iters else out


def quantify_resident(map_result, comm=None, return_iters=False, return_effective_lengths=False):
    """quantify(map_result.summarize()) without the class table leaving the GPU
    (seekmer/infer.py:88-130 + seekmer/mapper.py:134-141) -- one native call:
    fragment-length histogram (all-reduced over `comm`, an skm_comm handle, when
    given) -> effective lengths -> start vector -> EM -> TPM."""
    length = map_result.transcript_lengths
    tpm = numpy.empty(length.size, dtype='f8')
    eff = numpy.empty(length.size, dtype='f8') if return_effective_lengths else None
    iters = ctypes.c_int64()
    _native.check(_native.hip().skm_quant_infer(
        map_result._handle, comm, _native.ptr(length, _native.c_f64p), length.size, REL_TOL, X_FLOOR, 0,
        _native.ptr(tpm, _native.c_f64p), _native.ptr(eff, _native.c_f64p) if eff is not None else None,
        ctypes.byref(iters)))
    out = (tpm,)
    if return_iters:
        out += (iters.value,)
    if return_effective_lengths:
        out += (eff,)
    return out if len(out) > 1 else tpm


def bootstrap_quantify(results, x0, n_boot, seed=None, device=0):
    """The `-b N` loop of run() (seekmer/infer.py:79-82) as one device call on GPU `device`."""
    if n_boot <= 0:
        return []
    transcript_length = results.effective_lengths.astype('f8')
    if results.class_map.size == 0:
        return [numpy.zeros(transcript_length.size, dtype='f8') for _ in range(n_boot)]
    if seed is None:
        seed = int.from_bytes(__import__('os').urandom(8), 'little')
    x = x0.copy()
    x /= x.sum()
    quant, owned = _quant_for(results, device)
    try:
        out, _, _ = quant.bootstrap(n_boot, seed, x, transcript_length, tpm=True)
    finally:
        if owned:
            quant.close()
    return list(out)


def _bootstrap_share(table, x0, first, step, count, seed, device=0):
    """Replicates first, first + step, ... (`count` of them) of the `-b N` loop on this process's GPU:
    TPM vectors [count, T] (skm_quant_bootstrap_share_tpm)."""
    n_tx = table['effective_lengths'].size
    out = numpy.zeros((count, n_tx), dtype='f8')
    if count == 0:
        return out
    quant = _QuantHandle.from_csr(n_tx, table['class_offsets'], table['class_targets'], table['class_count'], device)
    try:
        x = numpy.array(x0, dtype='f8')
        x /= x.sum()
        length = numpy.ascontiguousarray(table['effective_lengths'], dtype='f8')
        iters = numpy.zeros(count, dtype=numpy.int64)
        _native.check(_native.hip().skm_quant_bootstrap_share_tpm(
            quant.handle, count, first, step, seed, _native.ptr(x, _native.c_f64p), _native.ptr(length, _native.c_f64p),
            REL_TOL, X_FLOOR, 0, _native.ptr(out, _native.c_f64p), _native.ptr(iters, _native.c_i64p)))
    finally:
        quant.close()
    return out


def bootstrap_ranks(results, x0, n_boot, ranks, seed=None, device=0, share=_bootstrap_share):
    """The `-b N` loop of run() (seekmer/infer.py:79-82) over the ranks: rank 0
    (the only one that holds `results`, the summary of the merged table, and `x0`, the main estimate)
    shares the merged table; rank r runs the replicates r, r + G, ... on its GPU with no collective;
    the TPM vectors are gathered on rank 0 and returned there in replicate order ([] elsewhere).
    A replicate's draw depends on (seed, its number) alone, so the list does not depend on G.
    `share(table, x0, first, step, count, seed, device)` is the per-rank piece (tests stand the
    oracle in for it)."""
    from . import parallel
    if n_boot <= 0:
        return []
    if ranks.world == 1:
        return bootstrap_quantify(results, x0, n_boot, seed=seed, device=device)
    table = None
    if ranks.rank == 0:
        if seed is None:
            seed = int.from_bytes(__import__('os').urandom(8), 'little')
        table = {'class_offsets': results.class_offsets, 'class_targets': results.class_targets,
                 'class_count': results.class_count, 'effective_lengths': results.effective_lengths.astype('f8'),
                 'x0': numpy.asarray(x0, dtype='f8'), 'seed': numpy.asarray([seed], dtype=numpy.uint64)}
    table = ranks.broadcast_arrays(table)
    seed = int(table['seed'][0])
    first, step, count = parallel.replicate_share(n_boot, ranks.rank, ranks.world)
    n_tx = table['effective_lengths'].size
    if table['class_count'].size == 0:                      # (quantify: an empty class_map gives zeros)
        mine = numpy.zeros((count, n_tx), dtype='f8')
    else:
        mine = share(table, table['x0'], first, step, count, seed, device)
    parts = ranks.gather_arrays_to_root({'tpm': mine})
    if ranks.rank != 0:
        return []
    out = [None] * n_boot
    for r, part in enumerate(parts):
        for j, number in enumerate(range(r, n_boot, ranks.world)):
            out[number] = part['tpm'][j]
    return out


def em(x, l, class_map, class_count, fixed_iters=0, return_iters=False, device=0):
    """Expectation-maximization (seekmer/infer.py:133-168)."""
    class_count = numpy.asarray(class_count, dtype='f8')
    offsets, targets = _csr_from_class_map(class_map, class_count.size)
    quant = _QuantHandle.from_csr(numpy.asarray(l).size, offsets, targets, class_count, device)
    try:
        x, iters = quant.em(x, l, fixed_iters=fixed_iters)
    finally:
        quant.close()
    return (x, iters) if return_iters else x


# ------------------------------------------------------------------- outputs
def output_results(output_path, index, start_time, results, main_abundance,
                   bootstrapped_abundance, genes=None, device=0):
    """Output the quantification results (seekmer/infer.py:171-197).

    genes: None, or (gene_ids, tx_gene, unique, other) of --genes (gene_map, gene_unique_counts): the run then
    also writes abundance.genes.tsv, the genes/ datasets of abundance.npz and the gene counts of run_info.json;
    every other byte is what it is without."""
    run_info = _generate_run_info(bootstrapped_abundance, index, results, start_time)
    if genes is not None:
        gene_ids, _, unique, other = genes
        run_info.update(n_genes=int(len(gene_ids)), n_gene_unique=int(numpy.sum(unique)), n_gene_ambiguous=int(other[0]),
                        n_gene_unnamed=int(other[1]))
        _LOG.info('Genes: %d; units inside one gene %d, ambiguous between genes %d, of unnamed transcripts %d',
                  run_info['n_genes'], run_info['n_gene_unique'], run_info['n_gene_ambiguous'], run_info['n_gene_unnamed'])
    with (output_path / 'run_info.json').open('w') as f:
        json.dump(run_info, f)
    est_counts = _infer_est_counts(index, results, main_abundance)
    _output_abundance_table(output_path, index, results, est_counts, main_abundance)
    gene_arrays = {}
    if genes is not None:
        gene_ids, tx_gene, unique, _ = genes
        table = gene_table(index, gene_ids, tx_gene, results, main_abundance, est_counts, unique, device=device)
        _output_gene_table(output_path, table)
        gene_arrays = {'genes/ids': table['gene_id'], 'genes/tpm': table['tpm'], 'genes/est_counts': table['est_count'],
                       'genes/lengths': table['length'], 'genes/eff_lengths': table['eff_length'],
                       'genes/unique_counts': table['unique_count']}
        if len(bootstrapped_abundance):     # (all replicates in one call)
            rows = gene_sums(tx_gene, len(gene_ids), numpy.stack(list(bootstrapped_abundance)), device=device)
            for i, row in enumerate(rows):
                gene_arrays['genes/bootstrap/bs{}'.format(i)] = row
    _output_arrays(output_path, index, results, run_info, est_counts, bootstrapped_abundance, extra=gene_arrays)


def _output_gene_table(output_path, table):
    """abundance.genes.tsv: GENE_COLUMNS, one line per named gene in gene_ids order; tab separated, floats as %g"""
    with (output_path / 'abundance.genes.tsv').open('w') as f:
        f.write('\t'.join(GENE_COLUMNS) + '\n')
        # (columns as Python lists: indexing numpy arrays element by element is most of such a loop's time)
        columns = [numpy.asarray(table[name]).tolist() for name in GENE_COLUMNS]
        f.writelines('%s\t%d\t%g\t%g\t%g\t%g\t%d\n' % (gene.decode(), n, length, eff, est, tpm, unique)
                     for gene, n, length, eff, est, tpm, unique in zip(*columns))


def _output_gene_matrix(path, gene_ids, names, matrix, fmt):
    """genes as rows, samples as columns in sample order; a header line of the sample names"""
    with path.open('w') as f:
        f.write('\t'.join(['gene_id'] + list(names)) + '\n')
        for gene, values in zip(numpy.asarray(gene_ids).tolist(), numpy.asarray(matrix).T.tolist()):
            f.write('\t'.join([gene.decode()] + [fmt % value for value in values]) + '\n')


def _generate_run_info(bootstrapped_abundance, index, results, start_time):
    """seekmer/infer.py:200-216"""
    class_target_count = numpy.bincount(results.class_map[0].astype(numpy.int64),
                                        minlength=results.class_count.size) \
        if results.class_map.size else numpy.zeros(results.class_count.size, dtype=numpy.int64)
    unique_count = results.class_count[class_target_count == 1].sum()
    run_info = {
        'n_targets': len(index.transcripts),
        'n_bootstraps': len(bootstrapped_abundance),
        'n_processed': results.total,
        'n_pseudoaligned': results.aligned,
        'n_unique': int(unique_count),
        'p_pseudoaligned': results.aligned / results.total,
        'p_unique': unique_count / results.total,
        'kallisto_version': '0.44.0',
        'index_version': 9000,
        'start_time': start_time.isoformat(sep=' '),
        'call': ' '.join([shlex.quote(arg) for arg in sys.argv]),
    }
    length_model = getattr(results, 'length_model', None)
    if length_model is not None:          # (--fragment-length / --sd: the effective lengths are the model's)
        run_info['fragment_length_model'] = {'mean': length_model[0], 'sd': length_model[1]}
    if getattr(results, 'bias_weights', None) is not None:      # (--bias: the effective lengths carry the hexamer weights)
        run_info['bias'] = True
    return run_info


def _output_abundance_table(output_path, index, results, est_counts, main_abundance):
    """abundance.tsv: target_id, length, eff_length (f4), est_count, tpm; tab
    separated, floats as %g (seekmer/infer.py:219-230)."""
    ids = index.transcripts['transcript_id']
    length = index.transcripts['length']
    eff = results.effective_lengths.astype('f4')
    with (output_path / 'abundance.tsv').open('w') as f:
        f.write('target_id\tlength\teff_length\test_count\ttpm\n')
        for i in range(len(ids)):
            f.write('%s\t%g\t%g\t%g\t%g\n' % (ids[i].decode(), float(length[i]), float(eff[i]),
                                            float(est_counts[i]), float(main_abundance[i])))


def _infer_est_counts(index, results, main_abundance):
    """Estimated read counts from the raw length (seekmer/infer.py:233-252)."""
    est_counts = main_abundance * index.transcripts['length']
    est_counts *= results.aligned / est_counts.sum()
    return est_counts


def _output_arrays(output_path, index, results, run_info, est_counts, bootstrapped_abundance, extra=None):
    """The datasets of abundance.h5 (seekmer/infer.py:255-325) as abundance.npz:
    PyTables/h5py are not installed here, so the kallisto-compatible HDF5
    container itself is out of reach; dataset names
    are kept ('aux/ids', 'est_counts', 'bootstrap/bs0', ...)."""
    bias_weights = getattr(results, 'bias_weights', None)        # (None without --bias: the reference's placeholders)
    arrays = {
        'aux/call': numpy.frombuffer(run_info['call'].encode() or b' ', dtype='S1'),
        'aux/index_version': numpy.asarray([run_info['index_version']]),
        'aux/start_time': numpy.frombuffer(run_info['start_time'].encode(), dtype='S1'),
        'aux/num_bootstrap': numpy.asarray([run_info['n_bootstraps']]),
        'aux/num_processed': numpy.asarray([run_info['n_processed']]),
        'aux/kallisto_version': numpy.frombuffer(run_info['kallisto_version'].encode(), dtype='S1'),
        'aux/ids': numpy.asarray(index.transcripts['transcript_id']),
        'aux/lengths': numpy.asarray(index.transcripts['length']),
        'aux/fld': results.fragment_length_frequencies.astype('i4'),
        'aux/eff_lengths': results.effective_lengths.astype('f8'),
        'aux/bias_observed': numpy.ones(4096, dtype='i4') if bias_weights is None else results.bias_observed.astype('i4'),
        'aux/bias_normalized': numpy.ones(4096, dtype='f8') if bias_weights is None else bias_weights.astype('f8'),
        'est_counts': est_counts.astype('f8'),
    }
    for i, bootstrap in enumerate(bootstrapped_abundance):
        arrays['bootstrap/bs{}'.format(i)] = bootstrap
    arrays.update(extra or {})              # (--genes: the genes/ datasets)
    with (output_path / 'abundance.npz').open('wb') as f:
        numpy.savez(f, **arrays)


def add_subcommand_parser(subparsers):
    """Add an infer command to the subparsers (seekmer/infer.py:328-353)."""
    parser = subparsers.add_parser('infer', help='infer transcript abundance')
    parser.add_argument('index_path', type=pathlib.Path, metavar='index',
                        help='specify a Seekmer index file')
    parser.add_argument('output_path', type=pathlib.Path, metavar='output',
                        help='specify a output folder')
    parser.add_argument('fastq_paths', type=pathlib.Path, metavar='fastq',
                        nargs='+', help='specify a FASTQ read file')
    parser.add_argument('-j', '--jobs', type=int, dest='job_count', metavar='N', default=1,
                        help='specify the maximum parallel job number')
    parser.add_argument('-m', '--save-readmap', action='store_true', dest='save_readmap',
                        help='output an readmap file')
    parser.add_argument('-s', '--single-ended', action='store_true', dest='single_ended',
                        help='specify whether the reads are single-ended')
    parser.add_argument('-b', '--bootstrap', type=int, dest='bootstrap', default=0,
                        help='specify the number of bootstrapped estimation')
    parser.add_argument('--device', type=int, default=0, help='GPU ordinal (default 0)')
    parser.add_argument('--seed', type=int, default=None,
                        help='seed of the bootstrap resampling (default: random)')
    parser.add_argument('--parse-threads', type=int, dest='parse_threads', default=None, metavar='N',
                        help='parse plain FASTQ files with N threads (default: up to 8; 0: one thread, '
                             'the batches of the reference)')
    add_strand_arguments(parser)
    add_length_model_arguments(parser)
    add_bias_argument(parser)
    add_gene_arguments(parser)


def add_many_subcommand_parser(subparsers):
    """Add the infer-many command: `infer` for many samples against one resident index."""
    parser = subparsers.add_parser(
        'infer-many', help='infer transcript abundance of many samples against one resident index',
        epilog='List the read files of all samples as arguments: every two files are one sample; with "-s" '
               '(single-ended reads) every file is one sample.  Sample NAME gets the folder output/NAME with '
               'the files that "infer" writes for it.')
    parser.add_argument('index_path', type=pathlib.Path, metavar='index',
                        help='specify a Seekmer index file')
    parser.add_argument('output_path', type=pathlib.Path, metavar='output',
                        help='specify a output folder')
    parser.add_argument('fastq_paths', type=pathlib.Path, metavar='fastq',
                        nargs='+', help='specify a FASTQ read file')
    parser.add_argument('-j', '--jobs', type=int, dest='job_count', metavar='N', default=1,
                        help='specify the maximum parallel job number')
    parser.add_argument('-s', '--single-ended', action='store_true', dest='single_ended',
                        help='specify whether the reads are single-ended')
    parser.add_argument('-b', '--bootstrap', type=int, dest='bootstrap', default=0,
                        help='specify the number of bootstrapped estimation')
    parser.add_argument('--device', type=int, default=0, help='GPU ordinal (default 0)')
    parser.add_argument('--seed', type=int, default=None,
                        help='seed of the bootstrap resampling, the same for every sample (default: random)')
    parser.add_argument('--names', type=str, default=None, metavar='A,B,C',
                        help='name the samples (default: each sample\'s first file name up to its first ".")')
    add_strand_arguments(parser)
    add_length_model_arguments(parser)
    add_bias_argument(parser)
    add_gene_arguments(parser)
    add_count_matrix_arguments(parser)
    add_barcode_arguments(parser)


def add_barcode_arguments(parser):
    """--barcodes and its companions: dest 'barcodes', 'barcode_file', 'barcode_start', 'barcode_mismatches',
    'min_units', 'umi_start', 'umi_length', 'umi_mismatches', and --discover-cells with 'discover_cells', 'barcode_length',
    'discover_keep_neighbours' (barcode_option checks the combinations once the arguments are parsed)."""
    parser.add_argument('--barcodes', type=pathlib.Path, dest='barcodes', default=None, metavar='WHITELIST',
                        help='the FASTQ files are ONE pooled sample: split it into the cells of this whitelist (a '
                             'barcode per line, optionally a tab and the cell\'s name) on the GPU; needs --barcode-file')
    parser.add_argument('--barcode-file', type=pathlib.Path, dest='barcode_file', default=None, metavar='FASTQ',
                        help='the barcode reads of the pooled sample, one per unit (with --barcodes)')
    parser.add_argument('--barcode-start', type=int, dest='barcode_start', default=None, metavar='N',
                        help='the barcode begins at base N of a barcode read (default 0)')
    parser.add_argument('--barcode-mismatches', type=int, dest='barcode_mismatches', default=None, choices=(0, 1),
                        help='substitutions a barcode may differ from its whitelist entry by (default 1)')
    parser.add_argument('--min-units', type=int, dest='min_units', default=None, metavar='N',
                        help='keep the cells with at least N assigned units (default 1)')
    parser.add_argument('--umi-length', type=int, dest='umi_length', default=None, metavar='L',
                        help='the barcode reads carry a UMI of L bases (1 to 16): inside a cell, count the reads of one '
                             'UMI and one equivalence class once (with --barcodes or --discover-cells; UMIs must be '
                             'equal letter for letter unless --umi-mismatches 1)')
    parser.add_argument('--umi-mismatches', type=int, dest='umi_mismatches', default=None, choices=(0, 1),
                        help='1: also remove a read when an EARLIER read of its cell has the same equivalence class and a '
                             'UMI one substitution away (default 0; with --umi-length)')
    parser.add_argument('--umi-start', type=int, dest='umi_start', default=None, metavar='N',
                        help='the UMI begins at base N of a barcode read (default 0; with --umi-length)')
    parser.add_argument('--discover-cells', type=int, dest='discover_cells', default=None, metavar='N',
                        help='instead of --barcodes: there is no whitelist, find the barcodes of about N expected cells in '
                             'the barcode reads on the GPU (a tenth of the count at rank N/100 is the threshold); needs '
                             '--barcode-length and --barcode-file')
    parser.add_argument('--barcode-length', type=int, dest='barcode_length', default=None, metavar='L',
                        help='a barcode is L bases long (1 to 32; with --discover-cells)')
    parser.add_argument('--discover-keep-neighbours', action='store_true', dest='discover_keep_neighbours',
                        help='keep a discovered barcode that is one substitution away from a larger one (default: it is '
                             'taken for a misreading, and its reads are corrected into the larger one)')


def barcode_option(parser, opts):
    """The parsed barcode options: a combination that cannot be is an argparse error; the defaults are filled in."""
    given = [flag for flag, key in (('--barcode-file', 'barcode_file'), ('--barcode-start', 'barcode_start'),
                                    ('--barcode-mismatches', 'barcode_mismatches'), ('--min-units', 'min_units'),
                                    ('--umi-length', 'umi_length'), ('--umi-start', 'umi_start'),
                                    ('--umi-mismatches', 'umi_mismatches'))
             if opts.get(key) is not None]
    discover = opts.get('discover_cells') is not None
    if opts.get('barcodes') is not None and discover:
        parser.error('one of --barcodes and --discover-cells: a whitelist, or cells found in the barcode reads')
    if not discover:
        if opts.get('barcodes') is not None and opts.get('barcode_length') is not None:
            parser.error('--barcode-length does not go with --barcodes: the whitelist gives the length')
        if opts.get('barcode_length') is not None:
            parser.error('--barcode-length goes with --discover-cells')
        if opts.get('discover_keep_neighbours'):             # (a flag: False when it is not given)
            parser.error('--discover-keep-neighbours goes with --discover-cells')
    if opts.get('barcodes') is None and not discover:
        if given:
            parser.error('%s goes with --barcodes' % given[0])
    else:
        flag = '--discover-cells' if discover else '--barcodes'
        if discover and opts['discover_cells'] < 1:
            parser.error('--discover-cells must be 1 or more')
        if discover and opts.get('barcode_length') is None:
            parser.error('--discover-cells needs the length of a barcode: --barcode-length L')
        if discover and not 1 <= opts['barcode_length'] <= mapper.MAX_BARCODE_LENGTH:
            parser.error('--barcode-length must be 1 to %d' % mapper.MAX_BARCODE_LENGTH)
        if opts.get('barcode_file') is None:
            parser.error('%s needs the barcode reads: --barcode-file FASTQ' % flag)
        if opts.get('names') is not None:
            parser.error('--names does not go with %s: the cells are named by %s'
                         % (flag, 'their barcodes' if discover else 'the whitelist'))
        if len(opts['fastq_paths']) != (1 if opts['single_ended'] else 2):
            parser.error('%s takes ONE pooled sample: two FASTQ files, or one with -s' % flag)
    if opts.get('barcode_start') is not None and opts['barcode_start'] < 0:
        parser.error('--barcode-start must be 0 or more')
    if opts.get('min_units') is not None and opts['min_units'] < 1:
        parser.error('--min-units must be 1 or more')
    if opts.get('umi_length') is not None and not 1 <= opts['umi_length'] <= mapper.MAX_UMI_LENGTH:
        parser.error('--umi-length must be 1 to %d' % mapper.MAX_UMI_LENGTH)
    if opts.get('umi_start') is not None and opts['umi_start'] < 0:
        parser.error('--umi-start must be 0 or more')
    if opts.get('umi_start') is not None and opts.get('umi_length') is None:
        parser.error('--umi-start goes with --umi-length')
    if opts.get('umi_mismatches') is not None and opts.get('umi_length') is None:
        parser.error('--umi-mismatches goes with --umi-length')
    for key, default in (('barcode_start', 0), ('barcode_mismatches', 1), ('min_units', 1), ('umi_start', 0), ('umi_length', 0),
                         ('umi_mismatches', 0)):
        if opts.get(key) is None:
            opts[key] = default
    return opts


def add_gene_arguments(parser):
    """--genes and --gene-map FILE: dest 'genes', 'gene_map' (gene_option makes the second imply the first)."""
    parser.add_argument('--genes', action='store_true', dest='genes',
                        help='also write gene-level tables: abundance.genes.tsv (sums per gene, and the reads that '
                             'belong to exactly one gene) from the genes the index was built with (one GPU)')
    parser.add_argument('--gene-map', type=pathlib.Path, dest='gene_map', default=None, metavar='FILE',
                        help='take the genes from FILE (transcript id, tab, gene id) instead; implies --genes')


def gene_option(opts):
    """The parsed options: --gene-map implies --genes -- unless --count-matrix or --matrix-only is given, which the map
    then serves: they need genes but do not switch the gene-level tables on.  --matrix-only and --count-molecules imply
    --count-matrix, --resolve-molecules implies --count-molecules, --distribute-molecules implies --resolve-molecules."""
    opts['resolve_molecules'] = bool(opts.get('resolve_molecules')) or bool(opts.get('distribute_molecules'))
    opts['count_molecules'] = bool(opts.get('count_molecules')) or bool(opts.get('resolve_molecules'))
    opts['count_matrix'] = bool(opts.get('count_matrix')) or bool(opts.get('matrix_only')) or bool(opts.get('count_molecules'))
    opts['genes'] = bool(opts.get('genes')) or (opts.get('gene_map') is not None and not opts['count_matrix'])
    return opts


def add_count_matrix_arguments(parser):
    """--count-matrix, --matrix-only, --count-molecules, --resolve-molecules and --distribute-molecules: dest
    'count_matrix', 'matrix_only', 'count_molecules', 'resolve_molecules', 'distribute_molecules' (gene_option makes the
    second and the third imply the first, the fourth the third and the fifth the fourth)."""
    parser.add_argument('--count-matrix', action='store_true', dest='count_matrix',
                        help='also write output/counts/: the sparse gene x cell matrix of the units that lie inside one '
                             'gene (matrix.mtx, genes.tsv, cells.tsv, matrix.npz), made on the GPU; the genes are the '
                             'index\'s or those of --gene-map')
    parser.add_argument('--matrix-only', action='store_true', dest='matrix_only',
                        help='write the count matrix, samples.tsv and the barcodes.* files only: stop after mapping (and '
                             'UMI collapse), run no EM, write no folder per sample; implies --count-matrix, refuses -b, '
                             '--bias and --genes')
    parser.add_argument('--count-molecules', action='store_true', dest='count_molecules',
                        help='also write counts/molecules.mtx and counts/molecules.npz: per gene and cell the number of '
                             'DISTINCT UMIs among the units inside that gene, where matrix.mtx counts a molecule once per '
                             'equivalence class its reads fell into; implies --count-matrix, needs --umi-length')
    parser.add_argument('--resolve-molecules', action='store_true', dest='resolve_molecules',
                        help='also write counts/molecules.resolved.mtx, .npz and .tsv: one gene per UMI and cell, named by '
                             'the intersection of the gene sets of the classes the UMI was seen in; multi-gene, unnamed and '
                             'colliding UMIs are tallied per cell; implies --count-molecules, needs --umi-length')
    parser.add_argument('--distribute-molecules', action='store_true', dest='distribute_molecules',
                        help='also write counts/molecules.em.mtx, .npz and .tsv: the multi-gene UMIs of --resolve-molecules '
                             'shared out among the genes of their intersection (16 at most) by a small EM per cell, values in '
                             'molecules; implies --resolve-molecules, needs --umi-length')


def add_bias_argument(parser):
    """--bias (kallisto's flag): dest 'bias'."""
    parser.add_argument('--bias', action='store_true', dest='bias',
                        help='correct the effective lengths for sequence bias: the hexamers the aligned reads start '
                             'with against those the expressed transcripts offer, then a second EM (one GPU)')


def add_length_model_arguments(parser):
    """-l/--fragment-length MEAN and --sd SD (kallisto's -l and -s; -s is --single-ended here): both or
    neither, which length_model_option checks once the arguments are parsed."""
    parser.add_argument('-l', '--fragment-length', type=float, dest='fragment_length', default=None, metavar='MEAN',
                        help='take the effective lengths from a normal fragment-length model with this mean '
                             'instead of the observed histogram (with --sd; needed for single-ended reads)')
    parser.add_argument('--sd', type=float, dest='sd', default=None, metavar='SD',
                        help='standard deviation of the fragment-length model (with --fragment-length)')


def length_model_option(parser, opts):
    """The parsed options' 'fragment_length' and 'sd' -> 'length_model' (None | (mean, sd)); one without
    the other, or a model that mapper.fragment_length_weights refuses, is an argparse error."""
    mean, sd = opts.pop('fragment_length', None), opts.pop('sd', None)
    if (mean is None) != (sd is None):
        parser.error('-l/--fragment-length and --sd go together: give both or neither')
    opts['length_model'] = None
    if mean is not None:
        try:
            mapper.fragment_length_weights(mean, sd)
        except ValueError as error:
            parser.error(str(error))
        opts['length_model'] = (mean, sd)
    return opts


def add_strand_arguments(parser):
    """--fr-stranded / --rf-stranded (kallisto's flags), one at most: dest 'strand'."""
    group = parser.add_mutually_exclusive_group()
    group.add_argument('--fr-stranded', action='store_const', const='fr', dest='strand', default=None,
                       help='strand-specific reads: mate 1 (or the single read) in the transcript\'s orientation')
    group.add_argument('--rf-stranded', action='store_const', const='rf', dest='strand', default=None,
                       help='strand-specific reads: mate 1 (or the single read) antisense to the transcript')
