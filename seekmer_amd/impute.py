"""Single-cell imputation -- the `seekmer.impute` surface (reference:
seekmer/impute.py:1-252) over the MI355X engine.  All cells are mapped in shared
launches into one device-resident class table that keeps their classes apart
(`mapper.map_sample_set`; one table per cell, `mapper.map_multiple_samples`,
outside the regime of SAMPLE_SET_* and with SKM_IMPUTE_PER_CELL=1), the cells'
fragment-length histograms are pooled, every cell is quantified once, a
cell-by-cell weight matrix is derived from the gene-level abundances, and every
cell is quantified again on the weighted blend of all cells' class tables.

What the engine changes: the blended problem has ONE class structure (the
concatenation of all cells' classes, impute.py:243-247) and only the class
counts differ from cell to cell (:248-252), so its two CSR views are built on
the GPU once.  The second round is then many EM problems on one structure:
the cells' blended counts are made on the device and eight cells at a time run
side by side in the batched EM (`_QuantHandle.em_blend`), each with the steps
and the bits of `set_counts` + the EM kernels for that cell alone -- the loop
that SKM_IMPUTE_SERIAL=1 still selects.  The first round -- the cells' own
tables, whose structures differ -- can run as one block-diagonal problem in
shared launches (`first_round`; SKM_SET_QUANT_SERIAL=1 keeps the loop, and so
does SKM_IMPUTE_SERIAL=1: with it both rounds run one cell at a time).
The arithmetic that decides results is the reference's, cited per function.
"""
import logging
import os
import pathlib

import numpy

from . import common
from . import infer
from . import mapper

__all__ = ('add_subcommand_parser', 'run')

_LOG = logging.getLogger(__name__)


def run(index_path, output_path, fastq_paths, job_count, single_ended, debug, power,
        device=0, seed=None, strand=None, length_model=None, **__):
    """The entrypoint of the imputation module (seekmer/impute.py:54-125).
    `seed` fixes the 2-means split of the weights (the reference leaves it to
    numpy's global generator).  strand: None, 'fr' or 'rf' for every cell (mapper.MapResult).
    length_model: None, or (mean, sd) of --fragment-length / --sd: every cell's effective lengths come
    from that model instead of the pooled histogram (mapper.fragment_length_weights)."""
    import pandas
    mapper.strand_mode(strand)
    length_model, _ = mapper.length_model_weights(length_model)
    for path in fastq_paths:
        if not pathlib.Path(path).exists():
            raise ValueError(f'invalid FastQ file: {path}')
    try:
        output_path.mkdir(parents=True)
    except FileExistsError:
        _LOG.warning('The output folder exists. Overriding...')
    _LOG.info('Inferring transcript abundance')
    infer._log_length_model(length_model, single_ended)
    index = common.KMerIndex.load(index_path)
    _LOG.info('Mapping all reads')
    width = 1 if single_ended else 2
    groups = [tuple(fastq_paths[i:i + width]) for i in range(0, len(fastq_paths) - width + 1, width)]
    # (a cell's reads: plain files are parsed straight to the mapper's 2-bit codes by the thread that
    # maps the cell -- one pass, a third of the bytes over PCIe; compressed ones through the ASCII reader)
    feeders = [common.PackedReadFeeder(list(group), paired=not single_ended)
               if common.PackedReadFeeder.eligible(group) else common.NativeReadFeeder(list(group), paired=not single_ended)
               for group in groups]
    if use_sample_set(groups):
        # (the set's one histogram IS the pooled one: every summary carries it)
        sample_set = mapper.map_sample_set(index, feeders, job_count=1 if debug else max(1, job_count),
                                           device=device, strand=strand, length_model=length_model)
        _LOG.info('Mapped all reads.')
        summaries = sample_set.summarize()
    else:
        sample_set = None
        map_results = mapper.map_multiple_samples(index, feeders, job_count=job_count, debug=debug,
                                                  device=device, strand=strand, length_model=length_model)
        _LOG.info('Mapped all reads.')
        pool_fragment_lengths(map_results)
        summaries = [result.summarize() for result in map_results]
    _LOG.info('First round quantification...')
    base = first_round(summaries, sample_set, device=device)
    del sample_set
    if power is not None:
        _LOG.info('Weighting cells.')
        weight = cell_weights(index, base, output_path, seed=seed)
        weight **= power
        _LOG.info('Second round quantification...')
        columns = requantify_blend(summaries, weight, device=device)
    else:
        columns = list(base)
    names = [str(group[0]) for group in groups]          # one column per cell, named by its first file
    table = pandas.DataFrame(dict(zip(names, columns)),
                             index=numpy.char.decode(index.transcripts['transcript_id']))
    _LOG.info('Writing results to %s...', output_path)
    table.to_csv(output_path / 'tpm.csv')
    return table


# Where the cells are mapped through one sample set (mapper.map_sample_set) instead of a mapper per cell.
# Measured ("Sample sets"; profiles/sample_set_ab.log: the mapping stage alone, packed reads in
# host memory to exported tables, against the parent commit's map_multiple_samples on the same GPU): the set
# is 7 x ahead at 64 and at 512 cells of 20 k pairs, 2.1 x at 8 cells, 1.7 x at 4, 1.3 x at 64 cells of 50 k
# pairs on the 190 k-transcript index, 1.2 x at 4 and at 2 cells of 2 M pairs; at 2 cells of 20 k pairs and at
# 4 cells of 8 M pairs the two are level within their spread.  No shape was found at which the mapper per
# cell is ahead, so the bounds are not a crossover.  One cell has nothing to share.  The size bound is where
# the gain was last seen (2 M pairs a cell): the set parses a cell completely before it adds it, so a cell's
# packed reads must fit in host memory, which the mapper per cell, fed piece by piece, does not ask for --
# and what the set buys, filled launches, a cell of that size has by itself.  Reading and parsing the files
# is outside what was measured.  SKM_IMPUTE_PER_CELL=1 (exactly that value, looked up at every call)
# selects the mapper per cell whatever the shape.
SAMPLE_SET_MIN_CELLS = 2
SAMPLE_SET_MAX_CELL_BYTES = 640 << 20     # the files of the largest cell: what 2 M pairs of 2 x 75 bases with short names come to
SAMPLE_SET_COMPRESSED_RATIO = 4           # a compressed file counts this many times its size (an estimate of its text; not measured)


# Where the first round -- every cell's own table -- runs in shared EM launches (mapper.SampleSet.quantify
# for cells mapped through a set, infer.quantify_tables otherwise) instead of infer.quantify() cell by cell.
# Measured ("Many class tables in shared EM launches"; profiles/set_quant_ab.log: the first round
# from mapped tables, the forms alternating in one process, against the parent commit's loop on the same GPU
# right after; ms for all cells, the later repetitions of three): 64 cells of 20 k pairs on 944 transcripts
# 10.6-10.9 (set) and 6.7-6.8 (tables) against 112.6-119.8 (10 x, 17 x); 512 such cells 75.1-75.9 and
# 56.8-59.5 against 914.4-937.6 (12 x, 16 x); 8 such cells 3.8-3.9 against 14.6-14.7 (3.8 x); 64 cells of
# 50 k pairs on 190 402 transcripts (2.63 M classes in all) 180.8-182.6 and 176.8-179.4 against 227.4-238.1
# (1.3 x: a gap of 50 ms against a spread of 11).  At 2 cells of 20 k pairs the forms are level (3.4-3.5
# against 3.6 ms), 3 to 7 cells were not run: the loop stays below 8.  The rule is those points and what lies
# between them, nothing rounded up: on tables of up to 944 transcripts from 8 cells and up to the 1 773 517
# classes in all of the 512 cells; on larger tables, up to the 190 402 transcripts and 2 629 763 classes in all
# that were measured, only from the 64 cells that were measured there -- fewer cells on such a table were not
# run, and the gain shrinks both with fewer cells (10 x to 3.8 x on the small table) and with more
# transcripts (10 x to 1.3 x at 64 cells): the shared launches step the whole table, the loop's EM runs in
# component tiles where it can.
SET_QUANT_MIN_SAMPLES = 8
SET_QUANT_SMALL_TRANSCRIPTS = 944
SET_QUANT_SMALL_CLASSES = 1_773_517
SET_QUANT_LARGE_MIN_SAMPLES = 64
SET_QUANT_MAX_TRANSCRIPTS = 190_402
SET_QUANT_MAX_CLASSES = 2_629_763


def use_set_quant(n_samples, n_tx, n_classes):
    """The rule of first_round() and of infer.run_many: samples, transcripts, classes of all samples together.
    SKM_SET_QUANT_SERIAL=1 (exactly that value, looked up at every call) selects the loop over the samples
    whatever the shape."""
    if os.environ.get('SKM_SET_QUANT_SERIAL') == '1':
        return False
    if n_samples >= SET_QUANT_MIN_SAMPLES and n_tx <= SET_QUANT_SMALL_TRANSCRIPTS and n_classes <= SET_QUANT_SMALL_CLASSES:
        return True
    return n_samples >= SET_QUANT_LARGE_MIN_SAMPLES and n_tx <= SET_QUANT_MAX_TRANSCRIPTS and n_classes <= SET_QUANT_MAX_CLASSES


def first_round(summaries, sample_set=None, device=0):
    """quantify() of every cell's own table (seekmer/impute.py:98): f8[cells, n_tx].  Inside the regime of
    use_set_quant the cells run in shared EM launches -- from the set's resident table when they were mapped
    through one, from the summaries otherwise -- bit for bit what the loop gives.  SKM_IMPUTE_SERIAL=1, the
    switch that keeps the second round one cell at a time, keeps this round so as well."""
    if summaries and os.environ.get('SKM_IMPUTE_SERIAL') != '1' \
            and use_set_quant(len(summaries), summaries[0].effective_lengths.size,
                                   sum(summary.class_count.size for summary in summaries)):
        if sample_set is not None:
            return numpy.asarray(sample_set.quantify())
        return numpy.asarray(infer.quantify_tables(summaries, device=device))
    return numpy.asarray([infer.quantify(summary) for summary in summaries])


def cell_text_bytes(group):
    """What the rule takes for the FASTQ text of one cell (its tuple of paths): the sizes of plain files,
    SAMPLE_SET_COMPRESSED_RATIO times those of compressed ones.  A path that is no file counts nothing
    (the reader says what is wrong with it)."""
    total = 0
    for path in map(pathlib.Path, group):
        if path.is_file():
            plain = common.PackedReadFeeder.eligible([path])
            total += path.stat().st_size * (1 if plain else SAMPLE_SET_COMPRESSED_RATIO)
    return total


def use_sample_set(groups):
    """The rule of run(): groups = every cell's tuple of FASTQ paths."""
    if os.environ.get('SKM_IMPUTE_PER_CELL') == '1' or len(groups) < SAMPLE_SET_MIN_CELLS:
        return False
    return max(cell_text_bytes(group) for group in groups) <= SAMPLE_SET_MAX_CELL_BYTES


def pool_fragment_lengths(map_results):
    """Single cells usually share one sequencing batch: every cell gets the sum
    of all cells' fragment-length counts (seekmer/impute.py:128-146).  The
    histograms live on the GPU; each one receives what the others counted."""
    counts = [result.fragment_length_counts for result in map_results]
    total = numpy.sum(counts, axis=0, dtype=numpy.int64) if counts else None
    for result, own in zip(map_results, counts):
        result.merge_fragment_lengths(total - own)


def gene_matrix(index, tpm_matrix):
    """Cell-by-gene abundance, truncated to integers as the reference's i8
    matrix does on assignment, genes named b'' dropped (impute.py:205-211)."""
    genes, gene_of_transcript = numpy.unique(index.transcripts['gene_id'], return_inverse=True)
    tpm_matrix = numpy.asarray(tpm_matrix, dtype='f8')
    # the transcripts of a gene side by side (stable: in transcript order), so that each gene is
    # one column slice and its row sums are numpy's own, as in the reference's masked .sum(axis=1)
    order = numpy.argsort(gene_of_transcript, kind='stable')
    by_gene = tpm_matrix[:, order]
    bounds = numpy.searchsorted(gene_of_transcript[order], numpy.arange(len(genes) + 1))
    matrix = numpy.zeros((len(tpm_matrix), len(genes)), dtype='i8')
    for gene in range(len(genes)):
        block = numpy.ascontiguousarray(by_gene[:, bounds[gene]:bounds[gene + 1]])
        matrix[:, gene] = block.sum(axis=1)          # (float -> i8 on assignment: truncation)
    named = genes != b''
    return matrix[:, named], genes[named]


def cell_weights(index, tpm_matrix, output_path=None, seed=None):
    """Cell-by-cell weights (seekmer/impute.py:187-226): Pearson correlation of
    the integer gene-level abundances; the off-diagonal, defined correlations
    are split in two by 1-D 2-means and only those of the upper cluster keep
    their value, everything else (and every NaN) becomes 0."""
    import pandas
    import sklearn.cluster
    matrix, genes = gene_matrix(index, tpm_matrix)
    if output_path is not None:
        pandas.DataFrame(matrix.T, index=numpy.char.decode(genes)).to_csv(
            output_path / 'initial_gene_table.csv')
    with numpy.errstate(invalid='ignore', divide='ignore'):
        weights = numpy.corrcoef(matrix)
    weights = numpy.atleast_2d(weights)
    informative = weights[(weights == weights) & (weights != 1.0)]
    split = sklearn.cluster.KMeans(2, random_state=seed)
    split.fit(informative[:, None])
    weights[weights != weights] = 0.0
    upper = split.predict(weights.reshape(-1, 1)) == split.cluster_centers_.argmax()
    weights = numpy.where(upper.reshape(weights.shape), weights, 0.0)
    if output_path is not None:
        pandas.DataFrame(weights).to_csv(output_path / 'weight.csv')
    return weights


def blend_structure(summaries):
    """(offsets, targets) of the blended problem: all cells' classes one after the other."""
    sizes = [numpy.bincount(s.class_map[0].astype(numpy.int64), minlength=s.class_count.size)
             for s in summaries]
    offsets = numpy.zeros(sum(s.size for s in sizes) + 1, dtype=numpy.int64)
    numpy.cumsum(numpy.concatenate(sizes), out=offsets[1:])
    targets = numpy.concatenate([s.class_map[1] for s in summaries]).astype(numpy.int32)
    return offsets, targets


def blend(summaries, weight):
    """The blended problem of seekmer/impute.py:229-252 in CSR form: (offsets,
    targets) = all cells' classes one after the other; counts[i] = for cell i
    the concatenation over cells j of count_j * weight[i, j] * total_i /
    total_j (totals = sums of the cells' own class counts)."""
    for summary in summaries:
        if summary.class_count.size == 0:
            raise ValueError('a cell without aligned reads cannot be blended')   # max() of nothing, :241
    offsets, targets = blend_structure(summaries)
    own = [s.class_count for s in summaries]
    counts = []
    for i, summary in enumerate(summaries):
        total = summary.class_count.sum()
        counts.append(numpy.concatenate([c * w * total / c.sum() for c, w in zip(own, weight[i, :])]))
    return offsets, targets, counts


def blend_sources(summaries):
    """What the device needs to make blend()'s counts itself: (own, class_cell, cell_total) = all
    cells' own class counts one after the other, the cell every class of the concatenation came
    from, and each cell's own count sum (c.sum() of blend()).  counts[i][k] of blend() is
    ((own[k] * weight[i, class_cell[k]]) * cell_total[i]) / cell_total[class_cell[k]]."""
    own = numpy.concatenate([s.class_count for s in summaries]).astype('f8')
    class_cell = numpy.repeat(numpy.arange(len(summaries), dtype=numpy.int32),
                              [s.class_count.size for s in summaries])
    cell_total = numpy.asarray([s.class_count.sum() for s in summaries], dtype='f8')
    return own, class_cell, cell_total


# Where the second round takes the batched EM: the regime in which it was measured ahead of the loop over
# the cells ("Many count vectors on one class table"; profiles/impute_many_ab.log).  Below
# eight cells -- one full working set -- four cells took 6.9 ms batched against 6.0 ms one by one (a
# working-set step costs about five single-problem steps and half the places are empty), eight took 10 ms
# against 41.  The other two bounds are the largest blended structure and transcript count measured (64
# cells x 50 k pairs on 190 402 transcripts, 2.63 M blended classes: 7.65 ms per cell against 16.5): the
# batched EM steps the whole table, the loop's single-problem EM runs in component tiles where it can, and
# how the two compare on larger tables is not known.
BATCH_MIN_CELLS = 8
BATCH_MAX_CLASSES = 3_000_000
BATCH_MAX_TRANSCRIPTS = 200_000


def requantify_blend(summaries, weight, device=0):
    """quantify() of every cell's blended table (seekmer/impute.py:101-108): one quantification
    handle for the shared class structure; the cells' blended counts are made on the device and the
    cells run eight at a time in the batched EM (_QuantHandle.em_blend), bit for bit what the loop
    over the cells gives.  That loop remains for SKM_IMPUTE_SERIAL=1, for cells whose effective
    lengths differ (they do not after pool_fragment_lengths) and outside the regime in which the batched
    form was measured ahead (BATCH_MIN_CELLS, BATCH_MAX_CLASSES, BATCH_MAX_TRANSCRIPTS)."""
    lengths = [summary.effective_lengths.astype('f8') for summary in summaries]
    if os.environ.get('SKM_IMPUTE_SERIAL') == '1' or len(summaries) < BATCH_MIN_CELLS \
            or sum(summary.class_count.size for summary in summaries) > BATCH_MAX_CLASSES \
            or lengths[0].size > BATCH_MAX_TRANSCRIPTS \
            or any(not numpy.array_equal(lengths[0], other) for other in lengths[1:]):
        return _requantify_blend_serial(summaries, weight, device)
    for summary in summaries:
        if summary.class_count.size == 0:
            raise ValueError('a cell without aligned reads cannot be blended')   # max() of nothing, :241
    offsets, targets = blend_structure(summaries)
    own, class_cell, cell_total = blend_sources(summaries)
    n_tx = lengths[0].size
    x = numpy.ones(n_tx, dtype='f8') / lengths[0]                       # infer.py:116-119
    x /= x.sum()
    handle = infer._QuantHandle.from_csr(n_tx, offsets, targets, own, device)
    try:
        columns, _, _ = handle.em_blend(class_cell, numpy.asarray(weight, dtype='f8'), cell_total, x, lengths[0], tpm=True)
    finally:
        handle.close()
    return list(columns)


def _requantify_blend_serial(summaries, weight, device=0):
    """The second round one cell at a time: the cell's counts swapped in for each run."""
    offsets, targets, counts = blend(summaries, weight)
    n_tx = summaries[0].effective_lengths.size
    handle = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts[0], device)
    columns = []
    try:
        for summary, cell_counts in zip(summaries, counts):
            lengths = summary.effective_lengths.astype('f8')
            x = numpy.ones(n_tx, dtype='f8') / lengths                  # infer.py:116-119
            x /= x.sum()
            handle.set_counts(cell_counts)
            x, _ = handle.em(x, lengths)
            columns.append(infer._tpm(x))
    finally:
        handle.close()
    return columns


def add_subcommand_parser(subparsers):
    """Add an impute command to the subparsers (seekmer/impute.py:18-51)."""
    parser = subparsers.add_parser(
        'impute', help='impute transcript abundance for single-cell data',
        epilog='Demultiplex the read files first and list them as arguments: every two files are one '
               'cell; with "-s" (single-ended reads) every file is one cell.')
    parser.add_argument('index_path', type=pathlib.Path, metavar='index',
                        help='specify a Seekmer index file')
    parser.add_argument('output_path', type=pathlib.Path, metavar='output',
                        help='specify a output folder')
    parser.add_argument('fastq_paths', type=pathlib.Path, metavar='fastq', nargs='+',
                        help='specify a FASTQ read file')
    parser.add_argument('-j', '--jobs', type=int, dest='job_count', metavar='N', default=1,
                        help='specify the maximum parallel job number')
    parser.add_argument('-p', '--power', type=int, dest='power', metavar='P', default=16,
                        help='specify the power of the weight matrix')
    parser.add_argument('-m', '--save-readmap', action='store_true', dest='save_readmap',
                        help='output an readmap file')
    parser.add_argument('-s', '--single-ended', action='store_true', dest='single_ended',
                        help='specify whether the reads are single-ended')
    parser.add_argument('--device', type=int, default=0, help='GPU ordinal (default 0)')
    parser.add_argument('--seed', type=int, default=None,
                        help='seed of the 2-means split of the cell weights (default: random)')
    infer.add_strand_arguments(parser)
    infer.add_length_model_arguments(parser)
