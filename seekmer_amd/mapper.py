"""Read mapping -- the `seekmer.mapper` surface (reference: seekmer/mapper.py,
seekmer/_mapper.pyx:31-105) over the MI355X engine.

``MapResult`` is backed by one device-resident mapper handle: the
equivalence-class counter and the fragment-length histogram live in HBM and
are materialised as ``collections.Counter`` / ``numpy`` objects only when the
attributes are read.  ``ReadMapper(index, map_result)(reads_iterator)`` packs
each batch and hands it to ``skm_mapper_map_batch``; there is no CPU mapping
path.

``SampleSet`` (``map_sample_set``) is the form for many small samples -- the
cells of ``impute``: one handle maps all samples' units in shared launches
into one table whose classes are (sample, tuple) and hands back every
sample's own table, bit for bit what a ``MapResult`` per sample gives.
"""
import collections
import ctypes
import logging
import multiprocessing.pool
import os
import queue
import threading

import numpy

from . import _native
from .common import PackedReadFeeder, PackedReads, ReadBatch, decompress_and_open

__all__ = ('BarcodeCensus', 'BarcodeTable', 'DEMUX_CHUNK_UNITS', 'MAX_FRAGMENT_LENGTH', 'MapResult', 'ReadMapper', 'SampleSet',
           'SummarizedResult', 'discover_barcodes', 'fragment_length_weights', 'group_units', 'map_barcoded', 'map_reads',
           'map_multiple_samples', 'map_sample_set', 'read_whitelist')

_LOG = logging.getLogger(__name__)

MAX_FRAGMENT_LENGTH = 2000          # seekmer/_mapper.pyx:18-20

EPS = numpy.finfo('f4').eps

STRAND_MODES = {None: _native.SKM_STRAND_NONE, 'fr': _native.SKM_STRAND_FR, 'rf': _native.SKM_STRAND_RF}


def strand_mode(strand):
    """None | 'fr' | 'rf' -> SKM_STRAND_* (include/seekmer_hip.h, skm_mapper_set_strand)"""
    if strand not in STRAND_MODES:
        raise ValueError('strand must be None, \'fr\' or \'rf\', not %r' % (strand,))
    return STRAND_MODES[strand]


def fragment_length_weights(mean, sd):
    """The fragment-length model of --fragment-length MEAN --sd SD: f8[2000], a normal density cut to
    the bins 1..1999 and normalised.  These weights stand in for fld / fld.sum() in the effective-length
    rule (seekmer/mapper.py:134-141).  They are made here, once, on the host: the device reads them as
    they are (skm_effective_lengths_weights), so it and a numpy model of the rule share the same p."""
    mean, sd = float(mean), float(sd)
    if not (numpy.isfinite(mean) and numpy.isfinite(sd) and 0 < mean < MAX_FRAGMENT_LENGTH and sd > 0):
        raise ValueError('a fragment-length model needs 0 < mean < %d and sd > 0, both finite, not (%r, %r)'
                         % (MAX_FRAGMENT_LENGTH, mean, sd))
    i = numpy.arange(float(MAX_FRAGMENT_LENGTH))
    w = numpy.exp(-0.5 * ((i - mean) / sd) ** 2)
    w[0] = 0
    total = w.sum()
    if not total > 0:
        raise ValueError('the fragment-length model (%r, %r) has no weight on any length 1..%d'
                         % (mean, sd, MAX_FRAGMENT_LENGTH - 1))
    return w / total


def length_model_weights(length_model):
    """None | (mean, sd) -> (None | (float mean, float sd), None | the model's weights)"""
    if length_model is None:
        return None, None
    mean, sd = length_model
    weights = numpy.ascontiguousarray(fragment_length_weights(mean, sd), dtype='f8')
    return (float(mean), float(sd)), weights


def gene_numbers(tx_gene, n_tx):
    """tx_gene as the contiguous int32[n_tx] the native gene calls take (ValueError for another length)"""
    tx_gene = numpy.ascontiguousarray(tx_gene, dtype=numpy.int32)
    if tx_gene.shape != (n_tx,):
        raise ValueError('a gene number for each of the %d transcripts, not %s' % (n_tx, tx_gene.shape))
    return tx_gene if tx_gene.size else numpy.zeros(1, dtype=numpy.int32)[:0]


def read_gene_matrix(handle):
    """The arrays of a skm_gene_matrix handle (indptr, indices, data, other), copied home; the handle is destroyed."""
    try:
        shape = [ctypes.c_int64(0) for _ in range(3)]
        _native.check(_native.hip().skm_gene_matrix_shape(handle, *[ctypes.byref(word) for word in shape]))
        n_samples, _, nnz = [int(word.value) for word in shape]
        indptr = numpy.zeros(n_samples + 1, dtype=numpy.int64)
        indices = numpy.zeros(max(nnz, 1), dtype=numpy.int32)
        data = numpy.zeros(max(nnz, 1), dtype=numpy.int64)
        other = numpy.zeros((max(n_samples, 1), 2), dtype=numpy.int64)
        _native.check(_native.hip().skm_gene_matrix_read(
            handle, _native.ptr(indptr, _native.c_i64p), _native.ptr(indices, _native.c_i32p),
            _native.ptr(data, _native.c_i64p), _native.ptr(other, _native.c_i64p)))
        return indptr, indices[:nnz], data[:nnz], other[:n_samples]
    finally:
        _native.hip().skm_gene_matrix_destroy(handle)


def molecule_matrix(sample, gene, umi, n_samples, n_genes, device=0):
    """(indptr, indices, data, other) of the molecule matrix of the triples (sample[i], gene[i], umi[i]): data counts the
    distinct UMIs of every (sample, gene), other is all zero (skm_gene_matrix_from_molecules: the sort, head and fill
    steps of DESIGN.md section 4, "Molecule matrix", on the device).  A sample outside [0, n_samples) or a gene
    outside [0, n_genes) raises."""
    sample = numpy.ascontiguousarray(sample, dtype=numpy.int32)
    gene = numpy.ascontiguousarray(gene, dtype=numpy.int32)
    umi = numpy.ascontiguousarray(umi, dtype=numpy.uint32)
    if sample.ndim != 1 or gene.shape != sample.shape or umi.shape != sample.shape:
        raise ValueError('sample, gene and umi are three arrays of one length')
    handle = ctypes.c_void_p()
    n = int(sample.size)
    _native.check(_native.hip().skm_gene_matrix_from_molecules(
        int(device), n, _native.ptr(sample, _native.c_i32p) if n else None, _native.ptr(gene, _native.c_i32p) if n else None,
        _native.ptr(umi, _native.c_u32p) if n else None, int(n_samples), int(n_genes), ctypes.byref(handle)))
    return read_gene_matrix(handle)


def read_resolved_matrix(handle):
    """(indptr, indices, data, tally int64[n_samples, 5]) of a handle that holds resolved molecules, copied home; the
    handle is destroyed.  tally[s] = (resolved, rescued, multi-gene, unnamed, collision)."""
    shape = ctypes.c_int64(0)
    tally = None
    try:
        _native.check(_native.hip().skm_gene_matrix_shape(handle, ctypes.byref(shape), None, None))
        tally = numpy.zeros((max(int(shape.value), 1), 5), dtype=numpy.int64)
        _native.check(_native.hip().skm_gene_matrix_read_tally(handle, _native.ptr(tally, _native.c_i64p)))
    except Exception:
        _native.hip().skm_gene_matrix_destroy(handle)
        raise
    indptr, indices, data, _ = read_gene_matrix(handle)
    return indptr, indices, data, tally[:int(shape.value)]


def resolved_molecule_matrix(class_offsets, class_targets, class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes,
                             device=0):
    """(indptr, indices, data, tally) of the molecules (mol_class[i], mol_umi[i]) resolved to one gene per (sample, UMI):
    the classes are a CSR (class_offsets, class_targets) with a sample each, the distinct classes of a sample's
    molecules with one UMI form a group, and the intersection of their gene sets is the group's verdict
    (skm_gene_matrix_from_molecule_classes: the sort, group, resolve and fill steps of DESIGN.md section 4, "Resolved
    molecules", on the device).  Two molecules with the same class and UMI count as one.  A class index, a sample or
    a transcript id out of range and an empty class raise."""
    class_offsets = numpy.ascontiguousarray(class_offsets, dtype=numpy.int64)
    class_targets = numpy.ascontiguousarray(class_targets, dtype=numpy.int32)
    class_sample = numpy.ascontiguousarray(class_sample, dtype=numpy.int32)
    mol_class = numpy.ascontiguousarray(mol_class, dtype=numpy.int32)
    mol_umi = numpy.ascontiguousarray(mol_umi, dtype=numpy.uint32)
    tx_gene = numpy.ascontiguousarray(tx_gene, dtype=numpy.int32)
    n_classes = int(class_sample.size)
    if class_offsets.shape != (n_classes + 1,) or mol_class.ndim != 1 or mol_umi.shape != mol_class.shape:
        raise ValueError('class_offsets[n_classes + 1] beside class_sample[n_classes]; mol_class and mol_umi of one length')
    if n_classes and class_targets.size != class_offsets[-1]:
        raise ValueError('class_targets holds %d ids, class_offsets ends at %d' % (class_targets.size, class_offsets[-1]))
    handle = ctypes.c_void_p()
    n = int(mol_class.size)
    _native.check(_native.hip().skm_gene_matrix_from_molecule_classes(
        int(device), n_classes, _native.ptr(class_offsets, _native.c_i64p),
        _native.ptr(class_targets, _native.c_i32p) if class_targets.size else None,
        _native.ptr(class_sample, _native.c_i32p) if n_classes else None, n,
        _native.ptr(mol_class, _native.c_i32p) if n else None, _native.ptr(mol_umi, _native.c_u32p) if n else None,
        int(n_samples), int(tx_gene.size), int(n_genes), _native.ptr(tx_gene, _native.c_i32p) if tx_gene.size else None,
        ctypes.byref(handle)))
    return read_resolved_matrix(handle)


def read_distributed_matrix(handle):
    """(indptr, indices, data float64[nnz], tally int64[n_samples, 8], to_unnamed float64[n_samples]) of a handle that
    holds distributed molecules, copied home; the handle is destroyed.  tally[s] = (resolved, distributed, wide, unnamed,
    collision, rows, steps, capped)."""
    try:
        shape = [ctypes.c_int64(0) for _ in range(3)]
        _native.check(_native.hip().skm_gene_matrix_shape(handle, *[ctypes.byref(word) for word in shape]))
        n_samples, _, nnz = [int(word.value) for word in shape]
        indptr = numpy.zeros(n_samples + 1, dtype=numpy.int64)
        indices = numpy.zeros(max(nnz, 1), dtype=numpy.int32)
        data = numpy.zeros(max(nnz, 1), dtype=numpy.float64)
        tally = numpy.zeros((max(n_samples, 1), 8), dtype=numpy.int64)
        to_unnamed = numpy.zeros(max(n_samples, 1), dtype=numpy.float64)
        _native.check(_native.hip().skm_gene_matrix_read(
            handle, _native.ptr(indptr, _native.c_i64p), _native.ptr(indices, _native.c_i32p), None, None))
        _native.check(_native.hip().skm_gene_matrix_read_weights(handle, _native.ptr(data, _native.c_f64p)))
        _native.check(_native.hip().skm_gene_matrix_read_em(
            handle, _native.ptr(tally, _native.c_i64p), _native.ptr(to_unnamed, _native.c_f64p)))
        return indptr, indices[:nnz], data[:nnz], tally[:n_samples], to_unnamed[:n_samples]
    finally:
        _native.hip().skm_gene_matrix_destroy(handle)


def distributed_molecule_matrix(class_offsets, class_targets, class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes,
                                max_steps=1000, device=0):
    """(indptr, indices, data, tally, to_unnamed) of the molecules (mol_class[i], mol_umi[i]) with the multi-gene groups
    shared out among their genes: the arguments and checks of resolved_molecule_matrix, the steps of DESIGN.md section
    4, "Distributed molecules", on the device with max_steps EM steps per sample at most
    (skm_gene_matrix_from_molecule_sets)."""
    class_offsets = numpy.ascontiguousarray(class_offsets, dtype=numpy.int64)
    class_targets = numpy.ascontiguousarray(class_targets, dtype=numpy.int32)
    class_sample = numpy.ascontiguousarray(class_sample, dtype=numpy.int32)
    mol_class = numpy.ascontiguousarray(mol_class, dtype=numpy.int32)
    mol_umi = numpy.ascontiguousarray(mol_umi, dtype=numpy.uint32)
    tx_gene = numpy.ascontiguousarray(tx_gene, dtype=numpy.int32)
    n_classes = int(class_sample.size)
    if class_offsets.shape != (n_classes + 1,) or mol_class.ndim != 1 or mol_umi.shape != mol_class.shape:
        raise ValueError('class_offsets[n_classes + 1] beside class_sample[n_classes]; mol_class and mol_umi of one length')
    if n_classes and class_targets.size != class_offsets[-1]:
        raise ValueError('class_targets holds %d ids, class_offsets ends at %d' % (class_targets.size, class_offsets[-1]))
    handle = ctypes.c_void_p()
    n = int(mol_class.size)
    _native.check(_native.hip().skm_gene_matrix_from_molecule_sets(
        int(device), n_classes, _native.ptr(class_offsets, _native.c_i64p),
        _native.ptr(class_targets, _native.c_i32p) if class_targets.size else None,
        _native.ptr(class_sample, _native.c_i32p) if n_classes else None, n,
        _native.ptr(mol_class, _native.c_i32p) if n else None, _native.ptr(mol_umi, _native.c_u32p) if n else None,
        int(n_samples), int(tx_gene.size), int(n_genes), _native.ptr(tx_gene, _native.c_i32p) if tx_gene.size else None,
        int(max_steps), ctypes.byref(handle)))
    return read_distributed_matrix(handle)


def gene_em_cells(cell_row_start, u, cell_set_start, set_start, set_rows, max_steps=1000, device=0):
    """(x float64[n_rows], steps int64[n_cells], capped int64[n_cells]): the EM of "Distributed molecules" alone, a block
    per cell (skm_gene_em_cells).  Cell c has the rows cell_row_start[c] .. cell_row_start[c + 1] - 1 with the counts
    u[] and the sets cell_set_start[c] .. cell_set_start[c + 1] - 1; set j holds the cell-local rows
    set_rows[set_start[j]:set_start[j + 1]], 2 to 16 of them, ascending.  Anything else raises."""
    cell_row_start = numpy.ascontiguousarray(cell_row_start, dtype=numpy.int64)
    cell_set_start = numpy.ascontiguousarray(cell_set_start, dtype=numpy.int64)
    u = numpy.ascontiguousarray(u, dtype=numpy.int64)
    set_start = numpy.ascontiguousarray(set_start, dtype=numpy.int64)
    set_rows = numpy.ascontiguousarray(set_rows, dtype=numpy.int32)
    n_cells = int(cell_row_start.size) - 1
    if n_cells < 0 or cell_set_start.shape != cell_row_start.shape or u.ndim != 1 or set_start.ndim != 1 or set_rows.ndim != 1:
        raise ValueError('cell_row_start and cell_set_start of n_cells + 1 words, u, set_start and set_rows flat')
    if u.size != cell_row_start[-1] or set_start.size != cell_set_start[-1] + 1 or set_rows.size != set_start[-1]:
        raise ValueError('u[%d], set_start[%d] and set_rows[%d] do not fit the offsets' % (u.size, set_start.size, set_rows.size))
    x = numpy.zeros(max(u.size, 1), dtype=numpy.float64)
    steps = numpy.zeros(max(n_cells, 1), dtype=numpy.int64)
    capped = numpy.zeros(max(n_cells, 1), dtype=numpy.int64)
    _native.check(_native.hip().skm_gene_em_cells(
        int(device), n_cells, _native.ptr(cell_row_start, _native.c_i64p), _native.ptr(u, _native.c_i64p) if u.size else None,
        _native.ptr(cell_set_start, _native.c_i64p), _native.ptr(set_start, _native.c_i64p),
        _native.ptr(set_rows, _native.c_i32p) if set_rows.size else None, int(max_steps), _native.ptr(x, _native.c_f64p),
        _native.ptr(steps, _native.c_i64p), _native.ptr(capped, _native.c_i64p)))
    return x[:u.size], steps[:n_cells], capped[:n_cells]


class SummarizedResult:
    """seekmer/mapper.py:18-37"""
    __slots__ = ['aligned', 'unaligned', 'total', 'class_map', 'class_count',
                 'fragment_length_frequencies', 'effective_lengths',
                 'class_offsets', 'class_targets', '_map_result', 'length_model', 'bias_observed', 'bias_weights']

    def __init__(self, aligned, unaligned, total, class_map, class_count,
                 fragment_length_frequencies, effective_lengths,
                 class_offsets=None, class_targets=None, map_result=None, length_model=None,
                 bias_observed=None, bias_weights=None):
        self.aligned = aligned
        self.unaligned = unaligned
        self.total = total
        self.class_map = class_map
        self.class_count = class_count
        self.fragment_length_frequencies = fragment_length_frequencies
        self.effective_lengths = effective_lengths
        self.class_offsets = class_offsets
        self.class_targets = class_targets
        self._map_result = map_result
        self.length_model = length_model      # (mean, sd) when the effective lengths come from a model
        # --bias (infer.bias_pass): the observed hexamer counts and the weights the effective lengths carry
        self.bias_observed = bias_observed
        self.bias_weights = bias_weights

    def detach(self):
        """Let go of the MapResult the summary came from (its table is in the summary): the mapper's
        handle and its device memory go when nothing else holds them."""
        self._map_result = None
        return self


class MapResult:
    """A mapping result collection with a lock (seekmer/mapper.py:40-145)."""

    def __init__(self, index, readmap=None, device=0, keep_spans=False, strand=None, length_model=None, bias=False):
        """keep_spans: also store every unit's MappedSpan (begin, end, anchor) for
        ReadMapper.last_batch -- parity tests and diagnostics; inference does not read them.
        strand: None (unstranded), 'fr' (--fr-stranded: mate 1 in the transcript's orientation) or
        'rf' (--rf-stranded: mate 1 antisense); every mapped unit keeps only the targets of that
        orientation (skm_mapper_set_strand).
        length_model: None, or (mean, sd) of a fragment-length model (fragment_length_weights): the
        effective lengths then come from it, here and in infer.quantify_resident
        (skm_mapper_set_length_weights); the histogram is counted and reported as ever.
        bias: also count the hexamer every aligned unit starts with (skm_mapper_set_bias), for the
        sequence-bias correction of infer.bias_correct: bias_observed()."""
        mode = strand_mode(strand)
        model, weights = length_model_weights(length_model)
        self.lock = threading.Lock()
        self.index = index
        self.readmap = readmap
        self.device = device
        self._handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_mapper_create(index.device_handle(device),
                                                      ctypes.byref(self._handle)))
        self._extra_fld = numpy.zeros(MAX_FRAGMENT_LENGTH, dtype='i8')
        self.keep_spans = bool(keep_spans)
        if keep_spans:
            _native.check(_native.hip().skm_mapper_keep_spans(self._handle, 1))
        self.strand = strand
        if mode != _native.SKM_STRAND_NONE:
            _native.check(_native.hip().skm_mapper_set_strand(self._handle, mode))
        self.length_model, self._length_weights = None, None
        if model is not None:
            self.set_length_model(model)
        self.bias = bool(bias)
        if self.bias:
            _native.check(_native.hip().skm_mapper_set_bias(self._handle, 1))

    def bias_observed(self):
        """int64[4096]: how many aligned units start with each hexamer (first base in the top two bits of
        the code; a unit with anything but an upper-case A, C, G or T among the six is not counted).  A
        MapResult made with bias=True; NativeError SKM_ERR_STATE otherwise."""
        out = numpy.zeros(4096, dtype=numpy.int64)
        _native.check(_native.hip().skm_mapper_bias_observed(self._handle, _native.ptr(out, _native.c_i64p)))
        return out

    def gene_unique_counts(self, tx_gene, n_genes):
        """(unique int64[n_genes], other int64[2]) of the table where it lies in HBM (skm_mapper_gene_counts): the
        units whose class lies inside one gene, by gene; other = (units ambiguous between genes, units of unnamed
        transcripts only).  tx_gene int32[n_tx]: gene number of every transcript, -1 without one (infer.gene_map)."""
        tx_gene = gene_numbers(tx_gene, self.index.transcripts.size)
        unique = numpy.zeros(max(int(n_genes), 1), dtype=numpy.int64)
        other = numpy.zeros(2, dtype=numpy.int64)
        _native.check(_native.hip().skm_mapper_gene_counts(
            self._handle, tx_gene.size, int(n_genes), _native.ptr(tx_gene, _native.c_i32p),
            _native.ptr(unique, _native.c_i64p), _native.ptr(other, _native.c_i64p)))
        return unique[:int(n_genes)], other

    def set_length_model(self, length_model):
        """(mean, sd), or None for the observed histogram again; it affects later calls only."""
        model, weights = length_model_weights(length_model)
        _native.check(_native.hip().skm_mapper_set_length_weights(
            self._handle, _native.ptr(weights, _native.c_f64p) if weights is not None else None))
        self.length_model, self._length_weights = model, weights

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            try:
                _native.hip().skm_mapper_destroy(handle)
            except Exception:
                pass
            self._handle = None

    # -- raw views of the device table --------------------------------------
    def sizes(self):
        """(classes, class_map rows, unaligned, total units)"""
        out = (ctypes.c_int64 * 4)()
        _native.check(_native.hip().skm_mapper_summary(self._handle, out))
        return tuple(int(v) for v in out)

    def export(self):
        """(class_offsets, class_targets, class_counts, first_seen, fld) in
        first-seen class order."""
        n_classes, n_rows, _, _ = self.sizes()
        offsets = numpy.zeros(n_classes + 1, dtype=numpy.int64)
        targets = numpy.zeros(max(n_rows, 1), dtype=numpy.int32)
        counts = numpy.zeros(max(n_classes, 1), dtype=numpy.int64)
        first = numpy.zeros(max(n_classes, 1), dtype=numpy.int64)
        fld = numpy.zeros(MAX_FRAGMENT_LENGTH, dtype=numpy.int64)
        _native.check(_native.hip().skm_mapper_export(
            self._handle, _native.ptr(offsets, _native.c_i64p), _native.ptr(targets, _native.c_i32p),
            _native.ptr(counts, _native.c_i64p), _native.ptr(first, _native.c_i64p),
            _native.ptr(fld, _native.c_i64p)))
        return offsets, targets[:n_rows], counts[:n_classes], first[:n_classes], fld

    @property
    def fragment_length_counts(self):
        fld = numpy.zeros(MAX_FRAGMENT_LENGTH, dtype=numpy.int64)
        _native.check(_native.hip().skm_mapper_export(
            self._handle, None, None, None, None, _native.ptr(fld, _native.c_i64p)))
        return fld

    @property
    def counter(self):
        """collections.Counter keyed by the id tuple; () = unaligned
        (seekmer/mapper.py:54, 70)."""
        offsets, targets, counts, _, _ = self.export()
        counter = collections.Counter()
        ids = targets.tolist()
        for k in range(counts.size):
            counter[tuple(ids[offsets[k]:offsets[k + 1]])] = int(counts[k])
        unaligned = self.sizes()[2]
        if unaligned:
            counter[()] = unaligned
        return counter

    # -- the reference's methods ---------------------------------------------
    def update(self, read_names, iterable):
        """Add mapping results given as id tuples (seekmer/mapper.py:60-75)."""
        tuples = [tuple(t) for t in iterable]
        local = collections.Counter(tuples)
        unaligned = local.pop((), 0)
        keys = list(local.keys())
        offsets = numpy.zeros(len(keys) + 1, dtype=numpy.int64)
        numpy.cumsum([len(k) for k in keys], out=offsets[1:])
        targets = numpy.asarray([t for k in keys for t in k] or [0], dtype=numpy.int32)
        counts = numpy.asarray([local[k] for k in keys] or [0], dtype=numpy.int64)
        base = self.sizes()[3]
        first_index = {}
        for i, t in enumerate(tuples):
            first_index.setdefault(t, i)
        first = numpy.asarray([base + first_index[k] for k in keys] or [0], dtype=numpy.int64)
        _native.check(_native.hip().skm_mapper_merge(
            self._handle, len(keys), _native.ptr(offsets, _native.c_i64p),
            _native.ptr(targets, _native.c_i32p), _native.ptr(counts, _native.c_i64p),
            _native.ptr(first, _native.c_i64p), unaligned, None))
        self._write_readmap(read_names, tuples)

    def _write_readmap(self, read_names, tuples):
        if self.readmap is None:
            return
        for read_name, targets in zip(read_names, tuples):
            ids = self.index.transcripts[list(targets),]['transcript_id']
            print(read_name.decode(), *[id_.decode() for id_ in ids], sep='\t', file=self.readmap)

    def merge_table(self, offsets, targets, counts, first_seen, unaligned, fld):
        """Counter.update + merge_fragment_lengths with another table."""
        _native.check(_native.hip().skm_mapper_merge(
            self._handle, counts.size,
            _native.ptr(numpy.ascontiguousarray(offsets, dtype=numpy.int64), _native.c_i64p),
            _native.ptr(numpy.ascontiguousarray(targets if targets.size else [0], dtype=numpy.int32), _native.c_i32p),
            _native.ptr(numpy.ascontiguousarray(counts if counts.size else [0], dtype=numpy.int64), _native.c_i64p),
            _native.ptr(numpy.ascontiguousarray(first_seen if first_seen.size else [0], dtype=numpy.int64), _native.c_i64p),
            int(unaligned),
            _native.ptr(numpy.ascontiguousarray(fld, dtype=numpy.int64), _native.c_i64p)))

    def device_table(self):
        """The table where it lies in HBM (skm_device_table): what a GPU-to-GPU hand-over copies."""
        table = _native.DeviceTable()
        _native.check(_native.hip().skm_mapper_device_table(self._handle, ctypes.byref(table)))
        return table

    def merge_resident(self, other):
        """Counter.update + merge_fragment_lengths with a table that lies on the same GPU (another
        MapResult, or a DeviceTable whose arrays were copied there): nothing crosses the host."""
        table = other if isinstance(other, _native.DeviceTable) else other.device_table()
        _native.check(_native.hip().skm_mapper_merge_device(self._handle, ctypes.byref(table)))

    def summarize(self):
        """seekmer/mapper.py:77-104: classes in Counter insertion order,
        class_map = int64[2, M] (row 0 class id, row 1 transcript id in tuple
        order, duplicates kept), class_count f8[C]."""
        offsets, targets, counts, _, fld = self.export()
        n_classes = counts.size
        _, _, unaligned, total = self.sizes()
        if targets.size:
            class_ids = numpy.repeat(numpy.arange(n_classes, dtype=numpy.int64), numpy.diff(offsets))
            class_map = numpy.vstack([class_ids, targets.astype(numpy.int64)])
        else:
            class_map = numpy.asarray([]).T
        class_count = counts.astype('f8')
        aligned = class_count.sum()
        return SummarizedResult(
            aligned=int(aligned),
            unaligned=int(unaligned),
            total=int(aligned + unaligned),
            class_map=class_map,
            class_count=class_count,
            fragment_length_frequencies=fld,
            effective_lengths=self._effective_lengths(fld),
            class_offsets=offsets,
            class_targets=targets,
            map_result=self,
            length_model=self.length_model,
        )

    def merge_fragment_lengths(self, fragment_length_counts):
        """seekmer/mapper.py:106-115"""
        fld = numpy.ascontiguousarray(fragment_length_counts, dtype=numpy.int64)
        empty = numpy.zeros(1, dtype=numpy.int64)
        _native.check(_native.hip().skm_mapper_merge(
            self._handle, 0, _native.ptr(empty, _native.c_i64p), None, None, None, 0,
            _native.ptr(fld, _native.c_i64p)))

    @property
    def harmonic_mean_fragment_length(self):
        """seekmer/mapper.py:117-132"""
        fld = self.fragment_length_counts
        assert fld[0] == 0
        numerator = fld.sum()
        if numerator == 0:
            return 0
        denominator = (fld[1:].astype('f8') / numpy.arange(1, MAX_FRAGMENT_LENGTH)).sum()
        return numerator / denominator

    @property
    def transcript_lengths(self):
        """index.transcripts['length'] as a contiguous f8 array (extracted once)."""
        cached = getattr(self, '_lengths', None)
        if cached is None:
            cached = numpy.ascontiguousarray(self.index.transcripts['length'], dtype='f8')
            self._lengths = cached
        return cached

    def _effective_lengths(self, fld):
        length = self.transcript_lengths
        if self._length_weights is not None:
            return _effective_lengths_weights(length, self._length_weights, self.device)[0]
        out = numpy.zeros(length.shape, dtype='f8')
        _native.check(_native.hip().skm_effective_lengths(
            self.device, _native.ptr(numpy.ascontiguousarray(fld, dtype=numpy.int64), _native.c_i64p),
            _native.ptr(length, _native.c_f64p), length.size, _native.ptr(out, _native.c_f64p)))
        return out

    @property
    def effective_lengths(self):
        """seekmer/mapper.py:134-141 (computed on the GPU); with a length model, from its weights"""
        if self._length_weights is not None:
            return self._effective_lengths(None)
        return self._effective_lengths(self.fragment_length_counts)

    def clear(self):
        """Clear the counter (seekmer/mapper.py:143-145)."""
        _native.check(_native.hip().skm_mapper_clear(self._handle))

    def sync(self):
        """Wait for every batch handed over with map_batch_async; raises the first failure."""
        _native.check(_native.hip().skm_mapper_sync(self._handle))

    def reset(self):
        """Fresh-MapResult state (counter, totals and histogram) on the same buffers."""
        _native.check(_native.hip().skm_mapper_reset(self._handle))

    def map_resident(self, d_bases, d_offsets, n_units, paired, max_read_len):
        """Map a batch that already lives in HBM (device pointers)."""
        _native.check(_native.hip().skm_mapper_map_batch_device(
            self._handle, d_bases, d_offsets, n_units, int(bool(paired)), max_read_len))

    def set_stats(self, enable):
        _native.check(_native.hip().skm_mapper_set_stats(self._handle, int(enable)))

    def access_stats(self):
        out = (ctypes.c_int64 * 48)()
        _native.check(_native.hip().skm_mapper_access_stats(self._handle, out))
        names = ('reads', 'read_bases', 'lookups', 'slots', 'contig_reads', 'targets_copied',
                 'targets_merged', 'seq_fetches', 'merges', 'tuple_ids')
        stats = {n: int(out[i]) for i, n in enumerate(names)}
        census = ('rounds', 'start_exec', 'start_lanes', 'lookup_exec', 'lookup_lanes', 'merge_exec',
                  'merge_lanes', 'left_exec', 'left_lanes', 'right_exec', 'right_lanes', 'emit_exec',
                  'emit_lanes', 'scan_exec', 'scan_lanes')
        stats['census'] = {n: int(out[16 + i]) for i, n in enumerate(census)}
        cycles = ('schedule', 'barrier', 'start', 'lookup', 'merge', 'left', 'right', 'emit', 'scan',
                  'emit_mate1', 'emit_intersect', 'emit_fld', 'emit_scan', 'emit_entries', 'emit_store')
        stats['wave_cycles'] = {n: int(out[32 + i]) for i, n in enumerate(cycles)}
        return stats

    def timing(self):
        """skm_mapper_timing by name; 'deferred_grows' (stats[7]) counts the times the class table
        grew under a batch whose bounded probes had deferred units, 'map_relaunches'
        (skm_mapper_map_relaunches) the map kernel launches repeated in a larger entry arena."""
        out = (ctypes.c_double * 8)()
        _native.check(_native.hip().skm_mapper_timing(self._handle, out))
        relaunches = ctypes.c_int64()
        _native.check(_native.hip().skm_mapper_map_relaunches(self._handle, ctypes.byref(relaunches)))
        return {'pack_ns': out[0], 'map_ns': out[1], 'class_ns': out[2],
                'batches': int(out[3]), 'units': int(out[4]), 'em_ns': out[5], 'em_iterations': int(out[6]),
                'deferred_grows': int(out[7]), 'map_relaunches': relaunches.value}

    def map_layout(self):
        """skm_mapper_map_layout: which map kernel the last launch took ('packed' or 'wide' unit contexts), its
        contexts per workgroup and its grid."""
        packed, contexts, blocks = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _native.check(_native.hip().skm_mapper_map_layout(self._handle, ctypes.byref(packed), ctypes.byref(contexts),
                                                           ctypes.byref(blocks)))
        return {'layout': 'packed' if packed.value else 'wide', 'contexts': contexts.value, 'blocks': blocks.value}


class ReadMapper:
    """A read mapper (seekmer/_mapper.pyx:31-105)."""

    def __init__(self, index, map_result):
        self.index = index
        self.map_result = map_result

    def map_batch(self, batch):
        """Map one batch and wait for it."""
        hip = _native.hip()
        _native.check(hip.skm_mapper_map_batch(
            self.map_result._handle, batch.bases.ctypes.data,
            _native.ptr(batch.offsets, _native.c_i64p), batch.count, int(batch.paired)))

    def map_batch_async(self, batch):
        """Hand one batch over (returns when its arrays are free again; the kernels run behind
        the next batch's parsing and copy).  MapResult.sync() -- or any read of the result --
        waits for what is queued.  A batch that knows its place in the sample
        (``batch.first_unit``) keeps the -j1 class order whatever the submission order."""
        hip = _native.hip()
        first_unit = getattr(batch, 'first_unit', None)
        first_unit = -1 if first_unit is None else int(first_unit)
        uniform = getattr(batch, 'uniform_len', None)
        if uniform is not None and batch.count:       # equal-length reads: the offsets stay on the host
            _native.check(hip.skm_mapper_map_batch_uniform_async(
                self.map_result._handle, batch.bases.ctypes.data + int(batch.offsets[0]), int(uniform),
                batch.count, int(batch.paired), first_unit))
            return
        _native.check(hip.skm_mapper_map_batch_async(
            self.map_result._handle, batch.bases.ctypes.data,
            _native.ptr(batch.offsets, _native.c_i64p), batch.count, int(batch.paired), first_unit))

    def push_packed(self, piece):
        """Hand over reads that are already packed (common.PackedReads): copied to HBM now, mapped in
        the background as soon as every stream of the sample covers a run of units."""
        _native.check(_native.hip().skm_mapper_push_packed(
            self.map_result._handle, ctypes.byref(piece.raw), int(piece.paired)))

    def drain_packed(self, feeder):
        """A PackedReadFeeder straight into the mapper without a Python step per piece
        (skm_mapper_map_packed_source over skm_fastq_packed_next); returns the pieces pushed."""
        reader = feeder.open()
        try:
            pieces = ctypes.c_int64()
            # (the files' sizes say about how many units are coming: tables sized once, not grown)
            _native.check(_native.hip().skm_mapper_expect_units(self.map_result._handle, reader.estimate()))
            _native.check(_native.hip().skm_mapper_map_packed_source(
                self.map_result._handle, ctypes.cast(_native.host().skm_fastq_packed_next, ctypes.c_void_p),
                reader.handle, int(feeder.paired), ctypes.byref(pieces)))
        finally:
            feeder.stats = reader.stats()
            reader.close()
        return pieces.value

    def last_batch(self, n_units):
        """(begin, end, anchor_entry, anchor_offset, counts, signed entries); the spans need a
        MapResult created with keep_spans=True."""
        spans = [numpy.zeros(max(n_units, 1), dtype=numpy.int32) for _ in range(4)]
        hip = _native.hip()
        _native.check(hip.skm_mapper_last_batch(
            self.map_result._handle, *[_native.ptr(a, _native.c_i32p) for a in spans],
            None, None, 0, None))
        counts, entries = self.last_tuples(n_units)
        return tuple(a[:n_units] for a in spans) + (counts, entries)

    def last_tuples(self, n_units):
        """(counts, signed entries) of the last batch, units in order."""
        hip = _native.hip()
        counts = numpy.zeros(max(n_units, 1), dtype=numpy.int32)
        needed = ctypes.c_int64()
        _native.check(hip.skm_mapper_last_batch(
            self.map_result._handle, None, None, None, None, _native.ptr(counts, _native.c_i32p),
            None, 0, ctypes.byref(needed)))
        entries = numpy.zeros(max(needed.value, 1), dtype=numpy.int32)
        _native.check(hip.skm_mapper_last_batch(
            self.map_result._handle, None, None, None, None, None,
            _native.ptr(entries, _native.c_i32p), entries.size, ctypes.byref(needed)))
        return counts[:n_units], entries[:needed.value]

    def __call__(self, reads_iterator):
        """Run the mapping loop (seekmer/_mapper.pyx:59-105)."""
        if isinstance(reads_iterator, PackedReadFeeder) and self.map_result.readmap is None:
            self.drain_packed(reads_iterator)
            self.map_result.sync()
            return
        for item in reads_iterator:
            if isinstance(item, PackedReads):
                if self.map_result.readmap is not None:
                    raise ValueError('-m/--save-readmap needs the reads as text: use NativeReadFeeder')
                self.push_packed(item)
                continue
            if isinstance(item, ReadBatch):
                batch = item
            else:
                read_count, read_names, reads = item
                batch = ReadBatch.from_lists(read_count, read_names, reads)
            if self.map_result.readmap is None:
                self.map_batch_async(batch)
                continue
            # -m/--save-readmap: the per-unit tuples of THIS batch are needed, so
            # keep other threads off the handle until they are fetched
            with self.map_result.lock:
                self.map_batch(batch)
                counts, entries = self.last_tuples(batch.count)
                ids = numpy.where(entries < 0, ~entries, entries).tolist()
                bounds = numpy.concatenate([[0], numpy.cumsum(counts)]).tolist()
                tuples = [tuple(ids[bounds[i]:bounds[i + 1]]) for i in range(batch.count)]
                self.map_result._write_readmap(batch.names, tuples)
        self.map_result.sync()            # (raises here what a queued batch failed with)


def _drain_worker(mapper, reads_queue, errors):
    """Thread body of map_reads: run the mapper over the queue; on a failure (device error,
    tag collision, bad batch) remember the first exception and keep taking batches up to the
    sentinel so the feeding thread never blocks on a full queue."""
    batches = iter(reads_queue.get, None)
    try:
        mapper(batches)
    except BaseException as error:        # noqa: B902 -- re-raised by map_reads in the caller's thread
        errors.append(error)
        for __ in batches:
            pass


def map_reads(index, read_feeder, job_count=1, readmap=None, debug=False, device=0, strand=None, length_model=None,
              bias=False):
    """Map reads (seekmer/mapper.py:148-193).  Unlike the reference's CPU workers the device
    calls can fail; a worker's exception is re-raised here once every thread has stopped,
    instead of being lost with its thread.  strand: None, 'fr' or 'rf'; length_model: None or
    (mean, sd); bias: count the aligned units' first hexamers (MapResult)."""
    map_result = _new_result(index, strand, length_model, bias, readmap=readmap, device=device)
    try:
        if debug or job_count <= 1 or isinstance(read_feeder, PackedReadFeeder):
            # (a packed feeder parses with its own threads and is drained natively: the GIL is not held)
            ReadMapper(index, map_result)(read_feeder)
        else:
            reads_queue = queue.Queue(job_count * 2)
            threads, errors = [], []
            for __ in range(job_count):
                thread = threading.Thread(target=_drain_worker,
                                          args=(ReadMapper(index, map_result), reads_queue, errors))
                threads.append(thread)
                thread.start()
            try:
                for batch in read_feeder:
                    if errors:
                        break
                    reads_queue.put(batch)
            finally:
                for __ in range(job_count):
                    reads_queue.put(None)
                for thread in threads:
                    thread.join()
                threads.clear()
            if errors:
                raise errors[0]
    finally:
        if readmap is not None:
            readmap.close()
    return map_result


def map_multiple_samples(index, read_feeders, job_count=1, debug=False, device=0, strand=None, length_model=None):
    """Map reads for multiple samples (seekmer/mapper.py:196-234); a failed sample raises.
    strand: None, 'fr' or 'rf', length_model: None or (mean, sd), for every sample (MapResult)."""
    strand_mode(strand)
    length_model_weights(length_model)
    map_results = []
    if debug:
        for read_feeder in read_feeders:
            result = _new_result(index, strand, length_model, device=device)
            map_results.append(result)
            ReadMapper(index, result)(read_feeder)
    else:
        pool = multiprocessing.pool.ThreadPool(job_count)
        pending = []
        for read_feeder in read_feeders:
            result = _new_result(index, strand, length_model, device=device)
            map_results.append(result)
            pending.append(pool.apply_async(_map, args=(index, result, read_feeder)))
        pool.close()
        pool.join()
        for job in pending:
            job.get()                     # re-raises what the worker raised
    return map_results


def _new_result(index, strand, length_model=None, bias=False, **kwargs):
    """MapResult(index, **kwargs, strand=strand, length_model=length_model, bias=bias); unstranded,
    without a model and without counting, the call is the one of before (a stand-in for MapResult
    need not know the later keywords)."""
    if strand is not None:
        kwargs['strand'] = strand
    if length_model is not None:
        kwargs['length_model'] = length_model
    if bias:
        kwargs['bias'] = True
    return MapResult(index, **kwargs)


def _map(index, map_result, read_feeder):
    ReadMapper(index, map_result)(read_feeder)
    return None


# ---- many small samples in shared launches (include/seekmer_hip.h, skm_sample_set_*) -------------------

def _slice_piece(piece, begin, end):
    """Reads [begin, end) of a PackedReads piece as a piece of its own (arrays copied)."""
    reads, masks = piece.exceptions
    inside = (reads >= begin) & (reads < end)
    return PackedReads.from_arrays(piece.stream, piece.first_read + begin, numpy.array(piece.codes[begin:end]),
                                   numpy.array(piece.lengths[begin:end]), reads[inside] - numpy.uint32(begin),
                                   numpy.array(masks[inside]), paired=piece.paired)


def sample_segments(pieces, paired):
    """The pieces of ONE sample as a packed reader hands them out (common.PackedReadFeeder: one stream
    single-ended, two streams paired, each numbered by unit; a piece that begins below what its stream
    holds replaces the reads from there on, and so does a cut, by nothing) -> the sample's units as
    in-order segments [(first_unit, mate1, mate2 or None), ...] over arrays of their own.  A pair of
    files counts min(records) units, zip(file1, file2) (seekmer/common.py:180-197): reads of one
    stream that the other never matches are in no segment."""
    streams = ([], [])
    for piece in pieces:
        if piece.stream not in ((0, 1) if paired else (0,)):
            raise ValueError('stream %d of a %s sample' % (piece.stream, 'paired' if paired else 'single-ended'))
        if not piece.is_cut and piece.n_reads == 0:
            continue
        held = streams[piece.stream]
        first = piece.first_read
        while held and held[-1].first_read >= first:
            held.pop()
        if held and held[-1].first_read + held[-1].n_reads > first:
            held[-1] = _slice_piece(held[-1], 0, first - held[-1].first_read)
        if piece.is_cut:
            continue
        if held and held[-1].first_read + held[-1].n_reads != first:
            raise ValueError('the reads of stream %d do not follow each other (unit %d after %d)'
                             % (piece.stream, first, held[-1].first_read + held[-1].n_reads))
        held.append(piece.held())
    if not paired:
        return [(piece.first_read, piece, None) for piece in streams[0]]
    segments = []
    i = j = 0
    while i < len(streams[0]) and j < len(streams[1]):
        a, b = streams[0][i], streams[1][j]
        begin = max(a.first_read, b.first_read)
        end = min(a.first_read + a.n_reads, b.first_read + b.n_reads)
        if begin < end:
            segments.append((begin,) + tuple(
                piece if (piece.first_read, piece.n_reads) == (begin, end - begin)
                else _slice_piece(piece, begin - piece.first_read, end - piece.first_read) for piece in (a, b)))
        if a.first_read + a.n_reads <= b.first_read + b.n_reads:
            i += 1
        else:
            j += 1
    return segments


def _effective_lengths(lengths, fld, device):
    """MapResult.effective_lengths (seekmer/mapper.py:134-141) for a histogram, on the GPU."""
    out = numpy.zeros(lengths.shape, dtype='f8')
    _native.check(_native.hip().skm_effective_lengths(
        device, _native.ptr(numpy.ascontiguousarray(fld, dtype=numpy.int64), _native.c_i64p),
        _native.ptr(lengths, _native.c_f64p), lengths.size, _native.ptr(out, _native.c_f64p)))
    return out


def _effective_lengths_many(lengths, fld, device):
    """_effective_lengths for every row of fld[n, 2000] in one native call: f8[n, n_tx]."""
    fld = numpy.ascontiguousarray(fld, dtype=numpy.int64).reshape(-1, MAX_FRAGMENT_LENGTH)
    out = numpy.zeros((fld.shape[0], lengths.size), dtype='f8')
    _native.check(_native.hip().skm_effective_lengths_many(
        device, fld.shape[0], _native.ptr(fld, _native.c_i64p) if fld.size else None,
        _native.ptr(lengths, _native.c_f64p), lengths.size, _native.ptr(out, _native.c_f64p) if out.size else None))
    return out


def _effective_lengths_weights(lengths, weights, device):
    """The same rule with p given (fragment_length_weights) instead of counted: weights f8[2000] or
    f8[n, 2000] -> f8[n, n_tx] in one native call."""
    weights = numpy.ascontiguousarray(weights, dtype='f8').reshape(-1, MAX_FRAGMENT_LENGTH)
    out = numpy.zeros((weights.shape[0], lengths.size), dtype='f8')
    _native.check(_native.hip().skm_effective_lengths_weights(
        device, weights.shape[0], _native.ptr(weights, _native.c_f64p), _native.ptr(lengths, _native.c_f64p),
        lengths.size, _native.ptr(out, _native.c_f64p)))
    return out


def harmonic_mean_fragment_lengths(counts):
    """MapResult.harmonic_mean_fragment_length (seekmer/mapper.py:117-132) for every row of
    counts[n, 2000]: a list of n numbers, 0 for an empty histogram."""
    means = []
    for fld in numpy.asarray(counts).reshape(-1, MAX_FRAGMENT_LENGTH):
        assert fld[0] == 0
        numerator = fld.sum()
        if numerator == 0:
            means.append(0)
            continue
        denominator = (fld[1:].astype('f8') / numpy.arange(1, MAX_FRAGMENT_LENGTH)).sum()
        means.append(numerator / denominator)
    return means


class SampleSet:
    """Many small samples on one device handle (skm_sample_set): their units share launches and one
    class table whose classes are (sample, target tuple).  Every sample's table -- class order,
    offsets, targets, counts, first-seen units counted inside the sample, unaligned and total units --
    is bit for bit that of a MapResult fed the sample's reads alone, however the samples are
    interleaved, cut into launches or spread over feeding threads.

    By default the set keeps ONE fragment-length histogram, the sum over its samples: what
    impute.pool_fragment_lengths gives every cell (seekmer/impute.py:128-146), and every summary carries
    it.  With ``per_sample_lengths`` it also keeps one histogram per sample, counted on the device after
    every launch from the units' spans: sample_fragment_length_counts, and every summary then carries
    its own sample's histogram and effective lengths, those of a MapResult fed the sample alone -- what
    an ordinary `infer` of the sample needs.  There is no readmap.  ``strand`` (None, 'fr', 'rf')
    applies to every sample.  So does ``length_model`` (None, or (mean, sd): fragment_length_weights):
    with one, every sample's effective lengths are the model's -- one row, made once, in summarize()
    and in quantify() -- whatever the histograms hold; those are counted and reported as ever.
    With ``bias`` the set also counts, per sample, the hexamer every aligned unit starts with
    (skm_sample_set_keep_bias), for the sequence-bias correction of infer.bias_correct_many:
    bias_observed().  Such a set numbers its samples below 2^15.
    With ``umi_bases`` (1..16; needs per_sample_lengths) every unit comes with a UMI and the set collapses
    duplicates on the device (skm_sample_set_keep_umis; DESIGN.md section 4, "UMI collapse"): inside a sample
    only the first unit of every (UMI, class) stays, and every table, total, histogram per sample and hexamer row
    is that of a set fed the surviving units alone; umi_removed() says how many went.  Such a set takes its reads
    through add_packed(..., umis=) only, and its POOLED histogram still holds the removed units.
    With ``umi_mismatches=1`` (needs umi_bases; skm_sample_set_set_umi_mismatches; DESIGN.md section 4, "UMI
    mismatches") a unit is also removed when an earlier unit of its sample has the same class and a UMI one
    substitution away, whether or not that earlier unit stayed; umi_near_removed() counts the units that only this
    removed.  0, the default, is the exact rule.

    Samples are numbered from 0.  A sample's reads are added as segments, each beginning at the unit
    where the sample's units so far end (NativeError SKM_ERR_STATE otherwise); any thread may add."""

    def __init__(self, index, paired, device=0, strand=None, per_sample_lengths=False, length_model=None, bias=False,
                 umi_bases=0, umi_mismatches=0):
        mode = strand_mode(strand)
        self.length_model, self._length_weights = length_model_weights(length_model)
        self.umi_bases = int(umi_bases)
        if not 0 <= self.umi_bases <= MAX_UMI_LENGTH:
            raise ValueError('UMIs of %r bases: 1 to %d are possible' % (umi_bases, MAX_UMI_LENGTH))
        self.umi_mismatches = check_umi_mismatches(umi_mismatches, self.umi_bases)
        self.index = index
        self.paired = bool(paired)
        self.device = device
        self.strand = strand
        self.per_sample_lengths = bool(per_sample_lengths)
        self.bias = bool(bias)
        self._handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_sample_set_create(index.device_handle(device), int(self.paired),
                                                          ctypes.byref(self._handle)))
        if mode != _native.SKM_STRAND_NONE:
            _native.check(_native.hip().skm_sample_set_set_strand(self._handle, mode))
        if self.per_sample_lengths:
            _native.check(_native.hip().skm_sample_set_keep_histograms(self._handle, 1))
        if self._length_weights is not None:
            _native.check(_native.hip().skm_sample_set_set_length_weights(
                self._handle, _native.ptr(self._length_weights, _native.c_f64p)))
        if self.bias:
            _native.check(_native.hip().skm_sample_set_keep_bias(self._handle, 1))
        if self.umi_bases:
            _native.check(_native.hip().skm_sample_set_keep_umis(self._handle, self.umi_bases))
        if self.umi_mismatches:
            _native.check(_native.hip().skm_sample_set_set_umi_mismatches(self._handle, self.umi_mismatches))

    def umi_near_removed(self):
        """The units removed so far only because an earlier unit of their sample and class had a UMI one substitution
        away (each the first of its own UMI): part of umi_removed()'s counts; 0 in a set without umi_mismatches=1."""
        n = ctypes.c_int64(0)
        _native.check(_native.hip().skm_sample_set_umi_near_removed(self._handle, ctypes.byref(n)))
        return int(n.value)

    def umi_removed(self):
        """int64[n_samples]: the units UMI collapse has removed from every sample (zeros in a set without UMIs)."""
        # (samples may be added meanwhile: the call says when there are more than the rows it was given)
        while True:
            out = numpy.zeros(len(self), dtype=numpy.int64)
            code = _native.hip().skm_sample_set_umi_removed(self._handle, out.size,
                                                            _native.ptr(out, _native.c_i64p) if out.size else None)
            if code == _native.SKM_ERR_ARG and len(self) > out.size:
                continue
            _native.check(code)
            return out

    def bias_observed(self):
        """int64[n_samples, 4096]: row i is MapResult.bias_observed() of sample i mapped alone (zeros for a sample
        without units).  Only a set made with bias=True; NativeError SKM_ERR_STATE otherwise."""
        # (samples may be added meanwhile: the call says when there are more than the rows it was given)
        while True:
            out = numpy.zeros((len(self), 4096), dtype=numpy.int64)
            code = _native.hip().skm_sample_set_bias_observed(self._handle, out.shape[0],
                                                              _native.ptr(out, _native.c_i64p) if out.size else None)
            if code == _native.SKM_ERR_ARG and len(self) > out.shape[0]:
                continue
            _native.check(code)
            return out

    def gene_unique_counts(self, tx_gene, n_genes):
        """(unique int64[n_samples, n_genes], other int64[n_samples, 2]): row i is MapResult.gene_unique_counts of
        sample i mapped alone (zeros for a sample without units), from the set's table where it lies in HBM
        (skm_sample_set_gene_counts)."""
        tx_gene = gene_numbers(tx_gene, self.index.transcripts.size)
        n_genes = int(n_genes)
        # (samples may be added meanwhile: the call says when there are more than the rows it was given)
        while True:
            rows = len(self)
            unique = numpy.zeros((rows, max(n_genes, 1)), dtype=numpy.int64)
            other = numpy.zeros((rows, 2), dtype=numpy.int64)
            if n_genes == 0:
                unique = unique[:, :0]
            code = _native.hip().skm_sample_set_gene_counts(
                self._handle, tx_gene.size, n_genes, _native.ptr(tx_gene, _native.c_i32p), rows,
                _native.ptr(unique, _native.c_i64p) if unique.size else None,
                _native.ptr(other, _native.c_i64p) if other.size else None)
            if code == _native.SKM_ERR_ARG and len(self) > rows:
                continue
            _native.check(code)
            return unique, other

    def gene_count_matrix(self, tx_gene, n_genes):
        """(indptr int64[n_samples + 1], indices int32[nnz], data int64[nnz], other int64[n_samples, 2]): what
        gene_unique_counts gives, as a CSR over samples made on the device (skm_sample_set_gene_matrix; DESIGN.md
        section 4, "Count matrix") -- row i holds the genes of sample i with a count, ascending, and no dense row
        exists anywhere."""
        tx_gene = gene_numbers(tx_gene, self.index.transcripts.size)
        handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_sample_set_gene_matrix(
            self._handle, tx_gene.size, int(n_genes), _native.ptr(tx_gene, _native.c_i32p), ctypes.byref(handle)))
        return read_gene_matrix(handle)

    def gene_molecule_matrix(self, tx_gene, n_genes):
        """The arrays of gene_count_matrix with molecules for units: data[k] is the number of distinct UMIs among the
        sample's surviving units whose class lies inside the gene (skm_sample_set_molecule_matrix; DESIGN.md section
        4, "Molecule matrix").  indptr, indices and other are gene_count_matrix's.  A set that keeps no UMIs
        (umi_bases=0) raises."""
        tx_gene = gene_numbers(tx_gene, self.index.transcripts.size)
        handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_sample_set_molecule_matrix(
            self._handle, tx_gene.size, int(n_genes), _native.ptr(tx_gene, _native.c_i32p), ctypes.byref(handle)))
        return read_gene_matrix(handle)

    def gene_resolved_matrix(self, tx_gene, n_genes):
        """(indptr, indices, data, tally int64[n_samples, 5]): one gene per (sample, UMI).  The distinct classes among a
        sample's live molecules -- the population of gene_molecule_matrix -- with one UMI form a group; the
        intersection of their gene sets names the group's gene (data counts such groups per gene) or makes the group
        multi-gene, unnamed or a collision: tally[s] = (resolved, rescued, multi-gene, unnamed, collision), rescued a
        part of resolved (skm_sample_set_resolved_matrix; DESIGN.md section 4, "Resolved molecules").  The pattern is
        the matrix's own, not gene_count_matrix's.  A set that keeps no UMIs (umi_bases=0) raises."""
        tx_gene = gene_numbers(tx_gene, self.index.transcripts.size)
        handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_sample_set_resolved_matrix(
            self._handle, tx_gene.size, int(n_genes), _native.ptr(tx_gene, _native.c_i32p), ctypes.byref(handle)))
        return read_resolved_matrix(handle)

    def gene_distributed_matrix(self, tx_gene, n_genes):
        """(indptr, indices, data float64[nnz], tally int64[n_samples, 8], to_unnamed float64[n_samples]): the groups of
        gene_resolved_matrix with the multi-gene ones shared out among their genes by an EM per sample.  data[k] is the
        weight of the gene in the sample, in molecules (0.001 at least); tally[s] = (resolved, distributed, wide,
        unnamed, collision, rows, steps, capped), the first five adding up to the sample's distinct UMIs; to_unnamed[s]
        is what the EM gave to "no gene" (skm_sample_set_distributed_matrix; DESIGN.md section 4, "Distributed
        molecules").  A set that keeps no UMIs (umi_bases=0) raises."""
        tx_gene = gene_numbers(tx_gene, self.index.transcripts.size)
        handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_sample_set_distributed_matrix(
            self._handle, tx_gene.size, int(n_genes), _native.ptr(tx_gene, _native.c_i32p), ctypes.byref(handle)))
        return read_distributed_matrix(handle)

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            try:
                _native.hip().skm_sample_set_destroy(handle)
            except Exception:
                pass
            self._handle = None

    def add_packed(self, sample, first_unit, mate1, mate2=None, umis=None):
        """Units [first_unit, first_unit + n) of `sample` as common.PackedReads (mate2: paired sets); umis: uint32[n],
        the units' UMIs, in a set made with umi_bases and only there."""
        if (mate2 is not None) != self.paired:
            raise ValueError('a %s set takes %s' % (('paired', 'both mates') if self.paired else ('single-ended', 'mate 1 alone')))
        if umis is not None:
            umis = numpy.ascontiguousarray(umis, dtype=numpy.uint32)
            if umis.shape != (mate1.n_reads,):
                raise ValueError('%d UMIs for %d units' % (umis.size, mate1.n_reads))
            _native.check(_native.hip().skm_sample_set_add_packed_umis(
                self._handle, int(sample), int(first_unit), ctypes.byref(mate1.raw),
                ctypes.byref(mate2.raw) if mate2 is not None else None, _native.ptr(umis, _native.c_u32p) if umis.size else None))
            return
        _native.check(_native.hip().skm_sample_set_add_packed(
            self._handle, int(sample), int(first_unit), ctypes.byref(mate1.raw),
            ctypes.byref(mate2.raw) if mate2 is not None else None))

    def add_batch(self, sample, first_unit, batch):
        """The same for a common.ReadBatch (text: bases back to back + offsets)."""
        if batch.count and bool(batch.paired) != self.paired:
            raise ValueError('a %s batch for a %s set' % ('paired' if batch.paired else 'single-ended',
                                                          'paired' if self.paired else 'single-ended'))
        _native.check(_native.hip().skm_sample_set_add_batch(
            self._handle, int(sample), int(first_unit), batch.bases.ctypes.data,
            _native.ptr(batch.offsets, _native.c_i64p), batch.count))

    def add_sample(self, sample, read_feeder):
        """All reads of `sample` from a feeder of its own: a common.PackedReadFeeder (parsed completely
        by this thread, then added as in-order segments) or an iterable of ReadBatch / (count, names,
        reads) items.  Returns the sample's units."""
        units = 0
        pieces = []
        for item in read_feeder:
            if isinstance(item, PackedReads):
                pieces.append(item.held())            # (a reader's piece is valid until its next one)
                continue
            if pieces:
                raise ValueError('packed and text reads in one sample')
            batch = item if isinstance(item, ReadBatch) else ReadBatch.from_lists(*item)
            self.add_batch(sample, units, batch)
            units += batch.count
        for first_unit, mate1, mate2 in sample_segments(pieces, self.paired):
            if first_unit != units:
                raise ValueError('sample %d: its reads begin at unit %d, not %d' % (sample, first_unit, units))
            self.add_packed(sample, first_unit, mate1, mate2)
            units = first_unit + mate1.n_reads
        if units == 0:
            self.add_batch(sample, 0, ReadBatch(0, numpy.zeros(0, dtype=numpy.uint8), numpy.zeros(1, dtype=numpy.int64),
                                                self.paired))
        return units

    def sync(self):
        """Wait for everything added to be mapped; raises the set's failure."""
        _native.check(_native.hip().skm_sample_set_sync(self._handle))

    def map_relaunches(self):
        """MapResult.timing()['map_relaunches'] of the set's launches (waits for what was added)."""
        n = ctypes.c_int64()
        _native.check(_native.hip().skm_sample_set_map_relaunches(self._handle, ctypes.byref(n)))
        return n.value

    def __bool__(self):
        return True                   # (a handle, not a container: its truth waits for nothing)

    def __len__(self):
        """The samples added so far (nothing is waited for)."""
        n = ctypes.c_int64()
        _native.check(_native.hip().skm_sample_set_summary(self._handle, 0, ctypes.byref(n), None))
        return n.value

    def sizes(self):
        """int64[n_samples, 4]: per sample (classes, class_map rows, unaligned, total units) -- MapResult.sizes()."""
        n = ctypes.c_int64(len(self))
        out = numpy.zeros((n.value, 4), dtype=numpy.int64)
        _native.check(_native.hip().skm_sample_set_summary(self._handle, n.value, ctypes.byref(n),
                                                           _native.ptr(out, _native.c_i64p) if out.size else None))
        return out

    @property
    def fragment_length_counts(self):
        """The set's pooled histogram: the sum over all its samples."""
        fld = numpy.zeros(MAX_FRAGMENT_LENGTH, dtype=numpy.int64)
        _native.check(_native.hip().skm_sample_set_histogram(self._handle, _native.ptr(fld, _native.c_i64p)))
        return fld

    @property
    def sample_fragment_length_counts(self):
        """int64[n_samples, 2000]: row i is MapResult.fragment_length_counts of sample i mapped alone
        (a set made with per_sample_lengths; ValueError otherwise)."""
        if not self.per_sample_lengths:
            raise ValueError('the set keeps one pooled histogram: make it with per_sample_lengths=True')
        # (samples may be added meanwhile: the call says when there are more than the rows it was given)
        while True:
            fld = numpy.zeros((len(self), MAX_FRAGMENT_LENGTH), dtype=numpy.int64)
            code = _native.hip().skm_sample_set_histograms(self._handle, fld.shape[0],
                                                           _native.ptr(fld, _native.c_i64p) if fld.size else None)
            if code == _native.SKM_ERR_ARG and len(self) > fld.shape[0]:
                continue
            _native.check(code)
            return fld

    def harmonic_mean_fragment_lengths(self):
        """One number per sample: MapResult.harmonic_mean_fragment_length of the sample mapped alone."""
        return harmonic_mean_fragment_lengths(self.sample_fragment_length_counts)

    def quantify(self, return_iters=False, return_effective_lengths=False):
        """infer.quantify(summary) for every sample of the set in shared EM launches
        (skm_sample_set_quantify): f8[n_samples, n_tx] TPM, row i bit for bit what quantify() gives on
        summarize()[i] -- sample i's own effective lengths with per_sample_lengths, the pooled ones
        otherwise; zeros for a sample without aligned units.  Optionally the EM steps per sample and
        the effective lengths [n_samples, n_tx].  NativeError SKM_ERR_UNDEFINED when a sample leaves
        no abundance above the floor, as quantify() on it."""
        from .infer import REL_TOL, X_FLOOR
        lengths = numpy.ascontiguousarray(self.index.transcripts['length'], dtype='f8')
        while True:       # (samples may be added meanwhile: the call says when there are more than the rows it was given)
            cap = len(self)
            n = ctypes.c_int64(cap)
            rows = max(cap, 1)
            tpm = numpy.zeros((rows, lengths.size), dtype='f8')
            effective = numpy.zeros((rows, lengths.size), dtype='f8') if return_effective_lengths else None
            iters = numpy.zeros(rows, dtype=numpy.int64)
            code = _native.hip().skm_sample_set_quantify(
                self._handle, _native.ptr(lengths, _native.c_f64p), lengths.size, REL_TOL, X_FLOOR, 0, cap,
                ctypes.byref(n), _native.ptr(tpm, _native.c_f64p),
                _native.ptr(effective, _native.c_f64p) if effective is not None else None, _native.ptr(iters, _native.c_i64p))
            if code == _native.SKM_ERR_ARG and n.value > cap:
                continue
            _native.check(code)
            break
        out = (tpm[:n.value],)
        if return_iters:
            out += (iters[:n.value],)
        if return_effective_lengths:
            out += (effective[:n.value],)
        return out if len(out) > 1 else out[0]

    def export(self):
        """[(class_offsets, class_targets, class_counts, first_seen), ...] per sample, each as
        MapResult.export() gives them for the sample alone (first_seen counted inside the sample)."""
        sizes = self.sizes()
        n_classes, n_rows = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
        bounds = numpy.zeros(len(sizes) + 1, dtype=numpy.int64)
        offsets = numpy.zeros(n_classes + 1, dtype=numpy.int64)
        targets = numpy.zeros(max(n_rows, 1), dtype=numpy.int32)
        counts = numpy.zeros(max(n_classes, 1), dtype=numpy.int64)
        first = numpy.zeros(max(n_classes, 1), dtype=numpy.int64)
        _native.check(_native.hip().skm_sample_set_export(
            self._handle, _native.ptr(bounds, _native.c_i64p), _native.ptr(offsets, _native.c_i64p),
            _native.ptr(targets, _native.c_i32p), _native.ptr(counts, _native.c_i64p), _native.ptr(first, _native.c_i64p)))
        tables = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            rows = offsets[lo:hi + 1]
            tables.append((rows - rows[0], targets[rows[0]:rows[-1]].copy(), counts[lo:hi].copy(), first[lo:hi].copy()))
        return tables

    def summarize(self):
        """[SummarizedResult, ...] per sample, as MapResult.summarize() (seekmer/mapper.py:77-104).  By
        default every item carries the POOLED histogram and the effective lengths that follow from it
        (one shared, read-only pair of arrays), i.e. what the samples' MapResults hold after
        impute.pool_fragment_lengths.  With per_sample_lengths item i carries sample i's own histogram
        and effective lengths: read-only rows of two arrays, the lengths of all samples made in one
        device call.  With a length model the histograms are those, and every item carries the model's
        effective lengths: one shared row from one launch."""
        sizes = self.sizes()
        tables = self.export()
        lengths = numpy.ascontiguousarray(self.index.transcripts['length'], dtype='f8')
        if self.per_sample_lengths:
            flds = self.sample_fragment_length_counts[:len(sizes)]
            if len(flds) != len(sizes):
                raise RuntimeError('samples were added while the set was summarized')
            flds.setflags(write=False)
        else:
            fld = self.fragment_length_counts
            fld.setflags(write=False)
            flds = [fld] * len(sizes)
        if self._length_weights is not None:
            effective = _effective_lengths_weights(lengths, self._length_weights, self.device)[0]
            effective.setflags(write=False)
            effectives = [effective] * len(sizes)
        elif self.per_sample_lengths:
            effectives = _effective_lengths_many(lengths, flds, self.device)
            effectives.setflags(write=False)
        else:
            effective = _effective_lengths(lengths, fld, self.device)
            effective.setflags(write=False)
            effectives = [effective] * len(sizes)
        summaries = []
        for i, ((offsets, targets, counts, _), (_, _, unaligned, _)) in enumerate(zip(tables, sizes)):
            if targets.size:
                class_ids = numpy.repeat(numpy.arange(counts.size, dtype=numpy.int64), numpy.diff(offsets))
                class_map = numpy.vstack([class_ids, targets.astype(numpy.int64)])
            else:
                class_map = numpy.asarray([]).T
            class_count = counts.astype('f8')
            aligned = class_count.sum()
            summaries.append(SummarizedResult(
                aligned=int(aligned), unaligned=int(unaligned), total=int(aligned + unaligned), class_map=class_map,
                class_count=class_count, fragment_length_frequencies=flds[i], effective_lengths=effectives[i],
                class_offsets=offsets, class_targets=targets, length_model=self.length_model))
        return summaries


def map_sample_set(index, read_feeders, job_count=1, device=0, strand=None, per_sample_lengths=False,
                   length_model=None, bias=False):
    """map_multiple_samples for many small samples (single cells): sample i = read_feeders[i], all of
    them mapped through ONE SampleSet in shared launches.  Each of `job_count` threads takes a sample
    at a time, parses its files completely and adds it; results do not depend on the thread count.
    The feeders must agree on paired / single-ended.  strand: None, 'fr' or 'rf' for every sample.
    per_sample_lengths: every sample keeps its own fragment-length histogram (SampleSet).
    length_model: None or (mean, sd), for every sample (SampleSet).
    bias: the set counts every sample's first hexamers (SampleSet.bias_observed).
    A failed sample raises."""
    strand_mode(strand)
    read_feeders = list(read_feeders)
    if job_count < 1:
        raise ValueError('job_count must be at least 1, not %r' % (job_count,))
    if not read_feeders:
        raise ValueError('no samples')
    layouts = {bool(feeder.paired) for feeder in read_feeders}     # (every feeder of common says which it is)
    if len(layouts) != 1:
        raise ValueError('paired and single-ended samples in one set')
    sample_set = SampleSet(index, layouts.pop(), device=device, strand=strand, per_sample_lengths=per_sample_lengths,
                           length_model=length_model, bias=bias)
    if job_count == 1:
        for sample, read_feeder in enumerate(read_feeders):
            sample_set.add_sample(sample, read_feeder)
    else:
        pool = multiprocessing.pool.ThreadPool(job_count)
        pending = [pool.apply_async(sample_set.add_sample, args=(sample, read_feeder))
                   for sample, read_feeder in enumerate(read_feeders)]
        pool.close()
        pool.join()
        for job in pending:
            job.get()                     # re-raises what the worker raised
    sample_set.sync()
    return sample_set


# ---- cell barcodes: a pooled run split into its cells (include/seekmer_hip.h, skm_barcodes_*) ---------------

DEMUX_CHUNK_UNITS = 1 << 22         # units grouped and gathered at a time (SKM_DEMUX_CHUNK_UNITS: fewer, for tests)
BARCODE_STATS = ('exact', 'corrected', 'ambiguous', 'no_match', 'unreadable')    # skm_barcodes_assign's stats[5]
MAX_BARCODE_LENGTH = 32
MAX_UMI_LENGTH = 16


def check_umi_mismatches(umi_mismatches, umi_length):
    """umi_mismatches as an int: 0 or 1, and 1 only with UMIs (umi_length > 0); ValueError otherwise"""
    if isinstance(umi_mismatches, bool) or umi_mismatches not in (0, 1):
        raise ValueError('UMI mismatches must be 0 or 1, not %r' % (umi_mismatches,))
    if umi_mismatches and not int(umi_length):
        raise ValueError('UMI mismatches go with UMIs: give their length (--umi-length L)')
    return int(umi_mismatches)


def check_whitelist(barcodes, names=None):
    """The whitelist rules ("Cell barcodes") -> (barcodes, names) as lists of str: one
    length of 1..32, upper-case ACGT only, no barcode twice; names (default: the barcodes) unique and usable as
    folder names.  ValueError otherwise; nothing native is touched."""
    barcodes = [b.decode() if isinstance(b, bytes) else str(b) for b in barcodes]
    names = list(barcodes) if names is None else [n.decode() if isinstance(n, bytes) else str(n) for n in names]
    if not barcodes:
        raise ValueError('the whitelist holds no barcode')
    if len(names) != len(barcodes):
        raise ValueError('%d names for %d barcodes' % (len(names), len(barcodes)))
    length = len(barcodes[0])
    if not 1 <= length <= MAX_BARCODE_LENGTH:
        raise ValueError('barcodes of %d bases: 1 to %d are possible' % (length, MAX_BARCODE_LENGTH))
    seen = set()
    for barcode in barcodes:
        if len(barcode) != length:
            raise ValueError('barcode %r is not %d bases long like the first' % (barcode, length))
        if barcode.strip('ACGT'):
            raise ValueError('barcode %r holds a character other than upper-case A, C, G, T' % (barcode,))
        if barcode in seen:
            raise ValueError('barcode %r is listed twice' % (barcode,))
        seen.add(barcode)
    seen = set()
    for name in names:
        if name in ('', '.', '..') or '/' in name:
            raise ValueError('%r cannot name a cell\'s output folder' % (name,))
        if name in seen:
            raise ValueError('cell name %r is used twice' % (name,))
        seen.add(name)
    return barcodes, names


def read_whitelist(path):
    """A whitelist file (possibly compressed) -> (barcodes, names): one barcode per line, an optional second
    tab-separated column names the cell (default: the barcode); lines that start with '#' and empty lines are
    skipped.  ValueError for anything check_whitelist refuses."""
    barcodes, names = [], []
    with decompress_and_open(path) as lines:
        for line in lines:
            line = line.decode() if isinstance(line, bytes) else line
            line = line.rstrip('\r\n')
            if not line or line.startswith('#'):
                continue
            fields = line.split('\t')
            if len(fields) > 2:
                raise ValueError('whitelist line %r: a barcode and at most one more column, the cell\'s name' % (line,))
            barcodes.append(fields[0])
            names.append(fields[1] if len(fields) == 2 else fields[0])
    return check_whitelist(barcodes, names)


class BarcodeTable:
    """A whitelist of cell barcodes on the device (skm_barcodes): cell i = barcodes[i].  ``assign`` gives every
    read of a piece of barcode reads its cell by the rule of DESIGN.md section 4, "Cell barcodes" (exact, or the
    one entry at Hamming distance 1); ``cell_units`` int64[n] and ``stats`` int64[5] (BARCODE_STATS: exact,
    corrected, ambiguous, no match, short or unreadable) run over all pieces assigned so far."""

    def __init__(self, barcodes, names=None, device=0):
        self.barcodes, self.names = check_whitelist(barcodes, names)
        self.length = len(self.barcodes[0])
        self.device = device
        self.cell_units = numpy.zeros(len(self.barcodes), dtype=numpy.int64)
        self.stats = numpy.zeros(len(BARCODE_STATS), dtype=numpy.int64)
        self._handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_barcodes_create(device, ''.join(self.barcodes).encode(), len(self.barcodes),
                                                        self.length, ctypes.byref(self._handle)))

    @classmethod
    def from_file(cls, path, device=0):
        return cls(*read_whitelist(path), device=device)

    def __len__(self):
        return len(self.barcodes)

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            try:
                _native.hip().skm_barcodes_destroy(handle)
            except Exception:
                pass
            self._handle = None

    def assign(self, piece, start=0, mismatches=1):
        """int32[piece.n_reads]: the cell of every read whose bases [start, start + L) are a whitelist entry or one
        substitution away from exactly one, -1 for every other read."""
        cell = numpy.full(max(piece.n_reads, 1), -1, dtype=numpy.int32)
        _native.check(_native.hip().skm_barcodes_assign(
            self._handle, ctypes.byref(piece.raw), int(start), int(mismatches), _native.ptr(cell, _native.c_i32p),
            _native.ptr(self.cell_units, _native.c_i64p), _native.ptr(self.stats, _native.c_i64p)))
        return cell[:piece.n_reads]


def group_units(sample, n_samples, device=0):
    """A run of units by sample on the GPU (skm_units_group): sample int32[n], negative = dropped ->
    (order int32[kept], offsets int64[n_samples + 1]): order = the kept units by ascending sample, in their
    original order inside a sample -- numpy.argsort(sample, kind='stable') without the dropped units."""
    sample = numpy.ascontiguousarray(sample, dtype=numpy.int32)
    order = numpy.zeros(max(sample.size, 1), dtype=numpy.int32)
    offsets = numpy.zeros(int(n_samples) + 1, dtype=numpy.int64)
    _native.check(_native.hip().skm_units_group(
        device, _native.ptr(sample, _native.c_i32p) if sample.size else None, sample.size, int(n_samples),
        _native.ptr(order, _native.c_i32p), _native.ptr(offsets, _native.c_i64p)))
    return order[:offsets[-1]], offsets


def umi_windows(piece, start, length, cell=None, device=0):
    """The UMIs of a piece of barcode reads on the GPU (skm_umi_windows): bases [start, start + length) of every
    read, 1 <= length <= 16, as uint32 (2 bits a base, first base in the top bits of the 2 * length used) ->
    (umi uint32[n], n_unreadable).  A read too short for the window, or with a position there that is not an
    upper-case ACGT, has UMI 0 and is counted; with `cell` (int32[n], changed in place) it also gets cell -1."""
    n = piece.n_reads
    umi = numpy.zeros(max(n, 1), dtype=numpy.uint32)
    unreadable = ctypes.c_int64(0)
    if cell is not None and (cell.dtype != numpy.int32 or cell.shape != (n,) or not cell.flags.c_contiguous
                             or not cell.flags.writeable):
        raise ValueError('cell: a writeable contiguous int32 array of the piece\'s %d reads' % n)
    _native.check(_native.hip().skm_umi_windows(
        device, ctypes.byref(piece.raw), int(start), int(length),
        _native.ptr(cell, _native.c_i32p) if cell is not None and n else None, _native.ptr(umi, _native.c_u32p),
        ctypes.byref(unreadable)))
    return umi[:n], unreadable.value


# ---- cell discovery: a whitelist from the barcode reads themselves (include/seekmer_hip.h, skm_barcode_census_*) ----

CENSUS_STATS = ('counted', 'short', 'unreadable')           # skm_barcode_census_add's stats[3]
CENSUS_INFO = ('rank', 'rank_count', 'threshold', 'candidates', 'dropped', 'picked')      # skm_barcode_census_pick's info[6]
MAX_DISCOVERED_CELLS = 1 << 24      # what skm_units_group takes


def barcode_strings(keys, length):
    """The 2 * length code bits of barcodes (uint64; A0 C1 G2 T3, first base in the top bits) as a list of str."""
    keys = numpy.asarray(keys, dtype=numpy.uint64)
    if keys.size == 0:
        return []
    shifts = (2 * numpy.arange(length - 1, -1, -1)).astype(numpy.uint64)
    letters = numpy.frombuffer(b'ACGT', dtype=numpy.uint8)[((keys[:, None] >> shifts) & numpy.uint64(3)).astype(numpy.intp)]
    return [row.tobytes().decode() for row in letters]


class BarcodeCensus:
    """An exact count of every distinct barcode of the pieces added, in HBM (skm_barcode_census; DESIGN.md section 4,
    "Cell discovery").  The window of a read is its bases [start, start + length); a shorter read is short, a window
    with any position that is not an upper-case ACGT unreadable, every other window counted.  ``stats`` int64[3]
    (CENSUS_STATS) runs over all pieces added so far; len() is the number of distinct barcodes."""

    def __init__(self, length, device=0):
        self.length = int(length)
        self.device = device
        self.stats = numpy.zeros(len(CENSUS_STATS), dtype=numpy.int64)
        self._handle = ctypes.c_void_p()
        _native.check(_native.hip().skm_barcode_census_create(device, self.length, ctypes.byref(self._handle)))

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            try:
                _native.hip().skm_barcode_census_destroy(handle)
            except Exception:
                pass
            self._handle = None

    def add(self, piece, start=0):
        _native.check(_native.hip().skm_barcode_census_add(self._handle, ctypes.byref(piece.raw), int(start),
                                                           _native.ptr(self.stats, _native.c_i64p)))

    def _size(self):
        distinct, counted = ctypes.c_int64(), ctypes.c_int64()
        _native.check(_native.hip().skm_barcode_census_size(self._handle, ctypes.byref(distinct), ctypes.byref(counted)))
        return distinct.value, counted.value

    def __len__(self):
        return self._size()[0]

    def ranked(self, limit=None):
        """(barcodes as str, counts int64): the census by count descending, then barcode ascending (A < C < G < T) --
        the first `limit` entries, or all of them.  Ranked on the device."""
        n = len(self) if limit is None else min(int(limit), len(self))
        keys, counts = numpy.zeros(max(n, 1), dtype=numpy.uint64), numpy.zeros(max(n, 1), dtype=numpy.int64)
        _native.check(_native.hip().skm_barcode_census_ranked(self._handle, n, _native.ptr(keys, _native.c_u64p),
                                                              _native.ptr(counts, _native.c_i64p)))
        return barcode_strings(keys[:n], self.length), counts[:n]

    def pick(self, expect_cells, drop_neighbours=True):
        """The cells by the rule of DESIGN.md section 4, "Cell discovery" -> (barcodes as str, counts int64, info):
        the picked barcodes in ranked order; info maps CENSUS_INFO to numbers.  ValueError for expect_cells < 1 and for
        a census without a counted barcode."""
        if int(expect_cells) < 1:
            raise ValueError('%r expected cells: 1 at least' % (expect_cells,))
        if len(self) == 0:
            raise ValueError('no readable barcode')
        info = numpy.zeros(len(CENSUS_INFO), dtype=numpy.int64)
        cap = min(len(self), max(4 * int(expect_cells), 1024))
        while True:
            keys, counts = numpy.zeros(cap, dtype=numpy.uint64), numpy.zeros(cap, dtype=numpy.int64)
            code = _native.hip().skm_barcode_census_pick(
                self._handle, int(expect_cells), 1 if drop_neighbours else 0, cap, _native.ptr(keys, _native.c_u64p),
                _native.ptr(counts, _native.c_i64p), _native.ptr(info, _native.c_i64p))
            if code == _native.SKM_ERR_STATE and info[5] > cap:
                cap = int(info[5])                    # (more than the first guess: the call has said how many)
                continue
            _native.check(code)
            n = int(info[5])
            return barcode_strings(keys[:n], self.length), counts[:n], dict(zip(CENSUS_INFO, info.tolist()))


def discover_barcodes(barcode_feeder, length, expect_cells, start=0, drop_neighbours=True, device=0, n_units=None):
    """The cell barcodes of a pooled run from its barcode reads alone -> (barcodes, counts, info), as
    BarcodeCensus.pick, info also holding CENSUS_STATS over the run's units, 'distinct', 'units' and every candidate in
    ranked order ('candidate_barcodes', 'candidate_counts').  barcode_feeder:
    a single-ended PackedReadFeeder over the barcode file, drained here (map_barcoded reads the file again with a
    feeder of its own); n_units: the units of the run where the cDNA files hold fewer records than the barcode file
    (map_barcoded's cut; default: all the barcode file's)."""
    if not 1 <= int(length) <= MAX_BARCODE_LENGTH:
        raise ValueError('barcodes of %d bases: 1 to %d are possible' % (length, MAX_BARCODE_LENGTH))
    if int(expect_cells) < 1:
        raise ValueError('%r expected cells: 1 at least' % (expect_cells,))
    if int(start) < 0:
        raise ValueError('a barcode that starts at base %d' % start)
    if barcode_feeder.paired or len(barcode_feeder.paths) != 1:
        raise ValueError('one barcode file, read single-ended')
    if n_units is None:
        n_units = fastq_records(barcode_feeder.paths[0])
    census = BarcodeCensus(length, device=device)
    units = 0
    for piece in barcode_feeder:
        if piece.is_cut or piece.n_reads == 0 or units >= n_units:
            continue
        if piece.first_read != units:
            raise ValueError('the barcode reads do not follow each other (read %d after %d)' % (piece.first_read, units))
        if units + piece.n_reads > n_units:
            piece = _slice_piece(piece, 0, n_units - units)
        census.add(piece, start=start)
        units += piece.n_reads
    if units != n_units:
        raise ValueError('the barcode file gave %d reads, its lines said %d' % (units, n_units))
    barcodes, counts, info = census.pick(expect_cells, drop_neighbours=drop_neighbours)
    if len(barcodes) > MAX_DISCOVERED_CELLS:
        raise ValueError('%d barcodes picked, %d are possible: lower --discover-cells' % (len(barcodes), MAX_DISCOVERED_CELLS))
    info.update(zip(CENSUS_STATS, census.stats.tolist()), distinct=len(census), units=int(n_units))
    info['candidate_barcodes'], info['candidate_counts'] = census.ranked(info['candidates'])
    return barcodes, counts, info


class _Gathered:
    """One mate's reads of a chunk in grouped order (skm_packed_gather): arrays of its own, cut into the cells'
    segments without another copy."""

    def __init__(self, held, first_unit, order):
        """held: consecutive pieces of one stream, the first of which holds unit `first_unit`'s predecessor or
        it; order: chunk-relative unit numbers, relative to first_unit."""
        sources = (_native.PackedReads * len(held))()
        for k, piece in enumerate(held):
            ctypes.memmove(ctypes.byref(sources[k]), ctypes.byref(piece.raw), ctypes.sizeof(_native.PackedReads))
        at = numpy.ascontiguousarray(order + numpy.int32(first_unit - held[0].first_read), dtype=numpy.int32)
        self.code_words = max(piece.code_words for piece in held)
        cap = sum(piece.raw.n_exceptions for piece in held)
        self.codes = numpy.empty((at.size, self.code_words), dtype=numpy.uint64)
        self.lengths = numpy.empty(at.size, dtype=numpy.uint32)
        self.exception_reads = numpy.empty(max(cap, 1), dtype=numpy.uint32)
        self.exception_masks = numpy.empty((max(cap, 1), max(self.code_words, 1)), dtype=numpy.uint32)
        n = ctypes.c_int64()
        _native.check_host(_native.host().skm_packed_gather(
            sources, len(held), _native.ptr(at, _native.c_i32p), at.size, self.code_words, self.codes.ctypes.data,
            self.lengths.ctypes.data, self.exception_reads.ctypes.data, self.exception_masks.ctypes.data, cap,
            ctypes.byref(n)), 'skm_packed_gather')
        self.exception_reads = self.exception_reads[:n.value]
        self.exception_masks = self.exception_masks[:n.value]
        self.stream = held[0].stream
        self.paired = held[0].paired

    def segment(self, lo, hi):
        a, b = numpy.searchsorted(self.exception_reads, (lo, hi))
        return PackedReads.from_arrays(self.stream, 0, self.codes[lo:hi], self.lengths[lo:hi],
                                       self.exception_reads[a:b] - numpy.uint32(lo), self.exception_masks[a:b],
                                       paired=self.paired)


def demux_chunks(pieces, paired, sample, n_samples, chunk_units, group, add, umi=None):
    """Phase 2 of map_barcoded: the cDNA pieces of a pooled run, as a packed reader hands them out (one stream
    single-ended, two paired, each numbered by unit), against sample[u] for the run's units (int32, negative =
    dropped).  The streams are paired by unit as sample_segments pairs them; every `chunk_units` units that all
    streams cover are grouped -- group(sample[a:b], n_samples) -> (order, offsets), mapper.group_units -- each
    mate is gathered once into that order (skm_packed_gather), and every sample present gets one
    add(sample, first_unit, mate1, mate2 or None) with first_unit = its units so far.  The chunks are
    [0, c), [c, 2c), ... whatever the pieces' sizes; reads beyond sample.size units are dropped.  With umi (one
    value per unit of the run) every add also gets umis=, the values of exactly the segment's units in their
    order.  Returns (int64[n_samples] units added per sample, units walked)."""
    n_units = int(sample.size)
    chunk_units = max(1, int(chunk_units))
    streams = ([], []) if paired else ([],)
    ends = [0] * len(streams)
    added = numpy.zeros(max(int(n_samples), 1), dtype=numpy.int64)
    done = 0

    def flush(upto):
        nonlocal done
        while done < upto:
            end = min(done + chunk_units, upto)
            order, offsets = group(sample[done:end], n_samples)
            if len(order):
                mates = [_Gathered(held, done, order) for held in streams]
                umis = umi[done:end][order] if umi is not None else None
                for s in numpy.flatnonzero(numpy.diff(offsets)):
                    lo, hi = int(offsets[s]), int(offsets[s + 1])
                    segments = [mate.segment(lo, hi) for mate in mates]
                    if umis is not None:
                        add(int(s), int(added[s]), segments[0], segments[1] if paired else None, umis=umis[lo:hi])
                    else:
                        add(int(s), int(added[s]), segments[0], segments[1] if paired else None)
                    added[s] += hi - lo
            done = end
            for held in streams:          # (a piece that ends at or below `done` is not needed again)
                while held and held[0].first_read + held[0].n_reads <= done:
                    held.pop(0)

    for piece in pieces:
        if piece.stream not in range(len(streams)):
            raise ValueError('stream %d of a %s run' % (piece.stream, 'paired' if paired else 'single-ended'))
        if not piece.is_cut and piece.n_reads == 0:
            continue
        k, first = piece.stream, piece.first_read
        if first >= n_units:
            continue                      # (the surplus of a longer file)
        if first < ends[k]:               # a piece, or a cut, that replaces the reads from `first` on
            if first < done:
                raise ValueError('stream %d takes back unit %d, which is already in the set' % (k, first))
            held = streams[k]
            while held and held[-1].first_read >= first:
                held.pop()
            if held and held[-1].first_read + held[-1].n_reads > first:
                held[-1] = _slice_piece(held[-1], 0, first - held[-1].first_read)
            ends[k] = first
        if piece.is_cut:
            continue
        if first != ends[k]:
            raise ValueError('the reads of stream %d do not follow each other (unit %d after %d)' % (k, first, ends[k]))
        streams[k].append(piece.held())
        ends[k] = first + piece.n_reads
        ready = min(min(ends), n_units)
        flush(done + (ready - done) // chunk_units * chunk_units)
    flush(min(min(ends), n_units))
    return added[:int(n_samples)], done


def fastq_records(path, threads=4):
    """The records of a plain FASTQ file by the reference's rule (lines 4u .. 4u + 3 are record u whatever they
    hold; a trailing name line alone is none), from its newlines alone (skm_fastq_count_newlines)."""
    chunk = PackedReadFeeder.COUNT_CHUNK
    size = os.stat(path).st_size
    if size == 0:
        return 0
    n_chunks = (size + chunk - 1) // chunk
    counts = numpy.zeros(n_chunks, dtype=numpy.int64)
    open_line = ctypes.c_int(0)
    _native.check_host(_native.host().skm_fastq_count_newlines(
        str(path).encode(), chunk, 0, 1, max(1, int(threads)), _native.ptr(counts, _native.c_i64p), n_chunks,
        ctypes.byref(open_line)), 'skm_fastq_count_newlines')
    return (int(counts.sum()) + open_line.value + 2) // 4


def _demux_chunk_units():
    value = os.environ.get('SKM_DEMUX_CHUNK_UNITS')
    if value is None:
        return DEMUX_CHUNK_UNITS
    if not value.isdigit() or not 1 <= int(value) <= DEMUX_CHUNK_UNITS:
        raise ValueError('SKM_DEMUX_CHUNK_UNITS must be a whole number from 1 to %d, not %r' % (DEMUX_CHUNK_UNITS, value))
    return int(value)


def map_barcoded(index, table, barcode_feeder, read_feeder, paired, start=0, mismatches=1, min_units=1, device=0,
                 strand=None, per_sample_lengths=False, length_model=None, bias=False, umi_start=0, umi_length=0,
                 umi_mismatches=0):
    """One pooled run -> a SampleSet with one sample per kept cell.  table: a BarcodeTable; barcode_feeder: a
    single-ended PackedReadFeeder over the barcode file; read_feeder: a PackedReadFeeder over the pooled cDNA
    file (or pair of files).  The run holds min(records) units over these files (zip of the reference's feeders);
    a surplus in any file is dropped with one log line.

    Phase 1 drains the barcode file and assigns every piece on the GPU; cell[] of the whole run stays on the
    host (4 bytes a unit).  The kept cells are those with at least `min_units` assigned units, numbered densely
    in whitelist order: sample k of the set is cell kept[k].  Phase 2 walks the cDNA pieces in unit order
    (demux_chunks: at most DEMUX_CHUNK_UNITS units a chunk, SKM_DEMUX_CHUNK_UNITS in the environment for fewer)
    and adds every cell's reads of a chunk as one in-order segment.  Every kept cell goes through the set whatever
    its size.  Returns (SampleSet, kept int64[n_kept], stats): stats maps BARCODE_STATS to counts over the run's
    units, 'units' to their number and 'records' to the files' record counts (barcode file, cDNA files).

    umi_length (1..16; needs per_sample_lengths): the UMI of a unit is bases [umi_start, umi_start + umi_length) of its
    barcode read (umi_windows, on every barcode piece after its assign; umi[] of the run stays on the host beside
    cell[], 4 bytes a unit).  A unit without a readable UMI belongs to no cell; the cells' units -- stats['cell_units'],
    what min_units looks at -- are counted again from the final cell[] (stats['cell_assigned'] keeps the barcodes'
    count), and stats gains 'umi_unreadable', the units of the run without a readable UMI.  The set is made with
    umi_bases=umi_length and collapses duplicates (SampleSet); stats['cell_survivors'] int64[whitelist] are the units
    it left every kept cell (0 for a cell that is not kept) and stats['umi_duplicates'] those it removed.
    umi_mismatches (0 or 1; 1 needs umi_length): the set's umi_mismatches.  With 1 a unit also goes when an earlier unit
    of its cell and class has a UMI one substitution away; stats['umi_near_duplicates'] are the units that only this
    removed (0 with umi_mismatches=0), part of stats['umi_duplicates']."""
    strand_mode(strand)
    umi_start, umi_length = int(umi_start), int(umi_length)
    umi_mismatches = check_umi_mismatches(umi_mismatches, umi_length)
    if umi_length and not 1 <= umi_length <= MAX_UMI_LENGTH:
        raise ValueError('a UMI of %d bases: 1 to %d are possible' % (umi_length, MAX_UMI_LENGTH))
    if umi_start < 0 or (umi_start and not umi_length):
        raise ValueError('umi_start %d with umi_length %d' % (umi_start, umi_length))
    if umi_length and not per_sample_lengths:
        raise ValueError('UMI collapse needs per_sample_lengths')
    if int(min_units) < 1:
        raise ValueError('min_units must be at least 1, not %r' % (min_units,))
    if barcode_feeder.paired or len(barcode_feeder.paths) != 1:
        raise ValueError('one barcode file, read single-ended')
    if bool(read_feeder.paired) != bool(paired) or len(read_feeder.paths) != (2 if paired else 1):
        raise ValueError('one pooled sample: %s' % ('two cDNA files' if paired else 'one cDNA file'))
    chunk_units = _demux_chunk_units()
    records = [fastq_records(path) for path in list(barcode_feeder.paths) + list(read_feeder.paths)]
    n_units = min(records)
    if len(set(records)) != 1:
        _LOG.warning('The barcode file holds %d records, the cDNA files %s: the run is the first %d units of each',
                     records[0], ' and '.join(str(n) for n in records[1:]), n_units)
    if n_units >= 1 << 40:
        raise ValueError('a run of %d units' % n_units)
    # phase 1: the cell of every unit
    cell = numpy.full(n_units, -1, dtype=numpy.int32)
    umi = numpy.zeros(n_units, dtype=numpy.uint32) if umi_length else None
    umi_unreadable = 0
    units = 0
    units_before, stats_before = table.cell_units.copy(), table.stats.copy()       # (the table's counters run on)
    for piece in barcode_feeder:
        if piece.is_cut or piece.n_reads == 0 or units >= n_units:
            continue
        if piece.first_read != units:
            raise ValueError('the barcode reads do not follow each other (read %d after %d)' % (piece.first_read, units))
        if units + piece.n_reads > n_units:
            piece = _slice_piece(piece, 0, n_units - units)
        cell[units:units + piece.n_reads] = table.assign(piece, start=start, mismatches=mismatches)
        if umi_length:
            umi[units:units + piece.n_reads], unreadable = umi_windows(piece, umi_start, umi_length,
                                                                       cell=cell[units:units + piece.n_reads], device=device)
            umi_unreadable += unreadable
        units += piece.n_reads
    if units != n_units:
        raise ValueError('the barcode file gave %d reads, its lines said %d' % (units, n_units))
    cell_units = cell_assigned = table.cell_units - units_before
    if umi_length:                    # (the units that enter the set: those of the final cell[])
        cell_units = numpy.bincount(cell[cell >= 0], minlength=len(table)).astype(numpy.int64)
    kept = numpy.flatnonzero(cell_units >= int(min_units))
    limit = 1 << 15 if bias else 1 << 16 if per_sample_lengths else 1 << 24
    if kept.size > limit:
        raise ValueError('%d cells have at least %d units, a set holds %d at most%s: raise --min-units'
                         % (kept.size, min_units, limit, ' with --bias' if bias else ''))
    number = numpy.full(len(table) + 1, -1, dtype=numpy.int32)       # (cell -1 reads the last entry: dropped)
    number[kept] = numpy.arange(kept.size, dtype=numpy.int32)
    sample = number[cell]
    # phase 2: the reads, cell by cell, into the set
    sample_set = SampleSet(index, paired, device=device, strand=strand, per_sample_lengths=per_sample_lengths,
                           length_model=length_model, bias=bias, umi_bases=umi_length,
                           umi_mismatches=umi_mismatches)
    if kept.size:
        added, walked = demux_chunks(read_feeder, paired, sample, kept.size, chunk_units,
                                     lambda part, n: group_units(part, n, device=device), sample_set.add_packed, umi=umi)
        if walked != n_units or not numpy.array_equal(added, cell_units[kept]):
            raise ValueError('the cDNA files gave %d units, their lines said %d' % (walked, n_units))
        sample_set.sync()
    stats = {name: int(value) for name, value in zip(BARCODE_STATS, table.stats - stats_before)}
    stats.update(units=n_units, records=records, cells=int(kept.size), cell_units=cell_units)
    if umi_length:
        survivors = numpy.zeros_like(cell_units)
        removed = sample_set.umi_removed() if kept.size else numpy.zeros(0, dtype=numpy.int64)
        survivors[kept] = cell_units[kept] - removed
        stats.update(umi_unreadable=int(umi_unreadable), umi_duplicates=int(removed.sum()), cell_assigned=cell_assigned,
                     cell_survivors=survivors,
                     umi_near_duplicates=sample_set.umi_near_removed() if umi_mismatches and kept.size else 0)
    return sample_set, kept, stats
