/*
 * seekmer_hip.h -- C ABI of the MI355X (gfx950) engine behind `seekmer infer`.
 *
 * The reference (GuanLab/seekmer) has no FFI seam on this path: its Python
 * layer calls Cython extension classes directly.  Every entry point below
 * names the reference interface it replaces (file:line under
 * /root/reference); INTEGRATION.md shows the ctypes binding a maintainer
 * would add to the reference.  Plain pointers and sizes only; no exceptions
 * cross the boundary: every function returns an int status (0 = SKM_OK) and
 * skm_last_error() gives the message for the calling thread.
 *
 * Two shared libraries implement it:
 *   libseekmer_hip.so   -- everything that touches the GPU (skm_index_*,
 *                          skm_mapper_*, skm_sample_set_*, skm_quant_*, skm_bias_*,
 *                          skm_gene_*, skm_barcodes_*, skm_umi_windows, skm_units_group, skm_barcode_census_*,
 *                          skm_comm_*, skm_device_*)
 *   libseekmer_host.so  -- host-side native code with no GPU dependency
 *                          (skm_build_*, skm_fastq_*, skm_fastq_packed_*, skm_pack_*, skm_packed_gather,
 *                          skm_synth_*)
 */
#ifndef SEEKMER_HIP_H
#define SEEKMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKM_OK 0
#define SKM_ERR_ARG 1          /* bad argument */
#define SKM_ERR_HIP 2          /* HIP runtime error (message has the call) */
#define SKM_ERR_NO_DEVICE 3    /* no usable GPU */
#define SKM_ERR_COLLISION 4    /* two different class tuples share a 64-bit key */
#define SKM_ERR_STATE 5        /* call order / capacity */
#define SKM_ERR_IO 6
#define SKM_ERR_UNDEFINED 7    /* the reference's behaviour is undefined for this input */
#define SKM_ERR_COMM 8         /* RCCL error */

#define SKM_KMER_SIZE 25            /* seekmer/_kmer.pxd:9-17 */
#define SKM_MAX_FRAGMENT_LENGTH 2000 /* seekmer/_mapper.pyx:18-20 */

/* Array element layouts are the reference's numpy dtypes:
 *   kmers    {u64 kmer; i32 entry; i32 offset}                     16 B  seekmer/_common.pxd:15-17
 *   contigs  {i64 offset,length; u64 first_kmer,last_kmer;
 *             i64 target_offset,target_count}                      48 B  seekmer/_common.pxd:21-27
 *   sequences  char 'ACGT'                                               seekmer/_index_builder.pyx:568
 *   targets  {i32 entry; i32 offset}                                8 B  seekmer/_coordinate.pxd:8-10 */

const char *skm_last_error(void);
/* number of visible GPUs; SKM_ERR_NO_DEVICE when there is none */
int skm_device_count(int *count);

/* Raw HBM buffers for callers that keep batches resident (bench, pipelines). */
int skm_device_malloc(int device, int64_t bytes, void **out);
int skm_device_free(int device, void *ptr);
int skm_device_upload(int device, void *dst, const void *src, int64_t bytes);
int skm_device_download(int device, void *dst, const void *src, int64_t bytes);
int skm_device_synchronize(int device);
/* Page-locked host memory (hipHostMalloc).  A host batch that lives in it crosses PCIe by DMA
 * at the full link rate; from pageable memory the runtime stages the copy.  Plain allocator
 * signatures: skm_fastq_set_allocator takes this pair so that FASTQ slabs are page-locked. */
void *skm_pinned_alloc(size_t bytes);
void skm_pinned_free(void *ptr);
/* The GPU whose context page-locks the memory (default 0; one process per GPU sets its own before
 * the FASTQ reader's threads allocate).  The memory is portable: any device of the process may
 * copy from it. */
int skm_pinned_set_device(int device);
/* Diagnostic: rate of random 16-byte gathers over a table of `table_bytes`
 * (power of two); chain=0 independent (throughput), chain=1 dependent
 * (latency under load).  The ceiling the index probes are priced against. */
int skm_device_gather_ceiling(int device, int64_t table_bytes, int blocks, int per_lane,
                              int chain, double *gathers_per_second);
/* Diagnostics, tests: the engine's own prefix sum and stable radix sort (the class views of skm_quant_*, skm_units_group
 * and the ranking of skm_barcode_census_* rest on them) on the caller's host arrays -- upload, the production call,
 * download.  SKM_ERR_ARG for n < 0 or n >= 2^31, for NULL arrays with n > 0 (`out` of the scan: always needed), for a
 * key_kind or an end_bit outside what is listed below.
 * skm_device_scan_probe: out[0 .. n) = the exclusive prefix sums of in[0 .. n), out[n] = the total (n = 0: out[0] = 0);
 * in_place != 0 scans with input and output in ONE device buffer of n + 1 entries, the input in its first n.
 * skm_device_sort_probe: the (key, value) pairs in stable order of key & (2^min(width, 9 p) - 1), p =
 * max(1, ceil(end_bit / 9)) whole 9-bit passes, the full keys carried; key_kind 0 = uint32_t keys, 1 = uint64_t
 * (end_bit 0 .. 64), 2 = non-negative int32_t; end_bit 0 .. 32 for kinds 0 and 2.  n = 0 writes nothing. */
int skm_device_scan_probe(int device, const int64_t *in, int64_t n, int in_place, int64_t *out);
int skm_device_sort_probe(int device, int key_kind, const void *keys, const int32_t *vals, int64_t n, int end_bit,
                          void *keys_out, int32_t *vals_out);

/* ------------------------------------------------------------------ index
 * Replaces the memoryview binding of KMerIndex.__init__
 * (seekmer/_common.pyx:21-48).  Host arrays are borrowed for the call and
 * copied to HBM (the pooled sequences are re-packed to 2 bits per base); the
 * handle owns device memory only.  Limits (SKM_ERR_ARG beyond them): n_slots a
 * power of two <= 2^31, n_contigs < 2^25, n_targets + 32 n_contigs < 2^30 (the
 * contig records -- two 64-byte sides, one per end of the contig -- carry the first
 * eight targets and the junction successors of that end: one int32 address space),
 * n_bases < 2^31, at most 2^22 - 1 targets per contig.
 * skm_index_destroy gives up the caller's handle; the device copy is released once
 * every mapper created from it has been destroyed too (in either order). */
typedef struct skm_index skm_index;
int skm_index_create(const void *kmers, int64_t n_slots,
                     const void *contigs, int64_t n_contigs,
                     const char *sequences, int64_t n_bases,
                     const void *targets, int64_t n_targets,
                     int device, skm_index **out);
int skm_index_destroy(skm_index *index);
/* info[0]=n_slots [1]=n_contigs [2]=n_bases [3]=n_targets [4]=max target_count
 * [5]=device bytes held [6]=1 when every contig's first_kmer/last_kmer spell
 * its first/last k pooled bases (the mapper then takes 8-base windows at contig
 * ends from the contig row instead of the pool) [7]=1 when every contig's target
 * slice ascends by signed entry (short list merges then run on registers) */
int skm_index_info(const skm_index *index, int64_t info[8]);
/* How the device copy of the k-mer table is probed.  The reference's table is a set
 * (KMerIndex.map_kmer, seekmer/_common.pyx:54-97, returns the position stored with a k-mer
 * or none); the device keeps the same set a second time in 64-byte buckets of four entries
 * under a cheap hash, one sector per lookup.  layout[0]=1 when that copy is in use, 0 when
 * the reference's own layout is probed (a table the reference's probe does not reach
 * everywhere, or one holding a k-mer twice or with bits above 2k); [1]=buckets [2]=k-mers placed
 * [3]=placed outside their home bucket [4]=k-mers met twice or with such bits [5]=slots the
 * reference's probe does not reach
 * [6]=1 when every contig record carries its junction successors: the map_kmer results of the
 * eight k-mers a hop of _filter_targets_to_left/right (seekmer/_mapper.pyx:246-248, 308-310) can
 * ask for when it leaves the contig, computed once at upload, so that a hop reads its answer
 * from the record instead of visiting the k-mer table (results identical by construction;
 * off for a table probed in the reference's layout).  A junction k-mer that is neither the
 * first nor the last k-mer of its contig -- rare in a built index, but they exist: 39 of the 66 848
 * junction slots of the reference's chr21 test transcriptome, where a contig's extension by one base
 * spells a k-mer from the inside of another contig -- is marked "look it up".
 * [7]=slots of the signature table (0: none): per minimizer of the table's k-mers a 64-bit word
 * that says which k-mers it has; the roll past a sequencing error (_find_first_kmer,
 * seekmer/_mapper.pyx:207-216) asks it before the table -- a k-mer whose bit is clear is not in
 * the table, and a run of the read's k-mers shares a minimizer.  Results identical by
 * construction (no false negatives); SKM_NO_SIGNATURES=1 leaves it out. */
int skm_index_layout(const skm_index *index, int64_t layout[8]);
/* A download of the junction words of the contig records, for tests: succ[n_contigs * 8] and kept[n_contigs * 8]
 * in the order [contig][side][b], side 0 = the contig's end (k-mer: its tail k-mer with base b appended),
 * side 1 = its start (first k-mer with base b prepended), copied out of the records as they stand.  A word is
 * entry << 4 | 8 (the merge on the landing contig keeps what `kept` names of this contig's list) | 4 (it keeps
 * the whole running list) | kind, kind 0 = the k-mer is not in the table, 1 = it is the first k-mer of contig
 * `entry` (complemented: on the other strand), 2 = the last one, 3 = look it up; the entry is 0 for kinds 0 and 3.
 * SKM_ERR_STATE when layout[6] == 0. */
int skm_index_junctions(const skm_index *index, int32_t *succ, uint8_t *kept);
/* The lookups the mapper and the junction words are built from, one per query, for tests: (entry, offset)[n] of
 * kmers[n] (2k bits each) through mode 0 = map_kmer over the reference's layout, 1 = the bucket table's chain,
 * 2 = the bucket table with the home bucket's positions fetched with its keys; a k-mer that is not in the table
 * gives (0, -1).  Mode 3 = the signature table's verdict: entry = 1 when the k-mer may be in the table, 0 when
 * it is turned away (offset = 0).  SKM_ERR_STATE when the index has no bucket table (modes 1, 2) or no
 * signature table (mode 3). */
int skm_index_probe(const skm_index *index, int mode, const uint64_t *kmers, int64_t n, int32_t *entry,
                    int32_t *offset);
/* The transcripts' own sequences, for the sequence-bias correction (skm_bias_correct): rebuilt in HBM from
 * the index alone -- a target row (e, o) of a contig of length L with pooled bases S says T_e[o .. o + L) = S
 * for e >= 0 and T_~e[o + 25 - L .. o + 25) = revcomp(S) for e < 0 -- as 2-bit codes plus one "known" bit per
 * base; a base no row covers (a transcript shorter than 25, a k-mer the builder dropped) is unknown.
 * lengths[n_tx]: the transcript lengths (whole numbers below 2^31).  Built once per handle: a second call
 * with the same n_tx does nothing (another n_tx: SKM_ERR_STATE).  SKM_ERR_ARG when a row names a transcript
 * at or above n_tx or leaves its length.  skm_index_create keeps the host rows the pool is made from until
 * then; a handle that is never asked holds nothing of it on the device. */
int skm_index_build_transcripts(skm_index *index, const double *lengths, int64_t n_tx);
/* A download of the pool, for tests: bases_out[sum of lengths] = the transcripts back to back as 'ACGT'
 * ('N' where unknown), known_out[sum of lengths] = 1 / 0; either may be NULL.  SKM_ERR_STATE before
 * skm_index_build_transcripts. */
int skm_index_transcript_bases(skm_index *index, char *bases_out, uint8_t *known_out);

/* ------------------------------------------------------------------ mapper
 * One handle = ReadMapper + the MapResult it feeds
 * (seekmer/_mapper.pyx:31-105; seekmer/mapper.py:40-115): it maps batches
 * and accumulates the equivalence-class counter and the fragment-length
 * histogram in HBM. */
typedef struct skm_mapper skm_mapper;
int skm_mapper_create(skm_index *index, skm_mapper **out);
int skm_mapper_destroy(skm_mapper *mapper);

/* ReadMapper.__call__ for one batch (seekmer/_mapper.pyx:73-101): `bases`
 * holds the reads back to back, read r = [offsets[r], offsets[r+1]);
 * n_reads = n_units (single-ended) or 2*n_units (paired: reads 2u, 2u+1 are
 * the mates of unit u, the layout feed_pair_ended_reads yields,
 * seekmer/common.py:161-197).  Host buffers; copied to the GPU. */
int skm_mapper_map_batch(skm_mapper *mapper, const char *bases,
                         const int64_t *offsets, int64_t n_units, int paired);
/* The same without waiting for the kernels: the batch is copied to HBM on a staging stream
 * by the calling thread (returns once the host arrays are free again) and queued; one worker
 * per mapper maps the queued batches in submission order, so the copy of batch i+1 runs under
 * the kernels of batch i -- the overlap the reference gets from parsing in one thread and
 * mapping in others (seekmer/mapper.py:174-189).  Any thread may submit; integer results do
 * not depend on the interleaving.  first_unit >= 0 gives the batch's place in the sample (the
 * global index of its first unit): first-seen class order is then the -j1 order whatever the
 * submission order; -1 = after the units mapped so far.  skm_mapper_sync waits for everything
 * queued and returns the first failure; every call that reads or changes the table waits too.
 * After a failed batch the handle holds a partial table until skm_mapper_reset / _clear. */
int skm_mapper_map_batch_async(skm_mapper *mapper, const char *bases,
                               const int64_t *offsets, int64_t n_units, int paired,
                               int64_t first_unit);
/* A batch whose reads all have the same length (raw Illumina reads): `bases` holds them back to
 * back, read r = [r * read_len, (r + 1) * read_len); no offsets cross PCIe (8 bytes per read, 7 %
 * of a 2x100 bp batch), the device makes them.  The fixed-stride form of SURVEY.md 8(b).2. */
int skm_mapper_map_batch_uniform_async(skm_mapper *mapper, const char *bases, int32_t read_len,
                                       int64_t n_units, int paired, int64_t first_unit);
int skm_mapper_sync(skm_mapper *mapper);
/* An optional hint before a sample's reads arrive: about this many units will be mapped (a reader
 * knows its files' sizes).  The class table and the batch buffers are then sized once instead of
 * growing under the sample's first launches; results do not depend on it. */
int skm_mapper_expect_units(skm_mapper *mapper, int64_t n_units);
/* Reads packed on the host.
 * The mapper works on 2-bit codes and one "is an upper-case ACGT" bit per base
 * (seekmer/_kmer.pxd:253-273, seekmer/_mapper.pyx:500-501); in FASTQ text nearly every read has all
 * of those bits set.  A piece carries its reads as code words only (32 bases per u64 word, first
 * base in the top two bits, zero beyond the read's end: 32 bytes for a 100-base read) plus an
 * exception entry -- the bit plane -- for each read that holds any other character. */
#define SKM_PACKED_CUT (-1)
typedef struct skm_packed_reads {
    int32_t stream;                  /* 0 = single-end reads / mate 1 files, 1 = mate 2 files */
    int32_t code_words;              /* u64 words per read in `codes`; SKM_PACKED_CUT with n_reads == 0: a cut */
    int64_t first_read;              /* place of reads[0] in its stream = the unit it belongs to */
    int64_t n_reads;                 /* 0 = end of the sample -- or, with code_words == SKM_PACKED_CUT, a cut:
                                        the stream's reads from first_read on are dropped (the reader sends
                                        one when the mate-2 file of a pair of files was the longer one, before
                                        any read of the next pair of files) and more pieces follow */
    int64_t read_stride;             /* u64 words from one read's codes to the next (>= code_words) */
    int64_t uniform_len;             /* >= 0: every read is this long and `lengths` may be NULL */
    const uint64_t *codes;           /* read r = codes[r * read_stride .. + code_words) */
    const uint32_t *lengths;         /* [n_reads] */
    int64_t n_exceptions;
    const uint32_t *exception_reads; /* [n_exceptions] indices into this piece, ascending */
    const uint32_t *exception_masks; /* [n_exceptions][code_words]: bit 31 - i of word w set = base
                                        32 w + i is an upper-case A, C, G or T */
    const char *names;               /* stream 0 only, and only when asked for: names back to back */
    const int64_t *name_offsets;     /* [n_reads + 1] */
} skm_packed_reads;
/* ReadMapper.__call__ (seekmer/_mapper.pyx:73-101) for reads that arrive packed.  A piece is copied
 * to HBM by the calling thread (the call returns when its arrays are free again) and joins its
 * stream; the mapper's worker maps, in the background and in launches as large as what has arrived,
 * every run of units that its streams cover (single-ended: stream 0 alone; paired: unit u = read u
 * of stream 0 + read u of stream 1).  A piece whose first_read lies below the end of what its stream
 * holds replaces the reads from there on (a cut -- see skm_packed_reads -- replaces them by
 * nothing; either waits for a launch that is mapping from the replaced piece).  skm_mapper_sync -- and every call that reads the table
 * -- first maps every unit whose reads have all arrived; reads still without a mate are not part
 * of any result (zip(file1, file2): seekmer/common.py:180-197) and wait in HBM until their mates
 * come or the handle is reset, cleared or destroyed.  Class order does not depend on how the
 * pieces were cut or when they arrived: first-seen values are unit numbers. */
int skm_mapper_push_packed(skm_mapper *mapper, const skm_packed_reads *piece, int paired);
/* Drain a source of pieces (skm_fastq_packed_next with its reader as context) into the mapper
 * without leaving native code: next() until a piece with n_reads == 0 that is not a cut, every piece
 * pushed.  A source must keep the arrays of a piece valid until it has been asked for the next
 * piece BUT ONE: the copy of a piece to the GPU runs while the next piece is being fetched.
 * *n_pieces (optional) = pieces pushed. */
typedef int (*skm_packed_source)(void *context, skm_packed_reads *piece);
int skm_mapper_map_packed_source(skm_mapper *mapper, skm_packed_source next, void *context,
                                 int paired, int64_t *n_pieces);
/* Same with the batch already resident in HBM (device pointers; max_read_len
 * must bound every read length). */
int skm_mapper_map_batch_device(skm_mapper *mapper, const void *d_bases,
                                const void *d_offsets, int64_t n_units,
                                int paired, int32_t max_read_len);
/* Per-unit results of the LAST batch (what ReadMapper keeps in `results` and
 * `span`, seekmer/_mapper.pyx:83-99): any pointer may be NULL.  counts[u] =
 * number of targets, entries = signed target entries of all units back to
 * back in unit order (cap_entries bounds it; *n_entries = needed size).
 * begin / end / anchor are the MappedSpan fields (seekmer/_common.pxd:31-35);
 * nothing on the infer path reads them, so they are only written for batches
 * mapped after skm_mapper_keep_spans(mapper, 1) (SKM_ERR_STATE otherwise). */
int skm_mapper_last_batch(skm_mapper *mapper, int32_t *begin, int32_t *end,
                          int32_t *anchor_entry, int32_t *anchor_offset,
                          int32_t *counts, int32_t *entries,
                          int64_t cap_entries, int64_t *n_entries);
int skm_mapper_keep_spans(skm_mapper *mapper, int enable);
/* The read records of the LAST batch as the map kernel read them (tests): records first_read ..
 * first_read + n_reads of its n_units (single-ended) or 2 * n_units (paired: 2u, 2u + 1) records, copied
 * to out[n_reads][*record_words] u32 words.  A record is W = *words_per_read code words (u64: 32 bases a
 * word, 2 bits a base, A0 C1 G2 T3 in either case, anything else 0, the first base in the top bits),
 * then W flag words (u32: bit 31 - i of word w set = base 32 w + i is an upper-case A, C, G or T), then
 * the read's length, then zeros; codes and flags are zero beyond the read's end.  out may be NULL (the
 * two sizes only).  SKM_ERR_STATE before the first batch.
 * skm_pack_stage_reads: how many consecutive reads a workgroup of the packing kernel stages in LDS for
 * this W; 0 = reads too long for the stage, such launches take the kernel with one lane per word. */
int skm_mapper_copy_records(skm_mapper *mapper, int64_t first_read, int64_t n_reads, uint32_t *out,
                            int32_t *record_words, int32_t *words_per_read);
int skm_pack_stage_reads(int32_t words_per_read, int32_t *reads_per_block);
/* The map kernel exists twice, over two layouts of its unit contexts: packed (more contexts in a
 * workgroup's LDS; reads and target lists up to fixed bounds) and wide (everything the library accepts).
 * skm_map_geometry: which one a launch takes -- *packed 1 or 0 --, its contexts per workgroup and its
 * grid, from the launch's bounds alone: units, longest read, the index's longest target list
 * (skm_index_info: max_target_count), compute units of the device, block_cap = a cap on the grid (0: none).
 * No GPU is needed.  skm_mapper_map_layout: the same three of the mapper's last launch (SKM_ERR_STATE
 * before the first batch). */
int skm_map_geometry(int64_t n_units, int32_t max_read_len, int32_t max_target_count, int32_t cu_count,
                     int32_t block_cap, int32_t *packed, int32_t *contexts, int64_t *blocks);
int skm_mapper_map_layout(skm_mapper *mapper, int32_t *packed, int32_t *contexts, int32_t *blocks);
/* Strand-specific libraries (kallisto's --fr-stranded / --rf-stranded).  Every target entry of a
 * unit is signed: e >= 0 means mate 1 (or the single read) lies in transcript e's own orientation,
 * e < 0 that it lies antisense to transcript ~e.  SKM_STRAND_FR keeps a unit's entries with
 * e >= 0, SKM_STRAND_RF those with e < 0, in their order; the class is the tuple of their unsigned
 * ids, and a unit with no entry left is unaligned.  SKM_STRAND_NONE (the default) keeps all.  The
 * fragment-length histogram and the spans are those of the unfiltered unit; skm_mapper_last_batch
 * returns the kept (still signed) entries.  The mode applies to every batch the handle maps, not to
 * tables merged in (skm_mapper_merge*, skm_mapper_exchange_tables).  It survives skm_mapper_reset
 * and skm_mapper_clear, and can only change while the handle holds no units and has nothing queued
 * (a new handle, or after skm_mapper_reset / skm_mapper_clear): SKM_ERR_STATE otherwise,
 * SKM_ERR_ARG for an unknown mode. */
#define SKM_STRAND_NONE 0
#define SKM_STRAND_FR 1
#define SKM_STRAND_RF 2
int skm_mapper_set_strand(skm_mapper *mapper, int mode);
/* A fragment-length model for the effective lengths: p[2000], finite weights >= 0 that sum to 1
 * (mapper.fragment_length_weights makes them; SKM_ERR_ARG for a negative or non-finite one).  The
 * mapper keeps them in HBM, and skm_quant_infer then takes eff_t = sum_i max(len_t - i, 1) * p[i]
 * from them instead of from the histogram, on one rank and with a communicator (every rank must
 * hold the same weights).  NULL: back to the histogram.  It may be set or cleared at any time and
 * affects only later quantification calls; the histogram is counted and exported as ever, and
 * skm_mapper_reset / skm_mapper_clear leave the model in place. */
int skm_mapper_set_length_weights(skm_mapper *mapper, const double *p);
/* Sequence bias (--bias): a mapper asked to (enable != 0) counts, after every batch it maps, the hexamer
 * each aligned unit starts with -- the first six bases of mate 1 or of the single read, first base in the
 * top two bits of the 12-bit code; aligned = the unit's tuple is not empty after the strand filter; a unit
 * with a base among the six that is not an upper-case A, C, G or T is not counted.  The counts are exact
 * integers and do not depend on how the reads were cut into batches or pieces.  They are zeroed and kept
 * exactly where the fragment-length histogram is (skm_mapper_reset zeroes, skm_mapper_clear keeps), and
 * skm_mapper_merge* and skm_mapper_exchange_tables add no observations.  The setting survives
 * skm_mapper_reset and skm_mapper_clear and can only change while the handle holds no units and has
 * nothing queued, as skm_mapper_set_strand (SKM_ERR_STATE otherwise).  The map kernel is the same either way:
 * the counting is a kernel of its own over the batch's records.
 * skm_mapper_bias_observed: out[4096]; SKM_ERR_STATE on a mapper that does not count. */
int skm_mapper_set_bias(skm_mapper *mapper, int enable);
int skm_mapper_bias_observed(skm_mapper *mapper, int64_t out[4096]);
/* Counter sizes (MapResult.summarize, seekmer/mapper.py:77-104):
 * summary[0]=C classes [1]=M (class,target) rows [2]=unaligned [3]=total units */
int skm_mapper_summary(skm_mapper *mapper, int64_t summary[4]);
/* Classes in first-seen order (collections.Counter insertion order under -j1):
 * class_offsets[C+1], class_targets[M] unsigned ids in tuple order,
 * class_counts[C], first_seen[C] (global unit index), fld[2000]. */
int skm_mapper_export(skm_mapper *mapper, int64_t *class_offsets,
                      int32_t *class_targets, int64_t *class_counts,
                      int64_t *first_seen, int64_t *fld);
/* MapResult.merge_fragment_lengths / Counter.update with foreign data: merge
 * an exported table (e.g. another GPU's) into this one.  The classes of one call are distinct
 * tuples.  Two different tuples with one 64-bit key -- in the call, or one of them in the table --
 * refuse the merge with SKM_ERR_COLLISION (skm_mapper_merge_device likewise): a refused merge leaves
 * the unit totals (summary[2], summary[3]) and the histogram untouched; classes of the call may
 * have been added, so the table is good for skm_mapper_reset only. */
int skm_mapper_merge(skm_mapper *mapper, int64_t n_classes,
                     const int64_t *class_offsets, const int32_t *class_targets,
                     const int64_t *class_counts, const int64_t *first_seen,
                     int64_t unaligned, const int64_t *fld);
/* The same hand-over without the host: a mapper's table where it lies in HBM --
 * classes in registry order (any order: the merge is by key, first-seen values travel with the
 * classes), class c = ids[class_start[c] .. + class_len[c]) (unsigned ids, tuple order), counts as
 * doubles, plus the unit totals and the histogram -- and its merge into a mapper ON THE SAME GPU.
 * Between GPUs the arrays are first copied over xGMI (ncclSend / ncclRecv or a peer copy: n_classes
 * elements of class_start / class_len / class_count / first_seen, n_ids of ids, 2000 of fld) and the
 * struct re-pointed at the copies.  The pointers of skm_mapper_device_table stay valid until the
 * mapper maps, merges, resets or is destroyed. */
typedef struct skm_device_table {
    int32_t device;
    int64_t n_classes, n_ids;
    const int64_t *class_start;      /* [n_classes] into ids */
    const int64_t *class_len;        /* [n_classes] */
    const double *class_count;       /* [n_classes] */
    const uint64_t *first_seen;      /* [n_classes] global unit index of the class's first unit */
    const int32_t *ids;              /* [n_ids] */
    int64_t unaligned, units, first_seen_bound;
    const uint64_t *fld;             /* [2000] */
} skm_device_table;
int skm_mapper_device_table(skm_mapper *mapper, skm_device_table *out);
int skm_mapper_merge_device(skm_mapper *mapper, const skm_device_table *table);
int skm_mapper_clear(skm_mapper *mapper);           /* MapResult.clear, mapper.py:143-145 */
/* Back to the state of a fresh MapResult (counter, unit count AND histogram
 * zeroed) while keeping every HBM buffer allocated. */
int skm_mapper_reset(skm_mapper *mapper);
/* stats[0]=pack kernel ns [1]=map kernel ns [2]=class kernels ns [3]=batches
 * [4]=units (HIP-event times accumulated over batches on the mapper stream)
 * [5]=EM ns [6]=EM steps of the skm_quant_infer calls made on this mapper
 * [7]=times the class table grew with units in flight, i.e. after a pass of a batch whose bounded
 * probes deferred units (0 unless a batch outgrew what was reserved for it).
 * Test hook SKM_TEST_CLASS_SLOTS=N (power of two, 2 <= N <= 2^30; SKM_ERR_ARG otherwise), read by
 * skm_mapper_create: the table starts at N slots and the reservation ahead of a batch leaves the
 * slot count alone, so batches take the defer / grow / retry path; the growth steps themselves and
 * the sizing of the merges are those of production.  skm_mapper_clear and skm_mapper_reset keep
 * the table as large as it has grown. */
int skm_mapper_timing(skm_mapper *mapper, double stats[8]);
/* *count = map kernel launches this mapper has repeated because a batch's target ids outgrew the entry
 * arena (sized for about 8 ids a unit; the repeat runs in an arena of the first launch's cursor and
 * takes exactly what every tuple needs, so one repeat always suffices).  0 for ordinary reads.
 * Test hook SKM_TEST_MAP_BLOCKS=N (1 <= N <= 2^30; SKM_ERR_ARG otherwise), read by skm_mapper_create:
 * the map kernel's grid is min(N, what the batch and the device give), so a small batch refills the
 * unit contexts of a block many times and the block drains its tail as a large batch does; the
 * workspace and the arena are sized from the blocks launched, as ever. */
int skm_mapper_map_relaunches(skm_mapper *mapper, int64_t *count);
/* Access counters of the instrumented build of the map kernel (they define the
 * algorithmic bytes): enable, map, then read.  out[0]=reads
 * [1]=read bases [2]=lookups [3]=slots probed [4]=ContigEntry reads [5]=target
 * entries copied [6]=target entries merged [7]=8-base fetches [8]=merges
 * [9]=tuple ids; out[16..30] = scheduler census of the map kernel: rounds, then
 * (chunk executions, lanes) of start, lookup, merge, left, right, emit, scan;
 * out[32..46] = wave-cycle sums: schedule, (unused), then per action, then six
 * phases of the emission.  enable = 2 selects the census build instead: the production code
 * paths with the census and cycle sums (a profiling aid; its access counters undercount). */
int skm_mapper_set_stats(skm_mapper *mapper, int enable);
int skm_mapper_access_stats(skm_mapper *mapper, int64_t out[48]);

/* ------------------------------------------------------------- sample sets
 * map_multiple_samples (seekmer/mapper.py:196-234) for MANY SMALL samples -- the cells of `impute`:
 * one handle maps the units of all its samples in shared launches into one class table in which a
 * class is the pair (sample, target tuple), and hands back one class table per sample.
 *
 * Contract: every per-sample table -- classes in first-seen order, class_offsets, class_targets,
 * counts, first-seen unit numbers counted inside the sample, the unaligned and total unit counts --
 * is bit for bit what a skm_mapper of its own gives for that sample's reads, however the samples'
 * segments are interleaved, cut into launches, or spread over adding threads.  Two samples that
 * hold the same tuple keep separate classes: a record's 64-bit class key is that of (sample, tuple),
 * and two different tuples that meet in one slot fail the call with SKM_ERR_COLLISION as they do in a
 * mapper; counts are exact or the call fails.
 * The FRAGMENT-LENGTH HISTOGRAM of the set is the sum over all its samples, which is what
 * impute.pool_fragment_lengths gives every cell before anything reads it
 * (seekmer/impute.py:128-146).  A set asked to (skm_sample_set_keep_histograms, before the first
 * unit) also keeps one histogram per sample, each that of a mapper fed the sample's reads alone.
 * The strand mode (skm_mapper_set_strand) applies to the whole set.  Read names (-m) are not kept.
 *
 * Samples are numbered 0, 1, ... by the caller (below 2^24); the set holds the samples 0 .. the
 * largest number an add call has named.  A sample's reads arrive as one or more SEGMENTS, runs of
 * consecutive units, each beginning at the unit (`first_unit`) where the sample's units added so
 * far end: SKM_ERR_STATE otherwise.  Segments of different samples may be added in any order and
 * from any threads; the calling thread copies the segment to HBM (the call returns when the arrays
 * are free again) and one worker maps what is queued, at most 2^21 units a launch
 * (SKM_SAMPLE_SET_MAX_UNITS in the environment at create: fewer, for tests), a short queue waiting
 * for 2^15 units or for a call that reads the tables.  A segment of no units just makes the sample
 * exist.  After a failed launch the set stays failed: every later call returns that error.
 * A call that reads the tables (_summary with room for samples, _export) waits until every segment
 * added before it has been mapped and keeps adders waiting while it reads, so what it returns is
 * whole: the tables of exactly the segments added so far.  It may run while other threads add. */
typedef struct skm_sample_set skm_sample_set;
int skm_sample_set_create(skm_index *index, int paired, skm_sample_set **out);
int skm_sample_set_destroy(skm_sample_set *set);
/* only while the set holds no units (SKM_ERR_STATE otherwise) */
int skm_sample_set_set_strand(skm_sample_set *set, int mode);
/* skm_mapper_set_length_weights for the set: skm_sample_set_quantify then computes ONE row of
 * effective lengths from p and gives it to every sample, whether or not the set keeps a histogram
 * per sample, and its effective_lengths output carries those lengths.  NULL: back to the histograms. */
int skm_sample_set_set_length_weights(skm_sample_set *set, const double *p);
/* Units [first_unit, first_unit + n) of `sample` as packed reads (skm_packed_reads): unit
 * first_unit + r = read r of mate1 (+ read r of mate2 in a paired set; NULL in a single-ended one).
 * n = mate1->n_reads = mate2->n_reads; the pieces' `stream` and `first_read` are not looked at. */
int skm_sample_set_add_packed(skm_sample_set *set, int64_t sample, int64_t first_unit,
                              const skm_packed_reads *mate1, const skm_packed_reads *mate2);
/* The same for reads as text: the layout of skm_mapper_map_batch (paired: reads 2u, 2u + 1 are the
 * mates of unit first_unit + u). */
int skm_sample_set_add_batch(skm_sample_set *set, int64_t sample, int64_t first_unit,
                             const char *bases, const int64_t *offsets, int64_t n_units);
/* waits for everything added to be mapped; the set's failure, if there is one */
int skm_sample_set_sync(skm_sample_set *set);
/* skm_mapper_map_relaunches of the set's launches (waits for everything added to be mapped) */
int skm_sample_set_map_relaunches(skm_sample_set *set, int64_t *count);
/* *n_samples = samples of the set; summary[4 i .. 4 i + 3] for the samples i < min(cap_samples,
 * *n_samples) = skm_mapper_summary of sample i: C classes, M (class, target) rows, unaligned (the
 * sample's units minus the sum of its class counts), total units.  With cap_samples = 0 (summary
 * may be NULL) the call only counts the samples named so far and waits for nothing. */
int skm_sample_set_summary(skm_sample_set *set, int64_t cap_samples, int64_t *n_samples,
                           int64_t *summary);
/* All samples' tables one after the other: sample i owns the classes sample_class_offsets[i] ..
 * sample_class_offsets[i + 1] (array of n_samples + 1) of class_offsets[C + 1] (one CSR over all C
 * classes of the set), class_targets[M], class_counts[C], first_seen[C] -- the arrays of
 * skm_mapper_export with first_seen counted inside the sample.  Any pointer may be NULL. */
int skm_sample_set_export(skm_sample_set *set, int64_t *sample_class_offsets,
                          int64_t *class_offsets, int32_t *class_targets, int64_t *class_counts,
                          int64_t *first_seen);
/* fld[2000]: the set's pooled histogram, summed over its samples (with or without histograms
 * per sample) */
int skm_sample_set_histogram(skm_sample_set *set, int64_t *fld);
/* enable != 0: the set also keeps one fragment-length histogram per sample, in HBM.  Its mapper then
 * stores every unit's span (skm_mapper_keep_spans: 16 bytes a unit) and a kernel after each launch
 * counts the spans' lengths by the unit's sample (sample_fld_kernel, skm_samples.hip).  Only while
 * the set holds no units (SKM_ERR_STATE otherwise).  The histograms are rows of 16 KB indexed by the
 * sample NUMBER, so such a set numbers its samples below 2^16 (1 GiB of rows): an add call that
 * names a larger one fails with SKM_ERR_ARG. */
int skm_sample_set_keep_histograms(skm_sample_set *set, int enable);
/* fld[n_samples][2000], in sample order: row i is the histogram of a mapper fed sample i alone (all
 * zero for a sample without units); the rows add up to skm_sample_set_histogram.  Waits for
 * everything added to be mapped and keeps adders waiting while it reads, as _summary and _export.
 * SKM_ERR_STATE if the set does not keep them, SKM_ERR_ARG if cap_samples (rows of room in fld) is
 * below the samples named so far. */
int skm_sample_set_histograms(skm_sample_set *set, int64_t cap_samples, int64_t *fld);
/* Sequence bias (--bias) in a set.  enable != 0: the set also counts, per sample, the hexamer each aligned
 * unit starts with -- the rule of skm_mapper_set_bias, word for word -- in a kernel of its own
 * (sample_bias_kernel, skm_samples.hip) between the strand filter and class counting of every launch; a set
 * that was not asked launches what it always has.  Only while the set holds no units (SKM_ERR_STATE
 * otherwise).  The counts are rows of 4096 64-bit words in HBM (32 KB) indexed by the sample NUMBER, so such
 * a set numbers its samples below 2^15 (1 GiB of rows): an add call that names a larger one fails with
 * SKM_ERR_ARG.  Inside the kernel a block counts in 32-bit LDS bins that hold at most the 4096 records it
 * owns.
 * skm_sample_set_bias_observed: out[n_samples][4096], in sample order: row i is skm_mapper_bias_observed of a
 * mapper fed sample i alone (all zero for a sample without units), whatever the interleaving, the cut into
 * launches or the adding threads.  Waits for everything added to be mapped and keeps adders waiting while it
 * reads, as skm_sample_set_histograms.  SKM_ERR_STATE if the set does not count, SKM_ERR_ARG if cap_samples
 * (rows of room in out) is below the samples named so far. */
int skm_sample_set_keep_bias(skm_sample_set *set, int enable);
int skm_sample_set_bias_observed(skm_sample_set *set, int64_t cap_samples, int64_t *out);
/* UMI collapse ("UMI collapse").  umi_bases = 1 .. 16: every unit of the set comes with a UMI of
 * that many bases (2 bits a base, below 4^umi_bases), and inside a sample a unit is a DUPLICATE when an earlier unit
 * of the sample (a lower unit number) has the same UMI and the same class -- the same target tuple after the strand
 * filter.  The first unit of every (sample, UMI, class) stays; every later one is removed as if it had never been
 * added: it counts in no total, no class, no histogram per sample, no hexamer row, no first-seen unit.  A unit
 * without a class (unaligned) is never removed.  The molecules live in an exact set in HBM (32-byte slots, at most
 * half full: 64 bytes a molecule; sized ahead of every launch and grown by rehashing; an allocation that fails says
 * so) that two kernels of every launch consult between the strand filter and everything that counts
 * (skm_umi.hip); two molecules that share a 64-bit tag fail the call with SKM_ERR_COLLISION.  A set that was not
 * asked launches what it always has.  Only before the set's first segment, and only in a set that keeps a
 * histogram per sample (skm_sample_set_keep_histograms first; the POOLED histogram of skm_sample_set_histogram is
 * counted inside the map kernel and still holds the removed units): SKM_ERR_STATE otherwise.  0 switches it off.
 * SKM_TEST_UMI_SLOTS (a power of two >= 2, read by skm_sample_set_create) starts the molecule set at that many
 * slots and grows it only when a launch finds it full, for tests.
 * skm_sample_set_add_packed_umis: skm_sample_set_add_packed with umis[n], the UMI of every unit (SKM_ERR_ARG for
 * one that does not fit umi_bases); they are copied with the reads.  In a set that keeps UMIs it is the only way to
 * add (_add_packed and _add_batch return SKM_ERR_ARG), in any other set it returns SKM_ERR_ARG.
 * skm_sample_set_umi_removed: removed[n_samples], the units removed so far per sample (zeros in a set that keeps no
 * UMIs); every unit total the set reports (_summary, _export, the samples' unaligned counts) is the units added less
 * these.  Waits and holds adders as _summary; SKM_ERR_ARG if cap_samples is below the samples named so far.
 * skm_sample_set_set_umi_mismatches ("UMI mismatches"): mismatches = 1 also takes a UMI one
 * substitution away for a sequencing error.  Inside a sample a unit with a class is then removed when an EARLIER unit
 * of the sample (a lower unit number) has the same class and a UMI at Hamming distance 0 or 1 over the umi_bases
 * bases -- whether or not that earlier unit was itself removed; everything else is as above (unaligned units are never
 * removed, the class is the tuple after the strand filter, two samples or two classes are separate molecules).  The
 * rule is arrival-ordered and exact: a chain m0 - m1 - m2 with d(m0, m2) = 2 leaves one unit in the order m0, m1, m2
 * and two (m0, m2) in the order m0, m2, m1; it is neither a count-based nor a "directional" rule.  The result does
 * not depend on the grid, the cut into launches or the order in which samples are added.  0 (the default) is the
 * exact rule above and launches what it always has.  SKM_ERR_ARG for any other value; SKM_ERR_STATE in a set that
 * keeps no UMIs (skm_sample_set_keep_umis first) and after the set's first segment.
 * skm_sample_set_umi_near_removed: *n = the units removed so far ONLY because of such a neighbour (each the first
 * unit of its own exact molecule), over all samples; they are part of _umi_removed's counts.  0 in any other set.
 * Waits for the set's launches. */
int skm_sample_set_keep_umis(skm_sample_set *set, int umi_bases);
int skm_sample_set_set_umi_mismatches(skm_sample_set *set, int mismatches);
int skm_sample_set_umi_near_removed(skm_sample_set *set, int64_t *n);
int skm_sample_set_add_packed_umis(skm_sample_set *set, int64_t sample, int64_t first_unit, const skm_packed_reads *mate1,
                                   const skm_packed_reads *mate2, const uint32_t *umis);
int skm_sample_set_umi_removed(skm_sample_set *set, int64_t cap_samples, int64_t *removed);
/* DIAGNOSTICS, with no promise of stability: the set's bookkeeping on the host alone (no GPU is
 * touched), for tests.  They run the cutting, the log and the ordering by (sample, local first
 * seen) that the set itself runs; _split bisects the log on the host where the set does it in a
 * kernel (sample_assign_kernel).  Not part of the interface a caller should build on.  _plan: segments
 * (sample[i], n_units[i]) queued in this order before the first launch, cut into launches of at most
 * max_units units as the worker cuts them -> the log the export reads: entry e says that the set's
 * units from entry_global[e] (ascending, from 0) up to the next entry's are the units from
 * entry_local[e] on of sample entry_sample[e].  *n_entries = entries; the arrays are filled when
 * cap_entries holds them.  _split: such a log against the global first-seen units of C classes ->
 * class_sample[C], class_local[C] (first seen, counted inside the sample), order[C] (the classes by
 * sample, then by class_local: the export's order) and sample_class_offsets[n_samples + 1]. */
int skm_sample_set_plan(int64_t n_segments, const int32_t *sample, const int64_t *n_units,
                        int64_t max_units, int64_t cap_entries, int64_t *n_entries,
                        int64_t *entry_global, int64_t *entry_local, int32_t *entry_sample);
int skm_sample_set_split(int64_t n_entries, const int64_t *entry_global, const int64_t *entry_local,
                         const int32_t *entry_sample, int64_t n_samples, int64_t n_classes,
                         const int64_t *first_seen, int32_t *class_sample, int64_t *class_local,
                         int64_t *order, int64_t *sample_class_offsets);

/* ------------------------------------------------------------ gene-level tables
 * ("Gene-level tables".)  tx_gene[n_tx] gives every transcript's gene number,
 * 0 .. n_genes - 1, or -1 for a transcript without a gene; every call checks it on the host first
 * (SKM_ERR_ARG for a value outside that range) and no kernel indexes by an unchecked value.
 * skm_gene_sums: out[r][g] = the sum of values[r][t] over the transcripts t of gene g, added in
 * ascending t, one after the other, from +0.0 -- numpy.add.at(out[r], tx_gene[named], values[r][named])
 * bit for bit, whatever the grid.  Rows are staged in groups of at most 256 MB (SKM_GENE_GROUP, for
 * tests: fewer rows per group). */
int skm_gene_sums(int device, int64_t n_rows, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                  const double *values /*[n_rows][n_tx]*/, double *out /*[n_rows][n_genes]*/);
/* Units that belong to exactly one gene (the rule of the reference's _calculate_uniquely_mapped_counts,
 * seekmer/impute.py:149-183): a class whose transcripts all have tx_gene == g >= 0 adds its count to
 * unique[sample][g]; one whose transcripts all have tx_gene == -1 adds to other[sample][1] (unnamed);
 * every other class adds to other[sample][0] (ambiguous between genes).  Exact 64-bit integer sums.
 * Any class table given as the CSR of skm_mapper_export; class_sample NULL = one sample.  A sample
 * without classes gets zeros; so does every sample of an empty table.  SKM_ERR_ARG for a target not
 * below n_tx, a sample not below n_samples, a negative count, offsets that do not ascend. */
int skm_gene_unique_counts(int device, int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets,
                           const int64_t *class_counts, const int32_t *class_sample, int64_t n_samples,
                           int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                           int64_t *unique /*[n_samples][n_genes]*/, int64_t *other /*[n_samples][2]*/);
/* The same on the table where it lies in HBM: nothing but tx_gene goes up, nothing but the result
 * comes down.  SKM_ERR_ARG when a class names a transcript not below n_tx. */
int skm_mapper_gene_counts(skm_mapper *mapper, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                           int64_t *unique /*[n_genes]*/, int64_t other[2]);
/* Row i is skm_mapper_gene_counts of a mapper fed sample i alone (zeros for a sample without units).
 * Waits for everything added to be mapped and keeps adders waiting while it reads, as _export; the
 * classes' samples are the device arrays the set's view already holds.  SKM_ERR_ARG if cap_samples
 * (rows of room in unique and other) is below the samples named so far.  Device rows are made for
 * ranges of samples, 1 GiB of them at most (SKM_GENE_GROUP, for tests: fewer samples per range). */
int skm_sample_set_gene_counts(skm_sample_set *set, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                               int64_t cap_samples, int64_t *unique /*[n_samples][n_genes]*/, int64_t *other);
/* The count matrix ("Count matrix"): the same counts, by the same rule, as a CSR over
 * samples that is made and kept in HBM -- indptr int64[n_samples + 1]; indices int32[nnz], the gene numbers,
 * strictly ascending inside a sample; data int64[nnz], every one > 0 (a class inside one gene with a count
 * of 0 makes no entry); other int64[n_samples][2] as above.  Densified, row i is row i of
 * skm_sample_set_gene_counts / skm_gene_unique_counts, whatever the grid: the sums are 64-bit integers.
 * No dense row exists anywhere: the cost is that of sorting the classes by (sample, gene).
 * SKM_ERR_ARG for a table of 2^32 classes or more and for more than 2^31 - 2 samples; on any failure *out is NULL.
 * skm_sample_set_gene_matrix works from the set's resident table and waits and locks as skm_sample_set_gene_counts
 * does; skm_gene_matrix_from_classes takes the table of skm_gene_unique_counts, with that call's checks.
 * _shape: any pointer may be NULL.  _read copies the arrays home; any pointer may be NULL to skip that array.
 * The handle owns its device buffers until _destroy (NULL is allowed there). */
typedef struct skm_gene_matrix skm_gene_matrix;
int skm_sample_set_gene_matrix(skm_sample_set *set, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                               skm_gene_matrix **out);
int skm_gene_matrix_from_classes(int device, int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets,
                                 const int64_t *class_counts, const int32_t *class_sample, int64_t n_samples,
                                 int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, skm_gene_matrix **out);
int skm_gene_matrix_shape(const skm_gene_matrix *matrix, int64_t *n_samples, int64_t *n_genes, int64_t *nnz);
int skm_gene_matrix_read(const skm_gene_matrix *matrix, int64_t *indptr /*[n_samples + 1]*/, int32_t *indices /*[nnz]*/,
                         int64_t *data /*[nnz]*/, int64_t *other /*[n_samples][2]*/);
int skm_gene_matrix_destroy(skm_gene_matrix *matrix);
/* The molecule matrix ("Molecule matrix"): entry (sample, gene) = the number of DISTINCT UMIs
 * among the sample's surviving units whose class lies inside that gene (the rule above), UMIs compared letter for
 * letter -- where the count matrix adds up class counts and so counts a molecule once per class its reads fell into.
 * The same handle: indptr, indices and other are those of skm_sample_set_gene_matrix of the same set, every data
 * entry is >= 1 and <= the count matrix's.  A UMI seen in a class inside the gene and in an ambiguous class counts
 * once, for the first; ambiguous classes that share a UMI are not intersected.  Parity with other tools' UMI rules
 * is not claimed.
 * skm_sample_set_molecule_matrix is a pass over what the set holds in HBM after its launches -- the molecule set of
 * UMI collapse and the class table -- and waits and locks as skm_sample_set_gene_matrix does.  SKM_ERR_STATE for a
 * set that keeps no UMIs (skm_sample_set_keep_umis); SKM_ERR_ARG for 2^32 molecules or more and for the limits of the
 * count matrix: refused before anything is allocated.  Device memory while it runs: 8 bytes per slot of the class
 * table, 8 per slot of the molecule set, 48 per surviving molecule.
 * skm_gene_matrix_from_molecules makes the matrix of n host triples (sample, gene, UMI), other all zero: the
 * sort, head and fill steps alone.  SKM_ERR_ARG for a sample outside [0, n_samples) or a gene outside [0, n_genes).
 * On any failure *out is NULL. */
int skm_sample_set_molecule_matrix(skm_sample_set *set, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                   skm_gene_matrix **out);
int skm_gene_matrix_from_molecules(int device, int64_t n, const int32_t *sample, const int32_t *gene, const uint32_t *umi,
                                   int64_t n_samples, int64_t n_genes, skm_gene_matrix **out);
/* Resolved molecules ("Resolved molecules"): one gene per (sample, UMI).  The distinct classes
 * among a sample's live molecules -- the population of skm_sample_set_molecule_matrix -- with one UMI form a group;
 * G_k = { tx_gene[t] : t in class k }, -1 an element like any other, and I = the intersection of G_k over the group:
 *   I = {g}, g >= 0   resolved: entry (sample, g) += 1; also rescued when no class of the group lies inside one gene
 *   I = {-1}          unnamed           |
 *   I of two or more  multi-gene        | tallied only
 *   I empty           collision         |
 * UMIs are compared letter for letter; the same UMI in two samples forms two groups.  Parity with other tools' UMI
 * rules is not claimed.  The handle is an ordinary skm_gene_matrix (its pattern is NOT the count matrix's: a rescued
 * group can make an entry that matrix lacks, a collision can take one away); other[s] = { multi-gene + collision,
 * unnamed } in molecules.  skm_gene_matrix_read_tally gives tally[s] = { resolved, rescued, multi-gene, unnamed,
 * collision } (rescued is a part of resolved; the other four add up to the sample's distinct UMIs), and
 * SKM_ERR_STATE on a handle that any other call made.
 * skm_sample_set_resolved_matrix waits and locks as skm_sample_set_molecule_matrix does and has its refusals and
 * limits (checked before anything is allocated).  Device memory while it runs: 8 bytes per slot of the class table, 8
 * per slot of the molecule set, 40 per live molecule, 48 per group.
 * skm_gene_matrix_from_molecule_classes runs the sort, group, resolve and fill steps on host arrays: classes as the
 * CSR of skm_mapper_export with a sample each (class_sample NULL: sample 0, n_samples 1), molecules as (class, UMI);
 * two molecules with the same class and UMI count as one.  SKM_ERR_ARG for a mol_class outside [0, n_classes), a
 * class sample outside [0, n_samples), an id not below n_tx and an empty class.  On any failure *out is NULL. */
int skm_sample_set_resolved_matrix(skm_sample_set *set, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                   skm_gene_matrix **out);
int skm_gene_matrix_from_molecule_classes(int device, int64_t n_classes, const int64_t *class_offsets,
                                          const int32_t *class_targets, const int32_t *class_sample, int64_t n_molecules,
                                          const int32_t *mol_class, const uint32_t *mol_umi, int64_t n_samples, int64_t n_tx,
                                          int64_t n_genes, const int32_t *tx_gene, skm_gene_matrix **out);
int skm_gene_matrix_read_tally(const skm_gene_matrix *matrix, int64_t *tally /*[n_samples][5]*/);
/* Distributed molecules ("Distributed molecules"): the groups and the intersection I of "Resolved
 * molecules", with the multi-gene groups shared out among their genes by a small EM per sample.  -1 ("no gene") is the
 * element n_genes, the sink.  A group's list is the elements of I, ascending:
 *   one element g < n_genes   resolved      | the group adds 1 to that row of its sample
 *   the sink alone            unnamed       |
 *   2 to 16 elements          distributed: a set of the sample's EM
 *   more than 16              wide          | tallied only
 *   none                      collision     |
 * A sample's rows are the distinct elements of its lists, u[r] the lists of one element that name row r.  From
 * x[r] = u[r] + the sum of 1 / len(S) over the sets S that hold r, a step is d[j] = the sum of x over set j and
 * x'[r] = u[r] + the sum of x[r] / d[j] over the sets that hold r; the sample is done when no row with x' > 0.001 has
 * changed by more than 1 % of x', or after 1000 steps (capped).  All sums are IEEE doubles in one fixed order
 * (DESIGN.md states it), so the result is the plain-Python reference's bit for bit.  Entry (sample, g) = x[r] for
 * every row with g < n_genes and x[r] >= 0.001; nothing is renormalised; the sink row's x is the sample's to_unnamed.
 * Parity with alevin or bustools is not claimed.
 * The handle is a skm_gene_matrix whose data are doubles: skm_gene_matrix_read_weights reads them, and
 * skm_gene_matrix_read with a non-NULL data is SKM_ERR_STATE on it (indptr, indices and other = { wide + collision,
 * unnamed } are read as ever).  skm_gene_matrix_read_em gives tally[s] = { resolved, distributed, wide, unnamed,
 * collision, rows, steps, capped } -- the first five add up to the sample's distinct UMIs -- and to_unnamed[s].
 * Both are SKM_ERR_STATE on a handle that any other call made, as skm_gene_matrix_read_tally is on this one.
 * skm_sample_set_distributed_matrix waits and locks as skm_sample_set_resolved_matrix does and has its refusals and
 * limits (checked before anything is allocated); 2^31 - 1 list elements at most.  Device memory while it runs: that
 * call's per slot and per molecule, then 96 bytes per group, 52 per list element, 36 per row, 16 per set and 32 per sample.
 * skm_gene_matrix_from_molecule_sets is skm_gene_matrix_from_molecule_classes with these steps and max_steps >= 1 in
 * the place of 1000.  skm_gene_em_cells runs the EM alone on host arrays: cell c has the rows cell_row_start[c] ..
 * cell_row_start[c + 1] - 1 with u[] >= 0 and the sets cell_set_start[c] .. cell_set_start[c + 1] - 1, set j the
 * cell-local rows set_rows[set_start[j] .. set_start[j + 1]); x_out[n_rows], steps_out[n_cells], capped_out[n_cells].
 * SKM_ERR_ARG for a row outside its cell, a set of fewer than 2 or more than 16 rows, rows that do not ascend inside
 * a set, offsets that do not begin at 0 or descend, a negative u and max_steps < 1.  On any failure *out is NULL. */
int skm_sample_set_distributed_matrix(skm_sample_set *set, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                      skm_gene_matrix **out);
int skm_gene_matrix_from_molecule_sets(int device, int64_t n_classes, const int64_t *class_offsets,
                                       const int32_t *class_targets, const int32_t *class_sample, int64_t n_molecules,
                                       const int32_t *mol_class, const uint32_t *mol_umi, int64_t n_samples, int64_t n_tx,
                                       int64_t n_genes, const int32_t *tx_gene, int64_t max_steps, skm_gene_matrix **out);
int skm_gene_em_cells(int device, int64_t n_cells, const int64_t *cell_row_start, const int64_t *u,
                      const int64_t *cell_set_start, const int64_t *set_start, const int32_t *set_rows, int64_t max_steps,
                      double *x_out, int64_t *steps_out, int64_t *capped_out);
int skm_gene_matrix_read_weights(const skm_gene_matrix *matrix, double *data /*[nnz]*/);
int skm_gene_matrix_read_em(const skm_gene_matrix *matrix, int64_t *tally /*[n_samples][8]*/, double *to_unnamed /*[n_samples]*/);

/* ---------------------------------------------------------------- cell barcodes
 * ("Cell barcodes".)  A pooled run -- one barcode read per unit beside the cDNA reads --
 * is split into its cells on the GPU: skm_barcodes_assign says which whitelist entry every unit's barcode is,
 * skm_units_group orders a run of units by cell, and skm_packed_gather (libseekmer_host.so, below) moves the reads
 * into that order; the cells then enter a sample set as ordinary in-order segments.
 *
 * The whitelist: n barcodes of `length` characters back to back (n x length, no separators), 1 <= length <= 32,
 * upper-case ACGT only, no barcode twice: SKM_ERR_ARG otherwise (the message names the entry).  The handle owns an
 * open-addressing table in HBM (key = the 2 x length code bits, A0 C1 G2 T3, first base in the top bits; a power
 * of two slots, at most half full), built on the host and uploaded once; cell i = barcode i.  A whitelist of up to
 * 1024 entries is probed from a copy in LDS. */
typedef struct skm_barcodes skm_barcodes;
int skm_barcodes_create(int device, const char *barcodes /* n x length characters */, int64_t n, int length,
                        skm_barcodes **out);
int skm_barcodes_destroy(skm_barcodes *barcodes);
/* The cell of every read of a piece of barcode reads (a host piece, as for skm_sample_set_add_packed; `stream` and
 * `first_read` are not looked at).  The barcode of read r is its bases [start, start + length); in this order:
 * the read is shorter than start + length: short; two or more of the window's positions are not upper-case ACGT:
 * unreadable; all clean and equal to an entry: exact (even with another entry at distance 1); max_mismatches == 0:
 * no match; otherwise the candidates are the entries that differ from the window in exactly one position, a
 * non-clean position always counting as differing (so with one such position only the four bases there are tried):
 * one candidate: corrected; none: no match; several: ambiguous.  cell[r] = the entry of an exact or corrected read,
 * -1 for every other; cell_units[n] += the reads given to each entry; stats[5] += exact, corrected, ambiguous,
 * no match, short + unreadable (they add up to n_reads).  max_mismatches is 0 or 1; calls on one handle run one
 * after the other.  The window may lie anywhere in the read and straddle a code word. */
int skm_barcodes_assign(skm_barcodes *barcodes, const skm_packed_reads *reads, int start, int max_mismatches,
                        int32_t *cell /* [n_reads] */, int64_t *cell_units /* [n], added to */,
                        int64_t stats[5] /* added to */);
/* The UMI of every read of a piece of barcode reads (a host piece, as for skm_barcodes_assign): bases
 * [start, start + length), 1 <= length <= 16, as 2 bits a base (A0 C1 G2 T3), the first base in the top bits of the
 * 2 x length used bits of umi[r].  A read that is shorter than start + length, or that holds a position in the
 * window that is not an upper-case ACGT, has no UMI: umi[r] = 0, cell[r] = -1 (cell -- in/out, the cells of
 * skm_barcodes_assign -- may be NULL) and *n_unreadable += 1.  The window may lie anywhere in the read, before or
 * after the barcode, and straddle a code word; only the window's words are uploaded. */
int skm_umi_windows(int device, const skm_packed_reads *reads, int start, int length, int32_t *cell /* in/out, may be NULL */,
                    uint32_t *umi /* [n_reads] */, int64_t *n_unreadable /* added to */);
/* A run of n < 2^31 units by sample: sample[u] in [0, n_samples) or negative (dropped), n_samples <= 2^24 ->
 * order[] = the kept units grouped by ascending sample and in their original order inside a sample (room for n;
 * offsets[n_samples] are written), offsets[n_samples + 1]: sample s owns order[offsets[s] .. offsets[s + 1]).
 * numpy.argsort(kind='stable') of the samples with the dropped units cut off: the stable radix sort of the class
 * views (skm_quant_setup.hip), dropped units under key n_samples.  SKM_ERR_ARG for a sample >= n_samples. */
int skm_units_group(int device, const int32_t *sample, int64_t n, int64_t n_samples, int32_t *order,
                    int64_t *offsets /* [n_samples + 1] */);

/* ---------------------------------------------------------------- cell discovery
 * ("Cell discovery".)  A whitelist made from the barcode reads themselves: an exact count of
 * every distinct barcode, and from it the barcodes that are cells.  The handle owns the census table in HBM (open
 * addressing, 16 bytes a slot: key and count; a power of two slots, sized ahead of every add to at most half full;
 * an empty slot holds the key of the all-T 32-mer, which is counted in a counter of its own).  `length` is 1 .. 32:
 * SKM_ERR_ARG otherwise.  SKM_TEST_CENSUS_SLOTS=N (a power of two >= 2, read by _create) starts the table at N slots;
 * it then grows only when a launch finds it full.  A handle that found no memory for its table stays failed
 * (SKM_ERR_STATE from then on).  Calls on one handle run one after the other. */
typedef struct skm_barcode_census skm_barcode_census;
int skm_barcode_census_create(int device, int length, skm_barcode_census **out);
int skm_barcode_census_destroy(skm_barcode_census *census);
/* A piece of barcode reads (a host piece, as for skm_barcodes_assign).  The window of read r is its bases
 * [start, start + length): a read shorter than that is short; a window with any position that is not an upper-case
 * ACGT is unreadable (no tolerance, unlike skm_barcodes_assign); every other window is counted under its 2 x length
 * code bits (A0 C1 G2 T3, first base in the top bits).  stats[3] += counted, short, unreadable (they add up to
 * n_reads).  SKM_ERR_ARG for a negative start. */
int skm_barcode_census_add(skm_barcode_census *census, const skm_packed_reads *reads, int start,
                           int64_t stats[3] /* counted, short, unreadable; added to */);
int skm_barcode_census_size(skm_barcode_census *census, int64_t *n_distinct, int64_t *n_counted);
/* The census in ranked order -- count descending, then key ascending -- ranked on the device: the first
 * min(cap, n_distinct) entries. */
int skm_barcode_census_ranked(skm_barcode_census *census, int64_t cap, uint64_t *keys, int64_t *counts);
/* The cells.  rank = min((expect_cells + 99) / 100, n_distinct), m = the count at that rank (from 1),
 * threshold = max((m + 9) / 10, 1); the candidates are the entries with count >= threshold; with drop_neighbours a
 * candidate is dropped when a candidate earlier in ranked order differs from it in exactly one position (whether or
 * not that one is dropped itself); the picked barcodes are the candidates not dropped, in ranked order.
 * info[6] = rank, m, threshold, candidates, dropped, picked.  SKM_ERR_ARG for expect_cells < 1; SKM_ERR_STATE for a
 * census without a counted barcode, and when picked > cap (info is filled, nothing is copied, the handle stays
 * usable). */
int skm_barcode_census_pick(skm_barcode_census *census, int64_t expect_cells, int drop_neighbours, int64_t cap,
                            uint64_t *keys, int64_t *counts, int64_t info[6]);

/* ------------------------------------------------------------ quantification
 * MapResult.effective_lengths (seekmer/mapper.py:134-141). */
int skm_effective_lengths(int device, const int64_t *fld, const double *lengths,
                          int64_t n_tx, double *out);
/* The same for n histograms in one call: fld[n][2000] -> out[n][n_tx], row s bit for bit what
 * skm_effective_lengths gives for fld[s] (NaN for an empty histogram).  The lengths are uploaded
 * once; the histograms pass through the device in groups whose rows, of `fld` and of `out`, stay
 * within 256 MB each (SKM_EFF_MANY_GROUP in the environment: rows per group at most, for tests). */
int skm_effective_lengths_many(int device, int64_t n, const int64_t *fld, const double *lengths,
                               int64_t n_tx, double *out);
/* The same rule with p given instead of counted: n rows of weights p[n][2000] -> out[n][n_tx],
 * out[s][t] = sum_i max(lengths[t] - i, 1) * p[s][i] accumulated for i = 0..1999 in order, multiply
 * and add separate -- bit for bit the numpy loop over the same p.  Grouped as the call above
 * (SKM_EFF_MANY_GROUP).  SKM_ERR_ARG, before any device work, for a negative or non-finite weight,
 * a NULL array or a negative size; n == 0 or n_tx == 0 does nothing. */
int skm_effective_lengths_weights(int device, int64_t n, const double *p, const double *lengths,
                                  int64_t n_tx, double *out);

/* The sequence-bias correction of the effective lengths ("Sequence bias"), on the
 * pool of skm_index_build_transcripts.  strand: SKM_STRAND_*, observed[4096] (skm_mapper_bias_observed),
 * tpm[n_tx] the first pass's abundances, eff[n_tx] its effective lengths.  The windows of transcript t are
 * the positions p <= len_t - 6 with six known bases, h+ their hexamer and h- its reverse complement, the
 * shares (s+, s-) = (1/2, 1/2), (1, 0) for FR, (0, 1) for RF:
 *   E[h] = sum_t tpm_t sum_p (s+ [h+ = h] + s- [h- = h])
 *   b[h] = ((O[h] + 1) / (sum O + 4096)) / (E[h] / sum E) where E[h] > 0, 1 elsewhere; all 1 when sum O = 0
 *          or sum E = 0
 *   eff_out[t] = eff[t] * (1 / n_t) sum_p (s+ b[h+] + s- b[h-]), eff[t] for a transcript without windows
 * expected_out[4096] and b_out[4096] are optional.  E is accumulated in 96-bit fixed point (tpm_t scaled
 * by 2^94 / sum_t tpm_t n_t and rounded, three 32-bit limbs summed apart) with integer atomics and every
 * transcript's sum over its windows runs in a fixed order, so all three outputs are the same bits on every run and for every grid size
 * (SKM_BIAS_BLOCKS in the environment caps the grids: tests).  SKM_ERR_ARG, before any device work, for NULL
 * arrays, a negative size, a non-finite or negative tpm, a negative count or an unknown strand mode;
 * SKM_ERR_STATE when the pool has not been built; SKM_ERR_ARG when n_tx is not the pool's.
 * This call and skm_index_build_transcripts run once per sample and once per index: they allocate their
 * scratch with hipMalloc and work on the default stream with blocking copies, which also wait for work
 * queued on this process's other blocking streams; they are not meant for a loop. */
int skm_bias_correct(skm_index *index, int strand, const int64_t *observed, const double *tpm, const double *eff,
                     int64_t n_tx, double *expected_out, double *b_out, double *eff_out);
/* skm_bias_correct for n samples in one call (the samples of a sample set): observed[n][4096], tpm[n][n_tx],
 * eff[n][n_tx] -> expected_out[n][4096], b_out[n][4096] (both optional), eff_out[n][n_tx].  Row s is bit for bit
 * what skm_bias_correct returns for sample s alone: E is summed in the same fixed point with integer atomics, b
 * comes from integers, and a transcript's sum over its windows keeps the order that depends on the transcript
 * alone.  The sample is a grid dimension of the kernels; the lengths kernel holds the b tables of several
 * samples in LDS and decodes every transcript once for all of them (skm_bias.hip).  Scratch is allocated once,
 * for a group of consecutive rows whose buffers -- 5 words per transcript and 6 per hexamer a row -- stay
 * within 256 MB (and 32768 rows); SKM_BIAS_MANY_GROUP in the environment caps the rows per group (tests), and
 * SKM_BIAS_BLOCKS keeps its meaning.  The argument checks of skm_bias_correct apply to every row before any
 * device work (SKM_ERR_ARG); SKM_ERR_STATE when the pool has not been built; n == 0 does nothing. */
int skm_bias_correct_many(skm_index *index, int strand, int64_t n, const int64_t *observed, const double *tpm,
                          const double *eff, int64_t n_tx, double *expected_out, double *b_out, double *eff_out);
/* The host's half of E (libseekmer_host.so; no GPU): total_out = sum_t tpm[t] * windows[t] added in transcript
 * order, and W_t = round(tpm[t] * 2^94 / total), clamped below 2^95, as three 32-bit limbs lowest first:
 * limbs_out[k * n_tx + t].  A transcript without windows gets limbs 0; so does every transcript when the total
 * is 0.  SKM_ERR_ARG for a NULL array, a negative size or window count, a negative or non-finite abundance, and
 * for a total that cannot be scaled (it, or 2^94 over it, is not finite).  skm_bias_correct and
 * skm_bias_correct_many call the same function (skm_bias_weights.h). */
int skm_bias_fixed_weights(const double *tpm, const int32_t *windows, int64_t n_tx, uint64_t *limbs_out,
                           double *total_out);

/* Device-resident class table for infer.em / infer.quantify
 * (seekmer/infer.py:88-168).  class_counts are f8 as in
 * SummarizedResult.class_count. */
typedef struct skm_quant skm_quant;
int skm_quant_create(int device, int64_t n_tx, int64_t n_classes,
                     const int64_t *class_offsets, const int32_t *class_targets,
                     const double *class_counts, skm_quant **out);
/* Same, taking the table straight from a mapper without leaving HBM. */
int skm_quant_create_from_mapper(skm_mapper *mapper, int64_t n_tx, skm_quant **out);
int skm_quant_destroy(skm_quant *quant);
/* infer.em (seekmer/infer.py:133-168): x inout [n_tx], l = effective lengths.
 * Stops on the reference criterion max_{x'>x_floor} |x'-x|/x' <= rel_tol
 * (0.01, 1e-8 in the reference); fixed_iters>0 runs exactly that many steps
 * instead; max_iters>0 caps.  *iters = steps done.  Returns SKM_ERR_UNDEFINED
 * where numpy would raise (no x' > x_floor). */
int skm_quant_em(skm_quant *quant, double *x, const double *l, double rel_tol,
                 double x_floor, int64_t max_iters, int64_t fixed_iters,
                 int64_t *iters);
/* One bootstrap replicate set (seekmer/infer.py:79-82,108-111): n_boot
 * multinomial resamples of the class counts (counter-based RNG, `seed`), EM
 * from x0 each; out[n_boot][n_tx] raw EM results (before TPM scaling);
 * counts_out (optional) [n_boot][C] the resampled counts. */
int skm_quant_bootstrap(skm_quant *quant, int64_t n_boot, uint64_t seed,
                        const double *x0, const double *l, double rel_tol,
                        double x_floor, int64_t max_iters, double *out,
                        int64_t *counts_out, int64_t *iters_out);
/* The same with every replicate returned as the TPM vector quantify() makes of it
 * (seekmer/infer.py:127-129: x /= x.sum() / 1e6; x[x < 0.001] = 0; again), numpy's summation
 * order restated on the device -- what run() appends to its bootstrap list (infer.py:79-82). */
int skm_quant_bootstrap_tpm(skm_quant *quant, int64_t n_boot, uint64_t seed,
                            const double *x0, const double *l, double rel_tol,
                            double x_floor, int64_t max_iters, double *out,
                            int64_t *iters_out);
/* One rank's share of the `-b N` loop: the n_boot replicates numbered first,
 * first + step, first + 2 step, ... of the run; out[n_boot][n_tx] as skm_quant_bootstrap_tpm.  A
 * replicate's draw depends on (seed, its number) alone, so ranks r = 0 .. G-1 calling with
 * (first = r, step = G) on the same merged table produce, together, exactly the replicates of
 * skm_quant_bootstrap_tpm(N) -- no collective, one gather of the results. */
int skm_quant_bootstrap_share_tpm(skm_quant *quant, int64_t n_boot, int64_t first, int64_t step,
                                  uint64_t seed, const double *x0, const double *l, double rel_tol,
                                  double x_floor, int64_t max_iters, double *out,
                                  int64_t *iters_out);
/* EM with externally supplied class counts (parity of the bootstrap EM leg). */
int skm_quant_set_counts(skm_quant *quant, const double *class_counts);
/* K EM problems on the handle's class structure that differ in their class counts only: counts[K][C]
 * (host, the caller's class order), the common start vector x0[n_tx] and effective lengths l[n_tx];
 * out[K][n_tx] = the raw EM results, or with tpm != 0 the vectors quantify() makes of them
 * (seekmer/infer.py:127-129); iters_out[K] (optional) the steps of each.  Eight problems run side by
 * side and a place is refilled when its problem stops; every result and step count is bit for bit what
 * skm_quant_set_counts + skm_quant_em give for that count vector, whatever its neighbours are.  The
 * handle holds its own counts again afterwards.  SKM_ERR_UNDEFINED when a problem leaves no abundance
 * above x_floor; SKM_ERR_STATE with a communicator of several ranks attached (with one of one rank the
 * problems run one by one); n_sets == 0 does nothing. */
int skm_quant_em_many(skm_quant *quant, int64_t n_sets, const double *counts, const double *x0,
                      const double *l, double rel_tol, double x_floor, int tpm, double *out,
                      int64_t *iters_out);
/* The second round of impute (seekmer/impute.py:101-108, 229-252) as such a set of problems: the
 * handle holds the concatenation of all cells' classes with their OWN counts; class_cell[C] = the cell
 * a class came from, weight[n_cells][n_cells] row-major, cell_total[n_cells] = each cell's own count
 * sum.  Problem i = the table blended for cell i: class k counts ((own[k] * weight[i][class_cell[k]])
 * * cell_total[i]) / cell_total[class_cell[k]], made on the device.  counts_out (optional,
 * [n_cells][C], the caller's class order) returns the blended counts.  SKM_ERR_ARG also for a
 * class_cell value outside [0, n_cells).  Otherwise as skm_quant_em_many. */
int skm_quant_em_blend(skm_quant *quant, int64_t n_cells, const int32_t *class_cell,
                       const double *weight, const double *cell_total, const double *x0,
                       const double *l, double rel_tol, double x_floor, int tpm, double *out,
                       int64_t *iters_out, double *counts_out);
/* K DIFFERENT class tables over the same n_tx transcripts in shared EM launches (the companion of
 * skm_quant_em_many, which runs K count vectors on one table).  The tables are given as one host CSR:
 * table s owns classes [table_class_offsets[s], table_class_offsets[s + 1]) of class_offsets /
 * class_counts, class c the targets [class_offsets[c], class_offsets[c + 1]) of class_targets, each
 * target in [0, n_tx).  Table s starts from x0[s][n_tx] with the effective lengths l[s][n_tx].  The
 * tables are stacked into one block-diagonal problem (transcript t of table s is transcript s n_tx + t)
 * whose steps run in launches with one grid row per table; every table meets its own stopping rule
 * and is frozen from then on.  out[s][n_tx] and iters[s] (optional) are bit for bit what
 * skm_quant_create + skm_quant_em give for table s alone; tpm != 0: scaled as quantify() scales
 * (seekmer/infer.py:127-129).  A table without classes gives zeros and 0 steps.  The tables run in
 * groups of consecutive tables: stacked transcripts, classes and pairs of a group stay below 2^31, its
 * buffers within about 2 GiB (skm_set_quant_groups), its tables at most SKM_SET_QUANT_GROUP when that
 * is set (tests).  SKM_ERR_UNDEFINED when a table leaves no abundance above x_floor (the message names
 * the lowest such table); SKM_ERR_ARG, before any device work, for negative sizes, NULL arrays,
 * offsets that are not monotone and targets outside [0, n_tx); n_tables == 0 does nothing.  A class
 * without a tuple entry counts in its table's total and in nothing else, as in skm_quant_create (it is
 * left out of the stacked problem); a table whose classes are all such is SKM_ERR_ARG. */
int skm_quant_em_tables(int device, int64_t n_tx, int64_t n_tables, const int64_t *table_class_offsets,
                        const int64_t *class_offsets, const int32_t *class_targets,
                        const double *class_counts, const double *x0, const double *l, double rel_tol,
                        double x_floor, int64_t max_iters, int tpm, double *out, int64_t *iters);
/* The group cut of skm_quant_em_tables and skm_sample_set_quantify on the host alone (no GPU is
 * touched; tests): tables of table_classes[i] classes and table_ids[i] (class, target) pairs, at most
 * max_slots a group -> group g = tables [group_first[g], group_first[g + 1]), g < *n_groups
 * (group_first has room for n_tables + 1).  A table joins the group under way while the group keeps
 * at most max_slots (and 32768) tables, (tables) n_tx, its classes and its pairs below 2^31, and
 * tables * n_tx * 96 + classes * 64 + pairs * 24 bytes within 2^31; a group always holds one table. */
int skm_set_quant_groups(int64_t n_tables, int64_t n_tx, const int64_t *table_classes,
                         const int64_t *table_ids, int64_t max_slots, int64_t *n_groups,
                         int64_t *group_first);
/* quantify(summary) for every sample of a set, in shared EM launches as skm_quant_em_tables runs
 * them; the class tuples are gathered on the device from the set's table into the stacked problem.
 * lengths[n_tx] = the transcript lengths.  Sample i's effective lengths come from its own histogram
 * when the set keeps them (skm_sample_set_keep_histograms), from the pooled one otherwise; its start
 * vector is 1 / effective length over numpy's sum, its total its aligned units.  tpm[S][n_tx],
 * effective_lengths[S][n_tx] (optional) and iters[S] (optional) for the S = *n_samples samples named
 * so far are bit for bit what infer.quantify() gives on the sample's summary; a sample without
 * classes gives zeros and 0 steps.  Waits for everything added to be mapped and keeps adders waiting,
 * as _summary.  SKM_ERR_ARG when cap_samples (rows of room) is below S or a class names a transcript
 * not below n_tx; SKM_ERR_UNDEFINED as skm_quant_em_tables. */
int skm_sample_set_quantify(skm_sample_set *set, const double *lengths, int64_t n_tx, double rel_tol,
                            double x_floor, int64_t max_iters, int64_t cap_samples,
                            int64_t *n_samples, double *tpm, double *effective_lengths,
                            int64_t *iters);
/* The connected components of the (class, transcript) graph and the tiles the one-GPU EM steps them in
 * (diagnostics, tests).  info[0] = tiles were built, [1] = tiles, [2] = components above the tile capacity
 * (any: the EM steps the whole table as one problem), [3] = the EM of this handle runs on the tiles,
 * [4..6] = tile capacity in pairs, classes, transcripts, [7] = transcript ids per packing run (a tile lies
 * within one run).  Optional arrays: tx_label[n_tx] = smallest
 * transcript id of the transcript's component, tx_tile[n_tx] = its tile (n_tx: none), class_tile
 * [n_classes] = tile of every class in the caller's class order. */
int skm_quant_components(skm_quant *quant, int64_t info[8], int32_t *tx_label, int32_t *tx_tile,
                         int32_t *class_tile);
/* The tiles' arrays as the set-up left them on the device (EmTiles; diagnostics, tests), every array optional.
 * With S = tiles, T = n_tx, C = classes, M = pairs of the handle: tile_tx[S + 1] and tile_cls[S + 1] first place of
 * tile i in tx_list / cls_list; tx_list[T] transcript ids and cls_list[C] INTERNAL class indices, tile by tile;
 * tx_pair[T + 1] and cls_pair[C + 1] by place in the lists: first pair of the member in tx_cls / cls_tx;
 * cls_tx[M] tile-local transcript of every pair, class-major; tx_cls[M] tile-local class of every pair,
 * transcript-major; order[S] the tiles in launch order; perm[C] the caller's index of internal class k.
 * Only what belongs to the tiles is defined: list places below tile_tx[S] / tile_cls[S], the pair entries up to and
 * including those places, pairs below cls_pair[tile_cls[S]]; whatever lies behind belongs to components above
 * the capacity and is never read.  SKM_ERR_ARG when no tiles were built for the handle. */
int skm_quant_tile_arrays(skm_quant *quant, int64_t *tile_tx, int64_t *tile_cls, int32_t *tx_list, int32_t *cls_list,
                          int64_t *tx_pair, int64_t *cls_pair, uint16_t *cls_tx, uint16_t *tx_cls, int32_t *order,
                          int32_t *perm);
/* *built = 1 when the handle holds the whole table's transcript-major rows, 0 when no reader has asked for them
 * yet (diagnostics, tests).  The tile EM reads none of them: a handle whose table is tiles alone builds them when the
 * whole-table EM, the batched EM (skm_quant_em_many, _em_blend, the bootstrap) or a residual problem first needs
 * them; a handle with components above the tile capacity, or without tiles, at the latest with its first EM. */
int skm_quant_rows_built(skm_quant *quant, int *built);
/* numpy.sum(values[0 .. n)) as the device adds it up for the start vector and the TPM scaling (diagnostics, tests):
 * upload, the production launches, download.  *sum = the sum (n = 0: 0.0).  SKM_ERR_ARG for n < 0, n >= 2^31, NULL. */
int skm_device_np_sum_probe(int device, const double *values, int64_t n, double *sum);
/* timing[0]=EM kernel ns total [1]=iterations [2]=launches */
int skm_quant_timing(skm_quant *quant, double timing[4]);

/* ---------------------------------------------------------------- multi-GPU
 * Not in the reference (single process).  Reads shard across ranks; the only
 * data-path collective is one all-reduce(sum) of f64[n_tx] per EM step (RCCL
 * over xGMI), issued on the EM stream between the class pass and the
 * finalise pass.  A communicator is created once per process and attached to
 * every quant handle that should take part. */
typedef struct skm_comm skm_comm;
int skm_comm_unique_id(void *id128);                 /* rank 0: 128-byte id, single use */
int skm_comm_create(int device, const void *id128, int rank, int world, skm_comm **out);
int skm_comm_count(skm_comm *comm, int *count);     /* ncclCommCount: ranks RCCL itself sees */
int skm_comm_destroy(skm_comm *comm);
/* The table hand-over of SURVEY.md 8(e).1 over xGMI: `send`'s table goes to rank send_to as it lies
 * in HBM (ncclSend of skm_mapper_device_table's arrays), the table rank recv_from sends is received
 * into HBM and merged into `recv` by key (skm_mapper_merge_device) -- no host copy, no host sort.
 * Either side may be NULL.  Matching calls: rank r: (mapper, 0, NULL, -1), rank 0: (NULL, -1,
 * mapper, r) for every r > 0 in turn.  Experimental: no multi-GPU node has run it; a rank sending
 * to itself is what the one-GPU test exercises. */
int skm_mapper_exchange_tables(skm_mapper *send, int send_to, skm_mapper *recv, int recv_from, skm_comm *comm);
int skm_quant_set_comm(skm_quant *quant, skm_comm *comm);   /* NULL detaches */

/* One sample, mapper table -> TPM, without leaving the device: MapResult.effective_lengths
 * (seekmer/mapper.py:134-141, the histogram all-reduced over `comm`'s ranks when comm is
 * not NULL) + quantify() (seekmer/infer.py:88-130: start vector 1/l normalised with
 * numpy's sum, em(), TPM scaling).  lengths: host f8[n_tx] transcript lengths.  Host
 * outputs (each may be NULL): tpm[n_tx], effective_lengths[n_tx], *iters. */
int skm_quant_infer(skm_mapper *mapper, skm_comm *comm, const double *lengths, int64_t n_tx,
                    double rel_tol, double x_floor, int64_t max_iters,
                    double *tpm, double *effective_lengths, int64_t *iters);

/* ============================ libseekmer_host.so ========================== */

/* ContigAssembler.assemble (seekmer/_index_builder.pyx:105-150): pooled
 * transcript bases, transcript i = [seq_offsets[i], seq_offsets[i+1]). */
typedef struct skm_built skm_built;
int skm_build_index(const char *pool, const int64_t *seq_offsets, int64_t n_seqs,
                    int n_threads, skm_built **out);
/* sizes[0]=n_slots [1]=n_contigs [2]=n_bases [3]=n_targets */
int skm_built_sizes(const skm_built *b, int64_t sizes[4]);
int skm_built_copy(const skm_built *b, void *kmers, void *contigs,
                   char *sequences, void *targets);
int skm_built_free(skm_built *b);

/* feed_single_ended_reads / feed_pair_ended_reads (seekmer/common.py:126-197)
 * as a native batch packer over already-decompressed FASTQ text. */
typedef struct skm_fastq skm_fastq;
int skm_fastq_open(const char *const *paths, int n_paths, int paired,
                   int64_t batch_units, skm_fastq **out);
/* Before the first skm_fastq_next.  set_allocator: where slabs live (default malloc/free; with
 * skm_pinned_alloc/skm_pinned_free a batch crosses PCIe by DMA straight from its slab).
 * set_parallel: n_threads > 0 asks for the parallel engine -- the files are memory-mapped, their
 * newlines counted once, and whole batches are parsed side by side by n_threads workers and
 * handed out in file order; same batches as the sequential engine.  It needs plain files whose
 * line counts are multiples of four; *enabled = 0 (and the sequential engine stays) otherwise. */
int skm_fastq_set_allocator(skm_fastq *reader, void *(*alloc)(size_t), void (*release)(void *));
int skm_fastq_set_parallel(skm_fastq *reader, int n_threads, int *enabled);
/* Several readers, one sample (one rank per GPU): reader `rank` of `world` hands out the
 * batches k with k % world == rank (the parallel engine parses only those; the sequential
 * engine has to read past the others).  skm_fastq_batch_index: k of the batch handed out last
 * -- its first unit is k * batch_units of the whole sample. */
int skm_fastq_set_shard(skm_fastq *reader, int rank, int world);
int skm_fastq_batch_index(const skm_fastq *reader, int64_t *index);
/* the common length of the reads of the batch handed out last, or -1 when they differ
 * (skm_mapper_map_batch_uniform_async takes a batch of equal-length reads without offsets) */
int skm_fastq_batch_read_length(const skm_fastq *reader, int64_t *read_len);
/* next batch: *n_units = 0 at end.  Buffers are owned by the reader and stay
 * valid until the next call.  names: '\n'-separated. */
int skm_fastq_next(skm_fastq *reader, int64_t *n_units, const char **bases,
                   const int64_t **offsets, const char **names,
                   const int64_t **name_offsets);
/* Keep the arrays of the last skm_fastq_next alive past the next call: the
 * reader hands their storage over as *slab and fills another one from now on.
 * skm_fastq_recycle gives it back for re-use (reader NULL: just frees it) --
 * a large batch costs more in first-touch page faults than in parsing. */
typedef struct skm_fastq_slab skm_fastq_slab;
int skm_fastq_detach(skm_fastq *reader, skm_fastq_slab **slab);
int skm_fastq_recycle(skm_fastq *reader, skm_fastq_slab *slab);
int skm_fastq_close(skm_fastq *reader);

/* Bytes of file mappings nobody has open that the readers may keep for the next reader of the same
 * file (default 0: a mapping goes when its last reader closes; a caller that reads the same files
 * again and again -- a benchmark's passes -- saves the page-table set-up of the later passes). */
int skm_fastq_cache_bytes(int64_t bytes);
/* The page tables of the input ahead of its reader: map the files now and touch their pages from
 * n_threads helper threads -- for a run that knows its FASTQ files while it is still loading the index
 * (setting up the page tables of the text costs as much as parsing it).  A reader opened before
 * _finish finds the mappings in place; _finish stops the helpers and drops what nobody has open. */
/* File mappings that no reader uses any more (beyond skm_fastq_cache_bytes) are unmapped by a
 * background thread in small pieces.  _wait_unmapped returns once none of that is under way: for a
 * caller about to time a phase that faults pages or allocates -- both wait for the process's
 * memory-map lock, which the teardown takes over and over. */
int skm_fastq_wait_unmapped(void);
typedef struct skm_fastq_prefault skm_fastq_prefault;
int skm_fastq_prefault_start(const char *const *paths, int n_paths, int n_threads, skm_fastq_prefault **out);
int skm_fastq_prefault_finish(skm_fastq_prefault *handle);

/* ---- FASTQ text -> 2-bit reads on the host (skm_packed_reads, above) ------------------------- */
/* feed_single_ended_reads / feed_pair_ended_reads (seekmer/common.py:126-197) for plain (not
 * compressed) files, straight to packed pieces in ONE pass over the text: the files are cut into
 * `chunk_bytes` ranges that n_threads workers parse side by side, each from the first place in its
 * range that looks like a record start; the reader hands the pieces out in file order and checks,
 * piece by piece, that the walk before ended exactly where this one started -- the reference's
 * rule is purely line-number based (`i & 3`), and only that chain proves a guessed start to be a
 * line with i & 3 == 0.  A piece whose guess fails is parsed again from the proven place (one
 * thread), so the reads are the reference's for any text.  Paired input is two streams, mate 1
 * files and mate 2 files, each numbered by unit; a pair of files counts min(records) units
 * (zip(file1, file2)), and a piece whose first_read lies below what its stream already delivered
 * replaces the reads from there on.  A trailing name line without a bases line is dropped.
 * n_threads = 0 parses inside skm_fastq_packed_next.  SKM_ERR_IO: not regular files (pipes from
 * decompressors go through skm_fastq_open). */
typedef struct skm_fastq_packed skm_fastq_packed;
int skm_fastq_packed_open(const char *const *paths, int n_paths, int paired, int n_threads,
                          int64_t chunk_bytes, int want_names, skm_fastq_packed **out);
/* The same reader over a SHARE of the files, for a sample shared out over ranks
 * (NativeReadFeeder(shard=...) does this for the two-pass reader; seekmer/common.py:126-197 is one
 * process): file i is read from byte begin[i] to byte end[i], both starts of lines whose number is
 * a multiple of four (skm_fastq_locate_line), and the first unit carries the number first_unit --
 * pieces are numbered as the one-process reader numbers them.  A pair of files must hold the same
 * number of records in its two ranges. */
int skm_fastq_packed_open_ranges(const char *const *paths, int n_paths, int paired, int n_threads,
                                 int64_t chunk_bytes, int want_names, const int64_t *begin,
                                 const int64_t *end, int64_t first_unit, skm_fastq_packed **out);
/* Where the lines of a file start, without parsing it: the reference's records are lines 4u .. 4u + 3
 * of a file whatever they hold, so the place of unit u takes the number of newlines before it.
 * _count_newlines fills counts[k] for the chunks k = first_chunk, first_chunk + chunk_step, ... of
 * `chunk_bytes` bytes (n_chunks = ceil(file size / chunk_bytes), SKM_ERR_ARG otherwise; the other
 * entries are left alone: ranks count a share each and add the tables up), *last_line_open = the
 * file does not end in a newline (its last line counts all the same).  _locate_line: the byte at
 * which line `line` (from 0) starts given the counts of ALL chunks -- one chunk is walked --, the
 * file's size when it has fewer lines; SKM_ERR_STATE when the counts are not this file's. */
int skm_fastq_count_newlines(const char *path, int64_t chunk_bytes, int64_t first_chunk,
                             int64_t chunk_step, int n_threads, int64_t *counts, int64_t n_chunks,
                             int *last_line_open);
int skm_fastq_locate_line(const char *path, int64_t chunk_bytes, const int64_t *counts,
                          int64_t n_chunks, int64_t line, int64_t *byte_offset);
/* where the arrays that cross PCIe live (before the first _next; see skm_fastq_set_allocator) */
int skm_fastq_packed_set_allocator(skm_fastq_packed *reader, void *(*alloc)(size_t),
                                   void (*release)(void *));
/* next piece; piece->n_reads == 0 (and code_words != SKM_PACKED_CUT) at the end.  The arrays stay
 * valid through ONE more call (skm_packed_source's contract: the mapper's drain copies piece k to
 * the GPU while it asks for piece k + 1).  The signature is skm_packed_source (below) with the
 * reader as context. */
int skm_fastq_packed_next(void *reader, skm_packed_reads *piece);
/* stats[0]=pieces accepted as guessed [1]=pieces parsed again [2]=reads [3]=exceptions
 * [4]=parser variant in use (0 single characters, 1 16-byte blocks, 2 32-byte blocks)
 * [5]=units of the sample so far (paired: min over the two streams, per pair of files) */
int skm_fastq_packed_stats(const skm_fastq_packed *reader, int64_t stats[8]);
/* About how many units the files hold (each mate-1 / single-end file's size over the extent of its
 * first record): the hint for skm_mapper_expect_units. */
int skm_fastq_packed_estimate(const skm_fastq_packed *reader, int64_t *units);
int skm_fastq_packed_close(skm_fastq_packed *reader);
/* The same packing for reads that are already in memory (bases back to back + offsets, the layout
 * of skm_mapper_map_batch): codes[n_reads][code_words], lengths[n_reads]; exception arrays hold up
 * to cap_exceptions entries, *n_exceptions = how many there are (SKM_ERR_STATE when more than the
 * capacity, SKM_ERR_ARG when a read is longer than 32 * code_words).  variant: -1 best available,
 * or 0 / 1 / 2 as in skm_fastq_packed_stats (SKM_ERR_STATE when this CPU lacks it). */
int skm_pack_reads(const char *bases, const int64_t *offsets, int64_t n_reads, int32_t code_words,
                   uint64_t *codes, uint32_t *lengths, uint32_t *exception_reads,
                   uint32_t *exception_masks, int64_t cap_exceptions, int64_t *n_exceptions,
                   int variant);
/* force the parser variant of readers opened from now on (-1: best available); tests */
int skm_pack_set_variant(int variant);

/* Selected reads of packed pieces as ONE new piece (the demultiplexer's gather: no GPU).  The n_sources pieces
 * are numbered through -- read i of the concatenation is read i - (reads of the pieces before) of its piece --
 * and output read k = read order[k] of that numbering, k < count: codes[count][code_words] (code_words >= every
 * source's; the words beyond a source's are zero), lengths[count], and the exceptions of the chosen reads
 * re-indexed to k and ascending: exception_reads[*n_exceptions], exception_masks[*n_exceptions][code_words].
 * With codes == NULL the call only counts: *n_exceptions = the entries the same call will write (the sizing
 * call).  SKM_ERR_STATE when there are more than cap_exceptions (*n_exceptions says how many); SKM_ERR_ARG for
 * an order entry outside the pieces, a source wider than code_words, NULL arrays.  `stream`, `first_read` and
 * the names of the sources are not looked at. */
int skm_packed_gather(const skm_packed_reads *sources, int64_t n_sources, const int32_t *order, int64_t count,
                      int32_t code_words, uint64_t *codes, uint32_t *lengths, uint32_t *exception_reads,
                      uint32_t *exception_masks, int64_t cap_exceptions, int64_t *n_exceptions);

/* Seeded synthetic data; integer arithmetic only. */
int skm_synth_transcriptome(uint64_t seed, int64_t n_genes, int64_t *n_tx,
                            char **pool, int64_t **offsets);
int skm_synth_free(void *p);
int skm_synth_reads(uint64_t seed, const char *pool, const int64_t *tx_offsets,
                    int64_t n_tx, int64_t first_unit, int64_t n_units,
                    int read_len, int paired, int n_threads, char *bases);

/* The same reads as FASTQ text (names r<ten digits>/<mate>, constant qualities), for measuring
 * the path from files: bases = [n_units][mates][read_len] as skm_synth_reads fills it. */
int skm_synth_fastq_write(const char *bases, int64_t n_units, int read_len, int paired,
                          int64_t first_unit, const char *path1, const char *path2,
                          int n_threads);

#ifdef __cplusplus
}
#endif
#endif
