// Host-visible declarations of the kernel launchers (one translation unit per
// kernel family) and the plain structs they take.
#pragma once
#include "skm_device.h"

namespace skm {

// One batch on its way through the mapper (all pointers are device memory).
struct MapBatch {
    const uint32_t *records;      // [n_reads][record_words]: codes (u64 x W), ACGT bits (u32 x W), length
    int64_t n_units;
    int32_t words_per_read;       // W
    int32_t record_words;         // u32 words per record, a multiple of 16 (64 bytes)
    int32_t paired;
    int32_t *workspace;           // per-context mask extension words (slices > 64 targets)
    // Results.  Units finish out of order, so a wave writes what it finishes as RECORDS: 64
    // finished units take 64 consecutive places of their block's own range (block b owns
    // records [b * per_block, ...) like it owns those units), and the three stores of a wave
    // are full sectors.  Record r = {unit index, class key, arena offset | tuple length << 40}.
    int32_t *rec_unit;
    uint64_t *rec_key;            // 64-bit class key, 0 = empty tuple
    unsigned long long *rec_tuple;
    // per-unit spans (begin, end, anchor of MappedSpan, _common.pxd:31-35), by unit index;
    // only written when keep_spans is set (parity tests, diagnostics): nothing on the infer
    // path reads them
    int32_t keep_spans;
    int32_t *unit_begin, *unit_end;
    Coord *unit_anchor;
    int32_t *unit_entries;        // signed target entries, units in arena order
    int64_t ids_capacity;
    // ids a wave takes from the entry arena per atomic at the least (MAP_ARENA_CHUNK); 0: exactly what
    // an emission writes, so that the final cursor is the sum of the tuple lengths (the relaunch
    // after an overflow, map_batch_resident)
    int32_t ids_chunk;
    unsigned long long *ids_cursor;
    unsigned long long *fld;      // [2000] batch-local histogram
    unsigned long long *stats;    // [16] access counters (STATS build only)
    int32_t vote[8];              // quorum per action: start, lookup, merge, left, right, emit, scan
};

// map kernel geometry: lanes per persistent block and the occupancy the register
// allocator is asked to fit (waves per SIMD); 4 blocks per CU either way (LDS)
#ifndef SKM_MAP_THREADS
#define SKM_MAP_THREADS 256
#endif
#ifndef SKM_MAP_WAVES_PER_EU
#define SKM_MAP_WAVES_PER_EU 4
#endif
constexpr int MAP_THREADS = SKM_MAP_THREADS;
constexpr int MAP_BLOCKS_PER_CU = 4;
constexpr int MAP_LDS_PER_BLOCK = 160 * 1024 / MAP_BLOCKS_PER_CU;   // bytes of LDS a block may take
constexpr int MAP_ARENA_CHUNK = 2048;            // ids a wave takes from the entry arena per atomic

// ---- unit contexts of the map kernel: two layouts of one body (skm_map.hip: WideContexts, PackedContexts)
// The WIDE layout holds every launch the library accepts: 16 words + 7 ring entries + half a pair counter a
// context, 80 bytes, 480 contexts a block.  The PACKED layout keeps the same fields in 13 words:
//   state word   state | first hit kept | attempt | list size n | list length + 1 | list orientation
//   left word    span.begin | span.end | "is ACGT" bits of the read's last 8 bases
//   scan word    scan position | read length | "is ACGT" bits of the read's first 8 bases
// and two bits a pair slot for the pair counter: 66 1/8 bytes, MAP_CONTEXTS contexts in the same LDS.  What the
// widths below cannot hold takes the wide kernel (map_geometry).
constexpr int MAP_CONTEXTS_WIDE = 480;
#ifndef SKM_MAP_CONTEXTS
#define SKM_MAP_CONTEXTS 576
#endif
constexpr int MAP_CONTEXTS = SKM_MAP_CONTEXTS;   // contexts per block of the packed layout (tuning builds: at most what the LDS holds)
constexpr int MAP_PACKED_POS_BITS = 12;          // begin, end, scan position, read length: 0 .. read length
constexpr int MAP_PACKED_EDGE_BITS = 8;          // "is ACGT" of 8 bases
constexpr int MAP_PACKED_STATE_BITS = 5;         // (skm_map.hip asserts its last state fits)
constexpr int MAP_PACKED_COUNT_BITS = 12;        // entries left of the running list: 0 .. its length
constexpr int MAP_PACKED_TLEN_BITS = 12;         // length of the list's slice + 1 (0: the list is still to come)
static_assert(2 * MAP_PACKED_POS_BITS + MAP_PACKED_EDGE_BITS == 32, "three fields a word");
static_assert(MAP_PACKED_STATE_BITS + 2 + MAP_PACKED_COUNT_BITS + MAP_PACKED_TLEN_BITS + 1 == 32, "the state word");
constexpr int MAP_PACKED_MAX_LEN = (1 << MAP_PACKED_POS_BITS) - 1;           // longest read of a packed launch
constexpr int MAP_PACKED_MAX_TARGETS =                                       // largest max_target_count of one
    (1 << MAP_PACKED_COUNT_BITS) - 1 < (1 << MAP_PACKED_TLEN_BITS) - 2 ? (1 << MAP_PACKED_COUNT_BITS) - 1
                                                                       : (1 << MAP_PACKED_TLEN_BITS) - 2;
static_assert(MAP_CONTEXTS % 2 == 0 && MAP_CONTEXTS_WIDE % 2 == 0, "pair slots");
static_assert(MAP_CONTEXTS < 0x8000 && MAP_CONTEXTS_WIDE < 0x8000, "a ring entry is context | 0x8000");

// Which kernel a launch takes and its grid: a pure function of the launch's bounds.
//   max_len, max_target_count   the packed layout's bounds above (a context's unit index has 32 bits in both
//                               layouts -- narrowing it frees no word -- so units per block bound nothing)
//   block_cap                   SKM_TEST_MAP_BLOCKS, 0 = none
//   force                       MAP_LAYOUT_AUTO, or a test's choice; packed < 0: forced packed does not fit
enum : int { MAP_LAYOUT_AUTO = 0, MAP_LAYOUT_WIDE = 1, MAP_LAYOUT_PACKED = 2 };
struct MapGeometry {
    int packed;          // 1: map_units_kernel (packed contexts), 0: map_units_wide_kernel, -1: refused
    int contexts;        // contexts per block of that kernel
    int64_t blocks;
};
inline MapGeometry map_geometry(int64_t n_units, int max_len, int max_target_count, int cu_count, int block_cap,
                                int force)
{
    const bool fits = max_len <= MAP_PACKED_MAX_LEN && max_target_count <= MAP_PACKED_MAX_TARGETS;
    MapGeometry g{};
    g.packed = force == MAP_LAYOUT_WIDE ? 0 : (fits ? 1 : (force == MAP_LAYOUT_PACKED ? -1 : 0));
    g.contexts = g.packed == 1 ? MAP_CONTEXTS : MAP_CONTEXTS_WIDE;
    g.blocks = (n_units + g.contexts - 1) / g.contexts;
    if (g.blocks > (int64_t)cu_count * MAP_BLOCKS_PER_CU) g.blocks = (int64_t)cu_count * MAP_BLOCKS_PER_CU;
    if (block_cap > 0 && g.blocks > block_cap) g.blocks = block_cap;
    return g;
}

// ASCII reads -> records.  Blocks of pack_stage_reads(words_per_read) consecutive reads go through LDS
// (pack_reads_staged_kernel); 0 = reads too long for the stage, the launch takes pack_reads_kernel.
void launch_pack_reads(const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                       int words_per_read, int record_words, uint32_t *records, hipStream_t stream);
int pack_stage_reads(int words_per_read);
// host-packed reads (skm_packed_reads) -> records: `n_reads` reads whose code words lie `stride`
// u64 words apart go to dst, dst + dst_stride, ... (u32 words); *error = SKM_ERR_ARG when a length
// exceeds 32 * code_words.  Then the bit planes of the exception reads (indices relative to
// `first_read` of the same piece).
void launch_unpack_reads(const uint64_t *codes, int64_t stride, int code_words, const uint32_t *lengths,
                         uint32_t uniform_len, int64_t n_reads, int words_per_read, uint32_t *dst,
                         int64_t dst_stride, int *error, hipStream_t stream);
void launch_unpack_exceptions(const uint32_t *exc_reads, const uint32_t *exc_masks, int64_t n_exceptions,
                              int code_words, int64_t first_read, int words_per_read, uint32_t *dst,
                              int64_t dst_stride, hipStream_t stream);
// out[0] = longest read, out[1] = places where the offsets step backwards; then offsets -= base
void launch_offsets_scan(int64_t *offsets, int64_t n_reads, int64_t base, unsigned long long *out,
                         hipStream_t stream);
void launch_offsets_uniform(int64_t *offsets, int64_t n_reads, int64_t read_len, hipStream_t stream);
// build the bucket table from the reference table and check the reference probe (see DevBucket);
// report: [0] placed [1] placed outside the home bucket [2] k-mers met twice [3] slots the
// reference probe does not reach
void launch_bucket_build(const DevIndex &ix, uint64_t n_slots, DevBucket *buckets, uint32_t bucket_mask,
                         uint32_t bucket_shift, unsigned long long *report, hipStream_t stream);
// DevContig::succ of every record, by lookups over ix's bucket table (skm_index_create, once)
void launch_signature_build(const DevBucket *buckets, uint64_t n_buckets, uint64_t *signatures, uint32_t shift,
                            hipStream_t stream);
void launch_successor_build(const DevIndex &ix, DevContig *records, int64_t n_contigs, int force_lookup,
                            hipStream_t stream);
// one lookup per k-mer through the device functions of the index (skm_index_probe, tests); the caller has checked
// that the structure `mode` asks exists
void launch_index_probe(const DevIndex &ix, int mode, const uint64_t *kmers, int64_t n, int32_t *entry, int32_t *offset,
                        hipStream_t stream);
// stats: 0 production, 1 counting build, 2 census build (skm_map.hip); packed: MapGeometry::packed of the
// launch, whose grid and workspace the caller has sized for that kernel's contexts
void launch_map_units(const DevIndex &ix, const MapBatch &b, int grid_blocks, int stats, bool packed,
                      hipStream_t stream);
void launch_pack_sequences(const char *bases, int64_t n_bases, uint64_t *seq2, int64_t n_words,
                           hipStream_t stream);
// strand filter (skm_strand.hip), between the map kernel and class counting: every record of `b`
// keeps the entries of its unit that lie in the library's orientation (mode SKM_STRAND_FR: e >= 0,
// SKM_STRAND_RF: e < 0), compacted in place in the entry arena; its key and tuple length follow
void launch_strand_filter(const MapBatch &b, int mode, hipStream_t stream);

// ---- sample sets (skm_samples.hip): many samples' units in shared launches, one class table whose
// classes are (sample, tuple).  A SEGMENT is a run of consecutive units of one sample; the segments of
// a launch, and of the whole set in launch order, ascend by their first unit.
// index of the segment that holds `unit`: the last i with first[i] <= unit (first[0] <= unit)
template <class T>
__host__ __device__ __forceinline__ int64_t segment_find(const T *first, int64_t n, int64_t unit)
{
    int64_t lo = 0, hi = n;                       // first[lo] <= unit < first[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)first[mid] <= unit) lo = mid; else hi = mid;
    }
    return lo;
}
// the key of class (sample, tuple) from the tuple's key: for a fixed tuple key distinct samples give
// distinct keys (the constant is odd), so two samples' copies of one tuple never meet in a slot
constexpr uint64_t SAMPLE_KEY_STEP = 0xD6E8FEB86659FD93ULL;
__host__ __device__ __forceinline__ uint64_t sample_key(uint64_t key, uint32_t sample) { return key + sample * SAMPLE_KEY_STEP; }
constexpr int SAMPLE_LAUNCH_SEGMENTS = 2048;      // segments of one launch at most (their table lives in LDS)
struct SampleSalt {                               // the segments of one launch (device arrays)
    const int32_t *seg_first;                     // [n_segments] first unit of the segment inside the launch, ascending from 0
    const int32_t *seg_sample;                    // [n_segments]
    int32_t n_segments;
};
// between the strand filter and class counting: every record with a key takes the key of (its unit's
// sample, its tuple); a key that comes out as 0 raises SKM_ERR_COLLISION in *error (never "unaligned")
void launch_sample_salt(const MapBatch &b, const SampleSalt &salt, int *error, hipStream_t stream);
// after a launch mapped with keep_spans: hist[sample of unit u][fragment length of unit u] += 1 for every
// unit u < n_units of the launch whose span gives a length (the map kernel's fragment length rule on
// unit_begin / unit_end); hist holds MAX_FRAGMENT_LENGTH words for every sample the segments name
void launch_sample_fld(const int32_t *unit_begin, const int32_t *unit_end, int64_t n_units, const SampleSalt &salt,
                       unsigned long long *hist, hipStream_t stream);
// after the strand filter of a launch: rows[sample of the record's unit][hexamer] += 1 for every record whose
// tuple is not empty, by the rule of launch_bias_observed (skm_bias.h); rows holds 4096 words for every sample the
// segments name
void launch_sample_bias(const MapBatch &b, const SampleSalt &salt, unsigned long long *rows, hipStream_t stream);
// the set's segment log against the classes' global first-seen units: cls_sample[k], cls_local[k] =
// the sample of class k and its first-seen unit counted inside that sample
void launch_sample_assign(const int64_t *log_global, const int64_t *log_local, const int32_t *log_sample,
                          int64_t n_segments, const unsigned long long *cls_first_seen, int64_t n_classes,
                          int32_t *cls_sample, int64_t *cls_local, hipStream_t stream);

void launch_gather_probe(const void *table, uint64_t n_slots, int blocks, int per_lane, int chain,
                         unsigned long long *sink, hipStream_t stream);

// ---- equivalence-class table (skm_classes.hip)
struct alignas(32) ClassSlot {    // 32 B; key and first_seen side by side: one 16-byte load per probe
    unsigned long long key;       // 0 = empty
    unsigned long long first_seen;  // global unit index of the first unit of the class
    unsigned long long count;
    long long tuple;              // -1 until the tuple has been committed to the arena, then
                                  // arena offset (bits 0-39) | tuple length (bits 40-62)
};
// 64-bit key of a class tuple (unsigned ids in list order): tuple_key_seed(n), then one
// tuple_key_step per id.  The map kernel, the strand filter and the merge of foreign tables
// all key with these two, so equal tuples meet in one slot.  A result of 0 is stored as 1
// (0 marks an empty table slot).  Full tuples are compared later; this is only the tag.
__host__ __device__ __forceinline__ uint64_t tuple_key_seed(int n) { return 0x243F6A8885A308D3ULL ^ (uint64_t)n; }
__host__ __device__ __forceinline__ uint64_t tuple_key_step(uint64_t h, uint32_t id)
{
    h ^= id;
    h *= 0x9E3779B97F4A7C15ULL;
    h ^= h >> 32;
    return h;
}
__host__ __device__ inline long long tuple_pack(long long offset, int n) { return offset | ((long long)n << 40); }
__host__ __device__ inline long long tuple_offset(long long t) { return t & ((1LL << 40) - 1); }
__host__ __device__ inline int tuple_len(long long t) { return (int)(t >> 40); }
struct ClassTable {
    ClassSlot *slots;
    uint64_t slot_mask;
    int32_t *arena;               // committed tuples (unsigned ids)
    int64_t arena_capacity;
    unsigned long long *arena_cursor;
    unsigned long long *n_classes;
    unsigned long long *n_unaligned;
    unsigned long long *n_units;
    unsigned long long *global_fld;   // [2000]
    int64_t *class_list;          // dense registry: slot of every committed class
    int64_t class_list_capacity;
    unsigned long long *n_listed;
    unsigned long long *n_deferred;   // units whose probe ran past PROBE_LIMIT (table too full)
    unsigned long long *arena_committed;   // arena cursor as of the last finished launch
    int *error;                   // SKM_ERR_* raised by a kernel
};
constexpr int CLASS_PROBE_LIMIT = 128;
// The read-only probe beside probe_claim (skm_classes.hip), for a table that is final (no launch of the class kernels
// is under way): linear from key & slot_mask, ends at the key or at an empty slot, n_slots steps at most, plain
// loads only.  The slot of `key`, or ~0 when the table does not hold it.  `home_key` is the key word of the home
// slot, which the caller has fetched ahead (several probes in flight per lane).
__device__ __forceinline__ uint64_t class_probe_find(const ClassTable &t, unsigned long long key, unsigned long long home_key)
{
    uint64_t slot = key & t.slot_mask;
    unsigned long long cur = home_key;
    for (uint64_t n = 1; cur != key && cur != 0 && n <= t.slot_mask; ++n) {
        slot = (slot + 1) & t.slot_mask;
        cur = t.slots[slot].key;
    }
    return cur == key ? slot : ~0ULL;
}
// (the class kernels walk the batch record by record; unit_slot is indexed by record.)  insert:
// find-or-create + count + commit of the new classes + on-the-spot compare with classes of earlier
// launches, then the totals step (publishes the arena cursor; merge_fld: the batch histogram once)
void launch_class_insert(const ClassTable &t, const MapBatch &b, int64_t unit_base,
                         int64_t *unit_slot, bool retry_deferred, bool merge_fld, hipStream_t stream);
void launch_class_verify(const ClassTable &t, const MapBatch &b, const int64_t *unit_slot,
                         hipStream_t stream);
void launch_class_rehash(const ClassTable &from, const ClassTable &to, int64_t *forward,
                         hipStream_t stream);
void launch_slot_remap(int64_t *slots, int64_t n, const int64_t *forward, hipStream_t stream);
void launch_class_init(const ClassTable &t, hipStream_t stream);
void launch_class_compact(const ClassTable &t, int64_t n_classes, int64_t *cls_offset,
                          int64_t *cls_len, double *cls_count, unsigned long long *cls_first_seen,
                          hipStream_t stream);
void launch_class_merge(const ClassTable &t, int64_t n_classes, const int64_t *class_offsets,
                        const int32_t *class_targets, const int64_t *class_counts,
                        const int64_t *first_seen, hipStream_t stream);

// the same with the foreign table in HBM as class_compact leaves it (registry order, counts as
// doubles) + its unit totals and histogram: nothing crosses the host
void launch_class_merge_device(const ClassTable &t, int64_t n_classes, const int64_t *class_start,
                               const int64_t *class_len, const int32_t *ids, const double *class_counts,
                               const unsigned long long *first_seen, hipStream_t stream);
void launch_class_add_totals(const ClassTable &t, unsigned long long unaligned, unsigned long long units,
                             const unsigned long long *fld, hipStream_t stream);

// ---- quantification (skm_em.hip, skm_quant_setup.hip)
constexpr int EM_ROW_CAP = 512;   // longest run of one transcript's classes summed by one lane group

struct EmProblem {
    int64_t n_tx, n_classes, n_rows;
    // class-major side: class c owns ids[cls_offset[c] .. cls_offset[c+1])
    const int64_t *cls_offset;    // [C+1]
    const int32_t *ids;           // [M] transcript ids, tuple order inside a class
    const double *cls_count;      // [C]
    double *inner;                // [C] S_c / count_c of the current step
    // transcript-major side: rows = runs of <= EM_ROW_CAP entries of one transcript
    const int64_t *row_start;     // [R+1] into tx_cls
    const int32_t *row_tx;        // [R]
    const int32_t *tx_cls;        // [M] class index of every (transcript, class) pair, by transcript
    const int64_t *tx_row;        // [T+1] rows of each transcript
    double *row_sum;              // [R]
    const double *eff_len;        // [T]
    double *x[2];                 // ping-pong abundance vectors
    double *acc;                  // [T] numerators (multi-GPU all-reduce buffer)
    double n_total;               // sum of class counts over all ranks
    double rel_tol, x_floor;
    unsigned long long *ctl;      // control block: the CTL_ words below
    double *part_max;             // [EM_FINAL_BLOCKS]
    unsigned int *part_flags;     // [EM_FINAL_BLOCKS] bit0 = any, bit1 = nan
    int64_t max_iters, fixed_iters;
    // one rank: rows and finalize are ONE launch (em_rows_finalize_kernel); `arrivals` [T] counts the
    // rows of a many-row transcript that have been summed in the current step (zero between steps)
    int fused;
    unsigned int *arrivals;
    // further partials of the stopping rule, judged together with part_max / part_flags: those of the
    // component tiles (EmTiles::step_max, step_flags) when this problem is the residual beside them --
    // n_extra per step, the chunk's first step being number extra_first (0: none)
    const double *extra_max;
    const unsigned int *extra_flags;
    int64_t n_extra, extra_first;
};
// words of EmProblem::ctl: stopped, steps judged so far, no abundance above x_floor, a tile above the capacity
enum { CTL_DONE = 0, CTL_ITERS = 1, CTL_UNDEFINED = 3, CTL_TILE_FAULT = 4 };
#ifndef SKM_EM_FINAL_BLOCKS
#define SKM_EM_FINAL_BLOCKS 2048
#endif
constexpr int EM_FINAL_BLOCKS = SKM_EM_FINAL_BLOCKS;
// judge_previous: apply the stopping rule to finalize pass `steps_done` first (see em_evaluate)
void launch_em_inner(const EmProblem &p, int parity, bool judge_previous, int64_t steps_done, hipStream_t stream);
void launch_em_decide(const EmProblem &p, int64_t steps_done, hipStream_t stream);
void launch_em_rows(const EmProblem &p, int parity, hipStream_t stream);
void launch_em_rows_finalize(const EmProblem &p, int parity, hipStream_t stream);
void launch_em_rows_acc(const EmProblem &p, int parity, hipStream_t stream);   // several ranks: em_rows + em_rows_to_acc
void launch_em_rows_to_acc(const EmProblem &p, hipStream_t stream);
void launch_em_finalize(const EmProblem &p, int parity, bool from_acc, hipStream_t stream);
// out = the result of an EM that latched after ctl[CTL_ITERS] steps (x0 if even, x1 if odd)
void launch_em_result(const unsigned long long *ctl, const double *x0, const double *x1, int64_t n, double *out,
                      hipStream_t stream);

// ---- the EM of independent components in LDS (skm_em.hip: em_local_chunk_kernel).  One EM step couples a
// transcript only with the transcripts it shares a class with, so the connected components of the
// (class, transcript) graph can be stepped independently.  Consecutive components (by their smallest
// transcript id) are packed into TILES of at most EM_TILE_PAIRS pairs, EM_TILE_CLASSES classes and
// EM_TILE_TX transcripts; one workgroup keeps a tile's two views, `inner` and both abundance vectors in
// LDS and runs a whole chunk of steps with workgroup barriers only.
// (the four values are sweep aids, scripts/build_variant.sh with skm_abi_quant.hip, skm_em.hip and
// skm_quant_setup.hip: results do not depend on them)
#ifndef SKM_EM_TILE_PAIRS
#define SKM_EM_TILE_PAIRS 2048
#endif
#ifndef SKM_EM_TILE_CLASSES
#define SKM_EM_TILE_CLASSES 512
#endif
#ifndef SKM_EM_TILE_TX
#define SKM_EM_TILE_TX 128
#endif
#ifndef SKM_EM_TILE_SEGMENT
#define SKM_EM_TILE_SEGMENT 256
#endif
constexpr int EM_TILE_PAIRS = SKM_EM_TILE_PAIRS, EM_TILE_CLASSES = SKM_EM_TILE_CLASSES, EM_TILE_TX = SKM_EM_TILE_TX;
static_assert(EM_TILE_PAIRS <= 65535 && EM_TILE_CLASSES <= 65535 && EM_TILE_TX <= 65535, "tile-local indices and offsets are 16 bits wide");
constexpr int EM_TILE_SEGMENT = SKM_EM_TILE_SEGMENT;     // tiles are packed within runs of this many transcript ids (set-up)
static_assert(EM_TILE_SEGMENT > 0, "a packing run holds at least one transcript id");
constexpr int EM_CHUNK_MAX = 16;         // steps of one launch at most
constexpr int EM_TILE_CLASS_BATCH = 4;   // tuple entries a lane of the class phase fetches together; the set-up
                                         // lists a tile's classes by their number of such batches
struct EmTiles {
    int64_t n_tiles;
    const int64_t *tile_tx;       // [n_tiles + 1] first place of tile i in tx_list
    const int64_t *tile_cls;      // [n_tiles + 1] first place of tile i in cls_list
    const int32_t *tx_list;       // [T] transcript ids, tile by tile (inside a tile: those of many pairs first)
    const int32_t *cls_list;      // [C] internal class indices, tile by tile (inside a tile: those of many batches
                                  //     of EM_TILE_CLASS_BATCH entries first, ascending among equals)
    const int64_t *cls_pair;      // [C + 1] by place in cls_list: first pair of the class in cls_tx
    const int64_t *tx_pair;       // [T + 1] by place in tx_list: first pair of the transcript in tx_cls
                                  // (the four arrays above are written for the tiles' members and the one entry
                                  //  behind the last: what lies in no tile is listed nowhere and nothing reads it)
    const uint16_t *cls_tx;       // [M] tile-local transcript of every pair, class-major, tuple order
    const uint16_t *tx_cls;       // [M] tile-local class of every pair, transcript-major, internal class order
    double *step_max;             // [EM_CHUNK_MAX][n_tiles] the tiles' partials of the stopping rule, per step
    unsigned int *step_flags;     // [EM_CHUNK_MAX][n_tiles] bit0 = any, bit1 = nan
    double *snap;                 // [EM_CHUNK_MAX][T] the tiles' abundances after every step of the chunk in flight
    // the launch order: workgroup b of a chunk launch works on tile order[b], or order[n_tiles - 1 - b] with
    // order_reversed set; nullptr: on tile b.  A permutation of the tiles by descending pair count
    // (skm_quant_setup.hip: tile_order_kernel); no result depends on it.
    const int32_t *order;
    int32_t order_reversed;
    // tiles alone (no residual problem beside them): the chunk kernel judges its own steps and step_max /
    // step_flags are not written.  EM_JUDGE_WORDS words that are zero between launches (em_run clears them with
    // the control block; the workgroup that judges leaves them clear): [EM_JUDGE_MAX + s] the largest relative
    // change of step s over the tiles arrived so far (the bits of a double >= +0.0: they order as integers),
    // [EM_JUDGE_FLAGS + s] their flags, [EM_JUDGE_ARRIVED] the tiles arrived.  nullptr: step_max / step_flags.
    unsigned long long *judge;
};
// (each group of words in a 128-byte line of its own: the arrivals do not queue behind the partials)
enum { EM_JUDGE_MAX = 0, EM_JUDGE_FLAGS = 16, EM_JUDGE_ARRIVED = 32, EM_JUDGE_WORDS = 48 };
static_assert(EM_CHUNK_MAX <= 16, "a step's word of each kind");
constexpr int EM_CTL_WORDS = 16;         // EmProblem::ctl; a handle keeps the judge's words right behind them
// (tuning aid, scripts/build_variant.sh with skm_abi_quant.hip and skm_em.hip: 1 keeps the one-block launch that
// judged a chunk of tiles alone before the chunk kernel did)
#ifndef SKM_EM_JUDGE_LAUNCH
#define SKM_EM_JUDGE_LAUNCH 0
#endif
// Steps first_step + 1 .. first_step + n_steps (n_steps <= EM_CHUNK_MAX, the same for every chunk of a run) of
// every tile, from x_in (a tile reads its own transcripts only) to tiles.snap[0 .. n_steps).  Once the control
// block says stopped, the launch instead copies the tiles' entries of the step the EM stopped at -- one of the
// chunk before, still in tiles.snap -- to p.x[steps & 1].
void launch_em_local_chunk(const EmProblem &p, const EmTiles &tiles, const double *x_in, int n_steps, int64_t first_step,
                           hipStream_t stream);
// the stopping rule for steps first_step + 1 .. first_step + n_steps in order, from step_max / step_flags: latches
// the first that stops (SKM_EM_JUDGE_LAUNCH builds only)
#if SKM_EM_JUDGE_LAUNCH
void launch_em_local_decide(const EmProblem &p, const EmTiles &tiles, int64_t first_step, int n_steps, hipStream_t stream);
#endif

// ---- the EM for EM_BATCH problems of one class structure side by side (skm_em_batch.hip):
// the bootstrap replicates, count vectors of the caller's, the blended tables of the second round of `impute`.
// Arrays with a replicate dimension are [item][EM_BATCH].
constexpr int EM_BATCH = 8;
struct EmBatchProblem {
    int64_t n_tx, n_classes, n_rows;
    const int64_t *cls_offset;    // shared structure: as EmProblem
    const int32_t *ids;
    const int64_t *row_start;
    const int32_t *row_tx;
    const int32_t *tx_cls;
    const int64_t *tx_row;
    const double *eff_len;
    const double *cls_count;      // [C][EM_BATCH]
    double *inner;                // [C][EM_BATCH]
    double *row_sum;              // [R][EM_BATCH]
    double *x[2];                 // [T][EM_BATCH] ping-pong
    double *place_total;          // [EM_BATCH] sum of the class counts of the problem in each place (the refill writes it)
    double rel_tol, x_floor;
    unsigned long long *ctl;      // control block (32 words): the BCTL_ words below
    double *part_max;             // [EM_FINAL_BLOCKS][EM_BATCH]
    unsigned int *part_flags;     // [EM_FINAL_BLOCKS][EM_BATCH]
    int managed;                  // the device refills the places (launch_em_batch_manage): see skm_em_batch.hip
    unsigned long long *mgr;      // managed: the manager's words, planned for inside em_inner_batch (or nullptr)
    int64_t *iters_out;           // managed: step count of every replicate of the group
    int fused;                    // rows and finalize are one launch (em_rows_finalize_batch_kernel)
    unsigned int *arrivals;       // [T] rows of a many-row transcript summed so far in this step (zero between steps)
};
// words of EmBatchProblem::ctl: all stopped, the step at which the last one stopped; + r: replicate r
// stopped, its step count, undefined (no x above x_floor)
enum { BCTL_ALL_DONE = 0, BCTL_LAST_STEP = 1, BCTL_DONE = 8, BCTL_ITERS = 16, BCTL_UNDEFINED = 24 };
// words of `mgr` below: next replicate to start, replicates in the group, finished, a replicate had no
// abundance above x_floor; + r: replicate in place r + 1 (0: idle), the step it started at, the plan
// of this step: replicate to take / to put, + 1
enum { MGR_NEXT = 0, MGR_COUNT = 1, MGR_FINISHED = 2, MGR_UNDEFINED = 3, MGR_REP = 8, MGR_SINCE = 16, MGR_TAKE = 24,
       MGR_PUT = 32 };
// The working set kept full by the device: `mgr` is 64 words of HBM; counts_all[i][C] the class counts
// of replicate i of the group (internal class order), totals[2 i] their sum (pairs, as launch_np_sum_many
// leaves them), out_all[i][T] its result, iters_out[i] its step count (device memory).  _init fills the first places; _manage after EVERY step takes what has stopped and
// puts the next replicates in.  ctl[BCTL_ALL_DONE] is set once every replicate of the group has finished.
void launch_em_batch_manage_init(const EmBatchProblem &p, unsigned long long *mgr, unsigned long long *host_pinned64,
                                 int64_t n_reps, const double *counts_all, const double *totals, const double *x_start,
                                 double *out_all, hipStream_t stream);
void launch_em_batch_manage(const EmBatchProblem &p, unsigned long long *mgr, const double *counts_all, const double *totals,
                            const double *x_start, double *out_all, int64_t *iters_out, int64_t step, bool planned,
                            hipStream_t stream);
// one step (inner, rows, finalize); step > 0 first judges the step before it
void launch_em_batch_step(const EmBatchProblem &p, int64_t step, hipStream_t stream);
void launch_em_batch_decide(const EmBatchProblem &p, int64_t steps_done, hipStream_t stream);
// out[t] = x[t][r]
void launch_em_batch_take(const double *x, int64_t n_tx, int r, double *out, hipStream_t stream);
// fresh control block; bit r of `idle`: place r holds no replicate and counts as stopped
void launch_em_batch_ctl(unsigned long long *ctl, unsigned int idle, hipStream_t stream);
// rows[i][k] (i < n_rows, caller's class order) = the blended count of class k for cell first + i:
// ((own[k] * weight[first + i][class_cell[k]]) * cell_total[first + i]) / cell_total[class_cell[k]]
void launch_blend_counts(const double *own, const int32_t *class_cell, const double *weight, const double *cell_total,
                         int64_t n_cells, int64_t first, int64_t n_rows, int64_t n_classes, double *rows, hipStream_t stream);
// y[i][k] = x[i][perm[k]] for n_rows vectors of n doubles
void launch_permute_rows_f64(const double *x, const int32_t *perm, int64_t n, int64_t n_rows, double *y, hipStream_t stream);
// ---- the EM for many class tables over the same transcripts, stacked into one block-diagonal problem
// (skm_em_set.hip): table s of the group -- slot s -- owns stacked transcripts [s T, (s + 1) T), a class
// range and a row range of the stacked views, its own total and its own stopping rule.
struct EmSetSlot {                // 64 bytes, in HBM
    int64_t cls_first, cls_end;   // internal classes of the slot
    int64_t row_first, row_end;   // rows of the slot
    double n_total;               // sum of its class counts
    unsigned long long done;      // its control words: stopped (set from the start for a slot without classes),
    unsigned long long iters;     // steps judged so far = its step count once stopped,
    unsigned long long undefined; // no abundance above x_floor
};
struct EmSetProblem {
    const int64_t *cls_offset;    // the stacked views: as EmProblem
    const int32_t *ids;
    const double *cls_count;
    double *inner;
    const int64_t *row_start;
    const int32_t *row_tx;
    const int32_t *tx_cls;
    const int64_t *tx_row;
    double *row_sum;
    const double *eff_len;        // [slots][T]
    double *x[2];                 // [slots][T] ping-pong
    double rel_tol, x_floor;
    int64_t max_iters;
    EmSetSlot *slots;             // [n_slots]
    int n_slots;
    int n_parts;                  // blocks per slot of the rows launch = partials per slot (em_set_parts)
    double *part_max;             // [n_slots][n_parts]
    unsigned int *part_flags;     // [n_slots][n_parts] bit0 = any, bit1 = nan
    unsigned int *arrivals;       // [slots T] as EmProblem
};
// partials per slot for a group whose largest slot has `largest_rows` rows
int em_set_parts(int64_t largest_rows);
// one step (inner, rows + finalize) of every running slot; judge_previous: block (0, s) of the inner
// launch first applies slot s's stopping rule to finalize pass `step`
void launch_em_set_step(const EmSetProblem &p, int64_t largest_classes, int64_t step, bool judge_previous, hipStream_t stream);
// the stopping rule of every running slot for finalize pass steps_done; *running (zero before) += slots that go on
void launch_em_set_decide(const EmSetProblem &p, int64_t steps_done, unsigned long long *running, hipStream_t stream);
// out[s][t] = x[iters_s & 1][s T + t], zeros for a slot without classes
void launch_em_set_result(const EmSetSlot *slots, int n_slots, const double *x0, const double *x1, int64_t n_tx, double *out,
                          hipStream_t stream);
// ids[dst[k] + j] = arena[src[k] + j] + add[k] for j < dst[k + 1] - dst[k]
void launch_stack_tuples(const int64_t *src, const int64_t *dst, const int32_t *add, int64_t n_classes, const int32_t *arena,
                         int32_t *ids, hipStream_t stream);
// rows 1 .. n - 1 of x[n][n_tx] = row 0 (n <= 65536)
void launch_repeat_row(double *x, int64_t n_tx, int64_t n, hipStream_t stream);

// device-side construction of the class views (skm_quant_setup.hip)
struct QuantBuild {
    int64_t n_tx, n_classes, n_ids;
    int64_t *cls_offset;          // [C+1] out
    int32_t *ids;                 // [M]   out (class-major)
    double *cls_count;            // [C]   out
    int64_t first_seen_bound;     // every first-seen value of the table is below this (0: unknown)
    // the component tiles (EmTiles), built when tile_tx is given; tile_info[0] = tiles, [1] = components
    // above the tile capacity (then the tiles are not used), both read by the host when the set-up ends
    int64_t *tile_tx, *tile_cls;  // [T + 2], [T + 2] out
    int32_t *tx_list, *cls_list;  // [T], [C] out: the tiles' members (tile_tx[tiles], tile_cls[tiles] places)
    int64_t *cls_pair, *tx_pair;  // [C + 1], [T + 1] out: for those places and the one behind them
    uint16_t *tile_cls_tx, *tile_tx_cls;   // [M], [M] out
    int32_t *tx_label, *tx_tile, *cls_tile;   // [T], [T], [C] out: component (smallest id), tile of each
    int32_t *tile_order;          // [T + 1] out: the tiles by descending pair count (EmTiles::order)
    int64_t tile_info[2];
};
// One asynchronous pipeline: classes (from a mapper's table when `table` is given, the caller's
// order being first-seen order) in (smallest transcript id, caller's index) order for gather
// locality, perm[k] = caller's index of internal class k, then the component tiles from the classes
// alone.  Returns 0, or < 0.  The transcript-major rows are no part of it: quant_rows_build.
int quant_setup(const ClassTable *table, QuantBuild &q, int32_t *perm, hipStream_t stream);
// The transcript-major view of the whole table cut into rows of EM_ROW_CAP pairs, for the kernels that
// step the whole table (em_rows*_kernel, the batched and the set EM) and for the residual below.  The
// tile EM reads none of it, so a handle builds it when a reader first asks.  Queued on `stream`; the
// stream has drained on return.  Returns the number of rows, -3 when they exceed n_rows_cap, or < 0.
struct QuantRows {
    int32_t *tx_cls;              // [M]   out
    int64_t *tx_row;              // [T+1] out
    int64_t *row_start;           // [R+1] out (capacity n_rows_cap + 1)
    int32_t *row_tx;              // [R]   out
    int64_t n_rows_cap;
};
int64_t quant_rows_build(const QuantBuild &q, const QuantRows &rows, hipStream_t stream);
// The components above the tile capacity as an EM problem of their own (the "residual"): their classes
// (internal order kept, renumbered) and the rows of their transcripts, in the form em_inner_kernel and
// em_rows_finalize_kernel take; tx_row stays indexed by transcript id (no rows for a transcript of a tile).
// _count: counts[0] classes, [1] pairs, [2] rows (synchronises); _build: fills arrays of those sizes.
// Both read the whole table's rows.
struct QuantResidual {
    int64_t n_classes, n_ids, n_rows;
    int64_t *cls_offset;          // [n_classes + 1] out
    int32_t *ids;                 // [n_ids] out
    int32_t *cls_src;             // [n_classes] out: internal class index (where the count comes from)
    int64_t *row_start;           // [n_rows + 1] out
    int32_t *row_tx;              // [n_rows] out
    int32_t *tx_cls;              // [n_ids] out: residual class index
    int64_t *tx_row;              // [T + 1] out
};
int quant_residual_count(const QuantBuild &q, const QuantRows &rows, int64_t counts[3], hipStream_t stream);
int quant_residual_build(const QuantBuild &q, const QuantRows &rows, QuantResidual &r, hipStream_t stream);
// y[k] = x[perm[k]] (gather) or y[perm[k]] = x[k] (scatter), n doubles
void launch_permute_f64(const double *x, const int32_t *perm, int64_t n, double *y, bool scatter,
                        hipStream_t stream);
const char *quant_setup_failure();       // what made the last quant_setup of this thread return < 0
int64_t quant_rows_upper_bound(int64_t n_tx, int64_t n_ids);

// numpy.sum(a) bit for bit -> out[0], out[1] = out[0] / divisor; block_sums: ceil(n/8192) doubles
void launch_np_sum(const double *a, int64_t n, double divisor, double *block_sums, double *out,
                   hipStream_t stream);
// the same for `count` vectors `stride` elements apart: block_sums: count * ceil(n / 8192) doubles,
// out[2 v] = sum of vector v, out[2 v + 1] = sum / divisor
void launch_np_sum_many(const double *a, int64_t n, int64_t count, int64_t stride, double divisor,
                        double *block_sums, double *out, hipStream_t stream);
void launch_reciprocal(const double *l, int64_t n, double *x, hipStream_t stream);
void launch_divide(double *x, int64_t n, const double *s, bool threshold, double floor, hipStream_t stream);
// vector v of `count` (n elements, `stride` apart) divided by s[2 v]
void launch_divide_many(double *x, int64_t n, int64_t count, int64_t stride, const double *s, bool threshold,
                        double floor, hipStream_t stream);
void launch_effective_lengths(const unsigned long long *fld, const double *lengths, int64_t n_tx,
                              double *out, hipStream_t stream);
// the same for n <= 65535 histograms fld[n][2000] -> out[n][n_tx], row by row what the launch above gives
void launch_effective_lengths_many(const unsigned long long *fld, int64_t n, const double *lengths, int64_t n_tx,
                                   double *out, hipStream_t stream);
// the same rule with p given instead of counted (a fragment-length model): p[n][2000] -> out[n][n_tx],
// 1 <= n <= 65535, weights finite and >= 0
void launch_effective_lengths_weights(const double *p, int64_t n, const double *lengths, int64_t n_tx, double *out,
                                      hipStream_t stream);
// multinomial(n_draws, counts / n_draws) over the classes whose inclusive cumulative counts are
// `cum`: counts[c * stride] = draws of class c (f8).  tile_total: 4096 unsigned ints of scratch.
// false = table too large for the tiled draw.
bool launch_multinomial(const unsigned long long *cum, int64_t n_classes, int64_t n_draws,
                        uint64_t seed, uint64_t stream_id, unsigned int *tile_total, double *counts,
                        int stride, hipStream_t stream);
void launch_u64_to_double(const unsigned long long *in, int64_t n, double *out, hipStream_t stream);
void launch_double_to_u64(const double *in, int64_t n, unsigned long long *out, hipStream_t stream);

// ---- gene-level tables (skm_genes.hip)
// out[r][g] (r < n_rows <= 65535) = the sum of values[r][gene_tx[j]] for j = gene_off[g] .. gene_off[g + 1] - 1 in
// that order, from +0.0: with gene_tx the transcripts by gene, ascending inside a gene, numpy.add.at bit for bit
void launch_gene_sums(const double *values, int64_t n_rows, int64_t n_tx, const int64_t *gene_off,
                      const int32_t *gene_tx, int64_t n_genes, double *out, hipStream_t stream);
struct GeneClasses {              // a class table in HBM: a CSR (len = nullptr) or what class_compact leaves
    int64_t n_classes;
    const int64_t *start;         // [C]; [C + 1] offsets when len is nullptr
    const int64_t *len;           // [C] or nullptr
    const double *count_f64;      // [C] integers held as doubles, or nullptr: then count_i64
    const int64_t *count_i64;
    const int32_t *sample;        // [C] or nullptr: every class belongs to sample 0
    const int32_t *ids;           // unsigned transcript ids, tuple order
};
// for the classes of the samples sample_first <= s < sample_end: unique[s - sample_first][g] += count where every id
// of the class has tx_gene == g >= 0, other[s - sample_first][1] += count where every id has tx_gene == -1,
// other[s - sample_first][0] += count otherwise (both zeroed by the caller).  tx_gene[n_tx] holds -1 .. n_genes - 1
// (the caller has checked); an id not below n_tx sets *error = SKM_ERR_ARG and indexes nothing.
void launch_gene_unique(const GeneClasses &t, const int32_t *tx_gene, int64_t n_tx, int64_t n_genes, int64_t sample_first,
                        int64_t sample_end, unsigned long long *unique, unsigned long long *other, int *error,
                        hipStream_t stream);

// ---- count matrix (skm_gene_matrix.hip; DESIGN.md section 4, "Count matrix"): the same rule as a CSR over samples
// keys[c] = sample << 32 | gene for a class inside one named gene with a count > 0, n_samples << 32 for every other
// class (one of a sample outside [0, n_samples) among them); vals[c] = c; other[n_samples][2] (zeroed by the caller)
// as launch_gene_unique leaves it; *error as there.  n_classes < 2^32, n_samples <= 2^31 - 2 (the caller has checked).
void launch_gene_matrix_keys(const GeneClasses &t, const int32_t *tx_gene, int64_t n_tx, int64_t n_samples,
                             unsigned long long *keys, int32_t *vals, unsigned long long *other, int *error, hipStream_t stream);
// heads[i] = 1 where sorted key i is a (sample, gene) key that differs from key i - 1, else 0
void launch_gene_matrix_heads(const unsigned long long *keys, int64_t n, int64_t n_samples, int64_t *heads, hipStream_t stream);
// keys / vals sorted, runs[n + 1] the exclusive scan of heads with its total nnz -> indptr[n_samples + 1], indices[nnz],
// data[nnz] (zeroed by the caller; counts taken from t by vals).  n > 0.
void launch_gene_matrix_fill(const GeneClasses &t, const unsigned long long *keys, const int32_t *vals, const int64_t *runs,
                             int64_t n, int64_t n_samples, int64_t *indptr, int32_t *indices, unsigned long long *data,
                             hipStream_t stream);

// ---- cell barcodes (skm_barcodes.hip; DESIGN.md section 4, "Cell barcodes")
// The stable radix sort of skm_quant_setup.hip for (uint32 key, int32 value) pairs, in max(1, ceil(end_bit / 9))
// whole 9-bit passes (the order is by the key bits those passes cover; keys below 2^end_bit: by the key):
// 0 = done (the stream has drained), < 0 = no memory or n >= 2^32 (quant_setup_failure() says which).
int sort_pairs_u32(const uint32_t *keys_in, uint32_t *keys_out, const int32_t *vals_in, int32_t *vals_out, int64_t n,
                   int end_bit, hipStream_t stream);
// Its other two instantiations in use (non-negative int32 keys), and the exclusive scan of the same file -- out[0 .. n)
// the prefix sums of in[0 .. n), out[n] the total, in == out allowed -- for skm_device_sort_probe and
// skm_device_scan_probe (diagnostics, tests).  Same results; the stream has drained on return.
int sort_pairs_u64(const unsigned long long *keys_in, unsigned long long *keys_out, const int32_t *vals_in,
                   int32_t *vals_out, int64_t n, int end_bit, hipStream_t stream);
int sort_pairs_i32(const int32_t *keys_in, int32_t *keys_out, const int32_t *vals_in, int32_t *vals_out, int64_t n,
                   int end_bit, hipStream_t stream);
int exclusive_scan_total_i64(const int64_t *in, int64_t *out, int64_t n, hipStream_t stream);
constexpr int BARCODE_LDS_MAX_ENTRIES = 1024;     // whitelists up to this size are probed from a copy in LDS
constexpr int BARCODE_STATS = 5;                  // exact, corrected, ambiguous, no match, short or unreadable
struct BarcodeTable {             // the whitelist in HBM: open addressing, linear probing, at most half full
    const uint64_t *keys;         // [slots] the 2 L code bits of an entry (first base in the top bits of the 2 L)
    const int32_t *cells;         // [slots] its cell index, -1 = empty slot
    uint32_t slot_bits;           // slots = 1 << slot_bits
    int32_t length;               // L, 1 .. 32
    int64_t n_entries;
};
inline __host__ __device__ uint32_t barcode_slot(uint64_t key, uint32_t slot_bits)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ULL) >> 32) >> (32 - slot_bits);       // slot_bits >= 1
}
// candidate j of a window: with a non-clean position (bad != 0) base j of 4 there, else substitution j of 3 L
__device__ inline uint64_t barcode_candidate(uint64_t key, uint32_t bad, int length, int j)
{
    if (bad) {
        const int shift = 2 * (length - 1 - __clz(bad));
        return (key & ~(3ULL << shift)) | ((uint64_t)j << shift);
    }
    const int shift = 2 * (length - 1 - j / 3);
    const uint64_t base = (key >> shift) & 3;
    return key ^ ((base ^ ((base + 1 + j % 3) & 3)) << shift);
}
struct BarcodeWindows {           // the window words of a piece's reads, compacted: what the assign kernel reads
    int64_t n_reads;
    const uint64_t *codes;        // [n_reads][words] the code words that hold the window (words = 0: no read reaches it)
    int32_t words;                // 0, 1 or 2
    int32_t offset;               // the window starts at base `offset` (0 .. 31) of the first word
    const uint32_t *lengths;      // [n_reads], or nullptr: every read is uniform_len long
    int64_t uniform_len;
    int32_t start;                // the window is bases [start, start + L) of a read
    const uint32_t *clean;        // [n_reads]: bit 31 - i set = window position i is an upper-case ACGT
};
// clean[r] for the n_exceptions reads that have a bit plane (clean[] preset to all ones): masks[e][words] are the
// plane's 32-bit words that hold the window, offset = start % 32; exception_reads[e] < n_reads (the caller has checked)
void launch_barcode_clean(const uint32_t *exception_reads, const uint32_t *masks, int64_t n_exceptions, int words,
                          int offset, uint32_t *clean, hipStream_t stream);
// cell[r] = the cell of read r or -1; cell_units[cell] and stats[BARCODE_STATS] are added to
void launch_barcode_assign(const BarcodeTable &table, const BarcodeWindows &w, int max_mismatches, int32_t *cell,
                           unsigned long long *cell_units, unsigned long long *stats, hipStream_t stream);
// keys[u] = sample[u], or n_samples for a dropped unit (sample[u] < 0); vals[u] = u; a sample >= n_samples sets *error
void launch_group_keys(const int32_t *sample, int64_t n, int64_t n_samples, uint32_t *keys, int32_t *vals, int *error,
                       hipStream_t stream);
// offsets[s] (s <= n_samples) = the first place of the ascending keys[0 .. n) whose key is >= s
void launch_group_offsets(const uint32_t *sorted_keys, int64_t n, int64_t n_samples, int64_t *offsets, hipStream_t stream);

// ---- UMI collapse (skm_umi.hip; DESIGN.md section 4, "UMI collapse")
// umi[r] = the 2 L code bits of bases [w.start, w.start + length) of read r (first base in the top bits of the 2 L used
// bits; 1 <= length <= 16), 0 where the read is too short for the window or holds a position there that is not an
// upper-case ACGT; such a read gets cell[r] = -1 (cell may be nullptr) and adds one to *n_unreadable
void launch_umi_windows(const BarcodeWindows &w, int length, int32_t *cell, uint32_t *umi, unsigned long long *n_unreadable,
                        hipStream_t stream);
struct alignas(32) UmiSlot {      // 32 B: one molecule (sample, class, UMI) of a sample set
    unsigned long long tag;       // umi_tag(class_key, umi); 0 = empty
    unsigned long long class_key; // sample_key(the tuple's key, sample)
    uint32_t umi;
    uint32_t dropped;             // 1: the molecule's first unit was removed for a neighbour (mismatches = 1), so none of its
                                  // units stays; stored by that unit's lane alone, read by the molecule matrix alone
    unsigned long long min_unit;  // the smallest sample-local unit number seen of the molecule (~0: none yet)
};
// the tag of a molecule: a mix of its salted class key and its UMI.  Only where the probe starts and what it compares
// first: resolve compares key and UMI in full.
__host__ __device__ __forceinline__ uint64_t umi_tag(uint64_t class_key, uint32_t umi)
{
    uint64_t h = class_key ^ (((uint64_t)umi + 1) * 0x9E3779B97F4A7C15ULL);
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ULL;
    h ^= h >> 29;
    h *= 0x9E3779B97F4A7C15ULL;
    h ^= h >> 32;
    return h;
}
enum { UMI_CTL_ENTRIES = 0, UMI_CTL_LOST = 1, UMI_CTL_NEAR = 2, UMI_CTL_WORDS = 3 };
struct UmiSet {
    UmiSlot *slots;
    uint64_t slot_mask;           // slots - 1, a power of two of them
    unsigned long long *ctl;      // [UMI_CTL_ENTRIES] molecules in the set, [UMI_CTL_LOST] probes that found the set full,
                                  // [UMI_CTL_NEAR] units removed only because of a neighbour (mismatches = 1)
    int *error;                   // SKM_ERR_* raised by a kernel
};
struct UmiSegment {               // beside SampleSalt's arrays, for the same segments of a launch
    int64_t local_first;          // the sample-local unit number of the segment's first unit
    const uint32_t *umi;          // the UMIs of the segment's units, in unit order
};
void launch_umi_init(const UmiSet &t, hipStream_t stream);
// pass 1 and pass 2 over the records of a launch (after the strand filter, before anything counts); removed[sample]
// += the records that pass 2 made unaligned.  A full set adds to ctl[UMI_CTL_LOST] and changes no record wrongly: what
// it removes had an earlier copy.  mismatches = 1 (UMIs of umi_bases <= 16 bases): pass 2 also removes the first unit
// of a molecule when a molecule of the same class and a UMI one substitution away has an earlier unit, and adds the
// units that only this removed to ctl[UMI_CTL_NEAR]; mismatches = 0 launches the kernel it always has.
void launch_umi_claim(const UmiSet &t, const MapBatch &b, const SampleSalt &salt, const UmiSegment *segs, hipStream_t stream);
void launch_umi_resolve(const UmiSet &t, const MapBatch &b, const SampleSalt &salt, const UmiSegment *segs,
                        unsigned long long *removed, int umi_bases, int mismatches, hipStream_t stream);
// `to` (any slots' contents) becomes a set that holds the molecules of `from`
void launch_umi_rehash(const UmiSet &from, const UmiSet &to, hipStream_t stream);

// ---- molecule matrix (skm_molecules.hip; DESIGN.md section 4, "Molecule matrix"): distinct UMIs per (sample, gene)
// labels[slot] = n_samples << 32 for every slot of the class table (n_slots of them)
void launch_molecule_label_init(unsigned long long *labels, uint64_t n_slots, int64_t n_samples, hipStream_t stream);
// labels[class_list[c]] = sample << 32 | gene for class c of the view `t` (registry order: class c lies in table slot
// class_list[c]) when it lies inside one named gene with a count > 0; other[n_samples][2] (zeroed by the caller) and
// error[0] as launch_gene_matrix_keys leaves *error; a class_list entry not below n_slots sets error[1] = SKM_ERR_STATE
void launch_molecule_labels(const GeneClasses &t, const int64_t *class_list, uint64_t n_slots, const int32_t *tx_gene,
                            int64_t n_tx, int64_t n_samples, unsigned long long *labels, unsigned long long *other,
                            int *error, hipStream_t stream);
// live[i] = 1 where slot i of the molecule set holds a molecule that has a surviving unit (occupied, not dropped)
void launch_molecule_live(const UmiSet &set, int64_t *live, hipStream_t stream);
// place[] the exclusive scan of live[], n its total: the live molecule of slot i becomes molecule place[i] < n -- mol_label[] the label
// of its class's slot in `classes`, mol_umi[] its UMI, mol_number[] = place[i].  A class key that the table does not
// hold sets *error = SKM_ERR_STATE (and the molecule gets the label n_samples << 32).
void launch_molecule_keys(const UmiSet &set, const ClassTable &classes, const unsigned long long *labels,
                          const int64_t *place, int64_t n, int64_t n_samples, unsigned long long *mol_label,
                          unsigned long long *mol_umi, int32_t *mol_number, int *error, hipStream_t stream);
// the same three arrays from triples on the device (sample and gene checked by the caller)
void launch_molecule_triples(const int32_t *sample, const int32_t *gene, const uint32_t *umi, int64_t n,
                             unsigned long long *mol_label, unsigned long long *mol_umi, int32_t *mol_number,
                             hipStream_t stream);
// between the two sorts: label_out[i] = mol_label[order[i]], number_out[i] = i (order: the molecules by UMI)
void launch_molecule_gather(const unsigned long long *mol_label, const int32_t *order, int64_t n,
                            unsigned long long *label_out, int32_t *number_out, hipStream_t stream);
// labels[] sorted, umi_of[at[i]] the UMI of sorted place i (ascending inside a label: the sorts are stable):
// heads[i] = 1 where label i is an entry's label and differs from label i - 1; first[i] = 1 where it is an entry's
// label and (label, UMI) differs from place i - 1's
void launch_molecule_heads(const unsigned long long *labels, const int32_t *at, const unsigned long long *umi_of,
                           int64_t n, int64_t n_samples, int64_t *heads, uint32_t *first, hipStream_t stream);
// launch_gene_matrix_fill with first[] as what a lane adds
void launch_molecule_fill(const unsigned long long *labels, const uint32_t *first, const int64_t *runs, int64_t n,
                          int64_t n_samples, int64_t *indptr, int32_t *indices, unsigned long long *data,
                          hipStream_t stream);

// ---- resolved molecules (skm_molecule_resolve.hip; DESIGN.md section 4, "Resolved molecules"): one gene per (sample, UMI)
// by the intersection of the gene sets of the group's classes
enum { MOLECULE_RESOLVED = 0, MOLECULE_RESCUED = 1, MOLECULE_MULTI = 2, MOLECULE_UNNAMED = 3, MOLECULE_COLLISION = 4,
       MOLECULE_TALLY = 5 };      // the words of a sample's tally; rescued is a part of resolved
// words[class_list[c]] = sample << 32 | c for class c of the view `t` (words[] preset by launch_molecule_label_init); a
// class_list entry not below n_slots or a sample outside [0, n_samples) sets *error = SKM_ERR_STATE
void launch_resolve_class_slots(const GeneClasses &t, const int64_t *class_list, uint64_t n_slots, int64_t n_samples,
                                unsigned long long *words, int *error, hipStream_t stream);
// launch_molecule_keys with those words: mol_key[] = sample << 32 | UMI, mol_class[] the class index in the view,
// mol_number[] = place[i]; a class key that the table does not hold sets *error = SKM_ERR_STATE
void launch_resolve_keys(const UmiSet &set, const ClassTable &classes, const unsigned long long *class_of, const int64_t *place,
                         int64_t n, int64_t n_samples, unsigned long long *mol_key, uint32_t *mol_class, int32_t *mol_number,
                         int *error, hipStream_t stream);
// the same three arrays from molecules (in_class[i], in_umi[i]) on the device, a class's sample from class_sample[]
// (nullptr: 0); in_class within the table (the caller has checked)
void launch_resolve_pairs(const int32_t *class_sample, const int32_t *in_class, const uint32_t *in_umi, int64_t n,
                          unsigned long long *mol_key, uint32_t *mol_class, int32_t *mol_number, hipStream_t stream);
// keys[] sorted with order[] the sort's values: heads[i] = 1 where key i differs from key i - 1 (and for i = 0),
// class_sorted[i] = mol_class[order[i]]
void launch_resolve_heads(const unsigned long long *keys, const int32_t *order, const uint32_t *mol_class, int64_t n,
                          int64_t *heads, uint32_t *class_sorted, hipStream_t stream);
// runs[n + 1] the exclusive scan of heads[] with its total n_groups: per group g (out_label, out_umi, out_number)[g] =
// (sample << 32 | gene when resolved else n_samples << 32, UMI, g) and tally[sample][MOLECULE_TALLY] (zeroed by the
// caller) += 1 by outcome.  error[0] = SKM_ERR_ARG for an id not below n_tx, error[1] = SKM_ERR_STATE for a class index
// not below t.n_classes, a sample not below n_samples or a class of another sample than its molecule's.
void launch_molecule_resolve(const GeneClasses &t, const unsigned long long *keys, const uint32_t *classes, const int64_t *runs,
                             int64_t n, int64_t n_groups, const int32_t *tx_gene, int64_t n_tx, int64_t n_samples,
                             unsigned long long *out_label, unsigned long long *out_umi, int32_t *out_number,
                             unsigned long long *tally, int *error, hipStream_t stream);
// other[s] = { multi-gene + collision, unnamed } of tally[s]
void launch_resolve_other(const unsigned long long *tally, int64_t n_samples, unsigned long long *other, hipStream_t stream);

// ---- distributed molecules (skm_molecule_em.hip; DESIGN.md section 4, "Distributed molecules"): multi-gene groups
// shared out among their genes by an EM per cell
constexpr int GENE_SET_MAX = 16;                  // elements of a set at most; a group with more is wide
constexpr int GENE_EM_LDS_ROWS = 4096;            // rows of a cell whose x lives in LDS (32 KiB)
constexpr double GENE_EM_FLOOR = 0.001;           // molecules: the stopping rule's floor and the matrix's cut
constexpr double GENE_EM_TOL = 0.01;              // the largest relative change at which a cell is done
enum { GENE_EM_RESOLVED = 0, GENE_EM_DISTRIBUTED = 1, GENE_EM_WIDE = 2, GENE_EM_UNNAMED = 3, GENE_EM_COLLISION = 4,
       GENE_EM_ROWS = 5, GENE_EM_STEPS = 6, GENE_EM_CAPPED = 7, GENE_EM_TALLY = 8 };      // the words of a sample's tally
// launch_molecule_resolve's walk with every group's element list: stage[g][GENE_SET_MAX] holds group g's group_len[g]
// elements ascending (-1 as n_genes; 0 elements: wide or collision), group_cell[g] its sample, and
// tally[sample][GENE_EM_TALLY] (zeroed by the caller) += 1 in one of its first five words.  error[] as there.
void launch_molecule_sets(const GeneClasses &t, const unsigned long long *keys, const uint32_t *classes, const int64_t *runs,
                          int64_t n, int64_t n_groups, const int32_t *tx_gene, int64_t n_tx, int64_t n_genes, int64_t n_samples,
                          int32_t *stage, int32_t *group_len, int32_t *group_cell, unsigned long long *tally, int *error,
                          hipStream_t stream);
// per group: its elements, 1 where it is a set (2 elements or more), its elements where it is a set -- to be scanned
void launch_gene_sets_sizes(const int32_t *group_len, int64_t n_groups, int64_t *elements, int64_t *is_set,
                            int64_t *set_elements, hipStream_t stream);
// el_start / set_of / set_place [n_groups + 1]: the scans of those three.  Element e = el_start[g] + k gets el_key[e] =
// cell << 32 | element, el_number[e] = e, el_group[e] = g; set_start[n_sets + 1] the sets' places in the set-major lists.
void launch_gene_sets_elements(const int32_t *stage, const int32_t *group_len, const int32_t *group_cell, int64_t n_groups,
                               const int64_t *el_start, const int64_t *set_of, const int64_t *set_place, int64_t n_elements,
                               int64_t n_sets, unsigned long long *el_key, int32_t *el_number, int32_t *el_group,
                               int64_t *set_start, int *error, hipStream_t stream);
// heads[i] = 1 where sorted key i differs from key i - 1: a row begins
void launch_gene_rows_heads(const unsigned long long *keys, int64_t n, int64_t *heads, hipStream_t stream);
struct GeneRows {                 // what the passes over the sorted elements read and write (n > 0)
    const unsigned long long *keys;                   // [n] cell << 32 | element, sorted
    const int32_t *order;                             // [n] the element's number before the sort
    const int64_t *runs;                              // [n + 1] heads before place i; runs[n] = n_rows
    const int32_t *el_group, *group_len;              // [n], [n_groups]
    const int64_t *el_start, *set_of, *set_start;     // [n_groups + 1] twice, [n_sets + 1]
    int64_t n, n_groups, n_sets, n_rows, n_cells, n_set_elements;
    int64_t *cell_row_start;                          // [n_cells + 1]
    int32_t *row_element;                             // [n_rows]
    unsigned long long *u;                            // [n_rows] zeroed: the lists of one element per row
    int64_t *in_set;                                  // [n] 1 where the element belongs to a set
    int32_t *set_rows;                                // [n_set_elements] set-major: the rows of a set, ascending
    int *error;                                       // [2], as above
};
void launch_gene_rows(const GeneRows &p, hipStream_t stream);
// place[n + 1] the scan of p.in_set: row_set_start[n_rows + 1], row_sets[n_set_elements] (a row's sets, ascending)
void launch_gene_rows_transpose(const GeneRows &p, const int64_t *place, int64_t *row_set_start, int32_t *row_sets,
                                hipStream_t stream);
// sets[s] = tally[s][GENE_EM_DISTRIBUTED]: scanned, a cell's first set
void launch_gene_cell_sets(const unsigned long long *tally, int64_t n_cells, int64_t *sets, hipStream_t stream);
struct GeneEm {                   // the cells of one gene_em_kernel launch, a block each; rows and sets numbered over all cells
    int64_t n_cells, n_rows, n_sets, n_set_elements;
    const int64_t *cell_row_start, *cell_set_start;   // [n_cells + 1]
    const unsigned long long *u;                      // [n_rows]
    const int64_t *set_start;                         // [n_sets + 1]
    const int32_t *set_rows;                          // [n_set_elements] rows of the set's cell, ascending
    const int64_t *row_set_start;                     // [n_rows + 1]
    const int32_t *row_sets;                          // [n_set_elements] sets of the row's cell, ascending
    double *d;                                        // [n_sets]
    double *x;                                        // [n_rows] out
    int64_t *steps, *capped;                          // [n_cells] out
    int64_t max_steps;                                // >= 1
    int64_t lds_rows;                                 // cells of more rows work in x[] itself (<= GENE_EM_LDS_ROWS counts)
    int *error;                                       // [2]: error[1] = SKM_ERR_STATE for a range, row or set out of bounds
};
void launch_gene_em(const GeneEm &p, hipStream_t stream);
// keep[r] = 1 where row r names a gene and x[r] >= GENE_EM_FLOOR
void launch_gene_em_keep(const double *x, const int32_t *row_element, int64_t n_rows, int64_t n_genes, int64_t *keep,
                         hipStream_t stream);
// place[n_rows + 1] the scan of keep[] with its total nnz: indptr[n_cells + 1], indices[nnz], data[nnz]; per cell the
// tally's rows, steps and capped words, to_unnamed (the sink row's x, 0.0 without one) and other = { wide + collision, unnamed }
void launch_gene_em_fill(const double *x, const int32_t *row_element, const int64_t *place, const int64_t *cell_row_start,
                         const int64_t *steps, const int64_t *capped, int64_t n_rows, int64_t nnz, int64_t n_genes,
                         int64_t n_cells, int64_t *indptr, int32_t *indices, double *data, unsigned long long *tally,
                         double *to_unnamed, unsigned long long *other, hipStream_t stream);

// ---- cell discovery (skm_census.hip; DESIGN.md section 4, "Cell discovery")
constexpr unsigned long long CENSUS_EMPTY = ~0ULL;    // the key of an empty slot; its one preimage (32 T) is counted in ctl[]
struct alignas(16) CensusSlot {   // 16 B: one distinct barcode
    unsigned long long key;       // the 2 L code bits, CENSUS_EMPTY = empty
    unsigned long long count;     // the clean windows seen with this key
};
enum { CENSUS_CTL_ENTRIES = 0,    // occupied slots (the sentinel's barcode is not among them)
       CENSUS_CTL_SENTINEL = 1,   // windows whose key is CENSUS_EMPTY: the all-T 32-mer
       CENSUS_CTL_DEFERRED = 2,   // (key, count) pairs a launch could not place: the table was full
       CENSUS_CTL_COUNTED = 3, CENSUS_CTL_SHORT = 4, CENSUS_CTL_UNREADABLE = 5,      // the launch's units by kind
       CENSUS_CTL_WORDS = 8,      // what an add resets and reads back
       CENSUS_CTL_OUT = 6,        // [OUT .. OUT + 2] what the ranking kernels count: compacted entries, candidates, dropped
       CENSUS_CTL_ROOM = 16 };    // words of the block
struct CensusTable {
    CensusSlot *slots;            // [1 << slot_bits] open addressing, linear probing from barcode_slot(key, slot_bits)
    uint32_t slot_bits;           // 1 .. 31
    int32_t length;               // L
    unsigned long long *ctl;      // [CENSUS_CTL_ROOM]
    unsigned long long *deferred; // [deferred_cap][2] key, count of what found the table full (nullptr: only counted)
    int64_t deferred_cap;
};
// every slot empty
void launch_census_init(const CensusTable &t, hipStream_t stream);
// `to` (any slots' contents; room for all of them) becomes a table that holds the entries of `from`
void launch_census_rehash(const CensusTable &from, const CensusTable &to, hipStream_t stream);
// the clean windows of a piece are counted under their keys; ctl[COUNTED, SHORT, UNREADABLE] += the piece's units by
// kind (they add up to w.n_reads), ctl[ENTRIES] += the slots claimed, ctl[SENTINEL] += the all-T 32-mers.  What finds
// the table full is appended to t.deferred and counted in ctl[DEFERRED]
void launch_census_count(const CensusTable &t, const BarcodeWindows &w, hipStream_t stream);
// the n pairs of `pairs` ([n][2] key, count), none with the sentinel's key, are added to the table
void launch_census_replay(const CensusTable &t, const unsigned long long *pairs, int64_t n, hipStream_t stream);
// the occupied slots, and the sentinel's barcode if it was seen, as keys[] / counts[] in any order (room for
// ctl[ENTRIES] + 1), iota[i] = i beside them; ctl[OUT] += their number
void launch_census_compact(const CensusTable &t, unsigned long long *keys, unsigned long long *counts, int32_t *iota,
                           hipStream_t stream);
// word[i] = the 32 bits from `shift` on of (keys or counts)[perm[i]], XOR flip: what one stable sort pass orders by
void launch_census_sort_word(const unsigned long long *values, const int32_t *perm, int64_t n, int shift, uint32_t flip,
                             uint32_t *word, hipStream_t stream);
// out_keys[i] = keys[perm[i]], out_counts[i] = counts[perm[i]] for i < n
void launch_census_gather(const unsigned long long *keys, const unsigned long long *counts, const int32_t *perm, int64_t n,
                          unsigned long long *out_keys, unsigned long long *out_counts, hipStream_t stream);
// counts[] descending: ctl[OUT + 1] = the number of entries with counts[i] >= threshold (written only if there is one)
void launch_census_candidates(const unsigned long long *counts, int64_t n, unsigned long long threshold,
                              unsigned long long *ctl, hipStream_t stream);
// dropped[i] (i < n_candidates, entries in ranked order, all with count >= threshold) = 1 when one of the 3 L single
// substitutions of keys[i] is in the table with count >= threshold and ranks earlier, else 0; ctl[OUT + 2] += the ones
void launch_census_pick(const CensusTable &t, const unsigned long long *keys, const unsigned long long *counts,
                        int64_t n_candidates, unsigned long long threshold, uint32_t *dropped, int32_t *iota,
                        hipStream_t stream);

// one hipFuncGetAttributes per translation unit: its code object is loaded now, not by a sample's first launch
void warm_code_map();
void warm_code_classes();
void warm_code_em();
void warm_code_em_batch();
void warm_code_em_set();
void warm_code_quant_setup();

}  // namespace skm
