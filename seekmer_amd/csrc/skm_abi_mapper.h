// The index and mapper handles of the C ABI glue, for the units that look into them (skm_abi_index.hip, which owns
// the index; skm_abi.hip, which owns the mapper's map/class stage -- everything under `mu`; skm_abi_feed.hip, which
// owns `skm_mapper::feed`, how reads reach that stage -- everything under `feed.q_mu`; skm_abi_samples.hip,
// skm_abi_genes.hip and skm_abi_quant.hip), with the words of the mapper's counter blocks and the calls of the
// mapper that other units make.  The handles are the C ABI's global types and their members are types of `skm` and
// `skm::abi`, so this header names both namespaces as the units that include it do.
#pragma once
#include "skm_abi.h"
#include "skm_bias.h"
#include "skm_packed_book.h"

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace skm;
using namespace skm::abi;

struct skm_index {
    ~skm_index() { (void)hipSetDevice(device); }     // (then the members free the device copy)
    int device = 0;
    DevIndex d{};
    DevMem kmers, contigs, seq2, buckets, edge_kmers, signatures;
    int64_t n_slots = 0, bytes = 0;
    int64_t layout[8] = {0};          // skm_index_layout
    int cu_count = 256;
    // the caller's handle + one per mapper that maps against it: skm_index_destroy only gives up the
    // caller's, the device copy goes with the last one (garbage collectors finalise a mapper and
    // its index in any order; a mapper destroyed after its index used to read freed memory here)
    std::atomic<int> holders{1};
    // ---- the transcript pool of the sequence-bias correction (skm_bias.h), built by
    // skm_index_build_transcripts from the host rows below, which are dropped once it stands (all under pool_mu)
    std::mutex pool_mu;
    std::vector<PoolContig> pool_contigs;
    std::vector<Coord> pool_targets;
    bool pool_built = false;
    TxPool pool{};
    DevMem pool_codes, pool_known, pool_tx_word, pool_tx_len, pool_tx_windows;
    std::vector<int64_t> pool_tx_base;        // [n_tx + 1] first base of every transcript in a download
    std::vector<int32_t> pool_windows;        // [n_tx] n_t, host copy
};

struct skm_mapper {
    explicit skm_mapper(skm_index *index) : ix(index) { index->holders.fetch_add(1); }
    ~skm_mapper();
    Own<skm_index *, skm_index_destroy> ix;   // a hold on the index (declared first: given up last)
    PoolStream stream;
    Event ev[4];
    std::mutex mu;
    // class table
    ClassTable t{};
    DBuf<ClassSlot> slots;
    DBuf<int32_t> arena;
    DBuf<int64_t> class_list;
    DBuf<unsigned long long> counters;   // [0]=arena_cursor [1]=n_classes [2]=n_unaligned [3]=n_units [8..2007]=fld
    DBuf<int> error;
    // batch buffers
    DBuf<uint8_t> bases;
    DBuf<int64_t> offsets;
    DBuf<uint32_t> records;
    DBuf<int32_t> workspace;
    DBuf<int32_t> unit_begin, unit_end, rec_unit;
    DBuf<Coord> unit_anchor;
    DBuf<int64_t> unit_slot;
    DBuf<unsigned long long> rec_tuple;
    HostPinned pinned;                      // host-pinned readback words
    DBuf<uint64_t> rec_key;
    bool keep_spans = false, last_spans = false;   // spans wanted / written by the last batch
    int strand = SKM_STRAND_NONE;                  // skm_mapper_set_strand (under mu)
    bool bias = false;                             // skm_mapper_set_bias (under mu): count the aligned units' first hexamers
    DBuf<unsigned long long> bias_observed;        // [4096], zeroed where the histogram is
    // skm_mapper_set_length_weights (under mu): p[2000] of a fragment-length model; while it is in use the
    // quantification calls take the effective lengths from it and not from the histogram
    DBuf<double> length_weights;
    bool use_length_weights = false;
    DBuf<int32_t> unit_entries;
    DBuf<unsigned long long> batch_ctl;  // [0]=ids_cursor [8..2007]=fld [2048..2063]=stats
    int grid_blocks = 0;
    // (both under mu)
    int64_t expected_units = 0;       // skm_mapper_expect_units: the sample's size, announced before its reads
    bool packed_sized = false;        // the batch buffers hold a run of PACKED_MAX_UNITS already
    int64_t units_done = 0;
    int64_t first_seen_bound = 0;     // every first_seen in the table is below this
    int64_t last_units = 0, last_ids = 0;
    int64_t last_reads = 0;           // skm_mapper_copy_records: the records of the last batch ...
    int last_words = 0, last_record_words = 0;   // ... W and u32 words per record
    int64_t host_classes = 0, host_arena_used = 0;
    // the table's unit totals as the last mapped batch read them back (valid: nothing else -- a merge
    // of a foreign table -- has changed the device counters since): spares skm_quant_infer a
    // synchronous read of two words
    bool host_totals_valid = false;
    unsigned long long host_units = 0, host_unaligned = 0;
    int want_stats = 0;               // 0 production, 1 counting build, 2 census build
    double t_pack_ns = 0, t_map_ns = 0, t_class_ns = 0, batches = 0;
    double t_em_ns = 0, em_iters = 0;          // skm_quant_infer calls on this mapper
    bool test_class_slots = false;             // SKM_TEST_CLASS_SLOTS: table_reserve[_for_sample] leave the slot count alone
    int64_t deferred_grows = 0;                // table_grow calls with units in flight (after a pass that deferred units)
    int test_map_blocks = 0;                   // SKM_TEST_MAP_BLOCKS: a cap on the map kernel's grid (0: none)
    int test_map_layout = 0;                   // SKM_TEST_MAP_LAYOUT: MAP_LAYOUT_WIDE / _PACKED instead of map_geometry's choice
    int last_map_packed = -1, last_map_contexts = 0;   // skm_mapper_map_layout: the kernel of the last launch (-1: none yet)
    int64_t map_relaunches = 0;                // map kernel launches repeated because the entry arena overflowed
    unsigned long long stats_total[48] = {0};
    // ---- host batches: staging lanes + one worker (skm_mapper_map_batch[_async])
    // A host batch is copied to HBM on a lane's own stream by the thread that submits it (the
    // copy of batch i+1 runs under the kernels of batch i) and then queued; the worker maps
    // the queued batches in submission order on the mapper's stream, holding `mu` only for its
    // batch.  Every call that reads or changes the table first waits for the queue to drain.
    struct Lane {
        DBuf<uint8_t> bases;
        DBuf<int64_t> offsets;
        Stream stream;
        bool busy = false;
    };
    static constexpr int N_LANES = 3;
    struct Job { int lane; int64_t n_units; int paired; int64_t offset_base; int64_t first_unit; uint64_t ticket; };
    // The feed (skm_abi_feed.hip): everything in it but `scan_out` (the worker's, used under `mu`) is under q_mu.
    struct __attribute__((visibility("hidden"))) Feed {
        Lane lanes[N_LANES];
        std::mutex q_mu;
        std::condition_variable q_cv;             // job queued / stop
        std::condition_variable done_cv;          // job finished, lane released
        std::deque<Job> jobs;
        std::thread worker;
        bool worker_started = false, stop = false;
        uint64_t next_ticket = 1, done_ticket = 0;
        int job_error = SKM_OK;                   // first failure of a queued batch (sticky until reported)
        uint64_t job_error_ticket = 0;
        std::string job_error_msg;
        DBuf<unsigned long long> scan_out;        // device-side max read length / monotonicity of a batch
        // ---- packed pieces (skm_mapper_push_packed): reads that arrive as 2-bit code words wait in HBM,
        // one ascending list of pieces per stream, until the worker maps a run of units that every
        // stream covers (skm_packed_book.h).
        PackedBook book;
        Stream packed_stream;
        int packed_flush = 0;                     // callers waiting for everything mappable to be mapped
        int packed_waiters = 0;                   // pushers held back by the byte limit: whatever run there is gets mapped
        int64_t packed_max_pending = 8LL << 30;   // bytes of HBM that pieces may hold before a pusher waits
        bool packed_busy = false;
        // HBM held by pieces that wait to be mapped; a pusher that is ahead of the GPU by more than
        // PACKED_MAX_PENDING bytes waits (only while the worker has something to map: a caller that
        // pushes one stream long before the other is never blocked on itself)
        std::shared_ptr<std::atomic<int64_t>> packed_bytes = std::make_shared<std::atomic<int64_t>>(0);
        // (q_mu held) the first failure of a queued batch or run sticks; ticket 0: every wait reports it
        void record_failure(int rc, uint64_t ticket, const std::string &message);
        void shutdown();                          // stop the worker once it has finished what is queued, and join it
    } feed;
    int vote[8] = {1, 1, 1, 1, 1, 1, 1, 0};   // quorum per action (start, lookup, merge, left, right, emit, scan)
    // skm_mapper_device_table: the classes in registry order, as class_compact leaves them
    DBuf<int64_t> view_start, view_len;
    DBuf<double> view_count;
    DBuf<unsigned long long> view_first_seen;
};

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// words of skm_mapper::counters (CTR_*) and skm_mapper::batch_ctl (BC_*)
constexpr int CTR_ARENA = 0, CTR_CLASSES = 1, CTR_UNALIGNED = 2, CTR_UNITS = 3, CTR_LISTED = 4,
              CTR_DEFERRED = 5, CTR_COMMITTED = 6, CTR_FLD = 8;
constexpr int CTR_WORDS = 8 + MAX_FRAGMENT_LENGTH;
constexpr int BC_IDS = 0, BC_FLD = 8, BC_STATS = 2048, BC_WORDS = 2096;

// (skm_abi_feed.hip) wait until every queued batch up to `ticket` (0: all of them) has been mapped; reports (and,
// with `consume`, forgets) the first failure among them
int wait_jobs(skm_mapper *m, uint64_t ticket, bool consume);
// (skm_abi.hip) the weights of a fragment-length model: every one finite and >= 0
bool length_weights_valid(const double *p, int64_t count);
// (skm_abi.hip, m->mu held) what skm_mapper_expect_units announced: table and arena sized for the sample at once
int table_reserve_for_sample(skm_mapper *m, int64_t sample_units);

// ---- what the feed and a sample set, which drives its mapper's launches itself, use of the mapper
// map_batch_resident (skm_abi.hip, m->mu held) -- first_unit: global index of the batch's first unit (first-seen values count from it), or -1
// to continue after the units mapped so far
// fill_records: what makes the read records of the batch (records, words per read, u32 words per
// record); nullptr = pack_reads_kernel over ASCII bases + offsets
// salt: the batch is a launch of a sample set -- the segments whose samples go into the records' keys
// before class counting (skm_samples.hip); nullptr = one sample, keys as the map kernel made them
// collapse: a sample set that keeps UMIs -- what removes the duplicate units' records (skm_umi.hip) once the map
// attempt that stood and the strand filter have run, before anything counts; nullptr = nothing is launched
typedef std::function<int(uint32_t *, int, int)> RecordStage;
typedef std::function<int(const MapBatch &)> BatchStage;
int map_batch_resident(skm_mapper *m, const uint8_t *d_bases, const int64_t *d_offsets,
                       int64_t n_units, int paired, int max_len, int64_t first_unit = -1,
                       const RecordStage *fill_records = nullptr, const SampleSalt *salt = nullptr,
                       unsigned long long *sample_bias_rows = nullptr, const BatchStage *collapse = nullptr);

// ---- what a sample set uses of the feed (all defined in skm_abi_feed.hip)
// the read records of a launch's packed segments (`first_unit`: the unit that stands at record 0)
void packed_unpack(const std::vector<PackedSegment> &segments, int64_t first_unit, int mates, uint32_t *records, int words,
                   int record_words, int *error, hipStream_t stream);
// the arrays of a piece that holds reads
int packed_check_arrays(const skm_packed_reads *piece);
inline size_t packed_round(size_t b) { return (b + 255) & ~(size_t)255; }
// `bytes` of HBM from the pool, counted in *counter while the block lives
int packed_block(int64_t bytes, const std::shared_ptr<std::atomic<int64_t>> &counter, std::shared_ptr<char> *block);
// take the block (counted in *counter while it lives) and QUEUE the copies of the piece's arrays on `stream`
int packed_upload(const skm_packed_reads *piece, const std::shared_ptr<std::atomic<int64_t>> &counter, hipStream_t stream,
                  PackedPiece *out);

}  // namespace abi
}  // namespace skm
