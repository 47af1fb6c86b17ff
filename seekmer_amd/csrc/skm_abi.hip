// C ABI of libseekmer_hip.so (declared in include/seekmer_hip.h): handle
// management, HBM buffers, stream/event plumbing and the launch sequences.
// No torch types, no exceptions across the boundary.
#include "skm_abi.h"
#include "skm_bias.h"
#include "skm_bias_weights.h"

#include <dlfcn.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <atomic>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <unordered_map>
#include <mutex>
#include <thread>
#include <numeric>
#include <string>
#include <utility>
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
    Lane lanes[N_LANES];
    struct Job { int lane; int64_t n_units; int paired; int64_t offset_base; int64_t first_unit; uint64_t ticket; };
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
    // stream covers.  All of it under q_mu.
    struct Piece {
        int64_t first = 0, n = 0;             // units [first, first + n) of the stream (what is left of the piece)
        int64_t origin = 0;                   // first_read of the piece as pushed: the arrays start there
        int cw = 1;
        int64_t uniform_len = -1;
        std::shared_ptr<char> block;          // one HBM allocation: codes | lengths | exception reads | masks
        uint64_t *codes = nullptr;            // [n as pushed][cw]
        uint32_t *lengths = nullptr;          // or NULL (uniform_len)
        uint32_t *exc_reads_dev = nullptr, *exc_masks = nullptr;
        std::vector<uint32_t> exc_reads;      // host copy (indices relative to origin), for cutting runs
        bool in_job = false;
    };
    std::deque<Piece> pending[2];
    Stream packed_stream;
    int packed_paired = -1;                   // -1 until the first piece
    int packed_flush = 0;                     // callers waiting for everything mappable to be mapped
    int packed_waiters = 0;                   // pushers held back by the byte limit: whatever run there is gets mapped
    int64_t packed_max_pending = 8LL << 30;   // bytes of HBM that pieces may hold before a pusher waits
    bool packed_busy = false;
    int64_t packed_dropped = 0;               // reads that never got a mate
    // HBM held by pieces that wait to be mapped; a pusher that is ahead of the GPU by more than
    // PACKED_MAX_PENDING bytes waits (only while the worker has something to map: a caller that
    // pushes one stream long before the other is never blocked on itself)
    std::shared_ptr<std::atomic<int64_t>> packed_bytes = std::make_shared<std::atomic<int64_t>>(0);
    int vote[8] = {1, 1, 1, 1, 1, 1, 1, 0};   // quorum per action (start, lookup, merge, left, right, emit, scan)
    // skm_mapper_device_table: the classes in registry order, as class_compact leaves them
    DBuf<int64_t> view_start, view_len;
    DBuf<double> view_count;
    DBuf<unsigned long long> view_first_seen;
};

struct skm_quant {
    ~skm_quant()                              // (the buffers go once the stream has drained)
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
    int device = 0;
    PoolStream stream;
    PoolTimingEvent ev[2];
    PoolEvent chunk_ev[2];
    PoolPinned pinned;                        // host-pinned readback of the control block
    std::mutex mu;
    int64_t n_tx = 0, n_classes = 0, n_ids = 0, n_rows = 0;
    DBuf<int64_t> cls_offset, row_start, tx_row;
    DBuf<int32_t> ids, tx_cls, row_tx, perm;      // perm[k] = caller's index of internal class k
    DBuf<double> cls_count, cls_count_saved, inner, row_sum;
    DBuf<double> eff_len, x0, x1, acc, part_max;
    DBuf<unsigned int> part_flags, arrivals;
    DBuf<unsigned long long> ctl, cum;
    DBuf<unsigned int> tile_total;            // scratch of the tiled multinomial draw
    DBuf<double> x_start, boot_out;           // bootstrap: the common start vector, the replicates' results
    // working set of the batched EM (skm_em_batch.hip): eight problems of this class structure side by side
    struct Batch {
        DBuf<double> cls_count, inner, row_sum, x0, x1, part_max;
        DBuf<unsigned int> part_flags;
        DBuf<unsigned long long> ctl, mgr;
        DBuf<double> counts_all;              // [group][C] class counts of a group of problems (internal class order)
        DBuf<double> totals;                  // [group][2] their sums (pairs, as launch_np_sum_many leaves them)
        DBuf<int64_t> iters;                  // [group] their step counts
    } batch;
    // the component tiles of the class table (EmTiles, skm_kernels.h): built with the class views
    struct Tiles {
        DBuf<int64_t> tile_tx, tile_cls, cls_pair, tx_pair;
        DBuf<int32_t> tx_list, cls_list, tx_label, tx_tile, cls_tile;
        DBuf<int32_t> order;                  // [T + 1] the tiles by descending pair count: the launch order
        DBuf<uint16_t> cls_tx, tx_cls;
        DBuf<double> snap, step_max;          // snap: [EM_CHUNK_MAX][T] every step's abundances of the chunk in flight
        DBuf<unsigned int> step_flags;
        // the components above the capacity as an EM problem beside the tiles (QuantResidual)
        struct Residual {
            int64_t n_classes = 0, n_ids = 0, n_rows = 0;
            DBuf<int64_t> cls_offset, row_start, tx_row;
            DBuf<int32_t> ids, cls_src, row_tx, tx_cls;
            DBuf<double> cls_count, inner, row_sum;
            bool built = false;
        } residual;
        bool built = false;                   // the set-up has run
        int64_t n_tiles = 0, n_oversize = 0;  // n_oversize: components above the tile capacity (then the tiles are not used)
    } tiles;
    double n_total = 0;
    bool n_total_reduced = false;             // n_total already is the sum over all ranks
    // RCCL communicator (borrowed from an skm_comm), loaded lazily
    void *comm = nullptr;
    int rank = 0, world = 1;
    double t_em_ns = 0, iters_total = 0, launches = 0;
};

struct skm_comm {
    int device = 0;
    void *comm = nullptr;
    int rank = 0, world = 1;
};

// -------------------------------------------------------------------- index
extern "C" int skm_index_create(const void *kmers, int64_t n_slots, const void *contigs,
                                int64_t n_contigs, const char *sequences, int64_t n_bases,
                                const void *targets, int64_t n_targets, int device,
                                skm_index **out)
{
    if (!kmers || !contigs || !sequences || !targets || !out)
        return fail(SKM_ERR_ARG, "NULL array");
    if (n_slots <= 0 || (n_slots & (n_slots - 1)) || n_slots > (1LL << 31))
        return fail(SKM_ERR_ARG, "k-mer table size %lld is not a power of two <= 2^31", (long long)n_slots);
    if (n_contigs <= 0 || n_bases < ALIGN_LENGTH || n_targets < 0 || n_bases >= (1LL << 31)
            || n_targets + 32 * n_contigs >= (1LL << 30) || n_contigs >= (1LL << 25))
        return fail(SKM_ERR_ARG, "bad index sizes");
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    SKM_TRY(set_device(device));
    // Under the validation and the upload below, a helper loads the library's code objects and
    // parks two streams (hipStreamCreate: > 100 ms apiece, measured) for the handles of the first sample:
    // first-use costs of the GPU side that would otherwise fall into the sample's own run.
    std::thread warm([device]() {
        if (hipSetDevice(device) != hipSuccess) return;
        warm_code_map(); warm_code_classes(); warm_code_em(); warm_code_em_batch(); warm_code_em_set(); warm_code_quant_setup();
        static std::once_flag streams_once;
        std::call_once(streams_once, []() {
            hipStream_t a = nullptr, b = nullptr;
            if (pool_stream_acquire(&a) == hipSuccess && pool_stream_acquire(&b) == hipSuccess) {
                pool_stream_release(a);
                pool_stream_release(b);
            }
            void *block[2] = {nullptr, nullptr};           // (and the control-block readbacks of two handles)
            for (auto &p : block) if (pool_pinned_acquire(&p) != hipSuccess) p = nullptr;
            for (auto &p : block) pool_pinned_release(p);
        });
    });
    auto join_warm = on_exit([&]() { warm.join(); });

    // host-side validation: every shape the kernels index with must be in range
    const ContigEntry *hc = (const ContigEntry *)contigs;
    int64_t max_tc = 0;
    bool edge_windows = true;       // first_kmer / last_kmer spell the contig's first / last k bases
    auto encode = [&](int64_t at) {                      // _kmer.pxd:46-68 over the pooled bases
        uint64_t k = 0;
        for (int i = 0; i < K; ++i) {
            const unsigned ch = (unsigned char)sequences[at + i] & 0xDFu;
            k = (k << 2) | (ch == 'T' ? 3u : ch == 'G' ? 2u : ch == 'C' ? 1u : 0u);
        }
        return k;
    };
    for (int64_t c = 0; c < n_contigs; ++c) {
        if (hc[c].offset < 0 || hc[c].length < 0 || hc[c].offset + hc[c].length > n_bases
                || hc[c].target_offset < 0 || hc[c].target_length < 0
                || hc[c].target_offset + hc[c].target_length > n_targets)
            return fail(SKM_ERR_ARG, "contig %lld points outside the pooled arrays", (long long)c);
        max_tc = std::max<int64_t>(max_tc, hc[c].target_length);
        if (edge_windows && (hc[c].length < K || encode(hc[c].offset) != hc[c].first_kmer
                             || encode(hc[c].offset + hc[c].length - K) != hc[c].last_kmer))
            edge_windows = false;
    }
    bool sorted_targets = true;      // (the builder sorts (contig, entry, offset), _index_builder.pyx)
    {
        const Coord *ht = (const Coord *)targets;
        for (int64_t c = 0; c < n_contigs && sorted_targets; ++c) {
            const int64_t first = hc[c].target_offset, end = first + hc[c].target_length;
            for (int64_t t = first + 1; t < end; ++t)
                if (ht[t - 1].entry > ht[t].entry) { sorted_targets = false; break; }
        }
    }
    if (max_tc >= (1LL << 22))
        return fail(SKM_ERR_ARG, "a contig lists %lld targets (limit 4194303)", (long long)max_tc);
    const IndexEntry *hk = (const IndexEntry *)kmers;
    // (2 GiB of slots at 190k transcripts: checked by all host cores)
    const int n_workers = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<unsigned>(
                              std::max(1u, std::thread::hardware_concurrency()), 16u), n_slots >> 20));
    std::vector<int64_t> empty_part((size_t)n_workers, 0), bad_part((size_t)n_workers, -1);
    {
        std::vector<std::thread> workers;
        for (int w = 0; w < n_workers; ++w)
            workers.emplace_back([&, w]() {
                const int64_t first = n_slots * w / n_workers, last = n_slots * (w + 1) / n_workers;
                int64_t empty = 0;
                for (int64_t i = first; i < last; ++i) {
                    if (hk[i].kmer == KMER_INVALID) { ++empty; continue; }
                    const int32_t e = hk[i].pos.entry < 0 ? ~hk[i].pos.entry : hk[i].pos.entry;
                    if (hk[i].pos.offset >= 0
                            && (e < 0 || e >= n_contigs || hk[i].pos.offset + K > hc[e].length)) {
                        bad_part[(size_t)w] = i;
                        break;
                    }
                }
                empty_part[(size_t)w] = empty;
            });
        for (auto &t : workers) t.join();
    }
    int64_t empty = 0;
    for (int w = 0; w < n_workers; ++w) {
        if (bad_part[(size_t)w] >= 0)
            return fail(SKM_ERR_ARG, "k-mer slot %lld points outside its contig", (long long)bad_part[(size_t)w]);
        empty += empty_part[(size_t)w];
    }
    if (empty == 0) return fail(SKM_ERR_ARG, "k-mer table has no empty slot");

    std::unique_ptr<skm_index> ix(new skm_index());  // (any early return below: nothing is left behind)
    ix->device = device;
    DevMem d_ascii;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    ix->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const int64_t n_words = (n_bases + 31) / 32 + 1;
    HIP_TRY(hipMalloc(ix->kmers.out(), (size_t)n_slots * sizeof(IndexEntry)));
    HIP_TRY(hipMalloc(ix->seq2.out(), (size_t)n_words * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(d_ascii.out(), (size_t)n_bases));
    HIP_TRY(hipMemcpy(ix->kmers, kmers, (size_t)n_slots * sizeof(IndexEntry), hipMemcpyHostToDevice));
    int64_t n_overflow = 0;
    {   // contig records (skm_device.h: DevContig) and, behind them in the same allocation, the target
        // slices that do not fit a side; of every target only the signed entry is kept
        std::vector<DevContig> rows((size_t)n_contigs);
        std::vector<uint64_t> edges((size_t)n_contigs * 2);
        std::vector<int32_t> overflow;
        const Coord *ht = (const Coord *)targets;
        const int64_t row_words = (int64_t)sizeof(DevContig) / 4;      // (int32 words per record)
        for (int64_t c = 0; c < n_contigs; ++c) {
            DevContig &d = rows[(size_t)c];
            memset(&d, 0, sizeof(d));
            edges[(size_t)(2 * c)] = hc[c].first_kmer;
            edges[(size_t)(2 * c + 1)] = hc[c].last_kmer;
            const int64_t first = hc[c].target_offset, count = hc[c].target_length;
            const int64_t place = n_contigs * row_words + (int64_t)overflow.size();
            for (int s = 0; s < 2; ++s) {
                DevSide &side = d.side[s];
                side.offset = (int32_t)hc[c].offset;
                side.length = (int32_t)hc[c].length;
                // [0] the contig's last 8 bases (low bits of last_kmer), [1] its first 8 (top of first_kmer)
                const uint32_t edge8 = s == 0 ? (uint32_t)(hc[c].last_kmer & 0xffffu)
                                              : (uint32_t)(hc[c].first_kmer >> (2 * K - 16)) & 0xffffu;
                side.count_edge = ((uint32_t)std::min<int64_t>(count, 0xffff) << 16) | edge8;
                if (count <= CONTIG_INLINE_TARGETS) {
                    for (int64_t i = 0; i < count; ++i) side.targets[i] = ht[first + i].entry;
                } else {
                    side.targets[0] = (int32_t)place;
                    side.targets[1] = (int32_t)count;
                }
            }
            if (count > CONTIG_INLINE_TARGETS)
                for (int64_t i = 0; i < count; ++i) overflow.push_back(ht[first + i].entry);
        }
        n_overflow = (int64_t)overflow.size();
        const size_t row_bytes = (size_t)n_contigs * sizeof(DevContig);
        HIP_TRY(hipMalloc(ix->contigs.out(), row_bytes + (size_t)(n_overflow + 16) * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(ix->contigs, rows.data(), row_bytes, hipMemcpyHostToDevice));
        if (n_overflow)
            HIP_TRY(hipMemcpy((char *)ix->contigs.get() + row_bytes, overflow.data(), (size_t)n_overflow * sizeof(int32_t),
                              hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(ix->edge_kmers.out(), (edges.size() + 2) * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(ix->edge_kmers, edges.data(), edges.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(d_ascii, sequences, (size_t)n_bases, hipMemcpyHostToDevice));
    launch_pack_sequences((const char *)d_ascii.get(), n_bases, (uint64_t *)ix->seq2.get(), n_words, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    d_ascii.reset();
    ix->n_slots = n_slots;
    ix->d.kmers = (const IndexEntry *)ix->kmers.get();
    ix->d.slot_mask = (uint32_t)(n_slots - 1);
    ix->d.contigs = (const DevContig *)ix->contigs.get();
    ix->d.n_contigs = n_contigs;
    ix->d.seq2 = (const uint64_t *)ix->seq2.get();
    ix->d.n_bases = n_bases;
    ix->d.targets = (const int32_t *)ix->contigs.get();       // (rows and overflow slices as one int32 array)
    ix->d.edge_kmers = (const uint64_t *)ix->edge_kmers.get();
    ix->d.n_targets = n_targets;
    ix->d.max_target_count = (int32_t)std::max<int64_t>(max_tc, 1);
    ix->d.edge_windows = edge_windows ? 1 : 0;
    ix->d.sorted_targets = sorted_targets ? 1 : 0;
    ix->bytes = n_slots * (int64_t)sizeof(IndexEntry) + n_contigs * (int64_t)sizeof(DevContig)
                + n_overflow * (int64_t)sizeof(int32_t) + n_words * 8 + n_contigs * 16;
    {   // the same set of k-mers by bucket (skm_device.h: DevBucket): about one k-mer per bucket
        const int64_t occupied = n_slots - empty;
        uint64_t n_buckets = 16;
        while ((int64_t)n_buckets < occupied) n_buckets <<= 1;
        int log2_buckets = 0;
        while ((1ULL << log2_buckets) < n_buckets) ++log2_buckets;
        unsigned long long report[4] = {0, 0, 0, 0};
        const char *off = getenv("SKM_NO_BUCKETS");          // tuning aid: probe the reference's layout
        if (!(off && off[0] == '1') && n_buckets <= (1ULL << 31)) {
            DevMem d_report;
            HIP_TRY(hipMalloc(ix->buckets.out(), (size_t)n_buckets * sizeof(DevBucket)));
            HIP_TRY(hipMalloc(d_report.out(), sizeof(report)));
            HIP_TRY(hipMemset(d_report, 0, sizeof(report)));
            launch_bucket_build(ix->d, (uint64_t)n_slots, (DevBucket *)ix->buckets.get(), (uint32_t)(n_buckets - 1),
                                (uint32_t)(32 - log2_buckets), (unsigned long long *)d_report.get(), nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(report, d_report, sizeof(report), hipMemcpyDeviceToHost));
            ix->layout[1] = (int64_t)n_buckets;
            ix->layout[2] = (int64_t)report[0];
            ix->layout[3] = (int64_t)report[1];
            ix->layout[4] = (int64_t)report[2];
            ix->layout[5] = (int64_t)report[3];
            if ((int64_t)report[0] == occupied && report[2] == 0 && report[3] == 0) {
                ix->d.buckets = (const DevBucket *)ix->buckets.get();
                ix->d.bucket_mask = (uint32_t)(n_buckets - 1);
                ix->d.bucket_shift = (uint32_t)(32 - log2_buckets);
                ix->bytes += (int64_t)n_buckets * (int64_t)sizeof(DevBucket);
                ix->layout[0] = 1;
                const char *no_sig = getenv("SKM_NO_SIGNATURES");        // tuning aid: the roll asks the buckets straight away
                // signatures of the k-mers by minimizer (skm_device.h: kmer_min_hash): a slot per four k-mers
                int sig_bits = 10;
                while (sig_bits < 30 && (4LL << sig_bits) < occupied) ++sig_bits;
                const size_t sig_bytes = 2 * sizeof(uint64_t) << sig_bits;
                void *sig = nullptr;
                if (!(no_sig && no_sig[0] == '1') && hipMalloc(&sig, sig_bytes) != hipSuccess) {
                    (void)hipGetLastError();                   // (no room: the roll asks the buckets, as without them)
                    sig = nullptr;
                }
                ix->signatures.reset(sig);
                if (ix->signatures) {
                    HIP_TRY(hipMemset(ix->signatures, 0, sig_bytes));
                    launch_signature_build((const DevBucket *)ix->buckets.get(), n_buckets, (uint64_t *)ix->signatures.get(),
                                           (uint32_t)(32 - sig_bits), nullptr);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipDeviceSynchronize());
                    if (getenv("SKM_TRACE_SIGNATURES")) {       // tuning aid: how full the signatures are
                        std::vector<uint64_t> head(std::min<size_t>((size_t)1 << 20, sig_bytes / 8));
                        HIP_TRY(hipMemcpy(head.data(), ix->signatures, head.size() * 8, hipMemcpyDeviceToHost));
                        int64_t bits = 0, used = 0, full = 0;
                        for (size_t k = 0; k + 1 < head.size(); k += 2) {
                            const int c = __builtin_popcountll(head[k]) + __builtin_popcountll(head[k + 1]);
                            bits += c; used += c != 0; full += c == 128;
                        }
                        fprintf(stderr, "[skm_index_create] signatures: 2^%d slots of 128 bits; of the first %zu: %.2f bits set per slot, "
                                "%.1f %% in use, %lld full\n", sig_bits, head.size() / 2, 2.0 * (double)bits / (double)head.size(),
                                200.0 * (double)used / (double)head.size(), (long long)full);
                    }
                    ix->d.signatures = (const uint64_t *)ix->signatures.get();
                    ix->d.signature_shift = (uint32_t)(32 - sig_bits);
                    ix->bytes += (int64_t)sig_bytes;
                    ix->layout[7] = (int64_t)1 << sig_bits;
                }
                const char *no_succ = getenv("SKM_NO_SUCCESSORS");     // tuning aid: every junction k-mer looked up
                if (!(no_succ && no_succ[0] == '1')) {
                    // junction successors of every contig record (skm_device.h: DevContig), by the
                    // lookup the kernels would do.  SKM_TEST_SUCC_LOOKUP=1 (test hook) marks them all
                    // "look it up", so that every hop takes the fall-back a real index hardly ever needs.
                    const char *force = getenv("SKM_TEST_SUCC_LOOKUP");
                    launch_successor_build(ix->d, (DevContig *)ix->contigs.get(), n_contigs, force && force[0] == '1',
                                           nullptr);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipDeviceSynchronize());
                    ix->d.successors = 1;
                    ix->layout[6] = 1;
                }
            } else {                 // not a set the reference's probe reaches everywhere: its layout decides
                ix->buckets.reset();
            }
        }
    }
    {   // what the transcript pool is rebuilt from, should a caller ask for it (skm_index_build_transcripts)
        const Coord *ht = (const Coord *)targets;
        ix->pool_targets.assign(ht, ht + n_targets);
        ix->pool_contigs.resize((size_t)n_contigs);
        for (int64_t c = 0; c < n_contigs; ++c)
            ix->pool_contigs[(size_t)c] = PoolContig{hc[c].target_offset, (int32_t)hc[c].offset, (int32_t)hc[c].length,
                                                     (int32_t)hc[c].target_length, 0};
    }
    *out = ix.release();                                  // (the caller's handle from here on)
    return SKM_OK;
}

extern "C" int skm_index_destroy(skm_index *ix)
{
    if (!ix) return SKM_OK;
    if (ix->holders.fetch_sub(1) == 1) delete ix;         // (else a mapper still maps against it)
    return SKM_OK;
}

extern "C" int skm_index_info(const skm_index *ix, int64_t info[8])
{
    if (!ix || !info) return fail(SKM_ERR_ARG, "NULL argument");
    info[0] = ix->n_slots;
    info[1] = ix->d.n_contigs;
    info[2] = ix->d.n_bases;
    info[3] = ix->d.n_targets;
    info[4] = ix->d.max_target_count;
    info[5] = ix->bytes;
    info[6] = ix->d.edge_windows;
    info[7] = ix->d.sorted_targets;
    return SKM_OK;
}

extern "C" int skm_index_layout(const skm_index *ix, int64_t layout[8])
{
    if (!ix || !layout) return fail(SKM_ERR_ARG, "NULL argument");
    for (int i = 0; i < 8; ++i) layout[i] = ix->layout[i];
    return SKM_OK;
}

extern "C" int skm_index_junctions(const skm_index *ix, int32_t *succ, uint8_t *kept)
{
    if (!ix || !succ || !kept) return fail(SKM_ERR_ARG, "NULL argument");
    if (!ix->layout[6]) return fail(SKM_ERR_STATE, "the contig records of this index carry no junction successors");
    SKM_TRY(set_device(ix->device));
    const int64_t n_contigs = ix->d.n_contigs;
    std::vector<DevContig> rows((size_t)n_contigs);
    if (n_contigs)
        HIP_TRY(hipMemcpy(rows.data(), ix->contigs, (size_t)n_contigs * sizeof(DevContig), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < n_contigs; ++c)
        for (int s = 0; s < 2; ++s)
            for (int b = 0; b < 4; ++b) {
                succ[c * 8 + s * 4 + b] = rows[(size_t)c].side[s].succ[b];
                kept[c * 8 + s * 4 + b] = rows[(size_t)c].side[s].kept[b];
            }
    return SKM_OK;
}

extern "C" int skm_index_probe(const skm_index *ix, int mode, const uint64_t *kmers, int64_t n, int32_t *entry,
                               int32_t *offset)
{
    if (!ix || n < 0 || (n && (!kmers || !entry || !offset))) return fail(SKM_ERR_ARG, "NULL array or negative size");
    if (mode < 0 || mode > 3) return fail(SKM_ERR_ARG, "unknown probe mode %d", mode);
    for (int64_t i = 0; i < n; ++i)
        if (kmers[i] & ~KMER_MASK) return fail(SKM_ERR_ARG, "query %lld has bits above the %d a k-mer has", (long long)i, 2 * K);
    if ((mode == 1 || mode == 2) && !ix->d.buckets) return fail(SKM_ERR_STATE, "this index is probed in the reference's layout: no buckets");
    if (mode == 3 && !ix->d.signatures) return fail(SKM_ERR_STATE, "this index has no signature table");
    if (n == 0) return SKM_OK;
    SKM_TRY(set_device(ix->device));
    DevMem d_kmers, d_entry, d_offset;
    HIP_TRY(hipMalloc(d_kmers.out(), (size_t)n * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(d_entry.out(), (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipMalloc(d_offset.out(), (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(d_kmers, kmers, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    launch_index_probe(ix->d, mode, (const uint64_t *)d_kmers.get(), n, (int32_t *)d_entry.get(), (int32_t *)d_offset.get(),
                       nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(entry, d_entry, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(offset, d_offset, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SKM_OK;
}

// ---- the transcript pool and the sequence-bias correction (skm_bias.hip) ----------------------------
extern "C" int skm_index_build_transcripts(skm_index *ix, const double *lengths, int64_t n_tx)
{
    if (!ix || n_tx < 0 || (n_tx && !lengths)) return fail(SKM_ERR_ARG, "bad argument");
    for (int64_t t = 0; t < n_tx; ++t)
        if (!(lengths[t] >= 0.0 && lengths[t] < 2147483648.0) || lengths[t] != std::floor(lengths[t]))
            return fail(SKM_ERR_ARG, "transcript %lld: its length is not a whole number below 2^31", (long long)t);
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    if (ix->pool_built) {
        if (ix->pool.n_tx == n_tx) return SKM_OK;
        return fail(SKM_ERR_STATE, "the transcript pool of this index holds %lld transcripts, not %lld",
                    (long long)ix->pool.n_tx, (long long)n_tx);
    }
    SKM_TRY(set_device(ix->device));
    std::vector<int64_t> tx_word((size_t)n_tx + 1, 0), tx_base((size_t)n_tx + 1, 0);
    std::vector<int32_t> tx_len((size_t)n_tx, 0);
    for (int64_t t = 0; t < n_tx; ++t) {
        tx_len[(size_t)t] = (int32_t)lengths[t];
        tx_word[(size_t)t + 1] = tx_word[(size_t)t] + (tx_len[(size_t)t] + 31) / 32;      // every transcript starts a word
        tx_base[(size_t)t + 1] = tx_base[(size_t)t] + tx_len[(size_t)t];
    }
    const int64_t n_words = tx_word[(size_t)n_tx];
    const int64_t n_contigs = (int64_t)ix->pool_contigs.size(), n_targets = (int64_t)ix->pool_targets.size();
    DevMem codes, known, d_word, d_len, d_windows, d_contigs, d_targets, d_bad;
    HIP_TRY(hipMalloc(codes.out(), (size_t)(n_words + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(known.out(), (size_t)(n_words + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(d_word.out(), (size_t)(n_tx + 1) * sizeof(int64_t)));
    HIP_TRY(hipMalloc(d_len.out(), (size_t)(n_tx + 1) * sizeof(int32_t)));
    HIP_TRY(hipMalloc(d_windows.out(), (size_t)(n_tx + 1) * sizeof(int32_t)));
    HIP_TRY(hipMalloc(d_contigs.out(), (size_t)(n_contigs + 1) * sizeof(PoolContig)));
    HIP_TRY(hipMalloc(d_targets.out(), (size_t)(n_targets + 1) * sizeof(Coord)));
    HIP_TRY(hipMalloc(d_bad.out(), sizeof(unsigned long long)));
    HIP_TRY(hipMemset(codes, 0, (size_t)(n_words + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMemset(known, 0, (size_t)(n_words + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemset(d_bad, 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemcpy(d_word, tx_word.data(), (size_t)(n_tx + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (n_tx) HIP_TRY(hipMemcpy(d_len, tx_len.data(), (size_t)n_tx * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_contigs)
        HIP_TRY(hipMemcpy(d_contigs, ix->pool_contigs.data(), (size_t)n_contigs * sizeof(PoolContig), hipMemcpyHostToDevice));
    if (n_targets)
        HIP_TRY(hipMemcpy(d_targets, ix->pool_targets.data(), (size_t)n_targets * sizeof(Coord), hipMemcpyHostToDevice));
    TxPool pool{(uint64_t *)codes.get(), (uint32_t *)known.get(), (const int64_t *)d_word.get(),
                (const int32_t *)d_len.get(), n_tx, n_words};
    launch_bias_pool_scatter(ix->d.seq2, (const PoolContig *)d_contigs.get(), n_contigs, (const Coord *)d_targets.get(), pool,
                             (unsigned long long *)d_bad.get(), nullptr);
    launch_bias_windows(pool, (int32_t *)d_windows.get(), nullptr);
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    std::vector<int32_t> windows((size_t)n_tx, 0);
    HIP_TRY(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
    if (n_tx) HIP_TRY(hipMemcpy(windows.data(), d_windows, (size_t)n_tx * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (bad)
        return fail(SKM_ERR_ARG, "%llu target rows name a transcript at or above %lld or leave its length: these are not the "
                                 "lengths of this index", bad, (long long)n_tx);
    ix->pool = pool;
    ix->pool_codes.reset(codes.release()); ix->pool_known.reset(known.release()); ix->pool_tx_word.reset(d_word.release());
    ix->pool_tx_len.reset(d_len.release()); ix->pool_tx_windows.reset(d_windows.release());
    ix->pool_tx_base = std::move(tx_base);
    ix->pool_windows = std::move(windows);
    ix->pool_built = true;
    std::vector<PoolContig>().swap(ix->pool_contigs);
    std::vector<Coord>().swap(ix->pool_targets);
    return SKM_OK;
}

extern "C" int skm_index_transcript_bases(skm_index *ix, char *bases_out, uint8_t *known_out)
{
    if (!ix) return fail(SKM_ERR_ARG, "NULL index");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    if (!ix->pool_built) return fail(SKM_ERR_STATE, "the transcript pool has not been built: call skm_index_build_transcripts");
    SKM_TRY(set_device(ix->device));
    const int64_t n_tx = ix->pool.n_tx, n_words = ix->pool.n_words;
    std::vector<uint64_t> codes((size_t)n_words + 1);
    std::vector<uint32_t> known((size_t)n_words + 1);
    std::vector<int64_t> tx_word((size_t)n_tx + 1);
    HIP_TRY(hipMemcpy(codes.data(), ix->pool_codes, (size_t)(n_words + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(known.data(), ix->pool_known, (size_t)(n_words + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tx_word.data(), ix->pool_tx_word, (size_t)(n_tx + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t t = 0; t < n_tx; ++t) {
        const int64_t first = ix->pool_tx_base[(size_t)t], len = ix->pool_tx_base[(size_t)t + 1] - first;
        for (int64_t p = 0; p < len; ++p) {
            const size_t w = (size_t)(tx_word[(size_t)t] + (p >> 5));
            const bool is_known = (known[w] >> (31 - (p & 31))) & 1u;
            if (bases_out) bases_out[first + p] = is_known ? "ACGT"[(codes[w] >> (62 - 2 * (p & 31))) & 3u] : 'N';
            if (known_out) known_out[first + p] = is_known ? 1 : 0;
        }
    }
    return SKM_OK;
}

namespace {

// the grid of the two kernels over the pool; SKM_BIAS_BLOCKS (test hook) caps it
int bias_blocks(const skm_index *ix, int *blocks)
{
    *blocks = ix->cu_count * 4;
    if (const char *v = getenv("SKM_BIAS_BLOCKS")) {
        const long long n = atoll(v);
        if (n < 1) return fail(SKM_ERR_ARG, "SKM_BIAS_BLOCKS must be at least 1, not '%s'", v);
        *blocks = (int)std::min<long long>(n, *blocks);
    }
    return SKM_OK;
}

// rows per group of skm_bias_correct_many: a row's buffers in HBM are BIAS_LIMBS + 2 words per transcript (weights,
// eff, eff') and BIAS_LIMBS + 3 per hexamer (O, E's limbs, E, b); a group's stay within 256 MB, and a group holds
// at most BIAS_MANY_MAX_GROUP rows (a grid dimension).  SKM_BIAS_MANY_GROUP (tests): fewer.
int64_t bias_many_group(int64_t n, int64_t n_tx)
{
    const int64_t row_bytes = ((BIAS_LIMBS + 2) * n_tx + (BIAS_LIMBS + 3) * (int64_t)BIAS_BINS) * 8;
    int64_t group = std::min<int64_t>((int64_t)(1LL << 28) / row_bytes, BIAS_MANY_MAX_GROUP);
    if (const char *v = getenv("SKM_BIAS_MANY_GROUP"))
        if (atoll(v) > 0) group = std::min<int64_t>(group, atoll(v));
    return std::max<int64_t>(1, std::min(group, n));
}

}  // namespace

extern "C" int skm_bias_correct(skm_index *ix, int strand, const int64_t *observed, const double *tpm, const double *eff,
                                int64_t n_tx, double *expected_out, double *b_out, double *eff_out)
{
    if (!ix || !observed || n_tx < 0 || (n_tx && (!tpm || !eff || !eff_out))) return fail(SKM_ERR_ARG, "NULL array or negative size");
    if (strand != SKM_STRAND_NONE && strand != SKM_STRAND_FR && strand != SKM_STRAND_RF)
        return fail(SKM_ERR_ARG, "unknown strand mode %d", strand);
    for (int i = 0; i < BIAS_BINS; ++i)
        if (observed[i] < 0) return fail(SKM_ERR_ARG, "observed count %d is negative", i);
    for (int64_t t = 0; t < n_tx; ++t)
        if (!(tpm[t] >= 0.0) || std::isinf(tpm[t]))
            return fail(SKM_ERR_ARG, "the abundance of transcript %lld is negative or not finite", (long long)t);
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    if (!ix->pool_built) return fail(SKM_ERR_STATE, "the transcript pool has not been built: call skm_index_build_transcripts");
    if (n_tx != ix->pool.n_tx)
        return fail(SKM_ERR_ARG, "%lld transcripts, but the pool holds %lld", (long long)n_tx, (long long)ix->pool.n_tx);
    SKM_TRY(set_device(ix->device));
    // E in 96-bit fixed point (skm_bias_weights.h): W_t as three 32-bit limbs that the device sums apart
    double total = 0.0;
    const double fixed_one = BIAS_FIXED_ONE;
    std::vector<unsigned long long> weight((size_t)n_tx * BIAS_LIMBS + 1, 0);      // [limb][n_tx]
    if (!bias_fixed_weights(tpm, ix->pool_windows.data(), n_tx, weight.data(), &total))
        return fail(SKM_ERR_ARG, "the abundances are too large or too small to scale");
    const double share = strand == SKM_STRAND_NONE ? 0.5 : 1.0;
    int blocks = 0;
    SKM_TRY(bias_blocks(ix, &blocks));
    DevMem d_weight, d_observed, d_expected, d_expected_out, d_b, d_eff, d_eff_out;
    HIP_TRY(hipMalloc(d_weight.out(), (size_t)(n_tx * BIAS_LIMBS + 1) * 8));
    HIP_TRY(hipMalloc(d_eff.out(), (size_t)(n_tx + 1) * 8));
    HIP_TRY(hipMalloc(d_eff_out.out(), (size_t)(n_tx + 1) * 8));
    HIP_TRY(hipMalloc(d_observed.out(), BIAS_BINS * 8));
    HIP_TRY(hipMalloc(d_expected.out(), BIAS_LIMBS * BIAS_BINS * 8));
    HIP_TRY(hipMalloc(d_expected_out.out(), BIAS_BINS * 8));
    HIP_TRY(hipMalloc(d_b.out(), BIAS_BINS * 8));
    HIP_TRY(hipMemset(d_expected, 0, BIAS_LIMBS * BIAS_BINS * 8));
    HIP_TRY(hipMemcpy(d_observed, observed, BIAS_BINS * 8, hipMemcpyHostToDevice));
    if (n_tx) {
        HIP_TRY(hipMemcpy(d_weight, weight.data(), (size_t)n_tx * BIAS_LIMBS * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_eff, eff, (size_t)n_tx * 8, hipMemcpyHostToDevice));
    }
    launch_bias_expected(ix->pool, (const unsigned long long *)d_weight.get(), strand, (unsigned long long *)d_expected.get(),
                         blocks, nullptr);
    launch_bias_weights((const unsigned long long *)d_observed.get(), (const unsigned long long *)d_expected.get(),
                        share * (total / fixed_one), (double *)d_expected_out.get(), (double *)d_b.get(), nullptr);
    launch_bias_lengths(ix->pool, (const int32_t *)ix->pool_tx_windows.get(), (const double *)d_b.get(), strand,
                        (const double *)d_eff.get(), (double *)d_eff_out.get(), blocks, nullptr);
    HIP_TRY(hipGetLastError());
    if (expected_out) HIP_TRY(hipMemcpy(expected_out, d_expected_out, BIAS_BINS * 8, hipMemcpyDeviceToHost));
    if (b_out) HIP_TRY(hipMemcpy(b_out, d_b, BIAS_BINS * 8, hipMemcpyDeviceToHost));
    if (n_tx) HIP_TRY(hipMemcpy(eff_out, d_eff_out, (size_t)n_tx * 8, hipMemcpyDeviceToHost));
    return SKM_OK;                                                   // (the copies home have waited for the kernels)
}

extern "C" int skm_bias_correct_many(skm_index *ix, int strand, int64_t n, const int64_t *observed, const double *tpm,
                                     const double *eff, int64_t n_tx, double *expected_out, double *b_out, double *eff_out)
{
    if (!ix || n < 0 || n_tx < 0 || (n && (!observed || (n_tx && (!tpm || !eff || !eff_out)))))
        return fail(SKM_ERR_ARG, "NULL array or negative size");
    if (strand != SKM_STRAND_NONE && strand != SKM_STRAND_FR && strand != SKM_STRAND_RF)
        return fail(SKM_ERR_ARG, "unknown strand mode %d", strand);
    for (int64_t i = 0; i < n * BIAS_BINS; ++i)
        if (observed[i] < 0) return fail(SKM_ERR_ARG, "row %lld: observed count %lld is negative", (long long)(i / BIAS_BINS), (long long)(i % BIAS_BINS));
    for (int64_t i = 0; i < n * n_tx; ++i)
        if (!(tpm[i] >= 0.0) || std::isinf(tpm[i]))
            return fail(SKM_ERR_ARG, "row %lld: the abundance of transcript %lld is negative or not finite", (long long)(i / n_tx), (long long)(i % n_tx));
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    if (!ix->pool_built) return fail(SKM_ERR_STATE, "the transcript pool has not been built: call skm_index_build_transcripts");
    if (n_tx != ix->pool.n_tx)
        return fail(SKM_ERR_ARG, "%lld transcripts, but the pool holds %lld", (long long)n_tx, (long long)ix->pool.n_tx);
    if (n == 0) return SKM_OK;
    // every row's total (skm_bias_weights.h) and the scale that takes its E back, before any device work
    const int64_t group = bias_many_group(n, n_tx);
    std::vector<unsigned long long> weight((size_t)(group * n_tx * BIAS_LIMBS) + 1, 0);     // [row][limb][n_tx], a group's
    std::vector<double> totals((size_t)n, 0.0), scale((size_t)n, 0.0);
    const double share = strand == SKM_STRAND_NONE ? 0.5 : 1.0;
    for (int64_t s = 0; s < n; ++s) {
        if (!bias_fixed_total(tpm + s * n_tx, ix->pool_windows.data(), n_tx, &totals[(size_t)s]))
            return fail(SKM_ERR_ARG, "row %lld: the abundances are too large or too small to scale", (long long)s);
        scale[(size_t)s] = share * (totals[(size_t)s] / BIAS_FIXED_ONE);
    }
    SKM_TRY(set_device(ix->device));
    int blocks = 0;
    SKM_TRY(bias_blocks(ix, &blocks));
    DBuf<unsigned long long> d_weight, d_observed, d_expected;
    DBuf<double> d_scale, d_expected_out, d_b, d_eff, d_eff_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_weight.ensure((size_t)(group * n_tx * BIAS_LIMBS) + 1));
    SKM_TRY(d_eff.ensure((size_t)(group * n_tx) + 1)); SKM_TRY(d_eff_out.ensure((size_t)(group * n_tx) + 1));
    SKM_TRY(d_observed.ensure((size_t)group * BIAS_BINS)); SKM_TRY(d_expected.ensure((size_t)group * BIAS_LIMBS * BIAS_BINS));
    SKM_TRY(d_expected_out.ensure((size_t)group * BIAS_BINS)); SKM_TRY(d_b.ensure((size_t)group * BIAS_BINS));
    SKM_TRY(d_scale.ensure((size_t)group));
    for (int64_t first = 0; first < n; first += group) {
        const int64_t here = std::min(group, n - first);
        for (int64_t s = 0; s < here; ++s)
            bias_fixed_limbs(tpm + (first + s) * n_tx, ix->pool_windows.data(), n_tx, totals[(size_t)(first + s)],
                             weight.data() + s * n_tx * BIAS_LIMBS);
        HIP_TRY(hipMemsetAsync(d_expected.p, 0, (size_t)here * BIAS_LIMBS * BIAS_BINS * 8, nullptr));
        HIP_TRY(hipMemcpy(d_observed.p, observed + first * BIAS_BINS, (size_t)here * BIAS_BINS * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_scale.p, scale.data() + first, (size_t)here * 8, hipMemcpyHostToDevice));
        if (n_tx) {
            HIP_TRY(hipMemcpy(d_weight.p, weight.data(), (size_t)(here * n_tx * BIAS_LIMBS) * 8, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_eff.p, eff + first * n_tx, (size_t)(here * n_tx) * 8, hipMemcpyHostToDevice));
        }
        // (results do not depend on a grid: with many rows a row's share of the device is smaller)
        const int rows_lengths = (int)((here + BIAS_LENGTHS_G - 1) / BIAS_LENGTHS_G);
        const int blocks_expected = (int)std::max<int64_t>(std::min<int64_t>(blocks, 4), std::min<int64_t>(blocks, (int64_t)ix->cu_count * 8 / (here * BIAS_LIMBS)));
        const int blocks_lengths = (int)std::max<int64_t>(std::min<int64_t>(blocks, 4), std::min<int64_t>(blocks, (int64_t)ix->cu_count * 8 / rows_lengths));
        launch_bias_expected_many(ix->pool, d_weight.p, here, strand, d_expected.p, blocks_expected, nullptr);
        launch_bias_weights_many(d_observed.p, d_expected.p, d_scale.p, here, d_expected_out.p, d_b.p, nullptr);
        launch_bias_lengths_many(ix->pool, (const int32_t *)ix->pool_tx_windows.get(), d_b.p, here, strand, d_eff.p, d_eff_out.p,
                                 blocks_lengths, nullptr);
        HIP_TRY(hipGetLastError());
        if (expected_out) HIP_TRY(hipMemcpy(expected_out + first * BIAS_BINS, d_expected_out.p, (size_t)here * BIAS_BINS * 8, hipMemcpyDeviceToHost));
        if (b_out) HIP_TRY(hipMemcpy(b_out + first * BIAS_BINS, d_b.p, (size_t)here * BIAS_BINS * 8, hipMemcpyDeviceToHost));
        if (n_tx) HIP_TRY(hipMemcpy(eff_out + first * n_tx, d_eff_out.p, (size_t)(here * n_tx) * 8, hipMemcpyDeviceToHost));
        else HIP_TRY(hipStreamSynchronize(nullptr));
    }
    drain.dismiss();                                                 // (the copies home have waited for the kernels)
    return SKM_OK;
}

// ------------------------------------------------------------------- mapper
namespace {

constexpr int CTR_ARENA = 0, CTR_CLASSES = 1, CTR_UNALIGNED = 2, CTR_UNITS = 3, CTR_LISTED = 4,
              CTR_DEFERRED = 5, CTR_COMMITTED = 6, CTR_FLD = 8;
constexpr int CTR_WORDS = 8 + MAX_FRAGMENT_LENGTH;
constexpr int BC_IDS = 0, BC_FLD = 8, BC_STATS = 2048, BC_WORDS = 2096;

void bind_table(skm_mapper *m, uint64_t n_slots)
{
    m->t.slots = m->slots.p;
    m->t.slot_mask = n_slots - 1;
    m->t.arena = m->arena.p;
    m->t.arena_capacity = (int64_t)m->arena.cap;
    m->t.arena_cursor = m->counters.p + CTR_ARENA;
    m->t.n_classes = m->counters.p + CTR_CLASSES;
    m->t.n_unaligned = m->counters.p + CTR_UNALIGNED;
    m->t.n_units = m->counters.p + CTR_UNITS;
    m->t.global_fld = m->counters.p + CTR_FLD;
    m->t.class_list = m->class_list.p;
    m->t.class_list_capacity = (int64_t)m->class_list.cap;
    m->t.n_listed = m->counters.p + CTR_LISTED;
    m->t.n_deferred = m->counters.p + CTR_DEFERRED;
    m->t.arena_committed = m->counters.p + CTR_COMMITTED;
    m->t.error = m->error.p;
}

int table_reset(skm_mapper *m, uint64_t n_slots)
{
    SKM_TRY(m->slots.ensure(n_slots));
    SKM_TRY(m->arena.ensure(1 << 20));
    SKM_TRY(m->class_list.ensure(1 << 16));
    SKM_TRY(m->counters.ensure(CTR_WORDS));
    SKM_TRY(m->error.ensure(1));
    HIP_TRY(hipMemsetAsync(m->counters.p, 0, CTR_WORDS * sizeof(unsigned long long), m->stream));
    HIP_TRY(hipMemsetAsync(m->error.p, 0, sizeof(int), m->stream));
    bind_table(m, n_slots);
    launch_class_init(m->t, m->stream);
    HIP_TRY(hipGetLastError());
    m->host_classes = 0;
    m->host_arena_used = 0;
    m->host_units = m->host_unaligned = 0;
    m->host_totals_valid = true;
    m->units_done = 0;
    m->first_seen_bound = 0;
    return SKM_OK;
}

// make the class table at least `want_slots` big (power of two), moving its
// entries; the registry (and, for a batch in flight, the unit -> slot map) is
// redirected through a forwarding array
int table_grow(skm_mapper *m, uint64_t want_slots, int64_t units_in_flight)
{
    uint64_t n_slots = m->t.slot_mask + 1;
    uint64_t need = n_slots;
    while (need < want_slots) need <<= 1;
    if (need == n_slots) return SKM_OK;
    if (units_in_flight > 0) m->deferred_grows += 1;
    DBuf<ClassSlot> new_slots;
    DBuf<int64_t> forward;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
    SKM_TRY(new_slots.ensure(need));
    SKM_TRY(forward.ensure(n_slots));
    ClassTable to = m->t;
    to.slots = new_slots.p;
    to.slot_mask = need - 1;
    launch_class_init(to, m->stream);
    launch_class_rehash(m->t, to, forward.p, m->stream);
    unsigned long long listed = 0;
    HIP_TRY(hipMemcpyAsync(&listed, m->counters.p + CTR_LISTED, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    launch_slot_remap(m->class_list.p, (int64_t)listed, forward.p, m->stream);
    launch_slot_remap(m->unit_slot.p, units_in_flight, forward.p, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    drain.dismiss();
    m->slots = std::move(new_slots);
    bind_table(m, need);
    return SKM_OK;
}

// What skm_mapper_expect_units announced (0: nothing): the table and the batch buffers are sized for
// it once instead of growing step by step under the first runs of a sample.
int table_reserve_for_sample(skm_mapper *m, int64_t sample_units)
{
    // (a hint, possibly a wild one: what it reserves is bounded -- 2^26 classes, 2 GB of table -- and
    // a sample that needs more grows the table as before)
    const double expect = (double)m->host_classes + (double)std::min<int64_t>(sample_units, 1LL << 29) / 8.0 + 1024.0;
    uint64_t want = 1 << 16;
    while ((double)want * 0.5 < expect && want < (1ULL << 26)) want <<= 1;
    if (!m->test_class_slots) SKM_TRY(table_grow(m, want, 0));
    SKM_TRY(m->class_list.ensure((size_t)(expect + 1024.0), true, m->stream));
    SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + (int64_t)(expect * 6.0) + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    return SKM_OK;
}

// Size the table for a batch of `n_units`: classes are far fewer than units in
// practice (0.09 per pair at 10 M pairs), so reserve for one new class per 8
// units at load <= 0.5 and let the bounded probe defer the rest.
int table_reserve(skm_mapper *m, int64_t n_units)
{
    const double expect = (double)m->host_classes + (double)n_units / 8.0 + 1024.0;
    uint64_t want = 1 << 16;
    while ((double)want * 0.5 < expect) want <<= 1;
    if (!m->test_class_slots) SKM_TRY(table_grow(m, want, 0));
    // registry and arena can never need more than one entry per unit / id of the batch
    SKM_TRY(m->class_list.ensure((size_t)(m->host_classes + n_units + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    return SKM_OK;
}

int read_error(skm_mapper *m)
{
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, m->error.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (err == SKM_ERR_COLLISION)
        return fail(SKM_ERR_COLLISION, "two different class tuples share a 64-bit key");
    if (err) return fail(err, "class table kernel reported error %d", err);
    return SKM_OK;
}

// first_unit: global index of the batch's first unit (first-seen values count from it), or -1
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
                       unsigned long long *sample_bias_rows = nullptr, const BatchStage *collapse = nullptr)
{
    const int64_t unit_base = first_unit >= 0 ? first_unit : m->units_done;
    skm_index *ix = m->ix;
    const int64_t n_reads = paired ? 2 * n_units : n_units;
    const int words = (max_len + 31) / 32 + 1;
    m->last_units = n_units;
    m->last_ids = 0;
    m->last_reads = 0;
    if (n_units == 0) return SKM_OK;

    const int record_words = ((3 * words + 1 + 15) / 16) * 16;      // 64-byte records
    SKM_TRY(m->records.ensure((size_t)n_reads * record_words + 16));
    m->last_reads = n_reads;
    m->last_words = words;
    m->last_record_words = record_words;
    if (n_units >= (1LL << 31)) return fail(SKM_ERR_ARG, "more than 2^31 - 1 units in one batch");
    if (m->keep_spans) {
        SKM_TRY(m->unit_begin.ensure(n_units));
        SKM_TRY(m->unit_end.ensure(n_units));
        SKM_TRY(m->unit_anchor.ensure(n_units));
    }
    m->last_spans = m->keep_spans;
    SKM_TRY(m->rec_unit.ensure(n_units));
    SKM_TRY(m->rec_tuple.ensure(n_units));
    SKM_TRY(m->unit_slot.ensure(n_units));
    SKM_TRY(m->rec_key.ensure(n_units));

    SKM_TRY(m->batch_ctl.ensure(BC_WORDS));

    // launch geometry: persistent blocks of 256 lanes, each with MAP_CONTEXTS unit contexts in LDS
    // (just under 40 KB -> 4 blocks per CU); fewer blocks when the per-context list workspace
    // (2 lists of max_target_count entries) would not fit the budget
    constexpr int64_t CONTEXTS = MAP_CONTEXTS;
    int64_t blocks = std::min<int64_t>((n_units + CONTEXTS - 1) / CONTEXTS, (int64_t)ix->cu_count * MAP_BLOCKS_PER_CU);
    if (m->test_map_blocks) blocks = std::min<int64_t>(blocks, m->test_map_blocks);
    // per context: mask extension words (live + staging, two mates) for slices > 64 targets
    const int64_t ext_words = std::max<int64_t>(0, (ix->d.max_target_count + 63) / 64 - 1);
    SKM_TRY(m->workspace.ensure((size_t)(blocks * CONTEXTS * 4 * ext_words * 2 + 16)));
    m->grid_blocks = (int)blocks;
    {   // the kernel addresses a block's records with 32-bit byte offsets
        const int64_t per_block = (n_units + blocks - 1) / blocks;
        if (per_block * (paired ? 2 : 1) * (int64_t)record_words * 4 >= (1LL << 32))
            return fail(SKM_ERR_ARG, "batch of %lld units with %d-base reads is too large for one launch",
                        (long long)n_units, max_len);
    }
    // entry arena: ~8 ids per unit plus one 2048-id slice of slack per wave
    SKM_TRY(m->unit_entries.ensure((size_t)n_units * 8 + (size_t)blocks * (MAP_THREADS / 64) * MAP_ARENA_CHUNK + 4096));

    MapBatch b{};
    b.records = m->records.p;
    b.n_units = n_units;
    b.words_per_read = words;
    b.record_words = record_words;
    b.paired = paired;
    b.workspace = m->workspace.p;
    b.unit_begin = m->unit_begin.p;
    b.unit_end = m->unit_end.p;
    b.unit_anchor = m->unit_anchor.p;
    b.keep_spans = m->keep_spans ? 1 : 0;
    b.rec_unit = m->rec_unit.p;
    b.rec_tuple = m->rec_tuple.p;
    b.rec_key = m->rec_key.p;
    b.ids_cursor = m->batch_ctl.p + BC_IDS;
    b.fld = m->batch_ctl.p + BC_FLD;
    b.stats = m->batch_ctl.p + BC_STATS;
    for (int i = 0; i < 8; ++i) b.vote[i] = m->vote[i];

    HIP_TRY(hipEventRecord(m->ev[0], m->stream));
    if (fill_records) SKM_TRY((*fill_records)(m->records.p, words, record_words));
    else launch_pack_reads(d_bases, d_offsets, n_reads, words, record_words, m->records.p, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev[1], m->stream));
    unsigned long long ids = 0;
    // A launch whose ids outgrow the arena stores none of the tuples that do not fit and is run again
    // in a larger one.  A wave takes max(its emission, MAP_ARENA_CHUNK) ids per grab and gives up what is
    // left of a chunk that the next emission does not fit, so the cursor of such a launch depends on
    // how the finished units happened to meet in emission waves, which differs from launch to launch:
    // it bounds no later launch of the same kind.  The relaunch therefore takes exactly what each
    // emission writes (ids_chunk = 0).  Its cursor is the sum of the batch's tuple lengths whatever the
    // grouping, and that sum is at most the first launch's cursor, because every emission of the first
    // launch lay wholly inside a chunk of its own wave and the chunks are disjoint.  An arena of the
    // first cursor's size cannot overflow a second time.
    for (int attempt = 0; attempt < 2; ++attempt) {
        b.unit_entries = m->unit_entries.p;
        b.ids_capacity = (int64_t)m->unit_entries.cap;
        b.ids_chunk = attempt == 0 ? MAP_ARENA_CHUNK : 0;
        HIP_TRY(hipMemsetAsync(m->batch_ctl.p, 0, BC_WORDS * sizeof(unsigned long long), m->stream));
        launch_map_units(ix->d, b, m->grid_blocks, m->want_stats, m->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(m->ev[2], m->stream));
        unsigned long long *cursor_and_flag = m->pinned + 32;
        HIP_TRY(hipMemcpyAsync(cursor_and_flag, b.ids_cursor, 16, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        ids = cursor_and_flag[0];
        if (cursor_and_flag[1]) return fail(SKM_ERR_STATE, "map kernel: the in-kernel scheduler stalled");
        if ((int64_t)ids <= b.ids_capacity) break;
        if (attempt == 1) return fail(SKM_ERR_STATE, "entry arena overflow");
        SKM_TRY(m->unit_entries.ensure((size_t)ids));
        m->map_relaunches += 1;
    }
    m->last_ids = (int64_t)ids;
    if (m->want_stats) {
        unsigned long long st[48];
        HIP_TRY(hipMemcpy(st, b.stats, sizeof(st), hipMemcpyDeviceToHost));
        for (int i = 0; i < 48; ++i) m->stats_total[i] += st[i];
    }
    // strand-specific library: the records keep the entries of its orientation (nothing is
    // launched unstranded)
    if (m->strand != SKM_STRAND_NONE) {
        launch_strand_filter(b, m->strand, m->stream);
        HIP_TRY(hipGetLastError());
    }
    if (collapse) SKM_TRY((*collapse)(b));
    if (m->bias) {             // --bias: the first hexamers of the units that are still aligned
        launch_bias_observed(m->records.p, record_words, words, paired, m->rec_tuple.p, m->rec_unit.p, n_units,
                             m->bias_observed.p, m->stream);
        HIP_TRY(hipGetLastError());
    }
    if (salt && sample_bias_rows) {   // a sample set that counts: the same rule, by the unit's sample
        launch_sample_bias(b, *salt, sample_bias_rows, m->stream);
        HIP_TRY(hipGetLastError());
    }
    if (salt) {
        launch_sample_salt(b, *salt, m->error.p, m->stream);
        HIP_TRY(hipGetLastError());
    }

    // class counting
    SKM_TRY(table_reserve(m, n_units));
    SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + (int64_t)ids + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    // A large batch on an empty table goes in two waves of records: once the classes of the first
    // quarter are committed, most records of the rest land on a committed class and are verified
    // inside class_insert (the slot's tuple word came with the probe); class_verify's second random
    // pass over the table is left with the first wave and the records of classes new in the second.
    const bool two_waves = m->host_classes == 0 && n_units >= (1 << 21);
    for (int pass = 0;; ++pass) {
        // insert (with the commit of the new classes) -> totals -> verify: one pipeline, one
        // synchronisation; the optimistic case needs a single pass
        HIP_TRY(hipMemsetAsync(m->counters.p + CTR_DEFERRED, 0, 8, m->stream));
        // (wave borders in sixteenths of the batch; SKM_CLASS_WAVES="2,8" etc. is a tuning aid)
        int cuts[8] = {4, 16, 16, 16, 16, 16, 16, 16};
        int n_waves = two_waves && pass == 0 ? 2 : 1;
#ifdef SKM_TUNING                                    // (tuning builds only: scripts/build_variant.sh)
        if (n_waves > 1)
            if (const char *e = getenv("SKM_CLASS_WAVES")) {
                int parsed[8], n = 0;
                bool ok = true;
                for (const char *c = e; *c && n < 7;) {
                    parsed[n] = atoi(c);
                    ok = ok && parsed[n] >= 1 && parsed[n] <= 16 && (n == 0 || parsed[n] > parsed[n - 1]);
                    ++n;
                    while (*c && *c != ',') ++c;
                    if (*c == ',') ++c;
                }
                if (ok && n > 0) {                 // strictly ascending sixteenths, else ignored
                    if (parsed[n - 1] < 16) parsed[n++] = 16;
                    for (int i = 0; i < n; ++i) cuts[i] = parsed[i];
                    n_waves = n;
                }
            }
#endif
        for (int wave = 0; wave < n_waves; ++wave) {
            const int64_t w0 = n_waves == 1 || wave == 0 ? 0 : n_units * cuts[wave - 1] / 16;
            const int64_t w1 = n_waves == 1 ? n_units : n_units * cuts[wave] / 16;
            MapBatch part = b;                   // records [w0, w1) of the batch
            part.rec_unit += w0; part.rec_key += w0; part.rec_tuple += w0;
            part.n_units = w1 - w0;
            launch_class_insert(m->t, part, unit_base, m->unit_slot.p + w0, pass > 0, pass == 0 && wave == 0, m->stream);
            launch_class_verify(m->t, part, m->unit_slot.p + w0, m->stream);
        }
        HIP_TRY(hipGetLastError());
        if (pass == 0) HIP_TRY(hipEventRecord(m->ev[3], m->stream));
        HIP_TRY(hipMemcpyAsync(m->pinned, m->counters.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(m->pinned + 16, m->error.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        const int err = *reinterpret_cast<int *>(m->pinned + 16);
        if (err == SKM_ERR_COLLISION)
            return fail(SKM_ERR_COLLISION, collapse ? "two different class tuples, or two different molecules, share a 64-bit key"
                                                    : "two different class tuples share a 64-bit key");
        if (err == SKM_ERR_ARG) return fail(SKM_ERR_ARG, "a packed read is longer than its code words hold");
        if (err) return fail(err, "class table kernel reported error %d", err);
        m->host_arena_used = (int64_t)m->pinned[CTR_ARENA];
        m->host_classes = (int64_t)m->pinned[CTR_CLASSES];
        m->host_units = m->pinned[CTR_UNITS];
        m->host_unaligned = m->pinned[CTR_UNALIGNED];
        m->host_totals_valid = true;
        if (m->pinned[CTR_LISTED] != m->pinned[CTR_CLASSES])
            return fail(SKM_ERR_STATE, "class registry out of step (%llu listed, %llu classes)",
                        m->pinned[CTR_LISTED], m->pinned[CTR_CLASSES]);
        if (m->pinned[CTR_DEFERRED] == 0) break;
        if (pass > 40) return fail(SKM_ERR_STATE, "class table cannot absorb the batch");
        // too full for bounded probing: grow 4x (its classes move along), retry the deferred units
        SKM_TRY(table_grow(m, (m->t.slot_mask + 1) * 4, n_units));
    }
    // keep the load below 0.5 for the next batch
    if ((uint64_t)m->host_classes * 2 > m->t.slot_mask + 1)
        SKM_TRY(table_grow(m, (m->t.slot_mask + 1) * 2, 0));
    m->units_done += n_units;
    m->first_seen_bound = std::max(m->first_seen_bound, std::max(m->units_done, unit_base + n_units));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[0], m->ev[1])); m->t_pack_ns += ms * 1e6;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[1], m->ev[2])); m->t_map_ns += ms * 1e6;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[2], m->ev[3])); m->t_class_ns += ms * 1e6;
    m->batches += 1;
    return SKM_OK;
}

}  // namespace

extern "C" int skm_mapper_create(skm_index *ix, skm_mapper **out)
{
    if (!ix || !out) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_device(ix->device));
    std::unique_ptr<skm_mapper> m(new skm_mapper(ix));     // (any early return below: nothing is left behind)
    HIP_TRY(pool_stream_acquire(m->stream.out()));
    for (auto &e : m->ev) HIP_TRY(hipEventCreate(e.out()));
    HIP_TRY(hipHostMalloc((void **)m->pinned.out(), 64 * sizeof(unsigned long long)));
    if (const char *v = getenv("SKM_MAP_STATS")) m->want_stats = v[0] == '2' ? 2 : 1;
    if (const char *v = getenv("SKM_TEST_PACKED_MAX_PENDING"))      // test hook: the pushers' byte limit
        if (atoll(v) > 0) m->packed_max_pending = atoll(v);
    if (const char *v = getenv("SKM_MAP_VOTE"))          // tuning aid: "start,lookup,merge,left,right,emit,scan"
        sscanf(v, "%d,%d,%d,%d,%d,%d,%d", &m->vote[0], &m->vote[1], &m->vote[2], &m->vote[3], &m->vote[4],
               &m->vote[5], &m->vote[6]);
    HIP_TRY(hipStreamCreateWithFlags(m->packed_stream.out(), hipStreamNonBlocking));   // (10 ms: not at the first piece's push)
    uint64_t first_slots = 1 << 16;
    if (const char *v = getenv("SKM_TEST_CLASS_SLOTS")) {        // test hook: a table that has to grow under a batch
        const long long n = atoll(v);
        if (n < 2 || n > (1LL << 30) || (n & (n - 1)))
            return fail(SKM_ERR_ARG, "SKM_TEST_CLASS_SLOTS must be a power of two from 2 to 2^30, not '%s'", v);
        first_slots = (uint64_t)n;
        m->test_class_slots = true;
    }
    if (const char *v = getenv("SKM_TEST_MAP_BLOCKS")) {         // test hook: few blocks, so that contexts are refilled
        const long long n = atoll(v);
        if (n < 1 || n > (1LL << 30))
            return fail(SKM_ERR_ARG, "SKM_TEST_MAP_BLOCKS must be a number from 1 to 2^30, not '%s'", v);
        m->test_map_blocks = (int)n;
    }
    SKM_TRY(table_reset(m.get(), first_slots));
    HIP_TRY(hipStreamSynchronize(m->stream));
    *out = m.release();                                     // (the caller's handle from here on)
    return SKM_OK;
}

skm_mapper::~skm_mapper()
{
    (void)hipSetDevice(ix->device);
    if (worker_started) {
        { std::lock_guard<std::mutex> hold(q_mu); stop = true; }
        q_cv.notify_all();
        worker.join();                     // (finishes what is queued)
    }
    // every stream drains before the members -- buffers, pieces, streams, events -- free themselves
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto &lane : lanes)
        if (lane.stream) (void)hipStreamSynchronize(lane.stream);
    if (packed_stream) (void)hipStreamSynchronize(packed_stream);
}

extern "C" int skm_mapper_destroy(skm_mapper *m)
{
    delete m;
    return SKM_OK;
}

namespace {

// ---- host batches: staging lanes and the mapping worker --------------------------------
int run_job(skm_mapper *m, const skm_mapper::Job &job)
{
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    skm_mapper::Lane &lane = m->lanes[job.lane];
    const int64_t n_reads = job.paired ? 2 * job.n_units : job.n_units;
    // longest read and monotonicity from the offsets in HBM (the lane's copy is complete)
    SKM_TRY(m->scan_out.ensure(2));
    HIP_TRY(hipMemsetAsync(m->scan_out.p, 0, 16, m->stream));
    launch_offsets_scan(lane.offsets.p, n_reads, job.offset_base, m->scan_out.p, m->stream);   // (and rebases them to 0)
    HIP_TRY(hipGetLastError());
    unsigned long long *scan = m->pinned + 40;
    HIP_TRY(hipMemcpyAsync(scan, m->scan_out.p, 16, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (scan[1]) return fail(SKM_ERR_ARG, "offsets are not monotone (%llu descents)", scan[1]);
    if (scan[0] > (1ULL << 20)) return fail(SKM_ERR_ARG, "read longer than 2^20 bases");
    return map_batch_resident(m, lane.bases.p, lane.offsets.p, job.n_units, job.paired, (int)scan[0],
                              job.first_unit);
}

// ---- packed pieces ----------------------------------------------------------------------
constexpr int64_t PACKED_MIN_UNITS = 1 << 15;      // smaller runs wait for more (or for a flush)
constexpr int64_t PACKED_MAX_UNITS = 1 << 21;      // one launch

// (q_mu held) the first run of units that every stream covers: [*lo, *hi), at most PACKED_MAX_UNITS
bool packed_find_run(skm_mapper *m, int64_t *lo, int64_t *hi)
{
    const auto &a = m->pending[0];
    if (a.empty()) return false;
    if (m->packed_paired != 1) {
        *lo = a.front().first;
        *hi = *lo;
        for (const auto &piece : a) {
            if (piece.first != *hi) break;
            *hi += piece.n;
            if (*hi - *lo >= PACKED_MAX_UNITS) { *hi = *lo + PACKED_MAX_UNITS; break; }
        }
        return *hi > *lo;
    }
    const auto &b = m->pending[1];
    size_t i = 0, j = 0;
    bool open = false;
    while (i < a.size() && j < b.size()) {
        const int64_t from = std::max(a[i].first, b[j].first);
        const int64_t to = std::min(a[i].first + a[i].n, b[j].first + b[j].n);
        if (from < to) {
            if (!open) { *lo = from; *hi = to; open = true; }
            else if (from == *hi) *hi = to;
            else break;
            if (*hi - *lo >= PACKED_MAX_UNITS) { *hi = *lo + PACKED_MAX_UNITS; break; }
        }
        if (a[i].first + a[i].n <= b[j].first + b[j].n) ++i; else ++j;
    }
    return open;
}

// (q_mu held) forget units [lo, hi) of a stream: they have been mapped.  What a piece holds
// before `lo` (reads whose mates have not arrived yet) and after `hi` stays, sharing the block.
void packed_consume(skm_mapper *m, int stream, int64_t lo, int64_t hi)
{
    auto &list = m->pending[stream];
    std::deque<skm_mapper::Piece> kept;
    for (auto &piece : list) {
        piece.in_job = false;
        const int64_t end = piece.first + piece.n;
        if (end <= lo || piece.first >= hi) { kept.push_back(std::move(piece)); continue; }
        if (piece.first < lo) {
            skm_mapper::Piece head = piece;
            head.n = lo - piece.first;
            kept.push_back(std::move(head));
        }
        if (end > hi) {
            skm_mapper::Piece tail = piece;
            tail.first = hi;
            tail.n = end - hi;
            kept.push_back(std::move(tail));
        }
    }
    list.swap(kept);
}

// (q_mu held) nothing more can be mapped: reads without a mate go
void packed_drop_all(skm_mapper *m)
{
    for (auto &list : m->pending) {
        for (auto &piece : list) m->packed_dropped += piece.n;
        list.clear();
    }
}

struct PackedSegment {               // part of one piece inside a run
    int mate;
    int64_t first, n;                // units
    const uint64_t *codes;
    const uint32_t *lengths;
    int cw;
    uint32_t uniform_len;
    const uint32_t *exc_reads, *exc_masks;   // device, already offset to the segment's first exception
    int64_t n_exc;
    int64_t exc_base;                // index (relative to the piece as pushed) of the segment's first read
};

// the parts of a stream's pieces that lie in units [lo, hi), as segments of a launch
void packed_segments(std::deque<skm_mapper::Piece> &pieces, int mate, int64_t lo, int64_t hi, bool mark_in_job,
                     std::vector<PackedSegment> *segments, int *max_cw)
{
    for (auto &piece : pieces) {
        const int64_t from = std::max(lo, piece.first), to = std::min(hi, piece.first + piece.n);
        if (from >= to) continue;
        if (mark_in_job) piece.in_job = true;
        PackedSegment seg{};
        seg.mate = mate;
        seg.first = from;
        seg.n = to - from;
        const int64_t skip = from - piece.origin;
        seg.codes = piece.codes + skip * piece.cw;
        seg.lengths = piece.lengths ? piece.lengths + skip : nullptr;
        seg.cw = piece.cw;
        seg.uniform_len = (uint32_t)std::max<int64_t>(piece.uniform_len, 0);
        const auto e0 = std::lower_bound(piece.exc_reads.begin(), piece.exc_reads.end(), (uint32_t)skip);
        const auto e1 = std::lower_bound(piece.exc_reads.begin(), piece.exc_reads.end(), (uint32_t)(skip + seg.n));
        seg.n_exc = e1 - e0;
        const int64_t at = e0 - piece.exc_reads.begin();
        seg.exc_reads = piece.exc_reads_dev + at;
        seg.exc_masks = piece.exc_masks + at * piece.cw;
        seg.exc_base = skip;
        *max_cw = std::max(*max_cw, piece.cw);
        segments->push_back(seg);
    }
}

int run_packed_job(skm_mapper *m, int64_t lo, int64_t hi, int paired, const std::vector<PackedSegment> &segments,
                   int max_cw)
{
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int mates = paired ? 2 : 1;
    if (!m->packed_sized && m->expected_units > 0) {
        // Runs grow with what has arrived (a few ten thousand units, then hundreds of thousands, then
        // PACKED_MAX_UNITS): sized run by run, every batch buffer is allocated three or four times in
        // a sample's first milliseconds.  Size them for the largest run of the announced sample once.
        const int64_t most = std::max<int64_t>(hi - lo, std::min(m->expected_units, PACKED_MAX_UNITS));
        const int words = max_cw + 1, record_words = ((3 * words + 1 + 15) / 16) * 16;
        SKM_TRY(m->records.ensure((size_t)most * mates * record_words + 16));
        SKM_TRY(m->rec_unit.ensure(most)); SKM_TRY(m->rec_tuple.ensure(most));
        SKM_TRY(m->unit_slot.ensure(most)); SKM_TRY(m->rec_key.ensure(most));
        SKM_TRY(m->unit_entries.ensure((size_t)most * 8 + (size_t)m->ix->cu_count * MAP_BLOCKS_PER_CU * (MAP_THREADS / 64) * 2048 + 4096));
        if (m->host_classes == 0) SKM_TRY(table_reserve_for_sample(m, m->expected_units));
        m->packed_sized = true;
    }
    const RecordStage fill = [&](uint32_t *records, int words, int record_words) -> int {
        for (const PackedSegment &seg : segments) {
            uint32_t *dst = records + ((seg.first - lo) * mates + seg.mate) * (int64_t)record_words;
            launch_unpack_reads(seg.codes, seg.cw, seg.cw, seg.lengths, seg.uniform_len, seg.n, words, dst,
                                (int64_t)mates * record_words, m->error.p, m->stream);
            if (seg.n_exc)
                launch_unpack_exceptions(seg.exc_reads, seg.exc_masks, seg.n_exc, seg.cw, seg.exc_base, words, dst,
                                         (int64_t)mates * record_words, m->stream);
        }
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    return map_batch_resident(m, nullptr, nullptr, hi - lo, paired, max_cw * 32, lo, &fill);
}

void worker_main(skm_mapper *m)
{
    for (;;) {
        skm_mapper::Job job;
        bool packed = false;
        int64_t lo = 0, hi = 0;
        int paired = 0, max_cw = 1;
        std::vector<PackedSegment> segments;
        {
            std::unique_lock<std::mutex> hold(m->q_mu);
            for (;;) {
                if (!m->jobs.empty()) break;
                if (m->job_error != SKM_OK && (!m->pending[0].empty() || !m->pending[1].empty())) {
                    packed_drop_all(m);         // after a failure the table is not to be trusted
                    m->done_cv.notify_all();
                }
                // (a pusher that waits at the byte limit may be the only one who could make the run
                // longer: its presence maps whatever run there is, as a flush does)
                if (packed_find_run(m, &lo, &hi)
                        && (hi - lo >= PACKED_MIN_UNITS || m->packed_flush || m->packed_waiters || m->stop)) {
                    packed = true;
                    break;
                }
                if (m->stop) {                  // stop requested and nothing left to map
                    packed_drop_all(m);
                    return;
                }
                m->q_cv.wait(hold);
            }
            if (!packed) {
                job = m->jobs.front();
                m->jobs.pop_front();
            } else {
                paired = m->packed_paired == 1;
                for (int s = 0; s < (paired ? 2 : 1); ++s)
                    packed_segments(m->pending[s], s, lo, hi, true, &segments, &max_cw);
                m->packed_busy = true;
            }
        }
        int rc = SKM_OK;
        std::string message;
        if (packed) {
            rc = run_packed_job(m, lo, hi, paired, segments, max_cw);
            if (rc != SKM_OK) {
                message = last_message();
                // kernels that read the pieces' blocks may still be queued: nothing is handed back
                // to the pool (and from there to the next pusher's copy) before the stream has drained
                (void)hipStreamSynchronize(m->stream);
            }
            {
                std::lock_guard<std::mutex> hold(m->q_mu);
                if (rc != SKM_OK && m->job_error == SKM_OK) {
                    m->job_error = rc;
                    m->job_error_ticket = 0;              // (reported by every wait)
                    m->job_error_msg = message;
                }
                for (int s = 0; s < (paired ? 2 : 1); ++s) packed_consume(m, s, lo, hi);
                m->packed_busy = false;
            }
            m->done_cv.notify_all();
            continue;
        }
        bool skip;
        {
            std::lock_guard<std::mutex> hold(m->q_mu);
            skip = m->job_error != SKM_OK;        // after a failure the table is not to be trusted
        }
        if (!skip) {
            rc = run_job(m, job);
            if (rc != SKM_OK) message = last_message();  // (this thread's message)
        }
        {
            std::lock_guard<std::mutex> hold(m->q_mu);
            if (rc != SKM_OK && m->job_error == SKM_OK) {
                m->job_error = rc;
                m->job_error_ticket = job.ticket;
                m->job_error_msg = message;
            }
            m->lanes[job.lane].busy = false;
            m->done_ticket = job.ticket;
        }
        m->done_cv.notify_all();
    }
}

// wait until every queued batch up to `ticket` has been mapped (0 = all of them AND every packed
// read whose mate has arrived; reads still without one keep waiting in HBM -- another thread may be
// about to push their mates -- until skm_mapper_reset / _clear / _destroy); reports (and, with
// `consume`, forgets) the first failure among them
int wait_jobs(skm_mapper *m, uint64_t ticket, bool consume)
{
    std::unique_lock<std::mutex> hold(m->q_mu);
    const uint64_t upto = ticket ? ticket : m->next_ticket - 1;
    m->done_cv.wait(hold, [&] { return m->done_ticket >= upto; });
    if (ticket == 0 && (m->packed_busy || !m->pending[0].empty() || !m->pending[1].empty())) {
        m->packed_flush++;
        m->q_cv.notify_all();
        m->done_cv.wait(hold, [&] {
            int64_t lo, hi;
            return !m->packed_busy && (m->job_error != SKM_OK || !packed_find_run(m, &lo, &hi));
        });
        m->packed_flush--;
    }
    if (m->job_error != SKM_OK && m->job_error_ticket <= upto) {
        const int rc = m->job_error;
        const std::string message = m->job_error_msg;
        if (consume) { m->job_error = SKM_OK; m->job_error_ticket = 0; m->job_error_msg.clear(); }
        set_message(message);
        return rc;
    }
    return SKM_OK;
}

// offsets == nullptr: every read is `uniform_len` bases long (the offsets are then made on the device)
int submit_batch(skm_mapper *m, const char *bases, const int64_t *offsets, int64_t uniform_len, int64_t n_units,
                 int paired, int64_t first_unit, uint64_t *ticket_out)
{
    if (!m || n_units < 0 || (!offsets && uniform_len < 0)) return fail(SKM_ERR_ARG, "bad argument");
    if (n_units > 0 && !bases) return fail(SKM_ERR_ARG, "bases is NULL");
    if (n_units >= (1LL << 31)) return fail(SKM_ERR_ARG, "more than 2^31 - 1 units in one batch");
    if (!offsets && uniform_len > (1 << 20)) return fail(SKM_ERR_ARG, "read longer than 2^20 bases");
    SKM_TRY(set_device(m->ix->device));
    const int64_t n_reads = paired ? 2 * n_units : n_units;
    const int64_t first_byte = offsets ? offsets[0] : 0;
    const int64_t n_bytes = offsets ? offsets[n_reads] - offsets[0] : n_reads * uniform_len;
    if (n_bytes < 0) return fail(SKM_ERR_ARG, "offsets are not monotone");
    // a free lane (at most N_LANES batches are in HBM at a time: one being mapped, others copied)
    int li = -1;
    {
        std::unique_lock<std::mutex> hold(m->q_mu);
        if (!m->worker_started) {
            m->worker = std::thread(worker_main, m);
            m->worker_started = true;
        }
        m->done_cv.wait(hold, [&] {
            for (int i = 0; i < skm_mapper::N_LANES; ++i) if (!m->lanes[i].busy) { li = i; return true; }
            return false;
        });
        m->lanes[li].busy = true;
    }
    skm_mapper::Lane &lane = m->lanes[li];
    auto release = on_exit([&]() {
        { std::lock_guard<std::mutex> hold(m->q_mu); lane.busy = false; }
        m->done_cv.notify_all();
    });
    if (!lane.stream) HIP_TRY(hipStreamCreateWithFlags(lane.stream.out(), hipStreamNonBlocking));
    SKM_TRY(lane.bases.ensure((size_t)n_bytes + 64));
    SKM_TRY(lane.offsets.ensure((size_t)n_reads + 1));
    // pinned sources go over the link at full rate and asynchronously; pageable ones are staged
    // by the runtime.  Either way the source is free again when this call returns.
    if (n_bytes)
        HIP_TRY(hipMemcpyAsync(lane.bases.p, bases + first_byte, (size_t)n_bytes, hipMemcpyHostToDevice, lane.stream));
    if (offsets)
        HIP_TRY(hipMemcpyAsync(lane.offsets.p, offsets, (size_t)(n_reads + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                               lane.stream));
    else
        launch_offsets_uniform(lane.offsets.p, n_reads, uniform_len, lane.stream);
    HIP_TRY(hipStreamSynchronize(lane.stream));
    uint64_t ticket;
    {
        std::lock_guard<std::mutex> hold(m->q_mu);
        ticket = m->next_ticket++;
        m->jobs.push_back(skm_mapper::Job{li, n_units, paired, first_byte, first_unit, ticket});
    }
    release.dismiss();
    m->q_cv.notify_one();
    if (ticket_out) *ticket_out = ticket;
    return SKM_OK;
}

}  // namespace

extern "C" int skm_mapper_map_batch_async(skm_mapper *m, const char *bases, const int64_t *offsets,
                                          int64_t n_units, int paired, int64_t first_unit)
{
    if (!offsets) return fail(SKM_ERR_ARG, "offsets is NULL");
    return submit_batch(m, bases, offsets, -1, n_units, paired, first_unit, nullptr);
}

extern "C" int skm_mapper_map_batch_uniform_async(skm_mapper *m, const char *bases, int32_t read_len,
                                                  int64_t n_units, int paired, int64_t first_unit)
{
    if (read_len < 0) return fail(SKM_ERR_ARG, "negative read length");
    return submit_batch(m, bases, nullptr, read_len, n_units, paired, first_unit, nullptr);
}

extern "C" int skm_mapper_expect_units(skm_mapper *m, int64_t n_units)
{
    if (!m || n_units < 0) return fail(SKM_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lock(m->mu);          // (run_packed_job reads them under it)
    m->expected_units = n_units;
    m->packed_sized = false;
    return SKM_OK;
}

extern "C" int skm_mapper_sync(skm_mapper *m)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    return wait_jobs(m, 0, true);
}

namespace {

// A piece on its way into the mapper: `stage` checks it, waits at the byte limit, takes a block of HBM
// and QUEUES the copies on the mapper's copy stream (*staged = false: a cut or an empty piece, dealt
// with on the spot); `commit` -- once the copies have completed -- makes the piece visible to the worker.
int packed_stage(skm_mapper *m, const skm_packed_reads *piece, int paired, skm_mapper::Piece *out, bool *staged);
int packed_commit(skm_mapper *m, skm_mapper::Piece &&held, int stream_index);

}  // namespace

extern "C" int skm_mapper_push_packed(skm_mapper *m, const skm_packed_reads *piece, int paired)
{
    if (!m || !piece) return fail(SKM_ERR_ARG, "NULL argument");
    skm_mapper::Piece held;
    bool staged = false;
    SKM_TRY(packed_stage(m, piece, paired, &held, &staged));
    if (!staged) return SKM_OK;
    HIP_TRY(hipStreamSynchronize(m->packed_stream));        // (the caller's arrays are free again)
    return packed_commit(m, std::move(held), piece->stream);
}

namespace {

// the arrays of a piece that holds reads
int packed_check_arrays(const skm_packed_reads *piece)
{
    const int64_t n = piece->n_reads;
    const int cw = piece->code_words;
    if (cw < 1 || cw > (1 << 15) || piece->read_stride < cw || !piece->codes) return fail(SKM_ERR_ARG, "bad code words");
    if (piece->uniform_len < 0 && !piece->lengths) return fail(SKM_ERR_ARG, "lengths is NULL");
    if (piece->uniform_len > 32LL * cw) return fail(SKM_ERR_ARG, "reads of %lld bases in %d code words", (long long)piece->uniform_len, cw);
    const int64_t n_exc = piece->n_exceptions;
    if (n_exc < 0 || n_exc > n || (n_exc > 0 && (!piece->exception_reads || !piece->exception_masks)))
        return fail(SKM_ERR_ARG, "bad exception list");
    for (int64_t e = 0; e < n_exc; ++e)
        if (piece->exception_reads[e] >= (uint64_t)n || (e && piece->exception_reads[e] <= piece->exception_reads[e - 1]))
            return fail(SKM_ERR_ARG, "exception reads must ascend and lie inside the piece");
    return SKM_OK;
}

// A piece's one HBM block: codes | lengths | exception reads | exception bit planes
size_t packed_round(size_t b) { return (b + 255) & ~(size_t)255; }
int64_t packed_block_bytes(const skm_packed_reads *piece)
{
    const size_t n = (size_t)piece->n_reads, cw = (size_t)piece->code_words, n_exc = (size_t)piece->n_exceptions;
    return (int64_t)(packed_round(n * cw * 8) + (piece->uniform_len >= 0 ? 0 : packed_round(n * 4)) + packed_round(n_exc * 4)
                     + packed_round(n_exc * cw * 4) + 256);
}

// take the block (counted in *counter while it lives) and QUEUE the copies of the piece's arrays on `stream`
int packed_upload(const skm_packed_reads *piece, const std::shared_ptr<std::atomic<int64_t>> &counter, hipStream_t stream,
                  skm_mapper::Piece *out)
{
    const int64_t n = piece->n_reads, n_exc = piece->n_exceptions;
    const int cw = piece->code_words;
    const bool uniform = piece->uniform_len >= 0;
    const size_t codes_bytes = packed_round((size_t)n * cw * 8);
    const size_t len_bytes = uniform ? 0 : packed_round((size_t)n * 4);
    const size_t exc_bytes = packed_round((size_t)n_exc * 4);
    const int64_t block_bytes = packed_block_bytes(piece);
    char *raw = nullptr;
    HIP_TRY(pool_alloc((void **)&raw, (size_t)block_bytes));
    skm_mapper::Piece &held = *out;
    counter->fetch_add(block_bytes);       // (the counter outlives its owner if a block does)
    held.block = std::shared_ptr<char>(raw, [counter, block_bytes](char *q) { pool_free(q); counter->fetch_sub(block_bytes); });
    held.first = held.origin = piece->first_read;
    held.n = n;
    held.cw = cw;
    held.uniform_len = uniform ? piece->uniform_len : -1;
    held.codes = (uint64_t *)raw;
    held.lengths = uniform ? nullptr : (uint32_t *)(raw + codes_bytes);
    held.exc_reads_dev = (uint32_t *)(raw + codes_bytes + len_bytes);
    held.exc_masks = (uint32_t *)(raw + codes_bytes + len_bytes + exc_bytes);
    if (n_exc) held.exc_reads.assign(piece->exception_reads, piece->exception_reads + n_exc);
    if (piece->read_stride == cw)
        HIP_TRY(hipMemcpyAsync(held.codes, piece->codes, (size_t)n * cw * 8, hipMemcpyHostToDevice, stream));
    else
        HIP_TRY(hipMemcpy2DAsync(held.codes, (size_t)cw * 8, piece->codes, (size_t)piece->read_stride * 8, (size_t)cw * 8,
                                 (size_t)n, hipMemcpyHostToDevice, stream));
    if (!uniform) HIP_TRY(hipMemcpyAsync(held.lengths, piece->lengths, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    if (n_exc) {
        HIP_TRY(hipMemcpyAsync(held.exc_reads_dev, piece->exception_reads, (size_t)n_exc * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(held.exc_masks, piece->exception_masks, (size_t)n_exc * cw * 4, hipMemcpyHostToDevice, stream));
    }
    return SKM_OK;
}

int packed_stage(skm_mapper *m, const skm_packed_reads *piece, int paired, skm_mapper::Piece *out, bool *staged)
{
    *staged = false;
    const int64_t n = piece->n_reads;
    const int cw = piece->code_words;
    if (n < 0 || n >= (1LL << 31) || piece->first_read < 0) return fail(SKM_ERR_ARG, "bad piece: %lld reads from %lld", (long long)n, (long long)piece->first_read);
    if (piece->stream < 0 || piece->stream > (paired ? 1 : 0)) return fail(SKM_ERR_ARG, "stream %d of a %s sample", piece->stream, paired ? "paired" : "single-ended");
    if (n == 0 && cw == SKM_PACKED_CUT) {
        // a cut: the stream's reads from first_read on are dropped (the longer file of a pair of
        // files, seekmer/common.py:180-197: zip() ends at the shorter one).  The run the worker may
        // be mapping from the same piece ends where both streams had reads, i.e. at or below the cut.
        std::unique_lock<std::mutex> hold(m->q_mu);
        auto &list = m->pending[piece->stream];
        const int64_t from = piece->first_read;
        m->done_cv.wait(hold, [&] {
            if (!m->packed_busy) return true;
            for (const auto &other : list)
                if (other.in_job && other.first + other.n > from) return false;
            return true;
        });
        while (!list.empty() && list.back().first >= from) { m->packed_dropped += list.back().n; list.pop_back(); }
        if (!list.empty() && list.back().first + list.back().n > from) {
            m->packed_dropped += list.back().first + list.back().n - from;
            list.back().n = from - list.back().first;
        }
        return SKM_OK;
    }
    if (n == 0) return SKM_OK;
    SKM_TRY(packed_check_arrays(piece));
    SKM_TRY(set_device(m->ix->device));
    {
        std::lock_guard<std::mutex> hold(m->q_mu);
        if (m->packed_paired >= 0 && m->packed_paired != (paired ? 1 : 0) && (!m->pending[0].empty() || !m->pending[1].empty() || m->packed_busy))
            return fail(SKM_ERR_STATE, "paired and single-ended pieces in one run");
        m->packed_paired = paired ? 1 : 0;
        if (!m->packed_stream) HIP_TRY(hipStreamCreateWithFlags(m->packed_stream.out(), hipStreamNonBlocking));
    }
    const int64_t block_bytes = packed_block_bytes(piece);
    {
        std::unique_lock<std::mutex> hold(m->q_mu);
        auto may_go = [&] {
            if (m->packed_bytes->load() + block_bytes <= m->packed_max_pending || m->job_error != SKM_OK) return true;
            int64_t lo, hi;
            return !(m->packed_busy || packed_find_run(m, &lo, &hi));     // nothing the worker could free
        };
        if (!may_go()) {
            m->packed_waiters++;                  // the worker now maps runs below PACKED_MIN_UNITS too
            m->q_cv.notify_all();
            m->done_cv.wait(hold, may_go);
            m->packed_waiters--;
        }
    }
    SKM_TRY(packed_upload(piece, m->packed_bytes, m->packed_stream, out));
    *staged = true;
    return SKM_OK;
}

int packed_commit(skm_mapper *m, skm_mapper::Piece &&held, int stream_index)
{
    {
        std::unique_lock<std::mutex> hold(m->q_mu);
        if (!m->worker_started) {
            m->worker = std::thread(worker_main, m);
            m->worker_started = true;
        }
        auto &list = m->pending[stream_index];
        // a piece that overlaps what its stream holds replaces the reads from its first one on
        auto overlapping = [&] {
            for (const auto &other : list)
                if (other.first < held.first + held.n && held.first < other.first + other.n) return true;
            return false;
        };
        bool overlaps = overlapping();
        if (overlaps) {
            // a piece the worker is mapping from right now (the longer file of a pair of unequal
            // length: its leftover reads are what this piece replaces): the run in flight ends where
            // both streams had reads, so waiting for it leaves only the leftover to cut off -- the
            // outcome does not depend on when the worker took the run
            auto in_flight = [&] {
                for (const auto &other : list)
                    if (other.in_job && other.first + other.n > held.first) return true;
                return false;
            };
            m->done_cv.wait(hold, [&] { return !m->packed_busy || !in_flight(); });
            for (const auto &other : list)
                if (other.first < held.first && other.first + other.n > held.first && other.in_job)
                    return fail(SKM_ERR_STATE, "a piece replaces reads that are being mapped");
            overlaps = overlapping();
        }
        if (overlaps) {
            while (!list.empty() && list.back().first >= held.first) list.pop_back();
            if (!list.empty() && list.back().first + list.back().n > held.first) list.back().n = held.first - list.back().first;
            list.push_back(std::move(held));
        } else {
            size_t at = list.size();
            while (at > 0 && list[at - 1].first > held.first) --at;
            list.insert(list.begin() + (long)at, std::move(held));
        }
    }
    m->q_cv.notify_all();
    return SKM_OK;
}

}  // namespace

extern "C" int skm_mapper_map_packed_source(skm_mapper *m, skm_packed_source next, void *context, int paired,
                                            int64_t *n_pieces)
{
    if (!m || !next) return fail(SKM_ERR_ARG, "NULL argument");
    if (n_pieces) *n_pieces = 0;
    // The copy of piece k runs while the source is asked for piece k + 1 (a source keeps a piece's
    // arrays valid through ONE more call, include/seekmer_hip.h): the drain loop -- one thread --
    // paid every piece's copy time in full before (524 pieces x 25 us of a 42 ms pass).
    SKM_TRY(set_device(m->ix->device));
    hipEvent_t copied[2] = {nullptr, nullptr};
    skm_mapper::Piece waiting;
    bool have_waiting = false;
    auto undo = on_exit([&]() {
        // (an early return with a copy still queued: its block goes back to the pool with `waiting`)
        if (have_waiting) (void)hipStreamSynchronize(m->packed_stream);
        for (auto &e : copied) pool_event_release(e, false);
    });
    for (auto &e : copied) HIP_TRY(pool_event_acquire(&e, false));
    int waiting_stream = 0, turn = 0;
    auto land = [&]() -> int {                   // the piece whose copy was queued a call ago joins its stream
        if (!have_waiting) return SKM_OK;
        have_waiting = false;
        HIP_TRY(hipEventSynchronize(copied[turn ^ 1]));
        return packed_commit(m, std::move(waiting), waiting_stream);
    };
    for (;;) {
        skm_packed_reads piece;
        memset(&piece, 0, sizeof(piece));
        const int rc = next(context, &piece);
        if (rc != SKM_OK) { (void)land(); return fail(rc, "the source of packed reads failed (%d)", rc); }
        if (piece.n_reads == 0 && piece.code_words != SKM_PACKED_CUT) return land();
        if (piece.n_reads == 0) SKM_TRY(land());         // a cut applies behind everything that came before it
        skm_mapper::Piece held;
        bool staged = false;
        const int staged_rc = packed_stage(m, &piece, paired, &held, &staged);
        if (staged_rc != SKM_OK) { (void)land(); return staged_rc; }
        if (staged) HIP_TRY(hipEventRecord(copied[turn], m->packed_stream));
        SKM_TRY(land());
        if (staged) {
            waiting = std::move(held);
            waiting_stream = piece.stream;
            have_waiting = true;
            turn ^= 1;
        }
        if (n_pieces) ++*n_pieces;
    }
}

extern "C" int skm_mapper_map_batch(skm_mapper *m, const char *bases, const int64_t *offsets,
                                    int64_t n_units, int paired)
{
    uint64_t ticket = 0;
    if (!offsets) return fail(SKM_ERR_ARG, "offsets is NULL");
    SKM_TRY(submit_batch(m, bases, offsets, -1, n_units, paired, -1, &ticket));
    return wait_jobs(m, ticket, true);
}

extern "C" int skm_mapper_map_batch_device(skm_mapper *m, const void *d_bases, const void *d_offsets,
                                           int64_t n_units, int paired, int32_t max_read_len)
{
    if (!m || !d_offsets || n_units < 0 || max_read_len < 0)
        return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    return map_batch_resident(m, (const uint8_t *)d_bases, (const int64_t *)d_offsets, n_units,
                              paired, max_read_len);
}

extern "C" int skm_mapper_last_batch(skm_mapper *m, int32_t *begin, int32_t *end,
                                     int32_t *anchor_entry, int32_t *anchor_offset, int32_t *counts,
                                     int32_t *entries, int64_t cap_entries, int64_t *n_entries)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t n = m->last_units;
    if (n_entries) *n_entries = 0;
    if (n == 0) return SKM_OK;
    if ((begin || end || anchor_entry || anchor_offset) && !m->last_spans)
        return fail(SKM_ERR_STATE, "the spans of the last batch were not kept: call skm_mapper_keep_spans(mapper, 1) before mapping");
    if (begin) HIP_TRY(hipMemcpy(begin, m->unit_begin.p, n * 4, hipMemcpyDeviceToHost));
    if (end) HIP_TRY(hipMemcpy(end, m->unit_end.p, n * 4, hipMemcpyDeviceToHost));
    if (anchor_entry || anchor_offset) {
        std::vector<Coord> a(n);
        HIP_TRY(hipMemcpy(a.data(), m->unit_anchor.p, n * sizeof(Coord), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            if (anchor_entry) anchor_entry[i] = a[i].entry;
            if (anchor_offset) anchor_offset[i] = a[i].offset;
        }
    }
    if (!counts && !entries && !n_entries) return SKM_OK;
    // the records of the batch (emission order) -> per unit
    std::vector<int32_t> unit(n);
    std::vector<unsigned long long> tuple(n);
    HIP_TRY(hipMemcpy(unit.data(), m->rec_unit.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tuple.data(), m->rec_tuple.p, n * 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> cnt(n, 0);
    std::vector<int64_t> off(n, 0);
    std::vector<char> seen(n, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t u = unit[r];
        if (u < 0 || u >= n || seen[u]) return fail(SKM_ERR_STATE, "record %lld names unit %lld", (long long)r, (long long)u);
        seen[u] = 1;
        cnt[u] = (int32_t)(tuple[r] >> 40);
        off[u] = (int64_t)(tuple[r] & ((1ULL << 40) - 1));
    }
    if (counts) memcpy(counts, cnt.data(), n * 4);
    if (n_entries) {
        int64_t total = 0;
        for (int64_t u = 0; u < n; ++u) total += cnt[u];
        *n_entries = total;           // the arena itself has per-wave slack
    }
    if (entries) {
        std::vector<int32_t> raw((size_t)std::max<int64_t>(m->last_ids, 1));
        if (m->last_ids)
            HIP_TRY(hipMemcpy(raw.data(), m->unit_entries.p, (size_t)m->last_ids * 4, hipMemcpyDeviceToHost));
        int64_t pos = 0;
        for (int64_t u = 0; u < n; ++u) {
            for (int i = 0; i < cnt[u]; ++i)
                if (pos + i < cap_entries) entries[pos + i] = raw[off[u] + i];
            pos += cnt[u];
        }
    }
    return SKM_OK;
}

extern "C" int skm_mapper_copy_records(skm_mapper *m, int64_t first_read, int64_t n_reads, uint32_t *out,
                                       int32_t *record_words, int32_t *words_per_read)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    if (m->last_reads == 0) return fail(SKM_ERR_STATE, "no batch has been mapped since the handle was made or reset");
    if (first_read < 0 || n_reads < 0 || first_read > m->last_reads || n_reads > m->last_reads - first_read)
        return fail(SKM_ERR_ARG, "reads %lld .. +%lld of a batch of %lld", (long long)first_read, (long long)n_reads,
                    (long long)m->last_reads);
    if (record_words) *record_words = m->last_record_words;
    if (words_per_read) *words_per_read = m->last_words;
    if (out && n_reads) {
        HIP_TRY(hipStreamSynchronize(m->stream));
        HIP_TRY(hipMemcpy(out, m->records.p + first_read * (int64_t)m->last_record_words,
                          (size_t)n_reads * m->last_record_words * 4, hipMemcpyDeviceToHost));
    }
    return SKM_OK;
}

extern "C" int skm_pack_stage_reads(int32_t words_per_read, int32_t *reads_per_block)
{
    if (words_per_read < 1 || !reads_per_block) return fail(SKM_ERR_ARG, "bad argument");
    *reads_per_block = pack_stage_reads(words_per_read);
    return SKM_OK;
}

extern "C" int skm_mapper_keep_spans(skm_mapper *m, int enable)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    m->keep_spans = enable != 0;
    return SKM_OK;
}

extern "C" int skm_mapper_set_strand(skm_mapper *m, int mode)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    if (mode != SKM_STRAND_NONE && mode != SKM_STRAND_FR && mode != SKM_STRAND_RF)
        return fail(SKM_ERR_ARG, "unknown strand mode %d", mode);
    (void)wait_jobs(m, 0, false);
    bool queued;
    {
        std::lock_guard<std::mutex> hold(m->q_mu);
        queued = !m->jobs.empty() || m->packed_busy || !m->pending[0].empty() || !m->pending[1].empty();
    }
    std::lock_guard<std::mutex> lock(m->mu);
    if (queued || m->units_done != 0)
        return fail(SKM_ERR_STATE, "the strand mode can only change on an empty mapper (new, or after "
                                   "skm_mapper_reset / skm_mapper_clear)");
    m->strand = mode;
    return SKM_OK;
}

extern "C" int skm_mapper_set_bias(skm_mapper *m, int enable)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, false);
    bool queued;
    {
        std::lock_guard<std::mutex> hold(m->q_mu);
        queued = !m->jobs.empty() || m->packed_busy || !m->pending[0].empty() || !m->pending[1].empty();
    }
    std::lock_guard<std::mutex> lock(m->mu);
    if (queued || m->units_done != 0)
        return fail(SKM_ERR_STATE, "hexamer counting can only change on an empty mapper (new, or after "
                                   "skm_mapper_reset / skm_mapper_clear)");
    if (enable) {
        SKM_TRY(set_device(m->ix->device));
        SKM_TRY(m->bias_observed.ensure(BIAS_BINS));
        HIP_TRY(hipMemsetAsync(m->bias_observed.p, 0, BIAS_BINS * sizeof(unsigned long long), m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    m->bias = enable != 0;
    return SKM_OK;
}

extern "C" int skm_mapper_bias_observed(skm_mapper *m, int64_t out[4096])
{
    if (!m || !out) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->bias) return fail(SKM_ERR_STATE, "this mapper does not count hexamers: call skm_mapper_set_bias(mapper, 1) before mapping");
    SKM_TRY(set_device(m->ix->device));
    HIP_TRY(hipMemcpy(out, m->bias_observed.p, BIAS_BINS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SKM_OK;
}

namespace {

// the weights of a fragment-length model: every one finite and >= 0 (checked on the host, before any device work)
bool length_weights_valid(const double *p, int64_t count)
{
    for (int64_t i = 0; i < count; ++i)
        if (!(p[i] >= 0.0) || std::isinf(p[i])) return false;
    return true;
}

}  // namespace

extern "C" int skm_mapper_set_length_weights(skm_mapper *m, const double *p)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    if (p && !length_weights_valid(p, MAX_FRAGMENT_LENGTH))
        return fail(SKM_ERR_ARG, "a fragment-length weight is negative or not finite");
    SKM_TRY(wait_jobs(m, 0, false));
    std::lock_guard<std::mutex> lock(m->mu);
    if (!p) {
        m->use_length_weights = false;
        return SKM_OK;
    }
    SKM_TRY(set_device(m->ix->device));
    SKM_TRY(m->length_weights.ensure(MAX_FRAGMENT_LENGTH));
    // (no quantification call is under way: they hold mu until their stream has drained)
    HIP_TRY(hipMemcpy(m->length_weights.p, p, MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
    m->use_length_weights = true;
    return SKM_OK;
}

extern "C" int skm_mapper_summary(skm_mapper *m, int64_t summary[4])
{
    if (!m || !summary) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    unsigned long long ctr[4];
    HIP_TRY(hipMemcpy(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));
    summary[0] = (int64_t)ctr[CTR_CLASSES];
    summary[1] = (int64_t)ctr[CTR_ARENA];
    summary[2] = (int64_t)ctr[CTR_UNALIGNED];
    summary[3] = (int64_t)ctr[CTR_UNITS];
    return SKM_OK;
}

extern "C" int skm_mapper_export(skm_mapper *m, int64_t *class_offsets, int32_t *class_targets,
                                 int64_t *class_counts, int64_t *first_seen, int64_t *fld)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    if (fld)
        HIP_TRY(hipMemcpy(fld, m->counters.p + CTR_FLD, MAX_FRAGMENT_LENGTH * 8, hipMemcpyDeviceToHost));
    if (!class_offsets && !class_targets && !class_counts && !first_seen) return SKM_OK;
    const int64_t C = m->host_classes, M = m->host_arena_used;
    if (class_offsets) class_offsets[0] = 0;
    if (C == 0) return SKM_OK;
    DBuf<int64_t> d_off, d_len; DBuf<double> d_cnt; DBuf<unsigned long long> d_fs;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
    SKM_TRY(d_off.ensure(C)); SKM_TRY(d_len.ensure(C)); SKM_TRY(d_cnt.ensure(C)); SKM_TRY(d_fs.ensure(C));
    launch_class_compact(m->t, C, d_off.p, d_len.p, d_cnt.p, d_fs.p, m->stream);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> off(C), len(C);
    std::vector<double> cnt(C);
    std::vector<unsigned long long> fs(C);
    std::vector<int32_t> arena((size_t)std::max<int64_t>(M, 1));
    HIP_TRY(hipMemcpyAsync(off.data(), d_off.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(len.data(), d_len.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(fs.data(), d_fs.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    if (M) HIP_TRY(hipMemcpyAsync(arena.data(), m->arena.p, (size_t)M * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    drain.dismiss();
    // Counter insertion order under -j1 = ascending first-seen unit (mapper.py:88)
    std::vector<int64_t> order(C);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return fs[a] < fs[b]; });
    int64_t pos = 0;
    for (int64_t k = 0; k < C; ++k) {
        const int64_t c = order[k];
        if (class_targets)
            memcpy(class_targets + pos, arena.data() + off[c], (size_t)len[c] * 4);
        pos += len[c];
        if (class_offsets) class_offsets[k + 1] = pos;
        if (class_counts) class_counts[k] = (int64_t)cnt[c];
        if (first_seen) first_seen[k] = (int64_t)fs[c];
    }
    return SKM_OK;
}

extern "C" int skm_mapper_merge(skm_mapper *m, int64_t n_classes, const int64_t *class_offsets,
                                const int32_t *class_targets, const int64_t *class_counts,
                                const int64_t *first_seen, int64_t unaligned, const int64_t *fld)
{
    if (!m || n_classes < 0 || unaligned < 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (!class_offsets || !class_targets || !class_counts || !first_seen))
        return fail(SKM_ERR_ARG, "NULL class arrays");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    m->host_totals_valid = false;             // (the totals change on the device below)
    SKM_TRY(set_device(m->ix->device));
    std::vector<unsigned long long> add(CTR_WORDS, 0);
    int64_t units = unaligned;
    for (int64_t c = 0; c < n_classes; ++c) units += class_counts[c];
    add[CTR_UNALIGNED] = (unsigned long long)unaligned;
    add[CTR_UNITS] = (unsigned long long)units;
    if (fld) for (int i = 0; i < MAX_FRAGMENT_LENGTH; ++i) add[CTR_FLD + i] = (unsigned long long)fld[i];
    if (n_classes) {
        const int64_t M = class_offsets[n_classes];
        {   // foreign classes may all be new: size for them at load <= 0.5, unbounded probes
            uint64_t want = 1 << 16;
            while ((double)want * 0.5 < (double)(m->host_classes + n_classes + 1024)) want <<= 1;
            SKM_TRY(table_grow(m, want, 0));
            SKM_TRY(m->class_list.ensure((size_t)(m->host_classes + n_classes + 1024), true, m->stream));
        }
        SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + M + 1024), true, m->stream));
        bind_table(m, m->t.slot_mask + 1);
        DBuf<int64_t> d_off, d_cnt, d_fs; DBuf<int32_t> d_ids;
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
        SKM_TRY(d_off.ensure(n_classes + 1)); SKM_TRY(d_cnt.ensure(n_classes));
        SKM_TRY(d_fs.ensure(n_classes)); SKM_TRY(d_ids.ensure(std::max<int64_t>(M, 1)));
        HIP_TRY(hipMemcpy(d_off.p, class_offsets, (n_classes + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_cnt.p, class_counts, n_classes * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_fs.p, first_seen, n_classes * 8, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(d_ids.p, class_targets, M * 4, hipMemcpyHostToDevice));
        launch_class_merge(m->t, n_classes, d_off.p, d_ids.p, d_cnt.p, d_fs.p, m->stream);
        HIP_TRY(hipGetLastError());
        unsigned long long ctr[8];
        HIP_TRY(hipMemcpyAsync(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
        SKM_TRY(read_error(m));
        drain.dismiss();                      // (read_error has synchronised the stream)
        m->host_arena_used = (int64_t)ctr[CTR_ARENA];
        m->host_classes = (int64_t)ctr[CTR_CLASSES];
    }
    // totals and histogram only once the classes are in: a failed merge leaves them untouched
    std::vector<unsigned long long> cur(CTR_WORDS);
    HIP_TRY(hipMemcpy(cur.data(), m->counters.p, CTR_WORDS * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < CTR_WORDS; ++i) cur[i] += add[i];
    HIP_TRY(hipMemcpy(m->counters.p, cur.data(), CTR_WORDS * 8, hipMemcpyHostToDevice));
    m->units_done += units;
    for (int64_t c = 0; c < n_classes; ++c)
        m->first_seen_bound = std::max(m->first_seen_bound, first_seen[c] + 1);
    m->first_seen_bound = std::max(m->first_seen_bound, m->units_done);
    return SKM_OK;
}

// The table where it lies (SURVEY 8(e).1 without the host: the hand-over between GPUs is then a
// copy of these arrays over xGMI, ncclSend / ncclRecv or a peer copy, and a merge by key).
extern "C" int skm_mapper_device_table(skm_mapper *m, skm_device_table *out)
{
    if (!m || !out) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    memset(out, 0, sizeof(*out));
    unsigned long long ctr[4];
    HIP_TRY(hipMemcpyAsync(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const int64_t C = (int64_t)ctr[CTR_CLASSES];
    out->device = m->ix->device;
    out->n_classes = C;
    out->n_ids = (int64_t)ctr[CTR_ARENA];
    out->unaligned = (int64_t)ctr[CTR_UNALIGNED];
    out->units = (int64_t)ctr[CTR_UNITS];
    out->first_seen_bound = m->first_seen_bound;
    out->fld = (const uint64_t *)(m->counters.p + CTR_FLD);
    out->ids = m->arena.p;
    if (C == 0) return SKM_OK;
    SKM_TRY(m->view_start.ensure(C)); SKM_TRY(m->view_len.ensure(C));
    SKM_TRY(m->view_count.ensure(C)); SKM_TRY(m->view_first_seen.ensure(C));
    launch_class_compact(m->t, C, m->view_start.p, m->view_len.p, m->view_count.p, m->view_first_seen.p, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    out->class_start = m->view_start.p;
    out->class_len = m->view_len.p;
    out->class_count = m->view_count.p;
    out->first_seen = (const uint64_t *)m->view_first_seen.p;
    return SKM_OK;
}

extern "C" int skm_mapper_merge_device(skm_mapper *m, const skm_device_table *table)
{
    if (!m || !table || table->n_classes < 0 || table->n_ids < 0 || table->unaligned < 0 || table->units < 0)
        return fail(SKM_ERR_ARG, "bad argument");
    if (table->n_classes && (!table->class_start || !table->class_len || !table->class_count || !table->first_seen || !table->ids))
        return fail(SKM_ERR_ARG, "NULL class arrays");
    if (table->device != m->ix->device)
        return fail(SKM_ERR_ARG, "the table lies on GPU %d, the mapper on GPU %d: copy it over first", table->device, m->ix->device);
    SKM_TRY(wait_jobs(m, 0, false));
    std::lock_guard<std::mutex> lock(m->mu);
    m->host_totals_valid = false;
    SKM_TRY(set_device(m->ix->device));
    const int64_t n_classes = table->n_classes;
    {   // foreign classes may all be new: size for them at load <= 0.5, unbounded probes
        uint64_t want = 1 << 16;
        while ((double)want * 0.5 < (double)(m->host_classes + n_classes + 1024)) want <<= 1;
        SKM_TRY(table_grow(m, want, 0));
        SKM_TRY(m->class_list.ensure((size_t)(m->host_classes + n_classes + 1024), true, m->stream));
    }
    SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + table->n_ids + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    if (n_classes) {
        launch_class_merge_device(m->t, n_classes, table->class_start, table->class_len, table->ids, table->class_count,
                                  (const unsigned long long *)table->first_seen, m->stream);
        HIP_TRY(hipGetLastError());
        SKM_TRY(read_error(m));
    }
    // totals and histogram only once the classes are in: a failed merge leaves them untouched (the
    // hand-over of a table happens once per sample: the launch boundary is on no hot path)
    launch_class_add_totals(m->t, (unsigned long long)table->unaligned, (unsigned long long)table->units,
                            (const unsigned long long *)table->fld, m->stream);
    HIP_TRY(hipGetLastError());
    unsigned long long ctr[8];
    HIP_TRY(hipMemcpyAsync(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->host_arena_used = (int64_t)ctr[CTR_ARENA];
    m->host_classes = (int64_t)ctr[CTR_CLASSES];
    m->host_units = ctr[CTR_UNITS];
    m->host_unaligned = ctr[CTR_UNALIGNED];
    m->host_totals_valid = true;
    m->units_done += table->units;
    m->first_seen_bound = std::max(m->first_seen_bound, std::max(table->first_seen_bound, m->units_done));
    return SKM_OK;
}

extern "C" int skm_mapper_clear(skm_mapper *m)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, true);            // (a failed queued batch is forgotten with the table)
    {
        std::lock_guard<std::mutex> hold(m->q_mu);      // (and packed reads that never got a mate)
        packed_drop_all(m);
    }
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // MapResult.clear only clears the counter (mapper.py:143-145): the FLD stays
    std::vector<unsigned long long> fld(MAX_FRAGMENT_LENGTH);
    HIP_TRY(hipMemcpy(fld.data(), m->counters.p + CTR_FLD, MAX_FRAGMENT_LENGTH * 8, hipMemcpyDeviceToHost));
    SKM_TRY(table_reset(m, m->t.slot_mask + 1));
    HIP_TRY(hipMemcpyAsync(m->counters.p + CTR_FLD, fld.data(), MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return SKM_OK;
}

extern "C" int skm_mapper_reset(skm_mapper *m)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, true);            // (a failed queued batch is forgotten with the table)
    {
        std::lock_guard<std::mutex> hold(m->q_mu);      // (and packed reads that never got a mate)
        packed_drop_all(m);
    }
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    SKM_TRY(table_reset(m, m->t.slot_mask + 1));
    if (m->bias) HIP_TRY(hipMemsetAsync(m->bias_observed.p, 0, BIAS_BINS * sizeof(unsigned long long), m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));         // (readers of the table use streams of their own)
    m->last_units = 0;
    m->last_ids = 0;
    m->last_reads = 0;
    return SKM_OK;
}

extern "C" int skm_mapper_timing(skm_mapper *m, double stats[8])
{
    if (!m || !stats) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    stats[0] = m->t_pack_ns; stats[1] = m->t_map_ns; stats[2] = m->t_class_ns;
    stats[3] = m->batches; stats[4] = (double)m->units_done;
    stats[5] = m->t_em_ns; stats[6] = m->em_iters; stats[7] = (double)m->deferred_grows;
    return SKM_OK;
}

extern "C" int skm_mapper_map_relaunches(skm_mapper *m, int64_t *count)
{
    if (!m || !count) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    *count = m->map_relaunches;
    return SKM_OK;
}

// access counters of the STATS build of the map kernel (SKM_MAP_STATS=1):
// [0]=reads [1]=read bases [2]=lookups [3]=slots [4]=contig reads [5]=targets
// copied [6]=targets merged [7]=8-base fetches [8]=merges [9]=tuple ids
extern "C" int skm_mapper_access_stats(skm_mapper *m, int64_t out[48])
{
    if (!m || !out) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    for (int i = 0; i < 48; ++i) out[i] = (int64_t)m->stats_total[i];
    return SKM_OK;
}

extern "C" int skm_mapper_set_stats(skm_mapper *m, int enable)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    m->want_stats = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    for (auto &v : m->stats_total) v = 0;
    return SKM_OK;
}

// ------------------------------------------------------------------ sample sets
// Many small samples through ONE mapper: their units share launches and the class table, in which a
// class is (sample, tuple) -- skm_samples.hip.  The set owns a mapper (its table, batch buffers, stream)
// and drives map_batch_resident itself: added segments wait in HBM in a queue, one worker cuts the
// front of the queue into launches and logs which units of which sample every launch held.
namespace {

struct SetChunk {                        // the reads of one added segment where they lie in HBM
    std::deque<skm_mapper::Piece> pieces[2];   // packed form: one piece per mate, numbered by the sample's units
    std::shared_ptr<char> ascii;         // ASCII form: one block, offsets | bases
    const uint8_t *bases = nullptr;      // biased: read r of the segment = bases[offsets[r] .. offsets[r + 1])
    const int64_t *offsets = nullptr;    // [reads + 1], as the caller gave them
    int64_t origin = 0;                  // the sample's unit of the segment's first read
    int max_len = 0;
    std::shared_ptr<uint32_t> umis;      // a set that keeps UMIs: umis[u - umi_origin] of the segment's unit u, in HBM
    int64_t umi_origin = 0;
};
struct SetQueued { int32_t sample; int64_t first, n; std::shared_ptr<SetChunk> data; };   // what is left of a segment
struct SetPart { int32_t sample; int64_t first, n, at; std::shared_ptr<SetChunk> data; }; // units [first, first + n) of
                                                                                         // the sample at place `at` of a launch

// the next launch: whole segments from the front of the queue, the last one cut where the launch is full
int64_t set_cut_launch(std::deque<SetQueued> &queue, int64_t max_units, std::vector<SetPart> *parts)
{
    int64_t n_units = 0;
    parts->clear();
    while (!queue.empty() && n_units < max_units && (int)parts->size() < SAMPLE_LAUNCH_SEGMENTS) {
        SetQueued &front = queue.front();
        const int64_t take = std::min(front.n, max_units - n_units);
        parts->push_back(SetPart{front.sample, front.first, take, n_units, front.data});
        n_units += take;
        if (take == front.n) queue.pop_front();
        else { front.first += take; front.n -= take; }
    }
    return n_units;
}

// which units of which sample the set's unit numbers are: one entry per part of every launch, in launch
// order, so `global` ascends and the entries tile [0, units)
struct SetLog {
    std::vector<int64_t> global, local;
    std::vector<int32_t> sample;
    int64_t units = 0;
    void append(const std::vector<SetPart> &parts)
    {
        for (const SetPart &part : parts) {
            global.push_back(units + part.at);
            local.push_back(part.first);
            sample.push_back(part.sample);
        }
        if (!parts.empty()) units += parts.back().at + parts.back().n;
    }
};

// classes by (sample, first-seen unit inside the sample): order[k] = the class in place k,
// sample_class_offsets[i] = place of sample i's first class
void set_split_order(int64_t n_samples, int64_t n_classes, const int32_t *class_sample, const int64_t *class_local,
                     int64_t *order, int64_t *sample_class_offsets)
{
    std::iota(order, order + n_classes, (int64_t)0);
    std::sort(order, order + n_classes, [&](int64_t a, int64_t b) {
        return class_sample[a] != class_sample[b] ? class_sample[a] < class_sample[b] : class_local[a] < class_local[b];
    });
    std::fill(sample_class_offsets, sample_class_offsets + n_samples + 1, (int64_t)0);
    for (int64_t k = 0; k < n_classes; ++k) sample_class_offsets[class_sample[k] + 1]++;
    for (int64_t i = 0; i < n_samples; ++i) sample_class_offsets[i + 1] += sample_class_offsets[i];
}

constexpr int64_t SET_MAX_SAMPLES = 1 << 24;
constexpr int64_t SET_MAX_HIST_SAMPLES = 1 << 16;   // with a histogram per sample: rows of 16 KB by sample NUMBER, 1 GiB at most
constexpr int64_t SET_MAX_BIAS_SAMPLES = 1 << 15;   // counting hexamers: rows of 32 KB (4096 x u64) by sample NUMBER, 1 GiB at most
constexpr int64_t SET_MAX_QUEUED = 4 * PACKED_MAX_UNITS;     // units that may wait in HBM before an adder waits

}  // namespace

struct skm_sample_set {
    skm_sample_set(skm_mapper *mapper, int paired_) : m(mapper), paired(paired_) {}
    ~skm_sample_set();
    Own<skm_mapper *, skm_mapper_destroy> m;      // (declared first: given up last)
    const int paired;
    int64_t max_units = PACKED_MAX_UNITS;         // of one launch (SKM_SAMPLE_SET_MAX_UNITS)
    std::mutex copy_mu;                           // one adder copies at a time
    Stream copy_stream;
    std::shared_ptr<std::atomic<int64_t>> bytes = std::make_shared<std::atomic<int64_t>>(0);
    DBuf<int32_t> seg_table;                      // the segments of the launch under way: first units | samples
    // one fragment-length histogram per sample (skm_sample_set_keep_histograms): [rows][2000], rows >= the
    // largest sample a launch has held + 1, every word up to hist.cap counted or zero; touched under m->mu
    bool keep_hist = false;
    DBuf<unsigned long long> hist;
    // one row of observed hexamers per sample (skm_sample_set_keep_bias): [rows][4096], kept as `hist` is
    bool keep_bias = false;
    DBuf<unsigned long long> bias_rows;
    // UMI collapse (skm_sample_set_keep_umis; skm_umi.hip): the molecule set -- umi_n_slots slots, a power of two,
    // sized ahead of every launch to at least twice (molecules so far + the launch's records) --, its two counters,
    // the units removed per sample (rows kept as `hist` is) and the segments' UMIs of the launch under way;
    // touched under m->mu.  SKM_TEST_UMI_SLOTS: the set starts at that many slots and grows only when a launch
    // finds it full.
    int umi_bases = 0;                            // 0: the set keeps no UMIs
    DBuf<UmiSlot> umi_slots;
    uint64_t umi_n_slots = 0, umi_test_slots = 0;
    int64_t umi_entries = 0;
    DBuf<unsigned long long> umi_ctl, umi_removed;
    DBuf<UmiSegment> umi_segs;
    // ---- under mu
    std::mutex mu;
    std::condition_variable work_cv, done_cv;
    std::deque<SetQueued> queue;
    int64_t queued_units = 0;
    std::vector<int64_t> sample_units;            // units added per sample = where its next segment must begin
    SetLog log;
    bool busy = false, stop = false, worker_started = false;
    int flush = 0;
    int error = SKM_OK;                           // the first failed launch: the set stays failed
    std::string error_msg;
    std::thread worker;
    // the tables by sample, made by the first reader after the last launch
    struct View {
        bool valid = false;
        std::vector<int64_t> start, len, count, local, order, sample_class_offsets, sample_rows, sample_aligned;
        std::vector<int64_t> units;               // sample_units as the view was made, all of them mapped, less `removed`
        std::vector<int64_t> removed;             // the units UMI collapse has removed, per sample (zeros without it)
        std::vector<int32_t> arena;
        // the classes where class_compact and sample_assign left them in HBM (registry order), kept with the view
        // for the calls that pass over the table on the device (skm_sample_set_gene_counts)
        DBuf<int64_t> d_start, d_len;
        DBuf<double> d_count;
        DBuf<int32_t> d_sample;
    } view;
};

namespace {

// the molecule set in `n_slots` slots (a power of two): a fresh set, or the molecules of the old one rehashed
// (m->mu is held; the stream drains before the old slots go back to the pool)
int set_umi_grow(skm_sample_set *s, uint64_t n_slots)
{
    skm_mapper *m = s->m;
    if (n_slots > (1ULL << 36)) return fail(SKM_ERR_STATE, "a molecule set of %llu slots", (unsigned long long)n_slots);
    DBuf<UmiSlot> fresh;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });
    if (fresh.ensure((size_t)n_slots) != SKM_OK) {
        const std::string why = last_message();
        return fail(SKM_ERR_HIP, "UMI collapse: no device memory for a molecule set of %llu slots, %llu MB (64 bytes a molecule "
                    "at load 1/2; %lld molecules so far): %s", (unsigned long long)n_slots,
                    (unsigned long long)(n_slots * sizeof(UmiSlot) >> 20), (long long)s->umi_entries, why.c_str());
    }
    const UmiSet to{fresh.p, n_slots - 1, s->umi_ctl.p, m->error.p};
    if (s->umi_n_slots) launch_umi_rehash(UmiSet{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, m->error.p}, to, m->stream);
    else launch_umi_init(to, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    drain.dismiss();
    s->umi_slots = std::move(fresh);
    s->umi_n_slots = n_slots;
    return SKM_OK;
}

int set_launch(skm_sample_set *s, const std::vector<SetPart> &parts, int64_t n_units, int64_t global_first)
{
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int mates = s->paired ? 2 : 1;
    const int n_parts = (int)parts.size();
    if (n_parts > SAMPLE_LAUNCH_SEGMENTS) return fail(SKM_ERR_STATE, "%d segments in one launch", n_parts);
    std::vector<int32_t> table(2 * (size_t)n_parts);
    std::vector<UmiSegment> umi_segments;         // (a set that keeps UMIs)
    std::vector<PackedSegment> segments;          // `first` = place in the launch
    int max_cw = 0, max_len = 0;
    for (int i = 0; i < n_parts; ++i) {
        const SetPart &part = parts[i];
        table[i] = (int32_t)part.at;
        table[n_parts + i] = part.sample;
        if (part.data->ascii) { max_len = std::max(max_len, part.data->max_len); continue; }
        for (int mate = 0; mate < mates; ++mate) {
            const size_t from = segments.size();
            packed_segments(part.data->pieces[mate], mate, part.first, part.first + part.n, false, &segments, &max_cw);
            for (size_t k = from; k < segments.size(); ++k) segments[k].first += part.at - part.first;
        }
    }
    max_len = std::max(max_len, max_cw * 32);
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (`table` is read by a queued copy)
    SKM_TRY(s->seg_table.ensure(2 * SAMPLE_LAUNCH_SEGMENTS));
    HIP_TRY(hipMemcpyAsync(s->seg_table.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    const SampleSalt salt{s->seg_table.p, s->seg_table.p + n_parts, n_parts};
    const RecordStage fill = [&](uint32_t *records, int words, int record_words) -> int {
        for (const PackedSegment &seg : segments) {
            uint32_t *dst = records + (seg.first * mates + seg.mate) * (int64_t)record_words;
            launch_unpack_reads(seg.codes, seg.cw, seg.cw, seg.lengths, seg.uniform_len, seg.n, words, dst,
                                (int64_t)mates * record_words, m->error.p, m->stream);
            if (seg.n_exc)
                launch_unpack_exceptions(seg.exc_reads, seg.exc_masks, seg.n_exc, seg.cw, seg.exc_base, words, dst,
                                         (int64_t)mates * record_words, m->stream);
        }
        for (const SetPart &part : parts) {
            if (!part.data->ascii) continue;
            launch_pack_reads(part.data->bases, part.data->offsets + (part.first - part.data->origin) * mates, part.n * mates,
                              words, record_words, records + part.at * mates * (int64_t)record_words, m->stream);
        }
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    if (s->keep_hist) {                           // room for the rows of this launch's samples, the new ones zero
        int32_t largest = 0;
        for (const SetPart &part : parts) largest = std::max(largest, part.sample);
        const size_t held = s->hist.cap;
        SKM_TRY(s->hist.ensure(((size_t)largest + 1) * MAX_FRAGMENT_LENGTH, true, m->stream));
        if (s->hist.cap > held)
            HIP_TRY(hipMemsetAsync(s->hist.p + held, 0, (s->hist.cap - held) * sizeof(unsigned long long), m->stream));
    }
    if (s->keep_bias) {
        int32_t largest = 0;
        for (const SetPart &part : parts) largest = std::max(largest, part.sample);
        const size_t held = s->bias_rows.cap;
        SKM_TRY(s->bias_rows.ensure(((size_t)largest + 1) * BIAS_BINS, true, m->stream));
        if (s->bias_rows.cap > held)
            HIP_TRY(hipMemsetAsync(s->bias_rows.p + held, 0, (s->bias_rows.cap - held) * sizeof(unsigned long long), m->stream));
    }
    // UMI collapse: the launch's segments with their UMIs, room in the molecule set, rows of removed[]; then claim and
    // resolve between the strand filter and everything that counts
    const BatchStage collapse = [&](const MapBatch &b) -> int {
        for (;;) {
            const UmiSet set{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, m->error.p};
            HIP_TRY(hipMemsetAsync(s->umi_ctl.p + UMI_CTL_LOST, 0, sizeof(unsigned long long), m->stream));
            launch_umi_claim(set, b, salt, s->umi_segs.p, m->stream);
            HIP_TRY(hipGetLastError());
            if (!s->umi_test_slots) break;        // (sized ahead: a full set is reported after the launch)
            unsigned long long *lost = m->pinned + 48;
            HIP_TRY(hipMemcpyAsync(lost, s->umi_ctl.p + UMI_CTL_LOST, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
            HIP_TRY(hipStreamSynchronize(m->stream));
            if (*lost == 0) break;
            // full under test: four times the slots, and the pass again -- find-or-claim and a minimum, so a
            // record that had its turn changes nothing by a second one
            SKM_TRY(set_umi_grow(s, s->umi_n_slots * 4));
        }
        const UmiSet set{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, m->error.p};
        launch_umi_resolve(set, b, salt, s->umi_segs.p, s->umi_removed.p, m->stream);
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    if (s->umi_bases) {
        int32_t largest = 0;
        umi_segments.reserve(n_parts);
        for (const SetPart &part : parts) {
            largest = std::max(largest, part.sample);
            if (!part.data->umis) return fail(SKM_ERR_STATE, "a segment without UMIs in a set that keeps them");
            umi_segments.push_back(UmiSegment{part.first, part.data->umis.get() + (part.first - part.data->umi_origin)});
        }
        SKM_TRY(s->umi_segs.ensure(SAMPLE_LAUNCH_SEGMENTS));
        HIP_TRY(hipMemcpyAsync(s->umi_segs.p, umi_segments.data(), umi_segments.size() * sizeof(UmiSegment), hipMemcpyHostToDevice, m->stream));
        const size_t held = s->umi_removed.cap;
        SKM_TRY(s->umi_removed.ensure((size_t)largest + 1, true, m->stream));
        if (s->umi_removed.cap > held)
            HIP_TRY(hipMemsetAsync(s->umi_removed.p + held, 0, (s->umi_removed.cap - held) * sizeof(unsigned long long), m->stream));
        if (!s->umi_ctl.p) {
            SKM_TRY(s->umi_ctl.ensure(UMI_CTL_WORDS));
            HIP_TRY(hipMemsetAsync(s->umi_ctl.p, 0, UMI_CTL_WORDS * sizeof(unsigned long long), m->stream));
        }
        uint64_t want = s->umi_test_slots ? s->umi_test_slots : 1024;
        if (!s->umi_test_slots)
            while (want < 2 * (uint64_t)(s->umi_entries + n_units)) want *= 2;
        if (s->umi_n_slots == 0 || (!s->umi_test_slots && want > s->umi_n_slots)) SKM_TRY(set_umi_grow(s, want));
    }
    SKM_TRY(map_batch_resident(m, nullptr, nullptr, n_units, s->paired, max_len, global_first, &fill, &salt,
                               s->keep_bias ? s->bias_rows.p : nullptr, s->umi_bases ? &collapse : nullptr));
    if (s->umi_bases) {                           // (the stream has drained)
        unsigned long long *ctl = m->pinned + 48;
        HIP_TRY(hipMemcpyAsync(ctl, s->umi_ctl.p, UMI_CTL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        if (ctl[UMI_CTL_LOST])
            return fail(SKM_ERR_STATE, "the molecule set of %llu slots was full for %llu records", (unsigned long long)s->umi_n_slots,
                        ctl[UMI_CTL_LOST]);
        s->umi_entries = (int64_t)ctl[UMI_CTL_ENTRIES];
    }
    if (s->keep_hist) {
        // the spans of the attempt that stood (an overflowing entry arena runs the map kernel again), after
        // the pair rule; they stay until this mapper's next launch, which the set's worker starts after this one
        if (!m->last_spans) return fail(SKM_ERR_STATE, "a set that keeps histograms mapped without spans");
        launch_sample_fld(m->unit_begin.p, m->unit_end.p, n_units, salt, s->hist.p, m->stream);
        HIP_TRY(hipGetLastError());
    }
    return SKM_OK;
}

void set_worker(skm_sample_set *s)
{
    for (;;) {
        std::vector<SetPart> parts;
        int64_t n_units = 0, global_first = 0;
        {
            std::unique_lock<std::mutex> hold(s->mu);
            s->work_cv.wait(hold, [&] {
                return s->stop || (!s->queue.empty()
                                   && (s->error != SKM_OK || s->flush || s->queued_units >= std::min(PACKED_MIN_UNITS, s->max_units)));
            });
            if (s->stop || s->error != SKM_OK) {          // nothing more is mapped: what waits goes
                s->queue.clear();
                s->queued_units = 0;
                s->done_cv.notify_all();
                if (s->stop) return;
                continue;
            }
            n_units = set_cut_launch(s->queue, s->max_units, &parts);
            s->queued_units -= n_units;
            global_first = s->log.units;
            s->log.append(parts);
            s->view.valid = false;
            s->busy = true;
        }
        const int rc = set_launch(s, parts, n_units, global_first);
        const std::string message = rc != SKM_OK ? last_message() : std::string();
        if (rc != SKM_OK) (void)hipStreamSynchronize(s->m->stream);   // (before the parts' blocks go back to the pool)
        parts.clear();
        {
            std::lock_guard<std::mutex> hold(s->mu);
            if (rc != SKM_OK) { s->error = rc; s->error_msg = message; }
            s->busy = false;
        }
        s->done_cv.notify_all();
    }
}

// wait until everything added has been mapped; the set's failure, if it has one
int set_wait(skm_sample_set *s)
{
    std::unique_lock<std::mutex> hold(s->mu);
    s->flush++;
    s->work_cv.notify_all();
    s->done_cv.wait(hold, [&] { return !s->busy && s->queue.empty(); });
    s->flush--;
    if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
    return SKM_OK;
}

// (before the copy) the caller's arguments, and room in the queue
int set_admit(skm_sample_set *s, int64_t sample, int64_t first_unit, int64_t n_units)
{
    if (sample < 0 || sample >= SET_MAX_SAMPLES) return fail(SKM_ERR_ARG, "sample %lld outside [0, 2^24)", (long long)sample);
    if (first_unit < 0 || n_units < 0 || n_units >= (1LL << 31)) return fail(SKM_ERR_ARG, "bad unit range");
    SKM_TRY(set_device(s->m->ix->device));
    std::unique_lock<std::mutex> hold(s->mu);
    if (s->keep_hist && sample >= SET_MAX_HIST_SAMPLES)
        return fail(SKM_ERR_ARG, "sample %lld: a set that keeps a histogram per sample numbers its samples below %lld",
                    (long long)sample, (long long)SET_MAX_HIST_SAMPLES);
    if (s->keep_bias && sample >= SET_MAX_BIAS_SAMPLES)
        return fail(SKM_ERR_ARG, "sample %lld: a set that counts hexamers per sample numbers its samples below %lld",
                    (long long)sample, (long long)SET_MAX_BIAS_SAMPLES);
    s->done_cv.wait(hold, [&] { return s->error != SKM_OK || s->queued_units <= SET_MAX_QUEUED; });
    if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
    return SKM_OK;
}

// (after the copy) the segment joins the queue if it begins where the sample's units so far end
int set_enqueue(skm_sample_set *s, int64_t sample, int64_t first_unit, int64_t n_units, std::shared_ptr<SetChunk> data)
{
    {
        std::lock_guard<std::mutex> hold(s->mu);
        if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
        if ((int64_t)s->sample_units.size() <= sample) s->sample_units.resize((size_t)sample + 1, 0);
        if (first_unit != s->sample_units[sample])
            return fail(SKM_ERR_STATE, "sample %lld: a segment from unit %lld after %lld units (segments are added in order)",
                        (long long)sample, (long long)first_unit, (long long)s->sample_units[sample]);
        s->sample_units[sample] += n_units;
        s->view.valid = false;
        if (n_units == 0) return SKM_OK;
        s->queue.push_back(SetQueued{(int32_t)sample, first_unit, n_units, std::move(data)});
        s->queued_units += n_units;
        if (!s->worker_started) {
            s->worker = std::thread(set_worker, s);
            s->worker_started = true;
        }
    }
    s->work_cv.notify_all();
    return SKM_OK;
}

// `hold` (s->mu) is taken here, when everything added has been mapped, and stays taken for the caller's
// reading: from that moment no segment joins the queue (an adder waits in set_enqueue), so what the caller
// reads, the log and the units per sample describe the same units.
// set_view: the tables by sample (s->view), made once after the last launch.
int set_hold(skm_sample_set *s, std::unique_lock<std::mutex> &hold)
{
    hold = std::unique_lock<std::mutex>(s->mu);
    s->flush++;
    s->work_cv.notify_all();
    s->done_cv.wait(hold, [&] { return !s->busy && s->queue.empty(); });
    s->flush--;
    if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
    return SKM_OK;
}

int set_view(skm_sample_set *s, std::unique_lock<std::mutex> &hold)
{
    SKM_TRY(set_hold(s, hold));
    if (s->view.valid) return SKM_OK;
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes, M = m->host_arena_used, n_samples = (int64_t)s->sample_units.size();
    const int64_t n_log = (int64_t)s->log.global.size();
    skm_sample_set::View &v = s->view;
    v.start.assign(C, 0); v.len.assign(C, 0); v.count.assign(C, 0); v.local.assign(C, 0); v.order.assign(C, 0);
    v.arena.assign((size_t)std::max<int64_t>(M, 1), 0);
    v.sample_class_offsets.assign(n_samples + 1, 0);
    v.sample_rows.assign(n_samples, 0); v.sample_aligned.assign(n_samples, 0);
    v.units = s->sample_units;
    v.removed.assign(n_samples, 0);
    int64_t removed_total = 0;
    if (s->umi_bases && s->umi_removed.cap && n_samples) {      // (a sample that no launch has held may lie past the rows)
        const int64_t rows = std::min<int64_t>(n_samples, (int64_t)s->umi_removed.cap);
        HIP_TRY(hipMemcpyAsync(v.removed.data(), s->umi_removed.p, (size_t)rows * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        for (int64_t i = 0; i < n_samples; ++i) {
            if (v.removed[i] < 0 || v.removed[i] > v.units[i])
                return fail(SKM_ERR_STATE, "sample %lld: %lld of %lld units removed", (long long)i, (long long)v.removed[i], (long long)v.units[i]);
            v.units[i] -= v.removed[i];               // a removed unit was never in the files
            removed_total += v.removed[i];
        }
    }
    std::vector<int32_t> cls_sample(C);
    if (C) {
        if (n_log == 0) return fail(SKM_ERR_STATE, "classes without a launch");
        DBuf<int64_t> &d_off = v.d_start, &d_len = v.d_len; DBuf<double> &d_cnt = v.d_count; DBuf<int32_t> &d_sample = v.d_sample;
        DBuf<int64_t> d_local, d_log; DBuf<unsigned long long> d_fs; DBuf<int32_t> d_log_sample;
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
        SKM_TRY(d_off.ensure(C)); SKM_TRY(d_len.ensure(C)); SKM_TRY(d_cnt.ensure(C)); SKM_TRY(d_fs.ensure(C));
        SKM_TRY(d_sample.ensure(C)); SKM_TRY(d_local.ensure(C)); SKM_TRY(d_log.ensure(2 * n_log)); SKM_TRY(d_log_sample.ensure(n_log));
        HIP_TRY(hipMemcpyAsync(d_log.p, s->log.global.data(), n_log * 8, hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(d_log.p + n_log, s->log.local.data(), n_log * 8, hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(d_log_sample.p, s->log.sample.data(), n_log * 4, hipMemcpyHostToDevice, m->stream));
        launch_class_compact(m->t, C, d_off.p, d_len.p, d_cnt.p, d_fs.p, m->stream);
        launch_sample_assign(d_log.p, d_log.p + n_log, d_log_sample.p, n_log, d_fs.p, C, d_sample.p, d_local.p, m->stream);
        HIP_TRY(hipGetLastError());
        std::vector<double> cnt(C);
        HIP_TRY(hipMemcpyAsync(v.start.data(), d_off.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(v.len.data(), d_len.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(cls_sample.data(), d_sample.p, C * 4, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(v.local.data(), d_local.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        if (M) HIP_TRY(hipMemcpyAsync(v.arena.data(), m->arena.p, (size_t)M * 4, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        drain.dismiss();
        for (int64_t k = 0; k < C; ++k) {
            if (cls_sample[k] < 0 || cls_sample[k] >= n_samples || v.start[k] < 0)
                return fail(SKM_ERR_STATE, "class %lld of the shared table belongs to no sample", (long long)k);
            v.count[k] = (int64_t)cnt[k];
            v.sample_rows[cls_sample[k]] += v.len[k];
            v.sample_aligned[cls_sample[k]] += v.count[k];
        }
    }
    set_split_order(n_samples, C, cls_sample.data(), v.local.data(), v.order.data(), v.sample_class_offsets.data());
    // (units_s - aligned_s is each sample's unaligned count; their sum is what the table counted -- less the units
    // that UMI collapse removed, which reached class counting looking unaligned)
    int64_t unaligned = 0;
    for (int64_t i = 0; i < n_samples; ++i) {
        if (v.sample_aligned[i] > v.units[i]) return fail(SKM_ERR_STATE, "sample %lld counts more units than it has", (long long)i);
        unaligned += v.units[i] - v.sample_aligned[i];
    }
    if (m->host_totals_valid && unaligned != (int64_t)m->host_unaligned - removed_total)
        return fail(SKM_ERR_STATE, "the samples' unaligned units (%lld) are not the table's (%llu less %lld removed)", (long long)unaligned,
                    m->host_unaligned, (long long)removed_total);
    v.valid = true;
    return SKM_OK;
}

}  // namespace

skm_sample_set::~skm_sample_set()
{
    (void)hipSetDevice(m->ix->device);
    if (worker_started) {
        { std::lock_guard<std::mutex> hold(mu); stop = true; }
        work_cv.notify_all();
        worker.join();                     // (finishes the launch under way; what waits is dropped)
    }
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
}

extern "C" int skm_sample_set_create(skm_index *ix, int paired, skm_sample_set **out)
{
    if (!ix || !out) return fail(SKM_ERR_ARG, "NULL argument");
    skm_mapper *mapper = nullptr;
    SKM_TRY(skm_mapper_create(ix, &mapper));
    std::unique_ptr<skm_sample_set> s(new skm_sample_set(mapper, paired ? 1 : 0));
    HIP_TRY(hipStreamCreateWithFlags(s->copy_stream.out(), hipStreamNonBlocking));
    if (const char *v = getenv("SKM_SAMPLE_SET_MAX_UNITS"))
        if (atoll(v) > 0) s->max_units = std::min<int64_t>(atoll(v), PACKED_MAX_UNITS);
    if (const char *v = getenv("SKM_TEST_UMI_SLOTS")) {          // test hook: a molecule set that has to grow under a launch
        const long long n = atoll(v);
        if (n < 2 || n > (1LL << 30) || (n & (n - 1)))
            return fail(SKM_ERR_ARG, "SKM_TEST_UMI_SLOTS must be a power of two from 2 to 2^30, not '%s'", v);
        s->umi_test_slots = (uint64_t)n;
    }
    *out = s.release();
    return SKM_OK;
}

extern "C" int skm_sample_set_destroy(skm_sample_set *s)
{
    delete s;
    return SKM_OK;
}

extern "C" int skm_sample_set_set_strand(skm_sample_set *s, int mode)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    {
        std::lock_guard<std::mutex> hold(s->mu);
        for (const int64_t units : s->sample_units)
            if (units) return fail(SKM_ERR_STATE, "the strand mode can only change on an empty sample set");
    }
    return skm_mapper_set_strand(s->m, mode);
}

extern "C" int skm_sample_set_set_length_weights(skm_sample_set *s, const double *p)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    return skm_mapper_set_length_weights(s->m, p);
}

extern "C" int skm_sample_set_keep_histograms(skm_sample_set *s, int enable)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    std::lock_guard<std::mutex> hold(s->mu);
    for (const int64_t units : s->sample_units)
        if (units) return fail(SKM_ERR_STATE, "histograms per sample can only be switched on an empty sample set");
    if (!enable && s->umi_bases) return fail(SKM_ERR_STATE, "a set that keeps UMIs keeps its histograms per sample");
    SKM_TRY(skm_mapper_keep_spans(s->m, enable));
    s->keep_hist = enable != 0;
    return SKM_OK;
}

extern "C" int skm_sample_set_keep_bias(skm_sample_set *s, int enable)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    std::lock_guard<std::mutex> hold(s->mu);
    for (const int64_t units : s->sample_units)
        if (units) return fail(SKM_ERR_STATE, "hexamer counts per sample can only be switched on an empty sample set");
    s->keep_bias = enable != 0;
    return SKM_OK;
}

extern "C" int skm_sample_set_keep_umis(skm_sample_set *s, int umi_bases)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    if (umi_bases < 0 || umi_bases > 16) return fail(SKM_ERR_ARG, "UMIs of %d bases: 1 to 16 are possible (0: none)", umi_bases);
    std::lock_guard<std::mutex> hold(s->mu);
    if (!s->sample_units.empty()) return fail(SKM_ERR_STATE, "UMIs can only be switched before the set's first segment");
    if (umi_bases && !s->keep_hist)
        return fail(SKM_ERR_STATE, "a set that keeps UMIs keeps a histogram per sample: call skm_sample_set_keep_histograms(set, 1) "
                    "first (the pooled histogram is counted inside the map kernel and cannot leave a unit out)");
    s->umi_bases = umi_bases;
    return SKM_OK;
}

namespace {

int set_umi_bases(skm_sample_set *s)
{
    std::lock_guard<std::mutex> hold(s->mu);
    return s->umi_bases;
}

int set_add_packed(skm_sample_set *s, int64_t sample, int64_t first_unit, const skm_packed_reads *mate1,
                   const skm_packed_reads *mate2, const uint32_t *umis)
{
    if ((mate2 != nullptr) != (s->paired != 0)) return fail(SKM_ERR_ARG, "a %s set takes %s", s->paired ? "paired" : "single-ended",
                                                           s->paired ? "both mates" : "mate 1 alone");
    const int64_t n = mate1->n_reads;
    if (mate2 && mate2->n_reads != n) return fail(SKM_ERR_ARG, "%lld reads of mate 1, %lld of mate 2", (long long)n, (long long)mate2->n_reads);
    SKM_TRY(set_admit(s, sample, first_unit, n));
    auto data = std::make_shared<SetChunk>();
    if (n) {
        const skm_packed_reads *mates[2] = {mate1, mate2};
        for (int k = 0; k < (s->paired ? 2 : 1); ++k) SKM_TRY(packed_check_arrays(mates[k]));
        std::lock_guard<std::mutex> copying(s->copy_mu);
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(s->copy_stream); });   // (the caller's arrays, the blocks)
        for (int k = 0; k < (s->paired ? 2 : 1); ++k) {
            skm_packed_reads piece = *mates[k];
            piece.first_read = first_unit;             // (numbered by the sample's units)
            skm_mapper::Piece held;
            SKM_TRY(packed_upload(&piece, s->bytes, s->copy_stream, &held));
            data->pieces[k].push_back(std::move(held));
        }
        if (umis) {                                    // the UMIs go with the chunk
            uint32_t *raw = nullptr;
            const int64_t block_bytes = (int64_t)packed_round((size_t)n * 4);
            HIP_TRY(pool_alloc((void **)&raw, (size_t)block_bytes));
            std::shared_ptr<std::atomic<int64_t>> counter = s->bytes;
            counter->fetch_add(block_bytes);
            data->umis = std::shared_ptr<uint32_t>(raw, [counter, block_bytes](uint32_t *q) { pool_free(q); counter->fetch_sub(block_bytes); });
            data->umi_origin = first_unit;
            HIP_TRY(hipMemcpyAsync(raw, umis, (size_t)n * 4, hipMemcpyHostToDevice, s->copy_stream));
        }
        drain.dismiss();
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    }
    return set_enqueue(s, sample, first_unit, n, std::move(data));
}

}  // namespace

extern "C" int skm_sample_set_add_packed(skm_sample_set *s, int64_t sample, int64_t first_unit,
                                         const skm_packed_reads *mate1, const skm_packed_reads *mate2)
{
    if (!s || !mate1) return fail(SKM_ERR_ARG, "NULL argument");
    if (set_umi_bases(s)) return fail(SKM_ERR_ARG, "a set that keeps UMIs takes its reads with them: skm_sample_set_add_packed_umis");
    return set_add_packed(s, sample, first_unit, mate1, mate2, nullptr);
}

extern "C" int skm_sample_set_add_packed_umis(skm_sample_set *s, int64_t sample, int64_t first_unit, const skm_packed_reads *mate1,
                                              const skm_packed_reads *mate2, const uint32_t *umis)
{
    if (!s || !mate1) return fail(SKM_ERR_ARG, "NULL argument");
    const int umi_bases = set_umi_bases(s);
    if (!umi_bases) return fail(SKM_ERR_ARG, "the set keeps no UMIs: call skm_sample_set_keep_umis before the first segment");
    if (mate1->n_reads > 0 && !umis) return fail(SKM_ERR_ARG, "NULL UMIs");
    if (umi_bases < 16)
        for (int64_t u = 0; u < mate1->n_reads; ++u)
            if (umis[u] >> (2 * umi_bases)) return fail(SKM_ERR_ARG, "UMI %lld (%u) does not fit %d bases", (long long)u, umis[u], umi_bases);
    return set_add_packed(s, sample, first_unit, mate1, mate2, mate1->n_reads > 0 ? umis : nullptr);
}

extern "C" int skm_sample_set_add_batch(skm_sample_set *s, int64_t sample, int64_t first_unit, const char *bases,
                                        const int64_t *offsets, int64_t n_units)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    if (set_umi_bases(s)) return fail(SKM_ERR_ARG, "a set that keeps UMIs takes its reads with them: skm_sample_set_add_packed_umis");
    if (n_units > 0 && (!bases || !offsets)) return fail(SKM_ERR_ARG, "NULL reads");
    SKM_TRY(set_admit(s, sample, first_unit, n_units));
    auto data = std::make_shared<SetChunk>();
    if (n_units) {
        const int64_t n_reads = s->paired ? 2 * n_units : n_units;
        int64_t longest = 0;
        for (int64_t r = 0; r < n_reads; ++r) {
            if (offsets[r + 1] < offsets[r]) return fail(SKM_ERR_ARG, "offsets are not monotone");
            longest = std::max(longest, offsets[r + 1] - offsets[r]);
        }
        if (longest > (1 << 20)) return fail(SKM_ERR_ARG, "read longer than 2^20 bases");
        const int64_t n_bytes = offsets[n_reads] - offsets[0];
        const size_t offsets_bytes = packed_round((size_t)(n_reads + 1) * 8);
        const int64_t block_bytes = (int64_t)(offsets_bytes + (size_t)n_bytes + 64);     // (the pack kernel reads 32 bytes at a time)
        char *raw = nullptr;
        HIP_TRY(pool_alloc((void **)&raw, (size_t)block_bytes));
        std::shared_ptr<std::atomic<int64_t>> counter = s->bytes;
        counter->fetch_add(block_bytes);
        data->ascii = std::shared_ptr<char>(raw, [counter, block_bytes](char *q) { pool_free(q); counter->fetch_sub(block_bytes); });
        data->offsets = (const int64_t *)raw;
        data->bases = (const uint8_t *)raw + offsets_bytes - offsets[0];
        data->origin = first_unit;
        data->max_len = (int)longest;
        std::lock_guard<std::mutex> copying(s->copy_mu);
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(s->copy_stream); });
        HIP_TRY(hipMemcpyAsync(raw, offsets, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, s->copy_stream));
        if (n_bytes)
            HIP_TRY(hipMemcpyAsync(raw + offsets_bytes, bases + offsets[0], (size_t)n_bytes, hipMemcpyHostToDevice, s->copy_stream));
        drain.dismiss();
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    }
    return set_enqueue(s, sample, first_unit, n_units, std::move(data));
}

extern "C" int skm_sample_set_sync(skm_sample_set *s)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    return set_wait(s);
}

extern "C" int skm_sample_set_map_relaunches(skm_sample_set *s, int64_t *count)
{
    if (!s || !count) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_wait(s));
    return skm_mapper_map_relaunches(s->m, count);
}

extern "C" int skm_sample_set_summary(skm_sample_set *s, int64_t cap_samples, int64_t *n_samples, int64_t *summary)
{
    if (!s || !n_samples || cap_samples < 0 || (cap_samples && !summary)) return fail(SKM_ERR_ARG, "bad argument");
    if (cap_samples == 0) {                               // (the number alone: nothing is waited for)
        std::lock_guard<std::mutex> counting(s->mu);
        *n_samples = (int64_t)s->sample_units.size();
        return SKM_OK;
    }
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    *n_samples = (int64_t)v.units.size();
    for (int64_t i = 0; i < std::min(cap_samples, *n_samples); ++i) {
        summary[4 * i + 0] = v.sample_class_offsets[i + 1] - v.sample_class_offsets[i];
        summary[4 * i + 1] = v.sample_rows[i];
        summary[4 * i + 2] = v.units[i] - v.sample_aligned[i];
        summary[4 * i + 3] = v.units[i];
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_export(skm_sample_set *s, int64_t *sample_class_offsets, int64_t *class_offsets,
                                     int32_t *class_targets, int64_t *class_counts, int64_t *first_seen)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    if (sample_class_offsets) std::copy(v.sample_class_offsets.begin(), v.sample_class_offsets.end(), sample_class_offsets);
    if (class_offsets) class_offsets[0] = 0;
    int64_t pos = 0;
    for (size_t k = 0; k < v.order.size(); ++k) {
        const int64_t c = v.order[k];
        if (class_targets) memcpy(class_targets + pos, v.arena.data() + v.start[c], (size_t)v.len[c] * 4);
        pos += v.len[c];
        if (class_offsets) class_offsets[k + 1] = pos;
        if (class_counts) class_counts[k] = v.count[c];
        if (first_seen) first_seen[k] = v.local[c];
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_histogram(skm_sample_set *s, int64_t *fld)
{
    if (!s || !fld) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_wait(s));
    return skm_mapper_export(s->m, nullptr, nullptr, nullptr, nullptr, fld);
}

extern "C" int skm_sample_set_histograms(skm_sample_set *s, int64_t cap_samples, int64_t *fld)
{
    if (!s || cap_samples < 0 || (cap_samples && !fld)) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_hold(s, hold));
    if (!s->keep_hist)
        return fail(SKM_ERR_STATE, "the set keeps no histogram per sample: call skm_sample_set_keep_histograms(set, 1) before adding");
    const int64_t n_samples = (int64_t)s->sample_units.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    if (n_samples == 0) return SKM_OK;
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // (a sample that no launch has held -- no units -- may lie past the buffer: its row is zero)
    const int64_t rows = std::min<int64_t>(n_samples, (int64_t)(s->hist.cap / MAX_FRAGMENT_LENGTH));
    std::fill(fld + rows * MAX_FRAGMENT_LENGTH, fld + n_samples * MAX_FRAGMENT_LENGTH, (int64_t)0);
    if (rows) {
        HIP_TRY(hipMemcpyAsync(fld, s->hist.p, (size_t)rows * MAX_FRAGMENT_LENGTH * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_bias_observed(skm_sample_set *s, int64_t cap_samples, int64_t *out)
{
    if (!s || cap_samples < 0 || (cap_samples && !out)) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_hold(s, hold));
    if (!s->keep_bias)
        return fail(SKM_ERR_STATE, "the set does not count hexamers: call skm_sample_set_keep_bias(set, 1) before adding");
    const int64_t n_samples = (int64_t)s->sample_units.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    if (n_samples == 0) return SKM_OK;
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // (a sample that no launch has held -- no units -- may lie past the buffer: its row is zero)
    const int64_t rows = std::min<int64_t>(n_samples, (int64_t)(s->bias_rows.cap / BIAS_BINS));
    std::fill(out + rows * BIAS_BINS, out + n_samples * BIAS_BINS, (int64_t)0);
    if (rows) {
        HIP_TRY(hipMemcpyAsync(out, s->bias_rows.p, (size_t)rows * BIAS_BINS * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_umi_removed(skm_sample_set *s, int64_t cap_samples, int64_t *removed)
{
    if (!s || cap_samples < 0 || (cap_samples && !removed)) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.removed.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    std::copy(v.removed.begin(), v.removed.end(), removed);
    return SKM_OK;
}

// ------------------------------------------------------------------ gene-level tables (skm_genes.hip)
namespace {

// SKM_GENE_GROUP (tests): rows of values per group of skm_gene_sums, samples per range of the gene counts
int64_t gene_group(int64_t fitting, int64_t n)
{
    int64_t group = fitting;
    if (const char *v = getenv("SKM_GENE_GROUP"))
        if (atoll(v) > 0) group = std::min<int64_t>(group, atoll(v));
    return std::max<int64_t>(1, std::min(group, n));
}

int gene_map_check(int64_t n_tx, int64_t n_genes, const int32_t *tx_gene)
{
    if (n_tx < 0 || n_genes < 0 || n_tx > INT32_MAX || n_genes > INT32_MAX || (n_tx && !tx_gene))
        return fail(SKM_ERR_ARG, "bad gene map");
    for (int64_t t = 0; t < n_tx; ++t)
        if (tx_gene[t] < -1 || tx_gene[t] >= n_genes)
            return fail(SKM_ERR_ARG, "transcript %lld has gene %d of %lld", (long long)t, tx_gene[t], (long long)n_genes);
    return SKM_OK;
}

// unique[n_samples][n_genes], other[n_samples][2] of a class table in HBM (stream drained on return).  Device rows
// exist for a range of samples at a time: 1 GiB of them at most.
int gene_counts_device(const GeneClasses &t, int64_t n_samples, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                       int64_t *unique, int64_t *other, hipStream_t stream)
{
    std::fill(unique, unique + n_samples * n_genes, (int64_t)0);
    std::fill(other, other + n_samples * 2, (int64_t)0);
    if (t.n_classes == 0 || n_samples == 0) return SKM_OK;
    if (n_tx == 0) return fail(SKM_ERR_ARG, "classes over no transcripts");
    const int64_t range = gene_group((int64_t)(1LL << 27) / std::max<int64_t>(n_genes, 1), n_samples);
    DBuf<int32_t> d_gene; DBuf<unsigned long long> d_rows; DBuf<int> d_error;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    const size_t row_words = (size_t)range * (size_t)(n_genes + 2);             // unique rows | other rows
    SKM_TRY(d_gene.ensure(n_tx)); SKM_TRY(d_rows.ensure(row_words)); SKM_TRY(d_error.ensure(1));
    HIP_TRY(hipMemcpyAsync(d_gene.p, tx_gene, n_tx * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_error.p, 0, sizeof(int), stream));
    for (int64_t first = 0; first < n_samples; first += range) {
        const int64_t here = std::min(range, n_samples - first);
        unsigned long long *d_other = d_rows.p + here * n_genes;
        HIP_TRY(hipMemsetAsync(d_rows.p, 0, (size_t)here * (size_t)(n_genes + 2) * 8, stream));
        launch_gene_unique(t, d_gene.p, n_tx, n_genes, first, first + here, d_rows.p, d_other, d_error.p, stream);
        HIP_TRY(hipGetLastError());
        if (n_genes)
            HIP_TRY(hipMemcpyAsync(unique + first * n_genes, d_rows.p, (size_t)(here * n_genes) * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(other + first * 2, d_other, (size_t)here * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    int error = 0;
    HIP_TRY(hipMemcpyAsync(&error, d_error.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.dismiss();
    if (error) return fail(SKM_ERR_ARG, "a class names a transcript not below n_tx = %lld", (long long)n_tx);
    return SKM_OK;
}

}  // namespace

// Rows in groups, so that the rows staged in HBM stay within 256 MB; the gene list goes up once.
extern "C" int skm_gene_sums(int device, int64_t n_rows, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                             const double *values, double *out)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    if (n_rows < 0 || (n_rows && ((n_tx && !values) || (n_genes && !out)))) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    if (n_rows == 0 || n_genes == 0) return SKM_OK;
    // the transcripts by gene, ascending inside a gene: a stable counting sort
    std::vector<int64_t> gene_off(n_genes + 1, 0);
    for (int64_t t = 0; t < n_tx; ++t)
        if (tx_gene[t] >= 0) gene_off[tx_gene[t] + 1]++;
    for (int64_t g = 0; g < n_genes; ++g) gene_off[g + 1] += gene_off[g];
    std::vector<int32_t> gene_tx((size_t)std::max<int64_t>(gene_off[n_genes], 1));
    {
        std::vector<int64_t> next(gene_off.begin(), gene_off.end() - 1);
        for (int64_t t = 0; t < n_tx; ++t)
            if (tx_gene[t] >= 0) gene_tx[next[tx_gene[t]]++] = (int32_t)t;
    }
    SKM_TRY(set_device(device));
    const int64_t group = gene_group(std::min<int64_t>((int64_t)(1LL << 25) / std::max<int64_t>(std::max(n_tx, n_genes), 1), 65535), n_rows);
    DBuf<int64_t> d_off; DBuf<int32_t> d_tx; DBuf<double> d_values, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_off.ensure(n_genes + 1)); SKM_TRY(d_tx.ensure(gene_tx.size()));
    SKM_TRY(d_values.ensure((size_t)std::max<int64_t>(group * n_tx, 1))); SKM_TRY(d_out.ensure((size_t)(group * n_genes)));
    HIP_TRY(hipMemcpy(d_off.p, gene_off.data(), (n_genes + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_tx.p, gene_tx.data(), gene_tx.size() * 4, hipMemcpyHostToDevice));
    for (int64_t first = 0; first < n_rows; first += group) {
        const int64_t here = std::min(group, n_rows - first);
        if (n_tx) HIP_TRY(hipMemcpy(d_values.p, values + first * n_tx, (size_t)(here * n_tx) * 8, hipMemcpyHostToDevice));
        launch_gene_sums(d_values.p, here, n_tx, d_off.p, d_tx.p, n_genes, d_out.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + first * n_genes, d_out.p, (size_t)(here * n_genes) * 8, hipMemcpyDeviceToHost));
    }
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}

extern "C" int skm_gene_unique_counts(int device, int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets,
                                      const int64_t *class_counts, const int32_t *class_sample, int64_t n_samples,
                                      int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, int64_t *unique, int64_t *other)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    if (n_classes < 0 || n_samples < 0 || (n_samples && (!other || (n_genes > 0 && !unique))))
        return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (!class_offsets || !class_counts || n_samples < 1)) return fail(SKM_ERR_ARG, "NULL class arrays");
    if (n_classes && !class_sample && n_samples > 1) return fail(SKM_ERR_ARG, "%lld samples without class_sample", (long long)n_samples);
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    const int64_t M = n_classes ? class_offsets[n_classes] : 0;
    for (int64_t c = 0; c < n_classes; ++c) {
        if (class_offsets[c] < 0 || class_offsets[c + 1] < class_offsets[c] || class_offsets[c + 1] - class_offsets[c] > INT32_MAX)
            return fail(SKM_ERR_ARG, "class_offsets are not those of a table");
        if (class_counts[c] < 0) return fail(SKM_ERR_ARG, "class %lld has a negative count", (long long)c);
        if (class_sample && (class_sample[c] < 0 || class_sample[c] >= n_samples))
            return fail(SKM_ERR_ARG, "class %lld belongs to sample %d of %lld", (long long)c, class_sample[c], (long long)n_samples);
    }
    if (M && !class_targets) return fail(SKM_ERR_ARG, "NULL class arrays");
    for (int64_t k = 0; k < M; ++k)
        if (class_targets[k] < 0 || class_targets[k] >= n_tx)
            return fail(SKM_ERR_ARG, "a class names transcript %d of %lld", class_targets[k], (long long)n_tx);
    SKM_TRY(set_device(device));
    DBuf<int64_t> d_off, d_cnt; DBuf<int32_t> d_ids, d_sample;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    GeneClasses t{};
    t.n_classes = n_classes;
    if (n_classes) {
        SKM_TRY(d_off.ensure(n_classes + 1)); SKM_TRY(d_cnt.ensure(n_classes)); SKM_TRY(d_ids.ensure((size_t)std::max<int64_t>(M, 1)));
        HIP_TRY(hipMemcpy(d_off.p, class_offsets, (n_classes + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_cnt.p, class_counts, n_classes * 8, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(d_ids.p, class_targets, M * 4, hipMemcpyHostToDevice));
        if (class_sample) {
            SKM_TRY(d_sample.ensure(n_classes));
            HIP_TRY(hipMemcpy(d_sample.p, class_sample, n_classes * 4, hipMemcpyHostToDevice));
            t.sample = d_sample.p;
        }
        t.start = d_off.p; t.count_i64 = d_cnt.p; t.ids = d_ids.p;
    }
    SKM_TRY(gene_counts_device(t, n_samples, n_tx, n_genes, tx_gene, unique, other, nullptr));
    drain.dismiss();
    return SKM_OK;
}

extern "C" int skm_mapper_gene_counts(skm_mapper *m, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                      int64_t *unique, int64_t other[2])
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!m || !other || (n_genes > 0 && !unique)) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes;
    DBuf<int64_t> d_off, d_len; DBuf<double> d_cnt; DBuf<unsigned long long> d_fs;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
    GeneClasses t{};
    t.n_classes = C;
    if (C) {
        SKM_TRY(d_off.ensure(C)); SKM_TRY(d_len.ensure(C)); SKM_TRY(d_cnt.ensure(C)); SKM_TRY(d_fs.ensure(C));
        launch_class_compact(m->t, C, d_off.p, d_len.p, d_cnt.p, d_fs.p, m->stream);
        HIP_TRY(hipGetLastError());
        t.start = d_off.p; t.len = d_len.p; t.count_f64 = d_cnt.p; t.ids = m->arena.p;
    }
    SKM_TRY(gene_counts_device(t, 1, n_tx, n_genes, tx_gene, unique, other, m->stream));
    drain.dismiss();
    return SKM_OK;
}

extern "C" int skm_sample_set_gene_counts(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                          int64_t cap_samples, int64_t *unique, int64_t *other)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s || cap_samples < 0 || (cap_samples && (!other || (n_genes > 0 && !unique)))) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.units.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    if (n_samples == 0) return SKM_OK;
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    GeneClasses t{};
    t.n_classes = (int64_t)v.start.size();
    if (t.n_classes) { t.start = v.d_start.p; t.len = v.d_len.p; t.count_f64 = v.d_count.p; t.sample = v.d_sample.p; t.ids = m->arena.p; }
    return gene_counts_device(t, n_samples, n_tx, n_genes, tx_gene, unique, other, m->stream);
}

extern "C" int skm_sample_set_plan(int64_t n_segments, const int32_t *sample, const int64_t *n_units, int64_t max_units,
                                   int64_t cap_entries, int64_t *n_entries, int64_t *entry_global, int64_t *entry_local,
                                   int32_t *entry_sample)
{
    if (n_segments < 0 || max_units < 1 || cap_entries < 0 || !n_entries || (n_segments && (!sample || !n_units)))
        return fail(SKM_ERR_ARG, "bad argument");
    std::deque<SetQueued> queue;
    std::unordered_map<int32_t, int64_t> next;
    for (int64_t i = 0; i < n_segments; ++i) {
        if (sample[i] < 0 || n_units[i] < 0) return fail(SKM_ERR_ARG, "bad segment %lld", (long long)i);
        if (n_units[i]) queue.push_back(SetQueued{sample[i], next[sample[i]], n_units[i], nullptr});
        next[sample[i]] += n_units[i];
    }
    SetLog log;
    std::vector<SetPart> parts;
    while (!queue.empty()) {
        set_cut_launch(queue, max_units, &parts);
        log.append(parts);
    }
    *n_entries = (int64_t)log.global.size();
    if (*n_entries > cap_entries) return SKM_OK;       // (the caller sizes its arrays and asks again)
    if (*n_entries && (!entry_global || !entry_local || !entry_sample)) return fail(SKM_ERR_ARG, "NULL entry arrays");
    std::copy(log.global.begin(), log.global.end(), entry_global);
    std::copy(log.local.begin(), log.local.end(), entry_local);
    std::copy(log.sample.begin(), log.sample.end(), entry_sample);
    return SKM_OK;
}

extern "C" int skm_sample_set_split(int64_t n_entries, const int64_t *entry_global, const int64_t *entry_local,
                                    const int32_t *entry_sample, int64_t n_samples, int64_t n_classes,
                                    const int64_t *first_seen, int32_t *class_sample, int64_t *class_local, int64_t *order,
                                    int64_t *sample_class_offsets)
{
    if (n_entries < 0 || n_samples < 0 || n_classes < 0 || !sample_class_offsets
            || (n_entries && (!entry_global || !entry_local || !entry_sample))
            || (n_classes && (!first_seen || !class_sample || !class_local || !order)))
        return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (n_entries == 0 || entry_global[0] != 0)) return fail(SKM_ERR_ARG, "the log does not start at unit 0");
    for (int64_t i = 0; i < n_entries; ++i)
        if (entry_sample[i] < 0 || entry_sample[i] >= n_samples || (i && entry_global[i] <= entry_global[i - 1]))
            return fail(SKM_ERR_ARG, "bad log entry %lld", (long long)i);
    for (int64_t k = 0; k < n_classes; ++k) {
        if (first_seen[k] < 0) return fail(SKM_ERR_ARG, "negative first-seen unit");
        const int64_t e = segment_find(entry_global, n_entries, first_seen[k]);
        class_sample[k] = entry_sample[e];
        class_local[k] = entry_local[e] + (first_seen[k] - entry_global[e]);
    }
    set_split_order(n_samples, n_classes, class_sample, class_local, order, sample_class_offsets);
    return SKM_OK;
}

// ------------------------------------------------------------ quantification
extern "C" int skm_effective_lengths(int device, const int64_t *fld, const double *lengths,
                                     int64_t n_tx, double *out)
{
    if (!fld || !lengths || !out || n_tx < 0) return fail(SKM_ERR_ARG, "bad argument");
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    SKM_TRY(set_device(device));
    if (n_tx == 0) return SKM_OK;
    DBuf<unsigned long long> d_fld; DBuf<double> d_len, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_fld.ensure(MAX_FRAGMENT_LENGTH)); SKM_TRY(d_len.ensure(n_tx)); SKM_TRY(d_out.ensure(n_tx));
    HIP_TRY(hipMemcpy(d_fld.p, fld, MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len.p, lengths, n_tx * 8, hipMemcpyHostToDevice));
    launch_effective_lengths(d_fld.p, d_len.p, n_tx, d_out.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, n_tx * 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copy home has waited for the kernel)
    return SKM_OK;
}

namespace {

// rows per group of n > 0 rows of 2000 words in, n_tx > 0 words out: 256 MB of output rows and of input rows
// at most (16 777 rows: one launch's gridDim.y holds them); SKM_EFF_MANY_GROUP (tests): fewer
int64_t effective_lengths_group(int64_t n, int64_t n_tx)
{
    int64_t group = std::min<int64_t>((int64_t)(1LL << 25) / n_tx, (int64_t)(1LL << 25) / MAX_FRAGMENT_LENGTH);
    if (const char *v = getenv("SKM_EFF_MANY_GROUP"))
        if (atoll(v) > 0) group = std::min<int64_t>(group, atoll(v));
    return std::max<int64_t>(1, std::min(group, n));
}

}  // namespace

// Groups of histograms, so that the rows staged in HBM, in and out, stay within 256 MB each (as many_rows_in);
// the lengths go up once.
extern "C" int skm_effective_lengths_many(int device, int64_t n, const int64_t *fld, const double *lengths,
                                          int64_t n_tx, double *out)
{
    if (n < 0 || n_tx < 0 || (n && (!fld || (n_tx && (!lengths || !out))))) return fail(SKM_ERR_ARG, "bad argument");
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    SKM_TRY(set_device(device));
    if (n == 0 || n_tx == 0) return SKM_OK;
    const int64_t group = effective_lengths_group(n, n_tx);
    DBuf<unsigned long long> d_fld; DBuf<double> d_len, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_fld.ensure((size_t)group * MAX_FRAGMENT_LENGTH)); SKM_TRY(d_len.ensure(n_tx)); SKM_TRY(d_out.ensure((size_t)(group * n_tx)));
    HIP_TRY(hipMemcpy(d_len.p, lengths, n_tx * 8, hipMemcpyHostToDevice));
    for (int64_t first = 0; first < n; first += group) {
        const int64_t here = std::min(group, n - first);
        HIP_TRY(hipMemcpy(d_fld.p, fld + first * MAX_FRAGMENT_LENGTH, (size_t)here * MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
        launch_effective_lengths_many(d_fld.p, here, d_len.p, n_tx, d_out.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + first * n_tx, d_out.p, (size_t)(here * n_tx) * 8, hipMemcpyDeviceToHost));
    }
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}

// The same rule for n rows of given weights, grouped as the histograms above.
extern "C" int skm_effective_lengths_weights(int device, int64_t n, const double *p, const double *lengths,
                                             int64_t n_tx, double *out)
{
    if (n < 0 || n_tx < 0 || !p || !lengths || !out) return fail(SKM_ERR_ARG, "bad argument");
    if (!length_weights_valid(p, n * MAX_FRAGMENT_LENGTH))
        return fail(SKM_ERR_ARG, "a fragment-length weight is negative or not finite");
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    SKM_TRY(set_device(device));
    if (n == 0 || n_tx == 0) return SKM_OK;
    const int64_t group = effective_lengths_group(n, n_tx);
    DBuf<double> d_p, d_len, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_p.ensure((size_t)group * MAX_FRAGMENT_LENGTH)); SKM_TRY(d_len.ensure(n_tx)); SKM_TRY(d_out.ensure((size_t)(group * n_tx)));
    HIP_TRY(hipMemcpy(d_len.p, lengths, n_tx * 8, hipMemcpyHostToDevice));
    for (int64_t first = 0; first < n; first += group) {
        const int64_t here = std::min(group, n - first);
        HIP_TRY(hipMemcpy(d_p.p, p + first * MAX_FRAGMENT_LENGTH, (size_t)here * MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
        launch_effective_lengths_weights(d_p.p, here, d_len.p, n_tx, d_out.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + first * n_tx, d_out.p, (size_t)(here * n_tx) * 8, hipMemcpyDeviceToHost));
    }
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}

namespace {

// SKM_EM_NO_COMPONENTS (tuning aid, looked up at every use so that one process can compare both forms):
// no component tiles are built, and an EM run steps the whole table with two launches per step
bool em_components_enabled() { return getenv("SKM_EM_NO_COMPONENTS") == nullptr; }
// what an EM run needs besides the handle's own state to step tiles: one rank (the all-reduce of several
// sits inside every step) and the fused rows + finalize launch (the unfused finalize walks every transcript)
bool em_tiles_possible(bool several_ranks)
{
    static const bool unfused = getenv("SKM_EM_UNFUSED") != nullptr;
    return !several_ranks && !unfused && em_components_enabled();
}

// several_ranks: the handle gets a communicator right after this call; the tiles, which only a one-rank EM
// can use, are then neither given room here nor built by quant_finish_setup
int quant_alloc(skm_quant *q, int device, int64_t n_tx, int64_t n_classes, int64_t n_ids, bool several_ranks = false)
{
    STALE_CHECK("quant_alloc entry");
    q->device = device;
    q->n_tx = n_tx;
    q->n_classes = n_classes;
    q->n_ids = n_ids;
    HIP_TRY(pool_stream_acquire(q->stream.out()));
    for (auto &e : q->ev) HIP_TRY(pool_event_acquire(e.out(), true));
    for (auto &e : q->chunk_ev) HIP_TRY(pool_event_acquire(e.out(), false));
    HIP_TRY(pool_pinned_acquire((void **)q->pinned.out()));
    const size_t C = (size_t)std::max<int64_t>(n_classes, 1), M = (size_t)std::max<int64_t>(n_ids, 1);
    const size_t T = (size_t)std::max<int64_t>(n_tx, 1);
    const size_t R = (size_t)quant_rows_upper_bound(n_tx, n_ids);
    SKM_TRY(q->cls_offset.ensure(C + 1));
    SKM_TRY(q->cls_count.ensure(C));
    SKM_TRY(q->inner.ensure(C));
    SKM_TRY(q->ids.ensure(M));
    SKM_TRY(q->perm.ensure(C));
    SKM_TRY(q->tx_cls.ensure(M));
    SKM_TRY(q->tx_row.ensure(T + 1));
    SKM_TRY(q->row_start.ensure(R + 1));
    SKM_TRY(q->row_tx.ensure(R));
    SKM_TRY(q->row_sum.ensure(R));
    SKM_TRY(q->eff_len.ensure(T));
    SKM_TRY(q->x0.ensure(T));
    SKM_TRY(q->x1.ensure(T));
    SKM_TRY(q->acc.ensure(T));
    SKM_TRY(q->ctl.ensure(EM_CTL_WORDS + EM_JUDGE_WORDS));       // (the tile judge's words lie behind the control block)
    SKM_TRY(q->part_max.ensure(EM_FINAL_BLOCKS));
    SKM_TRY(q->part_flags.ensure(EM_FINAL_BLOCKS));
    SKM_TRY(q->arrivals.ensure(T));
    HIP_TRY(hipMemsetAsync(q->arrivals.p, 0, T * sizeof(unsigned int), q->stream));
    if (em_tiles_possible(several_ranks)) {
        auto &t = q->tiles;
        SKM_TRY(t.tile_tx.ensure(T + 2)); SKM_TRY(t.tile_cls.ensure(T + 2));
        SKM_TRY(t.cls_pair.ensure(C + 1)); SKM_TRY(t.tx_pair.ensure(T + 1));
        SKM_TRY(t.tx_list.ensure(T)); SKM_TRY(t.cls_list.ensure(C));
        SKM_TRY(t.tx_label.ensure(T)); SKM_TRY(t.tx_tile.ensure(T)); SKM_TRY(t.cls_tile.ensure(C));
        SKM_TRY(t.cls_tx.ensure(M)); SKM_TRY(t.tx_cls.ensure(M));
        SKM_TRY(t.order.ensure(T + 1));
    }
    STALE_CHECK("quant_alloc exit");
    return SKM_OK;
}

QuantBuild quant_build_view(skm_quant *q)
{
    QuantBuild b{};
    b.n_tx = q->n_tx;
    b.n_classes = q->n_classes;
    b.n_ids = q->n_ids;
    b.cls_offset = q->cls_offset.p;
    b.ids = q->ids.p;
    b.cls_count = q->cls_count.p;
    b.tx_cls = q->tx_cls.p;
    b.tx_row = q->tx_row.p;
    b.row_start = q->row_start.p;
    b.row_tx = q->row_tx.p;
    b.n_rows_cap = (int64_t)q->row_tx.cap;
    if (q->tiles.tile_tx.p) {                      // (quant_alloc made room for the tiles)
        auto &t = q->tiles;
        b.tile_tx = t.tile_tx.p; b.tile_cls = t.tile_cls.p;
        b.tx_list = t.tx_list.p; b.cls_list = t.cls_list.p;
        b.cls_pair = t.cls_pair.p; b.tx_pair = t.tx_pair.p;
        b.tile_cls_tx = t.cls_tx.p; b.tile_tx_cls = t.tx_cls.p;
        b.tx_label = t.tx_label.p; b.tx_tile = t.tx_tile.p; b.cls_tile = t.cls_tile.p;
        b.tile_order = t.order.p;
    }
    return b;
}

int quant_finish_setup(skm_quant *q, const ClassTable *table, int64_t units_seen = -1)
{
    STALE_CHECK("quant_finish_setup");
    QuantBuild b = quant_build_view(q);
    b.first_seen_bound = units_seen > 0 ? units_seen : 0;      // first-seen values are unit indices below this
    const int64_t rows = quant_setup(table, b, q->perm.p, q->stream);
    if (rows < 0) return fail(SKM_ERR_HIP, "building the class views failed (%lld): %s", (long long)rows, quant_setup_failure());
    q->n_rows = rows;
    if (b.tile_tx) {
        q->tiles.built = true;
        q->tiles.n_tiles = b.tile_info[0];
        q->tiles.n_oversize = b.tile_info[1];
        if (q->tiles.n_tiles > 0) {
            SKM_TRY(q->tiles.step_max.ensure((size_t)(EM_CHUNK_MAX * q->tiles.n_tiles)));
            SKM_TRY(q->tiles.step_flags.ensure((size_t)(EM_CHUNK_MAX * q->tiles.n_tiles)));
            SKM_TRY(q->tiles.snap.ensure((size_t)EM_CHUNK_MAX * (size_t)q->n_tx));
        }
        if (q->tiles.n_oversize > 0 && q->tiles.n_tiles > 0) {
            // tiles AND components above the capacity: those become the residual problem (a table that
            // is one such component has no tiles and keeps the whole-table EM as it is)
            auto &r = q->tiles.residual;
            int64_t counts[3] = {0, 0, 0};
            if (quant_residual_count(b, counts, q->stream))
                return fail(SKM_ERR_HIP, "sizing the residual EM problem failed: %s", quant_setup_failure());
            r.n_classes = counts[0]; r.n_ids = counts[1]; r.n_rows = counts[2];
            SKM_TRY(r.cls_offset.ensure((size_t)r.n_classes + 1)); SKM_TRY(r.ids.ensure((size_t)std::max<int64_t>(r.n_ids, 1)));
            SKM_TRY(r.cls_src.ensure((size_t)std::max<int64_t>(r.n_classes, 1)));
            SKM_TRY(r.row_start.ensure((size_t)r.n_rows + 1)); SKM_TRY(r.row_tx.ensure((size_t)std::max<int64_t>(r.n_rows, 1)));
            SKM_TRY(r.tx_cls.ensure((size_t)std::max<int64_t>(r.n_ids, 1))); SKM_TRY(r.tx_row.ensure((size_t)q->n_tx + 1));
            SKM_TRY(r.cls_count.ensure((size_t)std::max<int64_t>(r.n_classes, 1)));
            SKM_TRY(r.inner.ensure((size_t)std::max<int64_t>(r.n_classes, 1)));
            SKM_TRY(r.row_sum.ensure((size_t)std::max<int64_t>(r.n_rows, 1)));
            QuantResidual out{};
            out.n_classes = r.n_classes; out.n_ids = r.n_ids; out.n_rows = r.n_rows;
            out.cls_offset = r.cls_offset.p; out.ids = r.ids.p; out.cls_src = r.cls_src.p;
            out.row_start = r.row_start.p; out.row_tx = r.row_tx.p; out.tx_cls = r.tx_cls.p; out.tx_row = r.tx_row.p;
            if (quant_residual_build(b, out, q->stream))
                return fail(SKM_ERR_HIP, "building the residual EM problem failed: %s", quant_setup_failure());
            r.built = true;
        }
    }
    return SKM_OK;
}

// ---- RCCL through dlopen: the library is only needed for N > 1
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;      // (table hand-over; optional)
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
};
struct UniqueId { char internal[128]; };
typedef int (*comm_init_fn)(void **, int, UniqueId, int);
Rccl g_rccl;
comm_init_fn g_comm_init = nullptr;

int load_rccl()
{
    if (g_rccl.lib) return SKM_OK;
    void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(SKM_ERR_COMM, "cannot load librccl.so: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(lib, "ncclGetUniqueId");
    g_comm_init = (comm_init_fn)dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(lib, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(lib, "ncclCommDestroy");
    g_rccl.CommCount = (int (*)(void *, int *))dlsym(lib, "ncclCommCount");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(lib, "ncclGetErrorString");
    g_rccl.Send = (int (*)(const void *, size_t, int, int, void *, hipStream_t))dlsym(lib, "ncclSend");
    g_rccl.Recv = (int (*)(void *, size_t, int, int, void *, hipStream_t))dlsym(lib, "ncclRecv");
    g_rccl.GroupStart = (int (*)())dlsym(lib, "ncclGroupStart");
    g_rccl.GroupEnd = (int (*)())dlsym(lib, "ncclGroupEnd");
    if (!g_rccl.GetUniqueId || !g_comm_init || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return fail(SKM_ERR_COMM, "librccl.so lacks a required symbol");
    g_rccl.lib = lib;
    return SKM_OK;
}

constexpr int NCCL_FLOAT64 = 8, NCCL_UINT64 = 5, NCCL_INT32 = 2, NCCL_SUM = 0;

#define NCCL_TRY(call)                                                                   \
    do {                                                                                 \
        int r_ = (call);                                                                 \
        if (r_ != 0)                                                                     \
            return fail(SKM_ERR_COMM, "%s failed: %s", #call,                            \
                        g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?");        \
    } while (0)

EmProblem em_problem(skm_quant *q, double rel_tol, double x_floor, int64_t max_iters,
                     int64_t fixed_iters)
{
    EmProblem p{};
    p.n_tx = q->n_tx;
    p.n_classes = q->n_classes;
    p.n_rows = q->n_rows;
    p.cls_offset = q->cls_offset.p;
    p.ids = q->ids.p;
    p.cls_count = q->cls_count.p;
    p.inner = q->inner.p;
    p.row_start = q->row_start.p;
    p.row_tx = q->row_tx.p;
    p.tx_cls = q->tx_cls.p;
    p.tx_row = q->tx_row.p;
    p.row_sum = q->row_sum.p;
    p.eff_len = q->eff_len.p;
    p.x[0] = q->x0.p;
    p.x[1] = q->x1.p;
    p.acc = q->acc.p;
    p.n_total = q->n_total;
    p.rel_tol = rel_tol;
    p.x_floor = x_floor;
    p.ctl = q->ctl.p;
    p.part_max = q->part_max.p;
    p.part_flags = q->part_flags.p;
    p.max_iters = max_iters;
    p.fixed_iters = fixed_iters;
    static const bool unfused = getenv("SKM_EM_UNFUSED") != nullptr;     // tuning aid: rows and finalize as two launches
    p.fused = q->comm || unfused ? 0 : 1;      // (several ranks: the all-reduce sits between rows and finalize)
    p.arrivals = q->arrivals.p;
    return p;
}

// one rank, every component within the tile capacity: the EM runs tile by tile in LDS (em_run_tiles)
bool em_uses_tiles(const skm_quant *q)
{
    return em_tiles_possible(q->comm != nullptr) && q->tiles.built && q->tiles.n_tiles > 0 &&
           (q->tiles.n_oversize == 0 || q->tiles.residual.built);
}

// The host one chunk of steps ahead of the device.  enqueue(slot) queues a chunk and, behind it, the copy
// of what the host reads about it to q->pinned + 8 * slot; chunk i + 1 is already queued when the host
// waits for chunk i's words, so the GPU never idles at a check-point (a converged EM turns at most one
// chunk of launches into no-ops).  Returns once stopped(words) says so, with the look-ahead chunk still
// queued and `words` those of the chunk that stopped.
template <class Enqueue, class Stopped>
int em_run_chunks_ahead(skm_quant *q, unsigned long long (&words)[8], Enqueue enqueue, Stopped stopped)
{
    auto enqueue_chunk = [&](int slot) -> int {
        SKM_TRY(enqueue(slot));
        HIP_TRY(hipEventRecord(q->chunk_ev[slot], q->stream));
        return SKM_OK;
    };
    SKM_TRY(enqueue_chunk(0));
    for (int slot = 0;; slot ^= 1) {
        SKM_TRY(enqueue_chunk(slot ^ 1));                 // stay one chunk ahead
        HIP_TRY(hipEventSynchronize(q->chunk_ev[slot]));
        memcpy(words, q->pinned + 8 * slot, sizeof(words));
        if (stopped(words)) return SKM_OK;
    }
}
bool em_ctl_done(const unsigned long long *ctl) { return ctl[CTL_DONE] != 0; }

// The component form of em_run's loop (after its preamble: control block cleared, ev[0] recorded).  Every
// chunk is ONE launch that steps all the tiles `chunk` times in LDS and leaves every step's abundances in
// the snapshot buffer -- the next chunk starts from the last of them -- and judges the chunk's steps in order
// itself (beside a residual problem: that problem's judge does).  The host stays one chunk ahead as before;
// the look-ahead chunk that finds the EM stopped (at step K) copies the tiles' entries of step K from the snapshots to x[K & 1],
// where the callers look for the result: no step runs twice and the stop costs no launch of its own.
int em_run_tiles(skm_quant *q, const EmProblem &p, int64_t chunk, int64_t *iters_out)
{
    auto &t = q->tiles;
    EmTiles tl{};
    tl.n_tiles = t.n_tiles;
    tl.tile_tx = t.tile_tx.p; tl.tile_cls = t.tile_cls.p;
    tl.tx_list = t.tx_list.p; tl.cls_list = t.cls_list.p;
    tl.cls_pair = t.cls_pair.p; tl.tx_pair = t.tx_pair.p;
    tl.cls_tx = t.cls_tx.p; tl.tx_cls = t.tx_cls.p;
    tl.step_max = t.step_max.p; tl.step_flags = t.step_flags.p;
    tl.snap = t.snap.p;
    // SKM_EM_TILE_ORDER (tuning aid, looked up at every run as SKM_EM_NO_COMPONENTS is): `identity` launches the
    // tiles in tile order, `reverse` smallest first; unset: largest first.  The results are the same bits.
    tl.order = t.order.p;
    if (const char *form = getenv("SKM_EM_TILE_ORDER")) {
        if (!strcmp(form, "identity")) tl.order = nullptr;
        else if (!strcmp(form, "reverse")) tl.order_reversed = 1;
        else return fail(SKM_ERR_ARG, "SKM_EM_TILE_ORDER is identity or reverse, not '%s'", form);
    }
    // With components above the capacity the residual problem runs beside the tiles, step by step with
    // the whole-table kernels on its own classes and rows (its transcripts' entries of x0 / x1; the
    // tiles' entries are the tiles' alone), and ITS judge takes the tiles' partials of the step along.
    const bool mixed = t.n_oversize > 0;
    // Tiles alone: the chunk launch judges its own steps (the workgroup that finishes last does), one launch a chunk.
    if (!mixed && !SKM_EM_JUDGE_LAUNCH) tl.judge = q->ctl.p + EM_CTL_WORDS;
    EmProblem pr = p;
    if (mixed) {
        auto &r = t.residual;
        pr.n_classes = r.n_classes; pr.n_rows = r.n_rows;
        pr.cls_offset = r.cls_offset.p; pr.ids = r.ids.p; pr.cls_count = r.cls_count.p; pr.inner = r.inner.p;
        pr.row_start = r.row_start.p; pr.row_tx = r.row_tx.p; pr.tx_cls = r.tx_cls.p; pr.tx_row = r.tx_row.p;
        pr.row_sum = r.row_sum.p;
        pr.fused = 1;
        pr.extra_max = t.step_max.p; pr.extra_flags = t.step_flags.p; pr.n_extra = t.n_tiles;
        launch_permute_f64(q->cls_count.p, r.cls_src.p, r.n_classes, r.cls_count.p, false, q->stream);   // (set_counts may have changed them)
    }
    int64_t queued = 0;
    auto enqueue_chunk = [&](int slot) -> int {
        launch_em_local_chunk(p, tl, queued == 0 ? q->x0.p : t.snap.p + (chunk - 1) * q->n_tx, (int)chunk, queued * chunk, q->stream);
        if (mixed) {
            pr.extra_first = queued * chunk;
            for (int64_t i = 0, k = queued * chunk; i < chunk; ++i, ++k) {
                launch_em_inner(pr, (int)(k & 1), i > 0, k, q->stream);
                launch_em_rows_finalize(pr, (int)(k & 1), q->stream);
            }
            launch_em_decide(pr, (queued + 1) * chunk, q->stream);
            q->launches += 2 * chunk + 2;
        } else {
#if SKM_EM_JUDGE_LAUNCH
            launch_em_local_decide(p, tl, queued * chunk, (int)chunk, q->stream);
            q->launches += 1;
#endif
            q->launches += 1;
        }
        ++queued;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q->pinned + 8 * slot, q->ctl.p, 8 * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    unsigned long long ctl[8] = {0};
    SKM_TRY(em_run_chunks_ahead(q, ctl, enqueue_chunk, em_ctl_done));
    // (a tile above the capacity cannot come out of the set-up; the kernel that meets one leaves it alone,
    // says so here and stops the run rather than going on with abundances nobody stepped)
    if (ctl[CTL_TILE_FAULT]) {
        HIP_TRY(hipStreamSynchronize(q->stream));
        return fail(SKM_ERR_STATE, "a component tile exceeds the tile capacity: the class views of this handle are damaged");
    }
    // (the look-ahead chunk, queued above, is the copy of step `steps` of the tiles to x[steps & 1])
    const int64_t steps = (int64_t)ctl[CTL_ITERS];
    HIP_TRY(hipEventRecord(q->ev[1], q->stream));
    HIP_TRY(hipEventSynchronize(q->ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
    q->t_em_ns += ms * 1e6;
    q->iters_total += (double)steps;
    if (iters_out) *iters_out = steps;
    if (ctl[CTL_UNDEFINED]) return fail(SKM_ERR_UNDEFINED, "no abundance above x_floor: numpy raises on max() of an empty selection");
    return SKM_OK;
}

// runs the EM from the abundance already in q->x0; result left in x[iters & 1]
int em_run(skm_quant *q, double rel_tol, double x_floor, int64_t max_iters, int64_t fixed_iters,
           int64_t *iters_out, int64_t chunk_steps = 16)
{
    // n = class_count.sum() over ALL ranks (infer.py:152)
    double n_total = q->n_total;
    if (q->comm && !q->n_total_reduced) {
        HIP_TRY(hipMemcpyAsync(q->acc.p, &n_total, 8, hipMemcpyHostToDevice, q->stream));
        NCCL_TRY(g_rccl.AllReduce(q->acc.p, q->acc.p, 1, NCCL_FLOAT64, NCCL_SUM, q->comm, q->stream));
        HIP_TRY(hipMemcpyAsync(&n_total, q->acc.p, 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
    }
    EmProblem p = em_problem(q, rel_tol, x_floor, max_iters, fixed_iters);
    p.n_total = n_total;
    // (with the control block the tile judge's words behind it: a run that ended in a tile fault or an error
    // leaves nothing there)
    HIP_TRY(hipMemsetAsync(q->ctl.p, 0, (EM_CTL_WORDS + EM_JUDGE_WORDS) * sizeof(unsigned long long), q->stream));
    int64_t k = 0;
    const int64_t chunk = fixed_iters > 0 ? std::min<int64_t>(fixed_iters, chunk_steps) : chunk_steps;
    HIP_TRY(hipEventRecord(q->ev[0], q->stream));
    if (em_uses_tiles(q) && chunk <= EM_CHUNK_MAX) return em_run_tiles(q, p, chunk, iters_out);
    // Steps are enqueued in chunks, the control block copied to pinned memory behind each (em_run_chunks_ahead).
    static const bool unfused_rows = getenv("SKM_EM_UNFUSED") != nullptr;
    auto enqueue_chunk = [&](int slot) -> int {
        for (int64_t i = 0; i < chunk; ++i, ++k) {
            // (the first step of a chunk follows the chunk-end em_decide: already judged)
            launch_em_inner(p, (int)(k & 1), i > 0, k, q->stream);
            if (q->comm) {
                // rows -> this rank's numerators (one launch, or two with SKM_EM_UNFUSED), summed over
                // the ranks, then the finalize on every rank alike
                if (unfused_rows) {
                    launch_em_rows(p, (int)(k & 1), q->stream);
                    launch_em_rows_to_acc(p, q->stream);
                } else {
                    launch_em_rows_acc(p, (int)(k & 1), q->stream);
                }
                NCCL_TRY(g_rccl.AllReduce(q->acc.p, q->acc.p, (size_t)q->n_tx, NCCL_FLOAT64, NCCL_SUM,
                                          q->comm, q->stream));
                launch_em_finalize(p, (int)(k & 1), true, q->stream);
            } else if (p.fused) {
                launch_em_rows_finalize(p, (int)(k & 1), q->stream);     // (rows + finalize: one launch)
            } else {
                launch_em_rows(p, (int)(k & 1), q->stream);
                launch_em_finalize(p, (int)(k & 1), false, q->stream);
            }
            q->launches += q->comm ? (unfused_rows ? 4 : 3) : (p.fused ? 2 : 3);
        }
        launch_em_decide(p, k, q->stream);
        q->launches += 1;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q->pinned + 8 * slot, q->ctl.p, 8 * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    unsigned long long ctl[8] = {0};
    SKM_TRY(em_run_chunks_ahead(q, ctl, enqueue_chunk, em_ctl_done));
    HIP_TRY(hipStreamSynchronize(q->stream));             // drain the look-ahead chunk (no-ops)
    HIP_TRY(hipEventRecord(q->ev[1], q->stream));
    HIP_TRY(hipEventSynchronize(q->ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
    q->t_em_ns += ms * 1e6;
    q->iters_total += (double)ctl[CTL_ITERS];
    if (iters_out) *iters_out = (int64_t)ctl[CTL_ITERS];
    if (ctl[CTL_UNDEFINED]) return fail(SKM_ERR_UNDEFINED, "no abundance above x_floor: numpy raises on max() of an empty selection");
    return SKM_OK;
}

}  // namespace

namespace {

// numpy.sum of a contiguous f8 array on the host, bit for bit (blocks of 8192, pairwise inside;
// see np_sum_blocks_kernel): n = class_count.sum() of infer.py:152 for counts that are not
// integers (blended single-cell tables, impute.py:248-252)
double np_pairwise_host(const double *a, int64_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_host(a, n2) + np_pairwise_host(a + n2, n - n2);
}

double np_sum_host(const double *a, int64_t n)
{
    double acc = 0.0;
    for (int64_t i = 0; i < n; i += 8192) acc += np_pairwise_host(a + i, std::min<int64_t>(8192, n - i));
    return acc;
}

}  // namespace

extern "C" int skm_quant_create(int device, int64_t n_tx, int64_t n_classes,
                                const int64_t *class_offsets, const int32_t *class_targets,
                                const double *class_counts, skm_quant **out)
{
    if (!out || n_tx <= 0 || n_classes < 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (!class_offsets || !class_targets || !class_counts))
        return fail(SKM_ERR_ARG, "NULL class arrays");
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    const int64_t M = n_classes ? class_offsets[n_classes] - class_offsets[0] : 0;
    for (int64_t c = 0; c < n_classes; ++c)
        if (class_offsets[c + 1] < class_offsets[c]) return fail(SKM_ERR_ARG, "class offsets are not monotone");
    const double total = np_sum_host(class_counts, n_classes);
    for (int64_t j = 0; j < M; ++j) {
        const int32_t t = class_targets[class_offsets[0] + j];
        if (t < 0 || t >= n_tx) return fail(SKM_ERR_ARG, "class target %d outside [0, n_tx)", t);
    }
    SKM_TRY(set_device(device));
    std::unique_ptr<skm_quant> q(new skm_quant());     // (any early return below: nothing is left behind)
    SKM_TRY(quant_alloc(q.get(), device, n_tx, n_classes, M));
    std::vector<int64_t> rebased(n_classes + 1, 0);
    for (int64_t c = 0; c <= n_classes && n_classes; ++c) rebased[c] = class_offsets[c] - class_offsets[0];
    HIP_TRY(hipMemcpy(q->cls_offset.p, rebased.data(), (n_classes + 1) * 8, hipMemcpyHostToDevice));
    if (n_classes) {
        HIP_TRY(hipMemcpy(q->cls_count.p, class_counts, n_classes * 8, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(q->ids.p, class_targets + class_offsets[0], M * 4, hipMemcpyHostToDevice));
    }
    q->n_total = total;
    SKM_TRY(quant_finish_setup(q.get(), nullptr));
    *out = q.release();                                 // (the caller's handle from here on)
    return SKM_OK;
}

extern "C" int skm_quant_create_from_mapper(skm_mapper *m, int64_t n_tx, skm_quant **out)
{
    if (!m || !out || n_tx <= 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes, M = m->host_arena_used;
    std::unique_ptr<skm_quant> q(new skm_quant());     // (any early return below: nothing is left behind)
    SKM_TRY(quant_alloc(q.get(), m->ix->device, n_tx, C, M));
    unsigned long long ctr[4];
    HIP_TRY(hipMemcpy(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));
    q->n_total = (double)(ctr[CTR_UNITS] - ctr[CTR_UNALIGNED]);
    SKM_TRY(quant_finish_setup(q.get(), &m->t, m->first_seen_bound));
    *out = q.release();                                 // (the caller's handle from here on)
    return SKM_OK;
}

// One sample from the resident class table to TPM without leaving the device:
// fragment-length histogram (all-reduced over the ranks of `comm`) -> effective
// lengths (mapper.py:134-141) -> start vector 1/l normalised with numpy's sum
// (infer.py:116-119) -> EM to the stop rule (:133-168) -> TPM scaling (:127-129).
extern "C" int skm_quant_infer(skm_mapper *m, skm_comm *comm, const double *lengths, int64_t n_tx,
                               double rel_tol, double x_floor, int64_t max_iters,
                               double *tpm, double *effective_lengths, int64_t *iters)
{
    if (!m || !lengths || n_tx <= 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    if (comm && comm->device != m->ix->device)
        return fail(SKM_ERR_ARG, "communicator and mapper live on different GPUs");
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes, M = m->host_arena_used;
    // SKM_TRACE_INFER=1: host wall time between the phases below, on stderr (tuning aid)
    static const bool trace = getenv("SKM_TRACE_INFER") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[skm_quant_infer] %-12s %8.1f us\n", what,
                std::chrono::duration<double, std::micro>(now - t_last).count());
        t_last = now;
    };
    // (the scratch is declared before the handle: the handle's destructor drains the stream first)
    DBuf<unsigned long long> fld;
    DBuf<double> sums;
    std::unique_ptr<skm_quant> q(new skm_quant());
    SKM_TRY(quant_alloc(q.get(), m->ix->device, n_tx, C, M, comm != nullptr));
    if (comm) { q->comm = comm->comm; q->rank = comm->rank; q->world = comm->world; }
    lap("alloc");
    const int64_t n_blocks = (n_tx + 8191) / 8192;
    SKM_TRY(fld.ensure(MAX_FRAGMENT_LENGTH + 1));
    SKM_TRY(sums.ensure(n_blocks + 2));
    double *const total = sums.p + n_blocks;          // [0] sum, [1] sum / divisor
    unsigned long long ctr[4] = {0, 0, m->host_unaligned, m->host_units};
    if (!m->host_totals_valid)
        HIP_TRY(hipMemcpy(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));   // (mapper stream is idle)
    unsigned long long aligned = ctr[CTR_UNITS] - ctr[CTR_UNALIGNED];
    HIP_TRY(hipMemcpyAsync(fld.p, m->counters.p + CTR_FLD, MAX_FRAGMENT_LENGTH * 8,
                           hipMemcpyDeviceToDevice, q->stream));
    if (q->comm) {
        // merge_fragment_lengths over the ranks, and with it (word 2000 of the same
        // collective) n = class_count.sum() of infer.py:152 over ALL ranks.  Whether there
        // is anything to quantify (infer.py:106-107 tests the merged table) must be decided
        // on the global sum: a rank whose shard produced no class still has to take part
        // in every collective of the EM below, with empty class views.
        q->pinned[32] = aligned;
        HIP_TRY(hipMemcpyAsync(fld.p + MAX_FRAGMENT_LENGTH, q->pinned + 32, 8, hipMemcpyHostToDevice, q->stream));
        NCCL_TRY(g_rccl.AllReduce(fld.p, fld.p, MAX_FRAGMENT_LENGTH + 1, NCCL_UINT64, NCCL_SUM, q->comm,
                                  q->stream));
        HIP_TRY(hipMemcpyAsync(q->pinned + 32, fld.p + MAX_FRAGMENT_LENGTH, 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        aligned = q->pinned[32];
        q->n_total_reduced = true;
        // test hook: "the other ranks aligned this many units" -- a rank whose own shard produced no
        // class (C == 0) then goes through the set-up and every collective of the EM with empty
        // class views, a state one rank cannot reach by itself (tests/test_gpu_parity.py)
        if (const char *v = getenv("SKM_TEST_ALIGNED_GLOBAL")) aligned += strtoull(v, nullptr, 10);
    }
    q->n_total = (double)aligned;
    HIP_TRY(hipMemcpyAsync(q->x1.p, lengths, n_tx * 8, hipMemcpyHostToDevice, q->stream));
    if (m->use_length_weights)                 // a fragment-length model: the same on every rank
        launch_effective_lengths_weights(m->length_weights.p, 1, q->x1.p, n_tx, q->eff_len.p, q->stream);
    else
        launch_effective_lengths(fld.p, q->x1.p, n_tx, q->eff_len.p, q->stream);
    // (the effective lengths go home at the end, with the TPM: a copy to pageable memory holds the
    // host up, and the kernels that follow are not launched meanwhile)
    // quantify(): no class -> zeros (infer.py:106-107); over several ranks "no class anywhere"
    // is "no aligned unit anywhere" (every aligned unit belongs to a class)
    if (q->comm ? aligned == 0 : C == 0) {
        if (effective_lengths)
            HIP_TRY(hipMemcpyAsync(effective_lengths, q->eff_len.p, n_tx * 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        if (tpm) memset(tpm, 0, (size_t)n_tx * 8);
        if (iters) *iters = 0;
        return SKM_OK;
    }
    launch_reciprocal(q->eff_len.p, n_tx, q->x0.p, q->stream);
    launch_np_sum(q->x0.p, n_tx, 1.0, sums.p, total, q->stream);
    launch_divide(q->x0.p, n_tx, total, false, 0.0, q->stream);
    lap("start vector");
    SKM_TRY(quant_finish_setup(q.get(), &m->t, m->first_seen_bound));
    lap("setup");
    if (trace) fprintf(stderr, "[skm_quant_infer] %lld classes, %lld transcripts, %lld rows\n", (long long)C, (long long)n_tx,
                       (long long)q->n_rows);
    int64_t it = 0;
    SKM_TRY(em_run(q.get(), rel_tol, x_floor, max_iters, 0, &it));
    lap("em");
    m->t_em_ns += q->t_em_ns;
    m->em_iters += (double)it;
    double *const x = (it & 1) ? q->x1.p : q->x0.p;
    launch_np_sum(x, n_tx, 1000000.0, sums.p, total, q->stream);
    launch_divide(x, n_tx, total + 1, true, 0.001, q->stream);
    launch_np_sum(x, n_tx, 1000000.0, sums.p, total, q->stream);
    launch_divide(x, n_tx, total + 1, false, 0.0, q->stream);
    HIP_TRY(hipGetLastError());
    if (tpm) HIP_TRY(hipMemcpyAsync(tpm, x, n_tx * 8, hipMemcpyDeviceToHost, q->stream));
    if (effective_lengths)
        HIP_TRY(hipMemcpyAsync(effective_lengths, q->eff_len.p, n_tx * 8, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    lap("tpm");
    if (iters) *iters = it;
    q.reset();
    lap("destroy");
    return SKM_OK;
}

extern "C" int skm_quant_destroy(skm_quant *q)
{
    if (!q) return SKM_OK;
    STALE_CHECK("quant_destroy entry");
    delete q;
    STALE_CHECK("quant_destroy exit");
    return SKM_OK;
}

extern "C" int skm_quant_em(skm_quant *q, double *x, const double *l, double rel_tol, double x_floor,
                            int64_t max_iters, int64_t fixed_iters, int64_t *iters)
{
    if (!q || !x || !l) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    HIP_TRY(hipMemcpyAsync(q->x0.p, x, q->n_tx * 8, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->eff_len.p, l, q->n_tx * 8, hipMemcpyHostToDevice, q->stream));
    int64_t it = 0;
    SKM_TRY(em_run(q, rel_tol, x_floor, max_iters, fixed_iters, &it));
    HIP_TRY(hipMemcpy(x, (it & 1) ? q->x1.p : q->x0.p, q->n_tx * 8, hipMemcpyDeviceToHost));
    if (iters) *iters = it;
    return SKM_OK;
}

extern "C" int skm_quant_components(skm_quant *q, int64_t info[8], int32_t *tx_label, int32_t *tx_tile,
                                    int32_t *class_tile)
{
    if (!q || !info) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    const auto &t = q->tiles;
    info[0] = t.built ? 1 : 0;
    info[1] = t.n_tiles;
    info[2] = t.n_oversize;
    info[3] = em_uses_tiles(q) ? 1 : 0;
    info[4] = EM_TILE_PAIRS; info[5] = EM_TILE_CLASSES; info[6] = EM_TILE_TX; info[7] = EM_TILE_SEGMENT;
    if (!t.built) {
        if (tx_label || tx_tile || class_tile) return fail(SKM_ERR_ARG, "no component tiles were built for this handle");
        return SKM_OK;
    }
    HIP_TRY(hipStreamSynchronize(q->stream));
    if (tx_label) HIP_TRY(hipMemcpy(tx_label, t.tx_label.p, q->n_tx * 4, hipMemcpyDeviceToHost));
    if (tx_tile) HIP_TRY(hipMemcpy(tx_tile, t.tx_tile.p, q->n_tx * 4, hipMemcpyDeviceToHost));
    if (class_tile && q->n_classes) {
        // internal (locality) order -> the caller's class order
        std::vector<int32_t> tile(q->n_classes), perm(q->n_classes);
        HIP_TRY(hipMemcpy(tile.data(), t.cls_tile.p, q->n_classes * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(perm.data(), q->perm.p, q->n_classes * 4, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < q->n_classes; ++k) class_tile[perm[k]] = tile[k];
    }
    return SKM_OK;
}

extern "C" int skm_quant_set_counts(skm_quant *q, const double *class_counts)
{
    if (!q || (!class_counts && q->n_classes)) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    const double total = np_sum_host(class_counts, q->n_classes);
    if (q->n_classes) {
        // caller's class order -> internal (locality) order
        SKM_TRY(q->cls_count_saved.ensure(q->n_classes));
        HIP_TRY(hipMemcpyAsync(q->cls_count_saved.p, class_counts, q->n_classes * 8, hipMemcpyHostToDevice, q->stream));
        launch_permute_f64(q->cls_count_saved.p, q->perm.p, q->n_classes, q->cls_count.p, false, q->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(q->stream));
    }
    q->n_total = total;
    return SKM_OK;
}

namespace {

// ---- many EM problems on ONE class structure: the group loop that `-b N` (bootstrap_impl), K count
// vectors of the caller's (skm_quant_em_many) and the second round of `impute` (skm_quant_em_blend)
// share.  The callers differ in where a problem's class counts come from, and say so with
//     fill(first, n, rows, totals): queue on the handle's stream whatever leaves rows[i][C] (device,
//     INTERNAL class order) = the class counts of problems first + i, i < n, and totals[2 i] (device;
//     pairs, as launch_np_sum_many leaves them) = their sums as numpy adds them up in the caller's order.
// Problem b starts from x0, runs the EM of seekmer/infer.py:133-168 to its stopping rule and leaves
// out[b][T]: the raw result, or with `tpm` what quantify() makes of it (infer.py:127-129).  The caller
// holds q->mu, has set the device and has checked its arguments; C > 0.  On every exit the handle
// holds the class counts and the total it came with.
//   batched: EM_BATCH problems side by side with the device refilling the places (skm_em_batch.hip);
//   otherwise (resampled counts wanted, a step cap set, a communicator attached: its collectives
//   must stay matched) one problem after the other through the single-problem EM.
//   slot_cap > 0 (tests): at most that many problems per group.
template <class Fill>
int em_group_run(skm_quant *q, int64_t n_problems, Fill &&fill, bool batched, int64_t slot_cap, const double *x0,
                 const double *l, double rel_tol, double x_floor, int64_t max_iters, double *out, int64_t *iters_out,
                 bool tpm)
{
    const int64_t C = q->n_classes, T = q->n_tx;
    skm_quant::Batch &w = q->batch;
    // the problems' results stay in HBM and come back in groups (one copy per group, not one per problem)
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(n_problems, (int64_t)(1LL << 28) / T));
    const int64_t by_counts = std::max<int64_t>(1, (int64_t)((1LL << 31) / (8 * std::max<int64_t>(C, 1))));
    int64_t slots = batched ? std::max<int64_t>(1, std::min(group, by_counts)) : 1;
    if (slot_cap > 0) slots = std::min(slots, slot_cap);
    SKM_TRY(q->cls_count_saved.ensure(C));
    SKM_TRY(q->x_start.ensure(T));
    SKM_TRY(q->boot_out.ensure((size_t)(slots * T)));
    SKM_TRY(w.totals.ensure((size_t)(2 * slots)));
    HIP_TRY(hipMemcpyAsync(q->cls_count_saved.p, q->cls_count.p, C * 8, hipMemcpyDeviceToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->eff_len.p, l, T * 8, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->x_start.p, x0, T * 8, hipMemcpyHostToDevice, q->stream));
    const double saved_total = q->n_total;
    int rc = SKM_OK;
    DBuf<double> sums;                               // (before `restore`: freed after the stream has drained)
    auto restore = on_exit([&]() {                   // every exit: the handle holds its own counts again
        (void)hipMemcpyAsync(q->cls_count.p, q->cls_count_saved.p, C * 8, hipMemcpyDeviceToDevice, q->stream);
        (void)hipStreamSynchronize(q->stream);
        q->n_total = saved_total;
    });
    // One problem the careful way (host-checked chunks of the single-problem EM): its counts straight
    // into the handle's, EM from x_start, result to `dst` (HBM).
    auto problem_checked = [&](int64_t b, int64_t *it_out, double *dst) -> int {
        SKM_TRY(fill(b, (int64_t)1, q->cls_count.p, w.totals.p));
        HIP_TRY(hipGetLastError());
        double total = 0.0;
        HIP_TRY(hipMemcpyAsync(&total, w.totals.p, 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipMemcpyAsync(q->x0.p, q->x_start.p, T * 8, hipMemcpyDeviceToDevice, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        q->n_total = total;
        SKM_TRY(em_run(q, rel_tol, x_floor, max_iters, 0, it_out, 8));
        HIP_TRY(hipMemcpyAsync(dst, (*it_out & 1) ? q->x1.p : q->x0.p, T * 8, hipMemcpyDeviceToDevice, q->stream));
        if (iters_out) iters_out[b] = *it_out;
        return SKM_OK;
    };
    // infer.py:127-129 on `count` results in HBM (TPM scaling with numpy's sums), when TPM is asked for
    auto scale = [&](double *results, int64_t count) -> int {
        if (!tpm || count <= 0) return SKM_OK;
        const int64_t n_blocks = (T + 8191) / 8192;
        SKM_TRY(sums.ensure((size_t)(count * (n_blocks + 2))));
        double *const totals = sums.p + count * n_blocks;            // (sum, sum / 1e6) per problem
        launch_np_sum_many(results, T, count, T, 1000000.0, sums.p, totals, q->stream);
        launch_divide_many(results, T, count, T, totals + 1, true, 0.001, q->stream);
        launch_np_sum_many(results, T, count, T, 1000000.0, sums.p, totals, q->stream);
        launch_divide_many(results, T, count, T, totals + 1, false, 0.0, q->stream);
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    auto send_home = [&](int64_t first, int64_t count) -> int {     // boot_out[0 .. count) = problems first ..
        if (count <= 0) return SKM_OK;
        SKM_TRY(scale(q->boot_out.p, count));
        HIP_TRY(hipMemcpyAsync(out + first * T, q->boot_out.p, (size_t)count * T * 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        return SKM_OK;
    };
    if (!batched) {
        for (int64_t b = 0; b < n_problems; ++b) {
            int64_t it = 0;
            SKM_TRY(problem_checked(b, &it, q->boot_out.p));
            SKM_TRY(send_home(b, 1));
        }
        return rc;
    }
    // EM_BATCH problems sit side by side in the batched EM (skm_em_batch.hip) and THE DEVICE keeps the
    // working set full: the class counts of a whole group of problems are made first (HBM has the
    // room: 8 MB per problem at a million classes), and after every step two small launches take
    // the results of the problems that have latched their stopping rule and put the next ones in
    // their places (launch_em_batch_manage) -- no host look between steps; the host queues steps
    // and reads now and then how many problems have finished.  (Through round 3's first half the
    // host looked every four steps and refilled: ~100 looks and a fifth of the phase's wall time in
    // gaps.)  Step counts have a long tail (most replicates of the 20 M-pair table stop near 30
    // steps, one in six needs 60-90): problems that wait for the slowest of a fixed group of eight
    // waste half the working set's steps.  Every problem still runs the single-problem EM's steps bit
    // for bit, whoever its neighbours are and whenever it starts.
    SKM_TRY(w.cls_count.ensure((size_t)C * EM_BATCH)); SKM_TRY(w.inner.ensure((size_t)C * EM_BATCH));
    SKM_TRY(w.row_sum.ensure((size_t)std::max<int64_t>(q->n_rows, 1) * EM_BATCH));
    SKM_TRY(w.x0.ensure((size_t)T * EM_BATCH)); SKM_TRY(w.x1.ensure((size_t)T * EM_BATCH));
    SKM_TRY(w.part_max.ensure((size_t)EM_FINAL_BLOCKS * EM_BATCH));
    SKM_TRY(w.part_flags.ensure((size_t)EM_FINAL_BLOCKS * EM_BATCH));
    SKM_TRY(w.ctl.ensure(32 + EM_BATCH));                        // (the places' totals lie behind the control block)
    SKM_TRY(w.mgr.ensure(64));
    SKM_TRY(w.counts_all.ensure((size_t)slots * C));
    SKM_TRY(w.iters.ensure((size_t)slots));
    EmBatchProblem p{};
    p.n_tx = T; p.n_classes = C; p.n_rows = q->n_rows;
    p.cls_offset = q->cls_offset.p; p.ids = q->ids.p; p.row_start = q->row_start.p; p.row_tx = q->row_tx.p;
    p.tx_cls = q->tx_cls.p; p.tx_row = q->tx_row.p; p.eff_len = q->eff_len.p;
    p.cls_count = w.cls_count.p; p.inner = w.inner.p; p.row_sum = w.row_sum.p;
    p.x[0] = w.x0.p; p.x[1] = w.x1.p;
    p.place_total = reinterpret_cast<double *>(w.ctl.p + 32);
    p.rel_tol = rel_tol; p.x_floor = x_floor;
    p.ctl = w.ctl.p; p.part_max = w.part_max.p; p.part_flags = w.part_flags.p;
    p.managed = 1;
    p.mgr = w.mgr.p;
    p.iters_out = w.iters.p;
    p.fused = getenv("SKM_EM_UNFUSED") ? 0 : 1;
    p.arrivals = q->arrivals.p;
    int64_t chunk = 16;                                          // steps queued between two looks at the progress
    if (const char *e = getenv("SKM_BOOTSTRAP_CHUNK")) chunk = std::max<int64_t>(1, atoll(e));   // (tests)
    unsigned long long *const look = q->pinned + 64;             // 64 + 8 words of the pinned block
    std::vector<int64_t> iters_host((size_t)slots);
    std::vector<double> totals_host((size_t)(2 * slots));        // (what the tail hands to the single-problem EM)
    for (int64_t w0 = 0; w0 < n_problems; w0 += slots) {
        const int64_t n = std::min(n_problems, w0 + slots) - w0;
        SKM_TRY(fill(w0, n, w.counts_all.p, w.totals.p));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(totals_host.data(), w.totals.p, (size_t)(2 * n) * 8, hipMemcpyDeviceToHost, q->stream));
        launch_em_batch_manage_init(p, w.mgr.p, look, n, w.counts_all.p, w.totals.p, q->x_start.p, q->boot_out.p, q->stream);
        HIP_TRY(hipGetLastError());
        for (int64_t k = 0;;) {
            for (int64_t i = 0; i < chunk; ++i, ++k) {
                launch_em_batch_step(p, k, q->stream);        // (its first kernel also plans for what has stopped)
                launch_em_batch_manage(p, w.mgr.p, w.counts_all.p, w.totals.p, q->x_start.p, q->boot_out.p, w.iters.p, k, true,
                                       q->stream);
            }
            // before the host looks, the last pass is judged too (otherwise only the next step's first
            // kernel would) and what it stops is taken: a place that is still occupied then is running
            launch_em_batch_decide(p, k, q->stream);
            launch_em_batch_manage(p, w.mgr.p, w.counts_all.p, w.totals.p, q->x_start.p, q->boot_out.p, w.iters.p, k - 1, false,
                                   q->stream);
            q->launches += 4 * chunk + 3;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(look, w.mgr.p, 24 * 8, hipMemcpyDeviceToHost, q->stream));
            HIP_TRY(hipMemcpyAsync(look + 24, w.ctl.p, 8 * 8, hipMemcpyDeviceToHost, q->stream));
            HIP_TRY(hipStreamSynchronize(q->stream));
            const unsigned long long *const all_done = look + 24;   // (the head of the control block, behind mgr's words)
            if (look[MGR_UNDEFINED])
                return fail(SKM_ERR_UNDEFINED, "no abundance above x_floor: numpy raises on max() of an empty selection");
            if (all_done[BCTL_ALL_DONE]) break;                  // every problem of the group has finished
            if (k > (1LL << 24)) return fail(SKM_ERR_STATE, "the batched EM does not stop");
            // The tail: nothing left to put in, a few problems still running.  A step of the
            // working set costs the same however many places are live (~5 single-problem steps), so
            // the last three or fewer go on one by one in the single-problem EM, from where they are.
            int live = 0;
            for (int r = 0; r < EM_BATCH; ++r) live += look[MGR_REP + r] != 0;
            if (look[MGR_NEXT] >= look[MGR_COUNT] && live <= 3) {
                for (int r = 0; r < EM_BATCH; ++r) {
                    if (look[MGR_REP + r] == 0) continue;
                    const int64_t rep = (int64_t)look[MGR_REP + r] - 1, since = (int64_t)look[MGR_SINCE + r];
                    launch_em_batch_take(p.x[k & 1], T, r, q->x0.p, q->stream);
                    launch_em_batch_take(w.cls_count.p, C, r, q->cls_count.p, q->stream);
                    HIP_TRY(hipGetLastError());
                    q->n_total = totals_host[(size_t)(2 * rep)];
                    int64_t more = 0;
                    SKM_TRY(em_run(q, rel_tol, x_floor, max_iters, 0, &more, 8));
                    HIP_TRY(hipMemcpyAsync(q->boot_out.p + rep * T, (more & 1) ? q->x1.p : q->x0.p, (size_t)T * 8,
                                           hipMemcpyDeviceToDevice, q->stream));
                    const int64_t steps = k - since + more;
                    HIP_TRY(hipMemcpyAsync(w.iters.p + rep, &steps, 8, hipMemcpyHostToDevice, q->stream));
                    HIP_TRY(hipStreamSynchronize(q->stream));      // (`steps` lives on this frame)
                    q->iters_total -= (double)more;                // (em_run has counted its own; the sum below counts all)
                }
                break;
            }
        }
        HIP_TRY(hipMemcpyAsync(iters_host.data(), w.iters.p, (size_t)n * 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        for (int64_t i = 0; i < n; ++i) {
            if (iters_out) iters_out[w0 + i] = iters_host[(size_t)i];
            q->iters_total += (double)iters_host[(size_t)i];
        }
        SKM_TRY(send_home(w0, n));
    }
    return rc;
}

// Replicate b of the call (b = 0 .. n_boot - 1) is replicate number rep_first + b * rep_step of the
// `-b N` run: its draw depends on (seed, that number) alone, so a rank's share of the replicates
// gives the same results as the one-GPU loop, replicate by replicate.
int bootstrap_impl(skm_quant *q, int64_t n_boot, uint64_t seed, const double *x0,
                   const double *l, double rel_tol, double x_floor, int64_t max_iters,
                   double *out, int64_t *counts_out, int64_t *iters_out, bool tpm,
                   int64_t rep_first = 0, int64_t rep_step = 1)
{
    if (!q || !x0 || !l || !out || n_boot < 0 || rep_first < 0 || rep_step < 1) return fail(SKM_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    // (seekmer/infer.py:108-111 resamples the table of the WHOLE sample: a handle that holds one
    // rank's share of the classes -- a communicator of several ranks attached -- cannot)
    if (q->comm && q->world > 1)
        return fail(SKM_ERR_STATE, "bootstraps resample the merged class table: detach the communicator "
                                   "(skm_quant_set_comm(quant, NULL)) and give every rank the merged table");
    auto number = [&](int64_t b) { return (uint64_t)(rep_first + b * rep_step); };
    const int64_t C = q->n_classes;
    if (C == 0) return fail(SKM_ERR_STATE, "no classes to resample");
    // integer cumulative counts of the observed table
    SKM_TRY(q->cum.ensure(C));
    SKM_TRY(q->tile_total.ensure(4096));
    SKM_TRY(q->inner.ensure(C));
    std::vector<double> cnt(C);
    HIP_TRY(hipMemcpyAsync(cnt.data(), q->cls_count.p, C * 8, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    std::vector<unsigned long long> cum(C);
    unsigned long long run = 0;
    for (int64_t c = 0; c < C; ++c) { run += (unsigned long long)cnt[c]; cum[c] = run; }
    if (run >= (1ULL << 32)) return fail(SKM_ERR_STATE, "more than 2^32 - 1 units to resample");
    HIP_TRY(hipMemcpyAsync(q->cum.p, cum.data(), C * 8, hipMemcpyHostToDevice, q->stream));
    const int64_t n_draws = (int64_t)run;            // n = class_count.sum(), infer.py:109
    // (a resample keeps the total: the same for every replicate; filled once, never changed while the
    // call runs, so the copies out of it need no synchronisation of their own)
    const std::vector<double> totals((size_t)(2 * std::max<int64_t>(n_boot, 1)), (double)n_draws);
    // a group's counts: one multinomial draw per replicate, straight into its row
    auto draw = [&](int64_t first, int64_t n, double *rows, double *totals_dev) -> int {
        for (int64_t i = 0; i < n; ++i)
            if (!launch_multinomial(q->cum.p, C, n_draws, seed, number(first + i), q->tile_total.p, rows + (size_t)i * C, 1,
                                    q->stream))
                return fail(SKM_ERR_STATE, "class table too large to resample (%lld classes)", (long long)C);
        HIP_TRY(hipGetLastError());
        for (int64_t i = 0; i < n && counts_out; ++i) {
            // internal (locality) class order -> caller's order; the counts fit a double exactly
            launch_permute_f64(rows + (size_t)i * C, q->perm.p, C, q->inner.p, true, q->stream);
            std::vector<double> as_double(C);
            HIP_TRY(hipMemcpyAsync(as_double.data(), q->inner.p, C * 8, hipMemcpyDeviceToHost, q->stream));
            HIP_TRY(hipStreamSynchronize(q->stream));
            for (int64_t c = 0; c < C; ++c) counts_out[(first + i) * C + c] = (int64_t)as_double[c];
        }
        HIP_TRY(hipMemcpyAsync(totals_dev, totals.data(), (size_t)(2 * n) * 8, hipMemcpyHostToDevice, q->stream));
        return SKM_OK;
    };
    // With the resampled counts wanted, a step cap set or a communicator attached (its collectives
    // must stay matched) every replicate goes the careful way.
    const bool batched = !counts_out && !q->comm && max_iters <= 0;
    return em_group_run(q, n_boot, draw, batched, 0, x0, l, rel_tol, x_floor, max_iters, out, iters_out, tpm);
}

// Rows of class counts in the caller's order, `produce`d piece by piece into a staging buffer, on their
// way into a group of em_group_run: the sum of each row as numpy adds it up (what skm_quant_set_counts
// computes on the host), then the row in the internal (locality) class order.  A piece is at most
// 256 MB, so neither side holds a second copy of a whole group and the caller's rows need not be
// page-locked.  The staging buffers belong to the call (ManyStage: sized before anything is queued, given
// back to the pool when the call ends), not to the handle, which may live long (infer._quant_for).
int64_t many_piece(int64_t n_classes, int64_t n_rows)
{
    return std::max<int64_t>(1, std::min<int64_t>(n_rows, (int64_t)(1LL << 25) / std::max<int64_t>(n_classes, 1)));
}

struct ManyStage {
    DBuf<double> rows, sums;
    int reserve(int64_t n_classes, int64_t n_rows)
    {
        const int64_t piece = many_piece(n_classes, n_rows);
        SKM_TRY(rows.ensure((size_t)(piece * n_classes)));
        SKM_TRY(sums.ensure((size_t)(piece * ((n_classes + 8191) / 8192))));
        return SKM_OK;
    }
};

template <class Produce>
int many_rows_in(skm_quant *q, ManyStage &stage, int64_t first, int64_t n, double *rows, double *totals,
                 int64_t n_rows_of_call, Produce &&produce)
{
    const int64_t C = q->n_classes, piece = many_piece(C, n_rows_of_call);
    for (int64_t i0 = 0; i0 < n; i0 += piece) {
        const int64_t m = std::min(piece, n - i0);
        SKM_TRY(produce(first + i0, m, stage.rows.p));
        launch_np_sum_many(stage.rows.p, C, m, C, 1.0, stage.sums.p, totals + 2 * i0, q->stream);
        launch_permute_rows_f64(stage.rows.p, q->perm.p, C, m, rows + (size_t)i0 * C, q->stream);
        HIP_TRY(hipGetLastError());
    }
    return SKM_OK;
}

// what the two entry points below check alike, before the handle is touched
int many_check(const skm_quant *q, int64_t n_sets, const double *x0, const double *l, const double *out, bool sources)
{
    if (!q || n_sets < 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_sets > 0 && (!x0 || !l || !out || !sources)) return fail(SKM_ERR_ARG, "NULL argument");
    return SKM_OK;
}

int many_state_check(const skm_quant *q)
{
    // (one rank's share of the classes is not the table the caller's counts belong to)
    if (q->comm && q->world > 1)
        return fail(SKM_ERR_STATE, "bootstraps resample the merged class table: detach the communicator "
                                   "(skm_quant_set_comm(quant, NULL)) and give every rank the merged table");
    if (q->n_classes == 0) return fail(SKM_ERR_STATE, "no classes to quantify");
    return SKM_OK;
}

int64_t many_slot_cap()
{
    const char *e = getenv("SKM_EM_MANY_SLOTS");                  // (tests: several groups from a few problems)
    return e ? std::max<int64_t>(1, atoll(e)) : 0;
}

}  // namespace

extern "C" int skm_quant_em_many(skm_quant *q, int64_t n_sets, const double *counts, const double *x0, const double *l,
                                 double rel_tol, double x_floor, int tpm, double *out, int64_t *iters_out)
{
    SKM_TRY(many_check(q, n_sets, x0, l, out, counts != nullptr));
    if (n_sets == 0) return SKM_OK;                               // (nothing to do, with or without a GPU)
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    SKM_TRY(many_state_check(q));
    const int64_t C = q->n_classes;
    ManyStage stage;                                              // (before the guard: freed after the stream has drained)
    SKM_TRY(stage.reserve(C, n_sets));
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(q->stream); });
    auto upload = [&](int64_t first, int64_t m, double *stage) -> int {
        HIP_TRY(hipMemcpyAsync(stage, counts + (size_t)first * C, (size_t)m * C * 8, hipMemcpyHostToDevice, q->stream));
        return SKM_OK;
    };
    auto fill = [&](int64_t first, int64_t n, double *rows, double *totals) -> int {
        return many_rows_in(q, stage, first, n, rows, totals, n_sets, upload);
    };
    return em_group_run(q, n_sets, fill, !q->comm, many_slot_cap(), x0, l, rel_tol, x_floor, 0, out, iters_out, tpm != 0);
}

extern "C" int skm_quant_em_blend(skm_quant *q, int64_t n_cells, const int32_t *class_cell, const double *weight,
                                  const double *cell_total, const double *x0, const double *l, double rel_tol,
                                  double x_floor, int tpm, double *out, int64_t *iters_out, double *counts_out)
{
    SKM_TRY(many_check(q, n_cells, x0, l, out, class_cell && weight && cell_total));
    if (n_cells == 0) return SKM_OK;                              // (nothing to do, with or without a GPU)
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    SKM_TRY(many_state_check(q));
    const int64_t C = q->n_classes;
    for (int64_t k = 0; k < C; ++k)
        if (class_cell[k] < 0 || class_cell[k] >= n_cells)
            return fail(SKM_ERR_ARG, "class_cell[%lld] = %d outside [0, n_cells)", (long long)k, (int)class_cell[k]);
    ManyStage stage;
    SKM_TRY(stage.reserve(C, n_cells));
    // what the kernel reads: the handle's own counts in the caller's class order, the class -> cell map,
    // the weights and the cells' totals (declared before the guard: freed after the stream has drained)
    DBuf<double> own, weight_dev, total_dev;
    DBuf<int32_t> cell_dev;
    SKM_TRY(own.ensure(C)); SKM_TRY(cell_dev.ensure(C));
    SKM_TRY(weight_dev.ensure((size_t)(n_cells * n_cells))); SKM_TRY(total_dev.ensure((size_t)n_cells));
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(q->stream); });
    launch_permute_f64(q->cls_count.p, q->perm.p, C, own.p, true, q->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cell_dev.p, class_cell, C * 4, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(weight_dev.p, weight, (size_t)(n_cells * n_cells) * 8, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(total_dev.p, cell_total, (size_t)n_cells * 8, hipMemcpyHostToDevice, q->stream));
    auto blend = [&](int64_t first, int64_t m, double *stage) -> int {
        launch_blend_counts(own.p, cell_dev.p, weight_dev.p, total_dev.p, n_cells, first, m, C, stage, q->stream);
        HIP_TRY(hipGetLastError());
        if (counts_out)
            HIP_TRY(hipMemcpyAsync(counts_out + (size_t)first * C, stage, (size_t)m * C * 8, hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    auto fill = [&](int64_t first, int64_t n, double *rows, double *totals) -> int {
        return many_rows_in(q, stage, first, n, rows, totals, n_cells, blend);
    };
    return em_group_run(q, n_cells, fill, !q->comm, many_slot_cap(), x0, l, rel_tol, x_floor, 0, out, iters_out, tpm != 0);
}

extern "C" int skm_quant_bootstrap(skm_quant *q, int64_t n_boot, uint64_t seed, const double *x0,
                                   const double *l, double rel_tol, double x_floor, int64_t max_iters,
                                   double *out, int64_t *counts_out, int64_t *iters_out)
{
    return bootstrap_impl(q, n_boot, seed, x0, l, rel_tol, x_floor, max_iters, out, counts_out, iters_out, false);
}

extern "C" int skm_quant_bootstrap_tpm(skm_quant *q, int64_t n_boot, uint64_t seed, const double *x0,
                                       const double *l, double rel_tol, double x_floor, int64_t max_iters,
                                       double *out, int64_t *iters_out)
{
    return bootstrap_impl(q, n_boot, seed, x0, l, rel_tol, x_floor, max_iters, out, nullptr, iters_out, true);
}

extern "C" int skm_quant_bootstrap_share_tpm(skm_quant *q, int64_t n_boot, int64_t first, int64_t step, uint64_t seed,
                                             const double *x0, const double *l, double rel_tol, double x_floor,
                                             int64_t max_iters, double *out, int64_t *iters_out)
{
    return bootstrap_impl(q, n_boot, seed, x0, l, rel_tol, x_floor, max_iters, out, nullptr, iters_out, true, first, step);
}

// ---- many class tables over the same transcripts in shared EM launches (skm_em_set.hip) ------------
// The tables of a GROUP are stacked into one block-diagonal problem on a handle of the call's own (class
// views without component tiles: quant_alloc's several_ranks switch), set up once by quant_setup and
// stepped by the segmented kernels until every slot has met its own stopping rule.  A group holds as
// many consecutive tables as keep
//   - slots * T below 2^31 (stacked transcript ids are int32) and the classes and pairs below 2^31,
//   - slots at most SET_QUANT_MAX_SLOTS (gridDim.y) and at most SKM_SET_QUANT_GROUP (tests),
//   - set_quant_bytes(), an estimate of the group's buffers and of the set-up's scratch, within
//     SET_QUANT_GROUP_BYTES (2 GiB); a single table above that still runs, as a group of its own.
// The next group reuses the buffers (they are sized for the largest group before the first runs).
namespace {

constexpr int64_t SET_QUANT_MAX_SLOTS = 32768;
constexpr int64_t SET_QUANT_GROUP_BYTES = 1LL << 31;

int64_t set_quant_bytes(int64_t slots, int64_t n_tx, int64_t n_classes, int64_t n_ids)
{
    return slots * n_tx * 96 + n_classes * 64 + n_ids * 24;
}

int64_t set_quant_slot_cap()
{
    const char *e = getenv("SKM_SET_QUANT_GROUP");                // (looked up at every call)
    const int64_t asked = e ? atoll(e) : 0;
    return asked > 0 ? std::min(asked, SET_QUANT_MAX_SLOTS) : SET_QUANT_MAX_SLOTS;
}

// group g = tables [first[g], first[g + 1]); `first` ends with n_tables
void set_quant_cut(int64_t n_tables, int64_t n_tx, const int64_t *table_classes, const int64_t *table_ids, int64_t max_slots,
                   std::vector<int64_t> *first)
{
    first->assign(1, 0);
    int64_t slots = 0, classes = 0, ids = 0;
    for (int64_t i = 0; i < n_tables; ++i) {
        const bool fits = slots < max_slots && (slots + 1) * n_tx < (1LL << 31) && classes + table_classes[i] < (1LL << 31)
                          && ids + table_ids[i] < (1LL << 31)
                          && set_quant_bytes(slots + 1, n_tx, classes + table_classes[i], ids + table_ids[i]) <= SET_QUANT_GROUP_BYTES;
        if (slots > 0 && !fits) {
            first->push_back(i);
            slots = classes = ids = 0;
        }
        ++slots; classes += table_classes[i]; ids += table_ids[i];
    }
    if (n_tables > 0) first->push_back(n_tables);
}

struct SetQuantRun {
    // (the scratch before the handle: the handle's destructor, which runs first, drains the stream)
    DBuf<EmSetSlot> slots;
    DBuf<unsigned long long> running;
    DBuf<double> out, sums;
    std::unique_ptr<skm_quant> q;
    int64_t n_tx = 0;
};

// room for the largest group of the cut
int set_quant_open(SetQuantRun &run, int device, int64_t n_tx, const std::vector<int64_t> &first, const int64_t *table_classes,
                   const int64_t *table_ids)
{
    int64_t slots = 1, classes = 0, ids = 0;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        int64_t c = 0, m = 0;
        for (int64_t i = first[g]; i < first[g + 1]; ++i) { c += table_classes[i]; m += table_ids[i]; }
        slots = std::max(slots, first[g + 1] - first[g]);
        classes = std::max(classes, c);
        ids = std::max(ids, m);
    }
    if (slots * n_tx >= (1LL << 31)) return fail(SKM_ERR_ARG, "%lld transcripts: stacked ids do not fit 32 bits", (long long)n_tx);
    run.n_tx = n_tx;
    run.q.reset(new skm_quant());
    SKM_TRY(quant_alloc(run.q.get(), device, slots * n_tx, classes, ids, true));
    SKM_TRY(run.slots.ensure((size_t)slots));
    SKM_TRY(run.running.ensure(2));
    SKM_TRY(run.out.ensure((size_t)(slots * n_tx)));
    SKM_TRY(run.sums.ensure((size_t)(slots * ((n_tx + 8191) / 8192 + 2))));
    return SKM_OK;
}

// One group of n tables.  The caller has queued on the handle's stream whatever fills, for the stacked
// problem: cls_offset [C + 1] (from 0), ids [M] (slot s's ids + s T), cls_count [C] -- classes table by
// table in each table's own order --, eff_len and x0 [n][T].  slot_classes / slot_total: classes and sum
// of the class counts of every table.  out [n][T] and iters [n] (host) get what skm_quant_create +
// skm_quant_em give for each table alone; tpm: scaled as quantify() scales (infer.py:127-129).
int set_quant_group(SetQuantRun &run, int64_t n, const int64_t *slot_classes, const double *slot_total, int64_t C, int64_t M,
                    double rel_tol, double x_floor, int64_t max_iters, bool tpm, double *out, int64_t *iters, int64_t first_table)
{
    skm_quant *q = run.q.get();
    const int64_t T = run.n_tx;
    // (on every way out, the failing ones too: copies from the callers' and this function's pageable staging
    // vectors may still be queued, and those vectors go before the handle's destructor drains the stream)
    struct Drain { hipStream_t stream; ~Drain() { (void)hipStreamSynchronize(stream); } } drain{q->stream};
    if (C == 0) {                                                 // (quantify(): no class -> zeros, infer.py:106-107)
        HIP_TRY(hipStreamSynchronize(q->stream));
        if (out) std::fill(out, out + n * T, 0.0);
        for (int64_t i = 0; i < n && iters; ++i) iters[i] = 0;
        return SKM_OK;
    }
    q->n_tx = n * T; q->n_classes = C; q->n_ids = M;
    SKM_TRY(quant_finish_setup(q, nullptr));
    // every transcript has its rows, slot s those of transcripts [s T, (s + 1) T)
    std::vector<int64_t> row_cut((size_t)n + 1);
    HIP_TRY(hipMemcpy2DAsync(row_cut.data(), 8, q->tx_row.p, (size_t)T * 8, 8, (size_t)n + 1, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    std::vector<EmSetSlot> slots((size_t)n);
    int64_t cls = 0, largest_classes = 0, largest_rows = 0;
    for (int64_t i = 0; i < n; ++i) {
        EmSetSlot &d = slots[(size_t)i];
        d.cls_first = cls; d.cls_end = cls += slot_classes[i];
        d.row_first = row_cut[(size_t)i]; d.row_end = row_cut[(size_t)i + 1];
        if (d.row_end - d.row_first < T || d.row_end > q->n_rows)
            return fail(SKM_ERR_STATE, "the stacked class views give table %lld rows [%lld, %lld)", (long long)(first_table + i),
                        (long long)d.row_first, (long long)d.row_end);
        d.n_total = slot_total[i];
        d.done = slot_classes[i] == 0 ? 1 : 0;
        d.iters = 0; d.undefined = 0;
        if (slot_classes[i]) {
            largest_classes = std::max(largest_classes, slot_classes[i]);
            largest_rows = std::max(largest_rows, d.row_end - d.row_first);
        }
    }
    if (cls != C) return fail(SKM_ERR_STATE, "the tables of the group hold %lld classes, not %lld", (long long)cls, (long long)C);
    EmSetProblem p{};
    p.cls_offset = q->cls_offset.p; p.ids = q->ids.p; p.cls_count = q->cls_count.p; p.inner = q->inner.p;
    p.row_start = q->row_start.p; p.row_tx = q->row_tx.p; p.tx_cls = q->tx_cls.p; p.tx_row = q->tx_row.p;
    p.row_sum = q->row_sum.p; p.eff_len = q->eff_len.p; p.x[0] = q->x0.p; p.x[1] = q->x1.p;
    p.rel_tol = rel_tol; p.x_floor = x_floor; p.max_iters = max_iters;
    p.slots = run.slots.p; p.n_slots = (int)n;
    p.n_parts = em_set_parts(largest_rows);
    SKM_TRY(q->part_max.ensure((size_t)(n * p.n_parts)));
    SKM_TRY(q->part_flags.ensure((size_t)(n * p.n_parts)));
    p.part_max = q->part_max.p; p.part_flags = q->part_flags.p;
    p.arrivals = q->arrivals.p;
    HIP_TRY(hipMemcpyAsync(run.slots.p, slots.data(), (size_t)n * sizeof(EmSetSlot), hipMemcpyHostToDevice, q->stream));
    // Steps are queued in chunks with the host one chunk ahead, as em_run does; what the host reads at a
    // chunk's end is the number of slots still running.
    const int64_t chunk = 16;
    int64_t k = 0;
    auto enqueue_chunk = [&](int slot) -> int {
        if (k > (1LL << 24)) return fail(SKM_ERR_STATE, "the EM of the stacked tables does not stop");
        HIP_TRY(hipMemsetAsync(run.running.p + slot, 0, 8, q->stream));
        for (int64_t i = 0; i < chunk; ++i, ++k) launch_em_set_step(p, largest_classes, k, i > 0, q->stream);
        launch_em_set_decide(p, k, run.running.p + slot, q->stream);
        q->launches += 2 * chunk + 1;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q->pinned + 8 * slot, run.running.p + slot, 8, hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    unsigned long long look[8];                           // ([0]: slots still running)
    SKM_TRY(em_run_chunks_ahead(q, look, enqueue_chunk, [](const unsigned long long *w) { return w[0] == 0; }));
    HIP_TRY(hipMemcpyAsync(slots.data(), run.slots.p, (size_t)n * sizeof(EmSetSlot), hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));             // (with it the look-ahead chunk: no-ops)
    for (int64_t i = 0; i < n; ++i) {
        if (slots[(size_t)i].undefined)
            return fail(SKM_ERR_UNDEFINED, "table %lld: no abundance above x_floor: numpy raises on max() of an empty selection",
                        (long long)(first_table + i));
        if (iters) iters[i] = (int64_t)slots[(size_t)i].iters;
        q->iters_total += (double)slots[(size_t)i].iters;
    }
    launch_em_set_result(run.slots.p, (int)n, q->x0.p, q->x1.p, T, run.out.p, q->stream);
    if (tpm) {
        double *const totals = run.sums.p + n * ((T + 8191) / 8192);  // (sum, sum / 1e6) per table
        launch_np_sum_many(run.out.p, T, n, T, 1000000.0, run.sums.p, totals, q->stream);
        launch_divide_many(run.out.p, T, n, T, totals + 1, true, 0.001, q->stream);
        launch_np_sum_many(run.out.p, T, n, T, 1000000.0, run.sums.p, totals, q->stream);
        launch_divide_many(run.out.p, T, n, T, totals + 1, false, 0.0, q->stream);
        for (int64_t i = 0; i < n; ++i)                   // (quantify() does not scale the zeros of a table without classes)
            if (slot_classes[i] == 0) HIP_TRY(hipMemsetAsync(run.out.p + i * T, 0, (size_t)T * 8, q->stream));
    }
    HIP_TRY(hipGetLastError());
    if (out) HIP_TRY(hipMemcpyAsync(out, run.out.p, (size_t)(n * T) * 8, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    return SKM_OK;
}

}  // namespace

extern "C" int skm_set_quant_groups(int64_t n_tables, int64_t n_tx, const int64_t *table_classes, const int64_t *table_ids,
                                    int64_t max_slots, int64_t *n_groups, int64_t *group_first)
{
    if (n_tables < 0 || n_tx <= 0 || max_slots < 1 || !n_groups || (n_tables && (!table_classes || !table_ids || !group_first)))
        return fail(SKM_ERR_ARG, "bad argument");
    for (int64_t i = 0; i < n_tables; ++i)
        if (table_classes[i] < 0 || table_ids[i] < 0) return fail(SKM_ERR_ARG, "negative size of table %lld", (long long)i);
    std::vector<int64_t> first;
    set_quant_cut(n_tables, n_tx, table_classes, table_ids, std::min(max_slots, SET_QUANT_MAX_SLOTS), &first);
    *n_groups = (int64_t)first.size() - 1;
    if (n_tables) std::copy(first.begin(), first.end(), group_first);
    return SKM_OK;
}

extern "C" int skm_quant_em_tables(int device, int64_t n_tx, int64_t n_tables, const int64_t *table_class_offsets,
                                   const int64_t *class_offsets, const int32_t *class_targets, const double *class_counts,
                                   const double *x0, const double *l, double rel_tol, double x_floor, int64_t max_iters,
                                   int tpm, double *out, int64_t *iters)
{
    if (n_tables < 0 || n_tx <= 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_tables == 0) return SKM_OK;                             // (nothing to do, with or without a GPU)
    if (!table_class_offsets || !x0 || !l || !out) return fail(SKM_ERR_ARG, "NULL argument");
    if (table_class_offsets[0] < 0) return fail(SKM_ERR_ARG, "negative class offset");
    for (int64_t s = 0; s < n_tables; ++s)
        if (table_class_offsets[s + 1] < table_class_offsets[s]) return fail(SKM_ERR_ARG, "table offsets are not monotone");
    const int64_t c_lo = table_class_offsets[0], c_hi = table_class_offsets[n_tables];
    if (c_hi > c_lo && (!class_offsets || !class_targets || !class_counts)) return fail(SKM_ERR_ARG, "NULL class arrays");
    for (int64_t c = c_lo; c < c_hi; ++c)
        if (class_offsets[c + 1] < class_offsets[c] || class_offsets[c] < 0) return fail(SKM_ERR_ARG, "class offsets are not monotone");
    if (c_hi > c_lo)
        for (int64_t j = class_offsets[c_lo]; j < class_offsets[c_hi]; ++j)
            if (class_targets[j] < 0 || class_targets[j] >= n_tx)
                return fail(SKM_ERR_ARG, "class target %d outside [0, n_tx)", (int)class_targets[j]);
    std::vector<int64_t> classes((size_t)n_tables), ids((size_t)n_tables), first;
    std::vector<double> total((size_t)n_tables);
    // A class without a tuple entry adds its count to the table's total and nothing else: no transcript's
    // sum reads it (skm_quant_create keeps it, with the key of no transcript).  In the stacked order that key
    // would put it behind the classes of EVERY table, outside its own table's range, so such classes are left
    // out of the stacked problem; the total still counts them.  A table of nothing but such classes has no
    // defined problem and no place here.
    for (int64_t s = 0; s < n_tables; ++s) {
        const int64_t a = table_class_offsets[s], b = table_class_offsets[s + 1];
        int64_t named = 0;
        for (int64_t c = a; c < b; ++c) named += class_offsets[c + 1] > class_offsets[c];
        if (b > a && named == 0) return fail(SKM_ERR_ARG, "table %lld: none of its %lld classes names a transcript", (long long)s, (long long)(b - a));
        classes[(size_t)s] = named;
        ids[(size_t)s] = b > a ? class_offsets[b] - class_offsets[a] : 0;
        total[(size_t)s] = b > a ? np_sum_host(class_counts + a, b - a) : 0.0;     // (as skm_quant_create)
    }
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    SKM_TRY(set_device(device));
    set_quant_cut(n_tables, n_tx, classes.data(), ids.data(), set_quant_slot_cap(), &first);
    std::vector<int64_t> offsets;                                 // (staging, declared before the run: its handle's destructor,
    std::vector<int32_t> stacked;                                 //  which drains the stream, then runs before they go)
    std::vector<double> counts;
    SetQuantRun run;
    SKM_TRY(set_quant_open(run, device, n_tx, first, classes.data(), ids.data()));
    skm_quant *q = run.q.get();
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int64_t t0 = first[g], n = first[g + 1] - t0;
        int64_t C = 0, M = 0;
        for (int64_t s = 0; s < n; ++s) { C += classes[(size_t)(t0 + s)]; M += ids[(size_t)(t0 + s)]; }
        if (C) {
            offsets.resize((size_t)C + 1);
            counts.resize((size_t)C);
            stacked.resize((size_t)M);
            int64_t k = 0, j_out = 0;
            for (int64_t s = 0; s < n; ++s) {
                const int32_t base = (int32_t)(s * n_tx);
                for (int64_t c = table_class_offsets[t0 + s]; c < table_class_offsets[t0 + s + 1]; ++c) {
                    if (class_offsets[c + 1] == class_offsets[c]) continue;
                    offsets[(size_t)k] = j_out;
                    counts[(size_t)k++] = class_counts[c];
                    for (int64_t j = class_offsets[c]; j < class_offsets[c + 1]; ++j) stacked[(size_t)j_out++] = class_targets[j] + base;
                }
            }
            offsets[(size_t)C] = j_out;
            if (k != C || j_out != M) return fail(SKM_ERR_STATE, "stacked %lld classes and %lld ids of %lld and %lld", (long long)k, (long long)j_out, (long long)C, (long long)M);
            HIP_TRY(hipMemcpyAsync(q->cls_offset.p, offsets.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->cls_count.p, counts.data(), (size_t)C * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->ids.p, stacked.data(), (size_t)M * 4, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->x0.p, x0 + t0 * n_tx, (size_t)(n * n_tx) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->eff_len.p, l + t0 * n_tx, (size_t)(n * n_tx) * 8, hipMemcpyHostToDevice, q->stream));
        }
        SKM_TRY(set_quant_group(run, n, classes.data() + t0, total.data() + t0, C, M, rel_tol, x_floor, max_iters, tpm != 0,
                                out + t0 * n_tx, iters ? iters + t0 : nullptr, t0));
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_quantify(skm_sample_set *s, const double *lengths, int64_t n_tx, double rel_tol, double x_floor,
                                       int64_t max_iters, int64_t cap_samples, int64_t *n_samples, double *tpm,
                                       double *effective_lengths, int64_t *iters)
{
    if (!s || !lengths || !n_samples || n_tx <= 0 || cap_samples < 0 || (cap_samples && !tpm))
        return fail(SKM_ERR_ARG, "bad argument");
    {
        std::lock_guard<std::mutex> counting(s->mu);              // (before any device work)
        *n_samples = (int64_t)s->sample_units.size();
    }
    if (cap_samples < *n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)*n_samples);
    if (*n_samples == 0) return SKM_OK;
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    const int64_t S = (int64_t)v.units.size();
    *n_samples = S;
    if (cap_samples < S) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)S);
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // a tuple's ids index the stacked abundance vectors: none may lie outside the caller's transcripts
    for (size_t k = 0; k < v.order.size(); ++k) {
        const int64_t c = v.order[k];
        if (v.len[c] <= 0) return fail(SKM_ERR_STATE, "class %lld of the set has no tuple", (long long)c);   // (it would leave its sample's range)
        for (int64_t j = 0; j < v.len[c]; ++j)
            if (v.arena[(size_t)(v.start[c] + j)] < 0 || v.arena[(size_t)(v.start[c] + j)] >= n_tx)
                return fail(SKM_ERR_ARG, "the set's classes name transcript %d: not below n_tx = %lld", (int)v.arena[(size_t)(v.start[c] + j)],
                            (long long)n_tx);
    }
    std::vector<int64_t> classes((size_t)S), ids((size_t)S), first;
    std::vector<double> total((size_t)S);
    for (int64_t i = 0; i < S; ++i) {
        classes[(size_t)i] = v.sample_class_offsets[(size_t)i + 1] - v.sample_class_offsets[(size_t)i];
        ids[(size_t)i] = v.sample_rows[(size_t)i];
        total[(size_t)i] = (double)v.sample_aligned[(size_t)i];   // n = its aligned units
    }
    set_quant_cut(S, n_tx, classes.data(), ids.data(), set_quant_slot_cap(), &first);
    // the class tuples stay where the mapper left them: a group's are gathered from the table's arena into
    // the stacked problem on the device, by the classes' places there -- a few words per class from the host
    DBuf<double> lengths_dev;
    DBuf<unsigned long long> hist;
    DBuf<int64_t> src, dst;
    DBuf<int32_t> add;
    std::vector<int64_t> h_src, h_dst;                            // (staging, before the run: see skm_quant_em_tables)
    std::vector<int32_t> h_add;
    std::vector<double> h_count;
    SetQuantRun run;
    SKM_TRY(set_quant_open(run, m->ix->device, n_tx, first, classes.data(), ids.data()));
    skm_quant *q = run.q.get();
    int64_t slots_max = 1, classes_max = 1;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        slots_max = std::max(slots_max, first[g + 1] - first[g]);
        classes_max = std::max(classes_max, v.sample_class_offsets[(size_t)first[g + 1]] - v.sample_class_offsets[(size_t)first[g]]);
    }
    SKM_TRY(lengths_dev.ensure((size_t)n_tx));
    SKM_TRY(src.ensure((size_t)classes_max)); SKM_TRY(dst.ensure((size_t)classes_max + 1)); SKM_TRY(add.ensure((size_t)classes_max));
    if (s->keep_hist) SKM_TRY(hist.ensure((size_t)slots_max * MAX_FRAGMENT_LENGTH));
    HIP_TRY(hipStreamSynchronize(m->stream));                     // (the table, the arena and the histograms are final)
    HIP_TRY(hipMemcpyAsync(lengths_dev.p, lengths, (size_t)n_tx * 8, hipMemcpyHostToDevice, q->stream));
    const int64_t hist_rows = (int64_t)(s->hist.cap / MAX_FRAGMENT_LENGTH);     // (a sample past them has an empty histogram)
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int64_t t0 = first[g], n = first[g + 1] - t0;
        const int64_t k0 = v.sample_class_offsets[(size_t)t0], C = v.sample_class_offsets[(size_t)(t0 + n)] - k0;
        h_src.resize((size_t)C); h_dst.resize((size_t)C + 1); h_add.resize((size_t)C); h_count.resize((size_t)C);
        int64_t M = 0;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = v.sample_class_offsets[(size_t)(t0 + i)]; k < v.sample_class_offsets[(size_t)(t0 + i) + 1]; ++k) {
                const int64_t c = v.order[(size_t)k];
                h_src[(size_t)(k - k0)] = v.start[(size_t)c];
                h_dst[(size_t)(k - k0)] = M;
                h_add[(size_t)(k - k0)] = (int32_t)(i * n_tx);
                h_count[(size_t)(k - k0)] = (double)v.count[(size_t)c];
                M += v.len[(size_t)c];
            }
        h_dst[(size_t)C] = M;
        if (m->use_length_weights) {              // a fragment-length model: one row for every sample
            launch_effective_lengths_weights(m->length_weights.p, 1, lengths_dev.p, n_tx, q->eff_len.p, q->stream);
            launch_repeat_row(q->eff_len.p, n_tx, n, q->stream);
        } else if (s->keep_hist) {
            const int64_t have = std::max<int64_t>(0, std::min(n, hist_rows - t0));
            HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)n * MAX_FRAGMENT_LENGTH * 8, q->stream));
            if (have) HIP_TRY(hipMemcpyAsync(hist.p, s->hist.p + t0 * MAX_FRAGMENT_LENGTH, (size_t)have * MAX_FRAGMENT_LENGTH * 8,
                                             hipMemcpyDeviceToDevice, q->stream));
            launch_effective_lengths_many(hist.p, n, lengths_dev.p, n_tx, q->eff_len.p, q->stream);
        } else {
            launch_effective_lengths(m->counters.p + CTR_FLD, lengths_dev.p, n_tx, q->eff_len.p, q->stream);
            launch_repeat_row(q->eff_len.p, n_tx, n, q->stream);
        }
        if (effective_lengths)
            HIP_TRY(hipMemcpyAsync(effective_lengths + t0 * n_tx, q->eff_len.p, (size_t)(n * n_tx) * 8, hipMemcpyDeviceToHost, q->stream));
        if (C) {
            // the start vector of skm_quant_infer, per sample: reciprocal, numpy's sum, divide
            double *const totals = run.sums.p + n * ((n_tx + 8191) / 8192);
            launch_reciprocal(q->eff_len.p, n * n_tx, q->x0.p, q->stream);
            launch_np_sum_many(q->x0.p, n_tx, n, n_tx, 1.0, run.sums.p, totals, q->stream);
            launch_divide_many(q->x0.p, n_tx, n, n_tx, totals, false, 0.0, q->stream);
            HIP_TRY(hipMemcpyAsync(src.p, h_src.data(), (size_t)C * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(dst.p, h_dst.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(add.p, h_add.data(), (size_t)C * 4, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->cls_offset.p, h_dst.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->cls_count.p, h_count.data(), (size_t)C * 8, hipMemcpyHostToDevice, q->stream));
            launch_stack_tuples(src.p, dst.p, add.p, C, m->arena.p, q->ids.p, q->stream);
            HIP_TRY(hipGetLastError());
        }
        SKM_TRY(set_quant_group(run, n, classes.data() + t0, total.data() + t0, C, M, rel_tol, x_floor, max_iters, true,
                                tpm + t0 * n_tx, iters ? iters + t0 : nullptr, t0));
    }
    return SKM_OK;
}

extern "C" int skm_quant_timing(skm_quant *q, double timing[4])
{
    if (!q || !timing) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    timing[0] = q->t_em_ns; timing[1] = q->iters_total; timing[2] = q->launches; timing[3] = 0;
    return SKM_OK;
}

// ---------------------------------------------------------------- multi-GPU
extern "C" int skm_comm_unique_id(void *id128)
{
    if (!id128) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(load_rccl());
    NCCL_TRY(g_rccl.GetUniqueId(id128));
    return SKM_OK;
}

extern "C" int skm_comm_create(int device, const void *id128, int rank, int world, skm_comm **out)
{
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return fail(SKM_ERR_ARG, "bad argument");
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    SKM_TRY(set_device(device));
    SKM_TRY(load_rccl());
    UniqueId id;
    memcpy(&id, id128, sizeof(id));
    skm_comm *c = new skm_comm();
    c->device = device;
    c->rank = rank;
    c->world = world;
    int r = g_comm_init(&c->comm, world, id, rank);
    if (r != 0) {
        delete c;
        return fail(SKM_ERR_COMM, "ncclCommInitRank failed: %s",
                    g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    }
    *out = c;
    return SKM_OK;
}

extern "C" int skm_comm_count(skm_comm *c, int *count)
{
    if (!c || !count) return fail(SKM_ERR_ARG, "NULL argument");
    if (!g_rccl.CommCount) return fail(SKM_ERR_COMM, "librccl.so lacks ncclCommCount");
    NCCL_TRY(g_rccl.CommCount(c->comm, count));
    return SKM_OK;
}

// SURVEY 8(e).1 over xGMI: a mapper's table goes from GPU to GPU as it lies in HBM
// (skm_mapper_device_table's arrays, ncclSend / ncclRecv) and is merged by key on the receiving GPU
// (class_merge_kernel over the received arrays): no host copy, no host sort.  One call does both
// directions so that a rank may pair a send with a receive (two ranks swapping, or -- the one-GPU
// test -- a rank sending to itself): first the sizes (a header of eight words), then the arrays.
extern "C" int skm_mapper_exchange_tables(skm_mapper *send, int send_to, skm_mapper *recv, int recv_from, skm_comm *comm)
{
    if (!comm || (!send && !recv)) return fail(SKM_ERR_ARG, "NULL argument");
    if ((send && send_to < 0) || (recv && recv_from < 0) || send_to >= comm->world || recv_from >= comm->world)
        return fail(SKM_ERR_ARG, "peer rank outside the communicator");
    if ((send && send->ix->device != comm->device) || (recv && recv->ix->device != comm->device))
        return fail(SKM_ERR_ARG, "communicator and mapper live on different GPUs");
    SKM_TRY(load_rccl());
    if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
        return fail(SKM_ERR_COMM, "librccl.so lacks ncclSend / ncclRecv");
    SKM_TRY(set_device(comm->device));
    skm_device_table out{};
    if (send) SKM_TRY(skm_mapper_device_table(send, &out));            // (waits for what the mapper has queued)
    PoolStream stream;
    HIP_TRY(pool_stream_acquire(stream.out()));
    DBuf<unsigned long long> header, fld, first_seen;
    DBuf<int64_t> start, len;
    DBuf<double> count;
    DBuf<int32_t> ids;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (every exit: before they go)
    SKM_TRY(header.ensure(16));
    unsigned long long words[16] = {(unsigned long long)out.n_classes, (unsigned long long)out.n_ids,
                                    (unsigned long long)out.unaligned, (unsigned long long)out.units,
                                    (unsigned long long)out.first_seen_bound, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(header.p, words, 8 * 8, hipMemcpyHostToDevice, stream));
    // (a group that has been started is always ended, whatever a call inside it returned)
    auto grouped = [&](const std::function<int()> &calls) -> int {
        NCCL_TRY(g_rccl.GroupStart());
        const int rc = calls();
        const int end = g_rccl.GroupEnd();
        if (rc != SKM_OK) return rc;
        NCCL_TRY(end);
        return SKM_OK;
    };
    SKM_TRY(grouped([&]() -> int {
        if (send) NCCL_TRY(g_rccl.Send(header.p, 8, NCCL_UINT64, send_to, comm->comm, stream));
        if (recv) NCCL_TRY(g_rccl.Recv(header.p + 8, 8, NCCL_UINT64, recv_from, comm->comm, stream));
        return SKM_OK;
    }));
    HIP_TRY(hipMemcpyAsync(words + 8, header.p + 8, 8 * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    skm_device_table in{};
    in.device = comm->device;
    if (recv) {
        in.n_classes = (int64_t)words[8]; in.n_ids = (int64_t)words[9];
        in.unaligned = (int64_t)words[10]; in.units = (int64_t)words[11]; in.first_seen_bound = (int64_t)words[12];
        if (in.n_classes < 0 || in.n_ids < 0 || in.n_classes >= (1LL << 40) || in.n_ids >= (1LL << 40))
            return fail(SKM_ERR_COMM, "received a table header that makes no sense");
        SKM_TRY(start.ensure(std::max<int64_t>(in.n_classes, 1))); SKM_TRY(len.ensure(std::max<int64_t>(in.n_classes, 1)));
        SKM_TRY(count.ensure(std::max<int64_t>(in.n_classes, 1))); SKM_TRY(first_seen.ensure(std::max<int64_t>(in.n_classes, 1)));
        SKM_TRY(ids.ensure(std::max<int64_t>(in.n_ids, 1))); SKM_TRY(fld.ensure(MAX_FRAGMENT_LENGTH));
    }
    SKM_TRY(grouped([&]() -> int {
    if (send) {
        if (out.n_classes) {
            NCCL_TRY(g_rccl.Send(out.class_start, (size_t)out.n_classes, NCCL_UINT64, send_to, comm->comm, stream));
            NCCL_TRY(g_rccl.Send(out.class_len, (size_t)out.n_classes, NCCL_UINT64, send_to, comm->comm, stream));
            NCCL_TRY(g_rccl.Send(out.class_count, (size_t)out.n_classes, NCCL_FLOAT64, send_to, comm->comm, stream));
            NCCL_TRY(g_rccl.Send(out.first_seen, (size_t)out.n_classes, NCCL_UINT64, send_to, comm->comm, stream));
        }
        if (out.n_ids) NCCL_TRY(g_rccl.Send(out.ids, (size_t)out.n_ids, NCCL_INT32, send_to, comm->comm, stream));
        NCCL_TRY(g_rccl.Send(out.fld, MAX_FRAGMENT_LENGTH, NCCL_UINT64, send_to, comm->comm, stream));
    }
    if (recv) {
        if (in.n_classes) {
            NCCL_TRY(g_rccl.Recv(start.p, (size_t)in.n_classes, NCCL_UINT64, recv_from, comm->comm, stream));
            NCCL_TRY(g_rccl.Recv(len.p, (size_t)in.n_classes, NCCL_UINT64, recv_from, comm->comm, stream));
            NCCL_TRY(g_rccl.Recv(count.p, (size_t)in.n_classes, NCCL_FLOAT64, recv_from, comm->comm, stream));
            NCCL_TRY(g_rccl.Recv(first_seen.p, (size_t)in.n_classes, NCCL_UINT64, recv_from, comm->comm, stream));
        }
        if (in.n_ids) NCCL_TRY(g_rccl.Recv(ids.p, (size_t)in.n_ids, NCCL_INT32, recv_from, comm->comm, stream));
        NCCL_TRY(g_rccl.Recv(fld.p, MAX_FRAGMENT_LENGTH, NCCL_UINT64, recv_from, comm->comm, stream));
    }
    return SKM_OK;
    }));
    HIP_TRY(hipStreamSynchronize(stream));
    if (!recv) return SKM_OK;
    in.class_start = start.p; in.class_len = len.p; in.class_count = count.p;
    in.first_seen = (const uint64_t *)first_seen.p; in.ids = ids.p; in.fld = (const uint64_t *)fld.p;
    return skm_mapper_merge_device(recv, &in);
}

extern "C" int skm_comm_destroy(skm_comm *c)
{
    if (!c) return SKM_OK;
    (void)hipSetDevice(c->device);
    if (c->comm && g_rccl.CommDestroy) NCCL_TRY(g_rccl.CommDestroy(c->comm));
    delete c;
    return SKM_OK;
}

extern "C" int skm_quant_set_comm(skm_quant *q, skm_comm *c)
{
    if (!q) return fail(SKM_ERR_ARG, "NULL quant");
    std::lock_guard<std::mutex> lock(q->mu);
    if (c && c->device != q->device) return fail(SKM_ERR_ARG, "communicator and quant live on different GPUs");
    q->comm = c ? c->comm : nullptr;
    q->rank = c ? c->rank : 0;
    q->world = c ? c->world : 1;
    return SKM_OK;
}
