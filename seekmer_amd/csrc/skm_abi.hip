// C ABI of libseekmer_hip.so (declared in include/seekmer_hip.h): handle
// management, HBM buffers, stream/event plumbing and the launch sequences
// of the index, the mapper, the sample sets and the gene-level tables.
// No torch types, no exceptions across the boundary.
#include "skm_abi_samples.h"
#include "skm_bias.h"
#include "skm_bias_weights.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    SKM_TRY(check_device(device));
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

}  // namespace

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

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

}  // namespace abi
}  // namespace skm

namespace {

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

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// the weights of a fragment-length model: every one finite and >= 0 (checked on the host, before any device work)
bool length_weights_valid(const double *p, int64_t count)
{
    for (int64_t i = 0; i < count; ++i)
        if (!(p[i] >= 0.0) || std::isinf(p[i])) return false;
    return true;
}

}  // namespace abi
}  // namespace skm

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

}  // namespace

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

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

}  // namespace abi
}  // namespace skm

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
    SKM_TRY(check_device(device));
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
    SKM_TRY(check_device(device));
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
