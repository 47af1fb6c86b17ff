// C ABI of libseekmer_hip.so: the index handle -- create, info, layout, junctions, probe -- and, on its
// transcript pool, the sequence-bias correction.  Nothing of the mapper.
#include "skm_abi_mapper.h"
#include "skm_bias.h"
#include "skm_bias_weights.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
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
