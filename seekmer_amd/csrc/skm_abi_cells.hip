// C ABI of libseekmer_hip.so: cell barcodes, UMI windows and cell discovery.
#include "skm_abi.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

using namespace skm;
using namespace skm::abi;

// ------------------------------------------------------------ cell barcodes (skm_barcodes.hip)
// The whitelist's table is built here, on the host, once per handle, and uploaded; the scratch of the assign calls
// lives in the handle and grows with the largest piece.  All work is on the default stream with blocking copies.
// What the window kernels (barcode_assign_kernel, umi_window_kernel, census_count_kernel) read of a host piece: only
// the one or two code words of every read that hold bases [start, start + length), the lengths unless uniform, and
// the dense clean word that barcode_clean_kernel scatters from the exception list.
struct WindowScratch {
    DBuf<uint64_t> codes;
    DBuf<uint32_t> lengths, clean, exception_reads, exception_masks;
};

namespace {

// a piece of packed reads as the window kernels take it (n_reads > 0 pieces are looked at in full)
int window_piece_check(const skm_packed_reads *reads)
{
    const int64_t n = reads->n_reads, n_exc = reads->n_exceptions;
    if (n < 0 || n >= (1LL << 31) || n_exc < 0 || n_exc > n) return fail(SKM_ERR_ARG, "a piece of %lld reads", (long long)n);
    if (n == 0) return SKM_OK;
    const int64_t code_words = reads->code_words;
    if (code_words < 0 || reads->read_stride < code_words || (code_words && !reads->codes) ||
        (!reads->lengths && reads->uniform_len < 0) || (n_exc && (!reads->exception_reads || !reads->exception_masks)))
        return fail(SKM_ERR_ARG, "not a piece of packed reads");
    for (int64_t e = 0; e < n_exc; ++e)
        if (reads->exception_reads[e] >= (uint64_t)n) return fail(SKM_ERR_ARG, "exception %lld names read %u of %lld", (long long)e, reads->exception_reads[e], (long long)n);
    return SKM_OK;
}

// the windows of a checked piece of n_reads > 0 reads go up (default stream; the copies block, the clean kernel is
// queued): *w is what the kernels take.  The caller drains the stream before the scratch goes.
int window_piece_upload(WindowScratch &s, const skm_packed_reads *reads, int start, int length, BarcodeWindows *w)
{
    const int64_t n = reads->n_reads, n_exc = reads->n_exceptions, code_words = reads->code_words;
    // the one or two words of every read that hold the window, as far as the piece has them
    const int64_t first_word = start / 32;
    const int offset = start % 32;
    const int words = (int)std::max<int64_t>(0, std::min<int64_t>(code_words - first_word, offset + length > 32 ? 2 : 1));
    SKM_TRY(s.codes.ensure((size_t)std::max<int64_t>(n * words, 1))); SKM_TRY(s.clean.ensure(n));
    if (words && reads->read_stride == words) {
        HIP_TRY(hipMemcpy(s.codes.p, reads->codes, (size_t)(n * words) * 8, hipMemcpyHostToDevice));
    } else if (words) {
        std::vector<uint64_t> window((size_t)(n * words));
        for (int64_t r = 0; r < n; ++r)
            for (int k = 0; k < words; ++k) window[r * words + k] = reads->codes[r * reads->read_stride + first_word + k];
        HIP_TRY(hipMemcpy(s.codes.p, window.data(), window.size() * 8, hipMemcpyHostToDevice));
    }
    if (reads->lengths) {
        SKM_TRY(s.lengths.ensure(n));
        HIP_TRY(hipMemcpy(s.lengths.p, reads->lengths, n * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemsetAsync(s.clean.p, 0xff, n * 4, nullptr));
    if (n_exc && words) {
        SKM_TRY(s.exception_reads.ensure(n_exc)); SKM_TRY(s.exception_masks.ensure(n_exc * words));
        HIP_TRY(hipMemcpy(s.exception_reads.p, reads->exception_reads, n_exc * 4, hipMemcpyHostToDevice));
        std::vector<uint32_t> planes((size_t)(n_exc * words));
        for (int64_t e = 0; e < n_exc; ++e)
            for (int k = 0; k < words; ++k) planes[e * words + k] = reads->exception_masks[e * code_words + first_word + k];
        HIP_TRY(hipMemcpy(s.exception_masks.p, planes.data(), planes.size() * 4, hipMemcpyHostToDevice));
        launch_barcode_clean(s.exception_reads.p, s.exception_masks.p, n_exc, words, offset, s.clean.p, nullptr);
        HIP_TRY(hipGetLastError());
    }
    *w = BarcodeWindows{n, s.codes.p, words, offset, reads->lengths ? s.lengths.p : nullptr, reads->uniform_len, start, s.clean.p};
    return SKM_OK;
}

}  // namespace

struct skm_barcodes {
    ~skm_barcodes() { (void)hipSetDevice(device); }  // (then the members free the device memory)
    int device = 0;
    int length = 0;
    int64_t n = 0;
    uint32_t slot_bits = 1;
    std::mutex mu;                                   // one assign call at a time: they share the scratch
    DBuf<uint64_t> keys;
    DBuf<int32_t> cells, cell;
    WindowScratch windows;
    DBuf<unsigned long long> units;                  // [n] + the five counters
};

extern "C" int skm_barcodes_create(int device, const char *barcodes, int64_t n, int length, skm_barcodes **out)
{
    SKM_TRY(check_device(device));
    if (!out || !barcodes) return fail(SKM_ERR_ARG, "bad argument");
    if (length < 1 || length > 32) return fail(SKM_ERR_ARG, "barcodes of %d bases: 1 to 32 are possible", length);
    if (n < 1 || n > (1LL << 28)) return fail(SKM_ERR_ARG, "a whitelist of %lld barcodes", (long long)n);
    uint32_t slot_bits = 1;
    while ((1LL << slot_bits) < 2 * n) ++slot_bits;
    const uint32_t mask = (uint32_t)((1ULL << slot_bits) - 1);
    std::vector<uint64_t> keys((size_t)mask + 1, 0);
    std::vector<int32_t> cells((size_t)mask + 1, -1);
    for (int64_t i = 0; i < n; ++i) {
        uint64_t key = 0;
        for (int j = 0; j < length; ++j) {
            const char c = barcodes[i * length + j];
            const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
            if (code < 0) return fail(SKM_ERR_ARG, "barcode %lld holds a character other than A, C, G, T", (long long)i);
            key = key << 2 | (uint64_t)code;
        }
        uint32_t s = barcode_slot(key, slot_bits);
        while (cells[s] >= 0) {
            if (keys[s] == key) return fail(SKM_ERR_ARG, "barcodes %d and %lld are the same", cells[s], (long long)i);
            s = (s + 1) & mask;
        }
        keys[s] = key;
        cells[s] = (int32_t)i;
    }
    SKM_TRY(set_device(device));
    auto b = std::make_unique<skm_barcodes>();
    b->device = device; b->length = length; b->n = n; b->slot_bits = slot_bits;
    SKM_TRY(b->keys.ensure(keys.size())); SKM_TRY(b->cells.ensure(cells.size()));
    HIP_TRY(hipMemcpy(b->keys.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->cells.p, cells.data(), cells.size() * 4, hipMemcpyHostToDevice));
    *out = b.release();
    return SKM_OK;
}

extern "C" int skm_barcodes_destroy(skm_barcodes *barcodes)
{
    delete barcodes;
    return SKM_OK;
}

extern "C" int skm_barcodes_assign(skm_barcodes *b, const skm_packed_reads *reads, int start, int max_mismatches,
                                   int32_t *cell, int64_t *cell_units, int64_t stats[5])
{
    if (!b || !reads || !cell_units || !stats) return fail(SKM_ERR_ARG, "bad argument");
    if (start < 0 || start > (1 << 24)) return fail(SKM_ERR_ARG, "a barcode that starts at base %d", start);
    if (max_mismatches != 0 && max_mismatches != 1) return fail(SKM_ERR_ARG, "%d mismatches: 0 or 1", max_mismatches);
    SKM_TRY(window_piece_check(reads));
    const int64_t n = reads->n_reads;
    if (n == 0) return SKM_OK;
    if (!cell) return fail(SKM_ERR_ARG, "not a piece of packed reads");
    std::lock_guard<std::mutex> hold(b->mu);
    SKM_TRY(set_device(b->device));
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: the scratch is in use)
    SKM_TRY(b->cell.ensure(n));
    SKM_TRY(b->units.ensure(b->n + BARCODE_STATS));
    BarcodeWindows w{};
    SKM_TRY(window_piece_upload(b->windows, reads, start, b->length, &w));
    HIP_TRY(hipMemsetAsync(b->units.p, 0, (b->n + BARCODE_STATS) * 8, nullptr));
    BarcodeTable table{b->keys.p, b->cells.p, b->slot_bits, b->length, b->n};
    launch_barcode_assign(table, w, max_mismatches, b->cell.p, b->units.p, b->units.p + b->n, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> counted((size_t)b->n + BARCODE_STATS);
    HIP_TRY(hipMemcpy(cell, b->cell.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counted.data(), b->units.p, counted.size() * 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copies home have waited for the kernels)
    for (int64_t c = 0; c < b->n; ++c) cell_units[c] += (int64_t)counted[c];
    for (int k = 0; k < BARCODE_STATS; ++k) stats[k] += (int64_t)counted[b->n + k];
    return SKM_OK;
}

// The scratch lives for the call; all work is on the default stream with blocking copies, as skm_barcodes_assign.
extern "C" int skm_umi_windows(int device, const skm_packed_reads *reads, int start, int length, int32_t *cell, uint32_t *umi,
                               int64_t *n_unreadable)
{
    SKM_TRY(check_device(device));
    if (!reads || !n_unreadable) return fail(SKM_ERR_ARG, "bad argument");
    if (start < 0 || start > (1 << 24)) return fail(SKM_ERR_ARG, "a UMI that starts at base %d", start);
    if (length < 1 || length > 16) return fail(SKM_ERR_ARG, "UMIs of %d bases: 1 to 16 are possible", length);
    SKM_TRY(window_piece_check(reads));
    const int64_t n = reads->n_reads;
    if (n == 0) return SKM_OK;
    if (!umi) return fail(SKM_ERR_ARG, "not a piece of packed reads");
    SKM_TRY(set_device(device));
    WindowScratch windows; DBuf<uint32_t> d_umi; DBuf<int32_t> d_cell;
    DBuf<unsigned long long> d_count;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_umi.ensure(n));
    SKM_TRY(d_count.ensure(1));
    if (cell) {
        SKM_TRY(d_cell.ensure(n));
        HIP_TRY(hipMemcpy(d_cell.p, cell, n * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemsetAsync(d_count.p, 0, 8, nullptr));
    BarcodeWindows w{};
    SKM_TRY(window_piece_upload(windows, reads, start, length, &w));
    launch_umi_windows(w, length, cell ? d_cell.p : nullptr, d_umi.p, d_count.p, nullptr);
    HIP_TRY(hipGetLastError());
    unsigned long long counted = 0;
    HIP_TRY(hipMemcpy(umi, d_umi.p, n * 4, hipMemcpyDeviceToHost));
    if (cell) HIP_TRY(hipMemcpy(cell, d_cell.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&counted, d_count.p, 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copies home have waited for the kernels)
    *n_unreadable += (int64_t)counted;
    return SKM_OK;
}

extern "C" int skm_units_group(int device, const int32_t *sample, int64_t n, int64_t n_samples, int32_t *order,
                               int64_t *offsets)
{
    SKM_TRY(check_device(device));
    if (n < 0 || n >= (1LL << 31) || n_samples < 1 || n_samples > (1LL << 24) || !offsets || (n && (!sample || !order)))
        return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    DBuf<int32_t> d_sample, d_iota, d_order; DBuf<uint32_t> d_keys, d_sorted; DBuf<int64_t> d_offsets; DBuf<int> d_error;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    SKM_TRY(d_sample.ensure(room)); SKM_TRY(d_iota.ensure(room)); SKM_TRY(d_order.ensure(room)); SKM_TRY(d_keys.ensure(room));
    SKM_TRY(d_sorted.ensure(room)); SKM_TRY(d_offsets.ensure(n_samples + 1)); SKM_TRY(d_error.ensure(1));
    HIP_TRY(hipMemsetAsync(d_error.p, 0, sizeof(int), nullptr));
    if (n) HIP_TRY(hipMemcpy(d_sample.p, sample, n * 4, hipMemcpyHostToDevice));
    launch_group_keys(d_sample.p, n, n_samples, d_keys.p, d_iota.p, d_error.p, nullptr);
    HIP_TRY(hipGetLastError());
    int end_bit = 1;
    while ((1LL << end_bit) <= n_samples) ++end_bit;      // (the keys go up to n_samples itself: the dropped units)
    if (sort_pairs_u32(d_keys.p, d_sorted.p, d_iota.p, d_order.p, n, end_bit, nullptr) != 0)
        return fail(SKM_ERR_HIP, "grouping %lld units: %s", (long long)n, quant_setup_failure());
    launch_group_offsets(d_sorted.p, n, n_samples, d_offsets.p, nullptr);
    HIP_TRY(hipGetLastError());
    int error = 0;
    HIP_TRY(hipMemcpy(&error, d_error.p, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(offsets, d_offsets.p, (n_samples + 1) * 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copies home have waited for the kernels)
    if (error) return fail(SKM_ERR_ARG, "a unit names a sample not below n_samples = %lld", (long long)n_samples);
    if (offsets[n_samples]) HIP_TRY(hipMemcpy(order, d_order.p, offsets[n_samples] * 4, hipMemcpyDeviceToHost));
    return SKM_OK;
}

// ------------------------------------------------------------ cell discovery (skm_census.hip)
// The census table lives in the handle and is sized ahead of every add to at least twice (distinct keys so far + the
// piece's reads); SKM_TEST_CENSUS_SLOTS starts it at that many slots instead, and it then grows only when a launch
// finds it full (the deferred pairs are replayed after the rehash).  The ranking is made by the first call that
// needs it after the last add and kept on the device.  All work is on the default stream with blocking copies.
struct skm_barcode_census {
    ~skm_barcode_census() { (void)hipSetDevice(device); }  // (then the members free the device memory)
    int device = 0;
    int length = 0;
    std::mutex mu;                                   // calls on one handle run one after the other
    uint32_t slot_bits = 0;
    bool test_slots = false;
    int64_t entries = 0, sentinel = 0, counted = 0;  // occupied slots, all-T 32-mers seen, clean windows counted
    bool failed = false;                             // no memory for the table, or a launch that lost units
    std::string failed_msg;
    DBuf<CensusSlot> slots;
    DBuf<unsigned long long> ctl, deferred;
    WindowScratch windows;                           // the windows of the piece at hand
    bool ranked = false;                             // ranked_keys / ranked_counts hold the census in ranked order
    int64_t n_ranked = 0;
    DBuf<unsigned long long> keys, counts, ranked_keys, ranked_counts, picked_keys, picked_counts;
    DBuf<int32_t> perm, perm_sorted;
    DBuf<uint32_t> word, word_sorted;
    CensusTable table(unsigned long long *list = nullptr, int64_t list_cap = 0) const
    {
        return CensusTable{slots.p, slot_bits, length, ctl.p, list, list_cap};
    }
};

namespace {

int census_fail(skm_barcode_census *c, int code, const std::string &msg)
{
    c->failed = true;
    c->failed_msg = msg;
    return fail(code, "%s", msg.c_str());
}

// the census in 1 << bits slots: a fresh table, or the entries of the old one rehashed (c->mu is held)
int census_grow(skm_barcode_census *c, uint32_t bits)
{
    char text[320];
    if (bits > 31) {
        snprintf(text, sizeof(text), "a census table of 2^%u slots (%lld distinct barcodes so far)", bits, (long long)c->entries);
        return census_fail(c, SKM_ERR_STATE, text);
    }
    DBuf<CensusSlot> fresh;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });
    if (fresh.ensure((size_t)1 << bits) != SKM_OK) {
        const std::string why = last_message();
        snprintf(text, sizeof(text), "cell discovery: no device memory for a census table of %llu slots, %llu MB (32 bytes a "
                 "distinct barcode at load 1/2; %lld distinct keys so far): ", 1ULL << bits,
                 (unsigned long long)(((1ULL << bits) * sizeof(CensusSlot)) >> 20), (long long)c->entries);
        return census_fail(c, SKM_ERR_HIP, text + why);
    }
    const CensusTable to{fresh.p, bits, c->length, c->ctl.p, nullptr, 0};
    if (c->slot_bits) {
        HIP_TRY(hipMemsetAsync(c->ctl.p + CENSUS_CTL_DEFERRED, 0, 8, nullptr));
        launch_census_rehash(c->table(), to, nullptr);
    } else {
        launch_census_init(to, nullptr);
    }
    HIP_TRY(hipGetLastError());
    unsigned long long lost = 0;                     // (the copy home waits for the kernels: the old slots can go)
    HIP_TRY(hipMemcpy(&lost, c->ctl.p + CENSUS_CTL_DEFERRED, 8, hipMemcpyDeviceToHost));
    drain.dismiss();
    if (c->slot_bits && lost) {
        snprintf(text, sizeof(text), "%llu barcodes found no slot in a census table of 2^%u slots", lost, bits);
        return census_fail(c, SKM_ERR_STATE, text);
    }
    c->slots = std::move(fresh);
    c->slot_bits = bits;
    return SKM_OK;
}

// the census in ranked order on the device: count descending, then key ascending (c->mu is held)
int census_rank(skm_barcode_census *c)
{
    if (c->ranked) return SKM_OK;
    const int64_t D = c->entries + (c->sentinel ? 1 : 0);
    if (D >= (1LL << 31)) return fail(SKM_ERR_STATE, "%lld distinct barcodes: fewer than 2^31 can be ranked", (long long)D);
    c->n_ranked = D;
    if (D == 0) { c->ranked = true; return SKM_OK; }
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });
    const size_t room = (size_t)c->entries + 1;
    SKM_TRY(c->keys.ensure(room)); SKM_TRY(c->counts.ensure(room)); SKM_TRY(c->ranked_keys.ensure(room));
    SKM_TRY(c->ranked_counts.ensure(room)); SKM_TRY(c->perm.ensure(room)); SKM_TRY(c->perm_sorted.ensure(room));
    SKM_TRY(c->word.ensure(room)); SKM_TRY(c->word_sorted.ensure(room));
    HIP_TRY(hipMemsetAsync(c->ctl.p + CENSUS_CTL_OUT, 0, 2 * 8, nullptr));
    launch_census_compact(c->table(), c->keys.p, c->counts.p, c->perm.p, nullptr);
    HIP_TRY(hipGetLastError());
    unsigned long long found = 0;
    HIP_TRY(hipMemcpy(&found, c->ctl.p + CENSUS_CTL_OUT, 8, hipMemcpyDeviceToHost));
    if ((int64_t)found != D) return fail(SKM_ERR_STATE, "the census table holds %llu barcodes, its counter says %lld", found, (long long)D);
    // stable passes from the last criterion to the first: key low and high words, then the complemented count words
    int count_bits = 1;
    while (count_bits < 63 && (1LL << count_bits) <= c->counted) ++count_bits;
    struct Pass { const unsigned long long *values; int shift; uint32_t flip; int bits; };
    std::vector<Pass> passes;
    passes.push_back({c->keys.p, 0, 0u, std::min(32, 2 * c->length)});
    if (c->length > 16) passes.push_back({c->keys.p, 32, 0u, 2 * c->length - 32});
    passes.push_back({c->counts.p, 0, count_bits >= 32 ? ~0u : (1u << count_bits) - 1u, std::min(32, count_bits)});
    if (count_bits > 32) passes.push_back({c->counts.p, 32, (uint32_t)((1ULL << (count_bits - 32)) - 1ULL), count_bits - 32});
    for (const Pass &p : passes) {
        launch_census_sort_word(p.values, c->perm.p, D, p.shift, p.flip, c->word.p, nullptr);
        HIP_TRY(hipGetLastError());
        if (sort_pairs_u32(c->word.p, c->word_sorted.p, c->perm.p, c->perm_sorted.p, D, p.bits, nullptr) != 0)
            return fail(SKM_ERR_HIP, "ranking %lld barcodes: %s", (long long)D, quant_setup_failure());
        std::swap(c->perm, c->perm_sorted);
    }
    launch_census_gather(c->keys.p, c->counts.p, c->perm.p, D, c->ranked_keys.p, c->ranked_counts.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    drain.dismiss();
    c->ranked = true;
    return SKM_OK;
}

}  // namespace

extern "C" int skm_barcode_census_create(int device, int length, skm_barcode_census **out)
{
    SKM_TRY(check_device(device));
    if (!out) return fail(SKM_ERR_ARG, "bad argument");
    if (length < 1 || length > 32) return fail(SKM_ERR_ARG, "barcodes of %d bases: 1 to 32 are possible", length);
    uint32_t bits = 10;
    bool test_slots = false;
    if (const char *v = getenv("SKM_TEST_CENSUS_SLOTS")) {       // test hook: a census table that has to grow under a launch
        const long long n = atoll(v);
        if (n < 2 || n > (1LL << 30) || (n & (n - 1)))
            return fail(SKM_ERR_ARG, "SKM_TEST_CENSUS_SLOTS must be a power of two from 2 to 2^30, not '%s'", v);
        bits = 1;
        while ((1LL << bits) < n) ++bits;
        test_slots = true;
    }
    SKM_TRY(set_device(device));
    auto c = std::make_unique<skm_barcode_census>();
    c->device = device; c->length = length; c->test_slots = test_slots;
    SKM_TRY(c->ctl.ensure(CENSUS_CTL_ROOM));
    HIP_TRY(hipMemsetAsync(c->ctl.p, 0, CENSUS_CTL_ROOM * 8, nullptr));
    SKM_TRY(census_grow(c.get(), bits));
    *out = c.release();
    return SKM_OK;
}

extern "C" int skm_barcode_census_destroy(skm_barcode_census *census)
{
    delete census;
    return SKM_OK;
}

extern "C" int skm_barcode_census_add(skm_barcode_census *c, const skm_packed_reads *reads, int start, int64_t stats[3])
{
    if (!c || !reads || !stats) return fail(SKM_ERR_ARG, "bad argument");
    if (start < 0 || start > (1 << 24)) return fail(SKM_ERR_ARG, "a barcode that starts at base %d", start);
    SKM_TRY(window_piece_check(reads));
    const int64_t n = reads->n_reads;
    std::lock_guard<std::mutex> hold(c->mu);
    if (c->failed) return fail(SKM_ERR_STATE, "the census has failed: %s", c->failed_msg.c_str());
    if (n == 0) return SKM_OK;
    SKM_TRY(set_device(c->device));
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: the scratch is in use)
    if (!c->test_slots) {
        uint32_t bits = c->slot_bits;
        while ((1LL << bits) < 2 * (c->entries + n)) ++bits;
        if (bits > c->slot_bits) SKM_TRY(census_grow(c, bits));
    }
    SKM_TRY(c->deferred.ensure((size_t)(2 * n)));
    HIP_TRY(hipMemsetAsync(c->ctl.p + CENSUS_CTL_DEFERRED, 0, (CENSUS_CTL_WORDS - CENSUS_CTL_DEFERRED) * 8, nullptr));
    BarcodeWindows w{};
    SKM_TRY(window_piece_upload(c->windows, reads, start, c->length, &w));
    c->ranked = false;
    launch_census_count(c->table(c->deferred.p, n), w, nullptr);
    HIP_TRY(hipGetLastError());
    unsigned long long ctl[CENSUS_CTL_WORDS];
    HIP_TRY(hipMemcpy(ctl, c->ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
    c->entries = (int64_t)ctl[CENSUS_CTL_ENTRIES];
    const int64_t deferred = (int64_t)ctl[CENSUS_CTL_DEFERRED];
    char text[200];
    if (deferred > n) {
        snprintf(text, sizeof(text), "a launch deferred %lld pairs of a piece of %lld reads", (long long)deferred, (long long)n);
        return census_fail(c, SKM_ERR_STATE, text);
    }
    if (deferred) {
        // the table was full: room for everything deferred, then the pairs again
        uint32_t bits = c->slot_bits + 1;
        while ((1LL << bits) < 2 * (c->entries + deferred)) ++bits;
        SKM_TRY(census_grow(c, bits));               // (leaves ctl[CENSUS_CTL_DEFERRED] at 0)
        launch_census_replay(c->table(), c->deferred.p, deferred, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(ctl, c->ctl.p, 3 * 8, hipMemcpyDeviceToHost));
        c->entries = (int64_t)ctl[CENSUS_CTL_ENTRIES];
        if (ctl[CENSUS_CTL_DEFERRED]) {
            snprintf(text, sizeof(text), "%llu barcodes found no slot in a table grown for them", ctl[CENSUS_CTL_DEFERRED]);
            return census_fail(c, SKM_ERR_STATE, text);
        }
    }
    drain.dismiss();                          // (the copies home have waited for the kernels)
    c->sentinel = (int64_t)ctl[CENSUS_CTL_SENTINEL];
    c->counted += (int64_t)ctl[CENSUS_CTL_COUNTED];
    for (int k = 0; k < 3; ++k) stats[k] += (int64_t)ctl[CENSUS_CTL_COUNTED + k];
    return SKM_OK;
}

extern "C" int skm_barcode_census_size(skm_barcode_census *c, int64_t *n_distinct, int64_t *n_counted)
{
    if (!c || !n_distinct || !n_counted) return fail(SKM_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> hold(c->mu);
    if (c->failed) return fail(SKM_ERR_STATE, "the census has failed: %s", c->failed_msg.c_str());
    *n_distinct = c->entries + (c->sentinel ? 1 : 0);
    *n_counted = c->counted;
    return SKM_OK;
}

extern "C" int skm_barcode_census_ranked(skm_barcode_census *c, int64_t cap, uint64_t *keys, int64_t *counts)
{
    if (!c || cap < 0 || (cap && (!keys || !counts))) return fail(SKM_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> hold(c->mu);
    if (c->failed) return fail(SKM_ERR_STATE, "the census has failed: %s", c->failed_msg.c_str());
    SKM_TRY(set_device(c->device));
    SKM_TRY(census_rank(c));
    const int64_t n = std::min(cap, c->n_ranked);
    if (n) {
        HIP_TRY(hipMemcpy(keys, c->ranked_keys.p, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts, c->ranked_counts.p, n * 8, hipMemcpyDeviceToHost));
    }
    return SKM_OK;
}

extern "C" int skm_barcode_census_pick(skm_barcode_census *c, int64_t expect_cells, int drop_neighbours, int64_t cap,
                                       uint64_t *keys, int64_t *counts, int64_t info[6])
{
    if (!c || !info || cap < 0 || (cap && (!keys || !counts))) return fail(SKM_ERR_ARG, "bad argument");
    if (expect_cells < 1) return fail(SKM_ERR_ARG, "%lld expected cells: 1 at least", (long long)expect_cells);
    std::lock_guard<std::mutex> hold(c->mu);
    if (c->failed) return fail(SKM_ERR_STATE, "the census has failed: %s", c->failed_msg.c_str());
    SKM_TRY(set_device(c->device));
    SKM_TRY(census_rank(c));
    const int64_t D = c->n_ranked;
    if (D == 0) return fail(SKM_ERR_STATE, "no readable barcode");
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });
    const int64_t rank = std::min(expect_cells / 100 + (expect_cells % 100 ? 1 : 0), D);
    unsigned long long m = 0, found[2] = {0, 0};
    HIP_TRY(hipMemcpy(&m, c->ranked_counts.p + (rank - 1), 8, hipMemcpyDeviceToHost));
    const unsigned long long threshold = std::max<unsigned long long>((m + 9) / 10, 1);
    HIP_TRY(hipMemsetAsync(c->ctl.p + CENSUS_CTL_OUT + 1, 0, 8, nullptr));
    launch_census_candidates(c->ranked_counts.p, D, threshold, c->ctl.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(found, c->ctl.p + CENSUS_CTL_OUT + 1, 8, hipMemcpyDeviceToHost));
    const int64_t n_candidates = (int64_t)found[0];
    if (n_candidates < rank || n_candidates > D) return fail(SKM_ERR_STATE, "%lld candidates of %lld barcodes", (long long)n_candidates, (long long)D);
    int64_t n_dropped = 0;
    const unsigned long long *from_keys = c->ranked_keys.p, *from_counts = c->ranked_counts.p;
    if (drop_neighbours) {
        HIP_TRY(hipMemsetAsync(c->ctl.p + CENSUS_CTL_OUT + 2, 0, 8, nullptr));
        launch_census_pick(c->table(), c->ranked_keys.p, c->ranked_counts.p, n_candidates, threshold, c->word.p, c->perm.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(found + 1, c->ctl.p + CENSUS_CTL_OUT + 2, 8, hipMemcpyDeviceToHost));
        n_dropped = (int64_t)found[1];
        if (n_dropped < 0 || n_dropped >= n_candidates) return fail(SKM_ERR_STATE, "%lld of %lld candidates dropped", (long long)n_dropped, (long long)n_candidates);
        if (n_dropped) {
            // the stable sort on the one flag bit is the compaction: the candidates that stay come first, in ranked order
            if (sort_pairs_u32(c->word.p, c->word_sorted.p, c->perm.p, c->perm_sorted.p, n_candidates, 1, nullptr) != 0)
                return fail(SKM_ERR_HIP, "picking from %lld candidates: %s", (long long)n_candidates, quant_setup_failure());
            SKM_TRY(c->picked_keys.ensure(n_candidates - n_dropped)); SKM_TRY(c->picked_counts.ensure(n_candidates - n_dropped));
            launch_census_gather(c->ranked_keys.p, c->ranked_counts.p, c->perm_sorted.p, n_candidates - n_dropped, c->picked_keys.p,
                                 c->picked_counts.p, nullptr);
            HIP_TRY(hipGetLastError());
            from_keys = c->picked_keys.p; from_counts = c->picked_counts.p;
        }
    }
    const int64_t n_picked = n_candidates - n_dropped;
    info[0] = rank; info[1] = (int64_t)m; info[2] = (int64_t)threshold; info[3] = n_candidates; info[4] = n_dropped; info[5] = n_picked;
    if (n_picked > cap) return fail(SKM_ERR_STATE, "%lld barcodes picked, room for %lld", (long long)n_picked, (long long)cap);
    HIP_TRY(hipMemcpy(keys, from_keys, n_picked * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, from_counts, n_picked * 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}
