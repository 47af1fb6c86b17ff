// sequential CPU versions of the launchers skm_barcode_census_* calls, for scripts/micro/census_host_asan.cpp: the same
// table layout and probing as skm_census.hip, one unit after the other
#include "seekmer_hip.h"
#include "skm_kernels.h"
#include <algorithm>
#include <numeric>
#include <vector>
namespace skm {
static bool add(const CensusTable &t, unsigned long long key, unsigned long long count)
{
    const uint64_t n = 1ULL << t.slot_bits; uint32_t s = barcode_slot(key, t.slot_bits);
    for (uint64_t i = 0; i < n; ++i, s = (s + 1) & (uint32_t)(n - 1)) {
        if (t.slots[s].key == CENSUS_EMPTY) { t.slots[s].key = key; ++t.ctl[CENSUS_CTL_ENTRIES]; }
        if (t.slots[s].key == key) { t.slots[s].count += count; return true; }
    }
    return false;
}
static void defer(const CensusTable &t, unsigned long long key, unsigned long long count)
{
    const unsigned long long at = t.ctl[CENSUS_CTL_DEFERRED]++;
    if (t.deferred && at < (unsigned long long)t.deferred_cap) { t.deferred[2 * at] = key; t.deferred[2 * at + 1] = count; }
}
static unsigned long long find(const CensusTable &t, unsigned long long key)
{
    if (key == CENSUS_EMPTY) return t.ctl[CENSUS_CTL_SENTINEL];
    const uint64_t n = 1ULL << t.slot_bits; uint32_t s = barcode_slot(key, t.slot_bits);
    for (uint64_t i = 0; i < n; ++i, s = (s + 1) & (uint32_t)(n - 1)) {
        if (t.slots[s].key == key) return t.slots[s].count;
        if (t.slots[s].key == CENSUS_EMPTY) return 0;
    }
    return 0;
}
void launch_census_init(const CensusTable &t, hipStream_t) { for (uint64_t i = 0; i < (1ULL << t.slot_bits); ++i) t.slots[i] = CensusSlot{CENSUS_EMPTY, 0}; }
void launch_census_rehash(const CensusTable &from, const CensusTable &to, hipStream_t s)
{
    launch_census_init(to, s);
    for (uint64_t i = 0; i < (1ULL << from.slot_bits); ++i) {
        if (from.slots[i].key == CENSUS_EMPTY) continue;
        const uint64_t n = 1ULL << to.slot_bits; uint32_t at = barcode_slot(from.slots[i].key, to.slot_bits); bool placed = false;
        for (uint64_t k = 0; k < n && !placed; ++k) { if (to.slots[at].key == CENSUS_EMPTY) { to.slots[at] = from.slots[i]; placed = true; } else at = (at + 1) & (uint32_t)(n - 1); }
        if (!placed) ++to.ctl[CENSUS_CTL_DEFERRED];
    }
}
void launch_census_count(const CensusTable &t, const BarcodeWindows &w, hipStream_t)
{
    const int L = t.length; const uint32_t bits = L == 32 ? ~0u : ~(~0u >> L); const bool two = w.offset + L > 32;
    for (int64_t u = 0; u < w.n_reads; ++u) {
        const int64_t len = w.lengths ? (int64_t)w.lengths[u] : w.uniform_len;
        if (w.words == 0 || len < (int64_t)w.start + L || (two && w.words < 2)) { ++t.ctl[CENSUS_CTL_SHORT]; continue; }
        if (~w.clean[u] & bits) { ++t.ctl[CENSUS_CTL_UNREADABLE]; continue; }
        const uint64_t *c = w.codes + u * w.words; uint64_t high = c[0] << (2 * w.offset);
        if (two) high |= c[1] >> (64 - 2 * w.offset);
        const unsigned long long key = high >> (64 - 2 * L);
        ++t.ctl[CENSUS_CTL_COUNTED];
        if (key == CENSUS_EMPTY) ++t.ctl[CENSUS_CTL_SENTINEL]; else if (!add(t, key, 1)) defer(t, key, 1);
    }
}
void launch_census_replay(const CensusTable &t, const unsigned long long *p, int64_t n, hipStream_t) { for (int64_t i = 0; i < n; ++i) if (!add(t, p[2 * i], p[2 * i + 1])) defer(t, 0, 0); }
void launch_census_compact(const CensusTable &t, unsigned long long *keys, unsigned long long *counts, int32_t *iota, hipStream_t)
{
    auto put = [&](unsigned long long k, unsigned long long c) { const unsigned long long at = t.ctl[CENSUS_CTL_OUT]++; if (at < t.ctl[CENSUS_CTL_ENTRIES] + 1) { keys[at] = k; counts[at] = c; iota[at] = (int32_t)at; } };
    if (t.ctl[CENSUS_CTL_SENTINEL]) put(CENSUS_EMPTY, t.ctl[CENSUS_CTL_SENTINEL]);
    for (uint64_t i = 0; i < (1ULL << t.slot_bits); ++i) if (t.slots[i].key != CENSUS_EMPTY) put(t.slots[i].key, t.slots[i].count);
}
void launch_census_sort_word(const unsigned long long *v, const int32_t *perm, int64_t n, int shift, uint32_t flip, uint32_t *word, hipStream_t) { for (int64_t i = 0; i < n; ++i) word[i] = (uint32_t)(v[perm[i]] >> shift) ^ flip; }
void launch_census_gather(const unsigned long long *k, const unsigned long long *c, const int32_t *perm, int64_t n, unsigned long long *ok, unsigned long long *oc, hipStream_t) { for (int64_t i = 0; i < n; ++i) { ok[i] = k[perm[i]]; oc[i] = c[perm[i]]; } }
void launch_census_candidates(const unsigned long long *c, int64_t n, unsigned long long th, unsigned long long *ctl, hipStream_t) { for (int64_t i = 0; i < n; ++i) if (c[i] >= th && (i + 1 == n || c[i + 1] < th)) ctl[CENSUS_CTL_OUT + 1] = (unsigned long long)(i + 1); }
void launch_census_pick(const CensusTable &t, const unsigned long long *keys, const unsigned long long *counts, int64_t n, unsigned long long th, uint32_t *dropped, int32_t *iota, hipStream_t)
{
    for (int64_t i = 0; i < n; ++i) {
        bool drop = false;
        for (int j = 0; j < 3 * t.length && !drop; ++j) {
            const int shift = 2 * (t.length - 1 - j / 3); const uint64_t base = (keys[i] >> shift) & 3;
            const unsigned long long other = keys[i] ^ ((base ^ ((base + 1 + j % 3) & 3)) << shift), seen = find(t, other);
            drop = seen >= th && (seen > counts[i] || (seen == counts[i] && other < keys[i]));
        }
        dropped[i] = drop; iota[i] = (int32_t)i; t.ctl[CENSUS_CTL_OUT + 2] += drop;
    }
}
void launch_barcode_clean(const uint32_t *er, const uint32_t *masks, int64_t n, int words, int offset, uint32_t *clean, hipStream_t)
{
    for (int64_t e = 0; e < n; ++e) { const uint32_t *m = masks + e * words; uint32_t v = m[0] << offset; if (offset && words == 2) v |= m[1] >> (32 - offset); clean[er[e]] = v; }
}
int sort_pairs_u32(const uint32_t *ki, uint32_t *ko, const int32_t *vi, int32_t *vo, int64_t n, int end_bit, hipStream_t)
{
    const uint32_t mask = end_bit >= 32 ? ~0u : (1u << end_bit) - 1u;
    std::vector<int64_t> order((size_t)n); std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return (ki[a] & mask) < (ki[b] & mask); });
    for (int64_t i = 0; i < n; ++i) { ko[i] = ki[order[i]]; vo[i] = vi[order[i]]; }
    return 0;
}
const char *quant_setup_failure() { return ""; }
}
