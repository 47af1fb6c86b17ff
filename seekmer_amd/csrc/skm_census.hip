// Cell discovery ("Cell discovery"): an exact count of every distinct barcode of a pooled run,
// and from it the barcodes that are cells -- a whitelist made from the reads themselves.
//
// (a) the census table: open addressing in HBM, linear probing from barcode_slot(key), 16 bytes a slot (key, count),
// a power of two slots, sized ahead of every launch to at most half full.  With L = 32 every 64-bit value is a key,
// so none is free to mean "empty": CENSUS_EMPTY (all ones, the all-T 32-mer) marks an empty slot, and that one
// barcode is counted in ctl[CENSUS_CTL_SENTINEL] instead of a slot.  A key never changes once it is set.
//
// (b) census_count_kernel.  One lane per unit, grid-stride; the window is cut out of the BarcodeWindows upload as
// barcode_assign_kernel cuts it.  A plate sends every unit to one of 96 counters, so a block first combines equal
// keys in an LDS table (CENSUS_LDS_SLOTS slots, claimed by a 64-bit LDS atomicCAS, at most CENSUS_LDS_PROBES probes)
// and sends one 64-bit atomic per distinct key and block to HBM when it is done; a key that finds no LDS slot goes
// to HBM directly.  In HBM: find or claim by atomicCAS on the key, then atomicAdd on the count.  The probe reads are
// plain loads: a stale "empty" only costs the CAS that reports the real key.  Integer adds: any order, same counts.
//   What finds the table full (tests: SKM_TEST_CENSUS_SLOTS) is appended to a list of (key, count) pairs, which the
// host replays after it has grown the table.  A pair stands for at least one unit of the piece, so the piece's
// unit count bounds the list; the index is checked against that room all the same.
//   Every index is bounded before use: a window that the piece's words do not hold is short (the host has checked
// the exception read numbers), slots by the mask, probe walks by the number of slots.
//
// (c) ranking: the occupied slots are compacted to (key, count) and ordered by the stable radix sort of
// skm_quant_setup.hip over a permutation, one pass per 32-bit word (the host drives it: skm_abi_cells.hip).
//
// (d) census_pick_kernel.  One lane per candidate (count >= threshold): its 3 L single substitutions are looked up
// in the census table; a neighbour that is a candidate too and ranks earlier (a larger count, or an equal count and
// a smaller key) drops the lane's candidate.  Whether that neighbour is dropped itself does not matter, so no lane
// waits for another.
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"

#include <algorithm>

namespace skm {

namespace {

constexpr int CENSUS_LDS_SLOTS = 1024;        // 12 KB a block: keys and 32-bit counts
constexpr int CENSUS_LDS_PROBES = 8;

// (key != CENSUS_EMPTY) `count` more windows under `key`; false: the table is full
__device__ __forceinline__ bool census_add(const CensusTable &t, unsigned long long key, unsigned long long count,
                                           unsigned int &claimed)
{
    const uint64_t n_slots = 1ULL << t.slot_bits;
    const uint32_t mask = (uint32_t)(n_slots - 1);
    uint32_t s = barcode_slot(key, t.slot_bits);
    for (uint64_t n = 0; n < n_slots; ++n) {
        unsigned long long cur = t.slots[s].key;
        if (cur == CENSUS_EMPTY) {
            cur = atomicCAS(&t.slots[s].key, CENSUS_EMPTY, key);
            if (cur == CENSUS_EMPTY) { ++claimed; cur = key; }
        }
        if (cur == key) {
            atomicAdd(&t.slots[s].count, count);
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}

__device__ __forceinline__ void census_defer(const CensusTable &t, unsigned long long key, unsigned long long count)
{
    const unsigned long long at = atomicAdd(t.ctl + CENSUS_CTL_DEFERRED, 1ULL);
    if (t.deferred && at < (unsigned long long)t.deferred_cap) {
        t.deferred[2 * at] = key;
        t.deferred[2 * at + 1] = count;
    }
}

// the count of `key` in the table, 0 if it is not there
__device__ __forceinline__ unsigned long long census_find(const CensusTable &t, unsigned long long key)
{
    if (key == CENSUS_EMPTY) return t.ctl[CENSUS_CTL_SENTINEL];
    const uint64_t n_slots = 1ULL << t.slot_bits;
    const uint32_t mask = (uint32_t)(n_slots - 1);
    uint32_t s = barcode_slot(key, t.slot_bits);
    for (uint64_t n = 0; n < n_slots; ++n) {
        const unsigned long long cur = t.slots[s].key;
        if (cur == key) return t.slots[s].count;
        if (cur == CENSUS_EMPTY) return 0;
        s = (s + 1) & mask;
    }
    return 0;
}

__global__ void __launch_bounds__(256)
census_init_kernel(CensusSlot *slots, uint64_t n_slots)
{
    for (uint64_t i = blockIdx.x * 256ULL + threadIdx.x; i < n_slots; i += gridDim.x * 256ULL) {
        slots[i].key = CENSUS_EMPTY;
        slots[i].count = 0;
    }
}

// one lane per old slot: its key claims a slot of the new table, which then takes the count with a plain store
// (every key is in one old slot only, so nobody else touches that count in this launch)
__global__ void __launch_bounds__(256)
census_rehash_kernel(CensusTable from, CensusTable to)
{
    const uint64_t n_from = 1ULL << from.slot_bits, n_to = 1ULL << to.slot_bits;
    const uint32_t mask = (uint32_t)(n_to - 1);
    for (uint64_t i = blockIdx.x * 256ULL + threadIdx.x; i < n_from; i += gridDim.x * 256ULL) {
        const CensusSlot entry = from.slots[i];
        if (entry.key == CENSUS_EMPTY) continue;
        uint32_t s = barcode_slot(entry.key, to.slot_bits);
        bool placed = false;
        for (uint64_t n = 0; n < n_to; ++n) {
            if (atomicCAS(&to.slots[s].key, CENSUS_EMPTY, entry.key) == CENSUS_EMPTY) { placed = true; break; }
            s = (s + 1) & mask;
        }
        if (placed) to.slots[s].count = entry.count;
        else atomicAdd(to.ctl + CENSUS_CTL_DEFERRED, 1ULL);       // (the host has made room; it reads the word and fails the handle)
    }
}

__global__ void __launch_bounds__(256)
census_count_kernel(CensusTable t, BarcodeWindows w)
{
    __shared__ unsigned long long s_keys[CENSUS_LDS_SLOTS];
    __shared__ unsigned int s_counts[CENSUS_LDS_SLOTS];
    __shared__ unsigned int s_stats[3], s_sentinel, s_claimed;
    for (int s = threadIdx.x; s < CENSUS_LDS_SLOTS; s += 256) { s_keys[s] = CENSUS_EMPTY; s_counts[s] = 0; }
    if (threadIdx.x < 3) s_stats[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_sentinel = 0; s_claimed = 0; }
    __syncthreads();
    const int L = t.length;
    const uint32_t window_bits = L == 32 ? ~0u : ~(~0u >> L);
    const bool two_words = w.offset + L > 32;
    unsigned int counted = 0, too_short = 0, unreadable = 0, claimed = 0;
    for (int64_t u = blockIdx.x * 256LL + threadIdx.x; u < w.n_reads; u += gridDim.x * 256LL) {
        const int64_t len = w.lengths ? (int64_t)w.lengths[u] : w.uniform_len;
        if (w.words == 0 || len < (int64_t)w.start + L || (two_words && w.words < 2)) { ++too_short; continue; }
        if (~w.clean[u] & window_bits) { ++unreadable; continue; }
        const uint64_t *c = w.codes + u * w.words;
        uint64_t high = c[0] << (2 * w.offset);
        if (two_words) high |= c[1] >> (64 - 2 * w.offset);           // (offset > 0 here)
        const unsigned long long key = high >> (64 - 2 * L);
        ++counted;
        if (key == CENSUS_EMPTY) { atomicAdd(&s_sentinel, 1u); continue; }
        uint32_t s = barcode_slot(key, 10);                           // (CENSUS_LDS_SLOTS = 1 << 10)
        bool placed = false;
        for (int n = 0; n < CENSUS_LDS_PROBES; ++n) {
            unsigned long long cur = s_keys[s];
            if (cur == CENSUS_EMPTY) {
                cur = atomicCAS(&s_keys[s], CENSUS_EMPTY, key);
                if (cur == CENSUS_EMPTY) cur = key;
            }
            if (cur == key) { atomicAdd(&s_counts[s], 1u); placed = true; break; }
            s = (s + 1) & (CENSUS_LDS_SLOTS - 1);
        }
        if (!placed && !census_add(t, key, 1ULL, claimed)) census_defer(t, key, 1ULL);
    }
    if (counted) atomicAdd(&s_stats[0], counted);
    if (too_short) atomicAdd(&s_stats[1], too_short);
    if (unreadable) atomicAdd(&s_stats[2], unreadable);
    __syncthreads();
    // one atomic per distinct key of the block
    for (int s = threadIdx.x; s < CENSUS_LDS_SLOTS; s += 256) {
        const unsigned long long key = s_keys[s];
        if (key == CENSUS_EMPTY) continue;
        const unsigned long long n = s_counts[s];
        if (!census_add(t, key, n, claimed)) census_defer(t, key, n);
    }
    if (claimed) atomicAdd(&s_claimed, claimed);
    __syncthreads();
    if (threadIdx.x < 3 && s_stats[threadIdx.x])
        atomicAdd(t.ctl + CENSUS_CTL_COUNTED + threadIdx.x, (unsigned long long)s_stats[threadIdx.x]);
    if (threadIdx.x == 3 && s_sentinel) atomicAdd(t.ctl + CENSUS_CTL_SENTINEL, (unsigned long long)s_sentinel);
    if (threadIdx.x == 4 && s_claimed) atomicAdd(t.ctl + CENSUS_CTL_ENTRIES, (unsigned long long)s_claimed);
}

__global__ void __launch_bounds__(256)
census_replay_kernel(CensusTable t, const unsigned long long *__restrict__ pairs, int64_t n)
{
    unsigned int claimed = 0;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL)
        if (!census_add(t, pairs[2 * i], pairs[2 * i + 1], claimed)) census_defer(t, 0, 0);     // (counted only: no list)
    if (claimed) atomicAdd(t.ctl + CENSUS_CTL_ENTRIES, (unsigned long long)claimed);
}

// a wave's occupied slots take consecutive places: one atomic per wave
__global__ void __launch_bounds__(256)
census_compact_kernel(CensusTable t, unsigned long long *__restrict__ keys, unsigned long long *__restrict__ counts,
                      int32_t *__restrict__ iota)
{
    const uint64_t n_slots = 1ULL << t.slot_bits;
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.ctl[CENSUS_CTL_SENTINEL]) {
        const unsigned long long at = atomicAdd(t.ctl + CENSUS_CTL_OUT, 1ULL);
        if (at < t.ctl[CENSUS_CTL_ENTRIES] + 1) {                      // (the room the host has made)
            keys[at] = CENSUS_EMPTY;
            counts[at] = t.ctl[CENSUS_CTL_SENTINEL];
            iota[at] = (int32_t)at;
        }
    }
    // (every lane of a wave makes every round: the ballot is the whole wave's)
    for (uint64_t base = blockIdx.x * 256ULL; base < n_slots; base += gridDim.x * 256ULL) {
        const uint64_t i = base + threadIdx.x;
        CensusSlot entry{CENSUS_EMPTY, 0};
        if (i < n_slots) entry = t.slots[i];
        const bool full = entry.key != CENSUS_EMPTY;
        const unsigned long long with = __ballot(full);
        if (!with) continue;
        unsigned long long first = 0;
        if (lane == __ffsll(with) - 1) first = atomicAdd(t.ctl + CENSUS_CTL_OUT, (unsigned long long)__popcll(with));
        first = ((unsigned long long)(uint32_t)__shfl((int)(first >> 32), __ffsll(with) - 1) << 32)
                | (uint32_t)__shfl((int)(uint32_t)first, __ffsll(with) - 1);
        if (full) {
            const unsigned long long at = first + __popcll(with & ((1ULL << lane) - 1ULL));
            if (at < t.ctl[CENSUS_CTL_ENTRIES] + 1) {                  // (the room the host has made)
                keys[at] = entry.key;
                counts[at] = entry.count;
                iota[at] = (int32_t)at;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
census_sort_word_kernel(const unsigned long long *__restrict__ values, const int32_t *__restrict__ perm, int64_t n, int shift,
                        uint32_t flip, uint32_t *__restrict__ word)
{
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL)
        word[i] = (uint32_t)(values[perm[i]] >> shift) ^ flip;
}

__global__ void __launch_bounds__(256)
census_gather_kernel(const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ counts,
                     const int32_t *__restrict__ perm, int64_t n, unsigned long long *__restrict__ out_keys,
                     unsigned long long *__restrict__ out_counts)
{
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int32_t from = perm[i];
        out_keys[i] = keys[from];
        out_counts[i] = counts[from];
    }
}

__global__ void __launch_bounds__(256)
census_candidates_kernel(const unsigned long long *__restrict__ counts, int64_t n, unsigned long long threshold,
                         unsigned long long *ctl)
{
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL)
        if (counts[i] >= threshold && (i + 1 == n || counts[i + 1] < threshold)) ctl[CENSUS_CTL_OUT + 1] = (unsigned long long)(i + 1);
}

__global__ void __launch_bounds__(256)
census_pick_kernel(CensusTable t, const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ counts,
                   int64_t n_candidates, unsigned long long threshold, uint32_t *__restrict__ dropped, int32_t *__restrict__ iota)
{
    __shared__ unsigned int s_dropped;
    if (threadIdx.x == 0) s_dropped = 0;
    __syncthreads();
    const int n_neighbours = 3 * t.length;
    unsigned int mine = 0;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n_candidates; i += gridDim.x * 256LL) {
        const unsigned long long key = keys[i], count = counts[i];
        bool drop = false;
        for (int j = 0; j < n_neighbours && !drop; ++j) {
            const unsigned long long other = barcode_candidate(key, 0u, t.length, j);
            const unsigned long long seen = census_find(t, other);
            drop = seen >= threshold && (seen > count || (seen == count && other < key));
        }
        dropped[i] = drop ? 1u : 0u;
        iota[i] = (int32_t)i;
        mine += drop;
    }
    if (mine) atomicAdd(&s_dropped, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_dropped) atomicAdd(t.ctl + CENSUS_CTL_OUT + 2, (unsigned long long)s_dropped);
}

unsigned census_grid(int64_t n)
{
    return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 2048);
}

}  // namespace

void launch_census_init(const CensusTable &t, hipStream_t stream)
{
    hipLaunchKernelGGL(census_init_kernel, dim3(census_grid(1LL << t.slot_bits)), dim3(256), 0, stream, t.slots, 1ULL << t.slot_bits);
}

void launch_census_rehash(const CensusTable &from, const CensusTable &to, hipStream_t stream)
{
    launch_census_init(to, stream);
    hipLaunchKernelGGL(census_rehash_kernel, dim3(census_grid(1LL << from.slot_bits)), dim3(256), 0, stream, from, to);
}

void launch_census_count(const CensusTable &t, const BarcodeWindows &w, hipStream_t stream)
{
    if (w.n_reads <= 0) return;
    // (a block's LDS table is flushed once, at its end: fewer, longer blocks send fewer atomics to HBM)
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((w.n_reads + 1023) / 1024, 1), 1024);
    hipLaunchKernelGGL(census_count_kernel, dim3(blocks), dim3(256), 0, stream, t, w);
}

void launch_census_replay(const CensusTable &t, const unsigned long long *pairs, int64_t n, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(census_replay_kernel, dim3(census_grid(n)), dim3(256), 0, stream, t, pairs, n);
}

void launch_census_compact(const CensusTable &t, unsigned long long *keys, unsigned long long *counts, int32_t *iota,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(census_compact_kernel, dim3(census_grid(1LL << t.slot_bits)), dim3(256), 0, stream, t, keys, counts, iota);
}

void launch_census_sort_word(const unsigned long long *values, const int32_t *perm, int64_t n, int shift, uint32_t flip,
                             uint32_t *word, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(census_sort_word_kernel, dim3(census_grid(n)), dim3(256), 0, stream, values, perm, n, shift, flip, word);
}

void launch_census_gather(const unsigned long long *keys, const unsigned long long *counts, const int32_t *perm, int64_t n,
                          unsigned long long *out_keys, unsigned long long *out_counts, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(census_gather_kernel, dim3(census_grid(n)), dim3(256), 0, stream, keys, counts, perm, n, out_keys, out_counts);
}

void launch_census_candidates(const unsigned long long *counts, int64_t n, unsigned long long threshold,
                              unsigned long long *ctl, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(census_candidates_kernel, dim3(census_grid(n)), dim3(256), 0, stream, counts, n, threshold, ctl);
}

void launch_census_pick(const CensusTable &t, const unsigned long long *keys, const unsigned long long *counts,
                        int64_t n_candidates, unsigned long long threshold, uint32_t *dropped, int32_t *iota,
                        hipStream_t stream)
{
    if (n_candidates <= 0) return;
    hipLaunchKernelGGL(census_pick_kernel, dim3(census_grid(n_candidates)), dim3(256), 0, stream, t, keys, counts, n_candidates,
                       threshold, dropped, iota);
}

}  // namespace skm
