// Cell barcodes ("Cell barcodes"): which cell of a whitelist every unit of a pooled run
// belongs to, and the units of a run grouped by cell.
//
// (a) barcode_clean_kernel + barcode_assign_kernel.  The whitelist is an open-addressing table in HBM (BarcodeTable,
// skm_kernels.h): key = the 2 L code bits of an entry, linear probing, at most half full, so a probe ends at an
// empty slot.  A whitelist of up to BARCODE_LDS_MAX_ENTRIES entries (a 96- or 384-well plate) is copied into LDS by
// every block, with per-block unit counters beside it; a larger one is probed where it lies (a 5 000-entry table
// is 96 KB and stays in L2).
//   One lane per unit, grid-stride.  A lane cuts its window out of one or two 64-bit code words, looks at the
// window's "clean" bits -- scattered beforehand from the piece's sparse exception list into one dense word per
// unit -- and probes once: most lanes are done there.  The lanes that are not (a substitution, one N) need the
// 3 L single substitutions, or the 4 bases at the N.  A lane that walked them alone would hold its wave for 3 L
// dependent probes; instead the wave takes such a unit together, 64 candidates a round, while they are few
// (units x rounds <= L), and each lane walks its own list only when so many lanes need it that this is cheaper.
// Both ways count the same candidates, so the answer does not depend on the path.
//   Every index is bounded before use: a window that the piece's words do not hold is "short", exception read
// numbers are checked by the host, a cell index comes from the table the host built.
//   The five counters are summed in LDS and leave a block as five atomics; units per cell are integer atomics
// (any order, same counts).
//
// (b) grouping: keys (the sample, or n_samples for a dropped unit) + the unit numbers go through the stable
// radix sort of skm_quant_setup.hip; offsets[] are the places where the ascending keys change.
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"

#include <algorithm>

namespace skm {

__global__ void __launch_bounds__(256)
barcode_clean_kernel(const uint32_t *__restrict__ exception_reads, const uint32_t *__restrict__ masks, int64_t n_exceptions,
                     int words, int offset, uint32_t *__restrict__ clean)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= n_exceptions) return;
    const uint32_t *m = masks + e * words;
    uint32_t v = m[0] << offset;
    if (offset && words == 2) v |= m[1] >> (32 - offset);
    clean[exception_reads[e]] = v;            // (positions past the words at hand read as not clean: they lie past L)
}

void launch_barcode_clean(const uint32_t *exception_reads, const uint32_t *masks, int64_t n_exceptions, int words,
                          int offset, uint32_t *clean, hipStream_t stream)
{
    if (n_exceptions <= 0 || words <= 0) return;
    hipLaunchKernelGGL(barcode_clean_kernel, dim3((unsigned)((n_exceptions + 255) / 256)), dim3(256), 0, stream,
                       exception_reads, masks, n_exceptions, words, offset, clean);
}

namespace {

enum { BC_EXACT = 0, BC_CORRECTED = 1, BC_AMBIGUOUS = 2, BC_NO_MATCH = 3, BC_UNREADABLE = 4 };

template <bool LDS>
__global__ void __launch_bounds__(256)
barcode_assign_kernel(BarcodeTable t, BarcodeWindows w, int max_mismatches, int32_t *__restrict__ cell,
                      unsigned long long *cell_units, unsigned long long *stats)
{
    constexpr int LDS_SLOTS = LDS ? 2 * BARCODE_LDS_MAX_ENTRIES : 1;
    __shared__ uint64_t s_keys[LDS_SLOTS];
    __shared__ int32_t s_cells[LDS_SLOTS];
    __shared__ unsigned int s_units[LDS ? BARCODE_LDS_MAX_ENTRIES : 1];
    __shared__ unsigned int s_stats[BARCODE_STATS];
    const uint32_t slot_mask = (1u << t.slot_bits) - 1u;
    if (LDS) {
        for (uint32_t s = threadIdx.x; s <= slot_mask; s += 256) { s_keys[s] = t.keys[s]; s_cells[s] = t.cells[s]; }
        for (int64_t c = threadIdx.x; c < t.n_entries; c += 256) s_units[c] = 0;
    }
    if (threadIdx.x < BARCODE_STATS) s_stats[threadIdx.x] = 0;
    __syncthreads();
    auto lookup = [&](uint64_t key) -> int {
        uint32_t s = barcode_slot(key, t.slot_bits);
        for (;;) {            // (at most half full: an empty slot ends every walk)
            const int c = LDS ? s_cells[s] : t.cells[s];
            if (c < 0) return -1;
            if ((LDS ? s_keys[s] : t.keys[s]) == key) return c;
            s = (s + 1) & slot_mask;
        }
    };
    const int lane = threadIdx.x & 63;
    const int L = t.length;
    const uint32_t window_bits = L == 32 ? ~0u : ~(~0u >> L);
    const bool two_words = w.offset + L > 32;
    // (every lane of a wave makes every round: the ballots below are the whole wave's)
    for (int64_t base = blockIdx.x * 256LL; base < w.n_reads; base += gridDim.x * 256LL) {
        const int64_t u = base + threadIdx.x;
        int category = -1, result = -1;
        bool need = false;
        uint64_t key = 0;
        uint32_t bad = 0;
        if (u < w.n_reads) {
            const int64_t len = w.lengths ? (int64_t)w.lengths[u] : w.uniform_len;
            if (w.words == 0 || len < (int64_t)w.start + L || (two_words && w.words < 2)) {
                category = BC_UNREADABLE;                     // short
            } else {
                const uint64_t *c = w.codes + u * w.words;
                uint64_t high = c[0] << (2 * w.offset);
                if (two_words) high |= c[1] >> (64 - 2 * w.offset);       // (offset > 0 here)
                key = high >> (64 - 2 * L);
                bad = ~w.clean[u] & window_bits;
                if (__popc(bad) >= 2) {
                    category = BC_UNREADABLE;
                } else {
                    if (!bad && (result = lookup(key)) >= 0) category = BC_EXACT;
                    else if (max_mismatches == 0) category = BC_NO_MATCH;
                    else need = true;
                }
            }
        }
        unsigned long long todo = __ballot(need);
        if (todo) {
            const int rounds = (3 * L + 63) / 64;
            if (__popcll(todo) * rounds <= L) {
                while (todo) {                                // the wave takes one unit's candidates together
                    const int src = __ffsll(todo) - 1;
                    todo &= todo - 1;
                    const uint64_t src_key = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), src) << 32)
                                             | (uint32_t)__shfl((int)(uint32_t)key, src);
                    const uint32_t src_bad = (uint32_t)__shfl((int)bad, src);
                    const int n_candidates = src_bad ? 4 : 3 * L;
                    int hits = 0, found = -1;
                    for (int first = 0; first < n_candidates; first += 64) {
                        const int j = first + lane;
                        const int c = j < n_candidates ? lookup(barcode_candidate(src_key, src_bad, L, j)) : -1;
                        const unsigned long long hit = __ballot(c >= 0);
                        hits += __popcll(hit);
                        if (hit) found = __shfl(c, __ffsll(hit) - 1);
                    }
                    if (lane == src) {
                        result = hits == 1 ? found : -1;
                        category = hits == 1 ? BC_CORRECTED : hits ? BC_AMBIGUOUS : BC_NO_MATCH;
                    }
                }
            } else if (need) {
                const int n_candidates = bad ? 4 : 3 * L;
                int hits = 0, found = -1;
                for (int j = 0; j < n_candidates && hits < 2; ++j) {
                    const int c = lookup(barcode_candidate(key, bad, L, j));
                    if (c >= 0) { ++hits; found = c; }
                }
                result = hits == 1 ? found : -1;
                category = hits == 1 ? BC_CORRECTED : hits ? BC_AMBIGUOUS : BC_NO_MATCH;
            }
        }
        if (u < w.n_reads) {
            cell[u] = result;
            if (result >= 0) {
                if (LDS) atomicAdd(&s_units[result], 1u);
                else atomicAdd(cell_units + result, 1ULL);
            }
        }
#pragma unroll
        for (int k = 0; k < BARCODE_STATS; ++k) {
            const unsigned long long with = __ballot(category == k);
            if (lane == 0 && with) atomicAdd(&s_stats[k], (unsigned int)__popcll(with));
        }
    }
    __syncthreads();
    if (threadIdx.x < BARCODE_STATS && s_stats[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)s_stats[threadIdx.x]);
    if (LDS)
        for (int64_t c = threadIdx.x; c < t.n_entries; c += 256)
            if (s_units[c]) atomicAdd(cell_units + c, (unsigned long long)s_units[c]);
}

__global__ void __launch_bounds__(256)
group_keys_kernel(const int32_t *__restrict__ sample, int64_t n, int64_t n_samples, uint32_t *__restrict__ keys,
                  int32_t *__restrict__ vals, int *error)
{
    for (int64_t u = blockIdx.x * 256LL + threadIdx.x; u < n; u += gridDim.x * 256LL) {
        const int32_t s = sample[u];
        if (s >= n_samples) *error = SKM_ERR_ARG;
        keys[u] = s < 0 || s >= n_samples ? (uint32_t)n_samples : (uint32_t)s;
        vals[u] = (int32_t)u;
    }
}

__global__ void __launch_bounds__(256)
group_offsets_kernel(const uint32_t *__restrict__ keys, int64_t n, int64_t n_samples, int64_t *__restrict__ offsets)
{
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i <= n; i += gridDim.x * 256LL) {
        const int64_t from = i == 0 ? 0 : (int64_t)keys[i - 1] + 1;
        const int64_t to = i == n ? n_samples : (int64_t)keys[i];         // (keys are <= n_samples)
        for (int64_t s = from; s <= to; ++s) offsets[s] = i;
    }
}

unsigned grid_for(int64_t n)
{
    return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 2048);
}

}  // namespace

void launch_barcode_assign(const BarcodeTable &table, const BarcodeWindows &w, int max_mismatches, int32_t *cell,
                           unsigned long long *cell_units, unsigned long long *stats, hipStream_t stream)
{
    if (w.n_reads <= 0) return;
    const bool lds = table.n_entries <= BARCODE_LDS_MAX_ENTRIES && (1LL << table.slot_bits) <= 2 * BARCODE_LDS_MAX_ENTRIES;
    if (lds)
        hipLaunchKernelGGL(barcode_assign_kernel<true>, dim3(grid_for(w.n_reads)), dim3(256), 0, stream, table, w,
                           max_mismatches, cell, cell_units, stats);
    else
        hipLaunchKernelGGL(barcode_assign_kernel<false>, dim3(grid_for(w.n_reads)), dim3(256), 0, stream, table, w,
                           max_mismatches, cell, cell_units, stats);
}

void launch_group_keys(const int32_t *sample, int64_t n, int64_t n_samples, uint32_t *keys, int32_t *vals, int *error,
                       hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(group_keys_kernel, dim3(grid_for(n)), dim3(256), 0, stream, sample, n, n_samples, keys, vals, error);
}

void launch_group_offsets(const uint32_t *sorted_keys, int64_t n, int64_t n_samples, int64_t *offsets, hipStream_t stream)
{
    hipLaunchKernelGGL(group_offsets_kernel, dim3(grid_for(n + 1)), dim3(256), 0, stream, sorted_keys, n, n_samples, offsets);
}

}  // namespace skm
