// Device-side construction of the EM problem: the class-major CSR and its
// transcript-major transpose cut into rows.  The caller's class order is the
// reference's (ascending first-seen unit = collections.Counter insertion order
// under -j1, /root/reference/seekmer/mapper.py:88); internally the classes are
// kept in (smallest transcript id, first-seen) order for gather locality, with
// perm[] leading back to the caller's order.
//
// From a mapper's table the first-seen RANK of every class comes from a bitmap
// over the unit indices (first-seen values are distinct: a unit belongs to one
// class) and a prefix popcount -- no sort; one stable 18-bit radix sort of the
// classes by smallest id remains (the hand-written sort_pairs below: no library
// code on the path), everything else is small index-moving kernels.  The tiles
// of the component EM need no sort and no transposed table: their sizes follow
// from the components, their members are dropped into place in any order and a
// workgroup per tile orders them and makes both of the tile's views in LDS
// (build_tiles).  The transcript-major rows of the WHOLE table -- the second
// stable sort, of the pairs by transcript -- are a pipeline of their own
// (quant_rows_build), run when something first steps the whole table.
// One-time setup per quantification, not part of the per-step hot loop.
#include "skm_kernels.h"
#include "skm_pool.h"

#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>

namespace skm {

namespace {

// Temporaries of one setup call: handed out from the caching pool, given back
// together after ONE stream synchronisation at the end (the setup is a single
// asynchronous pipeline; nothing in between needs the host).
struct Scratch {
    hipStream_t stream;
    std::vector<void *> held;
    explicit Scratch(hipStream_t s) : stream(s) {}
    template <class T>
    T *alloc(size_t n)
    {
        void *p = nullptr;
        if (pool_alloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
        held.push_back(p);
        return static_cast<T *>(p);
    }
    ~Scratch()
    {
        (void)hipStreamSynchronize(stream);
        for (void *p : held) pool_free(p);
    }
};
// what failed last, for the caller's message (hipGetLastError is consumed by the check itself)
thread_local char g_setup_failure[160] = "";
#define QB_ALLOC(var, type, n) type *var = scratch.alloc<type>(n); \
    if (!var) { snprintf(g_setup_failure, sizeof(g_setup_failure), "no memory for %s", #var); return -1; }

#define QB_TRY(call) do { const hipError_t qb_e = (call); if (qb_e != hipSuccess) { \
    snprintf(g_setup_failure, sizeof(g_setup_failure), "%s: %s", #call, hipGetErrorString(qb_e)); return -1; } } while (0)

__global__ void __launch_bounds__(256)
iota_kernel(int32_t *out, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) out[i] = (int32_t)i;
}

// dump of the table in registry order: arena offset, length, count, first-seen per class
// (+ the class's smallest transcript id, the locality key, when asked for).
// With `bits` (cleared beforehand) the lane also marks the class's first-seen value in the bitmap over the
// unit indices that the first-seen ranks come from: one bit per unit index; a bit found set already means
// two classes share a first-seen value (possible only for tables merged from hand-made input): *duplicate
// is raised (1; 2: a value outside the bound) and the caller takes the sorting path instead.
__global__ void __launch_bounds__(256)
table_dump_kernel(ClassTable t, int64_t n_classes, int64_t *arena_off, int64_t *len, double *count,
                  unsigned long long *first_seen, uint32_t *min_id, uint64_t bound, uint32_t *bits,
                  unsigned int *duplicate)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n_classes;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t.class_list[k];
        const ClassSlot s = t.slots[i];
        const int64_t off = s.tuple < 0 ? -1 : tuple_offset(s.tuple);
        const int64_t n = s.tuple < 0 ? 0 : tuple_len(s.tuple);
        arena_off[k] = off;
        len[k] = n;
        count[k] = (double)s.count;
        first_seen[k] = s.first_seen;
        if (bits) {
            const unsigned long long f = s.first_seen;
            if (f >= bound) atomicOr(duplicate, 2u);
            else {
                const uint32_t bit = 1u << (f & 31);
                if (atomicOr(&bits[f >> 5], bit) & bit) atomicOr(duplicate, 1u);
            }
        }
        if (min_id) {
            uint32_t m = 0xffffffffu;
            for (int64_t j = 0; j < n; ++j) m = min(m, (uint32_t)t.arena[off + j]);
            min_id[k] = m;
        }
    }
}

// ---- first-seen ranks from the bitmap over the unit indices (table_dump_kernel marks it)
__global__ void __launch_bounds__(256)
word_popcount_kernel(const uint32_t *bits, int64_t n_words, int64_t *count)
{
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < n_words;
         w += (int64_t)gridDim.x * blockDim.x) count[w] = __popc(bits[w]);
}

// rank r of class k = set bits below its own; by_rank[r] = k, key_by_rank[r] = its locality key
__global__ void __launch_bounds__(256)
first_seen_rank_kernel(const unsigned long long *first_seen, const uint32_t *min_id, int64_t n_classes,
                       uint64_t bound, const uint32_t *bits, const int64_t *word_base, int32_t *by_rank,
                       uint32_t *key_by_rank)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n_classes;
         k += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long f = first_seen[k];
        if (f >= bound) continue;
        const int64_t r = word_base[f >> 5] + __popc(bits[f >> 5] & ((1u << (f & 31)) - 1u));
        if (r >= n_classes) continue;             // (only after a duplicate; the result is discarded)
        by_rank[r] = (int32_t)k;
        key_by_rank[r] = min_id[k];
    }
}

// internal class j = the class of first-seen rank perm[j] = registry entry by_rank[perm[j]].
// With *duplicate raised the ranks are not a permutation (by_rank has places nobody wrote): every class
// is then left empty, so that what is queued behind -- the scan, the copy of the tuples, the tiles --
// walks no tuple and stays within its arrays until the host reads the flag and starts over.
__global__ void __launch_bounds__(256)
gather_by_rank_kernel(const int32_t *perm, const int32_t *by_rank, int64_t n, const int64_t *len_in,
                      const double *count_in, const int64_t *arena_off_in, int64_t *len_out,
                      double *count_out, int64_t *arena_off_out, const unsigned int *duplicate)
{
    const bool unusable = *duplicate != 0;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n;
         j += (int64_t)gridDim.x * blockDim.x) {
        if (unusable) { len_out[j] = 0; count_out[j] = 0.0; arena_off_out[j] = 0; continue; }
        const int32_t k = by_rank[perm[j]];
        len_out[j] = len_in[k];
        count_out[j] = count_in[k];
        arena_off_out[j] = arena_off_in[k];
    }
}

// ids of internal class j <- arena[src_off[j] ...]
__global__ void __launch_bounds__(256)
copy_tuples_direct_kernel(int64_t n, const int64_t *src_off, const int32_t *arena, const int64_t *cls_offset,
                          int32_t *ids)
{
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = src_off[j];
        const int64_t dst = cls_offset[j];
        const int64_t len = cls_offset[j + 1] - dst;
        // (eight ids in flight at a time: a tuple is 5.4 ids on average, somewhere in the arena)
        for (int64_t i = 0; i < len; i += 8) {
            int32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = i + k < len ? arena[src + i + k] : 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) if (i + k < len) ids[dst + i + k] = v[k];
        }
    }
}

__global__ void __launch_bounds__(256)
gather_classes_kernel(const int32_t *perm, int64_t n, const int64_t *len_in, const double *count_in,
                      int64_t *len_out, double *count_out)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int32_t src = perm[k];
        len_out[k] = len_in[src];
        count_out[k] = count_in[src];
    }
}

// copy every class's tuple from the arena to its place in class order
__global__ void __launch_bounds__(256)
copy_tuples_kernel(const int32_t *perm, int64_t n, const int64_t *arena_off, const int32_t *arena,
                   const int64_t *cls_offset, int32_t *ids)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = arena_off[perm[k]];
        const int64_t dst = cls_offset[k];
        const int64_t len = cls_offset[k + 1] - dst;
        for (int64_t j = 0; j < len; ++j) ids[dst + j] = arena[src + j];
    }
}

__global__ void __launch_bounds__(256)
set_last_offset_kernel(int64_t *offsets, const int64_t *lens, int64_t n)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n] = n ? offsets[n - 1] + lens[n - 1] : 0;
}

// class index of every pair, class-major
__global__ void __launch_bounds__(256)
pair_class_kernel(const int64_t *cls_offset, int64_t n_classes, int32_t *pair_cls)
{
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_classes;
         c += (int64_t)gridDim.x * blockDim.x)
        for (int64_t j = cls_offset[c]; j < cls_offset[c + 1]; ++j) pair_cls[j] = (int32_t)c;
}

// tx_offset[t] = first position of transcript t in the key-sorted pair list
__global__ void __launch_bounds__(256)
segment_starts_kernel(const int32_t *sorted_tx, int64_t n_pairs, int64_t n_tx, int64_t *tx_offset)
{
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= n_pairs;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = j == 0 ? -1 : sorted_tx[j - 1];
        const int64_t hi = j == n_pairs ? n_tx : sorted_tx[j];
        for (int64_t t = lo + 1; t <= hi; ++t) tx_offset[t] = j;
    }
}

__global__ void __launch_bounds__(256)
row_count_kernel(const int64_t *tx_offset, int64_t n_tx, int64_t *rows)
{
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tx;
         t += (int64_t)gridDim.x * blockDim.x) {
        // (at least one row, an empty one for a transcript no class names: the launch that sums the
        // rows is also the one that finalizes the transcripts, skm_em.hip: em_rows_finalize_kernel)
        const int64_t degree = tx_offset[t + 1] - tx_offset[t];
        rows[t] = degree > 0 ? (degree + EM_ROW_CAP - 1) / EM_ROW_CAP : 1;
    }
}

__global__ void __launch_bounds__(256)
row_fill_kernel(const int64_t *tx_offset, const int64_t *tx_row, int64_t n_tx, int64_t n_pairs,
                int64_t *row_start, int32_t *row_tx)
{
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tx;
         t += (int64_t)gridDim.x * blockDim.x) {
        int64_t pos = tx_offset[t];
        for (int64_t r = tx_row[t]; r < tx_row[t + 1]; ++r) {
            row_start[r] = pos;
            row_tx[r] = (int32_t)t;
            pos += EM_ROW_CAP;
        }
        if (t == n_tx - 1) row_start[tx_row[n_tx]] = n_pairs;
    }
}

// locality key of a class: its smallest transcript id
__global__ void __launch_bounds__(256)
class_min_id_kernel(const int64_t *cls_offset, const int32_t *ids, int64_t n_classes, uint32_t *key,
                    int64_t *len)
{
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_classes;
         c += (int64_t)gridDim.x * blockDim.x) {
        uint32_t m = 0xffffffffu;
        for (int64_t j = cls_offset[c]; j < cls_offset[c + 1]; ++j) m = min(m, (uint32_t)ids[j]);
        key[c] = m;
        len[c] = cls_offset[c + 1] - cls_offset[c];
    }
}

__global__ void __launch_bounds__(256)
copy_tuples_by_offset_kernel(const int32_t *perm, int64_t n, const int64_t *src_offset, const int32_t *src,
                             const int64_t *dst_offset, int32_t *dst)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t from = src_offset[perm[k]];
        const int64_t to = dst_offset[k];
        const int64_t len = dst_offset[k + 1] - to;
        for (int64_t j = 0; j < len; ++j) dst[to + j] = src[from + j];
    }
}

inline unsigned blocks_for(int64_t n)
{
    int64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > 256 * 16) b = 256 * 16;
    return (unsigned)b;
}

// ---- hand-written scan and stable radix sort (no library code on the path) -----------------------
// Exclusive prefix sums of n values, three small launches: per-tile sums, one block over the tile
// sums, per-tile scan with the tile's base.  SCAN_TILE values per block; the middle launch handles
// any number of tiles (each of its 1024 lanes walks a run of them).
constexpr int SCAN_TILE = 2048;               // 256 lanes x 8 values

template <class T>
__global__ void __launch_bounds__(256)
scan_tile_sums_kernel(const T *__restrict__ in, int64_t n, T *__restrict__ tile_sums)
{
    __shared__ T s_wave[4];
    const int64_t base = blockIdx.x * (int64_t)SCAN_TILE + threadIdx.x * 8;
    T sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) sum += base + k < n ? in[base + k] : (T)0;
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// tile_sums[i] <- sum of the tiles before i; *total (optional) <- the sum of all
template <class T>
__global__ void __launch_bounds__(1024)
scan_of_sums_kernel(T *tile_sums, int64_t n_tiles, T *total)
{
    __shared__ T s_part[1024];
    const int64_t per = (n_tiles + 1023) / 1024;
    const int64_t first = threadIdx.x * per, last = min(n_tiles, first + per);
    T sum = 0;
    for (int64_t i = first; i < last; ++i) sum += tile_sums[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int step = 1; step < 1024; step <<= 1) {
        const T add = (int)threadIdx.x >= step ? s_part[threadIdx.x - step] : (T)0;
        __syncthreads();
        s_part[threadIdx.x] += add;
        __syncthreads();
    }
    T at = s_part[threadIdx.x] - sum;
    for (int64_t i = first; i < last; ++i) { const T v = tile_sums[i]; tile_sums[i] = at; at += v; }
    if (total && threadIdx.x == 1023) *total = s_part[1023];
}

template <class T>
__global__ void __launch_bounds__(256)
scan_tiles_kernel(const T *__restrict__ in, int64_t n, const T *__restrict__ tile_base, T *__restrict__ out)
{
    __shared__ T s_wave[4];
    const int64_t base = blockIdx.x * (int64_t)SCAN_TILE + threadIdx.x * 8;
    T v[8], sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = base + k < n ? in[base + k] : (T)0; sum += v[k]; }
    T incl = sum;                                  // inclusive scan of the lanes' sums over the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T at = tile_base[blockIdx.x] + incl - sum;
    for (int w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (base + k < n) out[base + k] = at;
        at += v[k];
    }
}

// out[0..n) = exclusive prefix sums of in, `total` (device, optional) = the sum; in == out allowed
template <class T>
int exclusive_scan(Scratch &scratch, const T *in, T *out, int64_t n, T *total)
{
    hipStream_t stream = scratch.stream;
    if (n <= 0) {
        if (total) QB_TRY(hipMemsetAsync(total, 0, sizeof(T), stream));
        return 0;
    }
    const int64_t n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    QB_ALLOC(tile_sums, T, n_tiles);
    hipLaunchKernelGGL(scan_tile_sums_kernel<T>, dim3((unsigned)n_tiles), dim3(256), 0, stream, in, n, tile_sums);
    hipLaunchKernelGGL(scan_of_sums_kernel<T>, dim3(1), dim3(1024), 0, stream, tile_sums, n_tiles, total);
    hipLaunchKernelGGL(scan_tiles_kernel<T>, dim3((unsigned)n_tiles), dim3(256), 0, stream, in, n, tile_sums, out);
    return 0;
}

// exclusive scan of n int64 values into out[0..n) and the total into out[n] (all on the stream)
int exclusive_scan_with_total(Scratch &scratch, const int64_t *in, int64_t *out, int64_t n)
{
    if (n >= (1LL << 40)) return -2;
    return exclusive_scan<int64_t>(scratch, in, out, n, out + n);
}

// Stable least-significant-digit radix sort of (key, value) pairs in whole passes of 9 key bits
// (512 bins), as many as cover end_bit (sort_pairs below says what that orders by): the 18-bit keys
// of the class views take two passes.  A pass: a histogram per
// tile of 4096 pairs (digit-major, so that ONE exclusive scan over it gives every (digit, tile) its
// place), then the scatter -- a tile's four waves each own a quarter of it in order; a wave ranks 64
// pairs at a time with nine ballots (the lanes that share my digit) against its running per-digit
// base in LDS, the pairs are put in digit order in LDS and leave in runs.  Stable by construction:
// tiles, waves, 64-pair chunks and lanes are all taken in input order within a digit.
constexpr int RS_BITS = 9, RS_BINS = 1 << RS_BITS, RS_ITEMS = 16, RS_TILE = 256 * RS_ITEMS;

template <class K>
__global__ void __launch_bounds__(256)
radix_hist_kernel(const K *__restrict__ keys, int64_t n, int shift, uint32_t *__restrict__ hist, int64_t n_tiles)
{
    __shared__ uint32_t h[RS_BINS];
    for (int d = threadIdx.x; d < RS_BINS; d += 256) h[d] = 0;
    __syncthreads();
    const int64_t base = blockIdx.x * (int64_t)RS_TILE;
#pragma unroll 4
    for (int i = 0; i < RS_ITEMS; ++i) {
        const int64_t at = base + i * 256 + threadIdx.x;
        if (at < n) atomicAdd(&h[(uint32_t)((unsigned long long)keys[at] >> shift) & (RS_BINS - 1)], 1u);
    }
    __syncthreads();
    for (int d = threadIdx.x; d < RS_BINS; d += 256) hist[d * n_tiles + blockIdx.x] = h[d];
}

// one block per digit: hist[d][0 .. n_tiles) <- its exclusive prefix sums, digit_total[d] <- its sum
// (the scatter adds the digits before d: 512 totals, scanned by every block for itself)
__global__ void __launch_bounds__(256)
radix_digit_scan_kernel(uint32_t *hist, int64_t n_tiles, uint32_t *digit_total)
{
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_carry;
    uint32_t *row = hist + blockIdx.x * n_tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += 256 * 4) {
        const int64_t at = base + threadIdx.x * 4;
        uint32_t v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = at + k < n_tiles ? row[at + k] : 0u; sum += v[k]; }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t run = s_carry + incl - sum;
        for (int w = 0; w < wave; ++w) run += s_wave[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (at + k < n_tiles) row[at + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (threadIdx.x == 255) s_carry = run;           // (the last lane's running sum = everything so far)
        __syncthreads();
    }
    if (threadIdx.x == 0) digit_total[blockIdx.x] = s_carry;
}

template <class K>
__global__ void __launch_bounds__(256)
radix_scatter_kernel(const K *__restrict__ keys_in, const int32_t *__restrict__ vals_in, K *__restrict__ keys_out,
                     int32_t *__restrict__ vals_out, int64_t n, int shift, const uint32_t *__restrict__ offsets,
                     const uint32_t *__restrict__ digit_total, int64_t n_tiles)
{
    __shared__ uint32_t wave_base[4][RS_BINS];      // a wave's count per digit, then its running place in the tile
    __shared__ uint32_t tile_start[RS_BINS + 1];    // where a digit's pairs start in the tile's digit order
    __shared__ uint32_t s_scan[256];
    __shared__ uint32_t digit_base[RS_BINS];        // pairs of the whole input with a smaller digit
    __shared__ K s_keys[RS_TILE];
    __shared__ int32_t s_vals[RS_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < 4 * RS_BINS; d += 256) (&wave_base[0][0])[d] = 0;
    {   // digit_base = exclusive scan of the 512 digit totals (two digits per lane)
        const uint32_t t0 = digit_total[2 * threadIdx.x], t1 = digit_total[2 * threadIdx.x + 1];
        uint32_t incl = t0 + t1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_scan[wave] = incl;
        __syncthreads();
        uint32_t at = incl - (t0 + t1);
        for (int w = 0; w < wave; ++w) at += s_scan[w];
        digit_base[2 * threadIdx.x] = at;
        digit_base[2 * threadIdx.x + 1] = at + t0;
    }
    __syncthreads();
    // the wave's quarter of the tile, 64 consecutive pairs per chunk
    const int64_t first = blockIdx.x * (int64_t)RS_TILE + wave * (RS_TILE / 4);
    K key[RS_ITEMS];
    int32_t val[RS_ITEMS];
    uint32_t digit[RS_ITEMS];
#pragma unroll
    for (int c = 0; c < RS_ITEMS; ++c) {
        const int64_t at = first + c * 64 + lane;
        const bool valid = at < n;
        key[c] = valid ? keys_in[at] : (K)0;
        val[c] = valid ? vals_in[at] : 0;
        digit[c] = (uint32_t)((unsigned long long)key[c] >> shift) & (RS_BINS - 1);
        if (valid) atomicAdd(&wave_base[wave][digit[c]], 1u);
    }
    __syncthreads();
    // tile_start = exclusive scan over the digits of the tile's counts (two digits per lane)
    const int d0 = 2 * threadIdx.x;
    const uint32_t c0 = wave_base[0][d0] + wave_base[1][d0] + wave_base[2][d0] + wave_base[3][d0];
    const uint32_t c1 = wave_base[0][d0 + 1] + wave_base[1][d0 + 1] + wave_base[2][d0 + 1] + wave_base[3][d0 + 1];
    uint32_t incl = c0 + c1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_scan[wave] = incl;
    __syncthreads();
    uint32_t at0 = incl - (c0 + c1);
    for (int w = 0; w < wave; ++w) at0 += s_scan[w];
    tile_start[d0] = at0;
    tile_start[d0 + 1] = at0 + c0;
    if (threadIdx.x == 255) tile_start[RS_BINS] = at0 + c0 + c1;
    // a wave's running place for a digit: behind the earlier waves' pairs of that digit
    uint32_t run0 = at0, run1 = at0 + c0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t n0 = wave_base[w][d0], n1 = wave_base[w][d0 + 1];
        wave_base[w][d0] = run0; wave_base[w][d0 + 1] = run1;
        run0 += n0; run1 += n1;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < RS_ITEMS; ++c) {
        const bool valid = first + c * 64 + lane < n;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < RS_BITS; ++b) {
            const bool bit = (digit[c] >> b) & 1u;
            const unsigned long long with = __ballot(valid && bit);
            same &= bit ? with : ~with;
        }
        if (valid) {
            const uint32_t before = (uint32_t)__popcll(same & ((1ULL << lane) - 1ULL));
            const uint32_t place = wave_base[wave][digit[c]] + before;
            s_keys[place] = key[c];
            s_vals[place] = val[c];
            if (before == 0) wave_base[wave][digit[c]] += (uint32_t)__popcll(same);      // (the digit's first lane)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk reads the bases this one moved
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    const int64_t tile_first = blockIdx.x * (int64_t)RS_TILE;
    const uint32_t tile_n = (uint32_t)min((int64_t)RS_TILE, n - tile_first);
#pragma unroll 4
    for (int i = 0; i < RS_ITEMS; ++i) {
        const uint32_t j = i * 256 + threadIdx.x;
        if (j >= tile_n) continue;
        const K k = s_keys[j];
        const uint32_t d = (uint32_t)((unsigned long long)k >> shift) & (RS_BINS - 1);
        const int64_t to = (int64_t)digit_base[d] + offsets[d * n_tiles + blockIdx.x] + (j - tile_start[d]);
        keys_out[to] = k;
        vals_out[to] = s_vals[j];
    }
}

// Stable radix sort of (key, value) pairs; the result lands in keys_out / vals_out.  It runs
// max(1, ceil(end_bit / 9)) WHOLE 9-bit passes, so the pairs come out ordered by
// key & (2^(9 passes) - 1), or by the whole key where K is no wider than that -- NOT by the bits
// below end_bit alone: key bits in [end_bit, 9 passes) take part.  Bits above are ignored, and the full
// keys are carried.  localize relies on this: it sorts with end_bit = the bits of n_tx - 1 and gives
// an empty class the key 0xffffffff, all ones in every whole pass (no transcript id is above that),
// so that these classes come out last.  A caller that wants bits [0, end_bit) alone keeps its keys
// below 2^end_bit, as all the others do.
// (tests/test_gpu_scan_sort.py pins this against tests/sort_scan_reference.py)
template <class K>
int sort_pairs(Scratch &scratch, const K *keys_in, K *keys_out, const int32_t *vals_in, int32_t *vals_out,
               int64_t n, int end_bit)
{
    hipStream_t stream = scratch.stream;
    if (n <= 0) return 0;
    if (n >= (1LL << 32)) return -2;                                  // (offsets are 32-bit)
    const int passes = std::max(1, (end_bit + RS_BITS - 1) / RS_BITS);
    const int64_t n_tiles = (n + RS_TILE - 1) / RS_TILE;
    QB_ALLOC(hist, uint32_t, RS_BINS * n_tiles);
    QB_ALLOC(digit_total, uint32_t, RS_BINS);
    K *tmp_keys = nullptr;
    int32_t *tmp_vals = nullptr;
    if (passes > 1) {
        QB_ALLOC(tk, K, n); QB_ALLOC(tv, int32_t, n);
        tmp_keys = tk; tmp_vals = tv;
    }
    const K *src_k = keys_in;
    const int32_t *src_v = vals_in;
    for (int pass = 0; pass < passes; ++pass) {
        // (the last pass writes the caller's arrays; the passes before it alternate so that it can)
        const bool to_out = ((passes - 1 - pass) & 1) == 0;
        K *dst_k = to_out ? keys_out : tmp_keys;
        int32_t *dst_v = to_out ? vals_out : tmp_vals;
        const int shift = pass * RS_BITS;
        hipLaunchKernelGGL(radix_hist_kernel<K>, dim3((unsigned)n_tiles), dim3(256), 0, stream, src_k, n, shift, hist, n_tiles);
        hipLaunchKernelGGL(radix_digit_scan_kernel, dim3(RS_BINS), dim3(256), 0, stream, hist, n_tiles, digit_total);
        hipLaunchKernelGGL(radix_scatter_kernel<K>, dim3((unsigned)n_tiles), dim3(256), 0, stream, src_k, src_v, dst_k, dst_v, n,
                           shift, hist, digit_total, n_tiles);
        src_k = dst_k;
        src_v = dst_v;
    }
    return 0;
}

}  // namespace

// the sort above for callers outside this file (skm_barcodes.hip); the stream has drained on return
int sort_pairs_u32(const uint32_t *keys_in, uint32_t *keys_out, const int32_t *vals_in, int32_t *vals_out, int64_t n,
                   int end_bit, hipStream_t stream)
{
    Scratch scratch(stream);
    return sort_pairs<uint32_t>(scratch, keys_in, keys_out, vals_in, vals_out, n, end_bit);
}

// the other two instantiations in use and the scan, as they stand, for the diagnostic entry points
// (skm_device_sort_probe, skm_device_scan_probe: tests); the stream has drained on return
int sort_pairs_u64(const unsigned long long *keys_in, unsigned long long *keys_out, const int32_t *vals_in,
                   int32_t *vals_out, int64_t n, int end_bit, hipStream_t stream)
{
    Scratch scratch(stream);
    return sort_pairs<unsigned long long>(scratch, keys_in, keys_out, vals_in, vals_out, n, end_bit);
}

int sort_pairs_i32(const int32_t *keys_in, int32_t *keys_out, const int32_t *vals_in, int32_t *vals_out, int64_t n,
                   int end_bit, hipStream_t stream)
{
    Scratch scratch(stream);
    return sort_pairs<int32_t>(scratch, keys_in, keys_out, vals_in, vals_out, n, end_bit);
}

int exclusive_scan_total_i64(const int64_t *in, int64_t *out, int64_t n, hipStream_t stream)
{
    Scratch scratch(stream);
    return exclusive_scan_with_total(scratch, in, out, n);
}

int64_t quant_rows_upper_bound(int64_t n_tx, int64_t n_ids)
{
    return n_tx + n_ids / EM_ROW_CAP + 1;
}

namespace {

int build_from_table(Scratch &scratch, const ClassTable &t, QuantBuild &q)
{
    hipStream_t stream = scratch.stream;
    const int64_t n_classes = q.n_classes;
    if (n_classes == 0) {
        QB_TRY(hipMemsetAsync(q.cls_offset, 0, sizeof(int64_t), stream));
        return 0;
    }
    if (n_classes >= (1LL << 31) || q.n_ids >= (1LL << 31)) return -2;
    QB_ALLOC(arena_off, int64_t, n_classes); QB_ALLOC(len, int64_t, n_classes);
    QB_ALLOC(len_sorted, int64_t, n_classes); QB_ALLOC(count, double, n_classes);
    QB_ALLOC(first, unsigned long long, n_classes); QB_ALLOC(first_sorted, unsigned long long, n_classes);
    QB_ALLOC(iota, int32_t, n_classes); QB_ALLOC(perm, int32_t, n_classes);
    hipLaunchKernelGGL(table_dump_kernel, dim3(blocks_for(n_classes)), dim3(256), 0, stream,
                       t, n_classes, arena_off, len, count, first, (uint32_t *)nullptr, (uint64_t)0, (uint32_t *)nullptr,
                       (unsigned int *)nullptr);
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(n_classes)), dim3(256), 0, stream, iota, n_classes);
    int first_bits = 64;
    if (q.first_seen_bound > 0) {
        first_bits = 1;
        while (first_bits < 63 && (1LL << first_bits) <= q.first_seen_bound) ++first_bits;
    }
    if (sort_pairs(scratch, first, first_sorted, iota, perm, n_classes, first_bits)) return -1;
    hipLaunchKernelGGL(gather_classes_kernel, dim3(blocks_for(n_classes)), dim3(256), 0, stream, perm,
                       n_classes, len, count, len_sorted, q.cls_count);
    if (exclusive_scan_with_total(scratch, len_sorted, q.cls_offset, n_classes)) return -1;
    hipLaunchKernelGGL(copy_tuples_kernel, dim3(blocks_for(n_classes)), dim3(256), 0, stream, perm,
                       n_classes, arena_off, t.arena, q.cls_offset, q.ids);
    return 0;
}

// The same result as build_from_table + localize (classes by smallest transcript id, then by
// first-seen; perm[j] = first-seen rank of internal class j) with one sort instead of two and one
// copy of the tuples instead of two: the first-seen rank is a prefix popcount over a bitmap of
// the unit indices.  *shared_first_seen (a word of the scratch, on the device; nullptr: no class)
// != 0 once the stream has come this far: two classes share a first-seen value or one lies outside
// the bound, nothing usable was written and the caller falls back to the sorting path.
constexpr int64_t RANK_BITMAP_MAX_UNITS = 1LL << 31;      // 256 MiB of bits + 4 GiB of word sums at most

int build_from_table_ranked(Scratch &scratch, const ClassTable &t, QuantBuild &q, int32_t *perm,
                            const unsigned int **shared_first_seen)
{
    hipStream_t stream = scratch.stream;
    const int64_t C = q.n_classes;
    if (C == 0) {
        QB_TRY(hipMemsetAsync(q.cls_offset, 0, sizeof(int64_t), stream));
        return 0;
    }
    if (C >= (1LL << 31) || q.n_ids >= (1LL << 31)) return -2;
    const uint64_t bound = (uint64_t)q.first_seen_bound;
    const int64_t n_words = (int64_t)((bound + 31) / 32);
    QB_ALLOC(arena_off, int64_t, C); QB_ALLOC(len, int64_t, C); QB_ALLOC(count, double, C);
    QB_ALLOC(first, unsigned long long, C); QB_ALLOC(min_id, uint32_t, C);
    QB_ALLOC(bits, uint32_t, n_words); QB_ALLOC(duplicate, unsigned int, 1);
    QB_TRY(hipMemsetAsync(bits, 0, n_words * sizeof(uint32_t), stream));
    QB_TRY(hipMemsetAsync(duplicate, 0, sizeof(unsigned int), stream));
    hipLaunchKernelGGL(table_dump_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, t, C, arena_off, len, count,
                       first, min_id, bound, bits, duplicate);
    // (the host reads the flag when the whole set-up has been queued, with the copies the end of the set-up
    // waits for anyway: a table that raises it has run the rest for nothing -- first_seen_rank_kernel keeps
    // its writes within the arrays whatever the bitmap holds, gather_by_rank_kernel leaves every class
    // empty -- and goes through the sorting path then)
    *shared_first_seen = duplicate;
    QB_ALLOC(word_count, int64_t, n_words); QB_ALLOC(word_base, int64_t, n_words + 1);
    QB_ALLOC(by_rank, int32_t, C); QB_ALLOC(key_by_rank, uint32_t, C); QB_ALLOC(key_sorted, uint32_t, C);
    QB_ALLOC(iota, int32_t, C); QB_ALLOC(len_sorted, int64_t, C); QB_ALLOC(src_off, int64_t, C);
    hipLaunchKernelGGL(word_popcount_kernel, dim3(blocks_for(n_words)), dim3(256), 0, stream, bits, n_words,
                       word_count);
    if (exclusive_scan_with_total(scratch, word_count, word_base, n_words)) return -1;
    hipLaunchKernelGGL(first_seen_rank_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, first, min_id, C, bound,
                       bits, word_base, by_rank, key_by_rank);
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, iota, C);
    int end_bit = 1;
    while ((1LL << end_bit) < q.n_tx && end_bit < 32) ++end_bit;
    if (sort_pairs(scratch, key_by_rank, key_sorted, iota, perm, C, end_bit)) return -1;
    hipLaunchKernelGGL(gather_by_rank_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, perm, by_rank, C, len,
                       count, arena_off, len_sorted, q.cls_count, src_off, duplicate);
    if (exclusive_scan_with_total(scratch, len_sorted, q.cls_offset, C)) return -1;
    hipLaunchKernelGGL(copy_tuples_direct_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, C, src_off, t.arena,
                       q.cls_offset, q.ids);
    return 0;
}

// Reorder the classes (stably) by their smallest transcript id.  The EM result
// does not depend on class order beyond floating-point association, but the
// transcript-major pass gathers inner[c] over a transcript's classes, and
// classes that share transcripts then sit in neighbouring cache sectors
// instead of being spread over the whole first-seen order.  perm[k] = index of
// internal class k in the caller's order.
int localize(Scratch &scratch, QuantBuild &q, int32_t *perm)
{
    hipStream_t stream = scratch.stream;
    const int64_t C = q.n_classes, M = q.n_ids;
    if (C == 0) return 0;
    if (C >= (1LL << 31) || M >= (1LL << 31)) return -2;
    QB_ALLOC(key, uint32_t, C); QB_ALLOC(key_sorted, uint32_t, C); QB_ALLOC(iota, int32_t, C);
    QB_ALLOC(ids_copy, int32_t, M); QB_ALLOC(len, int64_t, C); QB_ALLOC(len_sorted, int64_t, C);
    QB_ALLOC(old_offset, int64_t, C + 1); QB_ALLOC(count_copy, double, C);
    hipLaunchKernelGGL(class_min_id_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_offset, q.ids, C,
                       key, len);
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, iota, C);
    int end_bit = 1;
    while ((1LL << end_bit) < q.n_tx && end_bit < 32) ++end_bit;
    if (sort_pairs(scratch, key, key_sorted, iota, perm, C, end_bit)) return -1;
    QB_TRY(hipMemcpyAsync(old_offset, q.cls_offset, (C + 1) * 8, hipMemcpyDeviceToDevice, stream));
    QB_TRY(hipMemcpyAsync(ids_copy, q.ids, M * 4, hipMemcpyDeviceToDevice, stream));
    QB_TRY(hipMemcpyAsync(count_copy, q.cls_count, C * 8, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(gather_classes_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, perm, C, len,
                       count_copy, len_sorted, q.cls_count);
    if (exclusive_scan_with_total(scratch, len_sorted, q.cls_offset, C)) return -1;
    hipLaunchKernelGGL(copy_tuples_by_offset_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, perm, C,
                       old_offset, ids_copy, q.cls_offset, q.ids);
    return 0;
}

// The transcript-major view of the whole table and its rows (quant_rows_build): one stable sort of the
// pairs by transcript, then the rows of at most EM_ROW_CAP pairs.
int transpose(Scratch &scratch, const QuantBuild &q, const QuantRows &rows_out)
{
    hipStream_t stream = scratch.stream;
    const int64_t C = q.n_classes, M = q.n_ids, T = q.n_tx;
    if (M >= (1LL << 31) || C >= (1LL << 31)) return -2;
    QB_ALLOC(pair_cls, int32_t, M); QB_ALLOC(sorted_tx, int32_t, M);
    QB_ALLOC(tx_offset, int64_t, T + 1); QB_ALLOC(rows, int64_t, T);
    if (M > 0) {
        hipLaunchKernelGGL(pair_class_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_offset, C,
                           pair_cls);
        int end_bit = 1;
        while ((1LL << end_bit) < T && end_bit < 31) ++end_bit;
        if (sort_pairs(scratch, (const int32_t *)q.ids, sorted_tx, (const int32_t *)pair_cls, rows_out.tx_cls, M, end_bit)) return -1;
    }
    hipLaunchKernelGGL(segment_starts_kernel, dim3(blocks_for(M + 1)), dim3(256), 0, stream, sorted_tx, M,
                       T, tx_offset);
    hipLaunchKernelGGL(row_count_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, tx_offset, T, rows);
    if (exclusive_scan_with_total(scratch, rows, rows_out.tx_row, T)) return -1;
    // rows <= T + M / EM_ROW_CAP, which is what row_start / row_tx were sized for
    hipLaunchKernelGGL(row_fill_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, tx_offset, rows_out.tx_row, T,
                       M, rows_out.row_start, rows_out.row_tx);
    return 0;
}

// ---- connected components of the (class, transcript) graph and their tiles (EmTiles, skm_kernels.h)
// Union-find over the transcripts with the smaller id as the parent, so that a component's root -- its
// label -- is its smallest transcript id whatever the order of the hooks.  A hook is one compare-and-swap
// on a ROOT (a word that still points to itself); the walks read with plain loads: what they may miss
// of another workgroup's hooks only costs a failed swap, which returns the current parent.
__device__ __forceinline__ int32_t cc_root(const int32_t *parent, int32_t v)
{
    int32_t p;
    while ((p = parent[v]) != v) v = p;
    return v;
}

// The same walk while the hooks are being made, halving the path it walks: a node two or more steps
// from the top is re-pointed to its grandparent with an atomic minimum.  Parents only ever get smaller
// and only ever name an ancestor, so the minimum keeps both; it never touches a root (a root has no
// grandparent), so the hooks' compare-and-swap still sees every root as it is.  Without it a table whose
// classes form one long chain walked O(transcripts) per hook.
__device__ __forceinline__ int32_t cc_root_halving(int32_t *parent, int32_t v, int32_t p)
{
    while (p != v) {
        const int32_t g = parent[p];
        if (g != p) atomicMin(&parent[v], g);
        v = p;
        p = g;
    }
    return v;
}
__device__ __forceinline__ int32_t cc_root_halving(int32_t *parent, int32_t v) { return cc_root_halving(parent, v, parent[v]); }

// The walk of cc_hook_kernel: its first CC_PLAIN_STEPS steps are plain loads, and only a walk that is longer goes
// on halving its path.  On a table of many small components nearly every walk ends within the plain steps, and the
// halving atomics, which such a table never needs, were a third of the kernel (profiles/rows_on_demand_ab.log); a
// long chain is halved as before from the step on.  cc_label_kernel, which walks every transcript once more,
// halves from the first step.
constexpr int CC_PLAIN_STEPS = 8;
__device__ __forceinline__ int32_t cc_root_hook(int32_t *parent, int32_t v, int32_t p)
{
    for (int step = 0; step < CC_PLAIN_STEPS; ++step) {
        if (p == v) return v;
        v = p;
        p = parent[v];
    }
    return cc_root_halving(parent, v, p);
}

// (one lane per class; several lanes per class put more swaps in flight on the same few roots and were
// slower: DESIGN.md, "The EM of independent components")
__global__ void __launch_bounds__(256)
cc_hook_kernel(const int64_t *cls_offset, const int32_t *ids, int64_t n_classes, int32_t *parent)
{
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_classes;
         c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t begin = cls_offset[c], end = cls_offset[c + 1];
        if (begin == end) continue;
        const int32_t v0 = ids[begin];
        int32_t b = cc_root_hook(parent, v0, parent[v0]);
        for (int64_t j = begin + 1; j < end; ++j) {
            const int32_t v = ids[j];
            int32_t a = cc_root_hook(parent, v, parent[v]);
            while (a != b) {                        // (a or b gets smaller every turn)
                if (a < b) { const int32_t s = a; a = b; b = s; }
                const int32_t old = atomicCAS(&parent[a], a, b);
                if (old == a) break;
                a = cc_root_hook(parent, old, parent[old]);
            }
            b = a < b ? a : b;
        }
    }
}

// label of every transcript; comp[3 r .. 3 r + 2] of root r: transcripts (pairs, classes: cc_classes_kernel).
// The walks go on halving the paths (a chain of classes hooked root to root leaves paths as long as the
// chain), and a wave adds once per root it meets, not once per transcript: on a table that is one
// component every transcript would otherwise add to the same word.
__global__ void __launch_bounds__(256)
cc_label_kernel(int32_t *parent, int64_t n_tx, int32_t *label, int32_t *comp)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane; t0 < n_tx; t0 += stride) {
        const int64_t t = t0 + lane;
        int32_t r = -1;
        if (t < n_tx) {
            r = cc_root_halving(parent, (int32_t)t);
            label[t] = r;
        }
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {                              // (wave-uniform: one turn per distinct root among the lanes)
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t r0 = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(r == r0);
            if (lane == leader) atomicAdd(&comp[3 * (int64_t)r0], (int)__popcll(same));
            todo &= ~same;
        }
    }
}

// comp[3 r + 1], comp[3 r + 2] of root r: the pairs and the classes of its component, both from the classes:
// a component's pairs are the lengths of its classes (a transcript a class names twice is two pairs).
// (a class without transcripts belongs nowhere; it is counted, and later listed, with transcript 0)
__global__ void __launch_bounds__(256)
cc_classes_kernel(const int64_t *cls_offset, const int32_t *ids, int64_t n_classes, const int32_t *label,
                  int32_t *comp)
{
    // (classes are kept by smallest transcript id, so neighbouring lanes mostly name one component: a run
    // of lanes with the same root adds its length and the pairs of its classes once -- a table that is one
    // component adds once per wave, not once per class)
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane; c0 < n_classes; c0 += stride) {
        const int64_t c = c0 + lane;
        int32_t r = -1, pairs = 0;
        if (c < n_classes) {
            const int64_t begin = cls_offset[c], end = cls_offset[c + 1];
            r = label[begin < end ? ids[begin] : 0];
            pairs = (int32_t)(end - begin);
        }
        int32_t incl = pairs;                       // inclusive prefix sums of the lengths over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int32_t before = __shfl_up(r, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || before != r);
        const unsigned long long later = lane == 63 ? 0ULL : heads >> (lane + 1);
        const int run = later ? __ffsll((long long)later) : 64 - lane;      // (to the next head: a head's run)
        const int32_t through = __shfl(incl, lane + run - 1, 64);           // the sums up to my run's last lane
        if (r >= 0 && ((heads >> lane) & 1ULL)) {
            atomicAdd(&comp[3 * (int64_t)r + 2], run);
            if (through - incl + pairs) atomicAdd(&comp[3 * (int64_t)r + 1], through - incl + pairs);
        }
    }
}

// One wave per run of EM_TILE_SEGMENT transcript ids: the components rooted there, in label order, go
// into the run's tiles one after the other, a new tile whenever the next component would exceed a
// capacity.  root_tile[r] = tile within the run, -1: not a root, -2: above the capacity by itself.
// Components are disjoint, so a tile's three fills are sums of its components' sizes: the wave takes 64
// ids at a time, forms the inclusive prefix sums of the sizes over its lanes (a component that goes into
// no tile counts as 0) and finds the open tile's end with a ballot -- the first lane whose prefix sum,
// less the sum at the tile's start, is above a capacity opens the next tile.  One turn of that loop per
// tile; the fill of the tile left open is carried to the next 64 ids.
// The walk runs twice.  STARTS = false leaves root_tile, the components above the capacity and per run
// seg_sizes[0 .. 3][run] = its tiles and the transcripts, classes and pairs that went into them.  After
// one scan over those (seg_scan_kernel: seg_base[k][run]) STARTS = true walks the same runs and writes,
// where a tile opens, what lies before it: tile_tx / tile_cls / tile_pair[seg_base[0][run] + tile of the
// run] = the run's base + the packed sizes before the component that opens it.  Nothing else differs.
template <bool STARTS>
__global__ void __launch_bounds__(256)
tile_pack_kernel(const int32_t *__restrict__ comp, int64_t n_tx, int64_t n_segments, int32_t *__restrict__ root_tile,
                 int64_t *__restrict__ seg_sizes, unsigned long long *__restrict__ oversize,
                 const int64_t *__restrict__ seg_base, int64_t *__restrict__ tile_tx, int64_t *__restrict__ tile_cls,
                 int64_t *__restrict__ tile_pair)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t g = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; g < n_segments; g += n_waves) {
        int tx = 0, pairs = 0, classes = 0, n = 0;          // (wave-uniform: the open tile's fill, the run's tiles)
        int run_tx = 0, run_pairs = 0, run_classes = 0;     // (wave-uniform: packed before these 64 ids)
        int64_t first_tile = 0, first_tx = 0, first_cls = 0, first_pair = 0;
        if (STARTS) {
            first_tile = seg_base[g]; first_tx = seg_base[(n_segments + 1) + g];
            first_cls = seg_base[2 * (n_segments + 1) + g]; first_pair = seg_base[3 * (n_segments + 1) + g];
        }
        const int64_t last = min(n_tx, (g + 1) * EM_TILE_SEGMENT);
        for (int64_t t0 = g * EM_TILE_SEGMENT; t0 < last; t0 += 64) {
            const int64_t t = t0 + lane;
            int c_tx = 0, c_pairs = 0, c_classes = 0;
            if (t < last) { c_tx = comp[3 * t]; c_pairs = comp[3 * t + 1]; c_classes = comp[3 * t + 2]; }
            const bool root = c_tx > 0;
            const bool big = c_tx > EM_TILE_TX || c_pairs > EM_TILE_PAIRS || c_classes > EM_TILE_CLASSES;
            const bool packed = root && !big;
            if (!packed) c_tx = c_pairs = c_classes = 0;
            int s_tx = c_tx, s_pairs = c_pairs, s_classes = c_classes;
            for (int d = 1; d < 64; d <<= 1) {
                const int a = __shfl_up(s_tx, d, 64), b = __shfl_up(s_pairs, d, 64), c = __shfl_up(s_classes, d, 64);
                if (lane >= d) { s_tx += a; s_pairs += b; s_classes += c; }
            }
            // (the prefix sums at the open tile's start: what the tile held before these 64 ids lies before lane 0)
            int base_tx = -tx, base_pairs = -pairs, base_classes = -classes, opened = 0;   // opened: tiles begun up to this lane
            const int before = n;
            unsigned long long behind = ~0ULL;                  // the lanes behind the last tile start
            for (;;) {
                const bool over = packed && (n == 0 || s_tx - base_tx > EM_TILE_TX || s_pairs - base_pairs > EM_TILE_PAIRS ||
                                             s_classes - base_classes > EM_TILE_CLASSES);
                const unsigned long long starts = __ballot(over) & behind;
                if (!starts) break;
                const int at = __ffsll((long long)starts) - 1;
                base_tx = __shfl(s_tx - c_tx, at, 64);
                base_pairs = __shfl(s_pairs - c_pairs, at, 64);
                base_classes = __shfl(s_classes - c_classes, at, 64);
                if (STARTS && lane == 0) {
                    tile_tx[first_tile + n] = first_tx + run_tx + base_tx;
                    tile_cls[first_tile + n] = first_cls + run_classes + base_classes;
                    tile_pair[first_tile + n] = first_pair + run_pairs + base_pairs;
                }
                ++n;
                if (lane >= at) ++opened;
                behind = at == 63 ? 0ULL : ~0ULL << (at + 1);   // (the component at the start fits by itself)
            }
            if (!STARTS) {
                if (t < last) root_tile[t] = !root ? -1 : big ? -2 : before + opened - 1;
                const unsigned long long bigs = __ballot(root && big);
                if (bigs && lane == 0) atomicAdd(oversize, (unsigned long long)__popcll(bigs));
            }
            const int all_tx = __shfl(s_tx, 63, 64), all_pairs = __shfl(s_pairs, 63, 64), all_classes = __shfl(s_classes, 63, 64);
            tx = all_tx - base_tx;
            pairs = all_pairs - base_pairs;
            classes = all_classes - base_classes;
            run_tx += all_tx; run_pairs += all_pairs; run_classes += all_classes;
        }
        if (!STARTS && lane == 0) {
            seg_sizes[g] = n;
            seg_sizes[n_segments + g] = run_tx;
            seg_sizes[2 * n_segments + g] = run_classes;
            seg_sizes[3 * n_segments + g] = run_pairs;
        }
    }
}

// seg_base[k][0 .. n_segments] = the exclusive prefix sums of seg_sizes[k][0 .. n_segments) and their total, k = 0:
// tiles, 1: transcripts, 2: classes, 3: pairs of the tiles, by ONE workgroup (a few hundred runs; each lane walks a
// stretch of them, so any number is handled).  It also writes the end entries that em_local_chunk_kernel and
// tile_order_kernel read behind the last tile: tile_tx / tile_cls / tile_pair[tiles] and the pair total at the place
// behind the last listed transcript and class.
__global__ void __launch_bounds__(1024)
seg_scan_kernel(const int64_t *__restrict__ seg_sizes, int64_t n_segments, int64_t *__restrict__ seg_base,
                int64_t *__restrict__ tile_tx, int64_t *__restrict__ tile_cls, int64_t *__restrict__ tile_pair,
                int64_t *__restrict__ tx_pair, int64_t *__restrict__ cls_pair)
{
    __shared__ int64_t s_part[4][1024];
    const int64_t per = (n_segments + 1023) / 1024;
    const int64_t first = min(n_segments, threadIdx.x * per), last = min(n_segments, first + per);
    int64_t sum[4];
    for (int k = 0; k < 4; ++k) {
        sum[k] = 0;
        for (int64_t i = first; i < last; ++i) sum[k] += seg_sizes[k * n_segments + i];
        s_part[k][threadIdx.x] = sum[k];
    }
    __syncthreads();
    for (int step = 1; step < 1024; step <<= 1) {
        int64_t add[4];
        for (int k = 0; k < 4; ++k) add[k] = (int)threadIdx.x >= step ? s_part[k][threadIdx.x - step] : 0;
        __syncthreads();
        for (int k = 0; k < 4; ++k) s_part[k][threadIdx.x] += add[k];
        __syncthreads();
    }
    for (int k = 0; k < 4; ++k) {
        int64_t at = s_part[k][threadIdx.x] - sum[k];
        for (int64_t i = first; i < last; ++i) { seg_base[k * (n_segments + 1) + i] = at; at += seg_sizes[k * n_segments + i]; }
    }
    if (threadIdx.x == 1023) {
        const int64_t tiles = s_part[0][1023], txs = s_part[1][1023], classes = s_part[2][1023], pairs = s_part[3][1023];
        seg_base[n_segments] = tiles; seg_base[2 * n_segments + 1] = txs;
        seg_base[3 * n_segments + 2] = classes; seg_base[4 * n_segments + 3] = pairs;
        tile_tx[tiles] = txs; tile_cls[tiles] = classes; tile_pair[tiles] = pairs;
        tx_pair[txs] = pairs; cls_pair[classes] = pairs;
    }
}

// ---- a tile's members: dropped into the tile's places in any order, then put in order by the tile's workgroup
// The lanes of a wave hold consecutive items; a run of neighbouring lanes that name the same tile draws its places
// with ONE returning add on the tile's cursor (tile < 0: the lane places nothing).  Returns the lane's place in its
// tile.  Called by whole waves.
__device__ __forceinline__ int32_t tile_draw_place(int32_t tile, int32_t *cursor, int lane)
{
    const int32_t before = __shfl_up(tile, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || before != tile);
    const int head = 63 - __clzll((long long)(heads & ((2ULL << lane) - 1ULL)));     // (the start of my run)
    int32_t base = 0;
    if (tile >= 0 && head == lane) {
        const unsigned long long later = lane == 63 ? 0ULL : heads >> (lane + 1);
        const int run = later ? __ffsll((long long)later) : 64 - lane;
        base = atomicAdd(&cursor[tile], run);
    }
    return __shfl(base, head, 64) + (lane - head);
}

// tile of every transcript (n_tx: a component above the capacity -- in no tile), and its place, not yet in
// order, among the tile's transcripts in tx_list
__global__ void __launch_bounds__(256)
tx_place_kernel(const int32_t *__restrict__ label, const int32_t *__restrict__ root_tile, const int64_t *__restrict__ seg_base,
                int64_t n_tx, const int64_t *__restrict__ tile_tx, int32_t *__restrict__ cursor, int32_t *__restrict__ tx_tile,
                int32_t *__restrict__ tx_list)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane; t0 < n_tx; t0 += stride) {
        const int64_t t = t0 + lane;
        int32_t tile = -1;
        if (t < n_tx) {
            const int32_t r = label[t], at = root_tile[r];
            tile = at < 0 ? -1 : (int32_t)(seg_base[r / EM_TILE_SEGMENT] + at);
            tx_tile[t] = tile < 0 ? (int32_t)n_tx : tile;
        }
        const int32_t place = tile_draw_place(tile, cursor, lane);
        if (tile >= 0) {
            const int64_t to = tile_tx[tile] + place;
            if (to >= 0 && to < n_tx) tx_list[to] = (int32_t)t;           // (always: a tile's transcripts are those counted into it)
        }
    }
}

// the same for the classes: a class lies in the tile of its first transcript (one without transcripts: of
// transcript 0, as cc_classes_kernel counted it)
__global__ void __launch_bounds__(256)
cls_place_kernel(const int64_t *__restrict__ cls_offset, const int32_t *__restrict__ ids, int64_t n_classes, int64_t n_tx,
                 const int32_t *__restrict__ tx_tile, const int64_t *__restrict__ tile_cls, int32_t *__restrict__ cursor,
                 int32_t *__restrict__ cls_tile, int32_t *__restrict__ cls_list)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane; c0 < n_classes; c0 += stride) {
        const int64_t c = c0 + lane;
        int32_t tile = -1;
        if (c < n_classes) {
            const int64_t begin = cls_offset[c];
            tile = tx_tile[begin < cls_offset[c + 1] ? ids[begin] : 0];
            cls_tile[c] = tile;
            if (tile == (int32_t)n_tx) tile = -1;
        }
        const int32_t place = tile_draw_place(tile, cursor, lane);
        if (tile >= 0) {
            const int64_t to = tile_cls[tile] + place;
            if (to >= 0 && to < n_classes) cls_list[to] = (int32_t)c;
        }
    }
}

// (tuning aid, scripts/build_variant.sh: 0 lists a tile's classes by ascending index alone, as before the
// class phase took its tuples in batches; the EM's results are the same either way)
#ifndef SKM_EM_CLASS_ORDER
#define SKM_EM_CLASS_ORDER 1
#endif

// Exclusive prefix sums, in place, of s_off[0 .. n) with their total in s_off[n], by the tile's workgroup of 256
// lanes in LDS (n <= CAP).  Ends with a barrier.
template <int CAP>
__device__ __forceinline__ void tile_scan(int n, int32_t *s_off, int32_t *s_wave)
{
    constexpr int PER = CAP / 256 + 1;                // (256 PER > CAP: the scan reaches entry n)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t v[PER], sum = 0;
#pragma unroll
    for (int p = 0; p < PER; ++p) { const int e = tid * PER + p; v[p] = e < n ? s_off[e] : 0; sum += v[p]; }
    int32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int32_t at = incl - sum;
    for (int w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        const int e = tid * PER + p;
        if (e <= n) s_off[e] = at;
        at += v[p];
    }
    __syncthreads();
}

// The order of a tile's transcripts and the prefix sums of their pairs, by the tile's workgroup of 256 lanes in LDS.
// In: n <= 256 members in any order, s_item[i] with the DISTINCT key s_key[i] and s_off[i] pairs; s_key has room for
// two words behind the keys.  Out: s_item in ascending order of the keys, s_off[0 .. n] the exclusive prefix sums of
// the pairs in that order and their total, s_place[i] = the place of the member that stood at i.
// A member's place is the number of keys below its own: the lanes read the keys two at a time, all the same words.
template <int CAP>
__device__ __forceinline__ void tile_rank_and_scan(int n, unsigned long long *s_key, int32_t *s_item, int32_t *s_off,
                                                   int32_t *s_wave, uint16_t *s_place)
{
    static_assert(CAP <= 256, "one member a lane");
    const int tid = threadIdx.x;
    const bool mine = tid < n;
    if (tid < 2) s_key[n + tid] = ~0ULL;              // (behind the keys: below no key)
    __syncthreads();
    const unsigned long long key = mine ? s_key[tid] : 0ULL;
    const int32_t item = mine ? s_item[tid] : 0, len = mine ? s_off[tid] : 0;
    int32_t rank = 0;
    for (int j = 0; j < n; j += 2) {
        const unsigned long long a = s_key[j], b = s_key[j + 1];
        rank += (a < key ? 1 : 0) + (b < key ? 1 : 0);
    }
    __syncthreads();
    if (mine && rank < n) { s_item[rank] = item; s_off[rank] = len; s_place[tid] = (uint16_t)rank; }
    __syncthreads();
    tile_scan<CAP>(n, s_off, s_wave);
}

// the largest k in [0, n) with s_off[k] <= p, for prefix sums with s_off[0] <= p < s_off[n]: the member that holds
// pair p (members without pairs repeat an entry and are passed over)
__device__ __forceinline__ int tile_find(const int32_t *s_off, int n, int p)
{
    int k = 0, above = n;
    while (above - k > 1) {
        const int mid = (k + above) >> 1;
        if (s_off[mid] <= p) k = mid; else above = mid;
    }
    return k;
}

// A stable counting sort of n <= 256 PER items by a key of KEY_BITS bits, by the tile's workgroup: the four waves
// own a quarter of the items each, in order; a wave counts its keys (s_hist[wave][key]), then -- with base(key),
// the place of the key's first item -- takes 64 items at a time and ranks the lanes that share a key by ballot
// against the wave's running place for the key, as radix_scatter_kernel does.  emit(item, place).
// tile_sort_count ends with a barrier, after which the caller may form what base() reads and calls tile_sort_place
// behind a barrier of its own; tile_sort_place ends with a barrier.
template <int KEY_BITS, class Key>
__device__ __forceinline__ void tile_sort_count(int n, Key key, uint32_t *s_hist)
{
    constexpr int KEYS = 1 << KEY_BITS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int d = tid; d < 4 * KEYS; d += 256) s_hist[d] = 0;
    __syncthreads();
    const int per = ((n + 255) >> 8) << 6, first = wave * per;
    for (int c0 = 0; c0 < per; c0 += 64) {
        const int p = first + c0 + lane;
        if (p < n) atomicAdd(&s_hist[wave * KEYS + (key(p) & (KEYS - 1))], 1u);
    }
    __syncthreads();
}

template <int KEY_BITS, class Key, class Base, class Emit>
__device__ __forceinline__ void tile_sort_place(int n, Key key, Base base, uint32_t *s_hist, Emit emit)
{
    constexpr int KEYS = 1 << KEY_BITS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int d = tid; d < KEYS; d += 256) {           // a wave's running place: behind the earlier waves' items of the key
        uint32_t run = base(d);
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t m = s_hist[w * KEYS + d]; s_hist[w * KEYS + d] = run; run += m; }
    }
    __syncthreads();
    const int per = ((n + 255) >> 8) << 6, first = wave * per;
    for (int c0 = 0; c0 < per; c0 += 64) {            // (wave-uniform)
        const int p = first + c0 + lane;
        const bool valid = p < n;
        const uint32_t k = valid ? (key(p) & (KEYS - 1)) : 0u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < KEY_BITS; ++b) {
            const bool bit = (k >> b) & 1u;
            const unsigned long long with = __ballot(valid && bit);
            same &= bit ? with : ~with;
        }
        if (valid) {
            const uint32_t before = (uint32_t)__popcll(same & ((1ULL << lane) - 1ULL));
            emit(p, s_hist[wave * KEYS + k] + before);
            if (before == 0) s_hist[wave * KEYS + k] += (uint32_t)__popcll(same);       // (the key's first lane)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk reads the places this one moved
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
}

// a pair of the tile while it is being moved to the transcript-major view: its transcript's place in the tile's
// list above its class's place (16 bits hold both at the capacities in use)
constexpr int bits_for(int n) { int b = 0; while ((1 << b) < n) ++b; return b; }      // the bits that hold 0 .. n - 1
constexpr int TILE_TX_BITS = bits_for(EM_TILE_TX), TILE_CLS_BITS = bits_for(EM_TILE_CLASSES);
static_assert(TILE_TX_BITS + TILE_CLS_BITS <= 32, "a tile's pair (transcript's place, class's place) is one word");
using TilePair = std::conditional<(TILE_TX_BITS + TILE_CLS_BITS <= 16), uint16_t, uint32_t>::type;
using TileSlot = std::conditional<(TILE_TX_BITS <= 8), uint8_t, uint16_t>::type;
constexpr int TILE_TURN_BITS = 5;                     // the turn values of the two orders: 0 .. 31
constexpr int TILE_SORT_KEYS = 1 << (TILE_TX_BITS > TILE_TURN_BITS ? TILE_TX_BITS : TILE_TURN_BITS);
constexpr int TILE_KEY_WORDS = std::max(std::max((EM_TILE_CLASSES + 8) / 2, EM_TILE_TX + 2), (2 * EM_TILE_PAIRS + 7) / 8);
constexpr int TILE_PAIR_TURNS = (EM_TILE_PAIRS + 255) / 256, TILE_CLS_TURNS = (EM_TILE_CLASSES + 255) / 256;
static_assert(EM_TILE_TX <= 256, "tile_rank_and_scan takes one transcript a lane");

// One workgroup per tile, a fixed grid striding over the *n_tiles tiles.  It reads the tile's transcripts and
// classes as the two placement kernels left them, puts them into the order the chunk kernel wants -- the order the
// two sorts by (tile, turns, index) gave before:
//   transcripts by min(ceil(degree / 8), 31) descending (degree_bits > 0), then id ascending: the row phase of
//   em_local_chunk_kernel gives a wave eight neighbours of the list at a time and loops as long as the longest;
//   classes by min(ceil(length / EM_TILE_CLASS_BATCH), 31) descending (length_bits > 0), then internal index
//   ascending: a lane of the class phase takes its tuple EM_TILE_CLASS_BATCH entries at a time and a wave loops as
//   long as the longest of its 64 classes
// -- and writes tx_list / cls_list back in place, tx_pair / cls_pair (the tile's first pair plus the prefix sums
// of degrees / lengths) and the tile's two views: tuples in tuple order, rows in the order of the whole table's
// transcript-major view (quant_rows_build), which this kernel does not read.  Everything comes from the tile's own
// classes, and the ids of a tuple are fetched once:
//   the classes are ranked by index, by counting (a class's rank is the number of indices below its own: the lanes
//   read the indices eight at a time, all the same words), and from that order a stable counting sort over the 32
//   turn values gives the list; both orders are kept (s_name: by index -> place in the list);
//   a lane per pair of the class-major view, in list order, finds its class in the prefix sums, fetches the id,
//   looks up the transcript's place as the placement kernel drew it (tx_local, written at the start), keeps that
//   place in LDS (s_slot) and counts the pair into the transcript's degree -- a class that names a transcript twice
//   counts twice.  A lane's pairs are fetched together, not one after the other;
//   the transcripts are ordered by those degrees, which leaves s_map: place as drawn -> place in the list, and the
//   class-major view is s_map of s_slot, written in whole runs;
//   the rows are the tile's pairs taken in ascending internal class index and tuple position -- the order of the
//   class-major view of the whole table, which its stable sort keeps within a transcript -- and moved by a stable
//   counting sort on the transcript's place in the list (tile_sort_count, tile_sort_place).
// A class's place in the list is a label only, so no sum of the EM changes with it.  The places as drawn pass
// through global memory inside the workgroup (written before a barrier, read after it); no workgroup reads what
// another wrote in this launch.
// A tile whose sizes are not what the packing promised is left alone (em_local_chunk_kernel then raises its
// fault word from the same sizes).
__global__ void __launch_bounds__(256)
tile_build_kernel(const int64_t *__restrict__ n_tiles, const int64_t *__restrict__ tile_tx, const int64_t *__restrict__ tile_cls,
                  const int64_t *__restrict__ tile_pair, int64_t n_tx, int64_t n_classes, int64_t n_ids,
                  const int64_t *__restrict__ cls_offset, const int32_t *__restrict__ ids, int degree_bits, int length_bits,
                  int32_t *tx_list, int32_t *cls_list, int64_t *__restrict__ tx_pair, int64_t *__restrict__ cls_pair,
                  int32_t *tx_local, uint16_t *__restrict__ out_cls_tx, uint16_t *__restrict__ out_tx_cls)
{
    // the keys of the transcripts' ranking; before that the classes' indices, and at the end the rows before they leave
    __shared__ __attribute__((aligned(16))) unsigned long long s_key[TILE_KEY_WORDS];
    __shared__ int32_t s_tx[EM_TILE_TX], s_tx_off[EM_TILE_TX + 1];
    __shared__ int32_t s_cls[EM_TILE_CLASSES], s_cls_off[EM_TILE_CLASSES + 1];       // the classes as listed
    __shared__ int32_t s_icls[EM_TILE_CLASSES], s_ioff[EM_TILE_CLASSES + 1];         // the classes in ascending index
    __shared__ int32_t s_src[EM_TILE_CLASSES];                   // as listed: a class's first id in ids
    __shared__ uint16_t s_name[EM_TILE_CLASSES];                 // in ascending index: a class's place in the list
    __shared__ TileSlot s_slot[EM_TILE_PAIRS];                   // class-major pairs: the transcript's place as drawn
    __shared__ uint16_t s_map[EM_TILE_TX];                       // place as drawn -> place in the list
    __shared__ TilePair s_pair[EM_TILE_PAIRS];                   // the pairs by ascending class index
    __shared__ uint32_t s_hist[4 * TILE_SORT_KEYS];              // tile_sort_count / tile_sort_place
    __shared__ uint32_t s_turn_base[1 << TILE_TURN_BITS];        // classes of fewer turns
    __shared__ int32_t s_wave[4];
    uint32_t *const s_index = reinterpret_cast<uint32_t *>(s_key);
    uint16_t *const s_rows = reinterpret_cast<uint16_t *>(s_key);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t tiles = *n_tiles;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t tx0 = tile_tx[tile], cls0 = tile_cls[tile], pair0 = tile_pair[tile];
        const int64_t tx_n = tile_tx[tile + 1] - tx0, cls_n = tile_cls[tile + 1] - cls0, pair_n = tile_pair[tile + 1] - pair0;
        if (tx0 < 0 || cls0 < 0 || pair0 < 0 || tx_n < 0 || cls_n < 0 || pair_n < 0 || tx_n > EM_TILE_TX ||
            cls_n > EM_TILE_CLASSES || pair_n > EM_TILE_PAIRS || tx0 + tx_n > n_tx || cls0 + cls_n > n_classes ||
            pair0 + pair_n > n_ids) continue;                       // (block-uniform)
        const int n_t = (int)tx_n, n_c = (int)cls_n, n_p = (int)pair_n;
        // ---- the members as they were placed
        for (int i = tid; i < n_t; i += 256) {
            const int32_t t = tx_list[tx0 + i];
            s_tx[i] = t;
            s_tx_off[i] = 0;
            if ((uint64_t)t < (uint64_t)n_tx) tx_local[t] = i;
        }
        int32_t cls[TILE_CLS_TURNS], len[TILE_CLS_TURNS];
#pragma unroll
        for (int u = 0; u < TILE_CLS_TURNS; ++u) {
            const int k = tid + 256 * u;
            cls[u] = k < n_c ? cls_list[cls0 + k] : -1;
        }
#pragma unroll
        for (int u = 0; u < TILE_CLS_TURNS; ++u) {
            const int k = tid + 256 * u;
            len[u] = (uint64_t)cls[u] < (uint64_t)n_classes ? (int32_t)(cls_offset[cls[u] + 1] - cls_offset[cls[u]]) : 0;
            if (k < n_c) s_index[k] = (uint32_t)cls[u];
        }
        if (tid < 8) s_index[n_c + tid] = 0xffffffffu;             // (behind the indices: below no index)
        __syncthreads();
        // ---- the classes in ascending index, then as listed
        {
            int32_t rank[TILE_CLS_TURNS];
#pragma unroll
            for (int u = 0; u < TILE_CLS_TURNS; ++u) rank[u] = 0;
            for (int j = 0; j < n_c; j += 8) {
                const uint4 a = *reinterpret_cast<const uint4 *>(s_index + j), b = *reinterpret_cast<const uint4 *>(s_index + j + 4);
#pragma unroll
                for (int u = 0; u < TILE_CLS_TURNS; ++u) {
                    const uint32_t mine = (uint32_t)cls[u];
                    rank[u] += (a.x < mine ? 1 : 0) + (a.y < mine ? 1 : 0) + (a.z < mine ? 1 : 0) + (a.w < mine ? 1 : 0) +
                               (b.x < mine ? 1 : 0) + (b.y < mine ? 1 : 0) + (b.z < mine ? 1 : 0) + (b.w < mine ? 1 : 0);
                }
            }
#pragma unroll
            for (int u = 0; u < TILE_CLS_TURNS; ++u)
                if (tid + 256 * u < n_c && rank[u] < n_c) { s_icls[rank[u]] = cls[u]; s_ioff[rank[u]] = len[u]; }
        }
        __syncthreads();
        const int longest_c = (1 << length_bits) - 1;
        auto turns_of = [&](int r) -> uint32_t {
            return (uint32_t)(longest_c - min((s_ioff[r] + EM_TILE_CLASS_BATCH - 1) / EM_TILE_CLASS_BATCH, longest_c));
        };
        tile_sort_count<TILE_TURN_BITS>(n_c, turns_of, s_hist);
        if (tid < 64) {                                             // classes of fewer turns: one wave scans the 32 values
            constexpr int TURNS = 1 << TILE_TURN_BITS;
            uint32_t m = 0;
            if (tid < TURNS) for (int w = 0; w < 4; ++w) m += s_hist[w * TURNS + tid];
            uint32_t incl = m;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (tid < TURNS) s_turn_base[tid] = incl - m;
        }
        __syncthreads();
        tile_sort_place<TILE_TURN_BITS>(n_c, turns_of, [&](int d) { return s_turn_base[d]; }, s_hist,
                                        [&](int r, uint32_t place) {
                                            if (place < (uint32_t)n_c) {
                                                s_name[r] = (uint16_t)place;
                                                s_cls[place] = s_icls[r];
                                                s_cls_off[place] = s_ioff[r];
                                            }
                                        });
        tile_scan<EM_TILE_CLASSES>(n_c, s_cls_off, s_wave);
        tile_scan<EM_TILE_CLASSES>(n_c, s_ioff, s_wave);
        for (int k = tid; k < n_c; k += 256) {
            const int32_t c = s_cls[k];
            cls_list[cls0 + k] = c;
            cls_pair[cls0 + k] = pair0 + s_cls_off[k];
            s_src[k] = s_cls_off[k + 1] > s_cls_off[k] && (uint64_t)c < (uint64_t)n_classes ? (int32_t)cls_offset[c] : 0;
        }
        // (only lengths that add up to the tile's pairs are walked: a place past them would be another tile's)
        const bool classes_fit = s_cls_off[n_c] == n_p && s_ioff[n_c] == n_p;       // (block-uniform: the entries stay)
        __syncthreads();
        // ---- the degrees: a lane per pair of the class-major view
        if (classes_fit) {
            int64_t at[TILE_PAIR_TURNS];
            int32_t id[TILE_PAIR_TURNS];
            uint32_t slot[TILE_PAIR_TURNS];
#pragma unroll
            for (int u = 0; u < TILE_PAIR_TURNS; ++u) {
                const int p = tid + 256 * u;
                at[u] = -1;
                if (p < n_p) { const int k = tile_find(s_cls_off, n_c, p); at[u] = (int64_t)s_src[k] + (p - s_cls_off[k]); }
            }
#pragma unroll
            for (int u = 0; u < TILE_PAIR_TURNS; ++u) id[u] = at[u] >= 0 && at[u] < n_ids ? ids[at[u]] : -1;
#pragma unroll
            for (int u = 0; u < TILE_PAIR_TURNS; ++u) slot[u] = (uint64_t)id[u] < (uint64_t)n_tx ? (uint32_t)tx_local[id[u]] : 0xffffffffu;
#pragma unroll
            for (int u = 0; u < TILE_PAIR_TURNS; ++u) {
                const int p = tid + 256 * u;
                if (p >= n_p) continue;
                const bool listed = slot[u] < (uint32_t)n_t;
                if (listed) atomicAdd(&s_tx_off[slot[u]], 1);
                s_slot[p] = (TileSlot)(listed ? slot[u] : 0u);
            }
        }
        __syncthreads();                                            // (the degrees stand; s_key is taken again)
        // ---- the transcripts as listed
        for (int i = tid; i < n_t; i += 256) {
            const int64_t degree = s_tx_off[i];
            const int64_t longest = (1 << degree_bits) - 1;
            s_key[i] = (unsigned long long)(longest - min((degree + 7) >> 3, longest)) << 32 | (uint32_t)s_tx[i];
        }
        __syncthreads();
        tile_rank_and_scan<EM_TILE_TX>(n_t, s_key, s_tx, s_tx_off, s_wave, s_map);
        for (int i = tid; i < n_t; i += 256) {
            tx_list[tx0 + i] = s_tx[i];
            tx_pair[tx0 + i] = pair0 + s_tx_off[i];
        }
        // ---- the two views
        if (classes_fit && s_tx_off[n_t] == n_p) {                  // (block-uniform)
#pragma unroll
            for (int u = 0; u < TILE_PAIR_TURNS; ++u) {
                const int p = tid + 256 * u;
                if (p >= n_p) continue;
                out_cls_tx[pair0 + p] = s_map[s_slot[p]];
                // (pair p of the classes in ascending index: of the class at r, listed at k)
                const int r = tile_find(s_ioff, n_c, p), k = min((int)s_name[r], n_c - 1);
                const int from = min(s_cls_off[k] + (p - s_ioff[r]), n_p - 1);
                s_pair[p] = (TilePair)(((uint32_t)s_map[s_slot[from]] & ((1u << TILE_TX_BITS) - 1u)) << TILE_CLS_BITS | (uint32_t)k);
            }
            __syncthreads();
            auto place_of = [&](int p) -> uint32_t { return (uint32_t)s_pair[p] >> TILE_CLS_BITS; };
            tile_sort_count<TILE_TX_BITS>(n_p, place_of, s_hist);
            tile_sort_place<TILE_TX_BITS>(n_p, place_of, [&](int d) { return d < n_t ? (uint32_t)s_tx_off[d] : (uint32_t)n_p; }, s_hist,
                                          [&](int p, uint32_t place) {
                                              if (place < (uint32_t)n_p) s_rows[place] = (uint16_t)(s_pair[p] & ((1u << TILE_CLS_BITS) - 1u));
                                          });
            for (int j = tid; j < n_p; j += 256) out_tx_cls[pair0 + j] = s_rows[j];
        }
        __syncthreads();                                            // (the next tile takes the arrays again)
    }
}

// EmTiles::order: the tiles by descending pair count (the row phase of the chunk kernel walks the pairs), so that
// a chunk launch starts its large tiles first and fills its last, thinly occupied round with the small ones.  A
// counting sort over TILE_ORDER_BINS size bins by ONE workgroup: a few thousand tiles, n_tx at the most.  The
// tiles of a bin stand in the order their lanes drew their places in: not stable, and no result depends on it.
constexpr int TILE_ORDER_BINS = 256;
__global__ void __launch_bounds__(1024)
tile_order_kernel(const int64_t *__restrict__ tile_cls, const int64_t *__restrict__ cls_pair, const int64_t *n_tiles,
                  int32_t *__restrict__ order)
{
    __shared__ unsigned int at[TILE_ORDER_BINS];      // tiles of the bin, then the next free place of the bin
    const int64_t tiles = *n_tiles;
    auto bin_of = [&](int64_t i) {
        const int64_t pairs = cls_pair[tile_cls[i + 1]] - cls_pair[tile_cls[i]];
        const int64_t fill = min(max(pairs, (int64_t)0), (int64_t)EM_TILE_PAIRS) * (TILE_ORDER_BINS - 1) / EM_TILE_PAIRS;
        return TILE_ORDER_BINS - 1 - (int)fill;       // (the fullest tiles in bin 0)
    };
    for (int d = threadIdx.x; d < TILE_ORDER_BINS; d += 1024) at[d] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < tiles; i += 1024) atomicAdd(&at[bin_of(i)], 1u);
    __syncthreads();
    if (threadIdx.x < 64) {                           // exclusive scan over the bins: four per lane of one wave
        constexpr int PER = TILE_ORDER_BINS / 64;
        unsigned int n[PER], sum = 0;
        for (int k = 0; k < PER; ++k) { n[k] = at[threadIdx.x * PER + k]; sum += n[k]; }
        unsigned int incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int o = __shfl_up(incl, d, 64);
            if ((int)threadIdx.x >= d) incl += o;
        }
        unsigned int first = incl - sum;
        for (int k = 0; k < PER; ++k) { at[threadIdx.x * PER + k] = first; first += n[k]; }
    }
    __syncthreads();
    for (int64_t i = threadIdx.x; i < tiles; i += 1024) order[atomicAdd(&at[bin_of(i)], 1u)] = (int32_t)i;
}
static_assert(TILE_ORDER_BINS % 64 == 0, "the scan gives every lane of a wave the same number of bins");

constexpr int TILE_BUILD_BLOCKS = 2048;       // tile_build_kernel's grid: eight workgroups a CU, striding over the tiles

int build_tiles(Scratch &scratch, QuantBuild &q)
{
    hipStream_t stream = scratch.stream;
    const int64_t C = q.n_classes, M = q.n_ids, T = q.n_tx;
    if (M >= (1LL << 31) || C >= (1LL << 31) || T >= (1LL << 31) - 2) return -2;
    const int64_t n_segments = (T + EM_TILE_SEGMENT - 1) / EM_TILE_SEGMENT;
    // comp[3 T], then the tiles' cursors of the two placement kernels, [T + 1] each: cleared together
    QB_ALLOC(parent, int32_t, T); QB_ALLOC(comp, int32_t, 3 * T + 2 * (T + 1)); QB_ALLOC(root_tile, int32_t, T);
    QB_ALLOC(seg_sizes, int64_t, 4 * n_segments); QB_ALLOC(seg_base, int64_t, 4 * (n_segments + 1));
    QB_ALLOC(oversize, unsigned long long, 1);
    QB_ALLOC(tile_pair, int64_t, T + 2);
    QB_ALLOC(tx_local, int32_t, T);
    int32_t *cursor_tx = comp + 3 * T, *cursor_cls = cursor_tx + (T + 1);
    const int64_t *n_tiles = seg_base + n_segments;
    QB_TRY(hipMemsetAsync(comp, 0, (3 * T + 2 * (T + 1)) * sizeof(int32_t), stream));
    QB_TRY(hipMemsetAsync(oversize, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, parent, T);
    hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_offset, q.ids, C, parent);
    hipLaunchKernelGGL(cc_label_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, parent, T, q.tx_label, comp);
    hipLaunchKernelGGL(cc_classes_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_offset, q.ids, C,
                       q.tx_label, comp);
    // the tiles' sizes are known from the components alone: their starts in the lists before anything is listed
    hipLaunchKernelGGL(tile_pack_kernel<false>, dim3(blocks_for(64 * n_segments)), dim3(256), 0, stream, comp, T, n_segments,
                       root_tile, seg_sizes, oversize, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr,
                       (int64_t *)nullptr);
    hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, stream, seg_sizes, n_segments, seg_base, q.tile_tx,
                       q.tile_cls, tile_pair, q.tx_pair, q.cls_pair);
    hipLaunchKernelGGL(tile_pack_kernel<true>, dim3(blocks_for(64 * n_segments)), dim3(256), 0, stream, comp, T, n_segments,
                       (int32_t *)nullptr, (int64_t *)nullptr, (unsigned long long *)nullptr, seg_base, q.tile_tx, q.tile_cls,
                       tile_pair);
    // members into their tiles in the order the lanes come by, then every tile in order by its own workgroup
    int end_bit = 1;
    while ((1LL << end_bit) < T + 1 && end_bit < 31) ++end_bit;
    const int degree_bits = end_bit + 5 <= 31 ? 5 : 0;          // (the width the sorts by (tile, turns) had room for)
    const int length_bits = SKM_EM_CLASS_ORDER ? degree_bits : 0;
    hipLaunchKernelGGL(tx_place_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, q.tx_label, root_tile, seg_base, T,
                       q.tile_tx, cursor_tx, q.tx_tile, q.tx_list);
    hipLaunchKernelGGL(cls_place_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_offset, q.ids, C, T, q.tx_tile,
                       q.tile_cls, cursor_cls, q.cls_tile, q.cls_list);
    hipLaunchKernelGGL(tile_build_kernel, dim3((unsigned)std::min<int64_t>(std::max<int64_t>(T, 1), TILE_BUILD_BLOCKS)), dim3(256),
                       0, stream, n_tiles, q.tile_tx, q.tile_cls, tile_pair, T, C, M, q.cls_offset, q.ids, degree_bits,
                       length_bits, q.tx_list, q.cls_list, q.tx_pair, q.cls_pair, tx_local, q.tile_cls_tx, q.tile_tx_cls);
    hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, stream, q.tile_cls, q.cls_pair, n_tiles, q.tile_order);
    QB_TRY(hipMemcpyAsync(&q.tile_info[0], n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    QB_TRY(hipMemcpyAsync(&q.tile_info[1], oversize, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    return 0;
}

}  // namespace

// The whole setup as one asynchronous pipeline on `stream`: classes from the mapper's table (when
// `table` is given) in locality order with perm[] back to first-seen order -- ranked by bitmap
// when the first-seen values allow it, by two sorts otherwise -- or the caller's classes
// reordered; then the component tiles, from the classes alone.  The host looks once, when all of it
// has been queued and the stream has drained: a ranked attempt that found two classes with one
// first-seen value is then thrown away and the sorting path runs.  Returns 0 or a negative code.
int quant_setup(const ClassTable *table, QuantBuild &q, int32_t *perm, hipStream_t stream)
{
    const bool can_rank = table && q.first_seen_bound > 0 && q.first_seen_bound <= RANK_BITMAP_MAX_UNITS;
    for (int attempt = can_rank ? 0 : 1; attempt < 2; ++attempt) {
        unsigned int shared_first_seen = 0;
        {
            Scratch scratch(stream);
            const unsigned int *flag = nullptr;
            if (attempt == 0) {
                if (build_from_table_ranked(scratch, *table, q, perm, &flag)) return -1;
            } else {
                if (table && build_from_table(scratch, *table, q)) return -1;
                if (localize(scratch, q, perm)) return -1;
            }
            if (q.tile_tx && build_tiles(scratch, q)) return -1;
            QB_TRY(hipGetLastError());
            if (flag) QB_TRY(hipMemcpyAsync(&shared_first_seen, flag, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        }                              // ~Scratch: the synchronisation
        if (shared_first_seen) continue;
        return 0;
    }
    return -1;
}

int64_t quant_rows_build(const QuantBuild &q, const QuantRows &rows, hipStream_t stream)
{
    int64_t n_rows = -1;
    {
        Scratch scratch(stream);
        if (transpose(scratch, q, rows)) return -1;
        QB_TRY(hipGetLastError());
        QB_TRY(hipMemcpyAsync(&n_rows, rows.tx_row + q.n_tx, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    }                                  // ~Scratch: the synchronisation
    if (n_rows > rows.n_rows_cap) return -3;
    return n_rows;
}

// ---- the residual: the components above the tile capacity as an EM problem of their own ---------
namespace {

// counts[0] classes, [1] pairs, [2] rows of the components above the capacity (tile == n_tx)
__global__ void __launch_bounds__(256)
residual_count_kernel(const int32_t *cls_tile, const int64_t *cls_offset, int64_t n_classes, const int32_t *tx_tile,
                      const int64_t *tx_row, int64_t n_tx, unsigned long long *counts)
{
    unsigned long long classes = 0, pairs = 0, rows = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < max(n_classes, n_tx);
         i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n_classes && cls_tile[i] == (int32_t)n_tx) { ++classes; pairs += cls_offset[i + 1] - cls_offset[i]; }
        if (i < n_tx && tx_tile[i] == (int32_t)n_tx) rows += tx_row[i + 1] - tx_row[i];
    }
    if (classes) atomicAdd(&counts[0], classes);
    if (pairs) atomicAdd(&counts[1], pairs);
    if (rows) atomicAdd(&counts[2], rows);
}

// keep[c] = class c is residual; len[c] = its pairs if so
__global__ void __launch_bounds__(256)
residual_class_sizes_kernel(const int32_t *cls_tile, const int64_t *cls_offset, int64_t n_classes, int32_t residual_tile,
                            int64_t *keep, int64_t *len)
{
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_classes;
         c += (int64_t)gridDim.x * blockDim.x) {
        const bool mine = cls_tile[c] == residual_tile;
        keep[c] = mine ? 1 : 0;
        len[c] = mine ? cls_offset[c + 1] - cls_offset[c] : 0;
    }
}

__global__ void __launch_bounds__(256)
residual_tx_sizes_kernel(const int32_t *tx_tile, const int64_t *tx_row, const int64_t *row_start, int64_t n_tx,
                         int64_t *rows, int64_t *len)
{
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tx;
         t += (int64_t)gridDim.x * blockDim.x) {
        const bool mine = tx_tile[t] == (int32_t)n_tx;
        rows[t] = mine ? tx_row[t + 1] - tx_row[t] : 0;
        len[t] = mine ? row_start[tx_row[t + 1]] - row_start[tx_row[t]] : 0;
    }
}

// residual class rank[c] <- class c: its tuple and where its count comes from
__global__ void __launch_bounds__(256)
residual_fill_cls_kernel(const int32_t *cls_tile, int64_t n_classes, int32_t residual_tile, const int64_t *rank,
                         const int64_t *cls_offset, const int32_t *ids, const int64_t *new_offset,
                         int64_t *out_offset, int32_t *out_ids, int32_t *out_src, int64_t n_residual)
{
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_classes;
         c += (int64_t)gridDim.x * blockDim.x) {
        if (cls_tile[c] != residual_tile) continue;
        const int64_t k = rank[c], src = cls_offset[c], n = cls_offset[c + 1] - src, dst = new_offset[c];
        out_offset[k] = dst;
        if (k == n_residual - 1) out_offset[n_residual] = dst + n;
        out_src[k] = (int32_t)c;
        for (int64_t j = 0; j < n; ++j) out_ids[dst + j] = ids[src + j];
    }
}

__global__ void __launch_bounds__(256)
residual_fill_tx_kernel(const int32_t *tx_tile, int64_t n_tx, const int64_t *tx_row, const int64_t *row_start,
                        const int32_t *tx_cls, const int64_t *rank, const int64_t *new_pair, int32_t *out)
{
    const int sub = threadIdx.x & 7;
    for (int64_t t = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3; t < n_tx;
         t += ((int64_t)gridDim.x * blockDim.x) >> 3) {
        if (tx_tile[t] != (int32_t)n_tx) continue;
        const int64_t src = row_start[tx_row[t]], n = row_start[tx_row[t + 1]] - src, dst = new_pair[t];
        for (int64_t j = sub; j < n; j += 8) out[dst + j] = (int32_t)rank[tx_cls[src + j]];
    }
}

}  // namespace

int quant_residual_count(const QuantBuild &q, const QuantRows &rows_in, int64_t counts[3], hipStream_t stream)
{
    Scratch scratch(stream);
    QB_ALLOC(sums, unsigned long long, 3);
    QB_TRY(hipMemsetAsync(sums, 0, 3 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(residual_count_kernel, dim3(blocks_for(std::max(q.n_classes, q.n_tx))), dim3(256), 0, stream,
                       q.cls_tile, q.cls_offset, q.n_classes, q.tx_tile, rows_in.tx_row, q.n_tx, sums);
    QB_TRY(hipGetLastError());
    QB_TRY(hipMemcpyAsync(counts, sums, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    QB_TRY(hipStreamSynchronize(stream));
    return 0;
}

int quant_residual_build(const QuantBuild &q, const QuantRows &rows_in, QuantResidual &r, hipStream_t stream)
{
    Scratch scratch(stream);
    const int64_t C = q.n_classes, T = q.n_tx;
    QB_ALLOC(keep, int64_t, C); QB_ALLOC(rank, int64_t, C + 1);
    QB_ALLOC(len, int64_t, std::max(C, T)); QB_ALLOC(new_offset, int64_t, C + 1);
    QB_ALLOC(rows, int64_t, T); QB_ALLOC(new_pair, int64_t, T + 1);
    hipLaunchKernelGGL(residual_class_sizes_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_tile, q.cls_offset, C,
                       (int32_t)T, keep, len);
    if (exclusive_scan_with_total(scratch, keep, rank, C)) return -1;
    if (exclusive_scan_with_total(scratch, len, new_offset, C)) return -1;
    hipLaunchKernelGGL(residual_fill_cls_kernel, dim3(blocks_for(C)), dim3(256), 0, stream, q.cls_tile, C, (int32_t)T, rank,
                       q.cls_offset, q.ids, new_offset, r.cls_offset, r.ids, r.cls_src, r.n_classes);
    hipLaunchKernelGGL(residual_tx_sizes_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, q.tx_tile, rows_in.tx_row,
                       rows_in.row_start, T, rows, len);
    if (exclusive_scan_with_total(scratch, rows, r.tx_row, T)) return -1;
    if (exclusive_scan_with_total(scratch, len, new_pair, T)) return -1;
    hipLaunchKernelGGL(row_fill_kernel, dim3(blocks_for(T)), dim3(256), 0, stream, new_pair, r.tx_row, T, r.n_ids,
                       r.row_start, r.row_tx);
    hipLaunchKernelGGL(residual_fill_tx_kernel, dim3(blocks_for(8 * T)), dim3(256), 0, stream, q.tx_tile, T, rows_in.tx_row,
                       rows_in.row_start, rows_in.tx_cls, rank, new_pair, r.tx_cls);
    QB_TRY(hipGetLastError());
    return 0;
}

const char *quant_setup_failure() { return g_setup_failure; }

void warm_code_quant_setup()
{
    hipFuncAttributes attributes;
    (void)hipFuncGetAttributes(&attributes, reinterpret_cast<const void *>(&iota_kernel));
    (void)hipFuncGetAttributes(&attributes, reinterpret_cast<const void *>(&table_dump_kernel));
}

}  // namespace skm
