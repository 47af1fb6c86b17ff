// Sequence-bias correction (--bias; DESIGN.md section 4, "Sequence bias").
//
// Random-hexamer priming makes fragments start more often at some hexamers than at others.  The
// correction compares the hexamers the aligned reads start with (observed, O) with the hexamers the
// expressed transcripts offer (expected, E), turns the ratio into a weight b per hexamer, and rescales
// every transcript's effective length by the mean weight of its windows; the EM then runs a second time.
//
// Five kernels, none on the mapping path of a run without --bias:
//   pool scatter   the transcripts' own 2-bit sequences, rebuilt once per index from contigs and target rows
//   windows        n_t of every transcript, once per index
//   observed       after each mapped batch of a mapper asked to count: a 4096-bin histogram in LDS
//   expected       over the pool, in 96-bit fixed point (three passes, a 32-bit limb of the weights each):
//                  integer atomics, bit-reproducible for any grid
//   weights        one block
//   lengths        over the pool, b in LDS; a transcript's sum is one wave's, in a fixed order
// skm_bias_correct_many runs the last three for many samples at once (the samples of a sample set): the sample
// is a grid dimension of `expected` and of `weights`, and a block of `lengths` holds the b tables of
// BIAS_LENGTHS_G samples in LDS and decodes a transcript's windows once for all of them.  Each kernel shares its
// arithmetic with the single-sample one, so a row has the bits of the single call.
// The kernels over the pool give one wave a transcript at a time: a lane takes the windows that start in
// every 64th word, so a wave reads a transcript's words as one stretch.
#include "../../include/seekmer_hip.h"
#include "skm_bias.h"

namespace skm {

namespace {

constexpr int BIAS_THREADS = 256;
constexpr int BIAS_WAVES = BIAS_THREADS / 64;

// the value of a 96-bit fixed-point sum kept as three sums of 32-bit limbs (each below 2^63), lowest limb first
__device__ __forceinline__ double limbs_value(unsigned long long l0, unsigned long long l1, unsigned long long l2)
{
    return ((double)l2 * 18446744073709551616.0 + (double)l1 * 4294967296.0) + (double)l0;
}

// reverse complement of a hexamer code
__device__ __forceinline__ uint32_t revcomp6(uint32_t h)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < BIAS_HEXAMER; ++i) {
        r = (r << 2) | (3u - (h & 3u));
        h >>= 2;
    }
    return r;
}

// words of transcript t in which a window starts (positions 0 .. len - 6)
__device__ __forceinline__ int32_t window_words(int32_t len)
{
    return len < BIAS_HEXAMER ? 0 : (len - BIAS_HEXAMER + 32) >> 5;
}

// f(h+) for every window that starts in word w of the transcript whose words begin at `base`, in
// position order.  A window may run into the next word: that is the transcript's own next word, or --
// when the transcript ends in this one -- a word whose bits are not looked at (p + 5 < len).
template <class F>
__device__ __forceinline__ void for_windows(const TxPool &pool, int64_t base, int32_t len, int32_t w, F f)
{
    const uint64_t c0 = pool.codes[base + w], c1 = pool.codes[base + w + 1];
    const uint64_t known = ((uint64_t)pool.known[base + w] << 32) | pool.known[base + w + 1];
    const int32_t left = len - (BIAS_HEXAMER - 1) - (w << 5);        // windows from this word on
    const int n = left < 32 ? left : 32;
    for (int i = 0; i < n; ++i) {
        if (((known << i) >> (64 - BIAS_HEXAMER)) != (1u << BIAS_HEXAMER) - 1u) continue;
        const uint64_t window = i == 0 ? c0 : (c0 << (2 * i)) | (c1 >> (64 - 2 * i));
        f((uint32_t)(window >> (64 - 2 * BIAS_HEXAMER)));
    }
}

__global__ void __launch_bounds__(BIAS_THREADS)
bias_pool_scatter_kernel(const uint64_t *__restrict__ seq2, const PoolContig *__restrict__ contigs, int64_t n_contigs,
                         const Coord *__restrict__ targets, TxPool pool, unsigned long long *bad_rows)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < n_contigs; c += n_waves) {
        const PoolContig pc = contigs[c];
        const int64_t L = pc.length;
        for (int32_t r = 0; r < pc.target_count; ++r) {               // (everything here is wave-uniform)
            const Coord row = targets[pc.target_offset + r];
            const bool forward = row.entry >= 0;
            const int64_t t = forward ? row.entry : ~row.entry;
            const int64_t a = forward ? (int64_t)row.offset : (int64_t)row.offset + K - L;   // T_t[a .. a + L)
            if (L <= 0 || t >= pool.n_tx || a < 0 || a + L > pool.tx_len[t]) {
                if (lane == 0) atomicAdd(bad_rows, 1ULL);
                continue;
            }
            const int64_t base = pool.tx_word[t];
            const int64_t w_last = (a + L - 1) >> 5;
            for (int64_t w = (a >> 5) + lane; w <= w_last; w += 64) {
                const int64_t p0 = w << 5;
                const int64_t lo = p0 > a ? p0 : a, hi = p0 + 32 < a + L ? p0 + 32 : a + L;
                const int n = (int)(hi - lo);                          // 1 .. 32 bases of this word
                uint64_t bits;
                if (forward) {
                    bits = packed_window(seq2, pc.offset + (lo - a));
                } else {                 // positions lo .. hi - 1 are the complement of S[L - 1 - (p - a)]
                    const uint64_t window = packed_window(seq2, pc.offset + (L - (hi - a)));
                    bits = revcomp32(window) << (2 * (32 - n));
                }
                const uint64_t keep = n == 32 ? ~0ULL : ~(~0ULL >> (2 * n));
                const uint32_t keep_known = n == 32 ? ~0u : ~(~0u >> n);
                atomicOr(reinterpret_cast<unsigned long long *>(pool.codes + base + w),
                         (unsigned long long)((bits & keep) >> (2 * (lo - p0))));
                atomicOr(pool.known + base + w, keep_known >> (lo - p0));
            }
        }
    }
}

__global__ void __launch_bounds__(BIAS_THREADS)
bias_windows_kernel(TxPool pool, int32_t *__restrict__ tx_windows)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = wave; t < pool.n_tx; t += n_waves) {
        const int32_t len = pool.tx_len[t], n_words = window_words(len);
        const int64_t base = pool.tx_word[t];
        int32_t count = 0;
        for (int32_t w = lane; w < n_words; w += 64) for_windows(pool, base, len, w, [&](uint32_t) { ++count; });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
        if (lane == 0) tx_windows[t] = count;
    }
}

__global__ void __launch_bounds__(BIAS_THREADS)
bias_observed_kernel(const uint32_t *__restrict__ records, int record_words, int words_per_read, int paired,
                     const unsigned long long *__restrict__ rec_tuple, const int32_t *__restrict__ rec_unit,
                     int64_t n_units, unsigned long long *observed)
{
    __shared__ unsigned int bins[BIAS_BINS];          // (a batch holds fewer than 2^31 units)
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS) bins[i] = 0;
    __syncthreads();
    for (int64_t r = blockIdx.x * (int64_t)BIAS_THREADS + threadIdx.x; r < n_units; r += (int64_t)gridDim.x * BIAS_THREADS) {
        if ((rec_tuple[r] >> 40) == 0) continue;                       // unaligned (after the strand filter)
        const int64_t read = (int64_t)rec_unit[r] * (paired ? 2 : 1);  // mate 1, or the single read
        const uint32_t *record = records + read * record_words;        // codes (u64 x W), ACGT bits (u32 x W), length
        if (record[3 * words_per_read] < (uint32_t)BIAS_HEXAMER) continue;
        if ((record[2 * words_per_read] >> (32 - BIAS_HEXAMER)) != (1u << BIAS_HEXAMER) - 1u) continue;
        const uint64_t codes = *reinterpret_cast<const uint64_t *>(record);
        atomicAdd(&bins[(uint32_t)(codes >> (64 - 2 * BIAS_HEXAMER))], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS)
        if (bins[i]) atomicAdd(&observed[i], (unsigned long long)bins[i]);
}

// one limb of one sample's weights over the pool, by a grid of `n_blocks` blocks of which this is `block`
__device__ __forceinline__ void expected_limb(const TxPool &pool, const unsigned long long *__restrict__ tx_weight, int plus,
                                              int minus, unsigned long long *expected, unsigned long long *bins,
                                              int64_t block, int64_t n_blocks)
{
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS) bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (block * (int64_t)BIAS_THREADS + threadIdx.x) >> 6;
    const int64_t n_waves = n_blocks * BIAS_WAVES;
    for (int64_t t = wave; t < pool.n_tx; t += n_waves) {
        const unsigned long long weight = tx_weight[t];
        if (weight == 0) continue;                                     // (most transcripts of a sample)
        const int32_t len = pool.tx_len[t], n_words = window_words(len);
        const int64_t base = pool.tx_word[t];
        for (int32_t w = lane; w < n_words; w += 64)
            for_windows(pool, base, len, w, [&](uint32_t h) {
                if (plus) atomicAdd(&bins[h], weight);
                if (minus) atomicAdd(&bins[revcomp6(h)], weight);
            });
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS)
        if (bins[i]) atomicAdd(&expected[i], bins[i]);
}

__global__ void __launch_bounds__(BIAS_THREADS)
bias_expected_kernel(TxPool pool, const unsigned long long *__restrict__ tx_weight, int plus, int minus,
                     unsigned long long *expected)
{
    __shared__ unsigned long long bins[BIAS_BINS];
    expected_limb(pool, tx_weight, plus, minus, expected, bins, blockIdx.x, gridDim.x);
}

// blockIdx.y = the limb, blockIdx.z = the sample: tx_weight[n][BIAS_LIMBS][n_tx], expected[n][BIAS_LIMBS][4096]
__global__ void __launch_bounds__(BIAS_THREADS)
bias_expected_many_kernel(TxPool pool, const unsigned long long *__restrict__ tx_weight, int plus, int minus,
                          unsigned long long *expected)
{
    __shared__ unsigned long long bins[BIAS_BINS];
    const int64_t row = (int64_t)blockIdx.z * BIAS_LIMBS + blockIdx.y;
    expected_limb(pool, tx_weight + row * pool.n_tx, plus, minus, expected + row * BIAS_BINS, bins, blockIdx.x, gridDim.x);
}

// one block, one sample
__device__ __forceinline__ void weights_of(const unsigned long long *__restrict__ observed,
                                           const unsigned long long *__restrict__ expected, double scale,
                                           double *__restrict__ expected_out, double *__restrict__ b, unsigned long long *sums)
{
    if (threadIdx.x < 1 + BIAS_LIMBS) sums[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long o = 0, e[BIAS_LIMBS] = {0, 0, 0};               // (integer sums: any order)
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS) {
        o += observed[i];
        for (int k = 0; k < BIAS_LIMBS; ++k) e[k] += expected[k * BIAS_BINS + i];
    }
    atomicAdd(&sums[0], o);
    for (int k = 0; k < BIAS_LIMBS; ++k) atomicAdd(&sums[1 + k], e[k]);
    __syncthreads();
    const double expected_total = limbs_value(sums[1], sums[2], sums[3]);
    const bool any = sums[0] != 0 && expected_total != 0.0;
    const double observed_total = (double)sums[0] + (double)BIAS_BINS;
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS) {
        const double e_i = limbs_value(expected[i], expected[BIAS_BINS + i], expected[2 * BIAS_BINS + i]);
        expected_out[i] = e_i * scale;
        b[i] = any && e_i != 0.0 ? (((double)observed[i] + 1.0) / observed_total) / (e_i / expected_total) : 1.0;
    }
}

__global__ void __launch_bounds__(BIAS_THREADS)
bias_weights_kernel(const unsigned long long *__restrict__ observed, const unsigned long long *__restrict__ expected,
                    double scale, double *__restrict__ expected_out, double *__restrict__ b)
{
    __shared__ unsigned long long sums[1 + BIAS_LIMBS];
    weights_of(observed, expected, scale, expected_out, b, sums);
}

// blockIdx.x = the sample: observed[n][4096], expected[n][BIAS_LIMBS][4096], scale[n], expected_out[n][4096], b[n][4096]
__global__ void __launch_bounds__(BIAS_THREADS)
bias_weights_many_kernel(const unsigned long long *__restrict__ observed, const unsigned long long *__restrict__ expected,
                         const double *__restrict__ scale, double *__restrict__ expected_out, double *__restrict__ b)
{
    __shared__ unsigned long long sums[1 + BIAS_LIMBS];
    const int64_t s = blockIdx.x;
    weights_of(observed + s * BIAS_BINS, expected + s * BIAS_LIMBS * BIAS_BINS, scale[s], expected_out + s * BIAS_BINS,
               b + s * BIAS_BINS, sums);
}

__global__ void __launch_bounds__(BIAS_THREADS)
bias_lengths_kernel(TxPool pool, const int32_t *__restrict__ tx_windows, const double *__restrict__ b, double share_plus,
                    double share_minus, const double *__restrict__ eff, double *__restrict__ eff_out)
{
    __shared__ double weights[BIAS_BINS];             // 32 KB
    for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS) weights[i] = b[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)BIAS_THREADS + threadIdx.x) >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * BIAS_WAVES;
    for (int64_t t = wave; t < pool.n_tx; t += n_waves) {
        const int32_t n_windows = tx_windows[t];
        if (n_windows == 0) {
            if (lane == 0) eff_out[t] = eff[t];
            continue;
        }
        const int32_t len = pool.tx_len[t], n_words = window_words(len);
        const int64_t base = pool.tx_word[t];
        // lane l sums the windows of the words l, l + 64, ... in position order, then the 64 lanes meet in a
        // butterfly: the order is a function of the transcript alone
        double sum = 0.0;
        for (int32_t w = lane; w < n_words; w += 64)
            for_windows(pool, base, len, w, [&](uint32_t h) {
                sum += share_plus * weights[h] + share_minus * weights[revcomp6(h)];
            });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) eff_out[t] = eff[t] * (sum / (double)n_windows);
    }
}

// The lengths of G samples at a time: blockIdx.y = the group of samples [G y, G y + G), whose b tables the block
// holds in LDS (G x 32 KB).  A transcript's windows are read and decoded once; every sample keeps a sum of its
// own that lane l feeds with the windows of the words l, l + 64, ... in position order and the 64 lanes close
// in the butterfly of bias_lengths_kernel: the terms, their order and the expression are that kernel's, so row s
// has the bits of the single call whatever G is.  A group past the last sample (n not a multiple of G) holds
// tables of zeros for the missing samples and writes nothing for them.
template <int G>
__global__ void __launch_bounds__(BIAS_THREADS)
bias_lengths_many_kernel(TxPool pool, const int32_t *__restrict__ tx_windows, const double *__restrict__ b, int64_t n,
                         double share_plus, double share_minus, const double *__restrict__ eff, double *__restrict__ eff_out)
{
    __shared__ double weights[G][BIAS_BINS];
    const int64_t first = (int64_t)blockIdx.y * G;
    const int here = n - first < G ? (int)(n - first) : G;
    for (int g = 0; g < G; ++g)
        for (int i = threadIdx.x; i < BIAS_BINS; i += BIAS_THREADS) weights[g][i] = g < here ? b[(first + g) * BIAS_BINS + i] : 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)BIAS_THREADS + threadIdx.x) >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * BIAS_WAVES;
    for (int64_t t = wave; t < pool.n_tx; t += n_waves) {
        const int32_t n_windows = tx_windows[t];
        if (n_windows == 0) {
            if (lane < here) eff_out[(first + lane) * pool.n_tx + t] = eff[(first + lane) * pool.n_tx + t];
            continue;
        }
        const int32_t len = pool.tx_len[t], n_words = window_words(len);
        const int64_t base = pool.tx_word[t];
        double sum[G];
#pragma unroll
        for (int g = 0; g < G; ++g) sum[g] = 0.0;
        for (int32_t w = lane; w < n_words; w += 64)
            for_windows(pool, base, len, w, [&](uint32_t h) {
                const uint32_t h_minus = revcomp6(h);
#pragma unroll
                for (int g = 0; g < G; ++g) sum[g] += share_plus * weights[g][h] + share_minus * weights[g][h_minus];
            });
#pragma unroll
        for (int g = 0; g < G; ++g) {
            double total = sum[g];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
            if (lane == 0 && g < here) eff_out[(first + g) * pool.n_tx + t] = eff[(first + g) * pool.n_tx + t] * (total / (double)n_windows);
        }
    }
}

int wave_grid(int64_t n_items, int cap)
{
    int64_t blocks = (n_items + BIAS_WAVES - 1) / BIAS_WAVES;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

}  // namespace

void launch_bias_pool_scatter(const uint64_t *seq2, const PoolContig *contigs, int64_t n_contigs, const Coord *targets,
                              const TxPool &pool, unsigned long long *bad_rows, hipStream_t stream)
{
    if (n_contigs == 0) return;
    hipLaunchKernelGGL(bias_pool_scatter_kernel, dim3((unsigned)wave_grid(n_contigs, 4096)), dim3(BIAS_THREADS), 0, stream,
                       seq2, contigs, n_contigs, targets, pool, bad_rows);
}

void launch_bias_windows(const TxPool &pool, int32_t *tx_windows, hipStream_t stream)
{
    if (pool.n_tx == 0) return;
    hipLaunchKernelGGL(bias_windows_kernel, dim3((unsigned)wave_grid(pool.n_tx, 4096)), dim3(BIAS_THREADS), 0, stream, pool,
                       tx_windows);
}

void launch_bias_observed(const uint32_t *records, int record_words, int words_per_read, int paired,
                          const unsigned long long *rec_tuple, const int32_t *rec_unit, int64_t n_units,
                          unsigned long long *observed, hipStream_t stream)
{
    if (n_units == 0) return;
    // (a block flushes 4096 bins: few blocks for a small batch, 16 units a lane at least)
    int64_t blocks = (n_units + 16 * BIAS_THREADS - 1) / (16 * BIAS_THREADS);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(bias_observed_kernel, dim3((unsigned)blocks), dim3(BIAS_THREADS), 0, stream, records, record_words,
                       words_per_read, paired, rec_tuple, rec_unit, n_units, observed);
}

void launch_bias_expected(const TxPool &pool, const unsigned long long *tx_weight, int strand,
                          unsigned long long *expected, int blocks, hipStream_t stream)
{
    if (pool.n_tx == 0) return;
    for (int limb = 0; limb < BIAS_LIMBS; ++limb)      // one pass per 32-bit limb of the weights: 32 KB of LDS each
        hipLaunchKernelGGL(bias_expected_kernel, dim3((unsigned)wave_grid(pool.n_tx, blocks)), dim3(BIAS_THREADS), 0, stream,
                           pool, tx_weight + limb * pool.n_tx, strand != SKM_STRAND_RF ? 1 : 0,
                           strand != SKM_STRAND_FR ? 1 : 0, expected + limb * BIAS_BINS);
}

void launch_bias_weights(const unsigned long long *observed, const unsigned long long *expected, double scale,
                         double *expected_out, double *b, hipStream_t stream)
{
    hipLaunchKernelGGL(bias_weights_kernel, dim3(1), dim3(BIAS_THREADS), 0, stream, observed, expected, scale, expected_out, b);
}

void launch_bias_lengths(const TxPool &pool, const int32_t *tx_windows, const double *b, int strand, const double *eff,
                         double *eff_out, int blocks, hipStream_t stream)
{
    if (pool.n_tx == 0) return;
    const double plus = strand == SKM_STRAND_NONE ? 0.5 : strand == SKM_STRAND_FR ? 1.0 : 0.0;
    hipLaunchKernelGGL(bias_lengths_kernel, dim3((unsigned)wave_grid(pool.n_tx, blocks)), dim3(BIAS_THREADS), 0, stream, pool,
                       tx_windows, b, plus, 1.0 - plus, eff, eff_out);
}

void launch_bias_expected_many(const TxPool &pool, const unsigned long long *tx_weight, int64_t n, int strand,
                               unsigned long long *expected, int blocks, hipStream_t stream)
{
    if (pool.n_tx == 0 || n <= 0) return;
    hipLaunchKernelGGL(bias_expected_many_kernel, dim3((unsigned)wave_grid(pool.n_tx, blocks), BIAS_LIMBS, (unsigned)n),
                       dim3(BIAS_THREADS), 0, stream, pool, tx_weight, strand != SKM_STRAND_RF ? 1 : 0,
                       strand != SKM_STRAND_FR ? 1 : 0, expected);
}

void launch_bias_weights_many(const unsigned long long *observed, const unsigned long long *expected, const double *scale,
                              int64_t n, double *expected_out, double *b, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(bias_weights_many_kernel, dim3((unsigned)n), dim3(BIAS_THREADS), 0, stream, observed, expected, scale,
                       expected_out, b);
}

void launch_bias_lengths_many(const TxPool &pool, const int32_t *tx_windows, const double *b, int64_t n, int strand,
                              const double *eff, double *eff_out, int blocks, hipStream_t stream)
{
    if (pool.n_tx == 0 || n <= 0) return;
    const double plus = strand == SKM_STRAND_NONE ? 0.5 : strand == SKM_STRAND_FR ? 1.0 : 0.0;
    constexpr int G = BIAS_LENGTHS_G;
    hipLaunchKernelGGL(bias_lengths_many_kernel<G>, dim3((unsigned)wave_grid(pool.n_tx, blocks), (unsigned)((n + G - 1) / G)),
                       dim3(BIAS_THREADS), 0, stream, pool, tx_windows, b, n, plus, 1.0 - plus, eff, eff_out);
}

}  // namespace skm
