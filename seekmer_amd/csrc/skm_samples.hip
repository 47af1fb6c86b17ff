// Sample sets: the units of many small samples (single cells) mapped in shared launches into ONE
// class table in which a class is the pair (sample, target tuple).
//
// The map kernel and the class kernels know nothing of samples.  A launch of a set is a list of
// segments (runs of consecutive units of one sample, back to back); between the map kernel (and the
// strand filter) and class counting, sample_salt_kernel replaces every record's 64-bit tuple key by the
// key of (sample, tuple) = key + sample * SAMPLE_KEY_STEP (mod 2^64).  The step is odd, so for one
// tuple key different samples give different keys: two samples that hold the same tuple never share a
// slot, and two DIFFERENT tuples that do meet in a slot are caught by the class kernels' full tuple
// compare as before (SKM_ERR_COLLISION) -- counts are exact or the call fails.  A salted key of 0
// (2^-64 per record) would read as "unaligned": it raises the same error instead.
//
// A set that keeps one fragment-length histogram per sample maps with keep_spans and runs
// sample_fld_kernel after every launch: the units' final spans, through the map kernel's fragment length
// rule, counted into the row of the unit's sample.
//
// A set that counts hexamers (--bias, skm_sample_set_keep_bias) runs sample_bias_kernel where a mapper runs
// bias_observed_kernel (skm_bias.hip): the same rule, the count going into the row of the unit's sample.
//
// At export, sample_assign_kernel gives every class its sample and its first-seen unit counted inside
// that sample from the set's segment log (global first unit, sample, local first unit of every
// segment, in launch order).
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"

namespace skm {

// One lane per record, grid-stride.  The launch's segment table (at most SAMPLE_LAUNCH_SEGMENTS
// entries, 16 KB) is copied to LDS once per block and searched by bisection: 11 LDS reads per record
// at most, against three streamed words of HBM.
__global__ void __launch_bounds__(256)
sample_salt_kernel(const int32_t *__restrict__ rec_unit, uint64_t *__restrict__ rec_key, int64_t n_records,
                   const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_sample, int n_segments,
                   int *error)
{
    __shared__ int32_t s_first[SAMPLE_LAUNCH_SEGMENTS], s_sample[SAMPLE_LAUNCH_SEGMENTS];
    for (int i = threadIdx.x; i < n_segments; i += blockDim.x) { s_first[i] = seg_first[i]; s_sample[i] = seg_sample[i]; }
    __syncthreads();
    bool zero = false;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n_records;
         r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = rec_key[r];
        if (key == 0) continue;                       // empty tuple: unaligned whatever the sample
        const int64_t seg = segment_find(s_first, n_segments, rec_unit[r]);
        const uint32_t sample = (uint32_t)s_sample[seg];
        if (sample == 0) continue;                    // (key + 0)
        const uint64_t salted = sample_key(key, sample);
        zero |= salted == 0;
        rec_key[r] = salted;
    }
    if (zero) atomicExch(error, SKM_ERR_COLLISION);
}

// Fragment lengths by sample.  A block takes SAMPLE_FLD_RUN consecutive units, 256 at a time.  A sample's
// units are consecutive, so most tiles of 256 lie inside one segment: those count the bins below
// SAMPLE_FLD_WINDOW in an LDS histogram that the block flushes (one 64-bit atomic per occupied bin) when its
// sample changes and at the end.  A tile that crosses a segment border (many tiny samples) and the rare long
// fragments add straight to HBM: neighbouring lanes then hit different rows or far bins.  Integer adds:
// any order gives the same histogram.
constexpr int SAMPLE_FLD_WINDOW = 512;            // (the map kernel's FLD_WINDOW)
constexpr int SAMPLE_FLD_RUN = 1024;

__global__ void __launch_bounds__(256)
sample_fld_kernel(const int32_t *__restrict__ unit_begin, const int32_t *__restrict__ unit_end, int64_t n_units,
                  const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_sample, int n_segments,
                  unsigned long long *__restrict__ hist)
{
    __shared__ int32_t s_first[SAMPLE_LAUNCH_SEGMENTS], s_sample[SAMPLE_LAUNCH_SEGMENTS];
    __shared__ uint32_t s_hist[SAMPLE_FLD_WINDOW];
    for (int i = threadIdx.x; i < n_segments; i += blockDim.x) { s_first[i] = seg_first[i]; s_sample[i] = seg_sample[i]; }
    for (int i = threadIdx.x; i < SAMPLE_FLD_WINDOW; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
    const int64_t run_first = (int64_t)blockIdx.x * SAMPLE_FLD_RUN;
    const int64_t run_end = run_first + SAMPLE_FLD_RUN < n_units ? run_first + SAMPLE_FLD_RUN : n_units;
    int64_t held = -1;                            // the sample whose counts s_hist holds (block-uniform)
    auto flush = [&]() {                          // (called by the whole block)
        __syncthreads();
        for (int i = threadIdx.x; i < SAMPLE_FLD_WINDOW; i += blockDim.x)
            if (s_hist[i]) {
                atomicAdd(&hist[held * MAX_FRAGMENT_LENGTH + i], (unsigned long long)s_hist[i]);
                s_hist[i] = 0;
            }
        __syncthreads();
    };
    for (int64_t tile = run_first; tile < run_end; tile += blockDim.x) {
        const int64_t tile_last = tile + blockDim.x <= run_end ? tile + blockDim.x - 1 : run_end - 1;
        const int64_t seg_a = segment_find(s_first, n_segments, tile), seg_b = segment_find(s_first, n_segments, tile_last);
        const bool one_segment = seg_a == seg_b;  // (block-uniform: both units are the tile's)
        if (one_segment && held != s_sample[seg_a]) {
            if (held >= 0) flush();
            held = s_sample[seg_a];
        }
        const int64_t u = tile + threadIdx.x;
        if (u > tile_last) continue;
        // fragment length rule, _mapper.pyx:90-94, on the span the map kernel stored for the unit
        int length = unit_end[u] - unit_begin[u] + K;
        if (length <= 0) continue;
        if (length >= MAX_FRAGMENT_LENGTH) length = MAX_FRAGMENT_LENGTH - 1;
        if (one_segment && length < SAMPLE_FLD_WINDOW) { atomicAdd(&s_hist[length], 1u); continue; }
        const int64_t sample = one_segment ? held : (int64_t)s_sample[segment_find(s_first, n_segments, u)];
        atomicAdd(&hist[sample * MAX_FRAGMENT_LENGTH + length], 1ULL);
    }
    if (held >= 0) flush();
}

// First hexamers by sample: the rule of bias_observed_kernel (skm_bias.hip), counted into rows[sample][4096].
// Records are not in unit order, but a block of the map kernel owns a range of units and writes their records
// into the same range, so neighbouring records are mostly one sample's.  A block takes SAMPLE_BIAS_RUN
// consecutive records, 256 at a time.  A tile whose records all belong to one sample (a block-wide vote) counts
// in a 4096-bin LDS histogram that the block flushes, one 64-bit atomic per occupied bin, when that sample
// changes and at the end; a mixed tile adds straight to HBM.  An LDS bin holds at most SAMPLE_BIAS_RUN < 2^32
// counts between flushes; a row word is 64 bits wide.  Integer adds only: the rows do not depend on the grid, on
// the cut into launches or on the order of arrival.
constexpr int SAMPLE_BIAS_RUN = 4096;
constexpr int SAMPLE_BIAS_BINS = 4096;            // (BIAS_BINS of skm_bias.h)
constexpr int SAMPLE_BIAS_HEXAMER = 6;

__global__ void __launch_bounds__(256)
sample_bias_kernel(const uint32_t *__restrict__ records, int record_words, int words_per_read, int paired,
                   const unsigned long long *__restrict__ rec_tuple, const int32_t *__restrict__ rec_unit,
                   int64_t n_records, const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_sample,
                   int n_segments, unsigned long long *__restrict__ rows)
{
    __shared__ int32_t s_first[SAMPLE_LAUNCH_SEGMENTS], s_sample[SAMPLE_LAUNCH_SEGMENTS];
    __shared__ uint32_t s_bins[SAMPLE_BIAS_BINS];
    __shared__ int32_t s_ref;
    for (int i = threadIdx.x; i < n_segments; i += blockDim.x) { s_first[i] = seg_first[i]; s_sample[i] = seg_sample[i]; }
    for (int i = threadIdx.x; i < SAMPLE_BIAS_BINS; i += blockDim.x) s_bins[i] = 0;
    __syncthreads();
    const int64_t run_first = (int64_t)blockIdx.x * SAMPLE_BIAS_RUN;
    const int64_t run_end = run_first + SAMPLE_BIAS_RUN < n_records ? run_first + SAMPLE_BIAS_RUN : n_records;
    int64_t held = -1;                            // the sample whose counts s_bins holds (block-uniform)
    auto flush = [&]() {                          // (called by the whole block)
        __syncthreads();
        for (int i = threadIdx.x; i < SAMPLE_BIAS_BINS; i += blockDim.x)
            if (s_bins[i]) {
                atomicAdd(&rows[held * SAMPLE_BIAS_BINS + i], (unsigned long long)s_bins[i]);
                s_bins[i] = 0;
            }
        __syncthreads();
    };
    for (int64_t tile = run_first; tile < run_end; tile += blockDim.x) {
        const int64_t r = tile + threadIdx.x;
        const bool mine = r < run_end;
        const int64_t unit = mine ? (int64_t)rec_unit[r] : 0;
        const int32_t sample = mine ? s_sample[segment_find(s_first, n_segments, unit)] : -1;
        if (threadIdx.x == 0) s_ref = sample;     // (the tile's first record exists)
        __syncthreads();
        const int32_t ref = s_ref;
        const bool one_sample = __syncthreads_and(!mine || sample == ref) != 0;      // block-uniform
        if (one_sample && held != ref) {
            if (held >= 0) flush();
            held = ref;
        }
        if (!mine || (rec_tuple[r] >> 40) == 0) continue;                  // unaligned (after the strand filter)
        const uint32_t *record = records + unit * (paired ? 2 : 1) * record_words;   // mate 1, or the single read
        if (record[3 * words_per_read] < (uint32_t)SAMPLE_BIAS_HEXAMER) continue;
        if ((record[2 * words_per_read] >> (32 - SAMPLE_BIAS_HEXAMER)) != (1u << SAMPLE_BIAS_HEXAMER) - 1u) continue;
        const uint32_t h = (uint32_t)(*reinterpret_cast<const uint64_t *>(record) >> (64 - 2 * SAMPLE_BIAS_HEXAMER));
        if (one_sample) atomicAdd(&s_bins[h], 1u);
        else atomicAdd(&rows[(int64_t)sample * SAMPLE_BIAS_BINS + h], 1ULL);
    }
    if (held >= 0) flush();
}

__global__ void __launch_bounds__(256)
sample_assign_kernel(const int64_t *__restrict__ log_global, const int64_t *__restrict__ log_local,
                     const int32_t *__restrict__ log_sample, int64_t n_segments,
                     const unsigned long long *__restrict__ cls_first_seen, int64_t n_classes,
                     int32_t *__restrict__ cls_sample, int64_t *__restrict__ cls_local)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n_classes;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t unit = (int64_t)cls_first_seen[k];
        const int64_t seg = segment_find(log_global, n_segments, unit);
        cls_sample[k] = log_sample[seg];
        cls_local[k] = log_local[seg] + (unit - log_global[seg]);
    }
}

void launch_sample_salt(const MapBatch &b, const SampleSalt &salt, int *error, hipStream_t stream)
{
    if (b.n_units == 0 || salt.n_segments <= 0) return;
    int64_t blocks = (b.n_units + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sample_salt_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, b.rec_unit, b.rec_key,
                       b.n_units, salt.seg_first, salt.seg_sample, (int)salt.n_segments, error);
}

void launch_sample_fld(const int32_t *unit_begin, const int32_t *unit_end, int64_t n_units, const SampleSalt &salt,
                       unsigned long long *hist, hipStream_t stream)
{
    if (n_units <= 0 || salt.n_segments <= 0) return;
    const int64_t blocks = (n_units + SAMPLE_FLD_RUN - 1) / SAMPLE_FLD_RUN;        // (at most 2^21 units a launch)
    hipLaunchKernelGGL(sample_fld_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, unit_begin, unit_end,
                       n_units, salt.seg_first, salt.seg_sample, (int)salt.n_segments, hist);
}

void launch_sample_bias(const MapBatch &b, const SampleSalt &salt, unsigned long long *rows, hipStream_t stream)
{
    if (b.n_units <= 0 || salt.n_segments <= 0) return;
    const int64_t blocks = (b.n_units + SAMPLE_BIAS_RUN - 1) / SAMPLE_BIAS_RUN;      // (at most 2^21 units a launch)
    hipLaunchKernelGGL(sample_bias_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, b.records, b.record_words,
                       b.words_per_read, b.paired, b.rec_tuple, b.rec_unit, b.n_units, salt.seg_first, salt.seg_sample,
                       (int)salt.n_segments, rows);
}

void launch_sample_assign(const int64_t *log_global, const int64_t *log_local, const int32_t *log_sample,
                          int64_t n_segments, const unsigned long long *cls_first_seen, int64_t n_classes,
                          int32_t *cls_sample, int64_t *cls_local, hipStream_t stream)
{
    if (n_classes == 0 || n_segments == 0) return;
    int64_t blocks = (n_classes + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sample_assign_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, log_global, log_local,
                       log_sample, n_segments, cls_first_seen, n_classes, cls_sample, cls_local);
}

}  // namespace skm
