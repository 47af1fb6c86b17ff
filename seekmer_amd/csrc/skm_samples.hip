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
