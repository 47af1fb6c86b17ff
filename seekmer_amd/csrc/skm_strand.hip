// Strand filter for strand-specific libraries (kallisto's --fr-stranded / --rf-stranded).
//
// The map kernel emits every unit's target entries SIGNED (seekmer/_common.pyx:143-179): e >= 0
// means mate 1 (or the single read) lies in transcript e's own orientation, e < 0 that it lies
// antisense to transcript ~e.  In a stranded mode a unit keeps the entries of the library's
// orientation, in their order, and its class key is recomputed over the kept unsigned ids with the
// map kernel's own seed and step (skm_kernels.h), so class counting runs on the filtered records
// unchanged.  The fragment length and the spans were recorded by the map kernel before this pass.
//
// One lane per record, grid-stride.  A record's entries are a short run of the arena (a few ids
// per unit); neighbouring records of a wave own neighbouring runs, so the lanes of a wave read one
// stretch of the arena.  The run is compacted in place from its own offset: no atomics, no other
// record's entries are touched.  A record whose entries all survive keeps its key and tuple word
// (the same tuple has the same key) and stores nothing.
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"

namespace skm {

__global__ void __launch_bounds__(256)
strand_filter_kernel(int32_t *entries, unsigned long long *rec_tuple, uint64_t *rec_key, int64_t n_records,
                     int keep_antisense)
{
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n_records;
         r += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long t = rec_tuple[r];
        const int n = (int)(t >> 40);
        if (n == 0) continue;
        const int64_t off = (int64_t)(t & ((1ULL << 40) - 1));
        int32_t *e = entries + off;
        int kept = 0;
        for (int i = 0; i < n; ++i) kept += (e[i] < 0) == (keep_antisense != 0);
        if (kept == n) continue;
        uint64_t key = tuple_key_seed(kept);
        int k = 0;
        for (int i = 0; i < n; ++i) {                 // (reads i before it writes k <= i)
            const int32_t v = e[i];
            if ((v < 0) != (keep_antisense != 0)) continue;
            e[k++] = v;
            key = tuple_key_step(key, (uint32_t)(v < 0 ? ~v : v));
        }
        if (key == 0) key = 1;
        rec_key[r] = kept ? key : 0;                  // 0: unaligned
        rec_tuple[r] = (unsigned long long)off | ((unsigned long long)kept << 40);
    }
}

void launch_strand_filter(const MapBatch &b, int mode, hipStream_t stream)
{
    if (b.n_units == 0 || mode == SKM_STRAND_NONE) return;
    int64_t blocks = (b.n_units + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(strand_filter_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, b.unit_entries,
                       b.rec_tuple, b.rec_key, b.n_units, mode == SKM_STRAND_RF ? 1 : 0);
}

}  // namespace skm
