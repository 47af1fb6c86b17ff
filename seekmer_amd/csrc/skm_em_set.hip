// The EM of /root/reference/seekmer/infer.py:133-168 for many class tables over the same transcripts
// in shared launches: the first-round quantification of the samples of a sample set, or of K tables of
// the caller's (skm_abi_quant.hip: set_quant_group).
//
// S tables over T transcripts are ONE block-diagonal problem: transcript t of table s is stacked
// transcript s * T + t, the classes are concatenated with their ids rebased by s * T, and no class
// couples two tables.  The set-up (skm_quant_setup.hip) keeps classes in (smallest transcript id,
// caller order) and cuts rows per transcript, so every table -- a SLOT here -- owns a contiguous class
// range and a contiguous row range, with the class order, tuple order and row cuts of a handle built
// for that table alone.  What is per slot is the total count, the stopping rule and the freeze:
//   - blockIdx.y is the slot; its descriptor (EmSetSlot) holds its ranges, its total and its control
//     words, its partials of the stopping rule are part_max / part_flags [slot][n_parts];
//   - a block reads its slot's `done` word first (block-uniform) and returns when it is set: a slot
//     that stopped after k steps keeps its result in x[k & 1], untouched, while the others go on;
//   - block (0, s) of the inner launch judges slot s's previous step, as block 0 of em_inner_kernel
//     does; a launch of one block per slot at every chunk end judges the chunk's last step and counts
//     the slots still running for the host's look-ahead loop.
// The kernels are em_inner_kernel and em_rows_finalize_kernel<false> (skm_em.hip) on a slot's ranges: the
// same bodies (skm_em_core.h) with another view.  A slot's result and step count do not depend on the
// grid that ran it, so they are bit for bit those of the single-table whole-table EM, which the tile EM
// is pinned to.
// No kernel waits for another block: the 2-D grids are not resident at once.
#include "skm_em_core.h"

#include <algorithm>

namespace skm {

namespace {

// (the verdict of em_evaluate, skm_em.hip, for one slot over its n_parts partials of step `steps_done`)
__device__ __forceinline__ bool evaluate_slot(const EmSetProblem &p, EmSetSlot &d, int64_t steps_done)
{
    __shared__ int s_done;
    const double *__restrict__ part_max = p.part_max + (int64_t)blockIdx.y * p.n_parts;
    const unsigned int *__restrict__ part_flags = p.part_flags + (int64_t)blockIdx.y * p.n_parts;
    double m = 0.0;
    unsigned int f = 0;
    for (int b = threadIdx.x; b < p.n_parts; b += blockDim.x) {
        const double o = part_max[b];
        m = o > m ? o : m;
        f |= part_flags[b];
    }
    if (em_block_reduce<1>(m, f)) {
        const EmVerdict verdict = em_stop_rule(f, m, p.rel_tol, steps_done, p.max_iters, 0);
        if (verdict.undefined) d.undefined = 1;
        d.iters = (unsigned long long)steps_done;
        d.done = verdict.done ? 1ULL : 0ULL;
        s_done = verdict.done ? 1 : 0;
    }
    __syncthreads();
    return s_done != 0;
}

// slot blockIdx.y of the set, as em_inner_body and em_rows_finalize_body see it (skm_em_core.h)
struct EmSlotView {
    const EmSetProblem &p;
    EmSetSlot &d;
    __device__ __forceinline__ int64_t cls_first() const { return d.cls_first; }
    __device__ __forceinline__ int64_t cls_end() const { return d.cls_end; }
    __device__ __forceinline__ int64_t row_first() const { return d.row_first; }
    __device__ __forceinline__ int64_t row_end() const { return d.row_end; }
    __device__ __forceinline__ double n_total() const { return d.n_total; }
    __device__ __forceinline__ bool done() const { return d.done != 0; }           // (the freeze)
    // block (0, s) judges slot s's step before this one; the slot's other blocks do not wait for it
    __device__ __forceinline__ bool judge(int, int64_t steps_done) const { return evaluate_slot(p, d, steps_done); }
    __device__ __forceinline__ int64_t part() const { return (int64_t)blockIdx.y * p.n_parts + blockIdx.x; }
};

// eval > 0: the finalize pass before this launch (number `steps_done`) has not been judged yet
__global__ void __launch_bounds__(256)
em_set_inner_kernel(EmSetProblem p, int parity, int eval, int64_t steps_done)
{
    em_inner_body(p, EmSlotView{p, p.slots[blockIdx.y]}, parity, eval > 0 && blockIdx.x == 0, eval, steps_done, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                  (int64_t)gridDim.x * blockDim.x);
}

__global__ void __launch_bounds__(256, 8)
em_set_rows_finalize_kernel(EmSetProblem p, int parity)
{
    em_rows_finalize_body<false>(p, EmSlotView{p, p.slots[blockIdx.y]}, parity, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                                 (int64_t)gridDim.x * blockDim.x);
}

// one block per slot: the chunk's last step judged; *running counts the slots that go on
__global__ void __launch_bounds__(256)
em_set_decide_kernel(EmSetProblem p, int64_t steps_done, unsigned long long *running)
{
    EmSetSlot &d = p.slots[blockIdx.y];
    if (d.done) return;
    if (!evaluate_slot(p, d, steps_done) && threadIdx.x == 0) atomicAdd(running, 1ULL);
}

// out[s][t] = the abundance slot s stopped with: x[iters & 1][s * T + t]; zeros for a slot without classes
__global__ void __launch_bounds__(256)
em_set_result_kernel(const EmSetSlot *__restrict__ slots, const double *__restrict__ x0, const double *__restrict__ x1,
                     int64_t n_tx, double *__restrict__ out)
{
    const EmSetSlot &d = slots[blockIdx.y];
    const bool empty = d.cls_end == d.cls_first;
    const double *__restrict__ x = ((d.iters & 1ULL) ? x1 : x0) + (int64_t)blockIdx.y * n_tx;
    double *__restrict__ to = out + (int64_t)blockIdx.y * n_tx;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tx; t += (int64_t)gridDim.x * blockDim.x)
        to[t] = empty ? 0.0 : x[t];
}

// ids[dst[k] + j] = arena[src[k] + j] + add[k], j < len[k]: the tuples of the set's classes, in the stacked
// problem's class order, on their way from the shared table's arena to the stacked id space
__global__ void __launch_bounds__(256)
stack_tuples_kernel(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const int32_t *__restrict__ add,
                    int64_t n_classes, const int32_t *__restrict__ arena, int32_t *__restrict__ ids)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n_classes; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t from = src[k], to = dst[k], n = dst[k + 1] - to;
        const int32_t base = add[k];
        for (int64_t j = 0; j < n; ++j) ids[to + j] = arena[from + j] + base;
    }
}

// rows 1 .. n - 1 of x[n][n_tx] = row 0
__global__ void __launch_bounds__(256)
repeat_row_kernel(double *__restrict__ x, int64_t n_tx)
{
    double *__restrict__ to = x + (int64_t)(blockIdx.y + 1) * n_tx;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tx; t += (int64_t)gridDim.x * blockDim.x)
        to[t] = x[t];
}

inline unsigned blocks_of(int64_t items, int per_block, int64_t cap)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    if (blocks < 1) blocks = 1;
    if (blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

}  // namespace

int em_set_parts(int64_t largest_rows)
{
    return (int)blocks_of(largest_rows, 32, EM_FINAL_BLOCKS);
}

void launch_em_set_step(const EmSetProblem &p, int64_t largest_classes, int64_t step, bool judge_previous, hipStream_t stream)
{
    const int parity = (int)(step & 1);
    hipLaunchKernelGGL(em_set_inner_kernel, dim3(blocks_of(largest_classes, 256, 256 * 8), (unsigned)p.n_slots), dim3(256), 0,
                       stream, p, parity, judge_previous ? 1 : 0, step);
    hipLaunchKernelGGL(em_set_rows_finalize_kernel, dim3((unsigned)p.n_parts, (unsigned)p.n_slots), dim3(256), 0, stream, p,
                       parity);
}

void launch_em_set_decide(const EmSetProblem &p, int64_t steps_done, unsigned long long *running, hipStream_t stream)
{
    hipLaunchKernelGGL(em_set_decide_kernel, dim3(1, (unsigned)p.n_slots), dim3(256), 0, stream, p, steps_done, running);
}

void launch_em_set_result(const EmSetSlot *slots, int n_slots, const double *x0, const double *x1, int64_t n_tx, double *out,
                          hipStream_t stream)
{
    hipLaunchKernelGGL(em_set_result_kernel, dim3(blocks_of(n_tx, 256, 64), (unsigned)n_slots), dim3(256), 0, stream, slots,
                       x0, x1, n_tx, out);
}

void launch_stack_tuples(const int64_t *src, const int64_t *dst, const int32_t *add, int64_t n_classes, const int32_t *arena,
                         int32_t *ids, hipStream_t stream)
{
    if (n_classes <= 0) return;
    hipLaunchKernelGGL(stack_tuples_kernel, dim3(blocks_of(n_classes, 256, 256 * 8)), dim3(256), 0, stream, src, dst, add,
                       n_classes, arena, ids);
}

void launch_repeat_row(double *x, int64_t n_tx, int64_t n, hipStream_t stream)
{
    if (n <= 1 || n_tx <= 0) return;
    hipLaunchKernelGGL(repeat_row_kernel, dim3(blocks_of(n_tx, 256, 64), (unsigned)(n - 1)), dim3(256), 0, stream, x, n_tx);
}

void warm_code_em_set()
{
    hipFuncAttributes attributes;
    (void)hipFuncGetAttributes(&attributes, reinterpret_cast<const void *>(&em_set_inner_kernel));
}

}  // namespace skm
