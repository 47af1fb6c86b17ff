// The EM of /root/reference/seekmer/infer.py:133-168 for many class tables over the same transcripts
// in shared launches: the first-round quantification of the samples of a sample set, or of K tables of
// the caller's (skm_abi.hip: set_quant_group).
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
// The arithmetic is that of em_inner_kernel and em_rows_finalize_kernel<false> (skm_em.hip),
// association for association: tuple sums in tuple order with four gathers in flight, 8-lane rows with
// the xor 4, 2, 1 butterfly, row sums added in row order from 0.0, a / l_t / n, NaN -> 0, the
// relative-change flags.  A slot's result and step count do not depend on the grid that ran it, so they
// are bit for bit those of the single-table whole-table EM, which the tile EM is pinned to.
// No kernel waits for another block: the 2-D grids are not resident at once.
#include "skm_kernels.h"

#include <algorithm>

namespace skm {

namespace {

// (the verdict of em_evaluate, skm_em.hip, for one slot over its n_parts partials of step `steps_done`)
__device__ bool evaluate_slot(const EmSetProblem &p, EmSetSlot &d, int64_t steps_done)
{
    __shared__ double s_max[4];
    __shared__ unsigned int s_flags[4];
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
    for (int k = 32; k > 0; k >>= 1) {
        const double o = __shfl_xor(m, k, 64);
        m = o > m ? o : m;
        f |= __shfl_xor(f, k, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_max[wave] = m; s_flags[wave] = f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < 4; ++w) { m = s_max[w] > m ? s_max[w] : m; f |= s_flags[w]; }
        bool done;
        if (!(f & 1u)) {
            d.undefined = 1;                  // numpy raises on max() of an empty selection
            done = true;
        } else {
            done = (f & 2u) || !(m > p.rel_tol);                 // NaN propagates through max()
            if (p.max_iters > 0 && steps_done >= p.max_iters) done = true;
        }
        d.iters = (unsigned long long)steps_done;
        d.done = done ? 1ULL : 0ULL;
        s_done = done ? 1 : 0;
    }
    __syncthreads();
    return s_done != 0;
}

// eval > 0: the finalize pass before this launch (number `steps_done`) has not been judged yet
__global__ void __launch_bounds__(256)
em_set_inner_kernel(EmSetProblem p, int parity, int eval, int64_t steps_done)
{
    EmSetSlot &d = p.slots[blockIdx.y];
    const int64_t cls_first = d.cls_first, cls_end = d.cls_end;
    // (the first class's row is fetched before the verdict on the previous step is known)
    const int64_t c_first = cls_first + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t begin_first = 0, end_first = 0;
    double count_first = 1.0;
    if (c_first < cls_end) {
        begin_first = p.cls_offset[c_first];
        end_first = p.cls_offset[c_first + 1];
        count_first = p.cls_count[c_first];
    }
    if (eval > 0 && blockIdx.x == 0) {
        // block (0, s) judges slot s's step before this one and latches the verdict; the slot's other
        // blocks do not wait for it (see em_inner_kernel: a pass of `inner` that nobody reads)
        if (d.done) return;                     // (block-uniform)
        if (evaluate_slot(p, d, steps_done)) return;
    } else if (d.done) {
        return;
    }
    const double *__restrict__ x = p.x[parity];
    for (int64_t c = c_first; c < cls_end; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t begin = c == c_first ? begin_first : p.cls_offset[c];
        const int64_t end = c == c_first ? end_first : p.cls_offset[c + 1];
        const double count = c == c_first ? count_first : p.cls_count[c];
        double s = 0.0;
        int64_t j = begin;
        for (; j + 4 <= end; j += 4) {          // four independent gathers in flight, summed in order
            const int32_t t0 = p.ids[j], t1 = p.ids[j + 1], t2 = p.ids[j + 2], t3 = p.ids[j + 3];
            const double x0 = x[t0], x1 = x[t1], x2 = x[t2], x3 = x[t3];
            s += x0; s += x1; s += x2; s += x3;
        }
        for (; j < end; ++j) s += x[p.ids[j]];
        p.inner[c] = s / count;
    }
}

// em_rows_finalize_kernel<false> on the rows of slot blockIdx.y, with its many-row protocol: row sums
// cross blocks as agent-scope stores and loads, the store completed before the arrival is counted, and
// the group whose row arrives last adds the transcript's sums up in row order.
__global__ void __launch_bounds__(256, 8)
em_set_rows_finalize_kernel(EmSetProblem p, int parity)
{
    const EmSetSlot &d = p.slots[blockIdx.y];
    if (d.done) return;                         // (block-uniform: the freeze)
    __shared__ double s_max[4];
    __shared__ unsigned int s_flags[4];
    const double *__restrict__ x = p.x[parity];
    double *__restrict__ x_new = p.x[parity ^ 1];
    const int64_t row_end = d.row_end;
    const double n_total = d.n_total;
    const int sub = threadIdx.x & 7;
    double local_max = 0.0;
    unsigned int flags = 0;
    for (int64_t r = d.row_first + ((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3); r < row_end;
         r += ((int64_t)gridDim.x * blockDim.x) >> 3) {
        const int64_t begin = p.row_start[r], end = p.row_start[r + 1];
        const int32_t t = p.row_tx[r];
        const double xt = x[t];
        const int64_t first_row = p.tx_row[t], rows_of_t = p.tx_row[t + 1] - first_row;
        const double eff = p.eff_len[t];
        double s = 0.0;
        int64_t e = begin + sub;
        for (; e + 8 < end; e += 16) {          // two independent gathers in flight per lane
            const int32_t c0 = p.tx_cls[e], c1 = p.tx_cls[e + 8];
            const double i0 = p.inner[c0], i1 = p.inner[c1];
            s += xt / i0;
            s += xt / i1;
        }
        for (; e < end; e += 8) s += xt / p.inner[p.tx_cls[e]];
        s += __shfl_xor(s, 4, 8);
        s += __shfl_xor(s, 2, 8);
        s += __shfl_xor(s, 1, 8);
        // 1: the transcript's only row; 2: the last of its rows to arrive (this group adds them up); 0: neither
        int mode = 0;
        unsigned long long *const sums = reinterpret_cast<unsigned long long *>(p.row_sum);
        if (sub == 0) {
            if (rows_of_t == 1) {
                mode = 1;
            } else {
                __hip_atomic_store(&sums[r], (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned int before = atomicAdd(&p.arrivals[t], 1u);
                mode = (int64_t)before + 1 == rows_of_t ? 2 : 0;
            }
        }
        mode = __shfl(mode, 0, 8);
        if (mode == 0) continue;
        double a = 0.0;
        if (mode == 1) {
            a += s;
        } else {
            for (int64_t k0 = 0; k0 < rows_of_t; k0 += 8) {
                const int64_t k = k0 + sub;
                const double mine = k < rows_of_t
                    ? __longlong_as_double((long long)__hip_atomic_load(&sums[first_row + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    : 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const double v = __shfl(mine, j, 8);
                    if (k0 + j < rows_of_t) a += v;
                }
            }
            if (sub == 0) atomicExch(&p.arrivals[t], 0u);             // (for the next step)
        }
        if (sub != 0) continue;
        double v = a / eff / n_total;                                 // infer.py:158
        if (v != v) v = 0.0;                                          // infer.py:159
        x_new[t] = v;
        if (v > p.x_floor) {                                          // infer.py:160
            const double change = fabs(v - xt) / v;
            if (change != change) flags |= 2u;
            else if (change > local_max) local_max = change;
            flags |= 1u;
        }
    }
    for (int k = 32; k > 0; k >>= 1) {
        const double o = __shfl_xor(local_max, k, 64);
        local_max = o > local_max ? o : local_max;
        flags |= __shfl_xor(flags, k, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_max[wave] = local_max; s_flags[wave] = flags; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = s_max[0];
        unsigned int f = s_flags[0];
        for (int w = 1; w < 4; ++w) { m = s_max[w] > m ? s_max[w] : m; f |= s_flags[w]; }
        // (every block of a running slot writes its pair every step, one without rows too: the judge
        // reads all n_parts of them)
        p.part_max[(int64_t)blockIdx.y * p.n_parts + blockIdx.x] = m;
        p.part_flags[(int64_t)blockIdx.y * p.n_parts + blockIdx.x] = f;
    }
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
