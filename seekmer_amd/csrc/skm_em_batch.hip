// The EM of /root/reference/seekmer/infer.py:133-168 for EM_BATCH problems at once that share
// their class structure and differ only in the class counts (and with them the total) and the
// abundance vector.  Three callers have problems of that shape (skm_abi_quant.hip: em_group_run):
//   - the bootstrap replicates of `-b N` (infer.py:79-82, 108-111 -- every replicate resamples the
//     counts of the SAME class table and starts from the same estimate; all totals are equal),
//   - K count vectors of the caller's on one class table (skm_quant_em_many),
//   - the second round of `impute` (impute.py:229-252: the concatenation of all cells' classes,
//     blended for each cell in turn -- skm_quant_em_blend; blend_counts_kernel below makes the
//     counts where they are used).
// "Replicate" below means any such problem.
//
// A single problem's step is three launches of 5-13 us that move 8 useful bytes per 64-byte
// sector they gather (x[t] per (class, transcript) pair, inner[c] per pair the other way round),
// and a replicate takes ~30 of them: run one by one, a third of the time is gaps between
// launches.  Here the replicates sit side by side -- x[t][r], inner[c][r], count[c][r], r = 0..7
// -- so that one gathered sector carries all eight, the index arrays are read once for the
// eight, and there is one launch where there were eight.
//
// Every replicate still runs ITS OWN iteration: the step's arithmetic is the single-problem kernels'
// (skm_em_core.h, with the replicates as a stride), its total divides its own numerators (place_total),
// the stopping rule (infer.py:160) is judged per replicate, and a replicate that has stopped is
// frozen (its x is carried from buffer to buffer unchanged) while the others go on, so its result
// and its step count are exactly what the one-by-one run gives -- bit for bit
// (tests/test_gpu_parity.py::test_bootstrap_draw_and_em, tests/test_gpu_em_many.py).
#include "skm_em_core.h"

#include <algorithm>

namespace skm {

namespace {

constexpr int R = EM_BATCH;
static_assert(R == 8, "the row sums pair lanes and replicates eight by eight");

// The stopping rule for each replicate over the partials of finalize pass `steps_done`; returns
// the mask of replicates that have stopped (now or earlier).  Block 0 of the next em_inner launch
// evaluates it; with `publish` it latches what is new.
__device__ unsigned int evaluate_batch(const EmBatchProblem &p, int n_parts, int64_t steps_done, bool publish)
{
    __shared__ double s_max[32][R];
    __shared__ unsigned int s_flags[32][R];
    __shared__ unsigned int s_mask;
    const int r = threadIdx.x & (R - 1), g = threadIdx.x >> 3;        // 256 lanes: 32 groups x 8 replicates
    double m = 0.0;
    unsigned int f = 0;
    for (int b = g; b < n_parts; b += 32) {
        const double o = p.part_max[b * R + r];
        m = o > m ? o : m;
        f |= p.part_flags[b * R + r];
    }
    s_max[g][r] = m;
    s_flags[g][r] = f;
    if (threadIdx.x == 0) s_mask = 0;
    __syncthreads();
    if (threadIdx.x < R) {
        for (int k = 0; k < 32; ++k) {
            m = s_max[k][r] > m ? s_max[k][r] : m;
            f |= s_flags[k][r];
        }
        const bool latched = p.ctl[BCTL_DONE + r] != 0;
        const EmVerdict verdict = em_stop_rule(f, m, p.rel_tol, steps_done, 0, 0);
        const bool done = verdict.done;
        if (publish && !latched && done) {
            if (verdict.undefined) p.ctl[BCTL_UNDEFINED + r] = 1;
            p.ctl[BCTL_ITERS + r] = (unsigned long long)steps_done;
            p.ctl[BCTL_DONE + r] = 1;
        }
        if (latched || done) atomicOr(&s_mask, 1u << r);
    }
    __syncthreads();
    const unsigned int mask = s_mask;
    // (who says "all done": the judge when the host fills the places -- nothing new can come before it
    // looks --, the assign kernel when the device does: a place that stops is refilled in the same step)
    if (publish && !p.managed && threadIdx.x == 0 && mask == (1u << R) - 1u && !p.ctl[BCTL_ALL_DONE]) {
        p.ctl[BCTL_LAST_STEP] = (unsigned long long)steps_done;
        p.ctl[BCTL_ALL_DONE] = 1;
    }
    return mask;
}

// What a latched stop means, place by place (one lane): the replicate's step count is recorded, its
// result is to be taken, the next replicate of the group (if any) is to be put in its place; the plan
// goes to mgr[MGR_TAKE ..], mgr[MGR_PUT ..] for em_batch_refill.  `deferred`: called from inside a step
// (block 0 of em_inner_batch, right after it has judged the step before), where the control block
// must stay as the step's other kernels read it -- a stopped place has to be carried through the
// step's finalize pass -- so the control words of a refilled place and the "all done" latch are
// left to em_batch_refill, which runs behind the step.
__device__ void plan_places(const EmBatchProblem &p, unsigned long long *mgr, int64_t *iters_out, int64_t step, bool deferred)
{
    bool any = false;
    for (int r = 0; r < R; ++r) {
        unsigned long long take = 0, put = 0;
        if (mgr[MGR_REP + r] != 0 && p.ctl[BCTL_DONE + r]) {
            const unsigned long long rep = mgr[MGR_REP + r] - 1;
            if (iters_out) iters_out[rep] = (int64_t)(p.ctl[BCTL_ITERS + r] - mgr[MGR_SINCE + r]);
            if (p.ctl[BCTL_UNDEFINED + r]) mgr[MGR_UNDEFINED] = 1;
            take = rep + 1;
            mgr[MGR_FINISHED] += 1;
            if (mgr[MGR_NEXT] < mgr[MGR_COUNT]) {
                put = ++mgr[MGR_NEXT];                              // (replicate mgr[MGR_NEXT] - 1, + 1)
                mgr[MGR_REP + r] = put;
                mgr[MGR_SINCE + r] = (unsigned long long)(step + 1);
                if (!deferred) {
                    p.ctl[BCTL_DONE + r] = 0;
                    p.ctl[BCTL_UNDEFINED + r] = 0;
                    p.ctl[BCTL_ITERS + r] = 0;
                }
            } else {
                mgr[MGR_REP + r] = 0;                               // idle from now on (it stays "stopped")
            }
        }
        mgr[MGR_TAKE + r] = take;
        mgr[MGR_PUT + r] = put;
        any |= mgr[MGR_REP + r] != 0;
    }
    if (!any && !deferred) {
        p.ctl[BCTL_LAST_STEP] = (unsigned long long)(step + 1);
        p.ctl[BCTL_ALL_DONE] = 1;
    }
}

__global__ void __launch_bounds__(256)
em_inner_batch_kernel(EmBatchProblem p, int parity, int eval_parts, int64_t steps_done)
{
    __shared__ int s_all;
    if (threadIdx.x == 0) s_all = p.ctl[BCTL_ALL_DONE] != 0;       // one reading per block
    __syncthreads();
    if (s_all) return;
    // block 0 judges the step before this one and latches what has stopped; the other blocks do not
    // wait (see em_inner_kernel: a pass of `inner` nobody reads, once per batch)
    if (eval_parts > 0 && blockIdx.x == 0
            && evaluate_batch(p, eval_parts, steps_done, true) == (1u << R) - 1u && !p.managed) return;
    // the device-managed working set: what has just been latched is planned for at once (the launch
    // of its own that used to do this after every step is gone); em_batch_refill carries it out
    if (p.managed && p.mgr && blockIdx.x == 0 && threadIdx.x == 0) plan_places(p, p.mgr, p.iters_out, steps_done, true);
    // R lanes per class, lane r = replicate r: the R lanes of a class read one 64-byte sector of x per
    // id together and four ids are in flight per lane (one lane per class with the replicates in
    // registers had ONE dependent 64-byte gather in flight per lane: 86 us per step against 50 for the
    // rows); every (class, replicate) sum still adds its ids in list order, as the single-problem
    // kernel does.  (The rows kernel the same way -- a wave per row, lane = entry residue x replicate --
    // was measured too: 97 ms per 100 replicates instead of 89; it keeps eight lanes per row.)
    const double *__restrict__ x = p.x[parity];
    const int r = threadIdx.x & (R - 1);
    for (int64_t c = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / R; c < p.n_classes;
         c += ((int64_t)gridDim.x * blockDim.x) / R) {
        p.inner[c * R + r] = em_tuple_sum<R>(p.ids, p.cls_offset[c], p.cls_offset[c + 1], x, r) / p.cls_count[c * R + r];
    }
}

__global__ void __launch_bounds__(256)
em_rows_batch_kernel(EmBatchProblem p, int parity)
{
    if (p.ctl[BCTL_ALL_DONE]) return;
    const double *__restrict__ x = p.x[parity];
    const int sub = threadIdx.x & 7;
    for (int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3; row < p.n_rows;
         row += ((int64_t)gridDim.x * blockDim.x) >> 3) {
        double xr[R], s[R];
        em_row_sums<R>(p.tx_cls, p.inner, p.row_start[row], p.row_start[row + 1], sub, x + (int64_t)p.row_tx[row] * R, xr, s);
        if (sub == 0) {
            double *__restrict__ out = p.row_sum + row * R;
#pragma unroll
            for (int r = 0; r < R; ++r) out[r] = s[r];
        }
    }
}

// x'_t of one (transcript, place): a stopped replicate keeps its result and notes no change
__device__ __forceinline__ void finalize_place(double a, double eff, double n_total, bool stopped, double before, double x_floor,
                                               double &x_new, double &local_max, unsigned int &flags)
{
    const double v = em_new_abundance(a, eff, n_total);
    if (stopped) {
        x_new = before;
    } else {
        x_new = v;
        em_note_change(v, before, x_floor, local_max, flags);
    }
}

// the block's partials of place r (lane i holds those of place i % R)
__device__ __forceinline__ void write_partials(const EmBatchProblem &p, int r, bool stopped, double m, unsigned int f)
{
    if (!em_block_reduce<R>(m, f)) return;
    // a frozen replicate reports "selected, no change": it stays stopped whatever is judged
    if (stopped) { m = 0.0; f = 1u; }
    p.part_max[blockIdx.x * R + r] = m;
    p.part_flags[blockIdx.x * R + r] = f;
}

__global__ void __launch_bounds__(256)
em_finalize_batch_kernel(EmBatchProblem p, int parity)
{
    if (p.ctl[BCTL_ALL_DONE]) return;
    // R lanes per transcript, lane r = replicate r (as in em_inner_batch): a lane follows ONE chain of
    // dependent loads instead of eight, and there are eight times the lanes to hide it.  The
    // arithmetic per (transcript, replicate) is unchanged; maxima and flags do not care about order.
    const double *__restrict__ x_old = p.x[parity];
    double *__restrict__ x_new = p.x[parity ^ 1];
    const int r = threadIdx.x & (R - 1);
    const bool stopped = p.ctl[BCTL_DONE + r] != 0;           // this lane's replicate is frozen
    const double n_total = p.place_total[r];                  // ... and this is the sum of its class counts
    double local_max = 0.0;
    unsigned int flags = 0;
    for (int64_t t = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / R; t < p.n_tx;
         t += ((int64_t)gridDim.x * blockDim.x) / R) {
        const double a = em_rows_stored_sum<R>(p.row_sum, p.tx_row[t], p.tx_row[t + 1], r);
        finalize_place(a, p.eff_len[t], n_total, stopped, x_old[t * R + r], p.x_floor, x_new[t * R + r], local_max, flags);
    }
    write_partials(p, r, stopped, local_max, flags);
}

// em_rows_batch and em_finalize_batch in ONE launch (skm_em.hip: em_rows_finalize_kernel is the
// single-problem form).  After the row's eight partial sums have been combined every lane of the
// 8-lane group holds all eight replicates' row sums; lane r finalizes replicate r of the row's
// transcript -- all eight lanes busy, with em_finalize_batch_kernel's arithmetic (a = 0.0 + row sum)
// -- when the transcript has this one row (every transcript of the benchmarked tables has), and for a
// transcript of several rows the group whose row arrives last adds them up in row order.
__global__ void __launch_bounds__(256)
em_rows_finalize_batch_kernel(EmBatchProblem p, int parity)
{
    if (p.ctl[BCTL_ALL_DONE]) return;
    const double *__restrict__ x = p.x[parity];
    double *__restrict__ x_new = p.x[parity ^ 1];
    const int sub = threadIdx.x & 7;
    const bool stopped = p.ctl[BCTL_DONE + sub] != 0;          // this lane's replicate (r = sub) is frozen
    const double n_total = p.place_total[sub];                 // ... and this is the sum of its class counts
    double local_max = 0.0;
    unsigned int flags = 0;
    for (int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3; row < p.n_rows;
         row += ((int64_t)gridDim.x * blockDim.x) >> 3) {
        const int64_t begin = p.row_start[row], end = p.row_start[row + 1];
        const int32_t t = p.row_tx[row];
        const int64_t first_row = p.tx_row[t], rows_of_t = p.tx_row[t + 1] - first_row;
        const double eff = p.eff_len[t];
        double xr[R], s[R];
        em_row_sums<R>(p.tx_cls, p.inner, begin, end, sub, x + (int64_t)t * R, xr, s);
        double mine = s[0], before = xr[0];                    // replicate `sub` of this row
#pragma unroll
        for (int r = 1; r < R; ++r) { mine = sub == r ? s[r] : mine; before = sub == r ? xr[r] : before; }
        double a = 0.0;
        if (rows_of_t == 1) {
            a += mine;
        } else {
            // every lane publishes its replicate's sum; lane 0 counts the row's arrival for the group
            const unsigned int arrived = __shfl(em_row_publish(p.row_sum, row * R + sub, mine, &p.arrivals[t], sub == 0), 0, 8);
            if ((int64_t)arrived != rows_of_t) continue;          // another row of this transcript is still to come
            a = em_rows_published_sum<R>(p.row_sum, first_row, rows_of_t, sub);
            if (sub == 0) em_row_arrivals_reset(&p.arrivals[t]);
        }
        finalize_place(a, eff, n_total, stopped, before, p.x_floor, x_new[(int64_t)t * R + sub], local_max, flags);
    }
    write_partials(p, sub, stopped, local_max, flags);
}

__global__ void __launch_bounds__(256)
em_decide_batch_kernel(EmBatchProblem p, int n_parts, int64_t steps_done)
{
    __shared__ int s_all;
    if (threadIdx.x == 0) s_all = p.ctl[BCTL_ALL_DONE] != 0;
    __syncthreads();
    if (s_all) return;
    evaluate_batch(p, n_parts, steps_done, true);
}

// out[t] = x[t][r]
__global__ void __launch_bounds__(256)
em_batch_take_kernel(const double *__restrict__ x, int64_t n_tx, int r, double *__restrict__ out)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_tx;
         i += (int64_t)gridDim.x * blockDim.x) out[i] = x[i * R + r];
}

// ---- the working set kept full by the device (`-b N`): after every step one small kernel decides,
// place by place, what a latched stop means -- the replicate's step count is recorded, its result is
// to be taken, the next replicate of the group (if any) is to be put in its place -- and a grid-wide
// kernel carries the plan out: result out, pre-drawn class counts and the common start vector in,
// the place's partials of "the step before" set to "still changing".  The host only queues steps
// and looks now and then whether everything has finished.  (mgr: the MGR_ words of skm_kernels.h)
__global__ void em_batch_assign_kernel(EmBatchProblem p, unsigned long long *mgr, int64_t *iters_out, int64_t step)
{
    if (threadIdx.x != 0 || p.ctl[BCTL_ALL_DONE]) return;
    plan_places(p, mgr, iters_out, step, false);
}

// the plan carried out; `into` = the abundance buffer the NEXT step reads (a stopped replicate's
// result is carried there by the finalize pass of this step).  A place's total comes in with its counts.
__global__ void __launch_bounds__(256)
em_batch_refill_kernel(EmBatchProblem p, const unsigned long long *__restrict__ mgr, const double *__restrict__ counts_all,
                       const double *__restrict__ totals, const double *__restrict__ x_start, double *__restrict__ out_all,
                       double *__restrict__ into, int64_t step)
{
    __shared__ unsigned long long plan[2 * R];
    if (threadIdx.x < 2 * R) plan[threadIdx.x] = mgr[MGR_TAKE + threadIdx.x];     // (TAKE and PUT are adjacent)
    __syncthreads();
    if (step >= 0 && blockIdx.x == 0 && threadIdx.x == 0 && !p.ctl[BCTL_ALL_DONE]) {
        // what plan_places left for behind the step: a refilled place starts over, and when no place
        // holds a replicate any more everything has finished
        bool live = false;
        for (int r = 0; r < R; ++r) {
            if (plan[R + r]) { p.ctl[BCTL_DONE + r] = 0; p.ctl[BCTL_UNDEFINED + r] = 0; p.ctl[BCTL_ITERS + r] = 0; }
            live |= mgr[MGR_REP + r] != 0;
        }
        if (!live) { p.ctl[BCTL_LAST_STEP] = (unsigned long long)(step + 1); p.ctl[BCTL_ALL_DONE] = 1; }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) any |= plan[i] != 0;
    if (!any) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double *cls_count = const_cast<double *>(p.cls_count);
    for (int r = 0; r < R; ++r) {
        const unsigned long long take = plan[r], put = plan[R + r];
        if (take)
            for (int64_t t = first; t < p.n_tx; t += stride) out_all[(int64_t)(take - 1) * p.n_tx + t] = into[t * R + r];
        if (put) {
            for (int64_t t = first; t < p.n_tx; t += stride) into[t * R + r] = x_start[t];
            const double *counts = counts_all + (int64_t)(put - 1) * p.n_classes;
            for (int64_t c = first; c < p.n_classes; c += stride) cls_count[c * R + r] = counts[c];
            if (first < EM_FINAL_BLOCKS) { p.part_max[first * R + r] = 1e300; p.part_flags[first * R + r] = 1u; }
            if (first == 0) p.place_total[r] = totals[2 * (put - 1)];        // (pairs: as launch_np_sum_many leaves them)
        }
    }
}

// fresh control block; the places in `idle` hold no replicate and count as stopped
__global__ void em_batch_ctl_kernel(unsigned long long *ctl, unsigned int idle)
{
    const int i = threadIdx.x;
    if (i < 32) ctl[i] = (i >= BCTL_DONE && i < BCTL_DONE + R && ((idle >> (i - BCTL_DONE)) & 1u)) ? 1ULL : 0ULL;
}

// ---- the counts of a group of problems on their way into counts_all (skm_quant_em_many, _em_blend)
//
// The blended class counts of seekmer/impute.py:248-252 for the cells first .. first +
// n_rows - 1, in the caller's class order: rows[i][k] = ((own[k] * weight[first + i][cell_of[k]]) *
// total[first + i]) / total[cell_of[k]] -- numpy's `c * w * total / c.sum()` operation by operation
// (multiply, multiply, IEEE divide; there is no addition, so nothing to contract, and the library is
// built without fast-math).  A lane keeps its class; the rows of the group go by in blockIdx.y.
__global__ void __launch_bounds__(256)
blend_counts_kernel(const double *__restrict__ own, const int32_t *__restrict__ class_cell, const double *__restrict__ weight,
                    const double *__restrict__ cell_total, int64_t n_cells, int64_t first, int64_t n_rows, int64_t n_classes,
                    double *__restrict__ rows)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n_classes; k += (int64_t)gridDim.x * blockDim.x) {
        const double c = own[k];
        const int32_t from = class_cell[k];
        const double from_total = cell_total[from];
        for (int64_t i = blockIdx.y; i < n_rows; i += gridDim.y) {
            const double w = weight[(first + i) * n_cells + from];
            rows[i * n_classes + k] = ((c * w) * cell_total[first + i]) / from_total;
        }
    }
}

// y[i][k] = x[i][perm[k]]: `n_rows` count vectors from the caller's class order to the internal one
__global__ void __launch_bounds__(256)
permute_rows_kernel(const double *__restrict__ x, const int32_t *__restrict__ perm, int64_t n, int64_t n_rows,
                    double *__restrict__ y)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t from = perm[k];
        for (int64_t i = blockIdx.y; i < n_rows; i += gridDim.y) y[i * n + k] = x[i * n + from];
    }
}

inline unsigned grid_of(int64_t items, int per_block, int64_t cap = 256 * 8)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    if (blocks < 1) blocks = 1;
    if (blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

}  // namespace

int em_batch_final_blocks(const EmBatchProblem &p)
{
    // (fused: the blocks of em_rows_finalize_batch, 32 rows each; else a lane per transcript and replicate)
    int64_t blocks = p.fused ? (p.n_rows + 31) / 32 : (p.n_tx * EM_BATCH + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > EM_FINAL_BLOCKS) blocks = EM_FINAL_BLOCKS;
    return (int)blocks;
}

void launch_em_batch_step(const EmBatchProblem &p, int64_t step, hipStream_t stream)
{
    const int parity = (int)(step & 1);
    hipLaunchKernelGGL(em_inner_batch_kernel, dim3(grid_of(p.n_classes, 256 / EM_BATCH)), dim3(256), 0, stream, p, parity,
                       step > 0 ? em_batch_final_blocks(p) : 0, step);
    if (p.fused) {
        hipLaunchKernelGGL(em_rows_finalize_batch_kernel, dim3((unsigned)em_batch_final_blocks(p)), dim3(256), 0, stream, p,
                           parity);
        return;
    }
    hipLaunchKernelGGL(em_rows_batch_kernel, dim3(grid_of(p.n_rows, 32)), dim3(256), 0, stream, p, parity);
    hipLaunchKernelGGL(em_finalize_batch_kernel, dim3((unsigned)em_batch_final_blocks(p)), dim3(256), 0, stream, p,
                       parity);
}

// the device-managed working set: set up for `n_reps` replicates (places 0 .. min(n_reps, 8) - 1 filled
// from counts_all[0 ..]), then after every step em_batch_manage
void launch_em_batch_manage_init(const EmBatchProblem &p, unsigned long long *mgr, unsigned long long *host, int64_t n_reps,
                                 const double *counts_all, const double *totals, const double *x_start, double *out_all,
                                 hipStream_t stream)
{
    for (int i = 0; i < 64; ++i) host[i] = 0;          // (64 words of page-locked memory of the caller's)
    const int filled = (int)std::min<int64_t>(n_reps, EM_BATCH);
    host[MGR_NEXT] = (unsigned long long)filled;
    host[MGR_COUNT] = (unsigned long long)n_reps;
    unsigned int idle = 0;
    for (int r = 0; r < EM_BATCH; ++r) {
        if (r < filled) { host[MGR_REP + r] = (unsigned long long)r + 1; host[MGR_PUT + r] = (unsigned long long)r + 1; }
        else idle |= 1u << r;
    }
    (void)hipMemcpyAsync(mgr, host, 64 * sizeof(unsigned long long), hipMemcpyHostToDevice, stream);
    hipLaunchKernelGGL(em_batch_ctl_kernel, dim3(1), dim3(64), 0, stream, p.ctl, idle);
    hipLaunchKernelGGL(em_batch_refill_kernel, dim3(1024), dim3(256), 0, stream, p, mgr, counts_all, totals, x_start, out_all,
                       p.x[0], (int64_t)-1);
}

// behind a step whose em_inner_batch has planned (p.mgr set): the refill alone; `planned` false (a
// look between chunks, behind em_batch_decide): the plan first, as a launch of its own
void launch_em_batch_manage(const EmBatchProblem &p, unsigned long long *mgr, const double *counts_all, const double *totals,
                            const double *x_start, double *out_all, int64_t *iters_out, int64_t step, bool planned,
                            hipStream_t stream)
{
    if (!planned) hipLaunchKernelGGL(em_batch_assign_kernel, dim3(1), dim3(64), 0, stream, p, mgr, iters_out, step);
    hipLaunchKernelGGL(em_batch_refill_kernel, dim3(1024), dim3(256), 0, stream, p, mgr, counts_all, totals, x_start,
                       out_all, p.x[(step + 1) & 1], step);
}

void launch_em_batch_decide(const EmBatchProblem &p, int64_t steps_done, hipStream_t stream)
{
    hipLaunchKernelGGL(em_decide_batch_kernel, dim3(1), dim3(256), 0, stream, p, em_batch_final_blocks(p), steps_done);
}

void launch_em_batch_take(const double *x, int64_t n_tx, int r, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(em_batch_take_kernel, dim3(grid_of(n_tx, 256)), dim3(256), 0, stream, x, n_tx, r, out);
}

void launch_em_batch_ctl(unsigned long long *ctl, unsigned int idle, hipStream_t stream)
{
    hipLaunchKernelGGL(em_batch_ctl_kernel, dim3(1), dim3(64), 0, stream, ctl, idle);
}

void launch_blend_counts(const double *own, const int32_t *class_cell, const double *weight, const double *cell_total,
                         int64_t n_cells, int64_t first, int64_t n_rows, int64_t n_classes, double *rows, hipStream_t stream)
{
    if (n_rows <= 0 || n_classes <= 0) return;
    hipLaunchKernelGGL(blend_counts_kernel, dim3(grid_of(n_classes, 256, 1024), (unsigned)std::min<int64_t>(n_rows, 64)),
                       dim3(256), 0, stream, own, class_cell, weight, cell_total, n_cells, first, n_rows, n_classes, rows);
}

void launch_permute_rows_f64(const double *x, const int32_t *perm, int64_t n, int64_t n_rows, double *y, hipStream_t stream)
{
    if (n_rows <= 0 || n <= 0) return;
    hipLaunchKernelGGL(permute_rows_kernel, dim3(grid_of(n, 256, 1024), (unsigned)std::min<int64_t>(n_rows, 64)), dim3(256), 0,
                       stream, x, perm, n, n_rows, y);
}

// (skm_index_create loads every code object of the library before the first sample needs it: the first
// launch out of a translation unit otherwise pays its load, tens of milliseconds, inside the run)
void warm_code_em_batch()
{
    hipFuncAttributes attributes;
    (void)hipFuncGetAttributes(&attributes, reinterpret_cast<const void *>(&em_inner_batch_kernel));
}

}  // namespace skm
