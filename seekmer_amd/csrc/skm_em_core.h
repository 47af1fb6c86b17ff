// The arithmetic of one EM step (seekmer/infer.py:152-160), written once for every kernel family that
// runs it: the whole-table and tile kernels (skm_em.hip), eight problems side by side
// (skm_em_batch.hip), many tables in one grid (skm_em_set.hip).  The kernels keep their grids, their
// index mapping and their memory layout and call these; a family's result is bit for bit another's
// because the additions, their order and the divisions are the ones below and no others.  Device only.
#pragma once
#include "skm_kernels.h"

namespace skm {

// S_c: the abundances of a class's tuple ids[begin .. end) added in tuple order (as numpy.bincount
// accumulates them), four independent gathers in flight.  Element t of the vector is x[t * STRIDE + at].
template <int STRIDE>
__device__ __forceinline__ double em_tuple_sum(const int32_t *__restrict__ ids, int64_t begin, int64_t end,
                                               const double *__restrict__ x, int at)
{
    double s = 0.0;
    int64_t j = begin;
    for (; j + 4 <= end; j += 4) {
        const int32_t t0 = ids[j], t1 = ids[j + 1], t2 = ids[j + 2], t3 = ids[j + 3];
        const double x0 = x[(int64_t)t0 * STRIDE + at], x1 = x[(int64_t)t1 * STRIDE + at];
        const double x2 = x[(int64_t)t2 * STRIDE + at], x3 = x[(int64_t)t3 * STRIDE + at];
        s += x0; s += x1; s += x2; s += x3;
    }
    for (; j < end; ++j) s += x[(int64_t)ids[j] * STRIDE + at];
    return s;
}

// the eight partial sums of a row, one per lane of its group, to the row's sum in every lane
__device__ __forceinline__ double em_row_butterfly(double s)
{
    s += __shfl_xor(s, 4, 8);
    s += __shfl_xor(s, 2, 8);
    s += __shfl_xor(s, 1, 8);
    return s;
}

// A row's sum of x_t / inner_c over tx_cls[begin .. end) (infer.py:157): lane `sub` of the row's eight
// adds entries begin + sub + 8 k in ascending k, then the butterfly.  PAIRED: two gathers in flight.
template <bool PAIRED, typename Cls, typename Off>
__device__ __forceinline__ double em_row_sum(const Cls *tx_cls, const double *inner, Off begin, Off end, int sub, double xt)
{
    double s = 0.0;
    Off e = begin + sub;
    if (PAIRED) {
        for (; e + 8 < end; e += 16) {
            const Cls c0 = tx_cls[e], c1 = tx_cls[e + 8];
            const double i0 = inner[c0], i1 = inner[c1];
            s += xt / i0;
            s += xt / i1;
        }
    }
    for (; e < end; e += 8) s += xt / inner[tx_cls[e]];
    return em_row_butterfly(s);
}

// the same for R problems side by side (x[t][R], inner[c][R]): xr = the transcript's abundances, s = the row's sums
template <int R>
__device__ __forceinline__ void em_row_sums(const int32_t *__restrict__ tx_cls, const double *__restrict__ inner_all,
                                            int64_t begin, int64_t end, int sub, const double *__restrict__ xt,
                                            double (&xr)[R], double (&s)[R])
{
#pragma unroll
    for (int r = 0; r < R; ++r) { xr[r] = xt[r]; s[r] = 0.0; }
    for (int64_t e = begin + sub; e < end; e += 8) {
        const double *__restrict__ inner = inner_all + (int64_t)tx_cls[e] * R;
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += xr[r] / inner[r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = em_row_butterfly(s[r]);
}

// ---- a transcript of several rows, summed by lane groups of different blocks.  Row sums cross blocks
// as 8-byte agent-scope atomic stores and loads (write-through / L2-bypassing: the XCDs' L2s are not
// coherent), a store completed before its arrival is counted; the group whose row arrives last adds
// the sums up in row order and clears the counter for the next step.
// Publishes row_sum[slot] = s; a lane with `counts` set then counts the row's arrival and gets the
// number arrived, its own included (the wait is per wave: the stores of its whole group are complete).
__device__ __forceinline__ unsigned int em_row_publish(double *row_sum, int64_t slot, double s, unsigned int *arrivals_t, bool counts)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(row_sum) + slot, (unsigned long long)__double_as_longlong(s),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return counts ? atomicAdd(arrivals_t, 1u) + 1u : 0u;
}
__device__ __forceinline__ double em_row_published(const double *row_sum, int64_t slot)
{
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(row_sum) + slot,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// 0.0 + the published sums of rows first_row .. first_row + rows_of_t - 1 in row order.  STRIDE 1: the
// eight lanes fetch eight sums at a time and hand them round (a transcript in 100 000 classes has 200
// rows); STRIDE R: lane `sub` owns problem `sub` and reads its own column.
template <int STRIDE>
__device__ __forceinline__ double em_rows_published_sum(const double *row_sum, int64_t first_row, int64_t rows_of_t, int sub)
{
    double a = 0.0;
    if (STRIDE == 1) {
        for (int64_t k0 = 0; k0 < rows_of_t; k0 += 8) {
            const int64_t k = k0 + sub;
            const double mine = k < rows_of_t ? em_row_published(row_sum, first_row + k) : 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double v = __shfl(mine, j, 8);
                if (k0 + j < rows_of_t) a += v;
            }
        }
    } else {
        for (int64_t k = 0; k < rows_of_t; ++k) a += em_row_published(row_sum, (first_row + k) * STRIDE + sub);
    }
    return a;
}
__device__ __forceinline__ void em_row_arrivals_reset(unsigned int *arrivals_t) { atomicExch(arrivals_t, 0u); }

// 0.0 + row sums first .. end - 1 that an earlier launch wrote (the unfused forms)
template <int STRIDE>
__device__ __forceinline__ double em_rows_stored_sum(const double *__restrict__ row_sum, int64_t first, int64_t end, int at)
{
    double a = 0.0;
    for (int64_t r = first; r < end; ++r) a += row_sum[r * STRIDE + at];
    return a;
}

// x'_t from the transcript's numerator
__device__ __forceinline__ double em_new_abundance(double a, double eff, double n_total)
{
    double v = a / eff / n_total;                                     // infer.py:158
    if (v != v) v = 0.0;                                              // infer.py:159
    return v;
}
// the stopping rule's view of x'_t: flags bit 0 = some abundance above x_floor, bit 1 = a NaN change
__device__ __forceinline__ void em_note_change(double v, double before, double x_floor, double &local_max, unsigned int &flags)
{
    if (v > x_floor) {                                                // infer.py:160
        const double change = fabs(v - before) / v;
        if (change != change) flags |= 2u;
        else if (change > local_max) local_max = change;
        flags |= 1u;
    }
}

// (max, or) over the lanes of a wave that are LOWEST apart, left in every one of them
template <int LOWEST>
__device__ __forceinline__ void em_wave_reduce(double &m, unsigned int &f)
{
    for (int d = 32; d >= LOWEST; d >>= 1) {
        const double o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
        f |= __shfl_xor(f, d, 64);
    }
}
// the four waves' slots (`stride` apart) folded into one
__device__ __forceinline__ void em_fold_waves(const double *s_max, const unsigned int *s_flags, int stride, double &m, unsigned int &f)
{
    m = s_max[0];
    f = s_flags[0];
    for (int w = 1; w < 4; ++w) { m = s_max[w * stride] > m ? s_max[w * stride] : m; f |= s_flags[w * stride]; }
}
// A block of 256 lanes, lane i holding (m, f) of problem i % LOWEST: true in the lanes i < LOWEST, which
// get their problem's (max, or) over the block.  (One barrier; once per kernel: the slots are not reused.)
template <int LOWEST>
__device__ __forceinline__ bool em_block_reduce(double &m, unsigned int &f)
{
    __shared__ double s_max[4][LOWEST];
    __shared__ unsigned int s_flags[4][LOWEST];
    em_wave_reduce<LOWEST>(m, f);
    const int wave = threadIdx.x >> 6, r = threadIdx.x & (LOWEST - 1);
    if ((threadIdx.x & 63) < LOWEST) { s_max[wave][r] = m; s_flags[wave][r] = f; }
    __syncthreads();
    if (threadIdx.x >= LOWEST) return false;
    em_fold_waves(&s_max[0][r], &s_flags[0][r], LOWEST, m, f);
    return true;
}

// The reference's stopping rule (infer.py:160) for finalize pass `steps_done` with flags f and largest
// relative change m over all transcripts.  max_iters, fixed_iters: 0 = none.
struct EmVerdict { bool done, undefined; };
__device__ __forceinline__ EmVerdict em_stop_rule(unsigned int f, double m, double rel_tol, int64_t steps_done,
                                                  int64_t max_iters, int64_t fixed_iters)
{
    if (fixed_iters > 0) return {steps_done >= fixed_iters, false};
    if (!(f & 1u)) return {true, true};                               // numpy raises on max() of an empty selection
    bool done = (f & 2u) || !(m > rel_tol);                           // NaN propagates through max()
    if (max_iters > 0 && steps_done >= max_iters) done = true;
    return {done, false};
}

// ---- the two kernels of a step in the single-problem shape, for a range of the class and row views.
// Problem: EmProblem or EmSetProblem (the views' fields have one set of names).  View says what differs:
//   cls_first(), cls_end(), row_first(), row_end()   the classes and rows covered
//   n_total()                                        the sum of the class counts
//   done()                                           the word that says "stopped"
//   judge(eval_parts, steps_done)                    the previous step judged by this block: stopped?
//   part()                                           where this block's partials of the stopping rule go
// The kernel says where the calling lane stands -- `lane` of `lanes` in the grid's x dimension, and whether
// its block is the one that judges -- because only there does the compiler fold blockDim.x into one scalar
// load: read in here, behind the test for block 0, it became a vector load in front of every block's first
// address (4 % of a sample set's EM at 8 samples).

// judges: the finalize pass before this launch (number `steps_done`, eval_parts partials) has not been judged
// yet, and this block does it
template <class Problem, class View>
__device__ __forceinline__ void em_inner_body(const Problem &p, const View &v, int parity, bool judges, int eval_parts,
                                              int64_t steps_done, int64_t lane, int64_t lanes)
{
    // the first class's row is fetched before the verdict on the previous step is known: its
    // latency then runs under the judging instead of after it
    const int64_t cls_end = v.cls_end();
    const int64_t c_first = v.cls_first() + lane;
    int64_t begin_first = 0, end_first = 0;
    double count_first = 1.0;
    if (c_first < cls_end) {
        begin_first = p.cls_offset[c_first];
        end_first = p.cls_offset[c_first + 1];
        count_first = p.cls_count[c_first];
    }
    if (judges) {
        // Block 0 judges the step before this one and latches the verdict; the other blocks do not
        // wait for it.  If the EM has just stopped they compute one pass of `inner` that nobody
        // reads (x is not touched by this kernel, and every later launch sees the latch and
        // returns): 13 us once per EM, against every block re-reading all the partials every step
        // (34.5 -> 32.8 us per step).
        if (v.done()) return;                   // (block-uniform)
        if (v.judge(eval_parts, steps_done)) return;
    } else if (v.done()) {
        return;
    }
    const double *__restrict__ x = p.x[parity];
    for (int64_t c = c_first; c < cls_end; c += lanes) {
        const int64_t begin = c == c_first ? begin_first : p.cls_offset[c];
        const int64_t end = c == c_first ? end_first : p.cls_offset[c + 1];
        const double count = c == c_first ? count_first : p.cls_count[c];
        p.inner[c] = em_tuple_sum<1>(p.ids, begin, end, x, 0) / count;  // infer.py:155-156
    }
}

// Rows and finalize in ONE launch.  Every transcript has at least one row (skm_quant_setup.hip), nearly
// every transcript exactly one: the 8-lane group that has summed such a row finalizes its transcript
// on the spot, and the rows of a transcript in more than EM_ROW_CAP classes go through the several-rows
// protocol above.  TO_ACC (several ranks): the numerator goes to p.acc instead, for the all-reduce
// that sits in front of em_finalize there, which then judges the step.
template <bool TO_ACC, class Problem, class View>
__device__ __forceinline__ void em_rows_finalize_body(const Problem &p, const View &v, int parity, int64_t lane, int64_t lanes)
{
    if (v.done()) return;                       // (block-uniform)
    const double *__restrict__ x = p.x[parity];
    double *__restrict__ x_new = p.x[parity ^ 1];
    const int64_t row_end = v.row_end();
    const double n_total = v.n_total();
    const int sub = threadIdx.x & 7;
    double local_max = 0.0;
    unsigned int flags = 0;
    for (int64_t r = v.row_first() + (lane >> 3); r < row_end; r += lanes >> 3) {
        const int64_t begin = p.row_start[r], end = p.row_start[r + 1];
        const int32_t t = p.row_tx[r];
        const double xt = x[t];
        // (what the finalize needs is asked for with x[t]: one round trip for all of it)
        const int64_t first_row = p.tx_row[t], rows_of_t = p.tx_row[t + 1] - first_row;
        const double eff = p.eff_len[t];
        const double s = em_row_sum<true>(p.tx_cls, p.inner, begin, end, sub, xt);
        // 1: the transcript's only row; 2: the last of its rows to arrive (this group adds them up); 0: neither
        int mode = 0;
        if (sub == 0) {
            if (rows_of_t == 1) mode = 1;
            else mode = (int64_t)em_row_publish(p.row_sum, r, s, &p.arrivals[t], true) == rows_of_t ? 2 : 0;
        }
        mode = __shfl(mode, 0, 8);
        if (mode == 0) continue;
        double a = 0.0;
        if (mode == 1) {
            a += s;
        } else {
            a = em_rows_published_sum<1>(p.row_sum, first_row, rows_of_t, sub);
            if (sub == 0) em_row_arrivals_reset(&p.arrivals[t]);
        }
        if (sub != 0) continue;
        if constexpr (TO_ACC) {
            p.acc[t] = a;
        } else {
            const double xv = em_new_abundance(a, eff, n_total);
            x_new[t] = xv;
            em_note_change(xv, xt, p.x_floor, local_max, flags);
        }
    }
    if (TO_ACC) return;
    // (every block writes its pair every step, one without rows too: the judge reads all of them)
    if (em_block_reduce<1>(local_max, flags)) {
        p.part_max[v.part()] = local_max;
        p.part_flags[v.part()] = flags;
    }
}

}  // namespace skm
