// Quantification kernels for gfx950: effective lengths, the EM step, the
// multinomial bootstrap draw.  They replace the numpy loop of
// /root/reference/seekmer/infer.py:133-168 (em), mapper.py:134-141
// (effective_lengths) and the scipy draw of infer.py:108-111.
//
// One EM step is a two-sided gather over two CSR views of the same
// (class, transcript) pairs, four launches on one stream and no
// floating-point atomics, so every step is bitwise reproducible:
//   em_inner     -- one lane per class: S_c = sum of x over the tuple in tuple
//                   order, inner_c = S_c / count_c            (infer.py:155-156)
//   em_rows      -- 8 lanes per row (a run of <= 512 classes of ONE transcript):
//                   sum of x_t / inner_c over the run          (infer.py:157)
//   em_finalize  -- one lane per transcript: x'_t = (sum of its rows) / l_t /
//                   n, NaN -> 0, relative change against x_t; block partials
//   (judging)    -- the reference's stopping rule (infer.py:160) over the block
//                   partials is evaluated at the head of the next em_inner
//                   launch (by its block 0) and by a one-block
//                   em_decide launch at the end of each enqueued chunk; it
//                   latches `done`, after which every later launch is a no-op
//                   -- the host enqueues steps in chunks and still stops at
//                   exactly the reference's iteration count.
// The arithmetic of the step is skm_em_core.h's; the kernels here are its grids and layouts.
// All three are gather/stream kernels bound by HBM/L2 bandwidth: no MFMA.
#include "skm_em_core.h"

namespace skm {

__device__ bool em_evaluate(const EmProblem &p, int n_parts, int64_t steps_done, bool publish);

// the whole table of an EmProblem, as em_inner_body and em_rows_finalize_body see it (skm_em_core.h)
struct EmWholeTable {
    const EmProblem &p;
    __device__ __forceinline__ int64_t cls_first() const { return 0; }
    __device__ __forceinline__ int64_t cls_end() const { return p.n_classes; }
    __device__ __forceinline__ int64_t row_first() const { return 0; }
    __device__ __forceinline__ int64_t row_end() const { return p.n_rows; }
    __device__ __forceinline__ double n_total() const { return p.n_total; }
    __device__ __forceinline__ bool done() const { return p.ctl[CTL_DONE] != 0; }
    __device__ __forceinline__ bool judge(int eval_parts, int64_t steps_done) const { return em_evaluate(p, eval_parts, steps_done, true); }
    __device__ __forceinline__ int64_t part() const { return blockIdx.x; }          // judged by em_evaluate in the next launch
};

__global__ void __launch_bounds__(256)
em_inner_kernel(EmProblem p, int parity, int eval_parts, int64_t steps_done)
{
    em_inner_body(p, EmWholeTable{p}, parity, eval_parts > 0 && blockIdx.x == 0, eval_parts, steps_done, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                  (int64_t)gridDim.x * blockDim.x);
}

__global__ void __launch_bounds__(256)
em_rows_kernel(EmProblem p, int parity)
{
    if (p.ctl[CTL_DONE]) return;
    const double *__restrict__ x = p.x[parity];
    const int sub = threadIdx.x & 7;
    for (int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3; r < p.n_rows;
         r += ((int64_t)gridDim.x * blockDim.x) >> 3) {
        const double s = em_row_sum<true>(p.tx_cls, p.inner, p.row_start[r], p.row_start[r + 1], sub, x[p.row_tx[r]]);
        if (sub == 0) p.row_sum[r] = s;
    }
}

// em_rows and em_finalize in ONE launch (one rank: nothing to all-reduce between them): one launch
// (5.1 us) and one launch gap less per step; bit for bit em_rows + em_finalize.  TO_ACC (several
// ranks): em_rows + em_rows_to_acc in one launch.
template <bool TO_ACC>
__global__ void __launch_bounds__(256, 8)       // (8 waves per SIMD: the 2048-block grid is resident at once)
em_rows_finalize_kernel(EmProblem p, int parity)
{
    em_rows_finalize_body<TO_ACC>(p, EmWholeTable{p}, parity, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                                  (int64_t)gridDim.x * blockDim.x);
}

// multi-GPU only (the unfused form, SKM_EM_UNFUSED): rows -> per-transcript numerators for the all-reduce
__global__ void __launch_bounds__(256)
em_rows_to_acc_kernel(EmProblem p)
{
    if (p.ctl[CTL_DONE]) return;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < p.n_tx;
         t += (int64_t)gridDim.x * blockDim.x)
        p.acc[t] = em_rows_stored_sum<1>(p.row_sum, p.tx_row[t], p.tx_row[t + 1], 0);
}

template <bool FROM_ACC>
__global__ void __launch_bounds__(256)
em_finalize_kernel(EmProblem p, int parity)
{
    if (p.ctl[CTL_DONE]) return;
    const double *__restrict__ x_old = p.x[parity];
    double *__restrict__ x_new = p.x[parity ^ 1];
    double local_max = 0.0;
    unsigned int flags = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < p.n_tx;
         t += (int64_t)gridDim.x * blockDim.x) {
        const double a = FROM_ACC ? p.acc[t] : em_rows_stored_sum<1>(p.row_sum, p.tx_row[t], p.tx_row[t + 1], 0);
        const double v = em_new_abundance(a, p.eff_len[t], p.n_total);
        x_new[t] = v;
        em_note_change(v, x_old[t], p.x_floor, local_max, flags);
    }
    if (em_block_reduce<1>(local_max, flags)) {
        p.part_max[blockIdx.x] = local_max;     // judged by em_evaluate in the next launch
        p.part_flags[blockIdx.x] = flags;
    }
}

// The stopping rule (infer.py:160) over the per-block partials of finalize pass number
// `steps_done` (1-based).  Every lane of the calling block takes part and gets the verdict;
// only the caller with `publish` set writes it to the control block.  It is evaluated at the
// head of the NEXT step's em_inner launch by that launch's block 0 (744 partials from L2 are
// cheaper than a launch of their own, 4.4 us), and by a one-block launch at the end of each
// enqueued chunk so that the host can read the state.
__device__ bool em_evaluate(const EmProblem &p, int n_parts, int64_t steps_done, bool publish)
{
    __shared__ int s_done;
    double m = 0.0;
    unsigned int f = 0;
    for (int b = threadIdx.x; b < n_parts; b += blockDim.x) {
        const double o = p.part_max[b];
        m = o > m ? o : m;
        f |= p.part_flags[b];
    }
    if (p.n_extra > 0) {                        // (the tiles' partials of this step: max and or, any order)
        const int64_t first = (steps_done - 1 - p.extra_first) * p.n_extra;
        for (int64_t b = threadIdx.x; b < p.n_extra; b += blockDim.x) {
            const double o = p.extra_max[first + b];
            m = o > m ? o : m;
            f |= p.extra_flags[first + b];
        }
    }
    if (em_block_reduce<1>(m, f)) {
        const EmVerdict verdict = em_stop_rule(f, m, p.rel_tol, steps_done, p.max_iters, p.fixed_iters);
        if (publish) {
            if (verdict.undefined) p.ctl[CTL_UNDEFINED] = 1;
            p.ctl[CTL_ITERS] = (unsigned long long)steps_done;
            p.ctl[CTL_DONE] = verdict.done ? 1ULL : 0ULL;
        }
        s_done = verdict.done ? 1 : 0;
    }
    __syncthreads();
    return s_done != 0;
}

__global__ void __launch_bounds__(256)
em_decide_kernel(EmProblem p, int n_parts, int64_t steps_done)
{
    if (p.ctl[CTL_DONE]) return;
    em_evaluate(p, n_parts, steps_done, true);
}

// ---- the EM of independent components, a chunk of steps per launch (EmTiles, skm_kernels.h)
// One workgroup per tile.  The tile's pairs in both views (16-bit tile-local indices), the class counts,
// `inner`, the effective lengths and both abundance vectors live in LDS for the whole chunk; a step is
//   class phase  one lane per class: S_c over the tuple in tuple order, inner_c = S_c / count_c.  A lane
//                takes EM_CLASS_BATCH entries at a time: the
//                indices, then the abundances -- all of them in flight at once -- and adds them one after
//                the other in tuple order; an entry past the tuple's end is not added (a select: adding
//                +0.0 would turn a sum of -0.0 into +0.0).  The set-up lists a tile's classes by the
//                number of such batches, so the 64 classes of a wave take like numbers of turns.
//   row phase    eight lanes per transcript, its rows of <= EM_ROW_CAP entries one after the other, the
//                row sums added in row order from 0.0, then the finalize (skm_em_core.h)
// with two workgroup barriers and nothing that crosses workgroups but the stopping rule's partials.  Tiles
// alone: each workgroup adds its partials of the chunk's steps to the judge's words and the one that arrives
// last judges the steps in order (em_tile_arrive, em_tiles_judge).  Beside a residual problem they go to
// step_max / step_flags [step][tile], which that problem's judge reads (em_evaluate).
// Every step's abundances also go to tl.snap[step][transcript]: the next chunk starts from the last of
// them, and the launch that finds the EM stopped -- the look-ahead chunk, which would otherwise do
// nothing -- copies its tile's entries of the step the rule was met at to p.x[steps & 1], where the
// callers look for the result.  No step is run twice, and the copy names the tile's transcripts only,
// so it serves beside a residual problem that keeps its own entries of p.x.
//
// Timing experiments only (scripts/build_variant.sh; the results of these builds are wrong):
// 1 = no class phase (inner is left as loaded: garbage), 2 = no row phase (x is never stepped).
#ifndef SKM_EM_TILE_EXPERIMENT
#define SKM_EM_TILE_EXPERIMENT 0
#endif
// entries of a class tuple fetched together (1: one after the other, the form this kernel began with)
#ifndef SKM_EM_CLASS_BATCH
#define SKM_EM_CLASS_BATCH 4
#endif
constexpr int EM_CLASS_BATCH = SKM_EM_CLASS_BATCH;
static_assert(EM_CLASS_BATCH == EM_TILE_CLASS_BATCH || EM_CLASS_BATCH == 1, "the set-up orders classes by turns of this width");

// ---- the chunk's verdict without a launch of its own (tiles alone; the words of EmTiles::judge)
// Called by wave 0 of a tile's workgroup, whose lane s (`has`: s < n_steps) holds the tile's partials (m, f) of
// step s.  They are a maximum over doubles that are +0.0 or above and never NaN (em_note_change sends a NaN to
// the flags) -- the bits of such doubles order as unsigned integers -- and an OR, so whatever order the tiles
// arrive in, the words end up as the pair that a pass over step_max / step_flags gives.  The XCDs' L2s are not
// coherent, so the words are touched by agent-scope accesses alone, as the row sums of skm_em_core.h are:
//   * a lane first reads its words (agent-scope load) and issues the atomic only where its value would change the
//     word: the maximum settles after a few arrivals, and thousands of atomics on 32 words would queue
//     (a word read too low costs a needless atomic, never a wrong one: between launches the words are zero,
//     and inside one they only grow);
//   * the wave's atomics are complete (vmcnt) before lane 0 counts the tile's arrival;
//   * the workgroup that counts the last arrival reads the words by atomic exchange, which clears them for the
//     next launch, and clears the counter.
// Nothing waits for another workgroup.  Returns the tiles arrived, this one included, in every lane.
__device__ __forceinline__ unsigned long long em_tile_arrive(unsigned long long *judge, bool has, double m, unsigned int f)
{
    if (has) {
        unsigned long long *word_max = judge + EM_JUDGE_MAX + threadIdx.x, *word_flags = judge + EM_JUDGE_FLAGS + threadIdx.x;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(m);
        if (__hip_atomic_load(word_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits)
            __hip_atomic_fetch_max(word_max, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f & ~(unsigned int)__hip_atomic_load(word_flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            __hip_atomic_fetch_or(word_flags, (unsigned long long)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long arrived = 0;
    if (threadIdx.x == 0)
        arrived = __hip_atomic_fetch_add(judge + EM_JUDGE_ARRIVED, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ULL;
    return __shfl(arrived, 0, 64);
}
// By wave 0 of the workgroup that arrived last: the stopping rule for steps first_step + 1 .. first_step + n_steps
// in order, the first that stops latched in the control block.
__device__ __forceinline__ void em_tiles_judge(const EmProblem &p, unsigned long long *judge, bool has, int64_t first_step, int n_steps)
{
    double m = 0.0;
    unsigned int f = 0;
    if (has) {
        m = __longlong_as_double((long long)__hip_atomic_exchange(judge + EM_JUDGE_MAX + threadIdx.x, 0ULL, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT));
        f = (unsigned int)__hip_atomic_exchange(judge + EM_JUDGE_FLAGS + threadIdx.x, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) __hip_atomic_store(judge + EM_JUDGE_ARRIVED, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool undefined = false, done = false;
    int64_t steps_done = first_step;
    for (int s = 0; s < n_steps && !done; ++s) {        // (wave-uniform: every lane walks the same pairs)
        steps_done = first_step + s + 1;
        const EmVerdict verdict = em_stop_rule(__shfl(f, s, 64), __shfl(m, s, 64), p.rel_tol, steps_done, p.max_iters, p.fixed_iters);
        undefined |= verdict.undefined;
        done = verdict.done;
    }
    if (threadIdx.x != 0) return;
    if (undefined) p.ctl[CTL_UNDEFINED] = 1;
    p.ctl[CTL_ITERS] = (unsigned long long)steps_done;
    p.ctl[CTL_DONE] = done ? 1ULL : 0ULL;
}

__global__ void __launch_bounds__(256)
em_local_chunk_kernel(EmProblem p, EmTiles tl, const double *x_in, int n_steps, int64_t first_step)
{
    static_assert(EM_TILE_TX <= 8 * 32, "a lane group of the row phase takes at most eight transcripts");
    __shared__ double s_x[2][EM_TILE_TX];
    __shared__ double s_eff[EM_TILE_TX];
    __shared__ double s_inner[EM_TILE_CLASSES];
    __shared__ double s_count[EM_TILE_CLASSES];
    __shared__ double s_max[EM_CHUNK_MAX][4];
    __shared__ unsigned int s_flags[EM_CHUNK_MAX][4];
    __shared__ int32_t s_tx[EM_TILE_TX];
    __shared__ uint16_t s_cls_tx[EM_TILE_PAIRS], s_tx_cls[EM_TILE_PAIRS];
    __shared__ uint16_t s_cls_off[EM_TILE_CLASSES + 1], s_tx_off[EM_TILE_TX + 1];
    // (the launch order: the set-up's largest tiles first, see EmTiles::order)
    const int64_t tile = tl.order ? tl.order[tl.order_reversed ? tl.n_tiles - 1 - blockIdx.x : blockIdx.x] : blockIdx.x;
    const int64_t tx0 = tl.tile_tx[tile], cls0 = tl.tile_cls[tile];
    const int n_tx = (int)(tl.tile_tx[tile + 1] - tx0), n_cls = (int)(tl.tile_cls[tile + 1] - cls0);
    const int64_t cp0 = tl.cls_pair[cls0], tp0 = tl.tx_pair[tx0];
    const int n_pairs = (int)(tl.cls_pair[cls0 + n_cls] - cp0);
    // The set-up keeps every tile within the capacities.  One that is not would overrun the arrays above:
    // it is left alone, and the run is stopped with the fault word set, which the host turns into an error.
    if (n_tx > EM_TILE_TX || n_cls > EM_TILE_CLASSES || n_pairs > EM_TILE_PAIRS || n_tx < 0 || n_cls < 0 || n_pairs < 0) {
        if (threadIdx.x == 0) { p.ctl[CTL_TILE_FAULT] = 1; p.ctl[CTL_DONE] = 1; }
        return;
    }
    const int tid = threadIdx.x;
    if (p.ctl[CTL_DONE]) {                      // (block-uniform)
        // The EM stopped in the chunk before this one, `at` steps into it: that step's abundances of
        // this tile's transcripts are the result.  (Nothing is copied after a tile fault -- the run
        // fails -- and the range check keeps a control block that a faulting tile of this very launch
        // is writing from naming a step outside the buffer.)
        const int64_t steps = (int64_t)p.ctl[CTL_ITERS], at = steps - 1 - (first_step - n_steps);
        if (p.ctl[CTL_TILE_FAULT] || first_step < n_steps || at < 0 || at >= n_steps) return;
        const double *__restrict__ from = tl.snap + at * p.n_tx;
        double *__restrict__ to = p.x[steps & 1];
        for (int i = tid; i < n_tx; i += 256) {
            const int32_t t = tl.tx_list[tx0 + i];
            to[t] = from[t];
        }
        return;
    }
    for (int j = tid; j < n_pairs; j += 256) {
        s_cls_tx[j] = tl.cls_tx[cp0 + j];
        s_tx_cls[j] = tl.tx_cls[tp0 + j];
    }
    for (int k = tid; k <= n_cls; k += 256) {
        s_cls_off[k] = (uint16_t)(tl.cls_pair[cls0 + k] - cp0);
        if (k < n_cls) s_count[k] = p.cls_count[tl.cls_list[cls0 + k]];
        if ((SKM_EM_TILE_EXPERIMENT & 1) && k < n_cls) s_inner[k] = 1.0;
    }
    for (int i = tid; i <= n_tx; i += 256) {
        s_tx_off[i] = (uint16_t)(tl.tx_pair[tx0 + i] - tp0);
        if (i < n_tx) {
            const int32_t t = tl.tx_list[tx0 + i];
            s_tx[i] = t;
            s_x[0][i] = x_in[t];
            s_eff[i] = p.eff_len[t];
        }
    }
    __syncthreads();
    const int sub = tid & 7, wave = tid >> 6;
    for (int step = 0; step < n_steps; ++step) {
        const double *x = s_x[step & 1];
        double *x_new = s_x[(step & 1) ^ 1];
        if (!(SKM_EM_TILE_EXPERIMENT & 1)) {
            for (int k = tid; k < n_cls; k += 256) {
                const int end = s_cls_off[k + 1];
                double s = 0.0;
                if (EM_CLASS_BATCH == 1) {
                    for (int j = s_cls_off[k]; j < end; ++j) s += x[s_cls_tx[j]];
                } else {
                    for (int j = s_cls_off[k]; j < end; j += EM_CLASS_BATCH) {
                        // (an entry past the end re-reads the tuple's last: a valid place, never added)
                        int t[EM_CLASS_BATCH];
                        double v[EM_CLASS_BATCH];
#pragma unroll
                        for (int b = 0; b < EM_CLASS_BATCH; ++b) t[b] = s_cls_tx[min(j + b, end - 1)];
#pragma unroll
                        for (int b = 0; b < EM_CLASS_BATCH; ++b) v[b] = x[t[b]];
                        s += v[0];
#pragma unroll
                        for (int b = 1; b < EM_CLASS_BATCH; ++b) {
                            const double with = s + v[b];
                            s = j + b < end ? with : s;
                        }
                    }
                }
                s_inner[k] = s / s_count[k];
            }
        }
        __syncthreads();
        double local_max = 0.0;
        unsigned int flags = 0;
        // (all eight lanes of a group hold a row's sum after the butterfly: lane `sub` keeps the
        // numerator of the group's transcript number `sub` and finalizes it after the loop, so that the
        // three divisions of the finalize run once per wave, not once per transcript of a group)
        double my_a = 0.0, my_xt = 0.0;
        int my_i = -1, turn = 0;
        if (!(SKM_EM_TILE_EXPERIMENT & 2)) {
            for (int i = tid >> 3; i < n_tx; i += 32, ++turn) {
                const double xt = x[i];
                const int end = s_tx_off[i + 1];
                int begin = s_tx_off[i];
                double a = 0.0;
                do {                                    // (a transcript in no class has one empty row)
                    const int row_end = min(begin + EM_ROW_CAP, end);
                    a += em_row_sum<false>(s_tx_cls, s_inner, begin, row_end, sub, xt);
                    begin = row_end;
                } while (begin < end);
                if (turn == sub) { my_a = a; my_xt = xt; my_i = i; }
            }
        }
        if (my_i >= 0) {
            const double v = em_new_abundance(my_a, s_eff[my_i], p.n_total);
            x_new[my_i] = v;
            tl.snap[step * p.n_tx + s_tx[my_i]] = v;
            em_note_change(v, my_xt, p.x_floor, local_max, flags);
        }
        em_wave_reduce<1>(local_max, flags);
        if ((tid & 63) == 0) { s_max[step][wave] = local_max; s_flags[step][wave] = flags; }
        __syncthreads();
    }
    if (tid >= 64) return;                      // (lane s of wave 0 holds the tile's partials of step s)
    double m = 0.0;
    unsigned int f = 0;
    if (tid < n_steps) em_fold_waves(s_max[tid], s_flags[tid], 1, m, f);
    if (tl.judge == nullptr) {                  // a residual problem beside the tiles: its judge reads these
        if (tid < n_steps) {
            tl.step_max[tid * tl.n_tiles + tile] = m;
            tl.step_flags[tid * tl.n_tiles + tile] = f;
        }
        return;
    }
    if (em_tile_arrive(tl.judge, tid < n_steps, m, f) != (unsigned long long)tl.n_tiles) return;
    em_tiles_judge(p, tl.judge, tid < n_steps, first_step, n_steps);
}

#if SKM_EM_JUDGE_LAUNCH
// (tuning builds only: the judge of a chunk of tiles alone as a launch of its own, as it was before
// em_tiles_judge; the A/B of profiles/em_tile_order_ab.log prices the two against each other)
// The stopping rule (em_evaluate) for the n_steps steps of a chunk, in order: wave s takes the maximum and
// the flags of step s over the tiles (max and or: the order does not matter), lane 0 then walks the steps
// and latches the first that stops.
__global__ void __launch_bounds__(64 * EM_CHUNK_MAX)
em_local_decide_kernel(EmProblem p, EmTiles tl, int64_t first_step, int n_steps)
{
    if (p.ctl[CTL_DONE]) return;
    __shared__ double s_max[EM_CHUNK_MAX];
    __shared__ unsigned int s_flags[EM_CHUNK_MAX];
    const int step = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (step < n_steps) {
        double m = 0.0;
        unsigned int f = 0;
        const double *__restrict__ step_max = tl.step_max + step * tl.n_tiles;
        const unsigned int *__restrict__ step_flags = tl.step_flags + step * tl.n_tiles;
        int64_t b = lane;
        for (; b + 7 * 64 < tl.n_tiles; b += 8 * 64) {       // (eight loads of each in flight)
            double o[8];
            unsigned int g[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { o[k] = step_max[b + 64 * k]; g[k] = step_flags[b + 64 * k]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { m = o[k] > m ? o[k] : m; f |= g[k]; }
        }
        for (; b < tl.n_tiles; b += 64) {
            const double o = step_max[b];
            m = o > m ? o : m;
            f |= step_flags[b];
        }
        em_wave_reduce<1>(m, f);
        if (lane == 0) { s_max[step] = m; s_flags[step] = f; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int s = 0; s < n_steps; ++s) {
        const int64_t steps_done = first_step + s + 1;
        const EmVerdict verdict = em_stop_rule(s_flags[s], s_max[s], p.rel_tol, steps_done, p.max_iters, p.fixed_iters);
        if (verdict.undefined) p.ctl[CTL_UNDEFINED] = 1;
        p.ctl[CTL_ITERS] = (unsigned long long)steps_done;
        p.ctl[CTL_DONE] = verdict.done ? 1ULL : 0ULL;
        if (verdict.done) break;
    }
}
#endif

// MapResult.effective_lengths, mapper.py:134-141: p = fld / fld.sum();
// eff_t = sum_i max(len_t - i, 1) * p_i accumulated for i = 0..1999 in order
// (compiled with -ffp-contract=off: separate multiply and add, as numpy).
// Where p comes from is a Source: stage() by the whole block (row `row` of the source's table; it ends
// on a barrier when it wrote LDS), then weight(i) = p_i for wave 0, which packs the bins.

// p = fld / fld.sum() of the histogram fld[row][2000]
struct HistogramWeights {
    struct Staged {
        unsigned long long counts[MAX_FRAGMENT_LENGTH];
        unsigned long long part[4];
    };
    const unsigned long long *fld;
    double total;
    __device__ __forceinline__ void stage(int64_t row, Staged &lds)
    {
        fld += row * MAX_FRAGMENT_LENGTH;
        // the histogram once into LDS (coalesced), its total by a block reduction (integers: any order)
        unsigned long long mine = 0;
        for (int i = threadIdx.x; i < MAX_FRAGMENT_LENGTH; i += blockDim.x) {
            lds.counts[i] = fld[i];
            mine += lds.counts[i];
        }
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if ((threadIdx.x & 63) == 0) lds.part[threadIdx.x >> 6] = mine;
        __syncthreads();
        total = (double)(long long)(lds.part[0] + lds.part[1] + lds.part[2] + lds.part[3]);
    }
    __device__ __forceinline__ double weight(int i, const Staged &lds) const
    {
        return (double)(long long)lds.counts[i] / total;
    }
};

// p as it was made on the host (mapper.fragment_length_weights): row `row` of p[n][2000], read where it
// lies -- each weight is read once, by wave 0, 64 neighbours at a time
struct GivenWeights {
    struct Staged {};
    const double *p;
    __device__ __forceinline__ void stage(int64_t row, Staged &) { p += row * MAX_FRAGMENT_LENGTH; }
    __device__ __forceinline__ double weight(int i, const Staged &) const { return p[i]; }
};

// blockIdx.y is the row: row y of the source gives row y of out[gridDim.y][n_tx], each by the arithmetic
// of a launch on that row alone (the lengths are shared).
template <class Source>
__device__ __forceinline__ void effective_lengths_rows(Source source, const double *__restrict__ lengths, int64_t n_tx,
                                                       double *__restrict__ out)
{
    out += (int64_t)blockIdx.y * n_tx;
    // Only the bins with p_i != 0 are visited: a term max(len - i, 1) * 0.0 is +0.0 and adding
    // +0.0 leaves the running sum as it is, bit for bit (the sum starts at +0.0 and every term
    // is >= 0); a NaN bin (empty histogram: 0 / 0) is not zero and stays in.  A fragment-length
    // histogram has a few hundred occupied bins out of 2000.
    __shared__ double p[MAX_FRAGMENT_LENGTH];
    __shared__ int bin[MAX_FRAGMENT_LENGTH];
    __shared__ typename Source::Staged staged;
    __shared__ int n_bins;
    source.stage((int64_t)blockIdx.y, staged);
    // wave 0 packs the non-zero bins in bin order (ballot + prefix count per 64 bins)
    if (threadIdx.x < 64) {
        int n = 0;
        for (int first = 0; first < MAX_FRAGMENT_LENGTH; first += 64) {
            const int i = first + (int)threadIdx.x;
            const double v = i < MAX_FRAGMENT_LENGTH ? source.weight(i, staged) : 0.0;
            const bool keep = i < MAX_FRAGMENT_LENGTH && !(v == 0.0);
            const unsigned long long kept = __ballot(keep);
            if (keep) {
                const int at = n + __popcll(kept & ((1ULL << threadIdx.x) - 1));
                p[at] = v;
                bin[at] = i;
            }
            n += __popcll(kept);
        }
        if (threadIdx.x == 0) n_bins = n;
    }
    __syncthreads();
    const int n = n_bins;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tx;
         t += (int64_t)gridDim.x * blockDim.x) {
        const double len = lengths[t];
        double acc = 0.0;
        for (int k = 0; k < n; ++k) {
            double v = len - (double)bin[k];
            if (v < 1.0) v = 1.0;
            acc += v * p[k];
        }
        out[t] = acc;
    }
}

__global__ void __launch_bounds__(256)
effective_lengths_kernel(const unsigned long long *__restrict__ fld,
                         const double *__restrict__ lengths, int64_t n_tx, double *__restrict__ out)
{
    effective_lengths_rows(HistogramWeights{fld, 0.0}, lengths, n_tx, out);
}

// The same rule with p given instead of counted: a fragment-length model (--fragment-length / --sd).
// Weights are finite and >= 0 (the callers check), so a skipped bin is a zero bin as above.
__global__ void __launch_bounds__(256)
effective_lengths_weights_kernel(const double *__restrict__ p,
                                 const double *__restrict__ lengths, int64_t n_tx, double *__restrict__ out)
{
    effective_lengths_rows(GivenWeights{p}, lengths, n_tx, out);
}

// Counter-based generator for the bootstrap draw (the reference draws from
// numpy's unseeded global generator, so only the distribution can be matched).
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// multinomial(n, count / n) -- the draw of seekmer/infer.py:108-111 -- as n categorical draws
// over the integer cumulative counts, in two stages so that every draw is decided and counted
// in LDS: the classes are cut into tiles of `tile` classes (at most MN_TILES tiles, at most
// MN_TILES classes each);
//   stage 1  n draws r ~ U[0, total) choose a TILE (LDS counters, one global add per tile and
//            workgroup): the tile totals are multinomial(n, tile masses);
//   stage 2  one workgroup per tile makes its tile's m draws among the tile's classes
//            (cumulative counts relative to the tile in LDS, LDS counters) and writes the counts.
// n iid draws sorted into tiles and then, given the tile totals, iid within the tiles under the
// conditional probabilities ARE n iid draws over the classes: exactly the multinomial, only the
// random stream differs from drawing class by class.  (One draw per class-level binary search
// and one device-scope atomic per draw was 1.45 ms for 20 M draws over 1 M classes: the
// scattered atomics alone are bound at ~20 G/s.)  Counter-based generator: the reference draws
// from numpy's unseeded global generator, so only the distribution can be matched.
//
// A draw costs what its arithmetic costs (20 M draws are ~100 G integer multiplies when every
// draw takes its own 64-bit hash and a 64 x 64 multiply-high; 32-bit multiplies issue at a
// quarter of the rate), so: one 64-bit hash serves TWO draws, each an exactly uniform integer
// below the range from 32 bits by multiply-high with rejection (Lemire; rejected with
// probability range / 2^32, then redrawn from a stream keyed by the draw's number), and the interval holding r
// is found from a guide table over power-of-two buckets of r (one LDS read, then 1-2 steps
// forward) instead of a 12-step binary search.
constexpr int MN_TILES = 4096;
constexpr int MN_GUIDE_BITS = 12;

struct MnStream {
    uint64_t base, spare;      // counter-mode keys of the paired draws and of the redraws
    __device__ __forceinline__ MnStream(uint64_t seed, uint64_t stream_id, uint64_t part)
    {
        base = mix64(seed ^ (stream_id * 0x9E3779B97F4A7C15ULL) ^ (part * 0xC2B2AE3D27D4EB4FULL));
        spare = mix64(base ^ 0xA0761D6478BD642FULL);
    }
    // the two 32-bit words of draw pair number `pair`
    __device__ __forceinline__ uint64_t words(uint64_t pair) const { return mix64(base + pair * 0xD1342543DE82EF95ULL); }
};
// exactly uniform in [0, range), range >= 1, from 32 random bits; `reject_below` = 2^32 mod range.
// A rejected word is replaced from a stream keyed by (pair, which of its two draws, attempt): the
// result depends on the draw's number alone, not on which lane of which launch geometry makes it.
__device__ __forceinline__ uint32_t mn_bounded(uint32_t word, uint32_t range, uint32_t reject_below,
                                               const MnStream &rng, uint64_t pair, uint32_t which)
{
    uint64_t m = (uint64_t)word * range;
    for (uint64_t attempt = 1; (uint32_t)m < reject_below; ++attempt) {
        const uint64_t again = mix64(rng.spare + pair * 0xD1342543DE82EF95ULL + (2 * attempt + which) * 0x9FB21C651E98DF25ULL);
        m = (uint64_t)(uint32_t)(again >> 32) * range;
    }
    return (uint32_t)(m >> 32);
}

// Interval search over ascending cumulative counts cum[0..n) (cum[n-1] = total > r): guide[g] =
// first index whose cumulative count exceeds the smallest r of bucket g = r >> shift.
struct MnGuide {
    int shift;
    __device__ __forceinline__ static int shift_for(uint32_t total)
    {
        const int bits = 32 - __clz(total - 1 | 1u);                 // total <= 2^bits
        return max(0, bits - MN_GUIDE_BITS);
    }
};
// every thread i < n fills the buckets whose smallest r lies in [cum[i-1], cum[i])
__device__ __forceinline__ void mn_fill_guide(const uint32_t *cum, int n, int shift, uint16_t *guide)
{
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t lo = i ? cum[i - 1] : 0u, hi = cum[i];
        const uint32_t w = 1u << shift;
        // buckets g with g * w in [lo, hi)
        uint32_t g = (uint32_t)(((uint64_t)lo + w - 1) >> shift);
        const uint32_t g_end = (uint32_t)(((uint64_t)hi + w - 1) >> shift);
        for (; g < g_end; ++g) guide[g] = (uint16_t)i;
    }
}
__device__ __forceinline__ int mn_find(const uint32_t *cum, const uint16_t *guide, int shift, uint32_t r)
{
    int i = guide[r >> shift];
    while (cum[i] <= r) ++i;
    return i;
}

__global__ void __launch_bounds__(1024)
multinomial_tiles_kernel(const unsigned long long *__restrict__ cum, int64_t n_classes, int tile, int n_tiles,
                         int64_t n_draws, uint64_t seed, uint64_t stream_id, unsigned int *__restrict__ tile_total)
{
    __shared__ uint32_t tile_cum[MN_TILES];
    __shared__ unsigned int count[MN_TILES];
    __shared__ uint16_t guide[1 << MN_GUIDE_BITS];
    for (int k = threadIdx.x; k < n_tiles; k += blockDim.x) {
        tile_cum[k] = (uint32_t)cum[min(n_classes, (int64_t)(k + 1) * tile) - 1];     // (total < 2^32: checked by the caller)
        count[k] = 0;
    }
    __syncthreads();
    const uint32_t total = tile_cum[n_tiles - 1];
    const int shift = MnGuide::shift_for(total);
    mn_fill_guide(tile_cum, n_tiles, shift, guide);
    __syncthreads();
    const uint32_t reject_below = (uint32_t)(0u - total) % total;
    MnStream rng(seed, stream_id, 0);
    // draws 2p and 2p + 1 share hash number p; the workgroups split the pairs evenly
    const int64_t n_pairs = (n_draws + 1) >> 1;
    const int64_t first = n_pairs * blockIdx.x / gridDim.x, last = n_pairs * (blockIdx.x + 1) / gridDim.x;
    for (int64_t p = first + threadIdx.x; p < last; p += blockDim.x) {
        const uint64_t w = rng.words((uint64_t)p);
        const uint32_t r0 = mn_bounded((uint32_t)(w >> 32), total, reject_below, rng, (uint64_t)p, 0u);
        atomicAdd(&count[mn_find(tile_cum, guide, shift, r0)], 1u);
        if (2 * p + 1 < n_draws) {
            const uint32_t r1 = mn_bounded((uint32_t)w, total, reject_below, rng, (uint64_t)p, 1u);
            atomicAdd(&count[mn_find(tile_cum, guide, shift, r1)], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_tiles; k += blockDim.x)
        if (count[k]) atomicAdd(&tile_total[k], count[k]);
}

// counts[(first_class + i) * stride] = draws of class first_class + i, as f8 (the EM's class counts)
// (the guide keeps its 4096 buckets for a tile of a few hundred classes too: with 512 the scans
// through the light classes of a bucket made this kernel 128 us instead of 72; and 256-lane
// workgroups, four per CU by their LDS, ran 353 us)
__global__ void __launch_bounds__(1024)
multinomial_classes_kernel(const unsigned long long *__restrict__ cum, int64_t n_classes, int tile,
                           const unsigned int *__restrict__ tile_total, uint64_t seed, uint64_t stream_id,
                           double *__restrict__ counts, int stride)
{
    __shared__ uint32_t local_cum[MN_TILES];
    __shared__ unsigned int count[MN_TILES];
    __shared__ uint16_t guide[1 << MN_GUIDE_BITS];
    const int64_t first_class = (int64_t)blockIdx.x * tile;
    const int n = (int)min((int64_t)tile, n_classes - first_class);
    const unsigned long long before = first_class ? cum[first_class - 1] : 0ULL;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        local_cum[i] = (uint32_t)(cum[first_class + i] - before);
        count[i] = 0;
    }
    __syncthreads();
    const uint32_t mass = local_cum[n - 1];
    const unsigned int draws = tile_total[blockIdx.x];       // (0 when the tile has no mass)
    if (draws) {                                             // (uniform over the workgroup)
        const int shift = MnGuide::shift_for(mass);
        mn_fill_guide(local_cum, n, shift, guide);
        __syncthreads();
        const uint32_t reject_below = (uint32_t)(0u - mass) % mass;
        MnStream rng(seed, stream_id, 1 + blockIdx.x);
        const unsigned int n_pairs = (unsigned int)(((unsigned long long)draws + 1) >> 1);    // (draws may be 2^32 - 1)
        for (unsigned int p = threadIdx.x; p < n_pairs; p += blockDim.x) {
            const uint64_t w = rng.words(p);
            const uint32_t r0 = mn_bounded((uint32_t)(w >> 32), mass, reject_below, rng, p, 0u);
            atomicAdd(&count[mn_find(local_cum, guide, shift, r0)], 1u);
            if (2ull * p + 1 < draws) {
                const uint32_t r1 = mn_bounded((uint32_t)w, mass, reject_below, rng, p, 1u);
                atomicAdd(&count[mn_find(local_cum, guide, shift, r1)], 1u);
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) counts[(first_class + i) * stride] = (double)count[i];
}

// the abundance an EM that ran `ctl[CTL_ITERS]` steps left behind: x0 after an even number of
// steps, x1 after an odd one (the host does not know the count when it queues this)
__global__ void __launch_bounds__(256)
em_result_kernel(const unsigned long long *__restrict__ ctl, const double *__restrict__ x0,
                 const double *__restrict__ x1, int64_t n, double *__restrict__ out)
{
    const double *__restrict__ x = (ctl[CTL_ITERS] & 1ULL) ? x1 : x0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) out[i] = x[i];
}

__global__ void __launch_bounds__(256)
permute_f64_kernel(const double *__restrict__ x, const int32_t *__restrict__ perm, int64_t n,
                   double *__restrict__ y, bool scatter)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (scatter) y[perm[i]] = x[i]; else y[i] = x[perm[i]];
    }
}

__global__ void __launch_bounds__(256)
u64_to_double_kernel(const unsigned long long *__restrict__ in, int64_t n, double *__restrict__ out)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (double)in[i];
}

__global__ void __launch_bounds__(256)
double_to_cum_u64_kernel(const double *__restrict__ in, int64_t n, unsigned long long *__restrict__ out)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (unsigned long long)in[i];
}

// ASCII pooled contig bases -> 2-bit words (first base in the top bits)
__global__ void __launch_bounds__(256)
pack_sequences_kernel(const char *__restrict__ bases, int64_t n_bases, uint64_t *__restrict__ seq2,
                      int64_t n_words)
{
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < n_words;
         w += (int64_t)gridDim.x * blockDim.x) {
        uint64_t c = 0;
        const int64_t first = w * 32;
        for (int i = 0; i < 32 && first + i < n_bases; ++i)
            c |= (uint64_t)two_bit_encode((uint8_t)bases[first + i]) << (62 - 2 * i);
        seq2[w] = c;
    }
}

static inline unsigned grid_for(int64_t n, int64_t cap = 256 * 16)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

static inline unsigned chip_grid(int64_t work_items, int items_per_block)
{
    int64_t blocks = (work_items + items_per_block - 1) / items_per_block;
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 8) blocks = 256 * 8;
    return (unsigned)blocks;
}

// blocks of the launch that writes the stopping rule's partials = partials the judge reads:
// em_finalize's (several ranks) or em_rows_finalize's (p.fused)
int em_final_blocks(const EmProblem &p)
{
    int64_t blocks = p.fused ? (p.n_rows + 31) / 32 : (p.n_tx + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > EM_FINAL_BLOCKS) blocks = EM_FINAL_BLOCKS;
    return (int)blocks;
}

void launch_em_inner(const EmProblem &p, int parity, bool judge_previous, int64_t steps_done, hipStream_t stream)
{
    hipLaunchKernelGGL(em_inner_kernel, dim3(chip_grid(p.n_classes, 256)), dim3(256), 0, stream, p, parity,
                       judge_previous ? em_final_blocks(p) : 0, steps_done);
}

void launch_em_decide(const EmProblem &p, int64_t steps_done, hipStream_t stream)
{
    hipLaunchKernelGGL(em_decide_kernel, dim3(1), dim3(256), 0, stream, p, em_final_blocks(p), steps_done);
}

void launch_em_rows(const EmProblem &p, int parity, hipStream_t stream)
{
    hipLaunchKernelGGL(em_rows_kernel, dim3(chip_grid(p.n_rows, 32)), dim3(256), 0, stream, p, parity);
}

void launch_em_rows_finalize(const EmProblem &p, int parity, hipStream_t stream)
{
    hipLaunchKernelGGL(em_rows_finalize_kernel<false>, dim3((unsigned)em_final_blocks(p)), dim3(256), 0, stream, p, parity);
}

void launch_em_rows_acc(const EmProblem &p, int parity, hipStream_t stream)
{
    EmProblem fused = p;
    fused.fused = 1;                            // (the grid of the fused form)
    hipLaunchKernelGGL(em_rows_finalize_kernel<true>, dim3((unsigned)em_final_blocks(fused)), dim3(256), 0, stream, p, parity);
}

void launch_em_local_chunk(const EmProblem &p, const EmTiles &tiles, const double *x_in, int n_steps, int64_t first_step,
                           hipStream_t stream)
{
    if (tiles.n_tiles <= 0 || n_steps <= 0) return;
    hipLaunchKernelGGL(em_local_chunk_kernel, dim3((unsigned)tiles.n_tiles), dim3(256), 0, stream, p, tiles, x_in,
                       std::min(n_steps, EM_CHUNK_MAX), first_step);
}

#if SKM_EM_JUDGE_LAUNCH
void launch_em_local_decide(const EmProblem &p, const EmTiles &tiles, int64_t first_step, int n_steps, hipStream_t stream)
{
    hipLaunchKernelGGL(em_local_decide_kernel, dim3(1), dim3(64 * EM_CHUNK_MAX), 0, stream, p, tiles, first_step,
                       std::min(n_steps, EM_CHUNK_MAX));
}
#endif

void launch_em_rows_to_acc(const EmProblem &p, hipStream_t stream)
{
    hipLaunchKernelGGL(em_rows_to_acc_kernel, dim3(chip_grid(p.n_tx, 256)), dim3(256), 0, stream, p);
}

void launch_em_finalize(const EmProblem &p, int parity, bool from_acc, hipStream_t stream)
{
    const int blocks = em_final_blocks(p);
    if (from_acc)
        hipLaunchKernelGGL(em_finalize_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, p, parity);
    else
        hipLaunchKernelGGL(em_finalize_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, p, parity);
}

// ---- numpy.sum of a contiguous f8 array, bit for bit ----------------------
// numpy adds the array up in blocks of 8192 elements (its reduction buffer),
// block sums accumulated left to right, and each block with pairwise_sum:
// below 8 elements a plain loop, up to 128 eight strided accumulators combined
// as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus the remainder in order, above
// that a split at n/2 rounded down to a multiple of 8 (numpy/_core/src/umath/
// loops_utils.h.src).  The start vector x /= x.sum() (seekmer/infer.py:118-119)
// and the TPM scaling (:127-129) go through it, so doing them on the device
// without it would move the EM input by an ulp.
// A full block of 8192 elements splits evenly all the way down: 64 leaves of 128 elements,
// combined as a balanced binary tree.  Eight lanes per leaf run numpy's eight strided
// accumulators (lane j adds elements j, j + 8, ... of the leaf in order), the combination
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) is a three-step butterfly over those lanes and the 64 leaf
// sums meet in a six-step butterfly -- the same additions in the same association (a + b = b + a
// exactly, so only the shape of the tree matters).
__device__ __forceinline__ void np_sum_full_block(const double *__restrict__ a, double *__restrict__ out)
{
    __shared__ double leaf[64];
    const int l = threadIdx.x >> 3, j = threadIdx.x & 7;          // 512 lanes: leaf, accumulator
    const double *p = a + l * 128 + j;
    double r = p[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) r += p[8 * i];
    r += __shfl_xor(r, 1, 8);
    r += __shfl_xor(r, 2, 8);
    r += __shfl_xor(r, 4, 8);
    if (j == 0) leaf[l] = r;
    __syncthreads();
    if (threadIdx.x < 64) {
        double s = leaf[threadIdx.x];
        for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
        if (threadIdx.x == 0) *out = s;
    }
}

// The last block of an array, 0 < len < 8192 elements, in the same shape.  Its tree depends on len alone and is at
// most seven splits deep (8191 -> 4103 -> 2055 -> 1031 -> 519 -> 263 -> 135 -> 71), so a node is named by the turns
// that lead to it, left = 0, right = 1, first turn in the highest of seven bits, the rest zero: 128 names, a node and
// its left child share one.  Eight lanes take a name, walk down from the root (no recursion, no list of leaves) and,
// if the walk ends at a leaf just as the turns run out, add the leaf up as numpy does: eight strided accumulators,
// the butterfly, then lane 0 the up to seven elements left over in order (a leaf below eight elements, which only
// a block below eight has: lane 0 alone, in order).  The leaf sums then meet level by level from the deepest: a
// lane per node walks to it and, if it was split, adds its right child's sum to the left child's, which stands
// under the node's own name.  The same additions in the same association as pairwise_sum's recursion.
constexpr int NP_SPLITS = 7, NP_NAMES = 1 << NP_SPLITS;

// the node reached from the root of a block of len elements by the highest `turns` bits of `name`: first element,
// size, and the number of turns made before a leaf ended the walk
__device__ __forceinline__ int np_walk(int len, int name, int turns, int *lo_out, int *n_out)
{
    int lo = 0, n = len, d = 0;
    for (; d < turns && n > 128; ++d) {
        int n2 = n / 2;
        n2 -= n2 % 8;
        if ((name >> (NP_SPLITS - 1 - d)) & 1) { lo += n2; n -= n2; } else n = n2;
    }
    *lo_out = lo; *n_out = n;
    return d;
}

__device__ __forceinline__ void np_sum_partial_block(const double *__restrict__ a, int len, double *__restrict__ out)
{
    __shared__ double node[NP_NAMES];
    const int j = threadIdx.x & 7;
    for (int name = threadIdx.x >> 3; name < NP_NAMES; name += 64) {          // (two turns of 64 names, block-uniform)
        int lo, n;
        const int d = np_walk(len, name, NP_SPLITS, &lo, &n);
        // (a leaf d turns down stands under the name whose other bits are zero; the rest of the names are idle)
        const bool mine = (name & ((1 << (NP_SPLITS - d)) - 1)) == 0;
        const int whole = n - n % 8;
        double r = 0.0;
        if (mine && n >= 8) {
            r = a[lo + j];
            for (int i = 8 + j; i < whole; i += 8) r += a[lo + i];
        }
        r += __shfl_xor(r, 1, 8);
        r += __shfl_xor(r, 2, 8);
        r += __shfl_xor(r, 4, 8);
        if (mine && j == 0) {
            for (int i = n >= 8 ? whole : 0; i < n; ++i) r += a[lo + i];     // numpy starts from -0.0 + a[0]; same value for our data
            node[name] = r;
        }
    }
    __syncthreads();
    for (int level = NP_SPLITS - 1; level >= 0; --level) {
        if ((int)threadIdx.x < (1 << level)) {
            const int name = threadIdx.x << (NP_SPLITS - level);
            int lo, n;
            const int d = np_walk(len, name, level, &lo, &n);
            if (d == level && n > 128) node[name] += node[name + (1 << (NP_SPLITS - 1 - level))];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = node[0];
}

__global__ void __launch_bounds__(512)
np_sum_blocks_kernel(const double *__restrict__ a, int64_t n, double *__restrict__ block_sums, int64_t stride)
{
    // (blockIdx.y: one of several vectors `stride` elements apart, its block sums after the others')
    a += blockIdx.y * stride;
    block_sums += blockIdx.y * (int64_t)gridDim.x;
    const int64_t first = blockIdx.x * (int64_t)8192;
    const int len = (int)min((int64_t)8192, n - first);
    if (len == 8192) {                      // (block-uniform)
        np_sum_full_block(a + first, block_sums + blockIdx.x);
        return;
    }
    np_sum_partial_block(a + first, len, block_sums + blockIdx.x);
}

// out[0] = the sum, out[1] = sum / divisor (vector blockIdx.x of several: its own block sums and pair)
__global__ void np_sum_final_kernel(const double *block_sums, int64_t n_blocks, double divisor, double *out)
{
    if (threadIdx.x != 0) return;
    block_sums += blockIdx.x * n_blocks;
    out += blockIdx.x * 2;
    double acc = 0.0;
    for (int64_t b = 0; b < n_blocks; ++b) acc += block_sums[b];
    out[0] = acc;
    out[1] = acc / divisor;
}

__global__ void __launch_bounds__(256)
reciprocal_kernel(const double *__restrict__ l, int64_t n, double *__restrict__ x)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) x[i] = 1.0 / l[i];
}

// x /= *s, then (TPM) x[x < floor] = 0
__global__ void __launch_bounds__(256)
divide_kernel(double *__restrict__ x, int64_t n, const double *__restrict__ s, bool threshold, double floor,
              int64_t stride)
{
    x += blockIdx.y * stride;                 // (one of several vectors, each with its own divisor pair)
    const double d = s[blockIdx.y * 2];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        double v = x[i] / d;
        if (threshold && v < floor) v = 0.0;
        x[i] = v;
    }
}

void launch_np_sum(const double *a, int64_t n, double divisor, double *block_sums, double *out,
                   hipStream_t stream)
{
    const int64_t n_blocks = (n + 8191) / 8192;
    if (n_blocks)
        hipLaunchKernelGGL(np_sum_blocks_kernel, dim3((unsigned)n_blocks), dim3(512), 0, stream,
                           a, n, block_sums, (int64_t)0);
    hipLaunchKernelGGL(np_sum_final_kernel, dim3(1), dim3(1), 0, stream, block_sums, n_blocks, divisor, out);
}

// the same for `count` vectors of n elements, `stride` apart: block_sums holds count * ceil(n / 8192)
// doubles, out[2 v] = sum of vector v, out[2 v + 1] = sum / divisor
void launch_np_sum_many(const double *a, int64_t n, int64_t count, int64_t stride, double divisor,
                        double *block_sums, double *out, hipStream_t stream)
{
    const int64_t n_blocks = (n + 8191) / 8192;
    for (int64_t v0 = 0; v0 < count; v0 += 32768) {              // (gridDim.y is limited to 65535)
        const unsigned here = (unsigned)std::min<int64_t>(32768, count - v0);
        if (n_blocks)
            hipLaunchKernelGGL(np_sum_blocks_kernel, dim3((unsigned)n_blocks, here), dim3(512), 0, stream,
                               a + v0 * stride, n, block_sums + v0 * n_blocks, stride);
        hipLaunchKernelGGL(np_sum_final_kernel, dim3(here), dim3(1), 0, stream, block_sums + v0 * n_blocks, n_blocks,
                           divisor, out + 2 * v0);
    }
}

void launch_reciprocal(const double *l, int64_t n, double *x, hipStream_t stream)
{
    hipLaunchKernelGGL(reciprocal_kernel, dim3(grid_for(n)), dim3(256), 0, stream, l, n, x);
}

void launch_divide(double *x, int64_t n, const double *s, bool threshold, double floor, hipStream_t stream)
{
    hipLaunchKernelGGL(divide_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, n, s, threshold, floor, (int64_t)0);
}

// vector v of `count` (n elements, `stride` apart) divided by s[2 v]
void launch_divide_many(double *x, int64_t n, int64_t count, int64_t stride, const double *s, bool threshold,
                        double floor, hipStream_t stream)
{
    for (int64_t v0 = 0; v0 < count; v0 += 32768) {
        const unsigned here = (unsigned)std::min<int64_t>(32768, count - v0);
        hipLaunchKernelGGL(divide_kernel, dim3(std::min<unsigned>(grid_for(n), 64u), here), dim3(256), 0, stream,
                           x + v0 * stride, n, s + 2 * v0, threshold, floor, stride);
    }
}

void launch_effective_lengths(const unsigned long long *fld, const double *lengths, int64_t n_tx,
                              double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(effective_lengths_kernel, dim3(grid_for(n_tx)), dim3(256), 0, stream, fld,
                       lengths, n_tx, out);
}

// rows of one launch (n <= 65535: gridDim.y; the callers' groups are smaller).  Every block packs its row
// first: few blocks per row when there are many of them.
static unsigned effective_lengths_blocks_per_row(int64_t n, int64_t n_tx)
{
    return std::min<unsigned>(grid_for(n_tx), n >= 64 ? 16u : 256u);
}

void launch_effective_lengths_many(const unsigned long long *fld, int64_t n, const double *lengths, int64_t n_tx,
                                   double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(effective_lengths_kernel, dim3(effective_lengths_blocks_per_row(n, n_tx), (unsigned)n), dim3(256), 0,
                       stream, fld, lengths, n_tx, out);
}

void launch_effective_lengths_weights(const double *p, int64_t n, const double *lengths, int64_t n_tx, double *out,
                                      hipStream_t stream)
{
    // one row: the grid of launch_effective_lengths
    const unsigned per_row = n == 1 ? (unsigned)grid_for(n_tx) : effective_lengths_blocks_per_row(n, n_tx);
    hipLaunchKernelGGL(effective_lengths_weights_kernel, dim3(per_row, (unsigned)n), dim3(256), 0, stream, p, lengths, n_tx, out);
}

int multinomial_tile(int64_t n_classes)
{
    int tile = 1;
    while ((n_classes + tile - 1) / tile > MN_TILES) tile <<= 1;
    return tile;
}

// tile_total: MN_TILES unsigned ints of scratch; counts[c * stride] receives class c's draws as f8.
// false when the table is too large for the tiled draw (more than MN_TILES^2 classes)
bool launch_multinomial(const unsigned long long *cum, int64_t n_classes, int64_t n_draws,
                        uint64_t seed, uint64_t stream_id, unsigned int *tile_total, double *counts,
                        int stride, hipStream_t stream)
{
    if (n_classes <= 0) return true;
    const int tile = multinomial_tile(n_classes);
    if (tile > MN_TILES || n_draws >= (1LL << 32)) return false;
    const int n_tiles = (int)((n_classes + tile - 1) / tile);
    (void)hipMemsetAsync(tile_total, 0, MN_TILES * sizeof(unsigned int), stream);
    if (n_draws > 0)
        hipLaunchKernelGGL(multinomial_tiles_kernel, dim3(512), dim3(1024), 0, stream, cum, n_classes, tile,
                           n_tiles, n_draws, seed, stream_id, tile_total);
    hipLaunchKernelGGL(multinomial_classes_kernel, dim3((unsigned)n_tiles), dim3(1024), 0, stream, cum, n_classes,
                       tile, tile_total, seed, stream_id, counts, stride);
    return true;
}

void launch_em_result(const unsigned long long *ctl, const double *x0, const double *x1, int64_t n, double *out,
                      hipStream_t stream)
{
    hipLaunchKernelGGL(em_result_kernel, dim3(grid_for(n)), dim3(256), 0, stream, ctl, x0, x1, n, out);
}

void launch_permute_f64(const double *x, const int32_t *perm, int64_t n, double *y, bool scatter,
                        hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(permute_f64_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, perm, n, y, scatter);
}

void launch_u64_to_double(const unsigned long long *in, int64_t n, double *out, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(u64_to_double_kernel, dim3(grid_for(n)), dim3(256), 0, stream, in, n, out);
}

void launch_double_to_u64(const double *in, int64_t n, unsigned long long *out, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(double_to_cum_u64_kernel, dim3(grid_for(n)), dim3(256), 0, stream, in, n, out);
}

void launch_pack_sequences(const char *bases, int64_t n_bases, uint64_t *seq2, int64_t n_words,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(pack_sequences_kernel, dim3(grid_for(n_words)), dim3(256), 0, stream, bases,
                       n_bases, seq2, n_words);
}

void warm_code_em()
{
    hipFuncAttributes attributes;
    (void)hipFuncGetAttributes(&attributes, reinterpret_cast<const void *>(&em_inner_kernel));
}

}  // namespace skm

// ------------------------------------------------------------ diagnostics
// Random 16-byte gathers over a table of `n_slots` slots: the ceiling the
// index probes of the mapper can be priced against.  `chain` = 1:
// every lane's next address depends on the slot it just read (latency under
// load); `chain` = 0: `per_lane` independent gathers (throughput).
namespace skm {
__global__ void __launch_bounds__(256)
gather_probe_kernel(const uint4 *__restrict__ table, uint64_t slot_mask, int per_lane, int chain,
                    unsigned long long *sink)
{
    uint64_t x = mix64(blockIdx.x * (uint64_t)blockDim.x + threadIdx.x + 1);
    unsigned long long acc = 0;
    if (chain) {
        for (int i = 0; i < per_lane; ++i) {
            const uint4 v = table[x & slot_mask];
            acc += v.x;
            x = mix64(x + v.y + i);
        }
    } else {
        for (int i = 0; i < per_lane; i += 4) {
            const uint64_t a = mix64(x + i), b2 = mix64(x + i + 1), c = mix64(x + i + 2), d = mix64(x + i + 3);
            const uint4 v0 = table[a & slot_mask], v1 = table[b2 & slot_mask], v2 = table[c & slot_mask],
                        v3 = table[d & slot_mask];
            acc += v0.x + v1.x + v2.x + v3.x;
        }
    }
    if (acc == 0x123456789ULL) *sink = acc;
}

void launch_gather_probe(const void *table, uint64_t n_slots, int blocks, int per_lane, int chain,
                         unsigned long long *sink, hipStream_t stream)
{
    hipLaunchKernelGGL(gather_probe_kernel, dim3(blocks), dim3(256), 0, stream, (const uint4 *)table,
                       n_slots - 1, per_lane, chain, sink);
}
}  // namespace skm
