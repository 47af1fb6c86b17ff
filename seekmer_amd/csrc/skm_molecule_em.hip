// Distributed molecules ("Distributed molecules"): the groups of "Resolved molecules" -- the
// distinct classes among a sample's live molecules with one UMI -- keep the whole intersection I of their gene sets,
// -1 ("no gene") as the element n_genes, the sink.  One element: the group adds 1 to that row of its cell; 2 to
// GENE_SET_MAX elements: the group is a set, shared out among its rows by an EM per cell; more: wide, none: collision,
// both tallied only.  A post-pass beside the resolved matrix, over the same sorted keys, classes and runs:
//   1. sets: the walk of molecule_resolve_kernel (skm_molecule_resolve.hip; a copy, so that kernel keeps its registers),
//      but every 64-candidate chunk of the pivot is walked and the distinct surviving values are collected across the
//      chunks: lane k of the wave holds the k-th distinct value, a value is appended when no lane holds it yet, the
//      seventeenth makes the group wide and ends it.  The values are then ranked by comparison and stored in ascending
//      order into the group's stage of GENE_SET_MAX words; group_len[] is the list's length (0: wide or collision),
//      group_cell[] the group's sample.  A group of one class goes through gene_classify: inside one gene or unnamed is
//      a list of one, ambiguous takes the wave's path with no other member.
//   2. elements: three scans over the groups (list lengths; sets; set lengths) number the elements, the sets and the
//      places of the set-major lists; every element becomes the key cell << 32 | element with its number.
//   3. rows (after ONE stable sort_pairs_u64 by that key, the caller's): heads and their scan number the rows; a pass
//      over the sorted elements gives every cell its row range and every row its element, adds the lists of one into
//      the integer u[row], flags the elements of sets and scatters their row into the set-major lists; the scan of
//      the flags places the transposed view (row -> set numbers, ascending because the sort is stable).
//   4. gene_em_kernel: one block of 256 lanes per cell, all steps in one launch.  x lives in LDS while the cell's rows
//      fit GENE_EM_LDS_ROWS and in the cell's slice of the output otherwise (the same body); d[] lives in HBM.  Phase A:
//      a lane per set adds its rows' x in ascending row order.  Phase B: eight lanes per row add x / d over the row's
//      sets in em_row_sum's order (skm_em_core.h), lane 0 of the eight stores x' in place (a row's new value reads its
//      own old value and d[] alone) and notes the change; the block's verdict goes through LDS, so every lane takes
//      the same branch at every barrier.  The loop ends by the stopping rule or at max_steps.
//   5. fill: rows with a gene and x >= GENE_EM_FLOOR are flagged and scanned, then indices, data, indptr, the tally's
//      rows, steps and capped words and to_unnamed are written.
// Doubles are added in one fixed order and never atomically; integer atomics add to u[] and the tally alone.  No
// scratch, no recursion, no inline assembly; every loop is bounded by n, a tuple's length, 64, GENE_SET_MAX or
// max_steps; no lane leaves a whole-wave part before its shuffles and ballots, none leaves the EM's block before its
// last barrier.  Every id is checked against n_tx before it indexes tx_gene (error[0] = SKM_ERR_ARG), every place,
// class index, group number, sample, row and set against its bound (error[1] = SKM_ERR_STATE).
#include "../../include/seekmer_hip.h"
#include "skm_em_core.h"
#include "skm_gene_rule.h"
#include "skm_kernels.h"

#include <algorithm>
#include <climits>

namespace skm {

namespace {

constexpr int NO_GENE = INT_MIN;              // a lane without an id (genes are >= -1)

__device__ __forceinline__ int class_length(const GeneClasses &t, int64_t c)
{
    return (int)(t.len ? t.len[c] : t.start[c + 1] - t.start[c]);
}

// the gene of the id at arena place `at`; NO_GENE and *error = SKM_ERR_ARG for an id not below n_tx
__device__ __forceinline__ int gene_at(const GeneClasses &t, int64_t at, const int32_t *tx_gene, int64_t n_tx, int *error)
{
    const uint32_t id = (uint32_t)t.ids[at];
    if (id >= (uint64_t)n_tx) { *error = SKM_ERR_ARG; return NO_GENE; }
    return tx_gene[id];
}

// tally[word] += the lanes of the wave with `mine` and that word: summed through the wave, one atomic per distinct word
__device__ inline void wave_count(int64_t word, bool mine, int lane, unsigned long long *tally)
{
    unsigned long long todo = __ballot(mine);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        const int64_t src_word = __shfl(word, src);
        const unsigned long long same = __ballot(word == src_word) & todo;
        if (lane == src) atomicAdd(tally + src_word, (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

// keys[] / classes[] in sorted order, runs[n + 1] the exclusive scan of the heads with its total n_groups (what
// molecule_resolve_kernel takes).  stage[n_groups][GENE_SET_MAX], group_len[n_groups] (zeroed), group_cell[n_groups].
// Two kernels, so that neither keeps more than its registers hold: the first takes the groups of one class by the gene
// rule itself -- inside one gene or unnamed is a list of one -- and leaves group_len = GENE_SET_WAVE for the second: a
// group of several members, or of one ambiguous class, which goes the same way with no other member.
constexpr int GENE_SET_WAVE = -1;

__global__ void __launch_bounds__(256)
molecule_sets_single_kernel(GeneClasses t, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ classes,
                            const int64_t *__restrict__ runs, int64_t n, int64_t n_groups, const int32_t *__restrict__ tx_gene,
                            int64_t n_tx, int n_genes, int64_t n_samples, int32_t *__restrict__ stage,
                            int32_t *__restrict__ group_len, int32_t *__restrict__ group_cell, unsigned long long *tally,
                            int *error)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    // (no lane leaves before the wave's shared parts below: a lane that owns no group just has nothing to add)
    int64_t group = -1, sample = 0, c = t.n_classes;
    bool head = false, single = false;
    if (i < n) {
        const int64_t g = runs[i];
        if (runs[i + 1] != g) {
            sample = (int64_t)(keys[i] >> 32);
            if (g < 0 || g >= n_groups || sample >= n_samples) error[1] = SKM_ERR_STATE;
            else {
                head = true;
                group = g;
                single = i + 1 == n || runs[i + 2] != g + 1;
                if (single) {
                    c = classes[i];
                    if (c >= t.n_classes) { error[1] = SKM_ERR_STATE; c = t.n_classes; }
                }
            }
        }
    }
    int outcome = -1, length = head && !single ? GENE_SET_WAVE : 0;
    const GeneClass one = gene_classify(t, c, lane, tx_gene, n_tx, 0, n_samples, error);
    if (head && single) {
        if (one.kind == GENE_KIND_NONE || one.sample != sample) error[1] = SKM_ERR_STATE;
        else if (one.kind == GENE_KIND_UNIQUE) { outcome = GENE_EM_RESOLVED; length = 1; stage[group * GENE_SET_MAX] = one.gene; }
        else if (one.kind == GENE_KIND_UNNAMED) { outcome = GENE_EM_UNNAMED; length = 1; stage[group * GENE_SET_MAX] = n_genes; }
        else length = GENE_SET_WAVE;
    }
    if (head) {
        group_len[group] = length;
        group_cell[group] = (int32_t)sample;
    }
    wave_count(sample * GENE_EM_TALLY + outcome, head && outcome >= 0, lane, tally);
}

__global__ void __launch_bounds__(256)
molecule_sets_kernel(GeneClasses t, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ classes,
                     const int64_t *__restrict__ runs, int64_t n, int64_t n_groups, const int32_t *__restrict__ tx_gene,
                     int64_t n_tx, int n_genes, int64_t n_samples, int32_t *__restrict__ stage, int32_t *group_len,
                     unsigned long long *tally, int *error)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    // (no lane leaves before the wave's shared parts below: a lane that owns no group just has nothing to add)
    int64_t group = -1, sample = 0;
    bool by_wave = false;
    if (i < n) {
        const int64_t g = runs[i];
        if (runs[i + 1] != g && g >= 0 && g < n_groups) {
            sample = (int64_t)(keys[i] >> 32);
            group = g;
            by_wave = sample < n_samples && group_len[g] == GENE_SET_WAVE;     // (a head the first kernel refused stays 0)
        }
    }
    int outcome = -1, length = 0;

    // by the whole wave (everything but `lane`, `held` and what a lane loads is the same in all lanes)
    unsigned long long todo = __ballot(by_wave);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int64_t first = __shfl(i, src), inside = __shfl(group, src) + 1;   // runs[p + 1] of a member p
        // the members first .. first + count - 1 and the pivot: the first member with the fewest ids
        // (places inside the group are counted from `first`: a group has fewer than 2^31 members, checked below)
        int count = 0, best_at = 0;
        int best_len = INT_MAX;
        for (int64_t base = first; base < n && count < INT_MAX - 64; base += 64) {
            const int64_t p = base + lane;
            const bool member = p < n && runs[p + 1] == inside;
            if (member) {
                const int64_t mc = classes[p];
                if (mc >= t.n_classes) error[1] = SKM_ERR_STATE;
                else {
                    const int len = class_length(t, mc);
                    if (len < best_len) { best_len = len; best_at = (int)(p - first); }
                }
            }
            const unsigned long long in = __ballot(member);
            count += __popcll(in);
            if (in != ~0ULL) break;
        }
        if (count >= INT_MAX - 64) error[1] = SKM_ERR_STATE;
        int pivot_len = best_len;
        for (int step = 32; step > 0; step >>= 1) {
            const int theirs = __shfl_xor(pivot_len, step);
            if (theirs < pivot_len) pivot_len = theirs;
        }
        int pivot_at = best_len == pivot_len ? best_at : INT_MAX;
        for (int step = 32; step > 0; step >>= 1) {
            const int theirs = __shfl_xor(pivot_at, step);
            if (theirs < pivot_at) pivot_at = theirs;
        }
        int held = NO_GENE, n_held = 0;           // lane k < n_held holds the k-th distinct element met; GENE_SET_MAX + 1: wide
        if (pivot_len != INT_MAX && pivot_at >= 0 && pivot_at < count && count < INT_MAX - 64) {
            const int64_t pivot_start = t.start[classes[first + pivot_at]];
            for (int chunk = 0; chunk < pivot_len && n_held <= GENE_SET_MAX; chunk += 64) {
                const int cand = chunk + lane < pivot_len ? gene_at(t, pivot_start + chunk + lane, tx_gene, n_tx, error) : NO_GENE;
                bool alive = cand != NO_GENE;
                for (int p = 0; p < count && __any(alive); ++p) {
                    const int64_t mc = classes[first + p];
                    if (p == pivot_at || mc >= t.n_classes) continue;
                    const int64_t m_start = t.start[mc];
                    const int m_len = class_length(t, mc);
                    bool hit = false;
                    for (int base = 0; base < m_len && __any(alive && !hit); base += 64) {
                        const int mine = base + lane < m_len ? gene_at(t, m_start + base + lane, tx_gene, n_tx, error) : NO_GENE;
#pragma unroll
                        for (int k = 0; k < 64; ++k) hit |= __shfl(mine, k) == cand;
                    }
                    alive = alive && hit;
                }
                // the chunk's survivors, one distinct value after the other, appended where no lane holds them yet
                unsigned long long left = __ballot(alive);
                while (left && n_held <= GENE_SET_MAX) {
                    const int v = __shfl(cand, __ffsll(left) - 1);
                    left &= ~__ballot(cand == v);
                    const int element = v < 0 ? n_genes : v;
                    if (__any(lane < n_held && held == element)) continue;
                    if (lane == n_held) held = element;       // (lane GENE_SET_MAX holds the one too many: never read)
                    ++n_held;
                }
            }
        }
        int verdict = GENE_EM_COLLISION;
        if (n_held > GENE_SET_MAX) verdict = GENE_EM_WIDE;
        else if (n_held > 0) {
            int rank = 0;                         // the elements below this lane's: its place in ascending order
#pragma unroll 1
            for (int k = 0; k < n_held; ++k) rank += __shfl(held, k) < held ? 1 : 0;
            if (lane < n_held) stage[(inside - 1) * GENE_SET_MAX + rank] = held;     // (inside - 1 = the group: checked at its head)
            verdict = n_held > 1 ? GENE_EM_DISTRIBUTED : __shfl(held, 0) < n_genes ? GENE_EM_RESOLVED : GENE_EM_UNNAMED;
        }
        if (lane == src) {
            outcome = verdict;
            length = verdict == GENE_EM_WIDE || verdict == GENE_EM_COLLISION ? 0 : n_held;
        }
    }

    if (by_wave) group_len[group] = outcome >= 0 ? length : 0;
    wave_count(sample * GENE_EM_TALLY + outcome, by_wave && outcome >= 0, lane, tally);
}

// the three words of a group that are scanned: its elements, 1 where it is a set, its elements where it is a set
__global__ void __launch_bounds__(256)
gene_sets_sizes_kernel(const int32_t *__restrict__ group_len, int64_t n_groups, int64_t *__restrict__ elements,
                       int64_t *__restrict__ is_set, int64_t *__restrict__ set_elements)
{
    const int64_t g = blockIdx.x * 256LL + threadIdx.x;
    if (g >= n_groups) return;
    int len = group_len[g];
    if (len < 0 || len > GENE_SET_MAX) len = 0;
    elements[g] = len;
    is_set[g] = len >= 2;
    set_elements[g] = len >= 2 ? len : 0;
}

// a lane per stage word: element el_start[g] + k of the n_elements gets its key, number and group; the first of a
// set's words stores the set's place in the set-major lists, group 0's lane the end of the last
__global__ void __launch_bounds__(256)
gene_sets_elements_kernel(const int32_t *__restrict__ stage, const int32_t *__restrict__ group_len,
                          const int32_t *__restrict__ group_cell, int64_t n_groups, const int64_t *__restrict__ el_start,
                          const int64_t *__restrict__ set_of, const int64_t *__restrict__ set_place, int64_t n_elements,
                          int64_t n_sets, unsigned long long *__restrict__ el_key, int32_t *__restrict__ el_number,
                          int32_t *__restrict__ el_group, int64_t *__restrict__ set_start, int *error)
{
    const int64_t word = blockIdx.x * 256LL + threadIdx.x;
    const int64_t g = word / GENE_SET_MAX;
    const int k = (int)(word % GENE_SET_MAX);
    if (g >= n_groups) return;
    if (word == 0) set_start[n_sets] = set_place[n_groups];
    const int len = group_len[g];
    if (k >= len || len > GENE_SET_MAX) return;
    const int64_t e = el_start[g] + k;
    if (e < 0 || e >= n_elements) { error[1] = SKM_ERR_STATE; return; }
    el_key[e] = (unsigned long long)(uint32_t)group_cell[g] << 32 | (uint32_t)stage[word];
    el_number[e] = (int32_t)e;
    el_group[e] = (int32_t)g;
    if (k == 0 && len >= 2) {
        const int64_t j = set_of[g];
        if (j < 0 || j >= n_sets) error[1] = SKM_ERR_STATE;
        else set_start[j] = set_place[g];
    }
}

__global__ void __launch_bounds__(256)
gene_rows_heads_kernel(const unsigned long long *__restrict__ keys, int64_t n, int64_t *__restrict__ heads)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i < n) heads[i] = i == 0 || keys[i - 1] != keys[i];
}

// the group of sorted place i, or -1 with error[1] set
__device__ __forceinline__ int64_t gene_rows_group(const int32_t *order, const int32_t *el_group, int64_t i, int64_t n,
                                                   int64_t n_groups, int64_t &from, int *error)
{
    from = (int64_t)(uint32_t)order[i];
    if (from >= n) { error[1] = SKM_ERR_STATE; return -1; }          // (a sort's values are a permutation of 0 .. n - 1)
    const int64_t g = el_group[from];
    if (g < 0 || g >= n_groups) { error[1] = SKM_ERR_STATE; return -1; }
    return g;
}

__global__ void __launch_bounds__(256)
gene_rows_kernel(GeneRows p)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i > p.n) return;
    const unsigned long long key = i < p.n ? p.keys[i] : (unsigned long long)p.n_cells << 32;
    const unsigned long long before = i > 0 ? p.keys[i - 1] : 0;
    const int64_t heads_before = p.runs[i];
    // the cells that begin at place i: those after the one of place i - 1, up to the one of place i (molecule_fill_kernel's way)
    const int64_t cell_from = i == 0 ? 0 : (int64_t)(before >> 32) + 1;
    int64_t cell_to = (int64_t)(key >> 32);
    if (cell_to > p.n_cells) cell_to = p.n_cells;
    for (int64_t s = cell_from; s <= cell_to; ++s) p.cell_row_start[s] = heads_before;
    if (i == p.n) return;
    if ((int64_t)(key >> 32) >= p.n_cells) { p.error[1] = SKM_ERR_STATE; p.in_set[i] = 0; return; }
    const bool head = i == 0 || before != key;
    const int64_t row = heads_before - (head ? 0 : 1);
    p.in_set[i] = 0;
    if (row < 0 || row >= p.n_rows) { p.error[1] = SKM_ERR_STATE; return; }
    if (head) p.row_element[row] = (int32_t)(uint32_t)key;
    int64_t from;
    const int64_t g = gene_rows_group(p.order, p.el_group, i, p.n, p.n_groups, from, p.error);
    if (g < 0) return;
    const int len = p.group_len[g];
    if (len == 1) { atomicAdd(p.u + row, 1ULL); return; }
    const int64_t j = p.set_of[g], k = from - p.el_start[g];
    if (len < 2 || len > GENE_SET_MAX || j < 0 || j >= p.n_sets || k < 0 || k >= len) { p.error[1] = SKM_ERR_STATE; return; }
    const int64_t at = p.set_start[j] + k;
    if (at < 0 || at >= p.n_set_elements) { p.error[1] = SKM_ERR_STATE; return; }
    p.set_rows[at] = (int32_t)row;
    p.in_set[i] = 1;
}

// the transposed view: place[] the exclusive scan of in_set[] (in_set[i] = place[i + 1] - place[i])
__global__ void __launch_bounds__(256)
gene_rows_transpose_kernel(GeneRows p, const int64_t *__restrict__ place, int64_t *__restrict__ row_set_start,
                           int32_t *__restrict__ row_sets)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i > p.n) return;
    if (i == p.n) { row_set_start[p.n_rows] = place[p.n]; return; }
    const int64_t row = p.runs[i];
    const int64_t at = place[i];
    if (p.runs[i + 1] != row && row >= 0 && row < p.n_rows) row_set_start[row] = at;    // a head: its row begins here
    if (place[i + 1] == at) return;
    int64_t from;
    const int64_t g = gene_rows_group(p.order, p.el_group, i, p.n, p.n_groups, from, p.error);
    if (g < 0) return;
    const int64_t j = p.set_of[g];
    if (at < 0 || at >= p.n_set_elements || j < 0 || j >= p.n_sets) { p.error[1] = SKM_ERR_STATE; return; }
    row_sets[at] = (int32_t)j;
}

__global__ void __launch_bounds__(256)
gene_cell_sets_kernel(const unsigned long long *__restrict__ tally, int64_t n_cells, int64_t *__restrict__ sets)
{
    const int64_t s = blockIdx.x * 256LL + threadIdx.x;
    if (s < n_cells) sets[s] = (int64_t)tally[s * GENE_EM_TALLY + GENE_EM_DISTRIBUTED];
}

// ---- the EM of a cell
// a row's sum of x / d[j] over its sets row_sets[begin .. end), a set without weight adding 0.0: lane `sub` of the
// row's eight adds entries begin + sub + 8 k in ascending k, then em_row_sum's butterfly
__device__ __forceinline__ double gene_row_sum(const GeneEm &p, int64_t begin, int64_t end, int sub, double xt, int *error)
{
    double s = 0.0;
    for (int64_t e = begin + sub; e < end; e += 8) {
        const int64_t j = p.row_sets[e];
        double dj = 0.0;
        if (j < 0 || j >= p.n_sets) *error = SKM_ERR_STATE;
        else dj = p.d[j];
        s += dj > 0.0 ? xt / dj : 0.0;
    }
    return em_row_butterfly(s);
}

// x: the cell's rows, in LDS or in the cell's slice of p.x.  Every lane of the block runs this to its end.
template <class X>
__device__ __forceinline__ void gene_em_body(X x, const GeneEm &p, int64_t row_first, int64_t rows, int64_t set_first,
                                             int64_t sets, double *s_max, unsigned int *s_flags, int64_t &steps, int &capped)
{
    const int tid = threadIdx.x, sub = tid & 7, wave = tid >> 6;
    steps = 0;
    capped = 0;
    if (sets == 0) {
        for (int64_t r = tid; r < rows; r += 256) x[r] = (double)p.u[row_first + r];
        return;
    }
    // step 0: every set gives each of its rows 1 / its length (d[j] = the length, x = 1)
    for (int64_t j = tid; j < sets; j += 256)
        p.d[set_first + j] = (double)(p.set_start[set_first + j + 1] - p.set_start[set_first + j]);
    __syncthreads();
    for (int64_t r = tid >> 3; r < rows; r += 32) {
        int64_t begin = p.row_set_start[row_first + r], end = p.row_set_start[row_first + r + 1];
        if (begin < 0 || end < begin || end > p.n_set_elements) { p.error[1] = SKM_ERR_STATE; end = begin = 0; }
        const double s = gene_row_sum(p, begin, end, sub, 1.0, p.error + 1);
        if (sub == 0) x[r] = (double)p.u[row_first + r] + s;
    }
    __syncthreads();
    for (;;) {
        // phase A: d[j] = 0.0 + the x of the set's rows, ascending
        for (int64_t j = tid; j < sets; j += 256) {
            int64_t begin = p.set_start[set_first + j], end = p.set_start[set_first + j + 1];
            if (begin < 0 || end < begin || end > p.n_set_elements) { p.error[1] = SKM_ERR_STATE; end = begin = 0; }
            double dj = 0.0;
            for (int64_t k = begin; k < end; ++k) {
                const int64_t r = (int64_t)p.set_rows[k] - row_first;
                if (r < 0 || r >= rows) p.error[1] = SKM_ERR_STATE;
                else dj += x[r];
            }
            p.d[set_first + j] = dj;
        }
        __syncthreads();
        // phase B: x'[r] = u[r] + the row's sum, in place; the largest relative change above the floor
        double local_max = 0.0;
        unsigned int flags = 0;
        for (int64_t r = tid >> 3; r < rows; r += 32) {
            int64_t begin = p.row_set_start[row_first + r], end = p.row_set_start[row_first + r + 1];
            if (begin < 0 || end < begin || end > p.n_set_elements) end = begin = 0;    // (raised in step 0)
            const double xt = x[r];
            const double s = gene_row_sum(p, begin, end, sub, xt, p.error + 1);
            if (sub == 0) {
                const double xn = (double)p.u[row_first + r] + s;
                x[r] = xn;
                em_note_change(xn, xt, GENE_EM_FLOOR, local_max, flags);
            }
        }
        ++steps;
        em_wave_reduce<1>(local_max, flags);
        if ((tid & 63) == 0) { s_max[wave] = local_max; s_flags[wave] = flags; }
        __syncthreads();
        // (every lane folds the same four slots: one verdict for the block; the slots are next written after phase A's barrier)
        double m;
        unsigned int f;
        em_fold_waves(s_max, s_flags, 1, m, f);
        if (!(f & 1u) || (f & 2u) || !(m > GENE_EM_TOL)) break;
        if (steps >= p.max_steps) { capped = 1; break; }
    }
}

__global__ void __launch_bounds__(256)
gene_em_kernel(GeneEm p)
{
    __shared__ double s_x[GENE_EM_LDS_ROWS];
    __shared__ double s_max[4];
    __shared__ unsigned int s_flags[4];
    const int64_t cell = blockIdx.x;
    if (cell >= p.n_cells) return;                // (block-uniform, as every branch down to the body)
    const int64_t row_first = p.cell_row_start[cell], row_end = p.cell_row_start[cell + 1];
    const int64_t set_first = p.cell_set_start[cell], set_end = p.cell_set_start[cell + 1];
    if (row_first < 0 || row_end < row_first || row_end > p.n_rows || set_first < 0 || set_end < set_first || set_end > p.n_sets) {
        if (threadIdx.x == 0) p.error[1] = SKM_ERR_STATE;
        return;
    }
    const int64_t rows = row_end - row_first;
    int64_t steps;
    int capped;
    if (rows <= p.lds_rows && rows <= GENE_EM_LDS_ROWS) {
        gene_em_body(&s_x[0], p, row_first, rows, set_first, set_end - set_first, s_max, s_flags, steps, capped);
        __syncthreads();
        for (int64_t r = threadIdx.x; r < rows; r += 256) p.x[row_first + r] = s_x[r];
    } else {
        gene_em_body(p.x + row_first, p, row_first, rows, set_first, set_end - set_first, s_max, s_flags, steps, capped);
    }
    if (threadIdx.x == 0) { p.steps[cell] = steps; p.capped[cell] = capped; }
}

// ---- fill
__global__ void __launch_bounds__(256)
gene_em_keep_kernel(const double *__restrict__ x, const int32_t *__restrict__ row_element, int64_t n_rows, int n_genes,
                    int64_t *__restrict__ keep)
{
    const int64_t r = blockIdx.x * 256LL + threadIdx.x;
    if (r < n_rows) keep[r] = (uint32_t)row_element[r] < (uint32_t)n_genes && x[r] >= GENE_EM_FLOOR;
}

// place[] the exclusive scan of keep[] with its total nnz
__global__ void __launch_bounds__(256)
gene_em_entries_kernel(const double *__restrict__ x, const int32_t *__restrict__ row_element, const int64_t *__restrict__ place,
                       int64_t n_rows, int64_t nnz, int32_t *__restrict__ indices, double *__restrict__ data)
{
    const int64_t r = blockIdx.x * 256LL + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t at = place[r];
    if (place[r + 1] == at || at < 0 || at >= nnz) return;
    indices[at] = row_element[r];
    data[at] = x[r];
}

__global__ void __launch_bounds__(256)
gene_em_cells_kernel(const double *__restrict__ x, const int32_t *__restrict__ row_element, const int64_t *__restrict__ place,
                     const int64_t *__restrict__ cell_row_start, const int64_t *__restrict__ steps,
                     const int64_t *__restrict__ capped, int64_t n_rows, int n_genes, int64_t n_cells,
                     int64_t *__restrict__ indptr, unsigned long long *__restrict__ tally, double *__restrict__ to_unnamed,
                     unsigned long long *__restrict__ other)
{
    const int64_t s = blockIdx.x * 256LL + threadIdx.x;
    if (s > n_cells) return;
    int64_t first = cell_row_start[s];
    if (first < 0 || first > n_rows) first = n_rows;                  // (raised by gene_em_kernel)
    indptr[s] = place[first];
    if (s == n_cells) return;
    int64_t end = cell_row_start[s + 1];
    if (end < first || end > n_rows) end = first;
    unsigned long long *mine = tally + s * GENE_EM_TALLY;
    mine[GENE_EM_ROWS] = (unsigned long long)(end - first);
    mine[GENE_EM_STEPS] = (unsigned long long)steps[s];
    mine[GENE_EM_CAPPED] = (unsigned long long)capped[s];
    to_unnamed[s] = end > first && row_element[end - 1] == n_genes ? x[end - 1] : 0.0;
    other[2 * s] = mine[GENE_EM_WIDE] + mine[GENE_EM_COLLISION];
    other[2 * s + 1] = mine[GENE_EM_UNNAMED];
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void launch_molecule_sets(const GeneClasses &t, const unsigned long long *keys, const uint32_t *classes, const int64_t *runs,
                          int64_t n, int64_t n_groups, const int32_t *tx_gene, int64_t n_tx, int64_t n_genes, int64_t n_samples,
                          int32_t *stage, int32_t *group_len, int32_t *group_cell, unsigned long long *tally, int *error,
                          hipStream_t stream)
{
    if (n <= 0 || n_groups <= 0) return;
    hipLaunchKernelGGL(molecule_sets_single_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, t, keys, classes, runs, n, n_groups,
                       tx_gene, n_tx, (int)n_genes, n_samples, stage, group_len, group_cell, tally, error);
    hipLaunchKernelGGL(molecule_sets_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, t, keys, classes, runs, n, n_groups,
                       tx_gene, n_tx, (int)n_genes, n_samples, stage, group_len, tally, error);
}

void launch_gene_sets_sizes(const int32_t *group_len, int64_t n_groups, int64_t *elements, int64_t *is_set,
                            int64_t *set_elements, hipStream_t stream)
{
    if (n_groups <= 0) return;
    hipLaunchKernelGGL(gene_sets_sizes_kernel, dim3(blocks_of(n_groups)), dim3(256), 0, stream, group_len, n_groups, elements,
                       is_set, set_elements);
}

void launch_gene_sets_elements(const int32_t *stage, const int32_t *group_len, const int32_t *group_cell, int64_t n_groups,
                               const int64_t *el_start, const int64_t *set_of, const int64_t *set_place, int64_t n_elements,
                               int64_t n_sets, unsigned long long *el_key, int32_t *el_number, int32_t *el_group,
                               int64_t *set_start, int *error, hipStream_t stream)
{
    if (n_groups <= 0) return;
    hipLaunchKernelGGL(gene_sets_elements_kernel, dim3(blocks_of(n_groups * GENE_SET_MAX)), dim3(256), 0, stream, stage,
                       group_len, group_cell, n_groups, el_start, set_of, set_place, n_elements, n_sets, el_key, el_number,
                       el_group, set_start, error);
}

void launch_gene_rows_heads(const unsigned long long *keys, int64_t n, int64_t *heads, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gene_rows_heads_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, keys, n, heads);
}

void launch_gene_rows(const GeneRows &p, hipStream_t stream)
{
    hipLaunchKernelGGL(gene_rows_kernel, dim3(blocks_of(p.n + 1)), dim3(256), 0, stream, p);
}

void launch_gene_rows_transpose(const GeneRows &p, const int64_t *place, int64_t *row_set_start, int32_t *row_sets,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(gene_rows_transpose_kernel, dim3(blocks_of(p.n + 1)), dim3(256), 0, stream, p, place, row_set_start,
                       row_sets);
}

void launch_gene_cell_sets(const unsigned long long *tally, int64_t n_cells, int64_t *sets, hipStream_t stream)
{
    if (n_cells <= 0) return;
    hipLaunchKernelGGL(gene_cell_sets_kernel, dim3(blocks_of(n_cells)), dim3(256), 0, stream, tally, n_cells, sets);
}

void launch_gene_em(const GeneEm &p, hipStream_t stream)
{
    if (p.n_cells <= 0) return;
    hipLaunchKernelGGL(gene_em_kernel, dim3((unsigned)p.n_cells), dim3(256), 0, stream, p);
}

void launch_gene_em_keep(const double *x, const int32_t *row_element, int64_t n_rows, int64_t n_genes, int64_t *keep,
                         hipStream_t stream)
{
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(gene_em_keep_kernel, dim3(blocks_of(n_rows)), dim3(256), 0, stream, x, row_element, n_rows, (int)n_genes,
                       keep);
}

void launch_gene_em_fill(const double *x, const int32_t *row_element, const int64_t *place, const int64_t *cell_row_start,
                         const int64_t *steps, const int64_t *capped, int64_t n_rows, int64_t nnz, int64_t n_genes,
                         int64_t n_cells, int64_t *indptr, int32_t *indices, double *data, unsigned long long *tally,
                         double *to_unnamed, unsigned long long *other, hipStream_t stream)
{
    if (n_rows > 0)
        hipLaunchKernelGGL(gene_em_entries_kernel, dim3(blocks_of(n_rows)), dim3(256), 0, stream, x, row_element, place, n_rows,
                           nnz, indices, data);
    hipLaunchKernelGGL(gene_em_cells_kernel, dim3(blocks_of(n_cells + 1)), dim3(256), 0, stream, x, row_element, place,
                       cell_row_start, steps, capped, n_rows, (int)n_genes, n_cells, indptr, tally, to_unnamed, other);
}

}  // namespace skm
