// Resolved molecules ("Resolved molecules"): the distinct classes among a sample's live molecules
// with one UMI form a group, and the intersection I of their gene sets G_k = { tx_gene[t] : t in T_k } (-1 an element
// like any other) is the group's verdict -- {g}, g >= 0: resolved, entry (sample, g) += 1, and rescued when no class of
// the group lies inside one gene on its own; {-1}: unnamed; two or more elements: multi-gene; empty: collision.  A
// post-pass over what a pooled run leaves in HBM, beside the molecule matrix of skm_molecules.hip:
//   1. class of a slot: one word per slot of the class table, sample << 32 | c where class c of the view lies in the
//      slot (class_list[c]), the sentinel n_samples << 32 of launch_molecule_label_init elsewhere.
//   2. live + scan (skm_molecules.hip, as they are) + keys: the keys kernel streams the molecule set's slots, finds
//      every live molecule's class with class_probe_find (MOL_WIDTH home slots in flight per lane) and writes the key
//      sample << 32 | UMI, the class index and the molecule's number.  A key not found is SKM_ERR_STATE.
//   3. ONE stable sort_pairs_u64 by that key (the caller's); heads (key differs from the place before) with the
//      class indices gathered into sorted order; the scan of the heads numbers the groups and gives their number.
//   4. resolve: a lane per sorted place, the lane at a group's head owns the group.  A group of one class (the bulk on
//      real data) is classified by gene_classify (skm_gene_rule.h): the first GENE_HEAD ids by the lane, long tuples
//      by the whole wave.  A group of several members is taken by the whole wave, one group after the other: its
//      members are consecutive sorted places read from global memory (a group that crosses a wave or a block needs
//      nothing of another wave); the member with the fewest ids is the pivot; the genes of the pivot's ids are the
//      candidates, 64 to a chunk, one per lane, each alive; every other member's ids are streamed 64 at a time, each
//      lane loads one gene, and 64 shuffle steps mark the candidates it hits -- a candidate no id of a member hits
//      dies, and a chunk ends when none is alive.  The verdict is the distinct values among the survivors (duplicate
//      genes in the pivot change nothing).  WORK of a group: len(pivot) x sum of len(member) / 64 wave steps at
//      most, plus sum of len(member) / 64 loads for a resolved group's rescue check.  Per group (label, UMI, number)
//      is written, label = sample << 32 | gene when resolved and n_samples << 32 otherwise; tally[sample][5] is
//      added to through the wave, one atomic per distinct word (as gene_add_other).
//   5. matrix: within a sample the groups' UMIs are distinct, so "distinct UMIs per label" is "groups per label":
//      the group triples go through the molecule matrix's own sort, heads, scan and fill (the caller's).
// Integers only, exact in any order.  No LDS, no scratch, no recursion; every loop is bounded by n, a tuple's length
// or 64; no lane leaves a whole-wave part before its shuffles and ballots; every store is a plain vector store or an
// atomic.  Every id is checked against n_tx before it indexes tx_gene (error[0] = SKM_ERR_ARG), every place against
// n, every class index against n_classes and every group number against n_groups (error[1] = SKM_ERR_STATE).
#include "../../include/seekmer_hip.h"
#include "skm_gene_rule.h"
#include "skm_kernels.h"

#include <algorithm>
#include <climits>

namespace skm {

namespace {

constexpr int RESOLVE_WIDTH = 4;              // molecules in flight per lane of the keys kernel (MOL_WIDTH's reasons)
constexpr int NO_GENE = INT_MIN;              // a lane without an id (genes are >= -1)

__global__ void __launch_bounds__(256)
resolve_class_slots_kernel(const int32_t *__restrict__ sample, int64_t n_classes, const int64_t *__restrict__ class_list,
                           uint64_t n_slots, int64_t n_samples, unsigned long long *words, int *error)
{
    const int64_t c = blockIdx.x * 256LL + threadIdx.x;
    if (c >= n_classes) return;
    const uint64_t slot = (uint64_t)class_list[c];
    const int64_t s = sample ? sample[c] : 0;
    if (slot < n_slots && s >= 0 && s < n_samples) words[slot] = (unsigned long long)s << 32 | (uint32_t)c;
    else *error = SKM_ERR_STATE;
}

// molecule_keys_kernel (skm_molecules.hip) with the slot's word where that kernel takes the slot's label
__global__ void __launch_bounds__(256)
resolve_keys_kernel(UmiSet set, ClassTable classes, const unsigned long long *__restrict__ class_of,
                    const int64_t *__restrict__ place, int64_t n, int64_t n_samples, unsigned long long *__restrict__ mol_key,
                    uint32_t *__restrict__ mol_class, int32_t *__restrict__ mol_number, int *error)
{
    const uint64_t n_slots = set.slot_mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * 256ULL;
    int fault = 0;
    for (uint64_t i0 = blockIdx.x * 256ULL + threadIdx.x; i0 < n_slots; i0 += RESOLVE_WIDTH * stride) {
        unsigned long long key[RESOLVE_WIDTH], home[RESOLVE_WIDTH];
        uint32_t umi[RESOLVE_WIDTH];
        int64_t at[RESOLVE_WIDTH];
        bool live[RESOLVE_WIDTH];
#pragma unroll
        for (int k = 0; k < RESOLVE_WIDTH; ++k) {
            const uint64_t i = i0 + k * stride;
            live[k] = false; key[k] = 0; umi[k] = 0; at[k] = 0;
            if (i < n_slots) {
                const UmiSlot *slot = &set.slots[i];
                live[k] = slot->tag != 0 && slot->dropped == 0;
                key[k] = slot->class_key;
                umi[k] = slot->umi;
                at[k] = place[i];
            }
        }
#pragma unroll
        for (int k = 0; k < RESOLVE_WIDTH; ++k)
            home[k] = classes.slots[key[k] & classes.slot_mask].key;      // (not live: any slot, unused)
#pragma unroll
        for (int k = 0; k < RESOLVE_WIDTH; ++k) {
            if (!live[k]) continue;
            if (at[k] < 0 || at[k] >= n) { fault = SKM_ERR_STATE; continue; }
            unsigned long long word = (unsigned long long)n_samples << 32;
            const uint64_t found = key[k] ? class_probe_find(classes, key[k], home[k]) : ~0ULL;
            if (found != ~0ULL) word = class_of[found];
            const bool known = (int64_t)(word >> 32) < n_samples;
            if (!known) fault = SKM_ERR_STATE;
            mol_key[at[k]] = (word & 0xFFFFFFFF00000000ULL) | umi[k];
            mol_class[at[k]] = known ? (uint32_t)word : ~0u;
            mol_number[at[k]] = (int32_t)(uint32_t)at[k];
        }
    }
    if (fault) atomicExch(error, fault);
}

// the same three arrays from molecules given as (class, UMI) on the device (both checked by the caller)
__global__ void __launch_bounds__(256)
resolve_pairs_kernel(const int32_t *__restrict__ class_sample, const int32_t *__restrict__ in_class,
                     const uint32_t *__restrict__ in_umi, int64_t n, unsigned long long *__restrict__ mol_key,
                     uint32_t *__restrict__ mol_class, int32_t *__restrict__ mol_number)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = (uint32_t)in_class[i];
    mol_key[i] = (unsigned long long)(uint32_t)(class_sample ? class_sample[c] : 0) << 32 | in_umi[i];
    mol_class[i] = c;
    mol_number[i] = (int32_t)(uint32_t)i;
}

__global__ void __launch_bounds__(256)
resolve_heads_kernel(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ order,
                     const uint32_t *__restrict__ mol_class, int64_t n, int64_t *__restrict__ heads,
                     uint32_t *__restrict__ class_sorted)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    heads[i] = i == 0 || keys[i - 1] != keys[i];
    const uint32_t from = (uint32_t)order[i];
    class_sorted[i] = from < (uint64_t)n ? mol_class[from] : ~0u;        // (a sort's values are a permutation of 0 .. n - 1)
}

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

// keys[] / classes[] in sorted order, runs[n + 1] the exclusive scan of the heads with its total n_groups.
__global__ void __launch_bounds__(256)
molecule_resolve_kernel(GeneClasses t, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ classes,
                        const int64_t *__restrict__ runs, int64_t n, int64_t n_groups, const int32_t *__restrict__ tx_gene,
                        int64_t n_tx, int64_t n_samples, unsigned long long *__restrict__ out_label,
                        unsigned long long *__restrict__ out_umi, int32_t *__restrict__ out_number,
                        unsigned long long *tally, int *error)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    // (no lane leaves before the wave's shared parts below: a lane that owns no group just has nothing to add)
    int64_t group = -1, sample = 0, c = t.n_classes;
    uint32_t umi = 0;
    bool head = false, single = false;
    if (i < n) {
        const int64_t g = runs[i];
        if (runs[i + 1] != g) {
            const unsigned long long key = keys[i];
            sample = (int64_t)(key >> 32);
            umi = (uint32_t)key;
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
    int outcome = -1, gene = -1;
    bool rescued = false;

    // groups of one class: the gene rule itself
    const GeneClass one = gene_classify(t, c, lane, tx_gene, n_tx, 0, n_samples, error);
    if (head && single) {
        if (one.kind == GENE_KIND_NONE || one.sample != sample) error[1] = SKM_ERR_STATE;
        else if (one.kind == GENE_KIND_UNIQUE) { outcome = MOLECULE_RESOLVED; gene = one.gene; }
        else outcome = one.kind == GENE_KIND_UNNAMED ? MOLECULE_UNNAMED : MOLECULE_MULTI;
    }

    // groups of several members, by the whole wave (everything but `lane` and what it loads is the same in all lanes)
    unsigned long long todo = __ballot(head && !single);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int64_t first = __shfl(i, src), inside = __shfl(group, src) + 1;   // runs[p + 1] of a member p
        // the members first .. first + count - 1 and the pivot: the first member with the fewest ids
        int64_t count = 0, best_at = first;
        int best_len = INT_MAX;
        for (int64_t base = first; base < n; base += 64) {
            const int64_t p = base + lane;
            const bool member = p < n && runs[p + 1] == inside;
            if (member) {
                const int64_t mc = classes[p];
                if (mc >= t.n_classes) error[1] = SKM_ERR_STATE;
                else {
                    const int len = class_length(t, mc);
                    if (len < best_len) { best_len = len; best_at = p; }
                }
            }
            const unsigned long long in = __ballot(member);
            count += __popcll(in);
            if (in != ~0ULL) break;
        }
        int pivot_len = best_len;
        for (int step = 32; step > 0; step >>= 1) {
            const int theirs = __shfl_xor(pivot_len, step);
            if (theirs < pivot_len) pivot_len = theirs;
        }
        const unsigned long long holders = __ballot(best_len == pivot_len);
        // (among the lanes that hold the fewest, the smallest place: the choice does not change the verdict, but it
        // should not depend on how a group lies in the wave)
        int64_t pivot_at = best_len == pivot_len ? best_at : INT64_MAX;
        for (int step = 32; step > 0; step >>= 1) {
            const int64_t theirs = __shfl_xor(pivot_at, step);
            if (theirs < pivot_at) pivot_at = theirs;
        }
        int verdict = -1, value = -1;
        bool alone = false;                       // some class of the group lies inside the gene on its own
        if (holders && pivot_len != INT_MAX && pivot_at >= first && pivot_at < first + count) {
            const int64_t pivot_start = t.start[classes[pivot_at]];
            int distinct = 0;                     // values among the surviving candidates so far: 0, 1 (`value`), 2 = more
            for (int chunk = 0; chunk < pivot_len && distinct < 2; chunk += 64) {
                const int cand = chunk + lane < pivot_len ? gene_at(t, pivot_start + chunk + lane, tx_gene, n_tx, error) : NO_GENE;
                bool alive = cand != NO_GENE;
                for (int64_t p = first; p < first + count && __any(alive); ++p) {
                    const int64_t mc = classes[p];
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
                const unsigned long long left = __ballot(alive);
                if (left) {
                    const int v = __shfl(cand, __ffsll(left) - 1);
                    const bool more = __any(alive && cand != v);
                    if (distinct == 0) { value = v; distinct = more ? 2 : 1; }
                    else if (more || v != value) distinct = 2;
                }
            }
            verdict = distinct == 0 ? MOLECULE_COLLISION : distinct > 1 ? MOLECULE_MULTI : value >= 0 ? MOLECULE_RESOLVED : MOLECULE_UNNAMED;
            if (verdict == MOLECULE_RESOLVED)
                for (int64_t p = first; p < first + count && !alone; ++p) {
                    const int64_t mc = classes[p];
                    if (mc >= t.n_classes) continue;
                    const int64_t m_start = t.start[mc];
                    const int m_len = class_length(t, mc);
                    int differs = 0;
                    for (int base = 0; base < m_len && !differs; base += 64)
                        differs = __any(base + lane < m_len && gene_at(t, m_start + base + lane, tx_gene, n_tx, error) != value);
                    alone = m_len > 0 && !differs;
                }
        }
        if (lane == src) {
            outcome = verdict;
            gene = value;
            rescued = verdict == MOLECULE_RESOLVED && !alone;
        }
    }

    if (head) {
        out_label[group] = outcome == MOLECULE_RESOLVED ? (unsigned long long)sample << 32 | (uint32_t)gene
                                                        : (unsigned long long)n_samples << 32;
        out_umi[group] = umi;
        out_number[group] = (int32_t)(uint32_t)group;
    }
    wave_count(sample * MOLECULE_TALLY + outcome, head && outcome >= 0, lane, tally);
    wave_count(sample * MOLECULE_TALLY + MOLECULE_RESCUED, head && rescued, lane, tally);
}

// other[s] = { multi-gene + collision, unnamed } of tally[s]
__global__ void __launch_bounds__(256)
resolve_other_kernel(const unsigned long long *__restrict__ tally, int64_t n_samples, unsigned long long *__restrict__ other)
{
    const int64_t s = blockIdx.x * 256LL + threadIdx.x;
    if (s >= n_samples) return;
    other[2 * s] = tally[s * MOLECULE_TALLY + MOLECULE_MULTI] + tally[s * MOLECULE_TALLY + MOLECULE_COLLISION];
    other[2 * s + 1] = tally[s * MOLECULE_TALLY + MOLECULE_UNNAMED];
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void launch_resolve_class_slots(const GeneClasses &t, const int64_t *class_list, uint64_t n_slots, int64_t n_samples,
                                unsigned long long *words, int *error, hipStream_t stream)
{
    if (t.n_classes <= 0) return;
    hipLaunchKernelGGL(resolve_class_slots_kernel, dim3(blocks_of(t.n_classes)), dim3(256), 0, stream, t.sample, t.n_classes,
                       class_list, n_slots, n_samples, words, error);
}

void launch_resolve_keys(const UmiSet &set, const ClassTable &classes, const unsigned long long *class_of, const int64_t *place,
                         int64_t n, int64_t n_samples, unsigned long long *mol_key, uint32_t *mol_class, int32_t *mol_number,
                         int *error, hipStream_t stream)
{
    if (n <= 0) return;
    const uint64_t lanes = (set.slot_mask + RESOLVE_WIDTH) / RESOLVE_WIDTH;
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>((lanes + 255) / 256, 1), 2048);
    hipLaunchKernelGGL(resolve_keys_kernel, dim3(grid), dim3(256), 0, stream, set, classes, class_of, place, n, n_samples,
                       mol_key, mol_class, mol_number, error);
}

void launch_resolve_pairs(const int32_t *class_sample, const int32_t *in_class, const uint32_t *in_umi, int64_t n,
                          unsigned long long *mol_key, uint32_t *mol_class, int32_t *mol_number, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(resolve_pairs_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, class_sample, in_class, in_umi, n,
                       mol_key, mol_class, mol_number);
}

void launch_resolve_heads(const unsigned long long *keys, const int32_t *order, const uint32_t *mol_class, int64_t n,
                          int64_t *heads, uint32_t *class_sorted, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(resolve_heads_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, keys, order, mol_class, n, heads,
                       class_sorted);
}

void launch_molecule_resolve(const GeneClasses &t, const unsigned long long *keys, const uint32_t *classes, const int64_t *runs,
                             int64_t n, int64_t n_groups, const int32_t *tx_gene, int64_t n_tx, int64_t n_samples,
                             unsigned long long *out_label, unsigned long long *out_umi, int32_t *out_number,
                             unsigned long long *tally, int *error, hipStream_t stream)
{
    if (n <= 0 || n_groups <= 0) return;
    hipLaunchKernelGGL(molecule_resolve_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, t, keys, classes, runs, n, n_groups,
                       tx_gene, n_tx, n_samples, out_label, out_umi, out_number, tally, error);
}

void launch_resolve_other(const unsigned long long *tally, int64_t n_samples, unsigned long long *other, hipStream_t stream)
{
    if (n_samples <= 0) return;
    hipLaunchKernelGGL(resolve_other_kernel, dim3(blocks_of(n_samples)), dim3(256), 0, stream, tally, n_samples, other);
}

}  // namespace skm
