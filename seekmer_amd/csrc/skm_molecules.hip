// Molecule matrix ("Molecule matrix"): entry (sample, gene) = the number of DISTINCT UMIs among
// the sample's surviving units whose class lies inside that gene -- a post-pass over what a pooled run leaves in HBM
// (the molecule set of skm_umi.hip, the class table, both final), with the gene rule of skm_gene_rule.h.
//   1. labels: one lane per class of the set's view, a wave per 64 classes.  A class inside one named gene with a
//      count > 0 gets the label sample << 32 | gene, stored BY TABLE SLOT (class c of the view lies in slot
//      class_list[c]); every other slot keeps the sentinel n_samples << 32, above all labels.  The `other` words are
//      added here, by the one copy of the rule.
//   2. live + scan + keys: live[i] = slot i of the molecule set is occupied and not marked dropped; the project's
//      scan gives every live molecule its number, so the compacted order does not depend on the grid.  The keys
//      kernel streams the set's slots (32 bytes each), finds the class key of every live one in the class table with
//      a read-only probe (MOL_WIDTH home slots in flight per lane, as umi_claim_kernel keeps UMI_WIDTH), takes that
//      slot's label and writes (label, UMI, number).  A key the table does not hold is SKM_ERR_STATE: a molecule
//      survived, so its class exists.
//   3. order: (sample, gene, UMI) does not fit 64 bits, so two stable sort_pairs_u64 calls (the caller's): by UMI,
//      then by the label gathered into that order (molecule_gather_kernel).
//   4. heads, scan, fill: as skm_gene_matrix.hip, where a run is a stretch of equal labels and what is summed over it
//      is the flag "first of its (label, UMI)" -- the UMIs ascend inside a label, so equal ones are neighbours.
//      The fill kernel is gene_matrix_fill_kernel's text with that one difference; it stands here as a kernel of its
//      own because sharing the body through a template changed the register allocation of the unit matrix's kernel.
// Integers only, exact in any order; every store is a plain vector store or an atomic add.  Every index is bounded
// before use: table slots by the mask or against n_slots, molecule numbers against n.
#include "../../include/seekmer_hip.h"
#include "skm_gene_rule.h"
#include "skm_kernels.h"

#include <algorithm>

namespace skm {

namespace {

__global__ void __launch_bounds__(256)
molecule_label_init_kernel(unsigned long long *__restrict__ labels, uint64_t n_slots, unsigned long long sentinel)
{
    for (uint64_t i = blockIdx.x * 256ULL + threadIdx.x; i < n_slots; i += gridDim.x * 256ULL) labels[i] = sentinel;
}

__global__ void __launch_bounds__(256)
molecule_labels_kernel(GeneClasses t, const int64_t *__restrict__ class_list, uint64_t n_slots, const int32_t *tx_gene,
                       int64_t n_tx, int64_t n_samples, unsigned long long *labels, unsigned long long *other, int *error)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const GeneClass g = gene_classify(t, c, lane, tx_gene, n_tx, 0, n_samples, error);
    if (c < t.n_classes && g.kind == GENE_KIND_UNIQUE && g.count > 0) {
        const uint64_t slot = (uint64_t)class_list[c];
        if (slot < n_slots) labels[slot] = (unsigned long long)g.sample << 32 | (uint32_t)g.gene;
        else error[1] = SKM_ERR_STATE;
    }
    gene_add_other(g, 0, lane, other);
}

__global__ void __launch_bounds__(256)
molecule_live_kernel(const UmiSlot *__restrict__ slots, uint64_t n_slots, int64_t *__restrict__ live)
{
    for (uint64_t i = blockIdx.x * 256ULL + threadIdx.x; i < n_slots; i += gridDim.x * 256ULL)
        live[i] = slots[i].tag != 0 && slots[i].dropped == 0;
}

// Molecules are taken MOL_WIDTH at a time per lane: the set's slots and their places first, then the home slots of
// all their class keys, before any is looked at.  The kernel is one random 32-byte sector (the class slot) plus one
// random 8-byte word (its label) per molecule behind a streamed read; the chain slot -> class slot -> label of one
// molecule runs under the chains of the others.
constexpr int MOL_WIDTH = 4;

__global__ void __launch_bounds__(256)
molecule_keys_kernel(UmiSet set, ClassTable classes, const unsigned long long *__restrict__ labels,
                     const int64_t *__restrict__ place, int64_t n, unsigned long long sentinel,
                     unsigned long long *__restrict__ mol_label, unsigned long long *__restrict__ mol_umi,
                     int32_t *__restrict__ mol_number, int *error)
{
    const uint64_t n_slots = set.slot_mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * 256ULL;
    int fault = 0;
    for (uint64_t i0 = blockIdx.x * 256ULL + threadIdx.x; i0 < n_slots; i0 += MOL_WIDTH * stride) {
        unsigned long long key[MOL_WIDTH], home[MOL_WIDTH];
        uint32_t umi[MOL_WIDTH];
        int64_t at[MOL_WIDTH];
        bool live[MOL_WIDTH];
#pragma unroll
        for (int k = 0; k < MOL_WIDTH; ++k) {
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
        for (int k = 0; k < MOL_WIDTH; ++k)
            home[k] = classes.slots[key[k] & classes.slot_mask].key;      // (not live: any slot, unused)
#pragma unroll
        for (int k = 0; k < MOL_WIDTH; ++k) {
            if (!live[k]) continue;
            if (at[k] < 0 || at[k] >= n) { fault = SKM_ERR_STATE; continue; }
            unsigned long long label = sentinel;
            const uint64_t found = key[k] ? class_probe_find(classes, key[k], home[k]) : ~0ULL;
            if (found == ~0ULL) fault = SKM_ERR_STATE;
            else label = labels[found];
            mol_label[at[k]] = label;
            mol_umi[at[k]] = umi[k];
            mol_number[at[k]] = (int32_t)(uint32_t)at[k];
        }
    }
    if (fault) atomicExch(error, fault);
}

__global__ void __launch_bounds__(256)
molecule_triples_kernel(const int32_t *__restrict__ sample, const int32_t *__restrict__ gene, const uint32_t *__restrict__ umi,
                        int64_t n, unsigned long long *__restrict__ mol_label, unsigned long long *__restrict__ mol_umi,
                        int32_t *__restrict__ mol_number)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    mol_label[i] = (unsigned long long)(uint32_t)sample[i] << 32 | (uint32_t)gene[i];
    mol_umi[i] = umi[i];
    mol_number[i] = (int32_t)(uint32_t)i;
}

__global__ void __launch_bounds__(256)
molecule_gather_kernel(const unsigned long long *__restrict__ mol_label, const int32_t *__restrict__ order, int64_t n,
                       unsigned long long *__restrict__ label_out, int32_t *__restrict__ number_out)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const uint32_t from = (uint32_t)order[i];
    label_out[i] = from < (uint64_t)n ? mol_label[from] : ~0ULL;      // (a sort's values are a permutation of 0 .. n - 1)
    number_out[i] = (int32_t)(uint32_t)i;
}

__global__ void __launch_bounds__(256)
molecule_heads_kernel(const unsigned long long *__restrict__ labels, const int32_t *__restrict__ at,
                      const unsigned long long *__restrict__ umi_of, int64_t n, int64_t n_samples,
                      int64_t *__restrict__ heads, uint32_t *__restrict__ first)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const unsigned long long label = labels[i];
    const bool entry = (int64_t)(label >> 32) < n_samples;
    const bool head = entry && (i == 0 || labels[i - 1] != label);
    bool fresh = head;
    if (entry && !head) {
        const uint32_t mine = (uint32_t)at[i], below = (uint32_t)at[i - 1];
        fresh = mine >= (uint64_t)n || below >= (uint64_t)n || umi_of[mine] != umi_of[below];
    }
    heads[i] = head;
    first[i] = fresh;
}

// gene_matrix_fill_kernel (skm_gene_matrix.hip), with first[i] where that kernel takes a class's count.
// runs[i]: the heads before sorted element i, runs[n] = nnz.  data[nnz] zeroed by the caller.
__global__ void __launch_bounds__(256)
molecule_fill_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ first,
                     const int64_t *__restrict__ runs, int64_t n, int64_t n_samples, int64_t *__restrict__ indptr,
                     int32_t *__restrict__ indices, unsigned long long *data)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    // (no lane leaves before the wave's sum below: a lane without an entry just has run -1 and nothing to add)
    int64_t run = -1;
    unsigned long long sum = 0;
    if (i <= n) {
        const unsigned long long key = i < n ? keys[i] : (unsigned long long)n_samples << 32;
        const unsigned long long before = i > 0 ? keys[i - 1] : 0;
        const int64_t heads_before = runs[i];
        // the samples that begin at element i: those after the one of element i - 1, up to the one of element i
        const int64_t from = i == 0 ? 0 : (int64_t)(before >> 32) + 1;
        int64_t to = (int64_t)(key >> 32);
        if (to > n_samples) to = n_samples;                           // (indptr has n_samples + 1 words)
        for (int64_t s = from; s <= to; ++s) indptr[s] = heads_before;
        if ((int64_t)(key >> 32) < n_samples) {
            const bool head = i == 0 || before != key;
            run = heads_before - (head ? 0 : 1);
            if (head) indices[run] = (int32_t)(uint32_t)key;
            sum = first[i];
        }
    }
    // sum[lane] = the first-of-their-UMI flags of the lanes from this one to the end of its run inside the wave
    for (int step = 1; step < 64; step <<= 1) {
        const unsigned long long up = __shfl_down(sum, step);
        const int64_t up_run = __shfl_down(run, step);
        if (lane + step < 64 && up_run == run) sum += up;
    }
    const int64_t run_below = __shfl_up(run, 1);
    if (run >= 0 && (lane == 0 || run_below != run)) atomicAdd(data + run, sum);
}

unsigned stream_grid(uint64_t n, int per_lane)
{
    const uint64_t lanes = (n + per_lane - 1) / per_lane;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>((lanes + 255) / 256, 1), 2048);
}

}  // namespace

void launch_molecule_label_init(unsigned long long *labels, uint64_t n_slots, int64_t n_samples, hipStream_t stream)
{
    if (n_slots == 0) return;
    hipLaunchKernelGGL(molecule_label_init_kernel, dim3(stream_grid(n_slots, 1)), dim3(256), 0, stream, labels, n_slots,
                       (unsigned long long)n_samples << 32);
}

void launch_molecule_labels(const GeneClasses &t, const int64_t *class_list, uint64_t n_slots, const int32_t *tx_gene,
                            int64_t n_tx, int64_t n_samples, unsigned long long *labels, unsigned long long *other,
                            int *error, hipStream_t stream)
{
    if (t.n_classes <= 0) return;
    hipLaunchKernelGGL(molecule_labels_kernel, dim3((unsigned)((t.n_classes + 255) / 256)), dim3(256), 0, stream, t, class_list,
                       n_slots, tx_gene, n_tx, n_samples, labels, other, error);
}

void launch_molecule_live(const UmiSet &set, int64_t *live, hipStream_t stream)
{
    const uint64_t n_slots = set.slot_mask + 1;
    hipLaunchKernelGGL(molecule_live_kernel, dim3(stream_grid(n_slots, 1)), dim3(256), 0, stream, set.slots, n_slots, live);
}

void launch_molecule_keys(const UmiSet &set, const ClassTable &classes, const unsigned long long *labels,
                          const int64_t *place, int64_t n, int64_t n_samples, unsigned long long *mol_label,
                          unsigned long long *mol_umi, int32_t *mol_number, int *error, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(molecule_keys_kernel, dim3(stream_grid(set.slot_mask + 1, MOL_WIDTH)), dim3(256), 0, stream, set, classes,
                       labels, place, n, (unsigned long long)n_samples << 32, mol_label, mol_umi, mol_number, error);
}

void launch_molecule_triples(const int32_t *sample, const int32_t *gene, const uint32_t *umi, int64_t n,
                             unsigned long long *mol_label, unsigned long long *mol_umi, int32_t *mol_number,
                             hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(molecule_triples_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sample, gene, umi, n,
                       mol_label, mol_umi, mol_number);
}

void launch_molecule_gather(const unsigned long long *mol_label, const int32_t *order, int64_t n,
                            unsigned long long *label_out, int32_t *number_out, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(molecule_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mol_label, order, n,
                       label_out, number_out);
}

void launch_molecule_heads(const unsigned long long *labels, const int32_t *at, const unsigned long long *umi_of,
                           int64_t n, int64_t n_samples, int64_t *heads, uint32_t *first, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(molecule_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, labels, at, umi_of, n,
                       n_samples, heads, first);
}

void launch_molecule_fill(const unsigned long long *labels, const uint32_t *first, const int64_t *runs, int64_t n,
                          int64_t n_samples, int64_t *indptr, int32_t *indices, unsigned long long *data,
                          hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(molecule_fill_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, stream, labels, first, runs, n,
                       n_samples, indptr, indices, data);
}

}  // namespace skm
