// Count matrix ("Count matrix"): the gene-unique counts of a class table as a CSR over samples,
// made where the table lies in HBM.  The rule is that of skm_genes.hip (b), read from skm_gene_rule.h; what differs
// is where a unique class's count goes: not into a dense row of n_genes words per sample but into one entry per
// (sample, gene) that has a count at all.
//   1. keys: one lane per class, a wave per 64 classes.  A class inside one named gene with a count > 0 gets the key
//      sample << 32 | gene, every other class the key n_samples << 32, above all of those.  The `other` words are
//      added here, as in the dense kernel.
//   2. the project's stable radix sort (sort_pairs_u64) of (key, class) up to the bits of n_samples.
//   3. run heads: head[i] = key[i] is a (sample, gene) key and differs from key[i - 1]; their exclusive scan
//      (exclusive_scan_total_i64) numbers the runs, its total is nnz.
//   4. fill: one lane per sorted element.  run = heads before i, less one where i is no head; a head stores its gene
//      in indices[run]; the counts of the lanes of a wave that share a run are summed by shuffles -- a run is a
//      stretch of neighbouring lanes, so log2(64) steps of a segmented sum do --, and the first lane of the stretch
//      adds the sum to data[run] with ONE 64-bit integer atomic: a run that crosses waves or blocks gets one per wave.
//      indptr[s], for every sample between the one before element i and element i's own, is the number of heads
//      before i (group_offsets_kernel's walk, skm_barcodes.hip); element n stands for the end.
// Integers only, exact in any order; every store is a plain vector store or an atomic add.
#include "../../include/seekmer_hip.h"
#include "skm_gene_rule.h"
#include "skm_kernels.h"

namespace skm {

__global__ void __launch_bounds__(256)
gene_matrix_keys_kernel(GeneClasses t, const int32_t *tx_gene, int64_t n_tx, int64_t n_samples,
                        unsigned long long *keys, int32_t *vals, unsigned long long *other, int *error)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const GeneClass g = gene_classify(t, c, lane, tx_gene, n_tx, 0, n_samples, error);
    if (c < t.n_classes) {
        const bool entry = g.kind == GENE_KIND_UNIQUE && g.count > 0;
        keys[c] = entry ? (unsigned long long)g.sample << 32 | (uint32_t)g.gene : (unsigned long long)n_samples << 32;
        vals[c] = (int32_t)(uint32_t)c;
    }
    gene_add_other(g, 0, lane, other);
}

__global__ void __launch_bounds__(256)
gene_matrix_heads_kernel(const unsigned long long *__restrict__ keys, int64_t n, int64_t n_samples, int64_t *__restrict__ heads)
{
    const int64_t i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    heads[i] = (int64_t)(key >> 32) < n_samples && (i == 0 || keys[i - 1] != key);
}

// runs[i]: the heads before sorted element i, runs[n] = nnz (the scan of the kernel above).  data[nnz] zeroed by the caller.
__global__ void __launch_bounds__(256)
gene_matrix_fill_kernel(GeneClasses t, const unsigned long long *__restrict__ keys, const int32_t *__restrict__ vals,
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
        const int64_t to = (int64_t)(key >> 32);                      // (keys' samples are <= n_samples)
        for (int64_t s = from; s <= to; ++s) indptr[s] = heads_before;
        if ((int64_t)(key >> 32) < n_samples) {
            const bool head = i == 0 || before != key;
            run = heads_before - (head ? 0 : 1);
            if (head) indices[run] = (int32_t)(uint32_t)key;
            const uint32_t c = (uint32_t)vals[i];
            sum = t.count_f64 ? (unsigned long long)t.count_f64[c] : (unsigned long long)t.count_i64[c];
        }
    }
    // sum[lane] = the counts of the lanes from this one to the end of its run inside the wave
    for (int step = 1; step < 64; step <<= 1) {
        const unsigned long long up = __shfl_down(sum, step);
        const int64_t up_run = __shfl_down(run, step);
        if (lane + step < 64 && up_run == run) sum += up;
    }
    const int64_t run_below = __shfl_up(run, 1);
    if (run >= 0 && (lane == 0 || run_below != run)) atomicAdd(data + run, sum);
}

void launch_gene_matrix_keys(const GeneClasses &t, const int32_t *tx_gene, int64_t n_tx, int64_t n_samples,
                             unsigned long long *keys, int32_t *vals, unsigned long long *other, int *error, hipStream_t stream)
{
    if (t.n_classes <= 0) return;
    hipLaunchKernelGGL(gene_matrix_keys_kernel, dim3((unsigned)((t.n_classes + 255) / 256)), dim3(256), 0, stream, t, tx_gene,
                       n_tx, n_samples, keys, vals, other, error);
}

void launch_gene_matrix_heads(const unsigned long long *keys, int64_t n, int64_t n_samples, int64_t *heads, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gene_matrix_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, keys, n, n_samples, heads);
}

void launch_gene_matrix_fill(const GeneClasses &t, const unsigned long long *keys, const int32_t *vals, const int64_t *runs,
                             int64_t n, int64_t n_samples, int64_t *indptr, int32_t *indices, unsigned long long *data,
                             hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gene_matrix_fill_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, stream, t, keys, vals, runs, n,
                       n_samples, indptr, indices, data);
}

}  // namespace skm
