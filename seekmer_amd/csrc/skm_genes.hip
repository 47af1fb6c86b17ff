// Gene-level tables ("Gene-level tables"): two passes over what a run already holds.
//
// (a) gene sums.  out[r][g] = the sum of values[r][t] over the transcripts t of gene g, added in ascending t,
// one after the other, from +0.0: numpy.add.at's order, so the result is bit for bit numpy's and does not depend
// on the grid.  The host lists every gene's transcripts in ascending t (a stable counting sort); one lane owns one
// (row, gene) and walks the gene's list with a plain sequential add (-ffp-contract=off, no reassociation).
// Neighbouring lanes own neighbouring genes of one row: the gene list is read as one stretch, the row's values
// are gathered from L2 (a row of 190 k doubles is 1.5 MB).  No atomics: a float atomic's sum depends on arrival.
//
// (b) gene-unique counts (the reference's _calculate_uniquely_mapped_counts, seekmer/impute.py:149-183): a class
// whose transcripts ALL lie in one named gene adds its count to unique[sample][gene]; one whose transcripts are
// all unnamed adds to other[sample][1]; every other class (two genes, a gene and an unnamed transcript, no
// transcript at all) to other[sample][0].  Sums are 64-bit integers, exact in any order.
//   One lane per class, a wave per 64 consecutive classes.  A lane compares the genes of its class's first
// GENE_HEAD ids and stops at the first that differs -- most classes that span genes do within a few ids, and most
// classes are no longer than that.  What is still undecided is taken by the whole wave, one class after the
// other: 64 lanes read 64 consecutive ids, and the class ends at the first stretch that holds a difference.
// The `other` words are few and hot: lanes of a wave that add to the same word are summed through the wave
// first, one atomic per distinct word.  unique[sample][gene] is wide and rarely shared: one atomic per class.
// All state is a handful of registers: no scratch, no recursion.  Every id is checked against n_tx before it
// indexes tx_gene (*error otherwise); tx_gene's values and the classes' samples are checked by the host.
// The rule itself -- the head / whole-wave walk and the wave reduction of `other` -- is in skm_gene_rule.h, shared
// with the sparse rows of skm_gene_matrix.hip.
#include "../../include/seekmer_hip.h"
#include "skm_gene_rule.h"
#include "skm_kernels.h"

namespace skm {

__global__ void __launch_bounds__(256)
gene_sums_kernel(const double *values, int64_t n_tx, const int64_t *gene_off, const int32_t *gene_tx,
                 int64_t n_genes, double *out)
{
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= n_genes) return;
    const double *row = values + (int64_t)blockIdx.y * n_tx;
    const int64_t end = gene_off[g + 1];
    double sum = 0.0;
    for (int64_t j = gene_off[g]; j < end; ++j) sum += row[gene_tx[j]];
    out[(int64_t)blockIdx.y * n_genes + g] = sum;
}

void launch_gene_sums(const double *values, int64_t n_rows, int64_t n_tx, const int64_t *gene_off,
                      const int32_t *gene_tx, int64_t n_genes, double *out, hipStream_t stream)
{
    if (n_rows <= 0 || n_genes <= 0) return;
    hipLaunchKernelGGL(gene_sums_kernel, dim3((unsigned)((n_genes + 255) / 256), (unsigned)n_rows), dim3(256), 0, stream,
                       values, n_tx, gene_off, gene_tx, n_genes, out);
}

__global__ void __launch_bounds__(256)
gene_unique_kernel(GeneClasses t, const int32_t *tx_gene, int64_t n_tx, int64_t n_genes, int64_t sample_first,
                   int64_t sample_end, unsigned long long *unique, unsigned long long *other, int *error)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const GeneClass g = gene_classify(t, c, lane, tx_gene, n_tx, sample_first, sample_end, error);
    if (g.kind == GENE_KIND_UNIQUE)
        atomicAdd(unique + (g.sample - sample_first) * n_genes + g.gene, g.count);
    gene_add_other(g, sample_first, lane, other);
}

void launch_gene_unique(const GeneClasses &t, const int32_t *tx_gene, int64_t n_tx, int64_t n_genes, int64_t sample_first,
                        int64_t sample_end, unsigned long long *unique, unsigned long long *other, int *error,
                        hipStream_t stream)
{
    if (t.n_classes <= 0 || sample_end <= sample_first) return;
    hipLaunchKernelGGL(gene_unique_kernel, dim3((unsigned)((t.n_classes + 255) / 256)), dim3(256), 0, stream, t, tx_gene,
                       n_tx, n_genes, sample_first, sample_end, unique, other, error);
}

}  // namespace skm
