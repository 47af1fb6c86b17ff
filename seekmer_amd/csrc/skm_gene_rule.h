// The gene rule (skm_genes.hip, comment (b)) where both of its kernels read it: gene_unique_kernel (dense rows,
// skm_genes.hip) and gene_matrix_keys_kernel (sparse rows, skm_gene_matrix.hip).  One copy: what a class is --
// inside one named gene, unnamed, ambiguous -- is decided here and nowhere else.
//   Both functions are for WHOLE waves: every lane of a wave calls them, a lane without a class with c >= n_classes
// (they ballot and shuffle across the wave).  All state is a handful of registers: no scratch, no recursion.
#pragma once
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"

namespace skm {

constexpr int GENE_HEAD = 8;              // ids of a class that its own lane compares

enum { GENE_KIND_NONE = 0, GENE_KIND_UNIQUE = 1, GENE_KIND_AMBIGUOUS = 2, GENE_KIND_UNNAMED = 3 };

struct GeneClass {
    int64_t sample;                       // of the class (0 without a class)
    int gene;                             // GENE_KIND_UNIQUE: the gene every id lies in
    int kind;                             // GENE_KIND_NONE: no class, or one of a sample outside [sample_first, sample_end)
    unsigned long long count;
};

// Class c of the table.  A lane compares the genes of its class's first GENE_HEAD ids and stops at the first that
// differs; what is still undecided is taken by the whole wave, one class after the other: 64 lanes read 64
// consecutive ids, and the class ends at the first stretch that holds a difference.  Every id is checked against
// n_tx before it indexes tx_gene (*error = SKM_ERR_ARG otherwise, and the class counts as ambiguous).
__device__ inline GeneClass gene_classify(const GeneClasses &t, int64_t c, int lane, const int32_t *tx_gene, int64_t n_tx,
                                          int64_t sample_first, int64_t sample_end, int *error)
{
    int64_t start = 0, sample = 0;
    int len = 0, gene = -1, kind = GENE_KIND_NONE;
    unsigned long long count = 0;
    bool undecided = false;
    // (no lane leaves before the wave's shared part below: a lane without a class just has nothing to add)
    if (c < t.n_classes) {
        sample = t.sample ? t.sample[c] : 0;
        if (sample >= sample_first && sample < sample_end) {
            start = t.start[c];
            len = (int)(t.len ? t.len[c] : t.start[c + 1] - start);
            count = t.count_f64 ? (unsigned long long)t.count_f64[c] : (unsigned long long)t.count_i64[c];
            kind = GENE_KIND_AMBIGUOUS;                       // (what a class without ids stays)
            const int head = len < GENE_HEAD ? len : GENE_HEAD;
            bool same = head > 0;
            for (int j = 0; j < head && same; ++j) {
                const uint32_t id = (uint32_t)t.ids[start + j];
                if (id >= (uint64_t)n_tx) { *error = SKM_ERR_ARG; same = false; break; }
                const int g = tx_gene[id];
                if (j == 0) gene = g;
                same = g == gene;
            }
            if (same) {
                kind = gene >= 0 ? GENE_KIND_UNIQUE : GENE_KIND_UNNAMED;
                undecided = len > GENE_HEAD;
            }
        }
    }
    // the rest of the long classes, by the whole wave
    unsigned long long todo = __ballot(undecided);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int64_t src_start = __shfl(start, src);
        const int src_len = __shfl(len, src), src_gene = __shfl(gene, src);
        int differs = 0;
        for (int base = GENE_HEAD; base < src_len && !differs; base += 64) {
            bool bad = false;
            if (base + lane < src_len) {
                const uint32_t id = (uint32_t)t.ids[src_start + base + lane];
                if (id >= (uint64_t)n_tx) { *error = SKM_ERR_ARG; bad = true; }
                else bad = tx_gene[id] != src_gene;
            }
            differs = __any(bad);
        }
        if (lane == src && differs) kind = GENE_KIND_AMBIGUOUS;
    }
    return GeneClass{sample, gene, kind, count};
}

// other[sample - sample_first][0 / 1] += count for the ambiguous / unnamed classes of a wave.  The words are few and
// hot: lanes of a wave that add to the same word are summed through the wave first, one atomic per distinct word.
__device__ inline void gene_add_other(const GeneClass &g, int64_t sample_first, int lane, unsigned long long *other)
{
    const int64_t word = (g.sample - sample_first) * 2 + (g.kind == GENE_KIND_UNNAMED ? 1 : 0);
    unsigned long long todo = __ballot(g.kind == GENE_KIND_AMBIGUOUS || g.kind == GENE_KIND_UNNAMED);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        const int64_t src_word = __shfl(word, src);
        const unsigned long long mine = __ballot(word == src_word) & todo;
        unsigned long long sum = (mine >> lane) & 1 ? g.count : 0;
        for (int step = 32; step > 0; step >>= 1) sum += __shfl_xor(sum, step);
        if (lane == src) atomicAdd(other + src_word, sum);
        todo &= ~mine;
    }
}

}  // namespace skm
