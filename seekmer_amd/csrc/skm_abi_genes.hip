// C ABI of libseekmer_hip.so: gene-level tables -- sums of transcript values by gene, and the unique counts of a
// class table given on the host, held by a mapper or held by a sample set -- as dense rows, or as the sparse count
// matrix (skm_gene_matrix: a CSR over samples that stays in HBM until it is read), of units, of molecules or of
// molecules resolved to one gene per UMI.
#include "skm_abi_samples.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

using namespace skm;
using namespace skm::abi;

// ------------------------------------------------------------------ gene-level tables (skm_genes.hip)
namespace {

// SKM_GENE_GROUP (tests): rows of values per group of skm_gene_sums, samples per range of the gene counts
int64_t gene_group(int64_t fitting, int64_t n)
{
    int64_t group = fitting;
    if (const char *v = getenv("SKM_GENE_GROUP"))
        if (atoll(v) > 0) group = std::min<int64_t>(group, atoll(v));
    return std::max<int64_t>(1, std::min(group, n));
}

int gene_map_check(int64_t n_tx, int64_t n_genes, const int32_t *tx_gene)
{
    if (n_tx < 0 || n_genes < 0 || n_tx > INT32_MAX || n_genes > INT32_MAX || (n_tx && !tx_gene))
        return fail(SKM_ERR_ARG, "bad gene map");
    for (int64_t t = 0; t < n_tx; ++t)
        if (tx_gene[t] < -1 || tx_gene[t] >= n_genes)
            return fail(SKM_ERR_ARG, "transcript %lld has gene %d of %lld", (long long)t, tx_gene[t], (long long)n_genes);
    return SKM_OK;
}

// unique[n_samples][n_genes], other[n_samples][2] of a class table in HBM (stream drained on return).  Device rows
// exist for a range of samples at a time: 1 GiB of them at most.
int gene_counts_device(const GeneClasses &t, int64_t n_samples, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                       int64_t *unique, int64_t *other, hipStream_t stream)
{
    std::fill(unique, unique + n_samples * n_genes, (int64_t)0);
    std::fill(other, other + n_samples * 2, (int64_t)0);
    if (t.n_classes == 0 || n_samples == 0) return SKM_OK;
    if (n_tx == 0) return fail(SKM_ERR_ARG, "classes over no transcripts");
    const int64_t range = gene_group((int64_t)(1LL << 27) / std::max<int64_t>(n_genes, 1), n_samples);
    DBuf<int32_t> d_gene; DBuf<unsigned long long> d_rows; DBuf<int> d_error;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    const size_t row_words = (size_t)range * (size_t)(n_genes + 2);             // unique rows | other rows
    SKM_TRY(d_gene.ensure(n_tx)); SKM_TRY(d_rows.ensure(row_words)); SKM_TRY(d_error.ensure(1));
    HIP_TRY(hipMemcpyAsync(d_gene.p, tx_gene, n_tx * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_error.p, 0, sizeof(int), stream));
    for (int64_t first = 0; first < n_samples; first += range) {
        const int64_t here = std::min(range, n_samples - first);
        unsigned long long *d_other = d_rows.p + here * n_genes;
        HIP_TRY(hipMemsetAsync(d_rows.p, 0, (size_t)here * (size_t)(n_genes + 2) * 8, stream));
        launch_gene_unique(t, d_gene.p, n_tx, n_genes, first, first + here, d_rows.p, d_other, d_error.p, stream);
        HIP_TRY(hipGetLastError());
        if (n_genes)
            HIP_TRY(hipMemcpyAsync(unique + first * n_genes, d_rows.p, (size_t)(here * n_genes) * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(other + first * 2, d_other, (size_t)here * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    int error = 0;
    HIP_TRY(hipMemcpyAsync(&error, d_error.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.dismiss();
    if (error) return fail(SKM_ERR_ARG, "a class names a transcript not below n_tx = %lld", (long long)n_tx);
    return SKM_OK;
}

// a class table given on the host as the CSR of skm_mapper_export, with a sample per class or none
int host_classes_check(int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets, const int64_t *class_counts,
                       const int32_t *class_sample, int64_t n_samples, int64_t n_tx)
{
    if (n_classes && (!class_offsets || !class_counts || n_samples < 1)) return fail(SKM_ERR_ARG, "NULL class arrays");
    if (n_classes && !class_sample && n_samples > 1) return fail(SKM_ERR_ARG, "%lld samples without class_sample", (long long)n_samples);
    const int64_t M = n_classes ? class_offsets[n_classes] : 0;
    for (int64_t c = 0; c < n_classes; ++c) {
        if (class_offsets[c] < 0 || class_offsets[c + 1] < class_offsets[c] || class_offsets[c + 1] - class_offsets[c] > INT32_MAX)
            return fail(SKM_ERR_ARG, "class_offsets are not those of a table");
        if (class_counts[c] < 0) return fail(SKM_ERR_ARG, "class %lld has a negative count", (long long)c);
        if (class_sample && (class_sample[c] < 0 || class_sample[c] >= n_samples))
            return fail(SKM_ERR_ARG, "class %lld belongs to sample %d of %lld", (long long)c, class_sample[c], (long long)n_samples);
    }
    if (M && !class_targets) return fail(SKM_ERR_ARG, "NULL class arrays");
    for (int64_t k = 0; k < M; ++k)
        if (class_targets[k] < 0 || class_targets[k] >= n_tx)
            return fail(SKM_ERR_ARG, "a class names transcript %d of %lld", class_targets[k], (long long)n_tx);
    return SKM_OK;
}

struct HostClasses {              // that table in HBM (copies on the null stream)
    DBuf<int64_t> d_off, d_cnt; DBuf<int32_t> d_ids, d_sample;
    GeneClasses t{};
    int upload(int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets, const int64_t *class_counts,
               const int32_t *class_sample)
    {
        t.n_classes = n_classes;
        if (!n_classes) return SKM_OK;
        const int64_t M = class_offsets[n_classes];
        SKM_TRY(d_off.ensure(n_classes + 1)); SKM_TRY(d_cnt.ensure(n_classes)); SKM_TRY(d_ids.ensure((size_t)std::max<int64_t>(M, 1)));
        HIP_TRY(hipMemcpy(d_off.p, class_offsets, (n_classes + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_cnt.p, class_counts, n_classes * 8, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(d_ids.p, class_targets, M * 4, hipMemcpyHostToDevice));
        if (class_sample) {
            SKM_TRY(d_sample.ensure(n_classes));
            HIP_TRY(hipMemcpy(d_sample.p, class_sample, n_classes * 4, hipMemcpyHostToDevice));
            t.sample = d_sample.p;
        }
        t.start = d_off.p; t.count_i64 = d_cnt.p; t.ids = d_ids.p;
        return SKM_OK;
    }
};

}  // namespace

// Rows in groups, so that the rows staged in HBM stay within 256 MB; the gene list goes up once.
extern "C" int skm_gene_sums(int device, int64_t n_rows, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                             const double *values, double *out)
{
    SKM_TRY(check_device(device));
    if (n_rows < 0 || (n_rows && ((n_tx && !values) || (n_genes && !out)))) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    if (n_rows == 0 || n_genes == 0) return SKM_OK;
    // the transcripts by gene, ascending inside a gene: a stable counting sort
    std::vector<int64_t> gene_off(n_genes + 1, 0);
    for (int64_t t = 0; t < n_tx; ++t)
        if (tx_gene[t] >= 0) gene_off[tx_gene[t] + 1]++;
    for (int64_t g = 0; g < n_genes; ++g) gene_off[g + 1] += gene_off[g];
    std::vector<int32_t> gene_tx((size_t)std::max<int64_t>(gene_off[n_genes], 1));
    {
        std::vector<int64_t> next(gene_off.begin(), gene_off.end() - 1);
        for (int64_t t = 0; t < n_tx; ++t)
            if (tx_gene[t] >= 0) gene_tx[next[tx_gene[t]]++] = (int32_t)t;
    }
    SKM_TRY(set_device(device));
    const int64_t group = gene_group(std::min<int64_t>((int64_t)(1LL << 25) / std::max<int64_t>(std::max(n_tx, n_genes), 1), 65535), n_rows);
    DBuf<int64_t> d_off; DBuf<int32_t> d_tx; DBuf<double> d_values, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_off.ensure(n_genes + 1)); SKM_TRY(d_tx.ensure(gene_tx.size()));
    SKM_TRY(d_values.ensure((size_t)std::max<int64_t>(group * n_tx, 1))); SKM_TRY(d_out.ensure((size_t)(group * n_genes)));
    HIP_TRY(hipMemcpy(d_off.p, gene_off.data(), (n_genes + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_tx.p, gene_tx.data(), gene_tx.size() * 4, hipMemcpyHostToDevice));
    for (int64_t first = 0; first < n_rows; first += group) {
        const int64_t here = std::min(group, n_rows - first);
        if (n_tx) HIP_TRY(hipMemcpy(d_values.p, values + first * n_tx, (size_t)(here * n_tx) * 8, hipMemcpyHostToDevice));
        launch_gene_sums(d_values.p, here, n_tx, d_off.p, d_tx.p, n_genes, d_out.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + first * n_genes, d_out.p, (size_t)(here * n_genes) * 8, hipMemcpyDeviceToHost));
    }
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}

extern "C" int skm_gene_unique_counts(int device, int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets,
                                      const int64_t *class_counts, const int32_t *class_sample, int64_t n_samples,
                                      int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, int64_t *unique, int64_t *other)
{
    SKM_TRY(check_device(device));
    if (n_classes < 0 || n_samples < 0 || (n_samples && (!other || (n_genes > 0 && !unique))))
        return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    SKM_TRY(host_classes_check(n_classes, class_offsets, class_targets, class_counts, class_sample, n_samples, n_tx));
    SKM_TRY(set_device(device));
    HostClasses up;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(up.upload(n_classes, class_offsets, class_targets, class_counts, class_sample));
    const GeneClasses &t = up.t;
    SKM_TRY(gene_counts_device(t, n_samples, n_tx, n_genes, tx_gene, unique, other, nullptr));
    drain.dismiss();
    return SKM_OK;
}

extern "C" int skm_mapper_gene_counts(skm_mapper *m, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                      int64_t *unique, int64_t other[2])
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!m || !other || (n_genes > 0 && !unique)) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes;
    DBuf<int64_t> d_off, d_len; DBuf<double> d_cnt; DBuf<unsigned long long> d_fs;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
    GeneClasses t{};
    t.n_classes = C;
    if (C) {
        SKM_TRY(d_off.ensure(C)); SKM_TRY(d_len.ensure(C)); SKM_TRY(d_cnt.ensure(C)); SKM_TRY(d_fs.ensure(C));
        launch_class_compact(m->t, C, d_off.p, d_len.p, d_cnt.p, d_fs.p, m->stream);
        HIP_TRY(hipGetLastError());
        t.start = d_off.p; t.len = d_len.p; t.count_f64 = d_cnt.p; t.ids = m->arena.p;
    }
    SKM_TRY(gene_counts_device(t, 1, n_tx, n_genes, tx_gene, unique, other, m->stream));
    drain.dismiss();
    return SKM_OK;
}

extern "C" int skm_sample_set_gene_counts(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                          int64_t cap_samples, int64_t *unique, int64_t *other)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s || cap_samples < 0 || (cap_samples && (!other || (n_genes > 0 && !unique)))) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.units.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    if (n_samples == 0) return SKM_OK;
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    GeneClasses t{};
    t.n_classes = (int64_t)v.start.size();
    if (t.n_classes) { t.start = v.d_start.p; t.len = v.d_len.p; t.count_f64 = v.d_count.p; t.sample = v.d_sample.p; t.ids = m->arena.p; }
    return gene_counts_device(t, n_samples, n_tx, n_genes, tx_gene, unique, other, m->stream);
}

// ------------------------------------------------------------------ count matrix (skm_gene_matrix.hip)
struct skm_gene_matrix {
    ~skm_gene_matrix() { (void)hipSetDevice(device); }  // (then the members free the device memory)
    int device = 0;
    int64_t n_samples = 0, n_genes = 0, nnz = 0;
    DBuf<int64_t> indptr;                            // [n_samples + 1]
    DBuf<int32_t> indices;                           // [nnz]
    DBuf<unsigned long long> data, other;            // [nnz], [n_samples][2]
    DBuf<unsigned long long> tally;                  // [n_samples][MOLECULE_TALLY]: a resolved matrix alone
    bool has_tally = false;
    DBuf<double> to_unnamed;                         // [n_samples]: a distributed matrix alone, which holds doubles in
    bool has_em = false;                             // data[] and GENE_EM_TALLY words per sample in tally[]
};

namespace {

// what a key and the sort can number: never wrapped silently
int gene_matrix_limits(int64_t n_classes, int64_t n_samples)
{
    if (n_classes >= (1LL << 32))
        return fail(SKM_ERR_ARG, "a count matrix of %lld classes: fewer than 2^32 are possible", (long long)n_classes);
    if (n_samples > (int64_t)INT32_MAX - 1)
        return fail(SKM_ERR_ARG, "a count matrix of %lld samples: 2^31 - 2 at most are possible", (long long)n_samples);
    return SKM_OK;
}

// The CSR of a class table in HBM (stream drained on return): keys, the sort, run heads and their scan, fill.  nnz
// comes home between the scan and the fill: indices and data are made as long as they have to be.
int gene_matrix_device(const GeneClasses &t, int device, int64_t n_samples, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                       hipStream_t stream, skm_gene_matrix **out)
{
    const int64_t n = t.n_classes;
    SKM_TRY(gene_matrix_limits(n, n_samples));
    if (n && n_samples && n_tx == 0) return fail(SKM_ERR_ARG, "classes over no transcripts");
    std::unique_ptr<skm_gene_matrix> m(new skm_gene_matrix);
    m->device = device; m->n_samples = n_samples; m->n_genes = n_genes;
    DBuf<int32_t> d_gene, d_vals, d_order; DBuf<unsigned long long> d_keys, d_sorted; DBuf<int64_t> d_runs; DBuf<int> d_error;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    SKM_TRY(m->indptr.ensure((size_t)n_samples + 1)); SKM_TRY(m->other.ensure((size_t)std::max<int64_t>(2 * n_samples, 1)));
    HIP_TRY(hipMemsetAsync(m->indptr.p, 0, (size_t)(n_samples + 1) * 8, stream));
    HIP_TRY(hipMemsetAsync(m->other.p, 0, (size_t)std::max<int64_t>(2 * n_samples, 1) * 8, stream));
    int error = 0;
    if (n && n_samples) {
        SKM_TRY(d_gene.ensure(n_tx)); SKM_TRY(d_error.ensure(1));
        SKM_TRY(d_keys.ensure(n)); SKM_TRY(d_sorted.ensure(n)); SKM_TRY(d_vals.ensure(n)); SKM_TRY(d_order.ensure(n));
        SKM_TRY(d_runs.ensure((size_t)n + 1));
        HIP_TRY(hipMemcpyAsync(d_gene.p, tx_gene, n_tx * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_error.p, 0, sizeof(int), stream));
        launch_gene_matrix_keys(t, d_gene.p, n_tx, n_samples, d_keys.p, d_vals.p, m->other.p, d_error.p, stream);
        HIP_TRY(hipGetLastError());
        int end_bit = 33;
        while ((1LL << (end_bit - 32)) <= n_samples) ++end_bit;   // (the keys go up to n_samples << 32 itself: the other classes)
        if (sort_pairs_u64(d_keys.p, d_sorted.p, d_vals.p, d_order.p, n, end_bit, stream) != 0)
            return fail(SKM_ERR_HIP, "sorting %lld classes by sample and gene: %s", (long long)n, quant_setup_failure());
        launch_gene_matrix_heads(d_sorted.p, n, n_samples, d_runs.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_runs.p, d_runs.p, n, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the entries of %lld classes: %s", (long long)n, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&m->nnz, d_runs.p + n, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&error, d_error.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (error) return fail(SKM_ERR_ARG, "a class names a transcript not below n_tx = %lld", (long long)n_tx);
        if (m->nnz < 0 || m->nnz > n) return fail(SKM_ERR_HIP, "%lld entries from %lld classes", (long long)m->nnz, (long long)n);
    }
    SKM_TRY(m->indices.ensure((size_t)std::max<int64_t>(m->nnz, 1))); SKM_TRY(m->data.ensure((size_t)std::max<int64_t>(m->nnz, 1)));
    if (n && n_samples) {
        HIP_TRY(hipMemsetAsync(m->data.p, 0, (size_t)std::max<int64_t>(m->nnz, 1) * 8, stream));
        launch_gene_matrix_fill(t, d_sorted.p, d_order.p, d_runs.p, n, n_samples, m->indptr.p, m->indices.p, m->data.p, stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    drain.dismiss();
    *out = m.release();
    return SKM_OK;
}

// ---- molecule matrix (skm_molecules.hip)
// what the sort's 32-bit values can number: never wrapped silently
int molecule_limits(int64_t n_molecules, int64_t n_samples)
{
    if (n_molecules >= (1LL << 32))
        return fail(SKM_ERR_ARG, "a molecule matrix of %lld molecules: fewer than 2^32 are possible", (long long)n_molecules);
    if (n_samples > (int64_t)INT32_MAX - 1)
        return fail(SKM_ERR_ARG, "a molecule matrix of %lld samples: 2^31 - 2 at most are possible", (long long)n_samples);
    return SKM_OK;
}

struct MoleculeKeys {             // n molecules in HBM: label (sample << 32 | gene, or n_samples << 32), UMI, number 0 .. n - 1
    DBuf<unsigned long long> label, umi; DBuf<int32_t> number;
    int ensure(int64_t n) { SKM_TRY(label.ensure(n)); SKM_TRY(umi.ensure(n)); SKM_TRY(number.ensure(n)); return SKM_OK; }
};

// Steps 3 and 4 (stream drained on return): the two stable sorts, heads and their scan, fill.  m->indptr is zeroed,
// m->other is what the caller made of it.  `keys` is used up: its arrays are the sorts' second buffers.
int molecule_matrix_sorted(skm_gene_matrix *m, MoleculeKeys &keys, int64_t n, int umi_bits, hipStream_t stream)
{
    const int64_t n_samples = m->n_samples;
    DBuf<unsigned long long> d_umi_sorted; DBuf<int32_t> d_order, d_at; DBuf<uint32_t> d_first; DBuf<int64_t> d_runs;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    if (n && n_samples) {
        SKM_TRY(d_umi_sorted.ensure(n)); SKM_TRY(d_order.ensure(n)); SKM_TRY(d_at.ensure(n)); SKM_TRY(d_first.ensure(n));
        SKM_TRY(d_runs.ensure((size_t)n + 1));
        // least significant key first: by UMI, then (stable) by the label gathered into that order
        if (sort_pairs_u64(keys.umi.p, d_umi_sorted.p, keys.number.p, d_order.p, n, std::max(umi_bits, 1), stream) != 0)
            return fail(SKM_ERR_HIP, "sorting %lld molecules by UMI: %s", (long long)n, quant_setup_failure());
        unsigned long long *by_umi = keys.umi.p, *sorted = keys.label.p;      // (both free once the gather has run)
        launch_molecule_gather(keys.label.p, d_order.p, n, by_umi, keys.number.p, stream);
        HIP_TRY(hipGetLastError());
        int end_bit = 33;
        while ((1LL << (end_bit - 32)) <= n_samples) ++end_bit;   // (the labels go up to n_samples << 32 itself)
        if (sort_pairs_u64(by_umi, sorted, keys.number.p, d_at.p, n, end_bit, stream) != 0)
            return fail(SKM_ERR_HIP, "sorting %lld molecules by sample and gene: %s", (long long)n, quant_setup_failure());
        launch_molecule_heads(sorted, d_at.p, d_umi_sorted.p, n, n_samples, d_runs.p, d_first.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_runs.p, d_runs.p, n, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the entries of %lld molecules: %s", (long long)n, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&m->nnz, d_runs.p + n, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (m->nnz < 0 || m->nnz > n) return fail(SKM_ERR_HIP, "%lld entries from %lld molecules", (long long)m->nnz, (long long)n);
    }
    SKM_TRY(m->indices.ensure((size_t)std::max<int64_t>(m->nnz, 1))); SKM_TRY(m->data.ensure((size_t)std::max<int64_t>(m->nnz, 1)));
    if (n && n_samples) {
        HIP_TRY(hipMemsetAsync(m->data.p, 0, (size_t)std::max<int64_t>(m->nnz, 1) * 8, stream));
        launch_molecule_fill(keys.label.p, d_first.p, d_runs.p, n, n_samples, m->indptr.p, m->indices.p, m->data.p, stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    drain.dismiss();
    return SKM_OK;
}

// an empty matrix of n_samples rows: indptr and other zero
int molecule_matrix_new(int device, int64_t n_samples, int64_t n_genes, hipStream_t stream, std::unique_ptr<skm_gene_matrix> &m)
{
    m.reset(new skm_gene_matrix);
    m->device = device; m->n_samples = n_samples; m->n_genes = n_genes;
    SKM_TRY(m->indptr.ensure((size_t)n_samples + 1)); SKM_TRY(m->other.ensure((size_t)std::max<int64_t>(2 * n_samples, 1)));
    HIP_TRY(hipMemsetAsync(m->indptr.p, 0, (size_t)(n_samples + 1) * 8, stream));
    HIP_TRY(hipMemsetAsync(m->other.p, 0, (size_t)std::max<int64_t>(2 * n_samples, 1) * 8, stream));
    return SKM_OK;
}

// Steps 1 and 2 on a set's resident state (s->mu and m->mu are held): labels by table slot, the live molecules
// numbered by the scan, their (label, UMI); then the steps above.
int molecule_matrix_set(skm_sample_set *s, const GeneClasses &t, int64_t n_samples, int64_t n_tx, int64_t n_genes,
                        const int32_t *tx_gene, skm_gene_matrix **out)
{
    skm_mapper *mp = s->m;
    hipStream_t stream = mp->stream;
    SKM_TRY(gene_matrix_limits(t.n_classes, n_samples));
    SKM_TRY(molecule_limits(s->umi_entries, n_samples));
    if (t.n_classes && n_samples && n_tx == 0) return fail(SKM_ERR_ARG, "classes over no transcripts");
    const uint64_t class_slots = mp->t.slots ? mp->t.slot_mask + 1 : 0;
    if (t.n_classes && (!class_slots || !mp->t.class_list)) return fail(SKM_ERR_STATE, "classes without a table");
    std::unique_ptr<skm_gene_matrix> m;
    DBuf<int32_t> d_gene; DBuf<unsigned long long> d_labels; DBuf<int64_t> d_place; DBuf<int> d_error; MoleculeKeys keys;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    SKM_TRY(molecule_matrix_new(mp->ix->device, n_samples, n_genes, stream, m));
    int64_t n = 0;
    int error[2] = {0, 0};
    if (t.n_classes && n_samples) {
        SKM_TRY(d_gene.ensure(n_tx)); SKM_TRY(d_error.ensure(2)); SKM_TRY(d_labels.ensure((size_t)class_slots));
        HIP_TRY(hipMemcpyAsync(d_gene.p, tx_gene, n_tx * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_error.p, 0, 2 * sizeof(int), stream));
        launch_molecule_label_init(d_labels.p, class_slots, n_samples, stream);
        launch_molecule_labels(t, mp->t.class_list, class_slots, d_gene.p, n_tx, n_samples, d_labels.p, m->other.p, d_error.p, stream);
        HIP_TRY(hipGetLastError());
        if (s->umi_n_slots) {
            const UmiSet set{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, mp->error.p};
            SKM_TRY(d_place.ensure((size_t)s->umi_n_slots + 1));
            launch_molecule_live(set, d_place.p, stream);
            HIP_TRY(hipGetLastError());
            if (exclusive_scan_total_i64(d_place.p, d_place.p, (int64_t)s->umi_n_slots, stream) != 0)
                return fail(SKM_ERR_HIP, "numbering the molecules of %llu slots: %s", (unsigned long long)s->umi_n_slots, quant_setup_failure());
            HIP_TRY(hipMemcpyAsync(&n, d_place.p + s->umi_n_slots, 8, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (n < 0 || n > s->umi_entries)
                return fail(SKM_ERR_STATE, "%lld live molecules in a set of %lld", (long long)n, (long long)s->umi_entries);
            if (n) {
                SKM_TRY(keys.ensure(n));
                launch_molecule_keys(set, mp->t, d_labels.p, d_place.p, n, n_samples, keys.label.p, keys.umi.p, keys.number.p,
                                     d_error.p + 1, stream);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipMemcpyAsync(error, d_error.p, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (error[0]) return fail(SKM_ERR_ARG, "a class names a transcript not below n_tx = %lld", (long long)n_tx);
        if (error[1]) return fail(SKM_ERR_STATE, "a surviving molecule's class is not in the class table");
    }
    SKM_TRY(molecule_matrix_sorted(m.get(), keys, n, 2 * s->umi_bases, stream));
    drain.dismiss();
    *out = m.release();
    return SKM_OK;
}

// ---- resolved molecules (skm_molecule_resolve.hip)
struct ResolveKeys {              // n molecules in HBM: key (sample << 32 | UMI), class index, number 0 .. n - 1
    DBuf<unsigned long long> key; DBuf<uint32_t> cls; DBuf<int32_t> number;
    int ensure(int64_t n) { SKM_TRY(key.ensure(n)); SKM_TRY(cls.ensure(n)); SKM_TRY(number.ensure(n)); return SKM_OK; }
};

// Steps 3 to 5 (stream drained on return): the one sort, heads and their scan, resolve, then the molecule matrix's own
// steps over the groups.  m is what molecule_matrix_new left; d_error[2] is zeroed or holds what the caller's kernels
// raised (they run ahead on the stream).  n_groups and the errors come home in one synchronisation.
int resolved_matrix_sorted(skm_gene_matrix *m, const GeneClasses &t, ResolveKeys &keys, int64_t n, int umi_bits,
                           const int32_t *d_gene, int64_t n_tx, int *d_error, hipStream_t stream)
{
    const int64_t n_samples = m->n_samples;
    DBuf<unsigned long long> d_sorted; DBuf<int32_t> d_order; DBuf<uint32_t> d_class; DBuf<int64_t> d_runs; MoleculeKeys groups;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    SKM_TRY(m->tally.ensure((size_t)std::max<int64_t>(MOLECULE_TALLY * n_samples, 1)));
    HIP_TRY(hipMemsetAsync(m->tally.p, 0, (size_t)std::max<int64_t>(MOLECULE_TALLY * n_samples, 1) * 8, stream));
    m->has_tally = true;
    int64_t n_groups = 0;
    int error[2] = {0, 0};
    if (n && n_samples) {
        SKM_TRY(d_sorted.ensure(n)); SKM_TRY(d_order.ensure(n)); SKM_TRY(d_class.ensure(n)); SKM_TRY(d_runs.ensure((size_t)n + 1));
        int end_bit = 33;
        while ((1LL << (end_bit - 32)) <= n_samples) ++end_bit;   // (a key raised with an error holds n_samples itself)
        if (sort_pairs_u64(keys.key.p, d_sorted.p, keys.number.p, d_order.p, n, end_bit, stream) != 0)
            return fail(SKM_ERR_HIP, "sorting %lld molecules by sample and UMI: %s", (long long)n, quant_setup_failure());
        launch_resolve_heads(d_sorted.p, d_order.p, keys.cls.p, n, d_runs.p, d_class.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_runs.p, d_runs.p, n, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the groups of %lld molecules: %s", (long long)n, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&n_groups, d_runs.p + n, 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipMemcpyAsync(error, d_error, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (error[1]) return fail(SKM_ERR_STATE, "a surviving molecule's class is not in the class table");
    if (n_groups < 0 || n_groups > n) return fail(SKM_ERR_HIP, "%lld groups from %lld molecules", (long long)n_groups, (long long)n);
    if (n_groups) {
        SKM_TRY(groups.ensure(n_groups));
        launch_molecule_resolve(t, d_sorted.p, d_class.p, d_runs.p, n, n_groups, d_gene, n_tx, n_samples, groups.label.p,
                                groups.umi.p, groups.number.p, m->tally.p, d_error, stream);
        HIP_TRY(hipGetLastError());
        launch_resolve_other(m->tally.p, n_samples, m->other.p, stream);
        HIP_TRY(hipGetLastError());
    }
    SKM_TRY(molecule_matrix_sorted(m, groups, n_groups, umi_bits, stream));     // (drains the stream: the resolve kernel has run)
    HIP_TRY(hipMemcpyAsync(error, d_error, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.dismiss();
    if (error[0]) return fail(SKM_ERR_ARG, "a class names a transcript not below n_tx = %lld", (long long)n_tx);
    if (error[1]) return fail(SKM_ERR_STATE, "a group's class is not one of its sample's classes");
    return SKM_OK;
}

// ---- distributed molecules (skm_molecule_em.hip)
constexpr int64_t GENE_EM_MAX_STEPS = 1000;       // of a cell's EM in production

// SKM_TEST_GENE_EM_LDS_ROWS (tests; looked up at every call): cells of more rows take the EM's global path
int64_t gene_em_lds_rows()
{
    int64_t rows = GENE_EM_LDS_ROWS;
    if (const char *v = getenv("SKM_TEST_GENE_EM_LDS_ROWS"))
        if (*v && atoll(v) >= 0) rows = std::min<int64_t>(rows, atoll(v));
    return rows;
}

struct GeneEmBuffers {            // what gene_em_kernel works in and leaves, in HBM
    DBuf<double> x, d; DBuf<int64_t> steps, capped;
    int ensure(int64_t n_rows, int64_t n_sets, int64_t n_cells, hipStream_t stream)
    {
        SKM_TRY(x.ensure((size_t)std::max<int64_t>(n_rows, 1))); SKM_TRY(d.ensure((size_t)std::max<int64_t>(n_sets, 1)));
        SKM_TRY(steps.ensure((size_t)std::max<int64_t>(n_cells, 1))); SKM_TRY(capped.ensure((size_t)std::max<int64_t>(n_cells, 1)));
        HIP_TRY(hipMemsetAsync(x.p, 0, (size_t)std::max<int64_t>(n_rows, 1) * 8, stream));
        HIP_TRY(hipMemsetAsync(steps.p, 0, (size_t)std::max<int64_t>(n_cells, 1) * 8, stream));
        HIP_TRY(hipMemsetAsync(capped.p, 0, (size_t)std::max<int64_t>(n_cells, 1) * 8, stream));
        return SKM_OK;
    }
};

// resolved_matrix_sorted's steps 3 and 4 with every group's element list, then rows, the EM of every cell and the
// fill (stream drained on return).  m is what molecule_matrix_new left; d_error[2] as there.  Device memory beside
// the keys: 40 bytes per molecule, 96 per group (64 of them the stage), 52 per element, 36 per row,
// 16 per set, 32 per sample.
int distributed_matrix_sorted(skm_gene_matrix *m, const GeneClasses &t, ResolveKeys &keys, int64_t n, const int32_t *d_gene,
                              int64_t n_tx, int64_t max_steps, int *d_error, hipStream_t stream)
{
    const int64_t n_samples = m->n_samples, n_genes = m->n_genes;
    DBuf<unsigned long long> d_sorted, d_el_key, d_el_sorted, d_u; DBuf<uint32_t> d_class;
    DBuf<int32_t> d_order, d_stage, d_len, d_cell, d_el_number, d_el_order, d_el_group, d_row_element, d_set_rows, d_row_sets;
    DBuf<int64_t> d_runs, d_el_start, d_set_of, d_set_place, d_set_start, d_row_runs, d_cell_row_start, d_in_set, d_row_set_start,
        d_cell_set_start, d_keep;
    GeneEmBuffers em;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    const size_t tally_words = (size_t)std::max<int64_t>(GENE_EM_TALLY * n_samples, 1);
    SKM_TRY(m->tally.ensure(tally_words)); SKM_TRY(m->to_unnamed.ensure((size_t)std::max<int64_t>(n_samples, 1)));
    HIP_TRY(hipMemsetAsync(m->tally.p, 0, tally_words * 8, stream));
    HIP_TRY(hipMemsetAsync(m->to_unnamed.p, 0, (size_t)std::max<int64_t>(n_samples, 1) * 8, stream));
    m->has_em = true;
    int64_t n_groups = 0;
    int error[2] = {0, 0};
    if (n && n_samples) {
        SKM_TRY(d_sorted.ensure(n)); SKM_TRY(d_order.ensure(n)); SKM_TRY(d_class.ensure(n)); SKM_TRY(d_runs.ensure((size_t)n + 1));
        int end_bit = 33;
        while ((1LL << (end_bit - 32)) <= n_samples) ++end_bit;   // (a key raised with an error holds n_samples itself)
        if (sort_pairs_u64(keys.key.p, d_sorted.p, keys.number.p, d_order.p, n, end_bit, stream) != 0)
            return fail(SKM_ERR_HIP, "sorting %lld molecules by sample and UMI: %s", (long long)n, quant_setup_failure());
        launch_resolve_heads(d_sorted.p, d_order.p, keys.cls.p, n, d_runs.p, d_class.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_runs.p, d_runs.p, n, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the groups of %lld molecules: %s", (long long)n, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&n_groups, d_runs.p + n, 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipMemcpyAsync(error, d_error, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (error[1]) return fail(SKM_ERR_STATE, "a surviving molecule's class is not in the class table");
    if (n_groups < 0 || n_groups > n) return fail(SKM_ERR_HIP, "%lld groups from %lld molecules", (long long)n_groups, (long long)n);
    int64_t n_elements = 0, n_sets = 0, n_set_elements = 0, n_rows = 0;
    if (n_groups) {
        // sets, and the three scans that number elements, sets and the places of the set-major lists
        SKM_TRY(d_stage.ensure((size_t)n_groups * GENE_SET_MAX)); SKM_TRY(d_len.ensure(n_groups)); SKM_TRY(d_cell.ensure(n_groups));
        SKM_TRY(d_el_start.ensure((size_t)n_groups + 1)); SKM_TRY(d_set_of.ensure((size_t)n_groups + 1));
        SKM_TRY(d_set_place.ensure((size_t)n_groups + 1));
        HIP_TRY(hipMemsetAsync(d_len.p, 0, (size_t)n_groups * 4, stream));
        HIP_TRY(hipMemsetAsync(d_cell.p, 0, (size_t)n_groups * 4, stream));
        launch_molecule_sets(t, d_sorted.p, d_class.p, d_runs.p, n, n_groups, d_gene, n_tx, n_genes, n_samples, d_stage.p, d_len.p,
                             d_cell.p, m->tally.p, d_error, stream);
        HIP_TRY(hipGetLastError());
        launch_gene_sets_sizes(d_len.p, n_groups, d_el_start.p, d_set_of.p, d_set_place.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_el_start.p, d_el_start.p, n_groups, stream) != 0 ||
            exclusive_scan_total_i64(d_set_of.p, d_set_of.p, n_groups, stream) != 0 ||
            exclusive_scan_total_i64(d_set_place.p, d_set_place.p, n_groups, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the elements of %lld groups: %s", (long long)n_groups, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&n_elements, d_el_start.p + n_groups, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&n_sets, d_set_of.p + n_groups, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&n_set_elements, d_set_place.p + n_groups, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(error, d_error, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (error[0]) return fail(SKM_ERR_ARG, "a class names a transcript not below n_tx = %lld", (long long)n_tx);
        if (error[1]) return fail(SKM_ERR_STATE, "a group's class is not one of its sample's classes");
        if (n_elements < 0 || n_elements > n_groups * GENE_SET_MAX || n_sets < 0 || n_sets > n_groups || n_set_elements < 0 ||
            n_set_elements > n_elements)
            return fail(SKM_ERR_HIP, "%lld elements in %lld sets from %lld groups", (long long)n_elements, (long long)n_sets, (long long)n_groups);
        if (n_elements > INT32_MAX)
            return fail(SKM_ERR_ARG, "a distributed matrix of %lld elements: 2^31 - 1 at most are possible", (long long)n_elements);
    }
    if (n_elements) {
        // elements, the one sort, rows
        SKM_TRY(d_el_key.ensure(n_elements)); SKM_TRY(d_el_sorted.ensure(n_elements)); SKM_TRY(d_el_number.ensure(n_elements));
        SKM_TRY(d_el_order.ensure(n_elements)); SKM_TRY(d_el_group.ensure(n_elements)); SKM_TRY(d_set_start.ensure((size_t)n_sets + 1));
        SKM_TRY(d_row_runs.ensure((size_t)n_elements + 1)); SKM_TRY(d_in_set.ensure((size_t)n_elements + 1));
        SKM_TRY(d_cell_row_start.ensure((size_t)n_samples + 1)); SKM_TRY(d_cell_set_start.ensure((size_t)n_samples + 1));
        SKM_TRY(d_set_rows.ensure((size_t)std::max<int64_t>(n_set_elements, 1))); SKM_TRY(d_row_sets.ensure((size_t)std::max<int64_t>(n_set_elements, 1)));
        HIP_TRY(hipMemsetAsync(d_set_start.p, 0, (size_t)(n_sets + 1) * 8, stream));
        launch_gene_sets_elements(d_stage.p, d_len.p, d_cell.p, n_groups, d_el_start.p, d_set_of.p, d_set_place.p, n_elements, n_sets,
                                  d_el_key.p, d_el_number.p, d_el_group.p, d_set_start.p, d_error, stream);
        HIP_TRY(hipGetLastError());
        int end_bit = 33;
        while ((1LL << (end_bit - 32)) <= n_samples) ++end_bit;
        if (sort_pairs_u64(d_el_key.p, d_el_sorted.p, d_el_number.p, d_el_order.p, n_elements, end_bit, stream) != 0)
            return fail(SKM_ERR_HIP, "sorting %lld elements by sample and gene: %s", (long long)n_elements, quant_setup_failure());
        launch_gene_rows_heads(d_el_sorted.p, n_elements, d_row_runs.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_row_runs.p, d_row_runs.p, n_elements, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the rows of %lld elements: %s", (long long)n_elements, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&n_rows, d_row_runs.p + n_elements, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (n_rows < 1 || n_rows > n_elements) return fail(SKM_ERR_HIP, "%lld rows from %lld elements", (long long)n_rows, (long long)n_elements);
        SKM_TRY(d_row_element.ensure(n_rows)); SKM_TRY(d_u.ensure(n_rows)); SKM_TRY(d_row_set_start.ensure((size_t)n_rows + 1));
        SKM_TRY(d_keep.ensure((size_t)n_rows + 1)); SKM_TRY(em.ensure(n_rows, n_sets, n_samples, stream));
        HIP_TRY(hipMemsetAsync(d_u.p, 0, (size_t)n_rows * 8, stream));
        HIP_TRY(hipMemsetAsync(d_row_element.p, 0, (size_t)n_rows * 4, stream));
        HIP_TRY(hipMemsetAsync(d_set_rows.p, 0, (size_t)std::max<int64_t>(n_set_elements, 1) * 4, stream));
        HIP_TRY(hipMemsetAsync(d_row_sets.p, 0, (size_t)std::max<int64_t>(n_set_elements, 1) * 4, stream));
        HIP_TRY(hipMemsetAsync(d_row_set_start.p, 0, (size_t)(n_rows + 1) * 8, stream));
        GeneRows rows{};
        rows.keys = d_el_sorted.p; rows.order = d_el_order.p; rows.runs = d_row_runs.p; rows.el_group = d_el_group.p;
        rows.group_len = d_len.p; rows.el_start = d_el_start.p; rows.set_of = d_set_of.p; rows.set_start = d_set_start.p;
        rows.n = n_elements; rows.n_groups = n_groups; rows.n_sets = n_sets; rows.n_rows = n_rows; rows.n_cells = n_samples;
        rows.n_set_elements = n_set_elements; rows.cell_row_start = d_cell_row_start.p; rows.row_element = d_row_element.p;
        rows.u = d_u.p; rows.in_set = d_in_set.p; rows.set_rows = d_set_rows.p; rows.error = d_error;
        launch_gene_rows(rows, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_in_set.p, d_in_set.p, n_elements, stream) != 0)
            return fail(SKM_ERR_HIP, "placing the sets of %lld rows: %s", (long long)n_rows, quant_setup_failure());
        launch_gene_rows_transpose(rows, d_in_set.p, d_row_set_start.p, d_row_sets.p, stream);
        HIP_TRY(hipGetLastError());
        launch_gene_cell_sets(m->tally.p, n_samples, d_cell_set_start.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_cell_set_start.p, d_cell_set_start.p, n_samples, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the sets of %lld samples: %s", (long long)n_samples, quant_setup_failure());
        // the EM of every cell, then the entries
        GeneEm p{};
        p.n_cells = n_samples; p.n_rows = n_rows; p.n_sets = n_sets; p.n_set_elements = n_set_elements;
        p.cell_row_start = d_cell_row_start.p; p.cell_set_start = d_cell_set_start.p; p.u = d_u.p; p.set_start = d_set_start.p;
        p.set_rows = d_set_rows.p; p.row_set_start = d_row_set_start.p; p.row_sets = d_row_sets.p; p.d = em.d.p; p.x = em.x.p;
        p.steps = em.steps.p; p.capped = em.capped.p; p.max_steps = max_steps; p.lds_rows = gene_em_lds_rows(); p.error = d_error;
        launch_gene_em(p, stream);
        HIP_TRY(hipGetLastError());
        launch_gene_em_keep(em.x.p, d_row_element.p, n_rows, n_genes, d_keep.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_keep.p, d_keep.p, n_rows, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the entries of %lld rows: %s", (long long)n_rows, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&m->nnz, d_keep.p + n_rows, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(error, d_error, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (error[1]) { m->nnz = 0; return fail(SKM_ERR_STATE, "a row or a set of the EM lies outside its sample"); }
        if (m->nnz < 0 || m->nnz > n_rows) { m->nnz = 0; return fail(SKM_ERR_HIP, "entries from %lld rows", (long long)n_rows); }
    }
    SKM_TRY(m->indices.ensure((size_t)std::max<int64_t>(m->nnz, 1))); SKM_TRY(m->data.ensure((size_t)std::max<int64_t>(m->nnz, 1)));
    if (n_samples) {
        if (!n_elements) {                    // no row anywhere: what the fill reads, all zero
            SKM_TRY(d_cell_row_start.ensure((size_t)n_samples + 1)); SKM_TRY(d_keep.ensure(1)); SKM_TRY(d_row_element.ensure(1));
            SKM_TRY(em.ensure(0, 0, n_samples, stream));
            HIP_TRY(hipMemsetAsync(d_cell_row_start.p, 0, (size_t)(n_samples + 1) * 8, stream));
            HIP_TRY(hipMemsetAsync(d_keep.p, 0, 8, stream));
        }
        launch_gene_em_fill(em.x.p, d_row_element.p, d_keep.p, d_cell_row_start.p, em.steps.p, em.capped.p, n_rows, m->nnz, n_genes,
                            n_samples, m->indptr.p, m->indices.p, reinterpret_cast<double *>(m->data.p), m->tally.p,
                            m->to_unnamed.p, m->other.p, stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    drain.dismiss();
    return SKM_OK;
}

// Steps 1 and 2 on a set's resident state (s->mu and m->mu are held): the class of every table slot, the live
// molecules numbered by the scan, their (key, class); then the steps above -- the resolved matrix's, or with em_steps > 0
// the distributed matrix's.
int resolved_matrix_set(skm_sample_set *s, const GeneClasses &t, int64_t n_samples, int64_t n_tx, int64_t n_genes,
                        const int32_t *tx_gene, int64_t em_steps, skm_gene_matrix **out)
{
    skm_mapper *mp = s->m;
    hipStream_t stream = mp->stream;
    SKM_TRY(gene_matrix_limits(t.n_classes, n_samples));
    SKM_TRY(molecule_limits(s->umi_entries, n_samples));
    if (t.n_classes && n_samples && n_tx == 0) return fail(SKM_ERR_ARG, "classes over no transcripts");
    const uint64_t class_slots = mp->t.slots ? mp->t.slot_mask + 1 : 0;
    if (t.n_classes && (!class_slots || !mp->t.class_list)) return fail(SKM_ERR_STATE, "classes without a table");
    std::unique_ptr<skm_gene_matrix> m;
    DBuf<int32_t> d_gene; DBuf<unsigned long long> d_class_of; DBuf<int64_t> d_place; DBuf<int> d_error; ResolveKeys keys;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (an early return: before they go)
    SKM_TRY(molecule_matrix_new(mp->ix->device, n_samples, n_genes, stream, m));
    SKM_TRY(d_error.ensure(2)); SKM_TRY(d_gene.ensure((size_t)std::max<int64_t>(n_tx, 1)));
    HIP_TRY(hipMemsetAsync(d_error.p, 0, 2 * sizeof(int), stream));
    int64_t n = 0;
    if (t.n_classes && n_samples && s->umi_n_slots) {
        SKM_TRY(d_class_of.ensure((size_t)class_slots));
        HIP_TRY(hipMemcpyAsync(d_gene.p, tx_gene, n_tx * 4, hipMemcpyHostToDevice, stream));
        launch_molecule_label_init(d_class_of.p, class_slots, n_samples, stream);
        launch_resolve_class_slots(t, mp->t.class_list, class_slots, n_samples, d_class_of.p, d_error.p + 1, stream);
        HIP_TRY(hipGetLastError());
        const UmiSet set{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, mp->error.p};
        SKM_TRY(d_place.ensure((size_t)s->umi_n_slots + 1));
        launch_molecule_live(set, d_place.p, stream);
        HIP_TRY(hipGetLastError());
        if (exclusive_scan_total_i64(d_place.p, d_place.p, (int64_t)s->umi_n_slots, stream) != 0)
            return fail(SKM_ERR_HIP, "numbering the molecules of %llu slots: %s", (unsigned long long)s->umi_n_slots, quant_setup_failure());
        HIP_TRY(hipMemcpyAsync(&n, d_place.p + s->umi_n_slots, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (n < 0 || n > s->umi_entries)
            return fail(SKM_ERR_STATE, "%lld live molecules in a set of %lld", (long long)n, (long long)s->umi_entries);
        if (n) {
            SKM_TRY(keys.ensure(n));
            launch_resolve_keys(set, mp->t, d_class_of.p, d_place.p, n, n_samples, keys.key.p, keys.cls.p, keys.number.p,
                                d_error.p + 1, stream);
            HIP_TRY(hipGetLastError());
        }
    }
    if (em_steps > 0) SKM_TRY(distributed_matrix_sorted(m.get(), t, keys, n, d_gene.p, n_tx, em_steps, d_error.p, stream));
    else SKM_TRY(resolved_matrix_sorted(m.get(), t, keys, n, 2 * s->umi_bases, d_gene.p, n_tx, d_error.p, stream));
    drain.dismiss();
    *out = m.release();
    return SKM_OK;
}

}  // namespace

extern "C" int skm_sample_set_gene_matrix(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                          skm_gene_matrix **out)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s || !out) return fail(SKM_ERR_ARG, "bad argument");
    *out = nullptr;
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.units.size();
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    GeneClasses t{};
    t.n_classes = (int64_t)v.start.size();
    if (t.n_classes) { t.start = v.d_start.p; t.len = v.d_len.p; t.count_f64 = v.d_count.p; t.sample = v.d_sample.p; t.ids = m->arena.p; }
    return gene_matrix_device(t, m->ix->device, n_samples, n_tx, n_genes, tx_gene, m->stream, out);
}

extern "C" int skm_gene_matrix_from_classes(int device, int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets,
                                            const int64_t *class_counts, const int32_t *class_sample, int64_t n_samples,
                                            int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, skm_gene_matrix **out)
{
    SKM_TRY(check_device(device));
    if (n_classes < 0 || n_samples < 0 || !out) return fail(SKM_ERR_ARG, "bad argument");
    *out = nullptr;
    SKM_TRY(gene_matrix_limits(n_classes, n_samples));
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    SKM_TRY(host_classes_check(n_classes, class_offsets, class_targets, class_counts, class_sample, n_samples, n_tx));
    SKM_TRY(set_device(device));
    HostClasses up;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(up.upload(n_classes, class_offsets, class_targets, class_counts, class_sample));
    SKM_TRY(gene_matrix_device(up.t, device, n_samples, n_tx, n_genes, tx_gene, nullptr, out));
    drain.dismiss();
    return SKM_OK;
}

extern "C" int skm_sample_set_molecule_matrix(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                              skm_gene_matrix **out)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s || !out) return fail(SKM_ERR_ARG, "bad argument");
    *out = nullptr;
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    if (!s->umi_bases) return fail(SKM_ERR_STATE, "the set keeps no UMIs: a molecule matrix needs skm_sample_set_keep_umis");
    skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.units.size();
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    GeneClasses t{};
    t.n_classes = (int64_t)v.start.size();
    if (t.n_classes) { t.start = v.d_start.p; t.len = v.d_len.p; t.count_f64 = v.d_count.p; t.sample = v.d_sample.p; t.ids = m->arena.p; }
    return molecule_matrix_set(s, t, n_samples, n_tx, n_genes, tx_gene, out);
}

extern "C" int skm_gene_matrix_from_molecules(int device, int64_t n, const int32_t *sample, const int32_t *gene, const uint32_t *umi,
                                              int64_t n_samples, int64_t n_genes, skm_gene_matrix **out)
{
    SKM_TRY(check_device(device));
    if (n < 0 || n_samples < 0 || n_genes < 0 || n_genes > INT32_MAX || !out || (n && (!sample || !gene || !umi)))
        return fail(SKM_ERR_ARG, "bad argument");
    *out = nullptr;
    SKM_TRY(molecule_limits(n, n_samples));
    for (int64_t i = 0; i < n; ++i) {
        if (sample[i] < 0 || sample[i] >= n_samples)
            return fail(SKM_ERR_ARG, "molecule %lld belongs to sample %d of %lld", (long long)i, sample[i], (long long)n_samples);
        if (gene[i] < 0 || gene[i] >= n_genes)
            return fail(SKM_ERR_ARG, "molecule %lld lies in gene %d of %lld", (long long)i, gene[i], (long long)n_genes);
    }
    SKM_TRY(set_device(device));
    std::unique_ptr<skm_gene_matrix> m;
    DBuf<int32_t> d_sample, d_gene; DBuf<uint32_t> d_umi; MoleculeKeys keys;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(molecule_matrix_new(device, n_samples, n_genes, nullptr, m));
    if (n) {
        SKM_TRY(d_sample.ensure(n)); SKM_TRY(d_gene.ensure(n)); SKM_TRY(d_umi.ensure(n)); SKM_TRY(keys.ensure(n));
        HIP_TRY(hipMemcpy(d_sample.p, sample, n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_gene.p, gene, n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_umi.p, umi, n * 4, hipMemcpyHostToDevice));
        launch_molecule_triples(d_sample.p, d_gene.p, d_umi.p, n, keys.label.p, keys.umi.p, keys.number.p, nullptr);
        HIP_TRY(hipGetLastError());
    }
    SKM_TRY(molecule_matrix_sorted(m.get(), keys, n, 32, nullptr));
    drain.dismiss();
    *out = m.release();
    return SKM_OK;
}

namespace {

int sample_set_resolved_matrix(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, int64_t em_steps,
                               skm_gene_matrix **out)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s || !out) return fail(SKM_ERR_ARG, "bad argument");
    *out = nullptr;
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    if (!s->umi_bases)
        return fail(SKM_ERR_STATE, "the set keeps no UMIs: a %s matrix needs skm_sample_set_keep_umis", em_steps > 0 ? "distributed" : "resolved");
    skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.units.size();
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    GeneClasses t{};
    t.n_classes = (int64_t)v.start.size();
    if (t.n_classes) { t.start = v.d_start.p; t.len = v.d_len.p; t.count_f64 = v.d_count.p; t.sample = v.d_sample.p; t.ids = m->arena.p; }
    return resolved_matrix_set(s, t, n_samples, n_tx, n_genes, tx_gene, em_steps, out);
}

}  // namespace

extern "C" int skm_sample_set_resolved_matrix(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                              skm_gene_matrix **out)
{
    return sample_set_resolved_matrix(s, n_tx, n_genes, tx_gene, 0, out);
}

extern "C" int skm_sample_set_distributed_matrix(skm_sample_set *s, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene,
                                                 skm_gene_matrix **out)
{
    return sample_set_resolved_matrix(s, n_tx, n_genes, tx_gene, GENE_EM_MAX_STEPS, out);
}

namespace {

// em_steps > 0: the distributed matrix's steps with that many EM steps at most; 0: the resolved matrix's
int matrix_from_molecule_classes(int device, int64_t n_classes, const int64_t *class_offsets, const int32_t *class_targets,
                                 const int32_t *class_sample, int64_t n, const int32_t *mol_class, const uint32_t *mol_umi,
                                 int64_t n_samples, int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, int64_t em_steps,
                                 skm_gene_matrix **out)
{
    SKM_TRY(check_device(device));
    if (n_classes < 0 || n < 0 || n_samples < 0 || !out || (n && (!mol_class || !mol_umi))) return fail(SKM_ERR_ARG, "bad argument");
    *out = nullptr;
    SKM_TRY(gene_matrix_limits(n_classes, n_samples));
    SKM_TRY(molecule_limits(n, n_samples));
    SKM_TRY(gene_map_check(n_tx, n_genes, tx_gene));
    const std::vector<int64_t> ones((size_t)n_classes, 1);          // (a class's count plays no part: the molecules are given)
    SKM_TRY(host_classes_check(n_classes, class_offsets, class_targets, ones.data(), class_sample, n_samples, n_tx));
    for (int64_t c = 0; c < n_classes; ++c)
        if (class_offsets[c + 1] == class_offsets[c]) return fail(SKM_ERR_ARG, "class %lld is empty", (long long)c);
    for (int64_t i = 0; i < n; ++i)
        if (mol_class[i] < 0 || mol_class[i] >= n_classes)
            return fail(SKM_ERR_ARG, "molecule %lld has class %d of %lld", (long long)i, mol_class[i], (long long)n_classes);
    SKM_TRY(set_device(device));
    HostClasses up;
    std::unique_ptr<skm_gene_matrix> m;
    DBuf<int32_t> d_gene, d_mol_class; DBuf<uint32_t> d_mol_umi; DBuf<int> d_error; ResolveKeys keys;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(up.upload(n_classes, class_offsets, class_targets, ones.data(), class_sample));
    SKM_TRY(molecule_matrix_new(device, n_samples, n_genes, nullptr, m));
    SKM_TRY(d_error.ensure(2)); SKM_TRY(d_gene.ensure((size_t)std::max<int64_t>(n_tx, 1)));
    HIP_TRY(hipMemset(d_error.p, 0, 2 * sizeof(int)));
    if (n_tx) HIP_TRY(hipMemcpy(d_gene.p, tx_gene, n_tx * 4, hipMemcpyHostToDevice));
    if (n) {
        SKM_TRY(d_mol_class.ensure(n)); SKM_TRY(d_mol_umi.ensure(n)); SKM_TRY(keys.ensure(n));
        HIP_TRY(hipMemcpy(d_mol_class.p, mol_class, n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_mol_umi.p, mol_umi, n * 4, hipMemcpyHostToDevice));
        launch_resolve_pairs(up.t.sample, d_mol_class.p, d_mol_umi.p, n, keys.key.p, keys.cls.p, keys.number.p, nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (em_steps > 0) SKM_TRY(distributed_matrix_sorted(m.get(), up.t, keys, n, d_gene.p, n_tx, em_steps, d_error.p, nullptr));
    else SKM_TRY(resolved_matrix_sorted(m.get(), up.t, keys, n, 32, d_gene.p, n_tx, d_error.p, nullptr));
    drain.dismiss();
    *out = m.release();
    return SKM_OK;
}

}  // namespace

extern "C" int skm_gene_matrix_from_molecule_classes(int device, int64_t n_classes, const int64_t *class_offsets,
                                                     const int32_t *class_targets, const int32_t *class_sample, int64_t n,
                                                     const int32_t *mol_class, const uint32_t *mol_umi, int64_t n_samples,
                                                     int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, skm_gene_matrix **out)
{
    return matrix_from_molecule_classes(device, n_classes, class_offsets, class_targets, class_sample, n, mol_class, mol_umi,
                                        n_samples, n_tx, n_genes, tx_gene, 0, out);
}

extern "C" int skm_gene_matrix_from_molecule_sets(int device, int64_t n_classes, const int64_t *class_offsets,
                                                  const int32_t *class_targets, const int32_t *class_sample, int64_t n,
                                                  const int32_t *mol_class, const uint32_t *mol_umi, int64_t n_samples,
                                                  int64_t n_tx, int64_t n_genes, const int32_t *tx_gene, int64_t max_steps,
                                                  skm_gene_matrix **out)
{
    if (out) *out = nullptr;
    if (max_steps < 1) return fail(SKM_ERR_ARG, "max_steps = %lld: one step at least", (long long)max_steps);
    return matrix_from_molecule_classes(device, n_classes, class_offsets, class_targets, class_sample, n, mol_class, mol_umi,
                                        n_samples, n_tx, n_genes, tx_gene, max_steps, out);
}

// gene_em_kernel alone on host arrays: cell-local rows in, the transposed view made here
extern "C" int skm_gene_em_cells(int device, int64_t n_cells, const int64_t *cell_row_start, const int64_t *u,
                                 const int64_t *cell_set_start, const int64_t *set_start, const int32_t *set_rows,
                                 int64_t max_steps, double *x_out, int64_t *steps_out, int64_t *capped_out)
{
    SKM_TRY(check_device(device));
    if (n_cells < 0 || max_steps < 1 || !cell_row_start || !cell_set_start || (n_cells && (!steps_out || !capped_out)))
        return fail(SKM_ERR_ARG, "bad argument");
    if (n_cells > (int64_t)INT32_MAX - 1) return fail(SKM_ERR_ARG, "%lld cells: 2^31 - 2 at most are possible", (long long)n_cells);
    if (cell_row_start[0] != 0 || cell_set_start[0] != 0) return fail(SKM_ERR_ARG, "cell_row_start and cell_set_start begin at 0");
    for (int64_t c = 0; c < n_cells; ++c)
        if (cell_row_start[c + 1] < cell_row_start[c] || cell_set_start[c + 1] < cell_set_start[c])
            return fail(SKM_ERR_ARG, "cell %lld ends before it begins", (long long)c);
    const int64_t n_rows = cell_row_start[n_cells], n_sets = cell_set_start[n_cells];
    if (n_rows > INT32_MAX || n_sets > INT32_MAX) return fail(SKM_ERR_ARG, "%lld rows, %lld sets: 2^31 - 1 at most", (long long)n_rows, (long long)n_sets);
    if ((n_rows && (!u || !x_out)) || (n_sets && (!set_start || !set_rows))) return fail(SKM_ERR_ARG, "NULL argument");
    for (int64_t r = 0; r < n_rows; ++r)
        if (u[r] < 0) return fail(SKM_ERR_ARG, "row %lld has u = %lld", (long long)r, (long long)u[r]);
    if (n_sets && set_start[0] != 0) return fail(SKM_ERR_ARG, "set_start begins at 0");
    const int64_t n_set_elements = n_sets ? set_start[n_sets] : 0;
    for (int64_t j = 0; j < n_sets; ++j) {
        const int64_t len = set_start[j + 1] - set_start[j];
        if (len < 2 || len > GENE_SET_MAX) return fail(SKM_ERR_ARG, "set %lld has %lld rows: 2 to %d", (long long)j, (long long)len, GENE_SET_MAX);
    }
    if (n_set_elements > INT32_MAX) return fail(SKM_ERR_ARG, "%lld set elements: 2^31 - 1 at most", (long long)n_set_elements);
    // rows of the set's cell, ascending; the transposed view by counting (sets ascending inside a row)
    std::vector<int32_t> rows_global((size_t)std::max<int64_t>(n_set_elements, 1)), row_sets((size_t)std::max<int64_t>(n_set_elements, 1));
    std::vector<int64_t> row_set_start((size_t)n_rows + 1, 0);
    for (int64_t c = 0; c < n_cells; ++c) {
        const int64_t rows = cell_row_start[c + 1] - cell_row_start[c];
        for (int64_t j = cell_set_start[c]; j < cell_set_start[c + 1]; ++j)
            for (int64_t k = set_start[j]; k < set_start[j + 1]; ++k) {
                if (set_rows[k] < 0 || set_rows[k] >= rows)
                    return fail(SKM_ERR_ARG, "set %lld names row %d of its cell's %lld", (long long)j, set_rows[k], (long long)rows);
                if (k > set_start[j] && set_rows[k] <= set_rows[k - 1])
                    return fail(SKM_ERR_ARG, "the rows of set %lld do not ascend", (long long)j);
                rows_global[k] = (int32_t)(cell_row_start[c] + set_rows[k]);
                row_set_start[rows_global[k] + 1]++;
            }
    }
    for (int64_t r = 0; r < n_rows; ++r) row_set_start[r + 1] += row_set_start[r];
    {
        std::vector<int64_t> next(row_set_start.begin(), row_set_start.end() - 1);
        for (int64_t j = 0; j < n_sets; ++j)
            for (int64_t k = set_start[j]; k < set_start[j + 1]; ++k) row_sets[next[rows_global[k]]++] = (int32_t)j;
    }
    if (n_cells == 0) return SKM_OK;
    SKM_TRY(set_device(device));
    DBuf<int64_t> d_cell_row_start, d_cell_set_start, d_set_start, d_row_set_start; DBuf<unsigned long long> d_u;
    DBuf<int32_t> d_set_rows, d_row_sets; DBuf<int> d_error; GeneEmBuffers em;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_cell_row_start.ensure((size_t)n_cells + 1)); SKM_TRY(d_cell_set_start.ensure((size_t)n_cells + 1));
    SKM_TRY(d_set_start.ensure((size_t)n_sets + 1)); SKM_TRY(d_row_set_start.ensure((size_t)n_rows + 1));
    SKM_TRY(d_u.ensure((size_t)std::max<int64_t>(n_rows, 1))); SKM_TRY(d_set_rows.ensure(rows_global.size()));
    SKM_TRY(d_row_sets.ensure(row_sets.size())); SKM_TRY(d_error.ensure(2)); SKM_TRY(em.ensure(n_rows, n_sets, n_cells, nullptr));
    HIP_TRY(hipMemset(d_error.p, 0, 2 * sizeof(int)));
    HIP_TRY(hipMemcpy(d_cell_row_start.p, cell_row_start, (size_t)(n_cells + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cell_set_start.p, cell_set_start, (size_t)(n_cells + 1) * 8, hipMemcpyHostToDevice));
    const int64_t zero = 0;
    HIP_TRY(hipMemcpy(d_set_start.p, n_sets ? set_start : &zero, (size_t)(n_sets + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_row_set_start.p, row_set_start.data(), (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice));
    if (n_rows) HIP_TRY(hipMemcpy(d_u.p, u, (size_t)n_rows * 8, hipMemcpyHostToDevice));       // (non-negative: the same words)
    if (n_set_elements) {
        HIP_TRY(hipMemcpy(d_set_rows.p, rows_global.data(), (size_t)n_set_elements * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_row_sets.p, row_sets.data(), (size_t)n_set_elements * 4, hipMemcpyHostToDevice));
    }
    GeneEm p{};
    p.n_cells = n_cells; p.n_rows = n_rows; p.n_sets = n_sets; p.n_set_elements = n_set_elements;
    p.cell_row_start = d_cell_row_start.p; p.cell_set_start = d_cell_set_start.p; p.u = d_u.p; p.set_start = d_set_start.p;
    p.set_rows = d_set_rows.p; p.row_set_start = d_row_set_start.p; p.row_sets = d_row_sets.p; p.d = em.d.p; p.x = em.x.p;
    p.steps = em.steps.p; p.capped = em.capped.p; p.max_steps = max_steps; p.lds_rows = gene_em_lds_rows(); p.error = d_error.p;
    launch_gene_em(p, nullptr);
    HIP_TRY(hipGetLastError());
    int error[2] = {0, 0};
    HIP_TRY(hipMemcpy(error, d_error.p, 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (n_rows) HIP_TRY(hipMemcpy(x_out, em.x.p, (size_t)n_rows * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(steps_out, em.steps.p, (size_t)n_cells * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(capped_out, em.capped.p, (size_t)n_cells * 8, hipMemcpyDeviceToHost));
    drain.dismiss();
    if (error[1]) return fail(SKM_ERR_STATE, "a row or a set of the EM lies outside its cell");
    return SKM_OK;
}

extern "C" int skm_gene_matrix_read_weights(const skm_gene_matrix *m, double *data)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL argument");
    if (!m->has_em) return fail(SKM_ERR_STATE, "the matrix holds counts: skm_sample_set_distributed_matrix makes one that holds weights");
    if (m->nnz && !data) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_device(m->device));
    if (m->nnz) HIP_TRY(hipMemcpy(data, m->data.p, (size_t)m->nnz * 8, hipMemcpyDeviceToHost));
    return SKM_OK;
}

extern "C" int skm_gene_matrix_read_em(const skm_gene_matrix *m, int64_t *tally, double *to_unnamed)
{
    if (!m || !tally || !to_unnamed) return fail(SKM_ERR_ARG, "NULL argument");
    if (!m->has_em) return fail(SKM_ERR_STATE, "the matrix holds no EM: skm_sample_set_distributed_matrix makes one that does");
    SKM_TRY(set_device(m->device));
    if (m->n_samples) {
        HIP_TRY(hipMemcpy(tally, m->tally.p, (size_t)m->n_samples * GENE_EM_TALLY * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(to_unnamed, m->to_unnamed.p, (size_t)m->n_samples * 8, hipMemcpyDeviceToHost));
    }
    return SKM_OK;
}

extern "C" int skm_gene_matrix_read_tally(const skm_gene_matrix *m, int64_t *tally)
{
    if (!m || !tally) return fail(SKM_ERR_ARG, "NULL argument");
    if (!m->has_tally) return fail(SKM_ERR_STATE, "the matrix holds no tally: skm_sample_set_resolved_matrix makes one that does");
    SKM_TRY(set_device(m->device));
    if (m->n_samples) HIP_TRY(hipMemcpy(tally, m->tally.p, (size_t)m->n_samples * MOLECULE_TALLY * 8, hipMemcpyDeviceToHost));
    return SKM_OK;
}

extern "C" int skm_gene_matrix_shape(const skm_gene_matrix *m, int64_t *n_samples, int64_t *n_genes, int64_t *nnz)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL argument");
    if (n_samples) *n_samples = m->n_samples;
    if (n_genes) *n_genes = m->n_genes;
    if (nnz) *nnz = m->nnz;
    return SKM_OK;
}

extern "C" int skm_gene_matrix_read(const skm_gene_matrix *m, int64_t *indptr, int32_t *indices, int64_t *data, int64_t *other)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL argument");
    if (data && m->has_em) return fail(SKM_ERR_STATE, "the matrix holds weights: skm_gene_matrix_read_weights reads them");
    SKM_TRY(set_device(m->device));
    if (indptr) HIP_TRY(hipMemcpy(indptr, m->indptr.p, (size_t)(m->n_samples + 1) * 8, hipMemcpyDeviceToHost));
    if (indices && m->nnz) HIP_TRY(hipMemcpy(indices, m->indices.p, (size_t)m->nnz * 4, hipMemcpyDeviceToHost));
    if (data && m->nnz) HIP_TRY(hipMemcpy(data, m->data.p, (size_t)m->nnz * 8, hipMemcpyDeviceToHost));
    if (other && m->n_samples) HIP_TRY(hipMemcpy(other, m->other.p, (size_t)m->n_samples * 16, hipMemcpyDeviceToHost));
    return SKM_OK;
}

extern "C" int skm_gene_matrix_destroy(skm_gene_matrix *m)
{
    delete m;
    return SKM_OK;
}
