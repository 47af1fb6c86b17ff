"""The count matrix in plain Python: the gene rule of DESIGN.md section 4 ("Gene-level tables", "Count matrix")
accumulated into a dict {(sample, gene): count}, the CSR over samples that follows from it, and the lines of
matrix.mtx and cells.tsv.  Nothing here touches a GPU or the product."""
import numpy as np

MTX_HEADER = '%%MatrixMarket matrix coordinate integer general\n'


def accumulate(class_offsets, class_targets, class_counts, tx_gene, class_sample=None, n_samples=1):
    """({(sample, gene): count}, other[n_samples][2]): a class whose ids all lie in one named gene adds its count to
    (sample, gene); one whose ids are all unnamed adds to other[sample][1]; every other class -- one with no ids among
    them -- to other[sample][0]"""
    tx_gene = [int(g) for g in tx_gene]
    entries = {}
    other = [[0, 0] for _ in range(n_samples)]
    for c in range(len(class_counts)):
        s = 0 if class_sample is None else int(class_sample[c])
        seen = {tx_gene[int(t)] for t in class_targets[int(class_offsets[c]):int(class_offsets[c + 1])]}
        count = int(class_counts[c])
        if len(seen) == 1 and min(seen) >= 0:
            entries[(s, min(seen))] = entries.get((s, min(seen)), 0) + count
        elif seen == {-1}:
            other[s][1] += count
        else:
            other[s][0] += count
    return entries, np.asarray(other, dtype=np.int64).reshape(n_samples, 2)


def csr(entries, n_samples):
    """(indptr int64[n_samples + 1], indices int32[nnz], data int64[nnz]): the entries with a count, by sample, genes
    ascending inside a sample; a sum of zero makes no entry"""
    kept = sorted((key, count) for key, count in entries.items() if count != 0)
    indptr = np.zeros(n_samples + 1, dtype=np.int64)
    for (s, _), _ in kept:
        indptr[s + 1] += 1
    return (np.cumsum(indptr), np.asarray([g for (_, g), _ in kept], dtype=np.int32),
            np.asarray([count for _, count in kept], dtype=np.int64))


def matrix(class_offsets, class_targets, class_counts, tx_gene, class_sample=None, n_samples=1):
    """(indptr, indices, data, other) of a class table"""
    entries, other = accumulate(class_offsets, class_targets, class_counts, tx_gene, class_sample, n_samples)
    return csr(entries, n_samples) + (other,)


def dense(indptr, indices, data, n_genes):
    """int64[n_samples][n_genes] of a CSR over samples"""
    out = np.zeros((len(indptr) - 1, n_genes), dtype=np.int64)
    for s in range(len(indptr) - 1):
        for k in range(int(indptr[s]), int(indptr[s + 1])):
            out[s, int(indices[k])] += int(data[k])
    return out


def check_csr(indptr, indices, data, n_samples, n_genes):
    """what every count matrix promises: offsets that ascend from 0 to nnz, genes strictly ascending inside a sample
    and inside [0, n_genes), counts above zero"""
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.int64
    assert indptr.shape == (n_samples + 1,) and indices.shape == data.shape == (int(indptr[-1]),)
    assert indptr[0] == 0 and (np.diff(indptr) >= 0).all()
    assert (data > 0).all()
    for s in range(n_samples):
        row = indices[indptr[s]:indptr[s + 1]]
        assert (np.diff(row) > 0).all() and (row.size == 0 or (row[0] >= 0 and row[-1] < n_genes))


def mtx_lines(indptr, indices, data, n_genes, comment):
    """the lines of matrix.mtx: genes as rows, samples as columns, 1-based, samples ascending"""
    lines = [MTX_HEADER, comment + '\n', '%d %d %d\n' % (n_genes, len(indptr) - 1, len(data))]
    for s in range(len(indptr) - 1):
        for k in range(int(indptr[s]), int(indptr[s + 1])):
            lines.append('%d %d %d\n' % (int(indices[k]) + 1, s + 1, int(data[k])))
    return lines


def parse_mtx(lines):
    """(n_genes, comment, indptr, indices, data) back from the lines of matrix.mtx, which must be in CSR order"""
    assert lines[0] == MTX_HEADER and lines[1].startswith('%')
    n_genes, n_samples, nnz = (int(word) for word in lines[2].split())
    assert len(lines) == 3 + nnz
    triples = [tuple(int(word) for word in line.split()) for line in lines[3:]]
    assert triples == sorted(triples, key=lambda t: (t[1], t[0]))
    indptr = np.zeros(n_samples + 1, dtype=np.int64)
    for _, s, _ in triples:
        indptr[s] += 1
    return (n_genes, lines[1].rstrip('\n'), np.cumsum(indptr), np.asarray([g - 1 for g, _, _ in triples], dtype=np.int32),
            np.asarray([count for _, _, count in triples], dtype=np.int64))


def cells_lines(names, units, indptr, data, other):
    """the lines of cells.tsv: name, units, aligned units, units inside one gene, ambiguous between genes, units of
    unnamed transcripts, genes with a count"""
    lines = []
    for s, name in enumerate(names):
        inside = int(sum(int(v) for v in data[indptr[s]:indptr[s + 1]]))
        aligned = inside + int(other[s][0]) + int(other[s][1])
        lines.append('%s\t%d\t%d\t%d\t%d\t%d\t%d\n' % (name, units[s], aligned, inside, other[s][0], other[s][1],
                                                       indptr[s + 1] - indptr[s]))
    return lines
