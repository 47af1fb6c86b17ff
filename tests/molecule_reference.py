"""The molecule matrix in plain Python ("Molecule matrix"): entry (cell, gene) is the number of
distinct UMIs among the cell's surviving units whose class lies inside that gene.  Nothing here touches a GPU or the
product; the CSR arrays come from tests/gene_matrix_reference.py."""
import numpy as np

import gene_matrix_reference as mref


def kind(t, tx_gene):
    """a class (tuple of transcript ids, not empty): its gene g >= 0 when every id has tx_gene == g, -1 when every id is
    unnamed, -2 otherwise (ambiguous between genes, or between a gene and none)"""
    seen = {int(tx_gene[int(x)]) for x in t}
    return min(seen) if len(seen) == 1 else -2


def entries(cell, umi, tuples, stay, tx_gene):
    """cell[u] (negative: no cell), umi[u], tuples[u] (empty: unaligned), stay[u] in unit order ->
    ({(cell, gene): distinct UMIs}, {cell: [ambiguous units, unnamed units]}) over the units with stay[u].  UMIs are
    compared as the numbers they are; the same UMI in two cells, or in two genes of a cell, counts in each."""
    seen, other = {}, {}
    for c, m, t, keep in zip(cell, umi, tuples, stay):
        if not keep or c < 0 or not len(t):
            continue
        g = kind(t, tx_gene)
        if g >= 0:
            seen.setdefault((int(c), g), set()).add(int(m))
        else:
            other.setdefault(int(c), [0, 0])[1 if g == -1 else 0] += 1
    return {key: len(umis) for key, umis in seen.items()}, other


def unit_entries(cell, tuples, stay, tx_gene):
    """{(cell, gene): surviving units inside the gene}: what the unit (count) matrix holds"""
    out = {}
    for c, t, keep in zip(cell, tuples, stay):
        if keep and c >= 0 and len(t) and kind(t, tx_gene) >= 0:
            key = (int(c), kind(t, tx_gene))
            out[key] = out.get(key, 0) + 1
    return out


def matrix(cell, umi, tuples, stay, tx_gene, n_samples):
    """(indptr, indices, data, other int64[n_samples][2]) of entries()"""
    counted, other = entries(cell, umi, tuples, stay, tx_gene)
    rows = np.zeros((n_samples, 2), dtype=np.int64)
    for c, pair in other.items():
        rows[c] = pair
    return mref.csr(counted, n_samples) + (rows,)


def from_triples(sample, gene, umi):
    """{(sample, gene): distinct UMIs} of triples"""
    seen = {}
    for s, g, m in zip(sample, gene, umi):
        seen.setdefault((int(s), int(g)), set()).add(int(m))
    return {key: len(umis) for key, umis in seen.items()}
