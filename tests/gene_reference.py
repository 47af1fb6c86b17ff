"""The gene-level tables in plain numpy / Python: what seekmer_amd.infer's gene_map, gene_sums, gene_unique_counts and
gene_table state, written from their definitions ("Gene-level tables") for the tests to compare
with.  Nothing here touches a GPU or the product."""
import numpy as np


def gene_map_from_ids(genes):
    """(gene_ids, tx_gene) from one gene id per transcript (b'' = none)"""
    genes = np.asarray(genes)
    named = genes != b''
    gene_ids = np.unique(genes[named])
    tx_gene = np.full(genes.size, -1, dtype=np.int32)
    tx_gene[named] = np.searchsorted(gene_ids, genes[named])
    return gene_ids, tx_gene


def parse_gene_map(lines, transcript_ids):
    """One gene id per transcript from the lines of a two-column file (bytes): '#' comments, transcript ids cut at
    the first '.', a transcript not named has none.  Returns (genes, ids the index does not hold)."""
    place = {id_: i for i, id_ in enumerate(transcript_ids)}
    genes = [b''] * len(transcript_ids)
    unknown = 0
    for line in lines:
        line = line.rstrip(b'\r\n')
        if not line.strip() or line.startswith(b'#'):
            continue
        id_, gene = line.split(b'\t')[:2]
        id_ = id_.strip().split(b'.')[0]
        if id_ not in place:
            unknown += 1
            continue
        if genes[place[id_]] not in (b'', gene.strip()):
            raise ValueError(id_.decode())
        genes[place[id_]] = gene.strip()
    return genes, unknown


def gene_sums(tx_gene, n_genes, rows):
    """out[r][g] = the sum of rows[r][t] over tx_gene[t] == g, in ascending t from +0.0: numpy.add.at"""
    tx_gene = np.asarray(tx_gene)
    rows = np.atleast_2d(np.asarray(rows, dtype='f8'))
    named = tx_gene >= 0
    out = np.zeros((rows.shape[0], n_genes), dtype='f8')
    for r in range(rows.shape[0]):
        np.add.at(out[r], tx_gene[named], rows[r][named])
    return out


def gene_sums_loop(tx_gene, n_genes, rows):
    """the same, one Python float addition after the other"""
    rows = np.atleast_2d(np.asarray(rows, dtype='f8'))
    out = [[0.0] * n_genes for _ in range(rows.shape[0])]
    for r in range(rows.shape[0]):
        for t, g in enumerate(np.asarray(tx_gene).tolist()):
            if g >= 0:
                out[r][g] = out[r][g] + float(rows[r][t])
    return np.asarray(out, dtype='f8').reshape(rows.shape[0], n_genes)


def unique_counts(class_offsets, class_targets, class_counts, tx_gene, n_genes, class_sample=None, n_samples=1):
    """(unique[n_samples][n_genes], other[n_samples][2]): a class whose transcripts all lie in one named gene counts
    for that gene; one whose transcripts are all unnamed counts in other[1]; every other class in other[0]."""
    tx_gene = np.asarray(tx_gene)
    unique = np.zeros((n_samples, n_genes), dtype=np.int64)
    other = np.zeros((n_samples, 2), dtype=np.int64)
    for c in range(len(class_counts)):
        s = 0 if class_sample is None else int(class_sample[c])
        genes = np.unique(tx_gene[np.asarray(class_targets[class_offsets[c]:class_offsets[c + 1]], dtype=np.int64)])
        if genes.size == 1 and genes[0] >= 0:
            unique[s, genes[0]] += int(class_counts[c])
        elif genes.size == 1:
            other[s, 1] += int(class_counts[c])
        else:
            other[s, 0] += int(class_counts[c])
    return unique, other


def unique_counts_reduceat(class_offsets, class_targets, class_counts, tx_gene, n_genes, class_sample=None, n_samples=1):
    """the same in whole-array numpy, for tables too large for a Python loop (scripts/gene_cost.py): a class lies in
    one gene when the smallest and the largest gene number of its transcripts agree"""
    offsets = np.asarray(class_offsets, dtype=np.int64)
    counts = np.asarray(class_counts, dtype=np.int64)
    sample = np.zeros(counts.size, dtype=np.int64) if class_sample is None else np.asarray(class_sample, dtype=np.int64)
    unique = np.zeros((n_samples, n_genes), dtype=np.int64)
    other = np.zeros((n_samples, 2), dtype=np.int64)
    filled = np.flatnonzero(np.diff(offsets) > 0)
    np.add.at(other[:, 0], sample[np.diff(offsets) == 0], counts[np.diff(offsets) == 0])
    if filled.size:
        genes = np.asarray(tx_gene)[np.asarray(class_targets, dtype=np.int64)]
        # (reduceat over the starts of the filled classes: an empty class between two has no entries to skip)
        low = np.minimum.reduceat(genes, offsets[filled])
        high = np.maximum.reduceat(genes, offsets[filled])
        one, named = low == high, low >= 0
        np.add.at(unique, (sample[filled][one & named], low[one & named]), counts[filled][one & named])
        np.add.at(other[:, 1], sample[filled][one & ~named], counts[filled][one & ~named])
        np.add.at(other[:, 0], sample[filled][~one], counts[filled][~one])
    return unique, other


def unique_counts_loop(class_offsets, class_targets, class_counts, tx_gene, n_genes, class_sample=None, n_samples=1):
    """the same without numpy"""
    tx_gene = [int(g) for g in tx_gene]
    unique = [[0] * n_genes for _ in range(n_samples)]
    other = [[0, 0] for _ in range(n_samples)]
    for c in range(len(class_counts)):
        s = 0 if class_sample is None else int(class_sample[c])
        seen = {tx_gene[int(t)] for t in class_targets[int(class_offsets[c]):int(class_offsets[c + 1])]}
        if len(seen) == 1 and min(seen) >= 0:
            unique[s][min(seen)] += int(class_counts[c])
        elif seen == {-1}:
            other[s][1] += int(class_counts[c])
        else:
            other[s][0] += int(class_counts[c])
    return np.asarray(unique, dtype=np.int64).reshape(n_samples, n_genes), np.asarray(other, dtype=np.int64)


def gene_table(gene_ids, tx_gene, length, effective, tpm, est_counts, unique):
    """The columns of abundance.genes.tsv, per named gene over its transcripts"""
    tx_gene = np.asarray(tx_gene)
    n_genes = len(gene_ids)
    length, effective, tpm = (np.asarray(a, dtype='f8') for a in (length, effective, tpm))
    sums = gene_sums(tx_gene, n_genes, [tpm, est_counts, tpm * length, tpm * effective, length, effective])
    count = np.bincount(tx_gene[tx_gene >= 0], minlength=n_genes)
    table = {'gene_id': np.asarray(gene_ids), 'n_transcripts': count.astype(np.int64), 'tpm': sums[0], 'est_count': sums[1],
             'unique_count': np.asarray(unique, dtype=np.int64)}
    for name, weighted, plain in (('length', sums[2], sums[4]), ('eff_length', sums[3], sums[5])):
        column = np.zeros(n_genes)
        for g in range(n_genes):
            column[g] = weighted[g] / sums[0][g] if sums[0][g] > 0 else plain[g] / max(count[g], 1)
        table[name] = column
    return table


def gene_table_lines(table):
    """the lines of abundance.genes.tsv"""
    lines = ['gene_id\tn_transcripts\tlength\teff_length\test_count\ttpm\tunique_count\n']
    for g in range(len(table['gene_id'])):
        lines.append('%s\t%d\t%g\t%g\t%g\t%g\t%d\n' % (
            table['gene_id'][g].decode(), table['n_transcripts'][g], table['length'][g], table['eff_length'][g],
            table['est_count'][g], table['tpm'][g], table['unique_count'][g]))
    return lines
