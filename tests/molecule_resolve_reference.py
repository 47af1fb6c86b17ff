"""Resolved molecules in plain Python ("Resolved molecules"): the distinct classes among a cell's
live molecules with one UMI form a group, and the intersection of their gene sets names the group's gene.  Nothing
here touches a GPU or the product; the CSR arrays come from tests/gene_matrix_reference.py."""
import numpy as np

import gene_matrix_reference as mref

RESOLVED, RESCUED, MULTI, UNNAMED, COLLISION = range(5)


def gene_set(t, tx_gene):
    """the genes of a class (tuple of transcript ids), -1 ("no gene") an element like any other"""
    return frozenset(int(tx_gene[int(x)]) for x in t)


def verdict(sets):
    """the gene sets of a group's classes -> (outcome, gene or None, rescued)"""
    common = frozenset.intersection(*sets)
    if not common:
        return COLLISION, None, False
    if len(common) > 1:
        return MULTI, None, False
    g = min(common)
    if g < 0:
        return UNNAMED, None, False
    return RESOLVED, g, not any(len(s) == 1 for s in sets)


def resolve_groups(groups, tx_gene):
    """{(cell, umi): set of tuples} -> ({(cell, gene): n}, {cell: [resolved, rescued, multi, unnamed, collision]})"""
    counted, tally = {}, {}
    for (c, _), classes in groups.items():
        outcome, g, rescued = verdict([gene_set(t, tx_gene) for t in classes])
        row = tally.setdefault(c, [0, 0, 0, 0, 0])
        row[outcome] += 1
        if outcome == RESOLVED:
            counted[(c, g)] = counted.get((c, g), 0) + 1
            row[RESCUED] += 1 if rescued else 0
    return counted, tally


def resolve(cell, umi, tuples, stay, tx_gene):
    """cell[u] (negative: no cell), umi[u], tuples[u] (empty: unaligned), stay[u] in unit order -> the resolved entries
    and the tally per cell, over the units with stay[u] (the live molecules are their distinct (cell, class, UMI))"""
    groups = {}
    for c, m, t, keep in zip(cell, umi, tuples, stay):
        if keep and c >= 0 and len(t):
            groups.setdefault((int(c), int(m)), set()).add(tuple(int(x) for x in t))
    return resolve_groups(groups, tx_gene)


def _arrays(counted, tally, n_samples):
    rows = np.zeros((n_samples, 5), dtype=np.int64)
    for c, row in tally.items():
        rows[c] = row
    return mref.csr(counted, n_samples) + (rows,)


def matrix(cell, umi, tuples, stay, tx_gene, n_samples):
    """(indptr, indices, data, tally int64[n_samples][5]) of resolve()"""
    return _arrays(*resolve(cell, umi, tuples, stay, tx_gene), n_samples)


def from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene):
    """the same two dicts from molecules given as (class index, UMI); a class's cell is class_sample[class].  Two
    classes with equal tuples in one cell stay two classes: the index is what tells classes apart"""
    groups = {}
    for k, m in zip(mol_class, mol_umi):
        groups.setdefault((int(class_sample[int(k)]), int(m)), set()).add(int(k))
    counted, tally = {}, {}
    for (c, _), members in groups.items():
        outcome, g, rescued = verdict([gene_set(class_tuples[k], tx_gene) for k in members])
        row = tally.setdefault(c, [0, 0, 0, 0, 0])
        row[outcome] += 1
        if outcome == RESOLVED:
            counted[(c, g)] = counted.get((c, g), 0) + 1
            row[RESCUED] += 1 if rescued else 0
    return counted, tally


def matrix_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples):
    """(indptr, indices, data, tally) of from_classes()"""
    return _arrays(*from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene), n_samples)


def other(tally):
    """other[s] of the resolved matrix's handle: {multi-gene + collision, unnamed}"""
    tally = np.asarray(tally, dtype=np.int64).reshape(-1, 5)
    return np.stack([tally[:, MULTI] + tally[:, COLLISION], tally[:, UNNAMED]], axis=1)
