"""Distributed molecules in plain Python ("Distributed molecules"): the groups of "Resolved
molecules" keep the whole intersection of their gene sets, -1 ("no gene") as the element n_genes, the sink; a group of
2 to 16 elements is shared out among them by an EM per cell.  All arithmetic is IEEE double (Python floats) in the one
order the rule states, so the device's doubles are these bit for bit.  Nothing here touches a GPU or the product."""
import numpy as np

import molecule_resolve_reference as mres

GENE_SET_MAX = 16
GENE_EM_FLOOR = 0.001
GENE_EM_TOL = 0.01
MAX_STEPS = 1000
RESOLVED, DISTRIBUTED, WIDE, UNNAMED, COLLISION, ROWS, STEPS, CAPPED = range(8)


def element_list(sets, n_genes):
    """the gene sets of a group's classes -> (outcome, the elements of their intersection ascending, -1 as n_genes;
    None for a wide group or a collision)"""
    common = sorted(n_genes if g < 0 else g for g in frozenset.intersection(*sets))
    if not common:
        return COLLISION, None
    if len(common) > GENE_SET_MAX:
        return WIDE, None
    if len(common) > 1:
        return DISTRIBUTED, common
    return (RESOLVED if common[0] < n_genes else UNNAMED), common


def row_sum(terms):
    """em_row_sum's order (skm_em_core.h): eight partial sums, term k to partial k % 8, then the butterfly"""
    p = [0.0] * 8
    for k, term in enumerate(terms):
        p[k % 8] += term
    return ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]))


def em(u, sets, max_steps=MAX_STEPS):
    """u[r] and the sets (lists of rows, ascending) of one cell -> (x, steps, capped)"""
    u = [float(v) for v in u]
    if not sets:
        return u, 0, False
    holds = [[] for _ in u]                   # the sets that hold a row, ascending
    for j, rows in enumerate(sets):
        for r in rows:
            holds[r].append(j)
    x = [u[r] + row_sum([1.0 / len(sets[j]) for j in holds[r]]) for r in range(len(u))]
    steps = 0
    while True:
        d = []
        for rows in sets:
            total = 0.0
            for r in rows:
                total += x[r]
            d.append(total)
        new = [u[r] + row_sum([x[r] / d[j] if d[j] > 0 else 0.0 for j in holds[r]]) for r in range(len(u))]
        steps += 1
        changes = [abs(new[r] - x[r]) / new[r] for r in range(len(u)) if new[r] > GENE_EM_FLOOR]
        x = new
        if not changes or not (max(changes) > GENE_EM_TOL):
            return x, steps, False
        if steps == max_steps:
            return x, steps, True


def em_cells(cell_row_start, u, cell_set_start, set_start, set_rows, max_steps=MAX_STEPS):
    """the EM of every cell of the CSR arrays that skm_gene_em_cells takes -> (x float64, steps int64, capped int64)"""
    x, steps, capped = [], [], []
    for c in range(len(cell_row_start) - 1):
        sets = [[int(r) for r in set_rows[set_start[j]:set_start[j + 1]]] for j in range(cell_set_start[c], cell_set_start[c + 1])]
        got = em(u[cell_row_start[c]:cell_row_start[c + 1]], sets, max_steps)
        x += got[0]; steps.append(got[1]); capped.append(int(got[2]))
    return np.asarray(x, dtype=np.float64), np.asarray(steps, dtype=np.int64), np.asarray(capped, dtype=np.int64)


def cell_problems(groups, n_genes):
    """{(cell, umi): gene sets of the group's classes} -> ({cell: (row elements, u, sets)}, {cell: tally[:5]})"""
    lists, tally = {}, {}
    for (c, umi), sets in sorted(groups.items()):                    # a cell's groups in ascending UMI order
        outcome, elements = element_list(sets, n_genes)
        tally.setdefault(c, [0] * 5)[outcome] += 1
        lists.setdefault(c, [])
        if elements is not None:
            lists[c].append(elements)
    problems = {}
    for c, cell_lists in lists.items():
        rows = sorted({e for elements in cell_lists for e in elements})
        at = {e: r for r, e in enumerate(rows)}
        u = [0] * len(rows)
        for elements in cell_lists:
            if len(elements) == 1:
                u[at[elements[0]]] += 1
        problems[c] = (rows, u, [[at[e] for e in elements] for elements in cell_lists if len(elements) > 1])
    return problems, tally


def distribute(groups, n_samples, n_genes, max_steps=MAX_STEPS):
    """-> (indptr int64, indices int32, data float64, tally int64[n_samples, 8], to_unnamed float64[n_samples])"""
    problems, outcomes = cell_problems(groups, n_genes)
    tally = np.zeros((n_samples, 8), dtype=np.int64)
    to_unnamed = np.zeros(n_samples, dtype=np.float64)
    indptr, indices, data = [0], [], []
    for c in range(n_samples):
        tally[c, :5] = outcomes.get(c, [0] * 5)
        rows, u, sets = problems.get(c, ([], [], []))
        x, steps, capped = em(u, sets, max_steps)
        tally[c, ROWS:] = len(rows), steps, int(capped)
        for e, v in zip(rows, x):
            if e == n_genes:
                to_unnamed[c] = v
            elif v >= GENE_EM_FLOOR:
                indices.append(e); data.append(v)
        indptr.append(len(indices))
    return (np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32), np.asarray(data, dtype=np.float64), tally,
            to_unnamed)


def groups_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene):
    """molecules given as (class index, UMI), a class's cell class_sample[class] (molecule_resolve_reference.from_classes)"""
    members = {}
    for k, m in zip(mol_class, mol_umi):
        members.setdefault((int(class_sample[int(k)]), int(m)), set()).add(int(k))
    return {key: [mres.gene_set(class_tuples[k], tx_gene) for k in sorted(ks)] for key, ks in members.items()}


def matrix_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene, n_samples, n_genes, max_steps=MAX_STEPS):
    return distribute(groups_from_classes(class_tuples, class_sample, mol_class, mol_umi, tx_gene), n_samples, n_genes, max_steps)


def groups_from_units(cell, umi, tuples, stay, tx_gene):
    """cell[u] (negative: no cell), umi[u], tuples[u] (empty: unaligned), stay[u] in unit order (molecule_resolve_reference.resolve)"""
    classes = {}
    for c, m, t, keep in zip(cell, umi, tuples, stay):
        if keep and c >= 0 and len(t):
            classes.setdefault((int(c), int(m)), set()).add(tuple(int(x) for x in t))
    return {key: [mres.gene_set(t, tx_gene) for t in sorted(ts)] for key, ts in classes.items()}


def matrix(cell, umi, tuples, stay, tx_gene, n_samples, n_genes, max_steps=MAX_STEPS):
    return distribute(groups_from_units(cell, umi, tuples, stay, tx_gene), n_samples, n_genes, max_steps)


def check_csr(indptr, indices, data, n_samples, n_genes):
    """the CSR's shape, and every row's genes ascending and its weights at the cut or above"""
    assert indptr.shape == (n_samples + 1,) and indptr[0] == 0 and indptr[-1] == indices.size == data.size
    assert data.dtype == np.float64 and indices.dtype == np.int32
    for s in range(n_samples):
        genes = indices[indptr[s]:indptr[s + 1]]
        assert (np.diff(genes) > 0).all() and (genes >= 0).all() and (genes < n_genes).all()
    assert (data >= GENE_EM_FLOOR).all()
