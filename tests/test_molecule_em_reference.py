"""tests/molecule_em_reference.py against first principles ("Distributed molecules"): the closed
form of two genes, the conservation of molecules within a rounding bound that is derived here, cells without sets,
the tally identities against tests/molecule_resolve_reference.py, and the cap.  No device."""
import numpy as np
import pytest

import molecule_em_reference as emref
import molecule_resolve_reference as mres
from test_molecule_resolve_host import _random_units


@pytest.mark.parametrize('a,b,sets', [(3, 1, 2), (10, 30, 20), (1, 1, 1), (100, 1, 50), (5, 7, 11), (1, 200, 150)])
def test_the_closed_form_of_two_genes(a, b, sets):
    """u = [a, b] and M sets {0, 1}.  The molecules are conserved, x0 + x1 = T = a + b + M, so a step is
    x0' = a + M x0 / T: linear with rate rho = M / T and the fixed point a T / (a + b) = (a + b + M) a / (a + b).  The
    error shrinks by rho a step, so the last change is (1 - rho) / rho times the error that is left; the rule stops at
    a change of 1 % of x' at most, which leaves an error of 0.01 rho / (1 - rho) = 0.01 M / (a + b) of x': within 1 %
    for M <= a + b, the cases here (the error relative to the fixed point and not to x' differs in second order, which
    the cases' M < a + b covers)."""
    assert sets < a + b
    x, steps, capped = emref.em([a, b], [[0, 1]] * sets)
    want = [(a + b + sets) * a / (a + b), (a + b + sets) * b / (a + b)]
    print('steps %d, x %r, closed form %r' % (steps, x, want))
    assert not capped and steps >= 1
    for got, exact in zip(x, want):
        assert abs(got - exact) <= 0.01 * exact


def _cells(seed, n_umis):
    """random units (tests/test_molecule_resolve_host.py's) -> the cells' EM problems, the outcomes and the inputs"""
    import umi_reference
    rng = np.random.default_rng(seed)
    cell, umi, tuples, tx_gene, n_cells = _random_units(rng, 4000, n_umis)
    stay = umi_reference.survivors(cell, umi, tuples)
    groups = emref.groups_from_units(cell, umi, tuples, stay, tx_gene)
    return emref.cell_problems(groups, 12), (cell, umi, tuples, stay, tx_gene, n_cells)


def test_a_cell_keeps_its_molecules_within_rounding():
    """Every step gives back what it takes: the sum over r of x'[r] is the sum of u plus, for every set j, the sum over
    its rows of x[r] / d[j] = 1 -- whatever x was, so only the LAST step's rounding counts, and the sum of x equals
    resolved + unnamed + distributed (the lists of one, and one per set).  First order: every addition and division
    behind the sum rounds a value that is at most the total by a relative 2^-53.  Behind the sum are, in the last step,
    len(S_j) additions per d[j]; per row one division and one addition per set that holds it, the 7 additions of the
    butterfly and the addition of u; and the additions of the sum itself, one per row.  The bound is that count x 2^-53
    x the total, times 4 for the second order and for partial sums rounded more than once."""
    seen = 0
    for seed, n_umis in ((21, 40), (22, 400), (23, 60)):
        (problems, outcomes), _ = _cells(seed, n_umis)
        for c, (rows, u, sets) in problems.items():
            x, steps, capped = emref.em(u, sets)
            total = sum(u) + len(sets)
            assert total == outcomes[c][emref.RESOLVED] + outcomes[c][emref.UNNAMED] + outcomes[c][emref.DISTRIBUTED]
            operations = sum(len(s) for s in sets) + sum(2 * len(s) for s in sets) + 8 * len(rows) + len(rows)
            bound = 4 * operations * 2.0 ** -53 * total
            got = 0.0
            for v in x:
                got += v
            print('cell %d: %d rows, %d sets, %d steps, sum %r of %d, bound %.3g' % (c, len(rows), len(sets), steps, got, total, bound))
            assert abs(got - total) <= bound and not capped
            seen += len(sets) > 0 and steps >= 2
    assert seen >= 3


def test_a_cell_without_sets_is_its_counts():
    assert emref.em([3, 0, 5], []) == ([3.0, 0.0, 5.0], 0, False)
    assert emref.em([], []) == ([], 0, False)
    # and through the matrix: UMIs that hardly recur -- every group has one class; the groups inside one gene are the
    # resolved matrix's integers as doubles, 0 steps (the ambiguous classes are sets, so: only cells without any)
    (problems, _), (cell, umi, tuples, stay, tx_gene, n_cells) = _cells(24, 2 ** 32)
    keep = np.asarray([bool(s) and len({int(tx_gene[x]) for x in t}) == 1 for t, s in zip(tuples, stay)])
    got = emref.matrix(cell, umi, tuples, keep, tx_gene, n_cells, 12)
    want = mres.matrix(cell, umi, tuples, keep, tx_gene, n_cells)
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    assert got[2].tobytes() == want[2].astype(np.float64).tobytes() and want[2].sum() > 100
    assert not got[3][:, [emref.DISTRIBUTED, emref.WIDE, emref.STEPS, emref.CAPPED]].any()
    assert got[4].tolist() == want[3][:, mres.UNNAMED].astype(np.float64).tolist()


def test_the_tally_identities_against_the_resolved_matrix():
    """resolved, unnamed and collision are the resolved matrix's; distributed + wide is its multi-gene"""
    seen = np.zeros(5, dtype=np.int64)
    for seed, n_umis in ((31, 40), (32, 400), (33, 2 ** 32)):
        _, (cell, umi, tuples, stay, tx_gene, n_cells) = _cells(seed, n_umis)
        for n_genes_cut in (12, 3):            # 3: genes 3.. become "no gene", and with them sets shrink
            gene = np.where(np.asarray(tx_gene) >= n_genes_cut, -1, tx_gene)
            tally = emref.matrix(cell, umi, tuples, stay, gene, n_cells, n_genes_cut)[3]
            resolved = mres.matrix(cell, umi, tuples, stay, gene, n_cells)[3]
            assert tally[:, emref.RESOLVED].tolist() == resolved[:, mres.RESOLVED].tolist()
            assert tally[:, emref.UNNAMED].tolist() == resolved[:, mres.UNNAMED].tolist()
            assert tally[:, emref.COLLISION].tolist() == resolved[:, mres.COLLISION].tolist()
            assert (tally[:, emref.DISTRIBUTED] + tally[:, emref.WIDE]).tolist() == resolved[:, mres.MULTI].tolist()
            seen += tally[:, :5].sum(axis=0)
    assert (seen[[emref.RESOLVED, emref.DISTRIBUTED, emref.UNNAMED, emref.COLLISION]] >= 10).all(), seen
    # wide: more than 16 elements in the intersection
    sets = [frozenset(range(17)), frozenset(range(-1, 40))]
    assert emref.element_list(sets, 50) == (emref.WIDE, None)
    assert emref.element_list([frozenset(range(-1, 15))], 50) == (emref.DISTRIBUTED, list(range(15)) + [50])
    assert emref.element_list([frozenset([-1])], 50) == (emref.UNNAMED, [50])
    assert emref.element_list([frozenset([2]), frozenset([3])], 50) == (emref.COLLISION, None)


def test_a_slow_cell_is_capped():
    """a row without molecules of its own beside a row of 100 decays by a third a step: ten steps to fall below the
    floor, and max_steps = 3 ends it before"""
    u, sets = [100, 0], [[0, 1]] * 50
    x, steps, capped = emref.em(u, sets)
    assert steps > 3 and not capped and x[1] < emref.GENE_EM_FLOOR
    short, short_steps, short_capped = emref.em(u, sets, max_steps=3)
    assert short_steps == 3 and short_capped and short[1] > emref.GENE_EM_FLOOR
    assert emref.em(u, sets, max_steps=steps) == (x, steps, False)       # done at the cap: not capped
    assert emref.em([1, 1], [[0, 1]], max_steps=1) == ([1.5, 1.5], 1, False)
