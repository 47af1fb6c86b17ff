"""The rule of DESIGN.md section 4, "UMI mismatches", in plain Python / numpy: what the device code is held to.

With mismatches = 1, inside one cell a unit with a class is removed when an EARLIER unit of that cell (a lower unit
number) has the same class and a UMI at Hamming distance 0 or 1 over the `length` bases -- whether or not that earlier
unit was itself removed.  Unaligned units are never removed; a unit that belongs to no cell is no survivor.

survivors says it the way the device does it (two passes over a table of first units), survivors_by_definition the
way the sentence above does (every pair of units of a group); the tests hold the two against each other."""
import numpy as np


def _neighbours(umi, length):
    """the 3 * length UMIs one substitution away (2 bits a base)"""
    return [umi ^ (x << (2 * p)) for p in range(length) for x in (1, 2, 3)]


def survivors(cell, umi, tuples, length, mismatches):
    """cell[u] (negative: no cell), umi[u] (below 4 ** length), tuples[u] (the class, empty = unaligned) in unit order
    -> bool[n]: the units that stay"""
    if mismatches not in (0, 1):
        raise ValueError('mismatches %r' % (mismatches,))
    first = {}
    molecule = [None] * len(cell)
    for u, (c, m, t) in enumerate(zip(cell, umi, tuples)):
        t = tuple(int(x) for x in t)
        if c < 0 or not t:
            continue
        assert 0 <= int(m) < 4 ** length
        molecule[u] = (int(c), t, int(m))
        first.setdefault(molecule[u], u)
    stay = np.zeros(len(cell), dtype=bool)
    for u, c in enumerate(cell):
        if c < 0:
            continue
        if molecule[u] is None:
            stay[u] = True
            continue
        c, t, m = molecule[u]
        if first[(c, t, m)] != u:
            continue
        stay[u] = not (mismatches and any(first.get((c, t, other), u) < u for other in _neighbours(m, length)))
    return stay


def survivors_by_definition(cell, umi, tuples, length, mismatches):
    """the same, as the rule is stated: per (cell, class), a unit goes if some earlier unit is within distance
    `mismatches` -- quadratic, for the tests only"""
    groups = {}
    stay = np.zeros(len(cell), dtype=bool)
    for u, (c, t) in enumerate(zip(cell, tuples)):
        t = tuple(int(x) for x in t)
        if c < 0:
            continue
        if not t:
            stay[u] = True
            continue
        groups.setdefault((int(c), t), []).append(u)
    base = np.uint64(3) << (np.uint64(2) * np.arange(length, dtype=np.uint64))
    for units in groups.values():
        units = np.asarray(units)
        values = np.asarray(umi, dtype=np.uint64)[units]
        differ = values[:, None] ^ values[None, :]
        distance = ((differ[:, :, None] & base) != 0).sum(axis=2)
        earlier = np.tril(np.ones((len(units), len(units)), dtype=bool), -1)         # [u, v]: v comes before u
        stay[units] = ~((distance <= mismatches) & earlier).any(axis=1)
    return stay
