"""The UMI rules of DESIGN.md section 4, "UMI collapse", in plain Python / numpy: what the device code is held to.

windows: the UMI of a barcode read is its bases [start, start + length) as 2 bits a base (A0 C1 G2 T3), the first
base in the top bits of the 2 * length used; a read too short for the window, or with a character there that is not
an upper-case A, C, G or T, has none.
survivors: inside a cell the first unit of every (UMI, class) stays, and so does every unit without a class."""
import numpy as np

CODE = {'A': 0, 'C': 1, 'G': 2, 'T': 3}


def windows(reads, start, length):
    """reads: str per barcode read -> (umi uint32[n], readable bool[n]); umi is 0 where there is none"""
    umi = np.zeros(len(reads), dtype=np.uint32)
    readable = np.zeros(len(reads), dtype=bool)
    for r, read in enumerate(reads):
        window = read[start:start + length]
        if len(window) != length or any(c not in CODE for c in window):
            continue
        value = 0
        for c in window:
            value = value * 4 + CODE[c]
        umi[r], readable[r] = value, True
    return umi, readable


def survivors(cell, umi, tuples):
    """cell[u] (negative: the unit belongs to no cell), umi[u], tuples[u] (the unit's class as a tuple of target ids,
    empty = unaligned) in unit order -> bool[n]: the units of a cell that stay.  A unit that belongs to no cell
    is False."""
    stay = np.zeros(len(cell), dtype=bool)
    seen = set()
    for u, (c, m, t) in enumerate(zip(cell, umi, tuples)):
        if c < 0:
            continue
        t = tuple(int(x) for x in t)
        if not t:
            stay[u] = True
            continue
        molecule = (int(c), int(m), t)
        if molecule not in seen:
            seen.add(molecule)
            stay[u] = True
    return stay
