"""The cell-barcode rule and the stable grouping of DESIGN.md section 4, "Cell barcodes", restated in plain
Python and numpy.  Nothing of the package is used: this is what the device code is compared against.

assign(): the barcode of a read is its characters [start, start + L).  In this order:
  1. the read is shorter than start + L                                  -> short
  2. two or more window positions are not upper-case ACGT                -> unreadable
  3. all positions clean and the window is a whitelist entry             -> exact (even with a neighbour at distance 1)
  4. mismatches == 0                                                     -> no match
  5. candidates = entries that differ from the window in exactly one position, a non-clean position always
     counting as differing: one -> corrected, none -> no match, several -> ambiguous
Only exact and corrected reads get a cell."""
import numpy

EXACT, CORRECTED, AMBIGUOUS, NO_MATCH, UNREADABLE = range(5)      # (UNREADABLE counts short reads too)


def classify(index, length, read, start=0, mismatches=1):
    """(category, cell or -1) of one barcode read (str); index: {barcode: cell}"""
    if len(read) < start + length:
        return UNREADABLE, -1
    window = read[start:start + length]
    bad = [i for i, c in enumerate(window) if c not in 'ACGT']
    if len(bad) >= 2:
        return UNREADABLE, -1
    if not bad and window in index:
        return EXACT, index[window]
    if mismatches == 0:
        return NO_MATCH, -1
    candidates = set()
    for p in (bad if bad else range(length)):
        for base in 'ACGT':
            if base != window[p]:
                other = window[:p] + base + window[p + 1:]
                if other in index:
                    candidates.add(index[other])
    if len(candidates) == 1:
        return CORRECTED, candidates.pop()
    return (AMBIGUOUS if candidates else NO_MATCH), -1


def assign(whitelist, reads, start=0, mismatches=1):
    """whitelist: list of str, reads: list of str -> (cell int32[n], cell_units int64[len(whitelist)], stats int64[5])"""
    index = {barcode: i for i, barcode in enumerate(whitelist)}
    assert len(index) == len(whitelist)
    length = len(whitelist[0])
    cell = numpy.full(len(reads), -1, dtype=numpy.int32)
    cell_units = numpy.zeros(len(whitelist), dtype=numpy.int64)
    stats = numpy.zeros(5, dtype=numpy.int64)
    for u, read in enumerate(reads):
        category, c = classify(index, length, read, start, mismatches)
        stats[category] += 1
        cell[u] = c
        if c >= 0:
            cell_units[c] += 1
    return cell, cell_units, stats


def group(sample, n_samples):
    """sample int[n] (negative = dropped) -> (order of the kept units by ascending sample, original order inside a
    sample; offsets int64[n_samples + 1])"""
    sample = numpy.asarray(sample, dtype=numpy.int64)
    keys = numpy.where(sample < 0, n_samples, sample)
    order = numpy.argsort(keys, kind='stable')
    offsets = numpy.searchsorted(keys[order], numpy.arange(n_samples + 1), side='left').astype(numpy.int64)
    return order[:offsets[-1]].astype(numpy.int32), offsets
