"""The rule of cell discovery ("Cell discovery") in plain Python: collections.Counter and
nothing of the package.  Barcodes are str; A < C < G < T, which is also the order of str."""
import collections


def census(reads, length, start=0):
    """The barcode reads (str) of a run -> (Counter of clean windows, [counted, short, unreadable])."""
    counts = collections.Counter()
    stats = [0, 0, 0]
    for read in reads:
        if len(read) < start + length:
            stats[1] += 1
            continue
        window = read[start:start + length]
        if window.strip('ACGT'):              # any position that is not an upper-case A, C, G, T
            stats[2] += 1
            continue
        counts[window] += 1
        stats[0] += 1
    return counts, stats


def ranked(counts):
    """[(barcode, count)]: count descending, then barcode ascending"""
    return sorted(counts.items(), key=lambda item: (-item[1], item[0]))


def neighbours(barcode):
    """the 3 L barcodes that differ from `barcode` in exactly one position"""
    return [barcode[:p] + base + barcode[p + 1:] for p in range(len(barcode)) for base in 'ACGT' if base != barcode[p]]


def pick(counts, expect_cells, drop_neighbours=True):
    """A census (Counter, or dict barcode -> count) and N -> (picked [(barcode, count)], candidates
    [(barcode, count, picked 0/1)], info).  ValueError('no readable barcode') for an empty census."""
    if expect_cells < 1:
        raise ValueError('%r expected cells: 1 at least' % (expect_cells,))
    order = ranked(counts)
    if not order:
        raise ValueError('no readable barcode')
    rank = min((expect_cells + 99) // 100, len(order))
    m = order[rank - 1][1]
    threshold = max((m + 9) // 10, 1)
    candidates = [item for item in order if item[1] >= threshold]
    place = {barcode: i for i, (barcode, _) in enumerate(candidates)}
    dropped = set()
    if drop_neighbours:
        for i, (barcode, _) in enumerate(candidates):
            if any(place.get(other, i) < i for other in neighbours(barcode)):       # (dropped itself or not)
                dropped.add(barcode)
    picked = [item for item in candidates if item[0] not in dropped]
    info = dict(rank=rank, rank_count=m, threshold=threshold, candidates=len(candidates), dropped=len(dropped),
                picked=len(picked))
    return picked, [(barcode, count, int(barcode not in dropped)) for barcode, count in candidates], info


def discover(reads, length, expect_cells, start=0, drop_neighbours=True):
    """reads -> (picked, candidates, info) with the census's numbers in info as well"""
    counts, stats = census(reads, length, start)
    picked, candidates, info = pick(counts, expect_cells, drop_neighbours)
    info.update(counted=stats[0], short=stats[1], unreadable=stats[2], distinct=len(counts), units=len(reads))
    return picked, candidates, info
