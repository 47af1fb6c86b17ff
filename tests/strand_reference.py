"""Host reference of the strand filter (--fr-stranded / --rf-stranded) and the inputs its tests use.

The rule (include/seekmer_hip.h, skm_mapper_set_strand): a unit's signed target entries are those
the oracle's mapper emits (e >= 0: mate 1 in transcript e's orientation, e < 0: antisense to
transcript ~e).  Mode 'fr' keeps the entries with e >= 0, mode 'rf' those with e < 0, in their
order; a unit with none left is unaligned.  The fragment length of a unit is taken before the
filter, so the histogram is the unstranded run's."""
import numpy as np

_COMP = bytes.maketrans(b'ACGTacgtNn', b'TGCAtgcaNn')


def reverse_complement(seq):
    return bytes(seq).translate(_COMP)[::-1]


class FilteredUnits:
    """What oracle.Classes.update and the per-unit comparisons read: .count, .entries (signed),
    .offsets, tuples() / tuples_signed() as oracle.BatchResult has them."""

    def __init__(self, count, entries):
        self.count = np.ascontiguousarray(count, dtype=np.int32)
        self.entries = np.ascontiguousarray(entries, dtype=np.int32)
        self.offsets = np.zeros(self.count.size + 1, dtype=np.int64)
        np.cumsum(self.count, out=self.offsets[1:])

    def tuples_signed(self):
        e = self.entries.tolist()
        o = self.offsets.tolist()
        return [tuple(e[o[i]:o[i + 1]]) for i in range(self.count.size)]

    def tuples(self):
        return [tuple(~v if v < 0 else v for v in t) for t in self.tuples_signed()]


def keep_mask(entries, mode):
    entries = np.asarray(entries)
    if mode == 'fr':
        return entries >= 0
    if mode == 'rf':
        return entries < 0
    raise ValueError(mode)


def filter_units(count, entries, mode):
    """(counts, signed entries) of a batch, units back to back -> FilteredUnits under `mode`."""
    count = np.asarray(count, dtype=np.int64)
    entries = np.asarray(entries, dtype=np.int32)
    unit = np.repeat(np.arange(count.size), count)
    keep = keep_mask(entries, mode)
    return FilteredUnits(np.bincount(unit[keep], minlength=count.size), entries[keep])


def filter_result(result, mode):
    return filter_units(result.count, result.entries, mode)


def mixed_units(result):
    """Per unit: holds entries of both signs."""
    count = np.asarray(result.count, dtype=np.int64)
    unit = np.repeat(np.arange(count.size), count)
    neg = np.bincount(unit[np.asarray(result.entries) < 0], minlength=count.size)
    return (neg > 0) & (neg < count)


def emptied_units(result, mode):
    """Per unit: aligned unstranded, unaligned under `mode`."""
    return (np.asarray(result.count) > 0) & (filter_result(result, mode).count == 0)


# ---------------------------------------------------------------- the antisense fixture
DECOY = 6


def antisense_transcriptome(seed=11, n=6, length=1500):
    """`n` random transcripts of `length` bases, then a decoy: the reverse complement of transcript
    0's bases [200, 1200), so that every read of that stretch matches the decoy on the other strand."""
    rng = np.random.default_rng(seed)
    seqs = [bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, length)) for _ in range(n)]
    seqs.append(reverse_complement(seqs[0][200:1200]))
    ids = [b'TX%02d' % i for i in range(len(seqs))]
    return ids, seqs


def stranded_reads(seqs, rng, n_units, paired, mode, read_len=100, origins=range(DECOY)):
    """Reads of a stranded library, drawn from the transcripts `origins`: a fragment of 150-400
    bases; 'fr': mate 1 = its start, mate 2 = the reverse complement of its end; 'rf': the two
    swapped.  Single-ended: mate 1 only.  Returns (reads, origin of every unit)."""
    origins = list(origins)
    reads, origin = [], []
    for _ in range(n_units):
        t = origins[int(rng.integers(len(origins)))]
        s = seqs[t]
        frag = int(rng.integers(150, 401))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        m1, m2 = f[:read_len], reverse_complement(f[-read_len:])
        if mode == 'rf':
            m1, m2 = m2, m1
        reads.extend([m1, m2] if paired else [m1])
        origin.append(t)
    return reads, np.asarray(origin)
