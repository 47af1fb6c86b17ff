"""The sequence-bias model of --bias in numpy ("Sequence bias"): the yardstick of
tests/test_bias_host.py and tests/test_gpu_bias.py.  Every sum that is not a sum of integers is math.fsum.

Hexamer code: six bases in the mapper's 2-bit codes (A 0, C 1, G 2, T 3), the first base in the top two bits.
"""
import math

import numpy as np

K = 25
BINS = 4096
SHARES = {None: (0.5, 0.5), 'fr': (1.0, 0.0), 'rf': (0.0, 1.0)}       # (s+, s-)

_CODE = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate(b'ACGT'):
    _CODE[_c] = _i
_COMPLEMENT = bytes.maketrans(b'ACGT', b'TGCA')


def reverse_complement(seq):
    return bytes(seq).translate(_COMPLEMENT)[::-1]


def hexamer_code(six):
    """The code of six upper-case ACGT bytes, or -1 when one of them is anything else."""
    codes = _CODE[np.frombuffer(bytes(six), dtype=np.uint8)]
    if codes.size != 6 or (codes < 0).any():
        return -1
    return int((codes * 4 ** np.arange(5, -1, -1)).sum())


def revcomp_code(h):
    """Codes of the reverse complements (an int or an array of ints)."""
    h = np.asarray(h, dtype=np.int64)
    out = np.zeros_like(h)
    for i in range(6):
        out = out * 4 + (3 - ((h >> (2 * i)) & 3))
    return out


def observed_counts(first_reads, aligned):
    """O[4096]: one count per aligned unit at the hexamer of the first six bases of mate 1 (or the single
    read); a unit whose six bases are not all upper-case A, C, G or T is skipped."""
    out = np.zeros(BINS, dtype=np.int64)
    for read, is_aligned in zip(first_reads, aligned):
        if not is_aligned or len(read) < 6:
            continue
        h = hexamer_code(read[:6])
        if h >= 0:
            out[h] += 1
    return out


def rebuild_transcripts(contigs, sequences, targets, lengths):
    """The transcripts from the index alone: for a contig of length L with pooled bases S and a target row
    (e, o): e >= 0: T_e[o .. o + L) = S; e < 0: T_~e[o + 25 - L .. o + 25) = revcomp(S).  Returns (bases,
    known): per transcript a bytearray ('N' where no row covers the base) and a bool array.  A row that
    leaves its transcript raises."""
    pool = np.asarray(sequences).tobytes().upper()
    bases = [bytearray(b'N' * int(n)) for n in lengths]
    known = [np.zeros(int(n), dtype=bool) for n in lengths]
    for contig in contigs:
        offset, length = int(contig['offset']), int(contig['length'])
        forward = pool[offset:offset + length]
        backward = reverse_complement(forward)
        first = int(contig['target_offset'])
        for row in targets[first:first + int(contig['target_count'])]:
            e, o = int(row['entry']), int(row['offset'])
            t, a, s = (e, o, forward) if e >= 0 else (~e, o + K - length, backward)
            if a < 0 or a + length > len(bases[t]):
                raise ValueError('row (%d, %d) of a contig of %d bases leaves transcript %d' % (e, o, length, t))
            if known[t][a:a + length].any():            # (rows that overlap write the same bases)
                seen = known[t][a:a + length]
                assert bytes(np.frombuffer(bytes(bases[t][a:a + length]), 'S1')[seen]) == \
                    bytes(np.frombuffer(s, 'S1')[seen])
            bases[t][a:a + length] = s
            known[t][a:a + length] = True
    return bases, known


def windows(bases, known):
    """h+ of every window of one transcript (positions 0 .. len - 6 whose six bases are all known), in
    position order: int64[n_t]."""
    n = len(bases) - 5
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    codes = _CODE[np.frombuffer(bytes(bases), dtype=np.uint8)]
    good = np.asarray(known, dtype=bool) & (codes >= 0)
    h = np.zeros(n, dtype=np.int64)
    valid = np.ones(n, dtype=bool)
    for i in range(6):
        h = h * 4 + codes[i:i + n].clip(min=0)
        valid &= good[i:i + n]
    return h[valid]


def expected_counts(tx_windows, tpm, strand):
    """E[h] = sum_t w_t sum_p (s+ [h+ = h] + s- [h- = h])"""
    s_plus, s_minus = SHARES[strand]
    rows = []
    for h_plus, w in zip(tx_windows, tpm):
        if w == 0 or h_plus.size == 0:
            continue
        plus = np.bincount(h_plus, minlength=BINS).astype('f8')
        minus = np.bincount(revcomp_code(h_plus), minlength=BINS).astype('f8')
        rows.append(float(w) * (s_plus * plus + s_minus * minus))
    if not rows:
        return np.zeros(BINS, dtype='f8')
    rows = np.asarray(rows)
    return np.asarray([math.fsum(rows[:, h]) for h in range(BINS)], dtype='f8')


def weights(observed, expected):
    """b[h] = ((O[h] + 1) / (sum O + 4096)) / (E[h] / sum E) where E[h] > 0, 1 elsewhere; all 1 when sum O = 0
    or sum E = 0"""
    observed = np.asarray(observed, dtype=np.int64)
    total_o, total_e = int(observed.sum()), math.fsum(expected)
    b = np.ones(BINS, dtype='f8')
    if total_o == 0 or total_e == 0:
        return b
    seen = expected > 0
    b[seen] = ((observed[seen] + 1.0) / (total_o + float(BINS))) / (expected[seen] / total_e)
    return b


def corrected_lengths(eff, tx_windows, b, strand):
    """eff'_t = eff_t (1 / n_t) sum_p (s+ b[h+] + s- b[h-]); eff_t when n_t = 0"""
    s_plus, s_minus = SHARES[strand]
    out = np.array(eff, dtype='f8', copy=True)
    for t, h_plus in enumerate(tx_windows):
        if h_plus.size:
            terms = s_plus * b[h_plus] + s_minus * b[revcomp_code(h_plus)]
            out[t] = eff[t] * (math.fsum(terms.tolist()) / h_plus.size)
    return out


def correct(tx_windows, observed, tpm, eff, strand):
    """(E, b, eff') of the whole model"""
    expected = expected_counts(tx_windows, tpm, strand)
    b = weights(observed, expected)
    return expected, b, corrected_lengths(eff, tx_windows, b, strand)


# ---- the same, base by base and window by window in plain Python: what the arrays above are checked against
def brute_force(transcripts, knowns, observed, tpm, eff, strand):
    s_plus, s_minus = SHARES[strand]
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    per_tx = []
    for seq, known in zip(transcripts, knowns):
        found = []
        for p in range(len(seq) - 5):
            if not all(known[p + i] and seq[p + i] in code for i in range(6)):
                continue
            h_plus = 0
            for i in range(6):
                h_plus = h_plus * 4 + code[seq[p + i]]
            h_minus = 0
            for i in range(5, -1, -1):
                h_minus = h_minus * 4 + (3 - code[seq[p + i]])
            found.append((h_plus, h_minus))
        per_tx.append(found)
    terms = [[] for _ in range(BINS)]
    for found, w in zip(per_tx, tpm):
        for h_plus, h_minus in found:
            terms[h_plus].append(float(w) * s_plus)
            terms[h_minus].append(float(w) * s_minus)
    expected = [math.fsum(t) for t in terms]
    total_o, total_e = sum(int(o) for o in observed), math.fsum(expected)
    b = [1.0] * BINS
    if total_o and total_e:
        for h in range(BINS):
            if expected[h] > 0:
                b[h] = ((int(observed[h]) + 1.0) / (total_o + 4096.0)) / (expected[h] / total_e)
    out = []
    for found, e in zip(per_tx, eff):
        if not found:
            out.append(float(e))
            continue
        out.append(float(e) * (math.fsum(s_plus * b[hp] + s_minus * b[hm] for hp, hm in found) / len(found)))
    return np.asarray(expected), np.asarray(b), np.asarray(out)


# ---- a small transcriptome that meets every case of the reconstruction rule
def synthetic_transcriptome(seed=11):
    """(ids, sequences): A and B share a 60-base segment, C holds the reverse complement of that segment (a
    segment shared in both orientations), D crosses one 40-base stretch twice, E has exactly 25 bases, F has
    10 (no k-mer: all unknown), G is the reverse complement of a stretch of A with tails of its own."""
    rng = np.random.default_rng(seed)

    def random(n):
        return bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, n))
    shared, twice = random(60), random(40)
    a = random(80) + shared + random(70)
    b = random(50) + shared + random(90)
    c = random(65) + reverse_complement(shared) + random(45)
    d = random(30) + twice + random(55) + twice + random(35)
    e = random(25)
    f = random(10)
    g = random(40) + reverse_complement(a[10:75]) + random(30)
    ids = [b'A', b'B', b'C', b'D', b'E', b'F', b'G']
    return ids, [a, b, c, d, e, f, g]
