"""The inputs of the recordings of the compiled reference (tests/golden/reference_mapper.npz,
reference_builder.npz; recorder: tests/golden/make_reference_recordings.py).

Own code, `random.Random(seed)` only, so that the reads come out the same wherever they are
made: the recorder runs them through the reference on the build machine, the tests regenerate
them and check the recorded SHA-256 before they compare anything.

Every read has at least 25 bases: the reference reads past the end of a shorter one,
so what it returns for such a read cannot be recorded.  All mapper cases run on the index of the
whole chr21 transcriptome, whose k-mer table leaves slot 0 empty (the slot-0 finding).
"""
import hashlib
import random

COMPLEMENT = bytes.maketrans(b'ACGTacgt', b'TGCAtgca')

# the kinds of tests/test_gpu_parity.py::_adversarial_reads, the too-short kind replaced by reads
# of 25 to 30 bases
KINDS = ('plain', 'reverse', 'three_n', 'lower_run', 'substitutions', 'deletion', 'insertion',
         'short_25_30', 'exactly_25', 'random', 'random_head', 'all_lower')

READ_LENGTHS = (33, 100, 251)
UNITS = 3000
LONG_READS = 300

BUILDER_SLICES = (('chr21_0_1', 0, 1), ('chr21_0_2', 0, 2), ('chr21_0_3', 0, 3),
                  ('chr21_0_10', 0, 10), ('chr21_0_50', 0, 50), ('chr21_0_200', 0, 200),
                  ('chr21_100_300', 100, 300), ('chr21_0_800', 0, 800), ('chr21_all', 0, None))
SPARSE_LIMIT = 50           # cases of at most this many transcripts are recorded as arrays too


def reverse_complement(read):
    return bytes(read).translate(COMPLEMENT)[::-1]


def _random_bases(rng, n):
    return bytes(rng.choices(b'ACGT', k=n))


def perturb(read, kind, rng):
    """One read of at least 33 bases -> the read of the given kind (at least 25 bases)."""
    r = bytearray(read)
    if kind == 'reverse':
        r = bytearray(reverse_complement(r))
    elif kind == 'three_n':
        for _ in range(3):
            r[rng.randrange(len(r))] = ord('N')
    elif kind == 'lower_run':
        q = rng.randrange(len(r) - 10)
        r[q:q + 10] = bytes(r[q:q + 10]).lower()
    elif kind == 'substitutions':
        for _ in range(rng.randint(1, 5)):
            r[rng.randrange(len(r))] = rng.choice(b'ACGT')
    elif kind == 'deletion':
        del r[rng.randrange(5, len(r) - 5)]
    elif kind == 'insertion':
        r.insert(rng.randrange(5, len(r) - 5), rng.choice(b'ACGT'))
    elif kind == 'short_25_30':
        r = r[:rng.randint(25, 30)]
    elif kind == 'exactly_25':
        r = r[:25]
    elif kind == 'random':
        r = bytearray(_random_bases(rng, len(r)))
    elif kind == 'random_head':
        r[:30] = _random_bases(rng, 30)
    elif kind == 'all_lower':
        r = bytearray(bytes(r).lower())
    elif kind != 'plain':
        raise ValueError(kind)
    return bytes(r)


def single_reads(seqs, seed, n, read_len):
    rng = random.Random(seed)
    usable = [s for s in seqs if len(s) > read_len + 50]
    out = []
    for i in range(n):
        s = rng.choice(usable)
        at = rng.randrange(len(s) - read_len)
        out.append(perturb(s[at:at + read_len].upper(), KINDS[i % len(KINDS)], rng))
    return out


def paired_reads(seqs, seed, n, read_len):
    """Mates of real fragments of 60-700 bases (shorter than the read among them: the mates are
    then the whole fragment), from either strand; every fourth pair has one mate perturbed."""
    rng = random.Random(seed)
    usable = [s for s in seqs if len(s) > 750]
    out = []
    for i in range(n):
        s = rng.choice(usable)
        size = rng.randint(60, 700)
        at = rng.randrange(len(s) - size)
        fragment = s[at:at + size].upper()
        mates = [fragment[:read_len], reverse_complement(fragment[-read_len:])]
        if rng.random() < 0.5:
            mates.reverse()                     # the fragment from the other strand
        if i % 4 == 3:
            which = rng.randrange(2)
            mates[which] = perturb(mates[which], KINDS[1 + (i // 4) % (len(KINDS) - 1)], rng)
        out += mates
    return out


def long_reads(seqs, seed, n):
    rng = random.Random(seed)
    usable = [s for s in seqs if len(s) > 1600]
    out = []
    for _ in range(n):
        s = rng.choice(usable)
        size = rng.randint(600, 1500)
        at = rng.randrange(len(s) - size)
        r = bytearray(s[at:at + size].upper())
        for _ in range(rng.randint(2, 6)):
            r[rng.randrange(len(r))] = rng.choice(b'ACGT')
        out.append(bytes(r))
    return out


def mapper_cases(seqs, pairs21):
    """[(name, paired, reads)]: `seqs` the chr21 transcripts, `pairs21` the reference's 21 pairs
    interleaved (conftest.pairs21).  A paired case holds len(reads) // 2 units."""
    cases = [('pairs21', True, [bytes(r) for r in pairs21])]
    for k, read_len in enumerate(READ_LENGTHS):
        cases.append(('single%d' % read_len, False, single_reads(seqs, 1000 + k, UNITS, read_len)))
    for k, read_len in enumerate(READ_LENGTHS):
        cases.append(('paired%d' % read_len, True, paired_reads(seqs, 2000 + k, UNITS, read_len)))
    cases.append(('long', False, long_reads(seqs, 3000, LONG_READS)))
    for _, _, reads in cases:
        assert min(len(r) for r in reads) >= 25
    return cases


def builder_cases(seqs, with_extra_seqs):
    """[(name, transcripts)]"""
    cases = [('with_extra', list(with_extra_seqs))]
    for name, lo, hi in BUILDER_SLICES:
        cases.append((name, list(seqs[lo:hi])))
    return cases


def recorded_tuples(recording, name):
    """The recorded tuple of every unit of a mapper case, in unit order."""
    import numpy as np
    counts = recording[name + '/counts'].astype(np.int64)
    ids = recording[name + '/ids'].astype(np.int64).tolist()
    bounds = np.concatenate([[0], np.cumsum(counts)]).tolist()
    return [tuple(ids[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


def reads_digest(reads):
    return hashlib.sha256(b'\n'.join(reads)).hexdigest()


def array_digest(array):
    """SHA-256 of an array's bytes, little-endian and contiguous, in a fixed dtype."""
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


INVALID_KMER = 0xFFFFFFFFFFFFFFFF
KMER_MASK = (1 << 50) - 1


def pack_table(slots, kmer, entry, offset):
    """The occupied rows of a k-mer table in a form that deflates well: rows in (entry, offset)
    order, that is along the contigs, and each k-mer XORed with its predecessor shifted on by
    one base -- two bits inside a contig.  unpack_table gives the rows back in slot order."""
    import numpy as np
    order = np.lexsort((offset, entry))
    kmer = np.asarray(kmer, dtype='<u8')[order]
    shifted = np.zeros_like(kmer)
    shifted[1:] = (kmer[:-1] << np.uint64(2)) & np.uint64(KMER_MASK)
    return {'slots': np.asarray(slots)[order].astype('<i4'), 'kmer_xor': kmer ^ shifted,
            'entry': np.asarray(entry)[order].astype('<i4'), 'offset': np.asarray(offset)[order].astype('<i4')}


def unpack_table(slots, kmer_xor, entry, offset):
    import numpy as np
    kmer, last = [], 0
    for x in kmer_xor.tolist():
        last = x ^ ((last << 2) & KMER_MASK)
        kmer.append(last)
    order = np.argsort(slots, kind='stable')
    return (slots[order], np.array(kmer, dtype='<u8')[order], entry[order], offset[order])


def index_digests(kmers, contigs, sequences, targets):
    """What both recordings and tests digest of an index's four arrays.  The entry/offset of
    EMPTY rows are left out: the reference fills them with -1/-1, our builders with INT_MIN
    (the complement of 0x7FFFFFFF), and no reader looks at them."""
    import numpy as np
    kmer = np.ascontiguousarray(kmers['kmer'], dtype='<u8')
    occupied = kmer != np.uint64(INVALID_KMER)
    contig_table = np.stack([np.asarray(contigs[name]).astype('<i8') if contigs[name].dtype.kind == 'i'
                             else np.asarray(contigs[name]).astype('<u8').view('<i8')
                             for name in contigs.dtype.names], axis=1)
    target_names = targets.dtype.names
    return {
        'kmer': array_digest(kmer),
        'positions': array_digest(np.stack([kmers['entry'][occupied].astype('<i4'),
                                            kmers['offset'][occupied].astype('<i4')], axis=1)),
        'contigs': array_digest(contig_table),
        'sequences': hashlib.sha256(np.asarray(sequences).tobytes()).hexdigest(),
        'targets': array_digest(np.stack([targets[target_names[0]].astype('<i4'),
                                          targets[target_names[1]].astype('<i4')], axis=1)),
    }
