"""The mapper's read record, stated in numpy from its format (include/seekmer_hip.h:
skm_mapper_copy_records), not from either packing kernel.

A record of a batch whose longest read has L bases: W = (L + 31) // 32 + 1 words per read (one pad
word), record_words = 3 W + 1 rounded up to a multiple of 16 u32 words.
  u32 words 0 .. 2W      W code words, u64 little endian: base 32 w + i in bits 63 - 2 i, 62 - 2 i of
                         word w; A 0, C 1, G 2, T 3 in either case, anything else 0
  u32 words 2W .. 3W     W flag words: bit 31 - i of word w set = base 32 w + i is an upper-case ACGT
  u32 word 3W            the read's length
  the rest               zero
Everything beyond the read's end is zero."""
import numpy as np

_CODE = np.zeros(256, dtype=np.uint64)
_UPPER = np.zeros(256, dtype=bool)
for _i, _c in enumerate(b'ACGT'):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i            # lower case
    _UPPER[_c] = True


def words_per_read(longest):
    return (int(longest) + 31) // 32 + 1


def record_words(words):
    return (3 * words + 1 + 15) // 16 * 16


def records(bases, offsets, longest=None):
    """uint32 [n_reads][record_words] of the reads bases[offsets[r]:offsets[r + 1]]."""
    bases = np.frombuffer(bytes(bases), dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    lengths = np.diff(offsets)
    if longest is None:
        longest = int(lengths.max()) if n else 0
    W = words_per_read(longest)
    out = np.zeros((n, record_words(W)), dtype=np.uint32)
    for r in range(n):
        read = bases[offsets[r]:offsets[r + 1]]
        codes = np.zeros(W, dtype=np.uint64)
        flags = np.zeros(W, dtype=np.uint64)
        at = np.arange(read.size)
        np.bitwise_or.at(codes, at >> 5, _CODE[read] << (62 - 2 * (at & 31)).astype(np.uint64))
        np.bitwise_or.at(flags, at >> 5, _UPPER[read].astype(np.uint64) << (31 - (at & 31)).astype(np.uint64))
        out[r, 0:2 * W:2] = (codes & np.uint64(0xffffffff)).astype(np.uint32)
        out[r, 1:2 * W:2] = (codes >> np.uint64(32)).astype(np.uint32)
        out[r, 2 * W:3 * W] = flags.astype(np.uint32)
        out[r, 3 * W] = read.size
    return out


def code_words_of(recs, words):
    """[n][W] uint64 code words of records"""
    lo = recs[:, 0:2 * words:2].astype(np.uint64)
    hi = recs[:, 1:2 * words:2].astype(np.uint64)
    return (hi << np.uint64(32)) | lo


def flag_words_of(recs, words):
    return recs[:, 2 * words:3 * words]


# ---------------------------------------------------------------------------------------- the cases
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128, 129, 150, 160, 250)
ODD_BYTES = (b'N', b'n', b'a', b'c', b'g', b't', b'U', b'.', b'\xe9')


def random_reads(rng, lengths):
    """ACGT reads of the given lengths, back to back: (uint8 bases, int64 offsets)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    bases = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=int(offsets[-1]))].copy()
    return bases, offsets


def sprinkle(bases, offsets, reads, byte):
    """`byte` at positions 0, 15, 16, 31, 32 and the last base of the named reads (where the read is that long)."""
    for r in reads:
        begin, end = int(offsets[r]), int(offsets[r + 1])
        for p in (0, 15, 16, 31, 32, end - begin - 1):
            if 0 <= p < end - begin:
                bases[begin + p] = byte[0]
    return bases


def damage(bases, rng, share=0.05):
    """One base in twenty replaced by one of ODD_BYTES."""
    if bases.size:
        at = rng.integers(0, bases.size, size=max(1, int(bases.size * share)))
        bases[at] = np.frombuffer(b''.join(ODD_BYTES), dtype=np.uint8)[rng.integers(0, len(ODD_BYTES), size=at.size)]
    return bases


FALLBACK_LENGTH = 1400          # W = 45: more than the stage holds for 16 reads (asserted where the library is at hand)


def length_cases():
    """(name, read lengths): an even number of reads each, so that every case also serves as a paired batch"""
    for length in LENGTHS:
        yield 'uniform_%d' % length, [length] * 6
    yield 'ragged', list(LENGTHS) * 2
    # 3 + 7 + 1 = 11 bases first: read i of the rest starts at 11 + 100 i = 11 + 4 i (mod 16), never 0
    yield 'odd_starts', [3, 7, 1] + [100] * 37
    yield 'wide_record', [250] + [50] * 41              # words_per_read is 9 where 50-base reads need 3
    yield 'fallback', [FALLBACK_LENGTH, 100, 0, 1399, FALLBACK_LENGTH, 33]


def block_cases(reads_per_block, length):
    """(name, read lengths) around the block of the staged kernel"""
    for n in sorted({1, 2, reads_per_block - 1, reads_per_block, reads_per_block + 1, 2 * reads_per_block + 1}):
        if n > 0:
            yield 'reads_%d_of_%d' % (n, length), [length] * n


def batch_of(lengths, seed):
    """The reads of a case: random ACGT with one base in twenty damaged"""
    rng = np.random.default_rng(seed)
    bases, offsets = random_reads(rng, lengths)
    return damage(bases, rng), offsets


def odd_byte_batch(byte, seed=5):
    """40 reads of 100 bases behind one of 37 (so that no read starts at a multiple of 16 and read 20, bases
    1937 .. 2037, straddles 16-byte chunks at both ends), `byte` in the first, that one and the last read."""
    rng = np.random.default_rng(seed)
    bases, offsets = random_reads(rng, [37] + [100] * 39)
    return sprinkle(bases, offsets, (0, 20, 39), byte), offsets
