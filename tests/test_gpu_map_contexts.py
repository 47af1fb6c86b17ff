"""The map kernel's two layouts of its unit contexts (skm_kernels.h: map_geometry; skm_map.hip: PackedContexts,
WideContexts): which launch takes which, and that both give the CPU oracle's answer at the edges of the packed
fields.

Every GPU case compares, exactly, the units (count, signed entries, begin, end, anchor) and the FULL exported table
with the oracle's on the same reads: class offsets, ids, counts, the first-seen unit of every class, the
fragment-length histogram and the unaligned count.  What is pinned here:
  * fewer units than a block has contexts, and several times more through one block and two (SKM_TEST_MAP_BLOCKS):
    contexts and pair slots -- two bits of a shared word in the packed layout -- are reused many times;
  * read lengths k, k + 1, around one and two 32-base words, the longest read the packed fields hold and one base
    more (the wide kernel), and a batch that one long read sends to the wide kernel;
  * target lists of 64 to 300 entries (mask-extension words) in both layouts, and a list of exactly the packed
    layout's largest size and of one entry more;
  * the same reads through both kernels (SKM_TEST_MAP_LAYOUT): identical tables.
The widths are restated here from skm_kernels.h on purpose: a changed width has to change this file."""
import ctypes

import numpy as np
import pytest

import target_list_reference as lists
from strand_reference import reverse_complement
from test_gpu_parity import _compare_tables, _compare_units

K = 25
PACKED_CONTEXTS = 576
WIDE_CONTEXTS = 480
PACKED_MAX_LEN = 4095                # 12 bits a read position
PACKED_MAX_TARGETS = 4094            # 12 bits of list length + 1, 12 bits of list size
BLOCKS_PER_CU = 4


# ------------------------------------------------------------------------------------- the choice (no GPU)
def _geometry(native_libs, n_units, max_len, max_targets, cu_count=256, block_cap=0):
    packed, contexts, blocks = ctypes.c_int32(-7), ctypes.c_int32(), ctypes.c_int64()
    code = native_libs.hip().skm_map_geometry(n_units, max_len, max_targets, cu_count, block_cap,
                                              ctypes.byref(packed), ctypes.byref(contexts), ctypes.byref(blocks))
    assert code == 0
    return packed.value, contexts.value, blocks.value


@pytest.mark.parametrize('max_len,max_targets,packed', [
    (0, 0, 1), (100, 8, 1), (150, 300, 1),
    (PACKED_MAX_LEN, 8, 1), (PACKED_MAX_LEN + 1, 8, 0), (1 << 20, 8, 0),
    (100, PACKED_MAX_TARGETS, 1), (100, PACKED_MAX_TARGETS + 1, 0), (100, 1 << 24, 0),
    (PACKED_MAX_LEN, PACKED_MAX_TARGETS, 1), (PACKED_MAX_LEN + 1, PACKED_MAX_TARGETS + 1, 0),
])
def test_which_launch_takes_which_kernel(native_libs, max_len, max_targets, packed):
    """Around every bound of the packed layout.  The unit index of a context has 32 bits in both layouts (a
    narrower one frees no word), so the units of a block bound nothing: the largest batch the library takes,
    2^31 - 1 units on one block, keeps the kernel its reads and lists choose."""
    for n_units, cap in ((1, 0), (10_000_000, 0), ((1 << 31) - 1, 1)):
        got, contexts, blocks = _geometry(native_libs, n_units, max_len, max_targets, block_cap=cap)
        assert got == packed
        assert contexts == (PACKED_CONTEXTS if packed else WIDE_CONTEXTS)
        assert blocks == (cap or min(-(-n_units // contexts), 256 * BLOCKS_PER_CU))


def test_the_grid_follows_the_kernels_contexts(native_libs):
    """blocks = min(ceil(units / contexts), 4 per compute unit), then the test cap."""
    for contexts, max_len in ((PACKED_CONTEXTS, 100), (WIDE_CONTEXTS, PACKED_MAX_LEN + 1)):
        for n_units, cus, cap, want in ((0, 8, 0, 0), (1, 8, 0, 1), (contexts, 8, 0, 1), (contexts + 1, 8, 0, 2),
                                        (31 * contexts, 8, 0, 31), (32 * contexts + 1, 8, 0, 32), (10 ** 7, 256, 0, 1024),
                                        (10 ** 7, 256, 2, 2), (3, 256, 2, 1)):
            assert _geometry(native_libs, n_units, max_len, 8, cus, cap) == (int(contexts == PACKED_CONTEXTS), contexts, want)
    hip = native_libs.hip()
    out = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    refs = [ctypes.byref(v) for v in out]
    assert hip.skm_map_geometry(-1, 100, 8, 8, 0, *refs) == native_libs.SKM_ERR_ARG
    assert hip.skm_map_geometry(1, 100, 8, 0, 0, *refs) == native_libs.SKM_ERR_ARG
    assert hip.skm_map_geometry(1, 100, 8, 8, 0, None, refs[1], refs[2]) == native_libs.SKM_ERR_ARG


# ------------------------------------------------------------------------------------------- on the GPU
def _first_seen(expected):
    """The first unit of every class, classes in first-seen order (an empty tuple is no class)."""
    seen = {}
    for unit, ids in enumerate(expected.tuples()):
        if ids and ids not in seen:
            seen[ids] = unit
    return np.fromiter(seen.values(), dtype=np.int64, count=len(seen))


def _map(index, bases, offsets, n_units, paired):
    from seekmer_amd import common, mapper
    result = mapper.MapResult(index, keep_spans=True)
    rm = mapper.ReadMapper(index, result)
    rm.map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    return result, rm.last_batch(n_units)


def _check(oracle, oindex, index, reads, paired, layout, blocks=None):
    """Map `reads` on the GPU and on the oracle; everything equal; the launch took `layout`.  -> the export."""
    bases, offsets = oracle.pack_reads(reads)
    n_units = len(reads) // 2 if paired else len(reads)
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(oindex, bases, offsets, n_units, paired, fld)
    result, units = _map(index, bases, offsets, n_units, paired)
    took = result.map_layout()
    assert took['layout'] == layout, took
    assert took['contexts'] == (PACKED_CONTEXTS if layout == 'packed' else WIDE_CONTEXTS)
    if blocks is not None:
        assert took['blocks'] == blocks
    _compare_units(expected, units)
    _compare_tables(oracle, expected, fld, result)
    table = result.export()
    np.testing.assert_array_equal(table[3], _first_seen(expected), err_msg='first-seen units')
    assert result.sizes()[3] == n_units
    return table, expected


class Small:
    """A synthetic transcriptome of 40 genes and six long transcripts, each four transcripts of different genes
    back to back (5000 bases and more: they hold reads of the packed layout's longest length, which cross the
    joints by contig jumps); its product index and the oracle on the same arrays."""

    def __init__(self, oracle):
        from seekmer_amd import index_builder, synth
        ids, pool, tx_offsets = synth.transcriptome(23, 40)
        sequences = [s.upper() for s in synth.sequences_of(pool, tx_offsets)]
        by_length = sorted(range(len(sequences)), key=lambda i: -len(sequences[i]))
        for j in range(6):
            sequences.append(b''.join(sequences[i] for i in by_length[j:24 + j:6]))
            assert len(sequences[-1]) > 5000
        self.sequences = sequences
        self.joined = b''.join(sequences)
        tx_offsets = np.zeros(len(sequences) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in sequences], out=tx_offsets[1:])
        pool = np.frombuffer(self.joined + b'\0', dtype=np.uint8).copy()
        self.index = index_builder.build_pooled([b'S%05d' % i for i in range(len(sequences))], pool, tx_offsets)
        self.oindex = oracle.OracleIndex(self.index.kmers, self.index.contigs, self.index.sequences,
                                         self.index.targets, lengths=np.diff(tx_offsets))

    def reads(self, seed, n, length, mates=False):
        """`n` reads of exactly `length` bases.  Cut from one transcript where it is long enough, else from the
        transcripts back to back (a chimera: the read maps up to a junction the index does not have).  By kind:
        as cut, reverse complemented, with substitutions, with Ns, lower case in part, random bases in front (the
        first hit lies deep in the read), random bases behind, all random.  mates: every second read is cut a
        little downstream of the one before it and reverse complemented first, as the mate of a pair is."""
        rng = np.random.default_rng(seed)
        letters = np.frombuffer(b'ACGT', dtype=np.uint8)
        fitting = [s for s in self.sequences if len(s) >= length]
        out = []
        source, at = self.joined, 0
        for i in range(n):
            if mates and i % 2 == 1:
                at = min(at + int(rng.integers(0, 150)), len(source) - length)
                read = bytearray(reverse_complement(source[at:at + length]))
            else:
                source = fitting[int(rng.integers(len(fitting)))] if fitting and i % 3 else self.joined
                at = int(rng.integers(0, len(source) - length + 1))
                read = bytearray(source[at:at + length])
            kind = (i // 2 if mates else i) % 8          # (both mates of a pair alike)
            if kind == 1:
                read = bytearray(reverse_complement(bytes(read)))
            elif kind == 2:
                for _ in range(1 + length // 60):
                    read[int(rng.integers(length))] = int(letters[rng.integers(4)])
            elif kind == 3:
                read[int(rng.integers(length))] = ord('N')
            elif kind == 4:
                cut = int(rng.integers(length))
                read[cut:cut + 9] = bytes(read[cut:cut + 9]).lower()
            elif kind == 5 and length > 2 * K:
                front = int(rng.integers(1, length - K))
                read[:front] = letters[rng.integers(0, 4, front)].tobytes()
            elif kind == 6 and length > 2 * K:
                back = int(rng.integers(K, length))
                read[back:] = letters[rng.integers(0, 4, length - back)].tobytes()
            elif kind == 7:
                read = bytearray(letters[rng.integers(0, 4, length)].tobytes())
            assert len(read) == length
            out.append(bytes(read))
        return out


@pytest.fixture(scope='module')
def small(oracle, native_libs):
    return Small(oracle)


@pytest.mark.gpu
@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('n_units,blocks', [(100, None), (PACKED_CONTEXTS // 2 - 1, None), (5000, 1), (5000, 2)])
def test_fewer_units_than_contexts_and_many_more(oracle, small, n_units, blocks, paired, monkeypatch):
    """100 units and one pair slot short of a block's: no context is refilled, most never start.  5000 units
    through one block and through two: a context takes 9 units (a pair slot 17) one after the other, and the last
    units leave short queues and a draining block."""
    if blocks is None:
        monkeypatch.delenv('SKM_TEST_MAP_BLOCKS', raising=False)
    else:
        monkeypatch.setenv('SKM_TEST_MAP_BLOCKS', str(blocks))
    reads = small.reads(n_units + (blocks or 0), n_units * (2 if paired else 1), 100, mates=paired)
    _check(oracle, small.oindex, small.index, reads, paired, 'packed', blocks=blocks or 1)


@pytest.mark.gpu
@pytest.mark.parametrize('length', [K, K + 1, 31, 32, 33, 63, 64, 65, PACKED_MAX_LEN, PACKED_MAX_LEN + 1])
def test_read_lengths_at_the_edges_of_the_fields(oracle, small, length):
    """Every read of the batch has exactly `length` bases: one k-mer, two, the borders of the 32-base record words,
    the longest read of the packed layout (positions up to 4095 - k and a length of twelve set bits beside the
    edge flags in their words) and one base more, which the wide kernel maps."""
    layout = 'packed' if length <= PACKED_MAX_LEN else 'wide'
    n = 240 if length < 1000 else 64
    _, single = _check(oracle, small.oindex, small.index, small.reads(length, n, length), False, layout)
    _, pairs = _check(oracle, small.oindex, small.index, small.reads(length, n, length, mates=True), True, layout)
    assert (single.count > 0).any() and (pairs.count > 0).any()
    if length >= PACKED_MAX_LEN:                      # (the fields' top bits are in use)
        assert int(single.begin.max()) > 2048 and int(single.end.max()) > 2048


@pytest.mark.gpu
@pytest.mark.parametrize('paired', [True, False])
def test_one_long_read_sends_the_batch_to_the_wide_kernel(oracle, small, paired):
    """Reads of 30 to 300 bases and one of 5000: max_len alone chooses the kernel.  Without it: packed."""
    rng = np.random.default_rng(5)
    reads = [read for i in range(150) for read in small.reads(1000 + i, 2, int(rng.integers(30, 301)), mates=True)]
    _check(oracle, small.oindex, small.index, reads, paired, 'packed')
    reads[117] = small.reads(7, 3, 5000)[2]
    _check(oracle, small.oindex, small.index, reads, paired, 'wide')


class Lists:
    """tests/target_list_reference.py's transcriptome (lists of up to 300 entries), built once."""

    def __init__(self, oracle):
        from seekmer_amd import index_builder
        self.fixture = lists.fixture()
        ids, pool, tx_offsets = self.fixture.pooled()
        self.index = index_builder.build_pooled(ids, pool, tx_offsets)
        self.oindex = oracle.OracleIndex(self.index.kmers, self.index.contigs, self.index.sequences,
                                         self.index.targets, lengths=np.diff(tx_offsets))


@pytest.fixture(scope='module')
def long_lists(oracle, native_libs):
    return Lists(oracle)


@pytest.mark.gpu
@pytest.mark.parametrize('paired', [True, False])
def test_both_kernels_give_the_same_tables(oracle, small, long_lists, paired, monkeypatch):
    """The same reads through map_units_kernel and map_units_wide_kernel, on the synthetic transcriptome and on
    the long lists (final lists of 64 to 300 entries: mask words in the workspace, whose stride is the kernel's
    contexts), one block each so that contexts are reused: the oracle's tables both times, byte for byte alike."""
    monkeypatch.setenv('SKM_TEST_MAP_BLOCKS', '1')
    units = long_lists.fixture.pairs if paired else long_lists.fixture.singles
    cases = ((small.oindex, small.index, small.reads(77, 3000, 100, mates=paired)),
             (long_lists.oindex, long_lists.index, lists.reads_of(units)))
    assert long_lists.index.device_info()['max_target_count'] == 300
    for oindex, index, reads in cases:
        tables = {}
        for layout in ('packed', 'wide'):
            monkeypatch.setenv('SKM_TEST_MAP_LAYOUT', layout)
            tables[layout], expected = _check(oracle, oindex, index, reads, paired, layout, blocks=1)
        assert int(expected.count.max()) >= 64 or index is small.index
        for a, b in zip(tables['packed'], tables['wide']):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_the_layout_hook_refuses_what_it_does_not_know(small, monkeypatch):
    from seekmer_amd import mapper
    monkeypatch.setenv('SKM_TEST_MAP_LAYOUT', 'narrow')
    with pytest.raises(ValueError, match='SKM_TEST_MAP_LAYOUT'):
        mapper.MapResult(small.index)


@pytest.mark.gpu
def test_forced_packed_refuses_a_launch_that_does_not_fit(oracle, small, monkeypatch):
    from seekmer_amd import common, mapper
    monkeypatch.setenv('SKM_TEST_MAP_LAYOUT', 'packed')
    bases, offsets = oracle.pack_reads(small.reads(3, 4, PACKED_MAX_LEN + 1))
    result = mapper.MapResult(small.index)
    with pytest.raises(ValueError, match='do not fit'):
        mapper.ReadMapper(small.index, result).map_batch(common.ReadBatch(4, bases, offsets, False))


def _family(n, seed):
    """`n` transcripts that share a core of 80 bases; behind it the even members share a segment of 60, the last
    64 members another one, every other member has 60 bases of its own; 30 bases of its own at both ends.
    (tests/target_list_reference.py's construction, one family, two patterns.)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)

    def rand(k):
        return letters[rng.integers(0, 4, k)].tobytes()
    core, even, last = rand(80), rand(60), rand(60)
    sequences = []
    for m in range(n):
        seg = last if m >= n - 64 else (even if m % 2 == 0 else rand(60))
        sequences.append(rand(30) + core + seg + rand(30))
    return sequences, core, even, last


@pytest.mark.gpu
@pytest.mark.parametrize('n,layout', [(PACKED_MAX_TARGETS, 'packed'), (PACKED_MAX_TARGETS + 1, 'wide')])
def test_a_list_at_the_bound_of_the_list_fields(oracle, native_libs, n, layout):
    """One contig lists `n` transcripts: 4094, the largest list the packed state word holds (list length + 1 =
    4095, all twelve bits; the list's size the same), and 4095, which takes the wide kernel.  Reads inside the core
    keep the whole list (64 mask words); reads that run into a segment keep the even positions of the first n - 64
    or the last 64 positions, read forwards and mirrored; pairs intersect a whole list with a part."""
    from seekmer_amd import index_builder
    sequences, core, even, last = _family(n, n)
    tx_offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sequences], out=tx_offsets[1:])
    pool = np.frombuffer(b''.join(sequences) + b'\0', dtype=np.uint8).copy()
    index = index_builder.build_pooled([b'F%05d' % i for i in range(n)], pool, tx_offsets)
    oindex = oracle.OracleIndex(index.kmers, index.contigs, index.sequences, index.targets, lengths=np.diff(tx_offsets))
    assert index.device_info()['max_target_count'] == n
    singles, pairs = [], []
    for seg in (even, last):
        block = core + seg
        for lo, hi in ((0, 80), (10, 70), (30, 130), (50, 140), (55, 140)):
            singles += [block[lo:hi], reverse_complement(block[lo:hi])]
        for (lo1, hi1), (lo2, hi2) in (((0, 70), (85, 140)), ((10, 80), (80, 140)), ((30, 130), (60, 140))):
            mate1, mate2 = block[lo1:hi1], reverse_complement(block[lo2:hi2])
            pairs += [mate1, mate2, mate2, mate1]
    _, expected = _check(oracle, oindex, index, singles * 3, False, layout)
    assert int(expected.count.max()) == n and 64 in expected.count
    _, expected = _check(oracle, oindex, index, pairs * 3, True, layout)
    assert 64 in expected.count and int(expected.count.max()) >= (n - 64) // 2
