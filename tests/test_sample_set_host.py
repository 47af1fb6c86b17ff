"""The host-side pieces of the sample set that need no GPU: how queued segments are cut into launches
and logged (skm_sample_set_plan), how the classes of the shared table are split by sample
(skm_sample_set_split), how a packed reader's pieces become a cell's segments (mapper.sample_segments)
-- each against a brute-force numpy version -- and the argument errors of the Python surface."""
import ctypes

import numpy as np
import pytest


def _plan(native, samples, units, max_units):
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    units = np.ascontiguousarray(units, dtype=np.int64)
    n = ctypes.c_int64()
    call = native.hip().skm_sample_set_plan
    native.check(call(samples.size, native.ptr(samples, native.c_i32p), native.ptr(units, native.c_i64p), max_units, 0,
                      ctypes.byref(n), None, None, None))
    entry_global, entry_local = np.zeros(n.value, dtype=np.int64), np.zeros(n.value, dtype=np.int64)
    entry_sample = np.zeros(n.value, dtype=np.int32)
    if n.value:
        native.check(call(samples.size, native.ptr(samples, native.c_i32p), native.ptr(units, native.c_i64p), max_units,
                          n.value, ctypes.byref(n), native.ptr(entry_global, native.c_i64p),
                          native.ptr(entry_local, native.c_i64p), native.ptr(entry_sample, native.c_i32p)))
    return entry_global, entry_local, entry_sample


def _split(native, log, n_samples, first_seen):
    entry_global, entry_local, entry_sample = log
    first_seen = np.ascontiguousarray(first_seen, dtype=np.int64)
    c = first_seen.size
    class_sample, class_local = np.zeros(c, dtype=np.int32), np.zeros(c, dtype=np.int64)
    order, bounds = np.zeros(c, dtype=np.int64), np.zeros(n_samples + 1, dtype=np.int64)
    native.check(native.hip().skm_sample_set_split(
        entry_global.size, native.ptr(entry_global, native.c_i64p), native.ptr(entry_local, native.c_i64p),
        native.ptr(entry_sample, native.c_i32p), n_samples, c, native.ptr(first_seen, native.c_i64p),
        native.ptr(class_sample, native.c_i32p), native.ptr(class_local, native.c_i64p), native.ptr(order, native.c_i64p),
        native.ptr(bounds, native.c_i64p)))
    return class_sample, class_local, order, bounds


def _unit_owners(samples, units):
    """Brute force: (sample, unit inside the sample) of every unit of the set, in arrival order."""
    done = {}
    owner, local = [], []
    for s, n in zip(samples, units):
        start = done.get(int(s), 0)
        owner += [int(s)] * int(n)
        local += list(range(start, start + int(n)))
        done[int(s)] = start + int(n)
    return np.asarray(owner, dtype=np.int64), np.asarray(local, dtype=np.int64)


@pytest.mark.parametrize('max_units', [1, 7, 1000, 1 << 21])
def test_the_segment_log_tiles_the_units(native_libs, max_units):
    rng = np.random.default_rng(max_units)
    samples = rng.integers(0, 9, 60)
    units = rng.integers(0, 40, 60)
    units[rng.integers(0, 60, 8)] = 0
    entry_global, entry_local, entry_sample = _plan(native_libs, samples, units, max_units)
    owner, local = _unit_owners(samples, units)
    assert entry_global[0] == 0 and (np.diff(entry_global) > 0).all()
    ends = np.append(entry_global[1:], owner.size)
    # no entry crosses a launch border, and every unit of the set is what its entry says
    assert (entry_global // max_units == (ends - 1) // max_units).all()
    for g, e, l, s in zip(entry_global, ends, entry_local, entry_sample):
        assert (owner[g:e] == s).all()
        np.testing.assert_array_equal(local[g:e], np.arange(l, l + e - g))


def test_an_empty_plan(native_libs):
    assert [a.size for a in _plan(native_libs, [3, 1], [0, 0], 10)] == [0, 0, 0]
    with pytest.raises(ValueError):
        _plan(native_libs, [0], [5], 0)
    with pytest.raises(ValueError):
        _plan(native_libs, [-1], [5], 10)


@pytest.mark.parametrize('max_units', [5, 64, 1 << 21])
def test_the_split_by_sample(native_libs, max_units):
    rng = np.random.default_rng(100 + max_units)
    n_samples = 7
    samples = rng.integers(0, n_samples - 1, 50)          # (the last sample stays empty)
    units = rng.integers(1, 30, 50)
    log = _plan(native_libs, samples, units, max_units)
    owner, local = _unit_owners(samples, units)
    first_seen = rng.choice(owner.size, size=owner.size // 3, replace=False)     # one class per picked unit
    class_sample, class_local, order, bounds = _split(native_libs, log, n_samples, first_seen)
    np.testing.assert_array_equal(class_sample, owner[first_seen])
    np.testing.assert_array_equal(class_local, local[first_seen])
    want = np.lexsort((local[first_seen], owner[first_seen]))
    np.testing.assert_array_equal(order, want)
    np.testing.assert_array_equal(bounds, np.searchsorted(owner[first_seen][want], np.arange(n_samples + 1)))
    assert bounds[-1] == bounds[-2] == first_seen.size
    # local order inside a sample is global order: its segments were added in ascending order
    for i in range(n_samples):
        mine = order[bounds[i]:bounds[i + 1]]
        assert (np.diff(first_seen[mine]) > 0).all()


def test_the_split_checks_its_log(native_libs):
    good = (np.asarray([0, 4], dtype=np.int64), np.asarray([0, 0], dtype=np.int64), np.asarray([0, 1], dtype=np.int32))
    _split(native_libs, good, 2, [5, 1])
    for bad in ((good[0][::-1].copy(), good[1], good[2]),                                  # not ascending
                (np.asarray([1, 4], dtype=np.int64), good[1], good[2]),                   # does not start at 0
                (good[0], good[1], np.asarray([0, 2], dtype=np.int32))):                  # a sample outside the set
        with pytest.raises(ValueError):
            _split(native_libs, bad, 2, [5, 1])
    assert _split(native_libs, tuple(a[:0] for a in good), 3, [])[3].tolist() == [0, 0, 0, 0]


def _piece(common, stream, first, reads):
    bases = np.frombuffer(b''.join(reads) + b'\0', dtype=np.uint8)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    return common.PackedReads.from_ascii(bases, offsets, stream=stream, first_read=first, paired=True)


def _texts(piece):
    """A piece's reads back as text, N where the bit plane says so."""
    out = []
    exc = dict(zip(*[a.tolist() for a in piece.exceptions])) if piece.exceptions[0].size else {}
    for r in range(piece.n_reads):
        codes, n = piece.codes[r], int(piece.lengths[r])
        text = bytearray(b'ACGT'[(int(codes[i // 32]) >> (62 - 2 * (i % 32))) & 3] for i in range(n))
        if r in exc:
            for i in range(n):
                if not (exc[r][i // 32] >> (31 - i % 32)) & 1:
                    text[i] = ord('N')
        out.append(bytes(text))
    return out


def test_a_readers_pieces_become_in_order_segments(native_libs):
    """Two pairs of files, the first with the longer mate-2 file: pieces of different sizes per stream, a
    cut, a replacing piece -- against zip() of the reads."""
    from seekmer_amd import common, mapper
    rng = np.random.default_rng(9)

    def make(n):
        reads = [bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, int(rng.integers(30, 80)))) for _ in range(n)]
        for r in range(0, n, 5):
            reads[r] = reads[r][:7] + b'N' + reads[r][8:]
        return reads

    a1, a2, b1, b2 = make(23), make(31), make(12), make(9)
    pieces = [_piece(common, 0, 0, a1[:10]), _piece(common, 1, 0, a2[:17]), _piece(common, 0, 10, a1[10:]),
              _piece(common, 1, 17, a2[17:]),
              common.PackedReads.cut(1, 23),                      # the first pair of files held 23 units
              _piece(common, 0, 23, b1[:4]), _piece(common, 1, 23, b2), _piece(common, 0, 27, b1[4:]),
              _piece(common, 0, 30, b1[7:9])]                      # replaces b1[7:] by two reads: 32 reads of mate 1
    segments = mapper.sample_segments(pieces, True)
    want = list(zip(a1 + b1[:9], a2[:23] + b2))                   # zip(file1, file2), pair of files by pair of files
    got, at = [], 0
    for first, mate1, mate2 in segments:
        assert first == at and mate1.n_reads == mate2.n_reads > 0
        assert (mate1.stream, mate2.stream, mate1.first_read, mate2.first_read) == (0, 1, first, first)
        got += list(zip(_texts(mate1), _texts(mate2)))
        at += mate1.n_reads
    assert got == want and at == 32
    single = mapper.sample_segments([_piece(common, 0, 0, a1[:10]), _piece(common, 0, 10, a1[10:])], False)
    assert [(f, m.n_reads, other) for f, m, other in single] == [(0, 10, None), (10, 13, None)]
    assert mapper.sample_segments([], True) == []
    with pytest.raises(ValueError):
        mapper.sample_segments([_piece(common, 0, 0, a1[:10]), _piece(common, 0, 12, a1[12:])], False)    # a gap
    with pytest.raises(ValueError):
        mapper.sample_segments([_piece(common, 1, 0, a1[:10])], False)


class _Feeder:
    def __init__(self, paired):
        self.paired = paired

    def __iter__(self):
        raise AssertionError('the arguments are checked before any read is asked for')


def test_argument_errors_of_map_sample_set(native_libs):
    """All raised before a device is looked for."""
    from seekmer_amd import mapper
    with pytest.raises(ValueError, match='strand'):
        mapper.map_sample_set(None, [_Feeder(True)], strand='ff')
    with pytest.raises(ValueError, match='job_count'):
        mapper.map_sample_set(None, [_Feeder(True)], job_count=0)
    with pytest.raises(ValueError, match='no samples'):
        mapper.map_sample_set(None, [])
    with pytest.raises(ValueError, match='paired and single-ended'):
        mapper.map_sample_set(None, [_Feeder(True), _Feeder(False)])
    with pytest.raises(ValueError, match='strand'):
        mapper.SampleSet(None, True, strand='both')


def test_the_rule_of_impute(native_libs, tmp_path, monkeypatch):
    """use_sample_set: SKM_IMPUTE_PER_CELL=1 exactly, looked up at every call; the named bounds; a
    compressed file counts SAMPLE_SET_COMPRESSED_RATIO times its size, a missing one nothing."""
    from seekmer_amd import impute
    n = impute.SAMPLE_SET_MIN_CELLS + 1
    groups = []
    for cell in range(n):
        paths = (tmp_path / ('c%d_1.fastq' % cell), tmp_path / ('c%d_2.fastq' % cell))
        for path in paths:
            path.write_bytes(b'@r\nACGT\n+\nIIII\n' * (cell + 1))
        groups.append(paths)
    monkeypatch.delenv('SKM_IMPUTE_PER_CELL', raising=False)
    assert impute.use_sample_set(groups)
    monkeypatch.setenv('SKM_IMPUTE_PER_CELL', '1')
    assert not impute.use_sample_set(groups)
    monkeypatch.setenv('SKM_IMPUTE_PER_CELL', 'yes')
    assert impute.use_sample_set(groups)
    assert impute.use_sample_set(groups[:impute.SAMPLE_SET_MIN_CELLS])
    assert not impute.use_sample_set(groups[:impute.SAMPLE_SET_MIN_CELLS - 1])
    assert [impute.cell_text_bytes(group) for group in groups] == [2 * 15 * (cell + 1) for cell in range(n)]
    monkeypatch.setattr(impute, 'SAMPLE_SET_MAX_CELL_BYTES', 2 * 15 * n - 1)       # the largest cell: two files of 15 n bytes
    assert not impute.use_sample_set(groups)
    assert impute.use_sample_set(groups[:-1])
    packed = tmp_path / 'c0_1.fastq.gz'
    packed.write_bytes(b'x' * 10)
    assert impute.cell_text_bytes((packed, groups[0][1])) == 10 * impute.SAMPLE_SET_COMPRESSED_RATIO + 15
    assert impute.cell_text_bytes((tmp_path / 'absent.fastq', groups[0][1])) == 15
