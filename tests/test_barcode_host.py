"""Cell barcodes, the parts that need no GPU: the rule itself (tests/barcode_reference.py against hand-written
cases), the whitelist file, the command line, the host gather (skm_packed_gather against numpy fancy indexing) and
the chunk walk of mapper.demux_chunks with a stand-in for the device calls."""
import ctypes
import gzip

import numpy as np
import pytest

import barcode_reference as ref


# ---- the rule, one case per line of it ------------------------------------------------------------------------
WHITELIST = ['ACGTACGT', 'ACGTACGA', 'TTTTTTTT', 'GGGGCCCC', 'GGGGCCCA', 'CATCATCA']


@pytest.mark.parametrize('read, start, mismatches, category, cell', [
    ('ACGTAC', 0, 1, ref.UNREADABLE, -1),                # short
    ('AACGTACG', 1, 1, ref.UNREADABLE, -1),              # short by one base once the window starts at 1
    ('ANGTACNT', 0, 1, ref.UNREADABLE, -1),              # two positions that are not upper-case ACGT
    ('AcGTACgT', 0, 1, ref.UNREADABLE, -1),              # lower case is not clean either
    ('ACGTACGT', 0, 1, ref.EXACT, 0),                    # exact wins over the neighbour ACGTACGA at distance 1
    ('ACGTACGA', 0, 1, ref.EXACT, 1),
    ('xxTTTTTTTTyy', 2, 1, ref.EXACT, 2),                # the window starts where it is told to
    ('TTTTTTTTNN', 0, 1, ref.EXACT, 2),                  # what lies outside the window does not matter
    ('TTTATTTT', 0, 0, ref.NO_MATCH, -1),                # mismatches = 0: one substitution is no match
    ('TTTNTTTT', 0, 0, ref.NO_MATCH, -1),                # ... and neither is one N
    ('TTTATTTT', 0, 1, ref.CORRECTED, 2),                # one substitution, one candidate
    ('TTTNTTTT', 0, 1, ref.CORRECTED, 2),                # one N: the four bases there, one of them an entry
    ('CATCATCN', 0, 1, ref.CORRECTED, 5),
    ('TTAATTTT', 0, 1, ref.NO_MATCH, -1),                # two substitutions: no candidate
    ('TTANTTTT', 0, 1, ref.NO_MATCH, -1),                # an N and a substitution elsewhere: only the N's place is tried
    ('ACGTACGC', 0, 1, ref.AMBIGUOUS, -1),               # one substitution away from two entries
    ('ACGTACGN', 0, 1, ref.AMBIGUOUS, -1),               # N at p with two entries that differ only at p
    ('GGGGCCCN', 0, 1, ref.AMBIGUOUS, -1),
    ('GGGGCCCG', 0, 1, ref.AMBIGUOUS, -1),
])
def test_the_rule_line_by_line(read, start, mismatches, category, cell):
    index = {barcode: i for i, barcode in enumerate(WHITELIST)}
    assert ref.classify(index, 8, read, start, mismatches) == (category, cell)


def test_reference_counts_and_grouping():
    reads = ['ACGTACGT', 'TTTATTTT', 'ACGTACGC', 'TTAATTTT', 'AC', 'TTTTTTTT', 'NNTTTTTT']
    cell, units, stats = ref.assign(WHITELIST, reads)
    assert cell.tolist() == [0, 2, -1, -1, -1, 2, -1]
    assert units.tolist() == [1, 0, 2, 0, 0, 0] and stats.tolist() == [2, 1, 1, 1, 2] and stats.sum() == len(reads)
    order, offsets = ref.group([2, -1, 0, 2, 0, -1, 1, 2], 4)
    assert order.tolist() == [2, 4, 6, 0, 3, 7] and offsets.tolist() == [0, 2, 3, 6, 6]
    order, offsets = ref.group([], 3)
    assert order.size == 0 and offsets.tolist() == [0, 0, 0, 0]


# ---- the whitelist file ------------------------------------------------------------------------------------------
def test_whitelist_file(tmp_path):
    from seekmer_amd import mapper
    path = tmp_path / 'cells.txt'
    path.write_text('# plate 7\nACGT\tA1\n\nTTTT\nGGGA\tB 2\n')
    assert mapper.read_whitelist(path) == (['ACGT', 'TTTT', 'GGGA'], ['A1', 'TTTT', 'B 2'])
    packed = tmp_path / 'cells.txt.gz'
    with gzip.open(packed, 'wt') as f:
        f.write('ACGT\nTTTT\n')
    assert mapper.read_whitelist(packed) == (['ACGT', 'TTTT'], ['ACGT', 'TTTT'])


@pytest.mark.parametrize('text, message', [
    ('', 'no barcode'),
    ('# only a comment\n\n', 'no barcode'),
    ('ACGT\nACG\n', 'bases long'),
    ('A' * 33 + '\n', '1 to 32'),
    ('ACGT\nACGN\n', 'other than'),
    ('ACGT\nacgt\n', 'other than'),
    ('ACGT\nAC T\n', 'other than'),
    ('ACGT\nTTTT\nACGT\n', 'twice'),
    ('ACGT\tc1\nTTTT\tc1\n', 'twice'),
    ('ACGT\tTTTT\nTTTT\n', 'twice'),                     # a default name that meets a given one
    ('ACGT\ta/b\n', 'folder'),
    ('ACGT\t..\n', 'folder'),
    ('ACGT\t\n', 'folder'),
    ('ACGT\tc1\tmore\n', 'column'),
])
def test_malformed_whitelists_are_refused_before_any_read_file(tmp_path, text, message):
    from seekmer_amd import infer, mapper
    path = tmp_path / 'cells.txt'
    path.write_text(text)
    with pytest.raises(ValueError, match=message):
        mapper.BarcodeTable.from_file(path)
    # run_many refuses it before it looks at the read files (these do not exist) or makes the output folder
    with pytest.raises(ValueError, match=message):
        infer.run_many(tmp_path / 'no_index.npz', tmp_path / 'out', [tmp_path / 'r1.fastq', tmp_path / 'r2.fastq'], 1,
                       False, 0, False, barcodes=path, barcode_file=tmp_path / 'bc.fastq')
    assert not (tmp_path / 'out').exists()


# ---- the command line ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arguments, message', [
    (['r1.fq', 'r2.fq', '--barcode-file', 'b.fq'], 'goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--barcode-start', '3'], 'goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--barcode-mismatches', '0'], 'goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--min-units', '5'], 'goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt'], 'needs the barcode reads'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq', '--names', 'a,b'], '--names'),
    (['r1.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq'], 'ONE pooled sample'),
    (['r1.fq', 'r2.fq', 'r3.fq', 'r4.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq'], 'ONE pooled sample'),
    (['r1.fq', 'r2.fq', '-s', '--barcodes', 'w.txt', '--barcode-file', 'b.fq'], 'ONE pooled sample'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq', '--barcode-start', '-1'], '0 or more'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq', '--barcode-mismatches', '2'], 'invalid choice'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq', '--min-units', '0'], '1 or more'),
])
def test_the_command_line_refuses(arguments, message, capsys):
    from seekmer_amd.__main__ import parse_args
    with pytest.raises(SystemExit) as exit_:
        parse_args(['infer-many', 'index.npz', 'out'] + arguments)
    assert exit_.value.code == 2 and message in capsys.readouterr().err


def test_the_command_line_accepts():
    from seekmer_amd.__main__ import parse_args
    opts = parse_args(['infer-many', 'index.npz', 'out', 'r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq'])
    assert (opts['barcode_start'], opts['barcode_mismatches'], opts['min_units']) == (0, 1, 1)
    opts = parse_args(['infer-many', 'index.npz', 'out', 'r.fq', '-s', '--barcodes', 'w.txt', '--barcode-file', 'b.fq',
                       '--barcode-start', '6', '--barcode-mismatches', '0', '--min-units', '50'])
    assert (opts['barcode_start'], opts['barcode_mismatches'], opts['min_units']) == (6, 0, 50)
    opts = parse_args(['infer-many', 'index.npz', 'out', 'a.fq', 'b.fq', 'c.fq', 'd.fq'])      # (as ever)
    assert opts['barcodes'] is None and opts['barcode_file'] is None and opts['min_units'] == 1


def test_run_many_refuses_what_the_command_line_does(tmp_path):
    from seekmer_amd import infer
    white = tmp_path / 'w.txt'
    white.write_text('ACGT\n')
    reads = [tmp_path / 'r1.fastq', tmp_path / 'r2.fastq']
    call = lambda paths=reads, single=False, **k: infer.run_many(tmp_path / 'i.npz', tmp_path / 'out', paths, 1, single, 0, False, **k)
    with pytest.raises(ValueError, match='goes with --barcodes'):
        call(barcode_file=tmp_path / 'b.fastq')
    with pytest.raises(ValueError, match='barcode-file'):
        call(barcodes=white)
    with pytest.raises(ValueError, match='--names'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq', names='a')
    with pytest.raises(ValueError, match='ONE pooled sample'):
        call(paths=reads[:1], barcodes=white, barcode_file=tmp_path / 'b.fastq')
    with pytest.raises(ValueError, match='ONE pooled sample'):
        call(single=True, barcodes=white, barcode_file=tmp_path / 'b.fastq')
    with pytest.raises(ValueError, match='barcode-mismatches'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq', barcode_mismatches=2)
    with pytest.raises(ValueError, match='min-units'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq', min_units=0)
    with pytest.raises(ValueError, match='barcode-start'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq', barcode_start=-2)
    # a compressed read file is refused by name, before anything is written
    for path in reads + [tmp_path / 'b.fastq.gz']:
        path.write_bytes(b'')
    with pytest.raises(ValueError, match='plain FASTQ'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq.gz')
    assert not (tmp_path / 'out').exists()


# ---- the host gather ----------------------------------------------------------------------------------------------
def _piece(rng, n, code_words, stride, uniform, exceptions, first_read=0, stream=0):
    """A piece over arrays made here: codes strided by `stride` words, ragged or uniform lengths, `exceptions`
    reads with a bit plane.  Returns (raw struct, its arrays as dense numpy: codes, lengths, {read: plane})."""
    from seekmer_amd import _native
    flat = rng.integers(0, 2 ** 63, size=max(n * stride, 1), dtype=np.uint64)
    lengths = np.full(n, 32 * code_words - 3, dtype=np.uint32) if uniform else \
        rng.integers(1, 32 * code_words + 1, size=n).astype(np.uint32)
    reads = np.sort(rng.choice(n, size=min(exceptions, n), replace=False)).astype(np.uint32)
    masks = rng.integers(0, 2 ** 32, size=(reads.size, code_words), dtype=np.uint32)
    raw = _native.PackedReads()
    raw.stream, raw.code_words, raw.first_read, raw.n_reads, raw.read_stride = stream, code_words, first_read, n, stride
    raw.uniform_len = int(lengths[0]) if uniform and n else -1
    raw.codes = flat.ctypes.data
    raw.lengths = None if uniform and n else lengths.ctypes.data
    raw.n_exceptions = reads.size
    raw.exception_reads = reads.ctypes.data if reads.size else None
    raw.exception_masks = masks.ctypes.data if reads.size else None
    dense = np.stack([flat[r * stride:r * stride + code_words] for r in range(n)]) if n else np.zeros((0, code_words), np.uint64)
    return raw, (dense, lengths, dict(zip(reads.tolist(), masks)), (flat, lengths, reads, masks))


def _gather(native, pieces, order, code_words):
    sources = (native.PackedReads * len(pieces))(*[raw for raw, _ in pieces])
    order = np.ascontiguousarray(order, dtype=np.int32)
    n = ctypes.c_int64(-1)
    call = lambda codes, lengths, reads, masks, cap: native.host().skm_packed_gather(
        sources, len(pieces), native.ptr(order, native.c_i32p) if order.size else None, order.size, code_words,
        codes, lengths, reads, masks, cap, ctypes.byref(n))
    assert call(None, None, None, None, 0) == native.SKM_OK            # the sizing call
    cap = n.value
    codes = np.full((order.size, code_words), 0xdead, dtype=np.uint64)
    lengths = np.zeros(order.size, dtype=np.uint32)
    reads = np.zeros(max(cap, 1), dtype=np.uint32)
    masks = np.full((max(cap, 1), code_words), 0xbeef, dtype=np.uint32)
    if cap:
        assert call(codes.ctypes.data, lengths.ctypes.data, reads.ctypes.data, masks.ctypes.data, cap - 1) == native.SKM_ERR_STATE
        assert n.value == cap
    assert call(codes.ctypes.data, lengths.ctypes.data, reads.ctypes.data, masks.ctypes.data, cap) == native.SKM_OK
    assert n.value == cap
    return codes, lengths, reads[:cap], masks[:cap]


def _expect(pieces, order, code_words):
    """numpy fancy indexing over the concatenated pieces"""
    codes = np.concatenate([np.pad(d[0], ((0, 0), (0, code_words - d[0].shape[1]))) for _, d in pieces])
    lengths = np.concatenate([d[1] for _, d in pieces])
    planes, base = {}, 0
    for raw, d in pieces:
        planes.update({base + r: np.pad(m, (0, code_words - m.size)) for r, m in d[2].items()})
        base += raw.n_reads
    order = np.asarray(order, dtype=np.int64)
    chosen = [k for k, at in enumerate(order.tolist()) if at in planes]
    masks = np.stack([planes[order[k]] for k in chosen]) if chosen else np.zeros((0, code_words), np.uint32)
    return codes[order], lengths[order], np.asarray(chosen, dtype=np.uint32), masks


@pytest.mark.parametrize('code_words, stride, uniform, exceptions', [
    (3, 3, True, 0), (3, 3, False, 0), (3, 5, False, 9), (1, 1, True, 4), (2, 7, True, 40), (4, 4, False, 1),
])
def test_gather_is_fancy_indexing(native_libs, code_words, stride, uniform, exceptions):
    rng = np.random.default_rng(code_words * 100 + stride)
    piece = _piece(rng, 40, code_words, stride, uniform, exceptions)
    for order in (rng.permutation(40), np.arange(40), rng.integers(0, 40, size=25), [39], []):
        got, want = _gather(native_libs, [piece], order, code_words), _expect([piece], order, code_words)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        assert (np.diff(got[2].astype(np.int64)) > 0).all()           # the exceptions ascend


def test_gather_spans_source_pieces_of_different_widths(native_libs):
    rng = np.random.default_rng(5)
    pieces = [_piece(rng, 17, 2, 2, False, 5), _piece(rng, 1, 3, 4, True, 1), _piece(rng, 0, 3, 3, True, 0),
              _piece(rng, 30, 1, 6, True, 12)]
    for order in (rng.permutation(48), np.arange(10, 40), [16, 17, 18, 16], [47, 0], []):
        got, want = _gather(native_libs, pieces, order, 3), _expect(pieces, order, 3)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)


def test_gather_checks_its_arguments(native_libs):
    rng = np.random.default_rng(6)
    piece = _piece(rng, 8, 2, 2, False, 2)
    sources = (native_libs.PackedReads * 1)(piece[0])
    n = ctypes.c_int64()
    bad = native_libs.SKM_ERR_ARG
    for order, code_words in (([8], 2), ([-1], 2), ([0], 1)):              # outside the pieces; a source wider than the output
        order = np.asarray(order, dtype=np.int32)
        assert native_libs.host().skm_packed_gather(sources, 1, native_libs.ptr(order, native_libs.c_i32p), 1, code_words,
                                                    None, None, None, None, 0, ctypes.byref(n)) == bad


# ---- the chunk walk -----------------------------------------------------------------------------------------------
def _stream_pieces(rng, stream, n_units, cuts, paired):
    """One stream's reads as consecutive PackedReads pieces cut at `cuts`; read u carries u in its first code word"""
    from seekmer_amd.common import PackedReads
    pieces, bounds = [], [0] + list(cuts) + [n_units]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        codes = np.zeros((hi - lo, 2), dtype=np.uint64)
        codes[:, 0] = np.arange(lo, hi, dtype=np.uint64) * 2 + stream
        codes[:, 1] = rng.integers(0, 2 ** 63, size=hi - lo, dtype=np.uint64)
        lengths = rng.integers(33, 65, size=hi - lo).astype(np.uint32)
        marked = np.flatnonzero(np.arange(lo, hi) % 5 == 0).astype(np.uint32)          # every fifth unit has a bit plane
        masks = np.stack([(marked + lo).astype(np.uint32), np.full(marked.size, 7 + stream, dtype=np.uint32)], axis=1)
        pieces.append(PackedReads.from_arrays(stream, lo, codes, lengths, marked, masks, paired=paired))
    return pieces


@pytest.mark.parametrize('chunk_units', [1, 7, 1000])
@pytest.mark.parametrize('paired', [True, False])
def test_chunk_walk_gives_every_cell_its_units_in_order(native_libs, chunk_units, paired):
    from seekmer_amd import mapper
    rng = np.random.default_rng(chunk_units + paired)
    n_units, n_samples = 60, 5
    sample = rng.integers(-1, n_samples - 1, size=n_units).astype(np.int32)           # (sample 4 has no unit at all)
    streams = [_stream_pieces(rng, 0, n_units + 4, (13, 14, 40), paired)]              # (a surplus of four reads)
    if paired:
        streams.append(_stream_pieces(rng, 1, n_units, (5, 33), paired))
    pieces = [p for group in zip(*streams) for p in group] + [p for s in streams for p in s[min(map(len, streams)):]]
    groups, seen = [], {s: [] for s in range(n_samples)}

    def group(part, n):
        groups.append(len(part))
        return ref.group(part, n)

    def add(s, first_unit, mate1, mate2):
        assert first_unit == len(seen[s]), 'a segment begins where the cell\'s units so far end'
        assert (mate2 is not None) == paired and mate1.n_reads > 0
        units = (mate1.codes[:, 0] // np.uint64(2)).astype(np.int64)
        for k, mate in enumerate([mate1] + ([mate2] if paired else [])):
            assert mate.n_reads == units.size and mate.stream == k
            np.testing.assert_array_equal(mate.codes[:, 0], units.astype(np.uint64) * np.uint64(2) + np.uint64(k))
            source = streams[k]
            for row, u in enumerate(units.tolist()):                   # the read's other arrays came along
                piece = next(p for p in source if p.first_read <= u < p.first_read + p.n_reads)
                assert mate.codes[row, 1] == piece.codes[u - piece.first_read, 1]
                assert mate.lengths[row] == piece.lengths[u - piece.first_read]
            reads, masks = mate.exceptions
            assert reads.tolist() == [row for row, u in enumerate(units.tolist()) if u % 5 == 0]
            assert masks.tolist() == [[u, 7 + k] for u in units.tolist() if u % 5 == 0]
        seen[s] += units.tolist()

    added, walked = mapper.demux_chunks(pieces, paired, sample, n_samples, chunk_units, group, add)
    assert walked == n_units
    for s in range(n_samples):
        assert seen[s] == np.flatnonzero(sample == s).tolist() and added[s] == len(seen[s])
    # the chunks are [0, c), [c, 2 c), ... whatever the pieces' sizes
    assert groups == [min(chunk_units, n_units - a) for a in range(0, n_units, chunk_units)]


def test_chunk_walk_refuses_reads_that_do_not_follow(native_libs):
    from seekmer_amd import mapper
    rng = np.random.default_rng(3)
    pieces = _stream_pieces(rng, 0, 30, (10, 20), False)
    sample = np.zeros(30, dtype=np.int32)
    with pytest.raises(ValueError, match='do not follow'):
        mapper.demux_chunks([pieces[0], pieces[2]], False, sample, 1, 8, ref.group, lambda *a: None)
    with pytest.raises(ValueError, match='stream 1'):
        mapper.demux_chunks(_stream_pieces(rng, 1, 30, (), True), False, sample, 1, 8, ref.group, lambda *a: None)


def test_chunk_units_hook(monkeypatch):
    from seekmer_amd import mapper
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    assert mapper._demux_chunk_units() == mapper.DEMUX_CHUNK_UNITS == 1 << 22
    monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', '1000')
    assert mapper._demux_chunk_units() == 1000
    for bad in ('0', '-3', 'many', str((1 << 22) + 1)):
        monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', bad)
        with pytest.raises(ValueError, match='SKM_DEMUX_CHUNK_UNITS'):
            mapper._demux_chunk_units()


def test_fastq_records_follow_the_lines(native_libs, tmp_path):
    from seekmer_amd import mapper
    for text, records in ((b'', 0), (b'@a\nAC\n+\nII\n', 1), (b'@a\nAC\n+\nII\n@b\n', 1), (b'@a\nAC\n+\nII\n@b\nAC', 2),
                          (b'@a\nAC\n+\nII\n@b\nAC\n+\nII', 2)):
        path = tmp_path / 'r.fastq'
        path.write_bytes(text)
        assert mapper.fastq_records(path) == records, text


# ---- no GPU, no answer --------------------------------------------------------------------------------------------
def test_device_calls_need_a_device(native_libs):
    if native_libs.device_count() > 0:
        pytest.skip('a GPU is present')
    from seekmer_amd import mapper
    hip = native_libs.hip()
    handle = ctypes.c_void_p()
    assert hip.skm_barcodes_create(0, b'ACGTTTTT', 2, 4, ctypes.byref(handle)) == native_libs.SKM_ERR_NO_DEVICE
    assert not handle and b'no HIP device' in hip.skm_last_error()
    sample = np.zeros(4, dtype=np.int32)
    order, offsets = np.zeros(4, dtype=np.int32), np.zeros(2, dtype=np.int64)
    assert hip.skm_units_group(0, native_libs.ptr(sample, native_libs.c_i32p), 4, 1, native_libs.ptr(order, native_libs.c_i32p),
                               native_libs.ptr(offsets, native_libs.c_i64p)) == native_libs.SKM_ERR_NO_DEVICE
    with pytest.raises(native_libs.NativeError) as error:
        mapper.BarcodeTable(['ACGT', 'TTTT'])
    assert error.value.code == native_libs.SKM_ERR_NO_DEVICE
    with pytest.raises(native_libs.NativeError) as error:
        mapper.group_units(sample, 1)
    assert error.value.code == native_libs.SKM_ERR_NO_DEVICE
