"""Cell barcodes on the GPU: BarcodeTable.assign and group_units against tests/barcode_reference.py, exactly, and
`infer-many --barcodes` on pooled files against `infer-many` on the per-cell files that the reference
demultiplexer writes from the same reads: every cell's folder as tests/test_gpu_infer_many.py compares folders
(abundance.tsv byte for byte; run_info.json and abundance.npz equal but for the start time and the call)."""
import ctypes
import json

import numpy as np
import pytest

import barcode_reference as ref

pytestmark = pytest.mark.gpu

BASES = 'ACGT'
LDS_MAX = 1024                  # BARCODE_LDS_MAX_ENTRIES (skm_kernels.h): up to here the whitelist is probed from LDS


def _random_barcodes(rng, n, length):
    """n distinct barcodes of `length` bases"""
    seen = set()
    while len(seen) < n:
        seen.update(''.join(row) for row in rng.choice(list(BASES), size=(n - len(seen), length)))
    return sorted(seen, key=lambda _: rng.random())


def _substitute(rng, barcode, places):
    out = list(barcode)
    for p in rng.choice(len(barcode), size=places, replace=False):
        out[p] = rng.choice([b for b in BASES if b != out[p]])
    return ''.join(out)


def _close_whitelist(rng, n, length):
    """a whitelist in which a third of the entries have a neighbour at Hamming distance 1 and a third one at 2"""
    seen = dict.fromkeys(_random_barcodes(rng, n // 3, length))
    for barcode in list(seen):
        seen.setdefault(_substitute(rng, barcode, 1))
        seen.setdefault(_substitute(rng, barcode, min(2, length)))
    return list(seen)


def _barcode_reads(rng, whitelist, start, n):
    """n barcode reads around the whitelist: exact entries, every kind of damage, every kind of length"""
    length = len(whitelist[0])
    text = lambda k: ''.join(rng.choice(list(BASES), size=k))
    reads = []
    kinds = rng.choice(11, size=n, p=[.22, .12, .14, .08, .08, .06, .08, .08, .05, .04, .05])
    for kind in kinds:
        entry = whitelist[rng.integers(len(whitelist))]
        window, prefix, suffix = entry, text(start), text(rng.integers(0, 11))
        if kind == 1:
            window = _substitute(rng, entry, 1)
        elif kind == 2:
            window = _substitute(rng, entry, min(2, length))
        elif kind == 3 or (kind == 4 and length == 1):
            p = rng.integers(length)
            window = entry[:p] + 'N' + entry[p + 1:]
        elif kind == 4:
            p, q = rng.choice(length, size=2, replace=False)
            window = ''.join('N' if i in (p, q) else c for i, c in enumerate(entry))
        elif kind == 5:
            p = rng.integers(length)
            window = entry[:p] + entry[p].lower() + entry[p + 1:]
        elif kind == 6:           # a base that is not clean just outside the window: it must not matter
            if start and rng.random() < 0.5:
                prefix = prefix[:-1] + 'N'
            else:
                suffix = 'n' + suffix
        elif kind == 7:
            suffix, window = '', entry[:-1]                           # start + L - 1 bases
        elif kind == 8:
            suffix = ''                                                 # start + L bases
        elif kind == 9:
            prefix = window = suffix = ''                               # no bases at all
        elif kind == 10:
            window = text(length)
        reads.append(prefix + window + suffix)
    return reads


def _piece(reads, stride_extra=0):
    """the reads (str) as a packed piece; stride_extra > 0: its codes lie `stride_extra` words further apart"""
    from seekmer_amd import _native
    from seekmer_amd.common import PackedReads
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    bases = np.frombuffer((''.join(reads) + 'A').encode(), dtype=np.uint8)
    piece = PackedReads.from_ascii(bases, offsets)
    if not stride_extra or not reads:
        return piece
    codes, lengths, exception_reads, exception_masks = piece._keep
    stride = codes.shape[1] + stride_extra
    wide = np.full((len(reads), stride), 0x5555555555555555, dtype=np.uint64)
    wide[:, :codes.shape[1]] = codes
    raw = _native.PackedReads()
    ctypes.memmove(ctypes.byref(raw), ctypes.byref(piece.raw), ctypes.sizeof(raw))
    raw.read_stride, raw.codes = stride, wide.ctypes.data
    return PackedReads(raw, keep=(wide, lengths, exception_reads, exception_masks))


# (whitelist, length, start, reads, mismatches): the cases of the assign test, by name
def _case(name):
    seed = sum(name.encode())
    rng = np.random.default_rng(seed)
    shapes = {'L8': (8, 0, 96, 3000), 'L8_start28': (8, 28, 96, 3000), 'L16': (16, 0, 5000, 3000), 'L32': (32, 0, 96, 3000),
              'L32_start1': (32, 1, 96, 3000), 'L1': (1, 0, 2, 2000), 'one_entry': (8, 0, 1, 2000),
              'lds_threshold': (16, 0, LDS_MAX, 3000), 'lds_threshold_plus_1': (16, 0, LDS_MAX + 1, 3000),
              'close_pairs': (10, 3, 300, 4000), 'close_pairs_hbm': (12, 30, 3000, 4000), 'no_mismatch': (8, 5, 96, 3000)}
    length, start, n, n_reads = shapes[name]
    whitelist = _close_whitelist(rng, n, length) if name.startswith('close') else _random_barcodes(rng, n, length)
    return whitelist, start, _barcode_reads(rng, whitelist, start, n_reads), 0 if name == 'no_mismatch' else 1


CASES = ('L8', 'L8_start28', 'L16', 'L32', 'L32_start1', 'L1', 'one_entry', 'lds_threshold', 'lds_threshold_plus_1',
         'close_pairs', 'close_pairs_hbm', 'no_mismatch')


@pytest.fixture(scope='module')
def cases():
    """every case with the reference's answer, computed once"""
    out = {}
    for name in CASES:
        whitelist, start, reads, mismatches = _case(name)
        out[name] = (whitelist, start, reads, mismatches, ref.assign(whitelist, reads, start, mismatches))
    return out


def test_the_cases_are_not_trivial(cases):
    """the reference alone: every case assigns between a quarter and three quarters of its reads, and every counter
    is non-zero somewhere -- a device answer of 'nothing assigned' cannot pass"""
    total = np.zeros(5, dtype=np.int64)
    for name, (whitelist, start, reads, mismatches, (cell, units, stats)) in cases.items():
        assigned = (cell >= 0).mean()
        assert 0.25 <= assigned <= 0.75, (name, assigned)
        assert stats.sum() == len(reads) and units.sum() == (cell >= 0).sum() == stats[0] + stats[1]
        total += stats
    assert (total > 0).all(), total
    assert len(cases['lds_threshold'][0]) == LDS_MAX and len(cases['lds_threshold_plus_1'][0]) == LDS_MAX + 1
    assert cases['close_pairs'][4][2][ref.AMBIGUOUS] > 0 and cases['close_pairs_hbm'][4][2][ref.AMBIGUOUS] > 0


@pytest.mark.parametrize('name', CASES)
def test_assign_is_the_reference(native_libs, cases, name):
    from seekmer_amd import mapper
    whitelist, start, reads, mismatches, (cell, units, stats) = cases[name]
    table = mapper.BarcodeTable(whitelist)
    got = table.assign(_piece(reads), start=start, mismatches=mismatches)
    print(name, 'stats', table.stats.tolist(), 'reference', stats.tolist())
    np.testing.assert_array_equal(got, cell)
    np.testing.assert_array_equal(table.cell_units, units)
    np.testing.assert_array_equal(table.stats, stats)


@pytest.mark.parametrize('n_reads', [0, 1, 255, 256, 257, 10000])
def test_assign_piece_sizes_with_strided_codes(native_libs, n_reads):
    from seekmer_amd import mapper
    rng = np.random.default_rng(n_reads + 1)
    whitelist = _random_barcodes(rng, 384, 8)
    reads = _barcode_reads(rng, whitelist, 28, n_reads)               # (the window straddles the first two words)
    cell, units, stats = ref.assign(whitelist, reads, 28, 1)
    assert n_reads < 255 or 0.25 <= (cell >= 0).mean() <= 0.75
    table = mapper.BarcodeTable(whitelist)
    got = table.assign(_piece(reads, stride_extra=3), start=28, mismatches=1)
    np.testing.assert_array_equal(got, cell)
    np.testing.assert_array_equal(table.cell_units, units)
    np.testing.assert_array_equal(table.stats, stats)


def test_two_pieces_add_to_the_same_counters(native_libs, cases):
    from seekmer_amd import mapper
    whitelist, start, reads, mismatches, (cell, units, stats) = cases['close_pairs_hbm']
    table = mapper.BarcodeTable(whitelist)
    first = table.assign(_piece(reads[:1500]), start=start, mismatches=mismatches)
    assert 0 < table.stats.sum() == 1500
    second = table.assign(_piece(reads[1500:], stride_extra=1), start=start, mismatches=mismatches)
    np.testing.assert_array_equal(np.concatenate([first, second]), cell)
    np.testing.assert_array_equal(table.cell_units, units)
    np.testing.assert_array_equal(table.stats, stats)


def test_barcodes_create_refuses_bad_whitelists(native_libs):
    hip = native_libs.hip()
    handle = ctypes.c_void_p()
    for text, n, length in ((b'ACGTACGN', 2, 4), (b'ACGTACGT', 2, 4), (b'ACGTacgt', 2, 4), (b'A' * 33, 1, 33), (b'', 0, 4),
                            (b'ACGT', 1, 0)):
        assert hip.skm_barcodes_create(0, text, n, length, ctypes.byref(handle)) == native_libs.SKM_ERR_ARG, text
        assert not handle


# ---- grouping -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_samples', [1, 2, 513, 65536, 262145])         # (262145: 19 key bits, three passes of the sort)
@pytest.mark.parametrize('n', [0, 1, 4095, 4096, 4097, 3 * 4096 + 5])
def test_group_units_is_a_stable_argsort(native_libs, n, n_samples):
    from seekmer_amd import mapper
    rng = np.random.default_rng(n * 7 + n_samples)
    sample = rng.integers(0, n_samples, size=n).astype(np.int32)
    sample[rng.random(n) < 1 / 3] = -1                                  # about a third of the units are dropped
    order, offsets = mapper.group_units(sample, n_samples)
    want_order, want_offsets = ref.group(sample, n_samples)
    assert n < 4095 or 0.5 < want_order.size / n < 0.8
    np.testing.assert_array_equal(offsets, want_offsets)
    np.testing.assert_array_equal(order, want_order)


def test_group_units_edge_cases(native_libs):
    from seekmer_amd import mapper
    n = 2 * 4096 + 17
    for sample, n_samples in ((np.full(n, -1), 5), (np.full(n, 3), 5), (np.full(n, 0), 1), (np.arange(n) % 700, 700),
                              (-1 - np.arange(n) % 3, 2)):
        order, offsets = mapper.group_units(sample.astype(np.int32), n_samples)
        want_order, want_offsets = ref.group(sample, n_samples)
        np.testing.assert_array_equal(offsets, want_offsets)
        np.testing.assert_array_equal(order, want_order)
    with pytest.raises(ValueError, match='not below n_samples'):
        mapper.group_units(np.asarray([0, 1, 2], dtype=np.int32), 2)


# ---- end to end ---------------------------------------------------------------------------------------------------
READ_LEN = 75
CELL_PAIRS = (2000, 3500, 4000, 0, 2500, 3000)          # cell 3 is on the whitelist and has no reads at all
BARCODE_LENGTH = 12


def _write_fastq(path, reads):
    with open(path, 'w') as f:
        for i, read in enumerate(reads):
            f.write('@r%d\n%s\n+\n%s\n' % (i, read, 'I' * len(read)))


@pytest.fixture(scope='module')
def pooled(native_libs, tmp_path_factory):
    """The index of synth.transcriptome(5, 30); six whitelist cells; their pairs shuffled into one pooled pair of
    FASTQ files with a barcode file (85 % exact, 10 % one substitution, 5 % garbage, two errors or an N); and the
    same reads demultiplexed by the reference into one FASTQ pair per cell."""
    from seekmer_amd import index_builder, synth
    folder = tmp_path_factory.mktemp('pooled')
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    index_path = folder / 'index.npz'
    index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    rng = np.random.default_rng(2024)
    while True:                    # barcodes at distance >= 3 from each other: a substitution never reaches another cell
        whitelist = _random_barcodes(rng, len(CELL_PAIRS), BARCODE_LENGTH)
        if all(sum(a != b for a, b in zip(x, y)) >= 3 for i, x in enumerate(whitelist) for y in whitelist[:i]):
            break
    names = ['cell%d' % c for c in range(len(CELL_PAIRS))]
    (folder / 'whitelist.tsv').write_text('# six wells\n' + ''.join('%s\t%s\n' % row for row in zip(whitelist, names)))
    mates, truth = ([], []), []
    for c, n_pairs in enumerate(CELL_PAIRS):
        if not n_pairs:
            continue
        raw = synth.reads(100 + c % 2, pool, tx_offsets, c * 8000, n_pairs, READ_LEN, True)[0][:-1].tobytes().decode()
        for u in range(n_pairs):
            for mate in (0, 1):
                mates[mate].append(raw[(2 * u + mate) * READ_LEN:(2 * u + mate + 1) * READ_LEN])
        truth += [c] * n_pairs
    shuffle = rng.permutation(len(truth))
    mates = [[mate[u] for u in shuffle] for mate in mates]
    barcodes = []
    for u in shuffle:
        barcode, chance = whitelist[truth[u]], rng.random()
        if 0.85 <= chance < 0.95:
            barcode = _substitute(rng, barcode, 1)
        elif chance >= 0.95:
            barcode = [_substitute(rng, barcode, 2), ''.join(rng.choice(list(BASES), size=BARCODE_LENGTH)),
                       'N' + barcode[1:], barcode[:4] + 'NN' + barcode[6:]][rng.integers(4)]
        barcodes.append('GGA' + barcode + ''.join(rng.choice(list(BASES), size=8)))       # (3 bases, barcode, a tail)
    _write_fastq(folder / 'pool_1.fastq', mates[0])
    _write_fastq(folder / 'pool_2.fastq', mates[1])
    _write_fastq(folder / 'barcodes.fastq', barcodes)
    cell, cell_units, stats = ref.assign(whitelist, barcodes, start=3, mismatches=1)
    assert (stats[[0, 1, 3, 4]] > 0).all() and 0.9 < (cell >= 0).mean() < 1 and cell_units[3] == 0 and (np.delete(cell_units, 3) > 1500).all()
    for c in np.flatnonzero(cell_units):
        for mate in (0, 1):
            _write_fastq(folder / ('%s_%d.fastq' % (names[c], mate + 1)), [mates[mate][u] for u in np.flatnonzero(cell == c)])
    return dict(folder=folder, index=index_path, whitelist=whitelist, names=names, cell_units=cell_units, stats=stats)


def _per_cell_run(pooled, out, single=False, extra=()):
    """today's infer-many on the reference's per-cell files"""
    from seekmer_amd.__main__ import main
    folder = pooled['folder']
    kept = [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'])]
    files = [str(folder / ('%s_%d.fastq' % (name, mate))) for name in kept for mate in ((1,) if single else (1, 2))]
    assert main(['infer-many', str(pooled['index']), str(out), *files, '-b', '2', '--seed', '7', '--names', ','.join(kept),
                 *(['-s'] if single else []), *extra]) == 0
    return out


def _pooled_run(pooled, out, single=False, extra=()):
    from seekmer_amd.__main__ import main
    folder = pooled['folder']
    files = [str(folder / 'pool_1.fastq')] + ([] if single else [str(folder / 'pool_2.fastq')])
    assert main(['infer-many', str(pooled['index']), str(out), *files, '-b', '2', '--seed', '7',
                 '--barcodes', str(folder / 'whitelist.tsv'), '--barcode-file', str(folder / 'barcodes.fastq'),
                 '--barcode-start', '3', *(['-s'] if single else []), *extra]) == 0
    return out


@pytest.fixture(scope='module')
def per_cell(pooled):
    return _per_cell_run(pooled, pooled['folder'] / 'per_cell')


def _assert_same_folders(ours, theirs, names):
    from test_gpu_infer_many import _assert_same_outputs
    for name in names:
        _assert_same_outputs(ours / name, theirs / name)


def _assert_barcode_tables(pooled, out, min_units=1):
    rows = [line.split('\t') for line in (out / 'barcodes.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == pooled['whitelist'] and [row[1] for row in rows] == pooled['names']
    assert [int(row[2]) for row in rows] == pooled['cell_units'].tolist()
    assert [int(row[3]) for row in rows] == [int(n >= min_units) for n in pooled['cell_units']]
    summary = json.loads((out / 'barcodes.json').read_text())
    assert [summary[k] for k in ('exact', 'corrected', 'ambiguous', 'no_match', 'unreadable')] == pooled['stats'].tolist()
    assert summary['units'] == pooled['stats'].sum() == sum(CELL_PAIRS)
    assert summary['cells'] == sum(int(n >= min_units) for n in pooled['cell_units'])


def test_pooled_run_writes_the_files_of_the_per_cell_run(pooled, per_cell, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    monkeypatch.delenv('SKM_SET_QUANT_SERIAL', raising=False)
    out = _pooled_run(pooled, pooled['folder'] / 'demux')
    kept = [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'])]
    _assert_same_folders(out, per_cell, kept)
    assert (out / 'samples.tsv').read_bytes() == (per_cell / 'samples.tsv').read_bytes()
    _assert_barcode_tables(pooled, out)
    assert not (out / 'cell3').exists() and len(kept) == 5
    assert sorted(p.name for p in out.iterdir()) == sorted(kept + ['samples.tsv', 'barcodes.tsv', 'barcodes.json'])


def test_cells_spread_over_many_chunks(pooled, per_cell, monkeypatch):
    monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', '1000')
    out = _pooled_run(pooled, pooled['folder'] / 'demux_chunks')
    _assert_same_folders(out, per_cell, [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'])])
    assert (out / 'samples.tsv').read_bytes() == (per_cell / 'samples.tsv').read_bytes()
    _assert_barcode_tables(pooled, out)


def test_serial_set_quantification(pooled, per_cell, monkeypatch):
    monkeypatch.setenv('SKM_SET_QUANT_SERIAL', '1')
    out = _pooled_run(pooled, pooled['folder'] / 'demux_serial')
    _assert_same_folders(out, per_cell, [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'])])
    assert (out / 'samples.tsv').read_bytes() == (per_cell / 'samples.tsv').read_bytes()


def test_min_units_drops_the_smallest_cell(pooled, per_cell):
    smallest = int(np.argmin(np.where(pooled['cell_units'] > 0, pooled['cell_units'], 1 << 60)))
    min_units = int(pooled['cell_units'][smallest]) + 1
    out = _pooled_run(pooled, pooled['folder'] / 'demux_min_units', extra=['--min-units', str(min_units)])
    kept = [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'] >= min_units)]
    assert len(kept) == 4 and pooled['names'][smallest] not in kept
    _assert_same_folders(out, per_cell, kept)
    assert not (out / pooled['names'][smallest]).exists() and not (out / 'cell3').exists()
    lines = (per_cell / 'samples.tsv').read_text().splitlines(keepends=True)
    assert (out / 'samples.tsv').read_text() == ''.join(line for line in lines if line.split('\t')[0] in kept)
    _assert_barcode_tables(pooled, out, min_units)


def test_with_bias(pooled):
    theirs = _per_cell_run(pooled, pooled['folder'] / 'per_cell_bias', extra=['--bias'])
    out = _pooled_run(pooled, pooled['folder'] / 'demux_bias', extra=['--bias'])
    _assert_same_folders(out, theirs, [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'])])
    assert (out / 'samples.tsv').read_bytes() == (theirs / 'samples.tsv').read_bytes()


def test_single_ended(pooled):
    theirs = _per_cell_run(pooled, pooled['folder'] / 'per_cell_single', single=True)
    out = _pooled_run(pooled, pooled['folder'] / 'demux_single', single=True)
    _assert_same_folders(out, theirs, [pooled['names'][c] for c in np.flatnonzero(pooled['cell_units'])])
    assert (out / 'samples.tsv').read_bytes() == (theirs / 'samples.tsv').read_bytes()
    _assert_barcode_tables(pooled, out)


def test_a_surplus_of_records_is_dropped(pooled, tmp_path):
    """the run is min(records) units over the three files, as zip of the reference's feeders"""
    from seekmer_amd import common, mapper
    folder, n_units = pooled['folder'], 5000
    lines = (folder / 'pool_2.fastq').read_text().splitlines(keepends=True)
    (tmp_path / 'short_2.fastq').write_text(''.join(lines[:4 * n_units]))
    barcodes = (folder / 'barcodes.fastq').read_text().splitlines()[1::4]
    cell, cell_units, stats = ref.assign(pooled['whitelist'], barcodes[:n_units], start=3, mismatches=1)
    index = common.KMerIndex.load(pooled['index'])
    table = mapper.BarcodeTable.from_file(folder / 'whitelist.tsv')
    sample_set, kept, demux = mapper.map_barcoded(
        index, table, common.PackedReadFeeder([folder / 'barcodes.fastq'], paired=False),
        common.PackedReadFeeder([folder / 'pool_1.fastq', tmp_path / 'short_2.fastq'], paired=True), True, start=3)
    assert demux['records'] == [sum(CELL_PAIRS), sum(CELL_PAIRS), n_units] and demux['units'] == n_units
    assert [demux[k] for k in mapper.BARCODE_STATS] == stats.tolist() and stats.sum() == n_units
    np.testing.assert_array_equal(kept, np.flatnonzero(cell_units))
    np.testing.assert_array_equal(demux['cell_units'], cell_units)
    np.testing.assert_array_equal(sample_set.sizes()[:, 3], cell_units[kept])
