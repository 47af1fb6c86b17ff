"""Cell discovery on the GPU: BarcodeCensus against tests/discover_reference.py, exactly -- the census is the
Counter's multiset, the ranking its sorted order, the pick the reference's --, and `infer-many --discover-cells` on a
pooled run against the reference's list and against `infer-many --barcodes` on the list it wrote (cell folders as
tests/test_gpu_infer_many.py compares folders: abundance.tsv byte for byte, run_info.json and abundance.npz equal
but for the start time and the call; samples.tsv and barcodes.tsv byte for byte)."""
import ctypes
import json

import numpy as np
import pytest

import barcode_reference
import discover_reference as ref
from test_discover_host import HAND_CASES
from test_gpu_barcodes import BASES, _piece, _random_barcodes, _substitute, _write_fastq

pytestmark = pytest.mark.gpu

N_READS = 5000


def _text(rng, k):
    return ''.join(rng.choice(list(BASES), size=k))


def _census_reads(rng, pool, length, start, n, ragged=True):
    """n barcode reads around a pool of barcodes (a few of them frequent): clean windows, every kind of damage inside
    and outside the window, and -- ragged -- every kind of length"""
    weights = 1.0 / np.arange(1, len(pool) + 1)
    weights /= weights.sum()
    reads = []
    kinds = rng.choice(9, size=n, p=[.5, .1, .08, .08, .08, .05, .05, .03, .03])
    for kind in kinds:
        window = pool[rng.choice(len(pool), p=weights)]
        prefix, suffix = _text(rng, start), _text(rng, rng.integers(0, 11) if ragged else 4)
        if kind == 1:
            window = _text(rng, length)
        elif kind == 2:
            p = rng.integers(length)
            window = window[:p] + 'N' + window[p + 1:]
        elif kind == 3:
            p = rng.integers(length)
            window = window[:p] + window[p].lower() + window[p + 1:]
        elif kind == 4:           # a base that is not clean just outside the window: it must not matter
            if start and rng.random() < 0.5:
                prefix = prefix[:-1] + 'N'
            else:
                suffix = 'n' + suffix[1:] if not ragged else 'n' + suffix
        elif kind == 5 and ragged:
            suffix, window = '', window[:-1]                            # start + L - 1 bases
        elif kind == 6 and ragged:
            suffix = ''                                                  # start + L bases
        elif kind == 7 and ragged:
            prefix = window = suffix = ''                                # no bases at all
        elif kind == 8 and length >= 2:
            window = 'N' + window[1:-1] + 'n'
        reads.append(prefix + window + suffix)
    return reads


SHAPES = [(length, start) for length in (1, 5, 16, 31, 32) for start in (0, 3, 20)]
CASES = ['L%d_start%d' % shape for shape in SHAPES] + ['uniform_L16_start20', 'uniform_L32_start3', 'uniform_all_short',
                                                        'one_barcode', 'all_distinct', 'extremes_start0', 'extremes_start3']


def _case(name):
    """(length, start, reads) of a census case"""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith('L'):
        length, start = (int(part.lstrip('Lstar')) for part in name.split('_'))
        pool = _random_barcodes(rng, min(300, 4 ** length), length)
        return length, start, _census_reads(rng, pool, length, start, N_READS)
    if name.startswith('uniform_L'):
        length, start = (int(part.lstrip('Lstar')) for part in name.split('_')[1:])
        pool = _random_barcodes(rng, 300, length)
        reads = _census_reads(rng, pool, length, start, N_READS, ragged=False)
        assert len(set(map(len, reads))) == 1
        return length, start, reads
    if name == 'uniform_all_short':
        return 16, 3, [_text(rng, 18) for _ in range(1000)]             # start + L - 1 bases, every one of them
    if name == 'one_barcode':                                            # every unit to ONE counter
        return 12, 3, ['GGA' + 'ACGTTGCAACGT' + 'TT'] * N_READS
    if name == 'all_distinct':                                           # more keys than a block's LDS table holds
        return 16, 0, _random_barcodes(rng, N_READS, 16)
    length, start = 32, int(name[-1])
    pool = ['A' * 32, 'T' * 32, 'T' * 31 + 'G', 'A' * 31 + 'C', 'C' + 'T' * 31, 'T' * 16 + 'A' * 16] + _random_barcodes(rng, 50, 32)
    return length, start, _census_reads(rng, pool, length, start, N_READS)


@pytest.fixture(scope='module')
def cases():
    """every case with the reference's census, computed once"""
    out = {}
    for name in CASES:
        length, start, reads = _case(name)
        out[name] = (length, start, reads) + ref.census(reads, length, start)
    return out


def test_the_cases_are_not_trivial(cases):
    """the reference alone: a device answer of 'nothing counted' or 'everything counted' cannot pass"""
    for name, (length, start, reads, counts, stats) in cases.items():
        assert sum(stats) == len(reads) and sum(counts.values()) == stats[0]
        if name.startswith('L') and length > 1:
            assert stats[0] > 0.5 * len(reads) and stats[1] > 0 and stats[2] > 0, (name, stats)
        if name.startswith('uniform_L'):
            assert stats[0] > 0.5 * len(reads) and stats[1] == 0 and stats[2] > 0, (name, stats)
    assert len(cases['L16_start0'][3]) > 300 and len(cases['L1_start3'][3]) <= 4
    assert cases['uniform_all_short'][4] == [0, 1000, 0]
    assert cases['one_barcode'][3] == {'ACGTTGCAACGT': N_READS}
    assert len(cases['all_distinct'][3]) == N_READS
    for name in ('extremes_start0', 'extremes_start3'):
        assert cases[name][3]['A' * 32] > 100 and cases[name][3]['T' * 32] > 100


def _census_of(reads, length, start, n_pieces):
    from seekmer_amd import mapper
    census = mapper.BarcodeCensus(length)
    bounds = np.linspace(0, len(reads), n_pieces + 1).astype(int)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        census.add(_piece(reads[lo:hi], stride_extra=(lo % 3 if hi > lo else 0)), start=start)
    return census


@pytest.mark.parametrize('slots', [None, '2'])
@pytest.mark.parametrize('name', CASES)
def test_the_census_is_the_counter(native_libs, cases, name, slots, monkeypatch):
    if slots is None:
        monkeypatch.delenv('SKM_TEST_CENSUS_SLOTS', raising=False)
    else:
        monkeypatch.setenv('SKM_TEST_CENSUS_SLOTS', slots)             # a table that has to grow under the launches
    length, start, reads, counts, stats = cases[name]
    want = ref.ranked(counts)
    for n_pieces in (1, 3, 50):
        census = _census_of(reads, length, start, n_pieces)
        barcodes, numbers = census.ranked()
        print(name, slots, n_pieces, 'stats', census.stats.tolist(), 'distinct', len(census))
        assert census.stats.tolist() == stats
        assert len(census) == len(counts)
        assert list(zip(barcodes, numbers.tolist())) == want
        head, head_numbers = census.ranked(limit=7)
        assert list(zip(head, head_numbers.tolist())) == want[:7]


def _without_lengths(piece):
    """a piece of reads of one length as a reader hands it out: no lengths array, only uniform_len"""
    from seekmer_amd import _native
    from seekmer_amd.common import PackedReads
    assert piece.raw.uniform_len >= 0 and piece.n_reads > 0
    raw = _native.PackedReads()
    ctypes.memmove(ctypes.byref(raw), ctypes.byref(piece.raw), ctypes.sizeof(raw))
    raw.lengths = None
    return PackedReads(raw, keep=piece)          # (the arrays live as long as the piece they belong to)


@pytest.mark.parametrize('name', ['uniform_L16_start20', 'uniform_L32_start3', 'uniform_all_short'])
def test_a_piece_without_a_lengths_array(native_libs, cases, name, monkeypatch):
    """uniform_len alone says how long the reads are: the window inside it, and -- every read short -- past it"""
    from seekmer_amd import mapper
    monkeypatch.delenv('SKM_TEST_CENSUS_SLOTS', raising=False)
    length, start, reads, counts, stats = cases[name]
    census = mapper.BarcodeCensus(length)
    for lo in range(0, len(reads), 1700):
        census.add(_without_lengths(_piece(reads[lo:lo + 1700])), start=start)
    barcodes, numbers = census.ranked()
    assert census.stats.tolist() == stats and list(zip(barcodes, numbers.tolist())) == ref.ranked(counts)
    # the same reads, the window one base past their end: every one of them is short
    past = mapper.BarcodeCensus(length)
    past.add(_without_lengths(_piece(reads[:1700])), start=len(reads[0]) - length + 1)
    assert past.stats.tolist() == [0, min(1700, len(reads)), 0] and len(past) == 0
    # and ending exactly at their end: none is
    if len(reads[0]) >= length:
        edge = mapper.BarcodeCensus(length)
        edge.add(_without_lengths(_piece(reads[:1700])), start=len(reads[0]) - length)
        want, want_stats = ref.census(reads[:1700], length, len(reads[0]) - length)
        assert edge.stats.tolist() == want_stats and want_stats[1] == 0
        got, got_numbers = edge.ranked()
        assert list(zip(got, got_numbers.tolist())) == ref.ranked(want)


def test_an_empty_piece_and_an_empty_census(native_libs, cases):
    from seekmer_amd import mapper
    census = mapper.BarcodeCensus(16)
    barcodes, numbers = census.ranked()
    assert len(census) == 0 and barcodes == [] and numbers.size == 0
    census.add(_piece([]), start=3)
    assert len(census) == 0 and census.stats.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match='no readable barcode'):
        census.pick(10)
    info = np.zeros(6, dtype=np.int64)
    keys, counts = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.int64)
    code = native_libs.hip().skm_barcode_census_pick(census._handle, 10, 1, 4, native_libs.ptr(keys, native_libs.c_u64p),
                                                     native_libs.ptr(counts, native_libs.c_i64p), native_libs.ptr(info, native_libs.c_i64p))
    assert code == native_libs.SKM_ERR_STATE and b'no readable barcode' in native_libs.hip().skm_last_error()
    length, start, reads, want, stats = cases['L16_start3']            # the handle is as good as new
    census.add(_piece(reads), start=start)
    census.add(_piece([]), start=start)
    barcodes, numbers = census.ranked()
    assert list(zip(barcodes, numbers.tolist())) == ref.ranked(want) and census.stats.tolist() == stats


# ---- the pick -----------------------------------------------------------------------------------------------------
def _reads_of(counts, rng):
    reads = [barcode for barcode, n in counts.items() for _ in range(n)]
    return [reads[i] for i in rng.permutation(len(reads))]


def _random_census(rng):
    """about 3 000 distinct 8-mers: 300 cells, each with a few misreadings at distance 1, and ambient barcodes"""
    counts = {}
    for cell in _random_barcodes(rng, 300, 8):
        counts[cell] = int(rng.integers(20, 300))
        for _ in range(rng.integers(2, 9)):
            counts.setdefault(_substitute(rng, cell, 1), int(rng.integers(1, 40)))
    for barcode in _random_barcodes(rng, 1300, 8):
        counts.setdefault(barcode, int(rng.integers(1, 4)))
    return counts


EXTREMES = {'T' * 32: 500, 'T' * 31 + 'G': 100, 'A' * 32: 400, 'A' * 31 + 'C': 450, 'C' + 'T' * 31: 600, 'G' * 32: 70}


@pytest.fixture(scope='module')
def pick_cases():
    out = dict(HAND_CASES, extremes=EXTREMES, random=_random_census(np.random.default_rng(8)))
    assert 2500 < len(out['random']) < 3500
    for drop in (True, False):                   # the random census: neighbours are dropped, and not all of them
        _, _, info = ref.pick(out['random'], 300, drop)
        assert info['candidates'] > 300 and (info['dropped'] > 50) == drop and info['picked'] > 200
    return out


@pytest.mark.parametrize('slots', [None, '2'])
@pytest.mark.parametrize('name', list(HAND_CASES) + ['extremes', 'random'])
def test_pick_is_the_reference(native_libs, pick_cases, name, slots, monkeypatch):
    if slots is None:
        monkeypatch.delenv('SKM_TEST_CENSUS_SLOTS', raising=False)
    else:
        monkeypatch.setenv('SKM_TEST_CENSUS_SLOTS', slots)
    counts = pick_cases[name]
    length = len(next(iter(counts)))
    rng = np.random.default_rng(5)
    census = _census_of(_reads_of(counts, rng), length, 0, 3)
    assert len(census) == len(counts)
    for expect_cells in (1, 100, 101, 300, 3000, 10 ** 6):
        for drop in (True, False):
            picked, _, info = ref.pick(counts, expect_cells, drop)
            barcodes, numbers, got = census.pick(expect_cells, drop_neighbours=drop)
            print(name, expect_cells, drop, got)
            assert got == info
            assert list(zip(barcodes, numbers.tolist())) == picked


def test_a_cap_too_small_leaves_the_handle_usable(native_libs, pick_cases):
    hip = native_libs.hip()
    counts = pick_cases['shadow']
    census = _census_of(_reads_of(counts, np.random.default_rng(1)), 8, 0, 1)
    info = np.zeros(6, dtype=np.int64)
    keys, numbers = np.full(4, 7, dtype=np.uint64), np.full(4, 7, dtype=np.int64)
    call = lambda cap: hip.skm_barcode_census_pick(census._handle, 1, 1, cap, native_libs.ptr(keys, native_libs.c_u64p),
                                                   native_libs.ptr(numbers, native_libs.c_i64p), native_libs.ptr(info, native_libs.c_i64p))
    assert call(1) == native_libs.SKM_ERR_STATE
    assert info.tolist() == [1, 1000, 100, 3, 1, 2] and keys.tolist() == [7] * 4          # info is filled, nothing copied
    assert call(2) == 0 and numbers.tolist() == [1000, 900, 7, 7]
    picked, _, want = ref.pick(counts, 1)
    barcodes, got_numbers, got = census.pick(1)
    assert got == want and list(zip(barcodes, got_numbers.tolist())) == picked


def test_refusals(native_libs):
    from seekmer_amd import mapper
    hip = native_libs.hip()
    handle = ctypes.c_void_p()
    for length in (0, 33, -1):
        assert hip.skm_barcode_census_create(0, length, ctypes.byref(handle)) == native_libs.SKM_ERR_ARG
        assert not handle
        with pytest.raises(ValueError, match='1 to 32'):
            mapper.BarcodeCensus(length)
    census = mapper.BarcodeCensus(4)
    census.add(_piece(['ACGT', 'ACGT', 'TTTT']))
    with pytest.raises(ValueError, match='1 at least'):
        census.pick(0)
    info = np.zeros(6, dtype=np.int64)
    keys, numbers = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.int64)
    assert hip.skm_barcode_census_pick(census._handle, 0, 1, 4, native_libs.ptr(keys, native_libs.c_u64p),
                                       native_libs.ptr(numbers, native_libs.c_i64p),
                                       native_libs.ptr(info, native_libs.c_i64p)) == native_libs.SKM_ERR_ARG
    with pytest.raises(ValueError, match='starts at base'):
        census.add(_piece(['ACGT']), start=-1)
    assert census.pick(1)[0] == ['ACGT', 'TTTT'] and census.stats.tolist() == [3, 0, 0]      # (m = 2: the threshold is 1)


def test_the_slots_hook_is_checked(native_libs, monkeypatch):
    from seekmer_amd import mapper
    for bad in ('1', '3', '0', 'many'):
        monkeypatch.setenv('SKM_TEST_CENSUS_SLOTS', bad)
        with pytest.raises(ValueError, match='SKM_TEST_CENSUS_SLOTS'):
            mapper.BarcodeCensus(8)


# ---- end to end ---------------------------------------------------------------------------------------------------
READ_LEN = 75
LENGTH, START, UMI_LENGTH = 12, 3, 6
CELL_UNITS = (2900, 400, 2100, 650, 1500, 1200, 900, 2500, 500, 1800, 750, 1000)
SHADOW_UNITS, AMBIENT_UNITS = 350, 200


@pytest.fixture(scope='module')
def pooled(native_libs, tmp_path_factory):
    """The index of synth.transcriptome(5, 30) and one pooled run: twelve cells (barcodes at distance >= 3 from each
    other) of 400 to 2 900 pairs, 3 % of the barcodes with one substitution, a few with an N, a few reads too short;
    200 pairs under ambient random barcodes; 350 pairs under a shadow one substitution away from the largest cell.
    A barcode read is GGA, the barcode, a UMI of six bases, a tail."""
    from seekmer_amd import index_builder, synth
    folder = tmp_path_factory.mktemp('discover')
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    index_path = folder / 'index.npz'
    index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    rng = np.random.default_rng(2025)
    while True:
        cells = _random_barcodes(rng, len(CELL_UNITS), LENGTH)
        if all(sum(a != b for a, b in zip(x, y)) >= 3 for i, x in enumerate(cells) for y in cells[:i]):
            break
    shadow = _substitute(rng, cells[0], 1)
    owners = [c for c, n in enumerate(CELL_UNITS) for _ in range(n)] + [-1] * SHADOW_UNITS + [-2] * AMBIENT_UNITS
    owners = [owners[i] for i in rng.permutation(len(owners))]
    raw = synth.reads(101, pool, tx_offsets, 0, len(owners), READ_LEN, True)[0][:-1].tobytes().decode()
    mates = [[raw[(2 * u + mate) * READ_LEN:(2 * u + mate + 1) * READ_LEN] for u in range(len(owners))] for mate in (0, 1)]
    barcodes = []
    for owner in owners:
        barcode = shadow if owner == -1 else _text(rng, LENGTH) if owner == -2 else cells[owner]
        chance = rng.random()
        if chance < 0.03:
            barcode = _substitute(rng, barcode, 1)
        elif chance < 0.035:
            p = rng.integers(LENGTH)
            barcode = barcode[:p] + 'N' + barcode[p + 1:]
        read = 'GGA' + barcode + _text(rng, UMI_LENGTH) + _text(rng, 4)
        barcodes.append(read[:rng.integers(2, START + LENGTH)] if 0.035 <= chance < 0.04 else read)
    _write_fastq(folder / 'pool_1.fastq', mates[0])
    _write_fastq(folder / 'pool_2.fastq', mates[1])
    _write_fastq(folder / 'barcodes.fastq', barcodes)
    return dict(folder=folder, index=index_path, cells=cells, shadow=shadow, barcodes=barcodes)


def _run(pooled, out, extra):
    from seekmer_amd.__main__ import main
    folder = pooled['folder']
    assert main(['infer-many', str(pooled['index']), str(out), str(folder / 'pool_1.fastq'), str(folder / 'pool_2.fastq'),
                 '-b', '2', '--seed', '7', '--barcode-file', str(folder / 'barcodes.fastq'), '--barcode-start', str(START),
                 *extra]) == 0
    return out


DISCOVER = ['--discover-cells', '12', '--barcode-length', str(LENGTH)]


def _assert_same_runs(ours, theirs, names):
    from test_gpu_infer_many import _assert_same_outputs
    for name in names:
        _assert_same_outputs(ours / name, theirs / name)
    assert (ours / 'samples.tsv').read_bytes() == (theirs / 'samples.tsv').read_bytes()
    assert (ours / 'barcodes.tsv').read_bytes() == (theirs / 'barcodes.tsv').read_bytes()
    mine, other = json.loads((ours / 'barcodes.json').read_text()), json.loads((theirs / 'barcodes.json').read_text())
    assert 'discovery' in mine and 'discovery' not in other
    del mine['discovery']
    assert mine == other
    extra = {'barcodes.discovered.txt', 'barcodes.census.tsv'}
    assert {p.name for p in ours.iterdir()} - extra == {p.name for p in theirs.iterdir()} == set(names) | {'samples.tsv', 'barcodes.tsv', 'barcodes.json'}


def _assert_discovery(pooled, out, keep_neighbours):
    picked, candidates, info = ref.discover(pooled['barcodes'], LENGTH, 12, start=START, drop_neighbours=not keep_neighbours)
    lines = (out / 'barcodes.discovered.txt').read_text().splitlines()
    assert [line for line in lines if not line.startswith('#')] == [barcode for barcode, _ in picked]
    assert lines[0].startswith('#') and not any(line.startswith('#') for line in lines[3:])
    rows = [line.split('\t') for line in (out / 'barcodes.census.tsv').read_text().splitlines()]
    assert [(b, int(n), int(flag)) for b, n, flag in rows] == candidates
    assert json.loads((out / 'barcodes.json').read_text())['discovery'] == dict(
        expect_cells=12, barcode_length=LENGTH, units_counted=info['counted'], short=info['short'], unreadable=info['unreadable'],
        distinct=info['distinct'], rank=info['rank'], rank_count=info['rank_count'], threshold=info['threshold'],
        candidates=info['candidates'], dropped_neighbours=info['dropped'], picked=info['picked'], keep_neighbours=keep_neighbours)
    return [barcode for barcode, _ in picked], info


def test_the_pooled_run_is_what_the_issue_describes(pooled):
    """the reference alone"""
    picked, candidates, info = ref.discover(pooled['barcodes'], LENGTH, 12, start=START)
    assert info['rank'] == 1 and 2700 < info['rank_count'] <= 2900 and info['threshold'] == (info['rank_count'] + 9) // 10
    assert info['candidates'] == 13 and info['dropped'] == 1 and info['short'] > 0 and info['unreadable'] > 0
    assert sorted(b for b, _ in picked) == sorted(pooled['cells']) and picked[0][0] == pooled['cells'][0]
    assert [b for b, _, flag in candidates if not flag] == [pooled['shadow']]


def test_discovery_finds_the_cells_and_runs_as_the_whitelist_does(pooled, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    monkeypatch.delenv('SKM_TEST_CENSUS_SLOTS', raising=False)
    folder = pooled['folder']
    out = _run(pooled, folder / 'discover', DISCOVER)
    picked, info = _assert_discovery(pooled, out, False)
    assert len(picked) == 12 and pooled['shadow'] not in picked
    theirs = _run(pooled, folder / 'whitelist', ['--barcodes', str(out / 'barcodes.discovered.txt')])
    _assert_same_runs(out, theirs, picked)
    # the shadow's units have come back to the largest cell through the 1-mismatch correction
    cell, cell_units, stats = barcode_reference.assign(picked, pooled['barcodes'], start=START, mismatches=1)
    rows = [line.split('\t') for line in (out / 'barcodes.tsv').read_text().splitlines()]
    assert [int(row[2]) for row in rows] == cell_units.tolist() and cell_units[0] > CELL_UNITS[0] + 200


def test_keep_neighbours_makes_the_shadow_a_cell(pooled, monkeypatch):
    monkeypatch.delenv('SKM_TEST_CENSUS_SLOTS', raising=False)
    out = _run(pooled, pooled['folder'] / 'discover_keep', DISCOVER + ['--discover-keep-neighbours'])
    picked, info = _assert_discovery(pooled, out, True)
    assert len(picked) == 13 and pooled['shadow'] in picked
    cell, cell_units, stats = barcode_reference.assign(picked, pooled['barcodes'], start=START, mismatches=1)
    rows = [line.split('\t') for line in (out / 'barcodes.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == picked and [int(row[2]) for row in rows] == cell_units.tolist()
    assert cell_units[0] < CELL_UNITS[0] and cell_units[picked.index(pooled['shadow'])] > 300       # no longer corrected
    assert (out / pooled['shadow'] / 'abundance.tsv').exists()


def test_with_umis_many_chunks_and_a_table_that_grows(pooled, monkeypatch):
    monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', '1000')
    monkeypatch.setenv('SKM_TEST_CENSUS_SLOTS', '2')
    folder = pooled['folder']
    umis = ['--umi-length', str(UMI_LENGTH), '--umi-start', str(START + LENGTH)]
    out = _run(pooled, folder / 'discover_umi', DISCOVER + umis)
    picked, info = _assert_discovery(pooled, out, False)
    theirs = _run(pooled, folder / 'whitelist_umi', ['--barcodes', str(out / 'barcodes.discovered.txt')] + umis)
    _assert_same_runs(out, theirs, picked)
