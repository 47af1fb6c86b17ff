"""Cell discovery without a GPU: the rule of tests/discover_reference.py on hand-written censuses, and the
combinations of options that `infer-many --discover-cells` takes and refuses, on the command line and in run_many."""
import pytest

import discover_reference as ref


def _barcodes(picked):
    return [barcode for barcode, _ in picked]


# ---- the rule -----------------------------------------------------------------------------------------------------
def test_census_counts_clean_windows_only():
    reads = ['GGACGTTT', 'GGACGT', 'GGACG', 'GGACNT', 'GGAcGT', 'NGACGTN', 'GGTTTT', '']
    counts, stats = ref.census(reads, 4, start=2)
    assert counts == {'ACGT': 3, 'TTTT': 1}              # (an N outside the window does not matter)
    assert stats == [4, 2, 2] and sum(stats) == len(reads)


def test_ties_are_broken_by_key():
    counts = {'TTTT': 5, 'AAAA': 5, 'CCCC': 7, 'GGGG': 5, 'ACGT': 1}
    assert ref.ranked(counts) == [('CCCC', 7), ('AAAA', 5), ('GGGG', 5), ('TTTT', 5), ('ACGT', 1)]


@pytest.mark.parametrize('expect_cells, rank, m', [(1, 1, 1000), (100, 1, 1000), (101, 2, 500), (200, 2, 500), (201, 3, 40)])
def test_the_rank_is_a_hundredth_rounded_up(expect_cells, rank, m):
    counts = {'AAAA': 1000, 'CCCC': 500, 'GGGG': 40, 'TTTT': 4}
    _, _, info = ref.pick(counts, expect_cells)
    assert (info['rank'], info['rank_count'], info['threshold']) == (rank, m, (m + 9) // 10)


def test_a_rank_beyond_the_census_is_its_last_entry():
    counts = {'AAAA': 1000, 'CCCC': 500, 'GGGG': 40}
    picked, _, info = ref.pick(counts, 1000)             # r = 10 > D = 3
    assert (info['rank'], info['rank_count'], info['threshold']) == (3, 40, 4) and len(picked) == 3


@pytest.mark.parametrize('m, threshold', [(10, 1), (11, 2), (1, 1), (20, 2), (21, 3)])
def test_the_threshold_rounds_up(m, threshold):
    counts = {'AAAA': m, 'CCCC': 2, 'GGGG': 1}
    picked, candidates, info = ref.pick(counts, 1)
    assert info['threshold'] == threshold
    assert _barcodes(picked) == [b for b, n in ref.ranked(counts) if n >= threshold]


SHADOW = {'ACGTACGT': 1000, 'ACGTACGA': 120, 'TTGGCCAA': 900, 'GGGGCCCC': 99}


def test_a_shadow_at_distance_one_is_dropped():
    picked, candidates, info = ref.pick(SHADOW, 1)
    assert info['threshold'] == 100
    assert candidates == [('ACGTACGT', 1000, 1), ('TTGGCCAA', 900, 1), ('ACGTACGA', 120, 0)]
    assert _barcodes(picked) == ['ACGTACGT', 'TTGGCCAA']
    assert (info['candidates'], info['dropped'], info['picked']) == (3, 1, 2)


def test_keep_neighbours_keeps_the_shadow():
    picked, candidates, info = ref.pick(SHADOW, 1, drop_neighbours=False)
    assert _barcodes(picked) == ['ACGTACGT', 'TTGGCCAA', 'ACGTACGA'] and info['dropped'] == 0
    assert all(flag == 1 for _, _, flag in candidates)


# AAAA > AAAC > AACC in count; AAAC is dropped by AAAA, and AACC -- two away from AAAA -- by the dropped AAAC
CHAIN = {'AAAA': 1000, 'AAAC': 500, 'AACC': 400, 'GGGG': 300}


def test_a_dropped_candidate_still_drops_its_neighbour():
    picked, candidates, info = ref.pick(CHAIN, 1)
    assert _barcodes(picked) == ['AAAA', 'GGGG']
    assert candidates == [('AAAA', 1000, 1), ('AAAC', 500, 0), ('AACC', 400, 0), ('GGGG', 300, 1)]


def test_of_two_equal_neighbours_the_smaller_key_stays():
    picked, _, info = ref.pick({'ACGT': 50, 'ACGA': 50, 'TTTT': 50}, 1)
    assert _barcodes(picked) == ['ACGA', 'TTTT'] and info['dropped'] == 1


def test_a_neighbour_below_the_threshold_drops_nobody():
    picked, _, _ = ref.pick({'ACGT': 5, 'ACGA': 1000, 'ACGC': 99}, 1)        # ACGC is no candidate
    assert _barcodes(picked) == ['ACGA']


def test_no_readable_barcode_is_an_error():
    counts, stats = ref.census(['NNNN', 'ACGN', 'AC', 'acgt'], 4)
    assert not counts and stats == [0, 1, 3]
    with pytest.raises(ValueError, match='no readable barcode'):
        ref.pick(counts, 10)
    with pytest.raises(ValueError, match='no readable barcode'):
        ref.discover(['NNNN'], 4, 10)


HAND_CASES = {'shadow': SHADOW, 'chain': CHAIN, 'ties': {'TTTT': 5, 'AAAA': 5, 'CCCC': 7, 'GGGG': 5, 'ACGT': 1},
              'equal_neighbours': {'ACGT': 50, 'ACGA': 50, 'TTTT': 50}, 'below': {'ACGT': 5, 'ACGA': 1000, 'ACGC': 99},
              'ranks': {'AAAA': 1000, 'CCCC': 500, 'GGGG': 40, 'TTTT': 4}, 'm10': {'AAAA': 10, 'CCCC': 2, 'GGGG': 1},
              'm11': {'AAAA': 11, 'CCCC': 2, 'GGGG': 1}}


def test_discover_runs_the_census_and_the_pick():
    reads = [barcode for barcode, n in SHADOW.items() for _ in range(n)] + ['ACGTACGN', 'ACG']
    picked, candidates, info = ref.discover(reads, 8, 1)
    assert _barcodes(picked) == ['ACGTACGT', 'TTGGCCAA']
    assert (info['counted'], info['short'], info['unreadable'], info['distinct'], info['units']) == (2119, 1, 1, 4, 2121)


# ---- the command line ---------------------------------------------------------------------------------------------
DISCOVER = ['r1.fq', 'r2.fq', '--discover-cells', '500', '--barcode-length', '16', '--barcode-file', 'b.fq']


@pytest.mark.parametrize('arguments, message', [
    (['r1.fq', 'r2.fq', '--barcode-length', '16'], '--barcode-length goes with --discover-cells'),
    (['r1.fq', 'r2.fq', '--barcode-length', '0'], '--barcode-length goes with --discover-cells'),
    (['r1.fq', 'r2.fq', '--discover-keep-neighbours'], '--discover-keep-neighbours goes with --discover-cells'),
    (['r1.fq', 'r2.fq', '--barcode-file', 'b.fq'], '--barcode-file goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--barcode-start', '3'], '--barcode-start goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--barcode-mismatches', '0'], '--barcode-mismatches goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--min-units', '5'], '--min-units goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--umi-length', '8'], '--umi-length goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--discover-cells', '500', '--barcode-file', 'b.fq'], '--barcode-length'),
    (['r1.fq', 'r2.fq', '--discover-cells', '500', '--barcode-length', '16'], '--barcode-file'),
    (['r1.fq', 'r2.fq', '--discover-cells', '500', '--barcode-length', '0', '--barcode-file', 'b.fq'], '1 to 32'),
    (['r1.fq', 'r2.fq', '--discover-cells', '500', '--barcode-length', '33', '--barcode-file', 'b.fq'], '1 to 32'),
    (['r1.fq', 'r2.fq', '--discover-cells', '0', '--barcode-length', '16', '--barcode-file', 'b.fq'], '1 or more'),
    (DISCOVER + ['--barcodes', 'w.txt'], 'one of --barcodes and --discover-cells'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq', '--barcode-length', '16'], 'the whitelist gives the length'),
    (['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq', '--discover-keep-neighbours'],
     '--discover-keep-neighbours goes with --discover-cells'),
    (DISCOVER + ['--names', 'a,b'], '--names does not go with --discover-cells'),
    (['r3.fq', 'r4.fq'] + DISCOVER, 'ONE pooled sample'),
    (DISCOVER + ['-s'], 'ONE pooled sample'),
    (DISCOVER + ['--barcode-start', '-1'], '0 or more'),
    (DISCOVER + ['--barcode-mismatches', '2'], 'invalid choice'),
    (DISCOVER + ['--min-units', '0'], '1 or more'),
    (DISCOVER + ['--umi-length', '17'], '1 to 16'),
    (DISCOVER + ['--umi-start', '4'], '--umi-start goes with --umi-length'),
])
def test_the_command_line_refuses(arguments, message, capsys):
    from seekmer_amd.__main__ import parse_args
    with pytest.raises(SystemExit) as exit_:
        parse_args(['infer-many', 'index.npz', 'out'] + arguments)
    assert exit_.value.code == 2 and message in capsys.readouterr().err


def test_the_command_line_accepts():
    from seekmer_amd.__main__ import parse_args
    opts = parse_args(['infer-many', 'index.npz', 'out'] + DISCOVER)
    assert (opts['discover_cells'], opts['barcode_length'], opts['discover_keep_neighbours']) == (500, 16, False)
    assert opts['barcodes'] is None and (opts['barcode_start'], opts['barcode_mismatches'], opts['min_units']) == (0, 1, 1)
    opts = parse_args(['infer-many', 'index.npz', 'out', 'r.fq', '-s', '--discover-cells', '1', '--barcode-length', '32',
                       '--barcode-file', 'b.fq', '--discover-keep-neighbours', '--barcode-start', '6', '--barcode-mismatches',
                       '0', '--min-units', '50', '--umi-length', '10', '--umi-start', '38', '--bias', '--genes'])
    assert (opts['discover_cells'], opts['barcode_length'], opts['discover_keep_neighbours']) == (1, 32, True)
    assert (opts['barcode_start'], opts['barcode_mismatches'], opts['min_units'], opts['umi_length']) == (6, 0, 50, 10)
    opts = parse_args(['infer-many', 'index.npz', 'out', 'a.fq', 'b.fq', 'c.fq', 'd.fq'])      # (as ever)
    assert opts['discover_cells'] is None and opts['barcode_length'] is None and opts['discover_keep_neighbours'] is False


@pytest.mark.parametrize('command', ['infer', 'impute'])
@pytest.mark.parametrize('option', [['--discover-cells', '500'], ['--barcode-length', '16'], ['--discover-keep-neighbours']])
def test_the_other_commands_do_not_take_the_options(command, option, capsys):
    from seekmer_amd.__main__ import parse_args
    with pytest.raises(SystemExit) as exit_:
        parse_args([command, 'index.npz', 'out', 'r1.fq', 'r2.fq'] + option)
    assert exit_.value.code == 2 and 'unrecognized arguments' in capsys.readouterr().err


# ---- run_many -----------------------------------------------------------------------------------------------------
def test_run_many_refuses_what_the_command_line_does(tmp_path, monkeypatch):
    from seekmer_amd import infer
    white = tmp_path / 'w.txt'
    white.write_text('ACGT\n')
    reads = [tmp_path / 'r1.fastq', tmp_path / 'r2.fastq']                  # (they do not exist: nothing gets that far)
    barcode_file = tmp_path / 'b.fastq'
    call = lambda paths=reads, single=False, **k: infer.run_many(tmp_path / 'i.npz', tmp_path / 'out', paths, 1, single, 0, False, **k)
    found = dict(discover_cells=500, barcode_length=16, barcode_file=barcode_file)
    for message, options in (
            ('--barcode-length goes with --discover-cells', dict(barcode_length=16)),
            ('--discover-keep-neighbours goes with --discover-cells', dict(discover_keep_neighbours=True)),
            ('--barcode-file goes with --barcodes', dict(barcode_file=barcode_file)),
            ('go with --barcodes', dict(umi_length=8)),
            ('one of --barcodes and --discover-cells', dict(found, barcodes=white)),
            ('the whitelist gives the length', dict(barcodes=white, barcode_file=barcode_file, barcode_length=4)),
            ('--discover-keep-neighbours goes with --discover-cells',
             dict(barcodes=white, barcode_file=barcode_file, discover_keep_neighbours=True)),
            ('--barcode-length', dict(discover_cells=500, barcode_file=barcode_file)),
            ('--barcode-file', dict(discover_cells=500, barcode_length=16)),
            ('1 to 32', dict(found, barcode_length=0)),
            ('1 to 32', dict(found, barcode_length=33)),
            ('1 or more', dict(found, discover_cells=0)),
            ('--names does not go with --discover-cells', dict(found, names='a,b')),
            ('0 or more', dict(found, barcode_start=-1)),
            ('0 or 1', dict(found, barcode_mismatches=2)),
            ('1 or more', dict(found, min_units=0)),
            ('1 to 16', dict(found, umi_length=17)),
            ('--umi-start goes with --umi-length', dict(found, umi_start=3))):
        with pytest.raises(ValueError, match=message):
            call(**options)
        assert not (tmp_path / 'out').exists(), options
    with pytest.raises(ValueError, match='ONE pooled sample'):
        call(paths=reads + reads, **found)
    with pytest.raises(ValueError, match='ONE pooled sample'):
        call(single=True, **found)
    # several ranks, a read file that is not there, a compressed one: before the output folder is made
    from seekmer_amd import parallel

    class TwoRanks:
        world, closed = 2, False

        def close(self):
            TwoRanks.closed = True

    with monkeypatch.context() as patch:         # (what Ranks.from_env gives a process that a launcher started)
        patch.setattr(parallel.Ranks, 'from_env', classmethod(lambda cls, *a, **k: TwoRanks()))
        with pytest.raises(ValueError, match='one process on one GPU'):
            call(**found)
    assert TwoRanks.closed and not (tmp_path / 'out').exists()
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match='invalid FastQ file'):
        call(**found)
    for path in reads:
        path.write_text('@r\nACGT\n+\nIIII\n')
    packed = tmp_path / 'b.fastq.gz'
    packed.write_bytes(b'\x1f\x8b')
    with pytest.raises(ValueError, match='--discover-cells reads plain FASTQ files'):
        call(**dict(found, barcode_file=packed))
    assert not (tmp_path / 'out').exists()


def test_the_discovered_list_is_a_whitelist(tmp_path):
    """what run_many writes for the picked barcodes reads back as the whitelist it is used as"""
    from seekmer_amd import infer, mapper
    picked, candidates, info = ref.pick(SHADOW, 1)
    found = dict(info, counted=2119, short=1, unreadable=1, distinct=4, units=2121,
                 candidate_barcodes=[b for b, _, _ in candidates], candidate_counts=[n for _, n, _ in candidates])
    summary = infer._output_discovery(tmp_path, _barcodes(picked), found, 1, 8, 0, False)
    assert mapper.read_whitelist(tmp_path / 'barcodes.discovered.txt') == (_barcodes(picked), _barcodes(picked))
    lines = (tmp_path / 'barcodes.discovered.txt').read_text().splitlines()
    assert all(line.startswith('#') for line in lines[:3]) and lines[3:] == _barcodes(picked)
    assert 'threshold 100' in lines[1] and 'distinct 4, candidates 3, dropped 1' in lines[2]
    rows = [line.split('\t') for line in (tmp_path / 'barcodes.census.tsv').read_text().splitlines()]
    assert [(b, int(n), int(flag)) for b, n, flag in rows] == candidates
    assert summary == dict(expect_cells=1, barcode_length=8, units_counted=2119, short=1, unreadable=1, distinct=4, rank=1,
                           rank_count=1000, threshold=100, candidates=3, dropped_neighbours=1, picked=2, keep_neighbours=False)


# ---- no GPU, no answer --------------------------------------------------------------------------------------------
def test_a_census_needs_a_device(native_libs):
    import ctypes
    from seekmer_amd import mapper
    handle = ctypes.c_void_p()
    code = native_libs.hip().skm_barcode_census_create(0, 16, ctypes.byref(handle))
    if native_libs.device_count() > 0:
        assert code == 0 and handle and native_libs.hip().skm_barcode_census_destroy(handle) == 0
        return
    assert code == native_libs.SKM_ERR_NO_DEVICE and not handle and b'no HIP device' in native_libs.hip().skm_last_error()
    with pytest.raises(native_libs.NativeError) as error:
        mapper.BarcodeCensus(16)
    assert error.value.code == native_libs.SKM_ERR_NO_DEVICE
