"""UMI collapse without a GPU: tests/umi_reference.py on hand-written cases, the command line's refusals, and
demux_chunks handing every segment the UMIs of exactly its units."""
import numpy as np
import pytest

import barcode_reference
import umi_reference as ref


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('read, start, length, umi', [
    ('ACGT', 0, 4, 0b00011011),
    ('ACGT', 0, 1, 0),
    ('ACGT', 3, 1, 3),
    ('ACGT', 1, 2, 0b0110),
    ('TTTTTTTTTTTTTTTT', 0, 16, 2 ** 32 - 1),
    ('AAAAAAAAAAAAAAAA', 0, 16, 0),
    ('GGACGTACGTACGTCA', 14, 2, 0b0100),
    ('ACGT', 1, 4, None),                     # one base short
    ('ACGT', 4, 1, None),
    ('', 0, 1, None),
    ('ACNT', 0, 4, None),
    ('ACgT', 0, 4, None),
    ('ACNT', 0, 2, 0b0001),                   # the N lies behind the window
    ('nCGT', 1, 3, 0b011011),                 # ... or in front of it
])
def test_windows_line_by_line(read, start, length, umi):
    got, readable = ref.windows([read], start, length)
    assert readable[0] == (umi is not None) and got[0] == (umi or 0) and got.dtype == np.uint32


def test_survivors_by_hand():
    #        unit   0       1       2       3    4       5       6       7       8    9       10
    cell = [0,      0,      1,      0,      0,   -1,     0,      1,      0,      0,   0]
    umi = [7,       7,      7,      7,      7,   7,      9,      7,      7,      7,   0]
    tuples = [(1, 2), (1, 2), (1, 2), (2, 1), (), (1, 2), (1, 2), (1, 2), (1,), (), (1, 2)]
    stay = ref.survivors(np.asarray(cell), np.asarray(umi, dtype=np.uint32), tuples)
    # 1: a copy of 0; 2: another cell; 3: another class (the order of the ids counts); 4, 9: unaligned units always
    # stay; 5: no cell; 6, 10: another UMI; 7: a copy of 2; 8: another class
    assert stay.tolist() == [True, False, True, True, True, False, True, False, True, True, True]
    assert ref.survivors(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint32), []).size == 0
    # the first of many is the one that stays, however far apart
    far = ref.survivors(np.zeros(5000, dtype=np.int32), np.full(5000, 3, dtype=np.uint32), [(4,)] * 5000)
    assert far[0] and not far[1:].any()


# ---- the command line -----------------------------------------------------------------------------------------------
POOLED = ['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq']


@pytest.mark.parametrize('arguments, message', [
    (['r1.fq', 'r2.fq', '--umi-length', '8'], 'goes with --barcodes'),
    (['r1.fq', 'r2.fq', '--umi-start', '8'], 'goes with --barcodes'),
    (POOLED + ['--umi-length', '0'], '1 to 16'),
    (POOLED + ['--umi-length', '17'], '1 to 16'),
    (POOLED + ['--umi-length', '8', '--umi-start', '-1'], '0 or more'),
    (POOLED + ['--umi-start', '12'], 'goes with --umi-length'),
])
def test_the_command_line_refuses(arguments, message, capsys):
    from seekmer_amd.__main__ import parse_args
    with pytest.raises(SystemExit) as exit_:
        parse_args(['infer-many', 'index.npz', 'out'] + arguments)
    assert exit_.value.code == 2 and message in capsys.readouterr().err


def test_the_command_line_accepts():
    from seekmer_amd.__main__ import parse_args
    opts = parse_args(['infer-many', 'index.npz', 'out'] + POOLED)
    assert (opts['umi_start'], opts['umi_length']) == (0, 0)
    opts = parse_args(['infer-many', 'index.npz', 'out'] + POOLED + ['--umi-length', '16'])
    assert (opts['umi_start'], opts['umi_length']) == (0, 16)
    opts = parse_args(['infer-many', 'index.npz', 'out'] + POOLED + ['--umi-length', '1', '--umi-start', '28'])
    assert (opts['umi_start'], opts['umi_length']) == (28, 1)
    for command in ('infer', 'impute'):       # (neither takes the options)
        with pytest.raises(SystemExit):
            parse_args([command, 'index.npz', 'out', 'r1.fq', 'r2.fq', '--umi-length', '8'])


def test_run_many_refuses_what_the_command_line_does(tmp_path):
    from seekmer_amd import infer
    white = tmp_path / 'w.txt'
    white.write_text('ACGT\n')
    reads = [tmp_path / 'r1.fastq', tmp_path / 'r2.fastq']
    call = lambda **k: infer.run_many(tmp_path / 'i.npz', tmp_path / 'out', reads, 1, False, 0, False, **k)
    with pytest.raises(ValueError, match='go with --barcodes'):
        call(umi_length=8)
    for bad in (17, -1):
        with pytest.raises(ValueError, match='umi-length'):
            call(barcodes=white, barcode_file=tmp_path / 'b.fastq', umi_length=bad)
    with pytest.raises(ValueError, match='umi-start'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq', umi_length=8, umi_start=-1)
    with pytest.raises(ValueError, match='goes with --umi-length'):
        call(barcodes=white, barcode_file=tmp_path / 'b.fastq', umi_start=4)
    assert not (tmp_path / 'out').exists()


# ---- the chunk walk -------------------------------------------------------------------------------------------------
def _stream_pieces(rng, stream, n_units, cuts, paired):
    """One stream's reads as consecutive PackedReads pieces cut at `cuts`; read u carries u in its first code word"""
    from seekmer_amd.common import PackedReads
    pieces, bounds = [], [0] + list(cuts) + [n_units]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        codes = np.zeros((hi - lo, 2), dtype=np.uint64)
        codes[:, 0] = np.arange(lo, hi, dtype=np.uint64) * 2 + stream
        codes[:, 1] = rng.integers(0, 2 ** 63, size=hi - lo, dtype=np.uint64)
        lengths = rng.integers(33, 65, size=hi - lo).astype(np.uint32)
        none = np.zeros(0, dtype=np.uint32)
        pieces.append(PackedReads.from_arrays(stream, lo, codes, lengths, none, np.zeros((0, 2), dtype=np.uint32), paired=paired))
    return pieces


@pytest.mark.parametrize('chunk_units', [1, 7, 60])
@pytest.mark.parametrize('paired', [True, False])
def test_chunk_walk_hands_every_segment_the_umis_of_its_units(native_libs, chunk_units, paired):
    from seekmer_amd import mapper
    rng = np.random.default_rng(chunk_units + paired)
    n_units, n_samples = 60, 5
    sample = rng.integers(-1, n_samples - 1, size=n_units).astype(np.int32)           # (sample 4 has no unit at all)
    umi = rng.integers(0, 2 ** 32, size=n_units, dtype=np.uint32)
    streams = [_stream_pieces(rng, 0, n_units, (13, 14, 40), paired)]
    if paired:
        streams.append(_stream_pieces(rng, 1, n_units, (5, 33), paired))
    pieces = [p for group in zip(*streams) for p in group] + [p for s in streams for p in s[min(map(len, streams)):]]
    seen, segments = {s: [] for s in range(n_samples)}, []

    def add(s, first_unit, mate1, mate2, umis):
        assert first_unit == len(seen[s])
        units = (mate1.codes[:, 0] // np.uint64(2)).astype(np.int64)
        assert umis.dtype == np.uint32 and umis.shape == units.shape
        np.testing.assert_array_equal(umis, umi[units])                 # exactly its units', in their order
        seen[s] += units.tolist()
        segments.append(units.size)

    added, walked = mapper.demux_chunks(pieces, paired, sample, n_samples, chunk_units, barcode_reference.group, add, umi=umi)
    assert walked == n_units
    for s in range(n_samples):
        assert seen[s] == np.flatnonzero(sample == s).tolist() and added[s] == len(seen[s])
    if chunk_units == 1:
        assert segments == [1] * int((sample >= 0).sum())
    if chunk_units == 60:
        assert len(segments) == len(set(sample[sample >= 0].tolist()))              # the whole run: one segment a cell

    def plain(s, first_unit, mate1, mate2):   # (without umi= the callers of old get the call of old)
        pass
    mapper.demux_chunks(pieces, paired, sample, n_samples, chunk_units, barcode_reference.group, plain)
