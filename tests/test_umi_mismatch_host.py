"""The rule of `--umi-mismatches 1` ("UMI mismatches") on the host: the two statements of the
reference against each other and against hand-made cases, and the refusals that need no GPU."""
import numpy as np
import pytest

import umi_mismatch_reference as near
import umi_reference as exact


def _both(cell, umi, tuples, length, mismatches=1):
    a = near.survivors(cell, umi, tuples, length, mismatches)
    b = near.survivors_by_definition(cell, umi, tuples, length, mismatches)
    np.testing.assert_array_equal(a, b)
    return a.tolist()


def _case(rng, length):
    """few UMIs, few classes, few cells: neighbours abound"""
    n = int(rng.integers(0, 60))
    values = rng.integers(0, 4 ** length, size=int(rng.integers(1, 5)), dtype=np.uint64)
    flips = np.zeros(7, dtype=np.uint64)         # no substitution, or one of six
    flips[1:] = (rng.integers(1, 4, size=6) << (2 * rng.integers(0, length, size=6))).astype(np.uint64)
    umi = (rng.choice(values, size=n) ^ rng.choice(flips, size=n)).astype(np.uint32)
    classes = [(), (1,), (1, 2), (7,)]
    tuples = [classes[i] for i in rng.integers(0, len(classes), size=n)]
    cell = rng.integers(-1, 3, size=n).astype(np.int32)
    return cell, umi, tuples


def test_the_two_statements_agree_on_random_cases():
    rng = np.random.default_rng(5)
    removed_by_a_neighbour = 0
    for i in range(200):
        length = (1, 2, 5, 16)[i % 4]
        cell, umi, tuples = _case(rng, length)
        with_one = _both(cell, umi, tuples, length, 1)
        with_none = _both(cell, umi, tuples, length, 0)
        assert with_none == exact.survivors(cell, umi, tuples).tolist()
        assert all(b or not a for a, b in zip(with_one, with_none)), 'one mismatch only removes more'
        removed_by_a_neighbour += sum(b and not a for a, b in zip(with_one, with_none))
    assert removed_by_a_neighbour > 500


def test_by_hand():
    c = (3, 4)
    # a near copy next to its original; the original's own copy; distance 2 stays
    assert _both([0, 0, 0, 0], [0b0000, 0b0001, 0b0000, 0b1010], [c] * 4, 2) == [True, False, False, True]
    # a chain in the order m0, m1, m2 leaves one; in the order m0, m2, m1 it leaves two
    m0, m1, m2 = 0b000000, 0b000100, 0b110100
    assert _both([0, 0, 0], [m0, m1, m2], [c] * 3, 3) == [True, False, False]
    assert _both([0, 0, 0], [m0, m2, m1], [c] * 3, 3) == [True, True, False]
    # "earlier" ignores whether the earlier unit stayed: m1 was removed, m2 goes all the same
    assert _both([0, 0, 0, 0], [m0, m1, m1, m2], [c] * 4, 3) == [True, False, False, False]
    # another class, another cell, no cell, no class
    assert _both([0, 0], [5, 4], [c, (3,)], 2) == [True, True]
    assert _both([0, 1], [5, 4], [c, c], 2) == [True, True]
    assert _both([0, -1, 0], [5, 4, 4], [c, c, c], 2) == [True, False, False]
    assert _both([0, 0, 0], [5, 4, 5], [(), (), ()], 2) == [True, True, True]
    # the first and the last base, at 16 and at 5 bases; UMI 0 and UMI 4^L - 1
    for length in (16, 5):
        top, ones = 2 * (length - 1), 4 ** length - 1
        assert _both([0] * 3, [0, 1 << top, 3], [c] * 3, length) == [True, False, False]
        assert _both([0] * 3, [ones, ones ^ (2 << top), ones ^ 1], [c] * 3, length) == [True, False, False]
        assert _both([0] * 2, [1 << top, 1], [c] * 2, length) == [True, True]               # distance 2
        if length < 16:                       # a bit above the UMI's bases is no base of it
            with pytest.raises(AssertionError):
                near.survivors([0], [4 ** length], [c], length, 1)
    # a near UMI that itself appears twice: one near removal, one exact removal
    assert _both([0, 0, 0], [8, 9, 9], [c] * 3, 2) == [True, False, False]
    assert _both([0, 0, 0], [8, 9, 9], [c] * 3, 2, 0) == [True, True, False]
    assert _both([], [], [], 4) == []


def test_no_mismatch_is_the_exact_rule():
    rng = np.random.default_rng(6)
    cell, umi, tuples = _case(rng, 5)
    np.testing.assert_array_equal(near.survivors(cell, umi, tuples, 5, 0), exact.survivors(cell, umi, tuples))
    with pytest.raises(ValueError):
        near.survivors(cell, umi, tuples, 5, 2)


# ---- refusals: nothing is opened, no output folder is made ----------------------------------------------------------
POOLED = ['r1.fq', 'r2.fq', '--barcodes', 'w.txt', '--barcode-file', 'b.fq']
DISCOVER = ['r1.fq', 'r2.fq', '--discover-cells', '10', '--barcode-length', '12', '--barcode-file', 'b.fq']


@pytest.mark.parametrize('arguments, message', [
    (POOLED + ['--umi-mismatches', '1'], 'goes with --umi-length'),
    (DISCOVER + ['--umi-mismatches', '1'], 'goes with --umi-length'),
    (['r1.fq', 'r2.fq', '--umi-mismatches', '1'], 'goes with'),
    (POOLED + ['--umi-length', '8', '--umi-mismatches', '2'], 'invalid choice'),
    (POOLED + ['--umi-length', '8', '--umi-mismatches', '-1'], 'invalid choice'),
])
def test_the_command_line_refuses(arguments, message, capsys, tmp_path, monkeypatch):
    from seekmer_amd.__main__ import parse_args
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as exit_:
        parse_args(['infer-many', 'index.npz', 'out'] + arguments)
    assert exit_.value.code == 2 and message in capsys.readouterr().err
    assert not (tmp_path / 'out').exists()


def test_the_command_line_accepts():
    from seekmer_amd.__main__ import parse_args
    for pooled in (POOLED, DISCOVER):
        assert parse_args(['infer-many', 'index.npz', 'out'] + pooled + ['--umi-length', '8'])['umi_mismatches'] == 0
        for value in (0, 1):
            opts = parse_args(['infer-many', 'index.npz', 'out'] + pooled + ['--umi-length', '8', '--umi-mismatches', str(value)])
            assert opts['umi_mismatches'] == value
    assert parse_args(['infer-many', 'index.npz', 'out', 'r1.fq', 'r2.fq'])['umi_mismatches'] == 0


def test_run_many_and_map_barcoded_refuse(tmp_path):
    from seekmer_amd import infer, mapper
    reads = [tmp_path / 'r1.fastq', tmp_path / 'r2.fastq']          # (none of these files exists)
    call = lambda **k: infer.run_many(tmp_path / 'i.npz', tmp_path / 'out', reads, 1, False, 0, False, **k)
    pooled = dict(barcodes=tmp_path / 'w.txt', barcode_file=tmp_path / 'b.fastq')
    with pytest.raises(ValueError, match='go with UMIs'):
        call(umi_mismatches=1, umi_length=0, **pooled)
    with pytest.raises(ValueError, match='go with UMIs'):
        call(umi_mismatches=1)
    with pytest.raises(ValueError, match='go with UMIs'):
        call(umi_mismatches=1, discover_cells=10, barcode_length=12, barcode_file=tmp_path / 'b.fastq')
    for bad in (2, -1, 0.5, None):
        with pytest.raises(ValueError, match='0 or 1'):
            call(umi_mismatches=bad, umi_length=8, **pooled)
    assert not (tmp_path / 'out').exists()
    with pytest.raises(ValueError, match='go with UMIs'):
        mapper.map_barcoded(None, None, None, None, True, per_sample_lengths=True, umi_mismatches=1, umi_length=0)
    with pytest.raises(ValueError, match='0 or 1'):
        mapper.map_barcoded(None, None, None, None, True, per_sample_lengths=True, umi_mismatches=2, umi_length=8)
