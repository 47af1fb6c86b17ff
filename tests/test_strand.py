"""--fr-stranded / --rf-stranded without a GPU: the command line, the hand-over of `strand` to the
mappers, and the preconditions of the GPU tests, checked with the oracle on the host filter
(tests/strand_reference.py)."""
import numpy as np
import pytest

from strand_reference import DECOY, antisense_transcriptome, filter_result, stranded_reads


class _Stop(Exception):
    pass


def test_the_two_flags_exclude_each_other(tmp_path, capsys):
    from seekmer_amd import __main__ as cli
    for command in ('infer', 'impute'):
        with pytest.raises(SystemExit) as stop:
            cli.main([command, str(tmp_path / 'i.npz'), str(tmp_path / 'out'), str(tmp_path / 'r.fastq'),
                      '--fr-stranded', '--rf-stranded'])
        assert stop.value.code == 2
        assert 'not allowed with argument' in capsys.readouterr().err


def _parse(argv):
    import argparse
    from seekmer_amd import impute, infer
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(dest='subcommand')
    infer.add_subcommand_parser(subparsers)
    impute.add_subcommand_parser(subparsers)
    return vars(parser.parse_args(argv))


@pytest.mark.parametrize('command', ['infer', 'impute'])
def test_the_flags_set_strand(command):
    base = [command, 'i.npz', 'out', 'r_1.fastq', 'r_2.fastq']
    assert _parse(base)['strand'] is None
    assert _parse(base + ['--fr-stranded'])['strand'] == 'fr'
    assert _parse(base + ['--rf-stranded'])['strand'] == 'rf'


class _Index:
    transcripts = None

    def device_handle(self, device):
        return None


class _Hip:
    @staticmethod
    def skm_pinned_set_device(device):
        return 0


@pytest.mark.parametrize('strand', [None, 'fr', 'rf'])
def test_infer_run_hands_strand_to_map_reads(tmp_path, monkeypatch, strand):
    from seekmer_amd import _native, common, infer, mapper
    seen = {}

    def record(*args, **kwargs):
        seen.update(kwargs)
        raise _Stop()

    monkeypatch.setattr(mapper, 'map_reads', record)
    monkeypatch.setattr(_native, 'hip', lambda: _Hip())
    monkeypatch.setattr(common.KMerIndex, 'load', staticmethod(lambda path: _Index()))
    monkeypatch.setattr(infer, '_feeder', lambda *args, **kwargs: [])
    with pytest.raises(_Stop):
        infer.run(tmp_path / 'i.npz', tmp_path / 'out', [tmp_path / 'r.fastq'], 1, False, True, 0, False,
                  strand=strand)
    assert seen['strand'] == strand


@pytest.mark.parametrize('strand', [None, 'fr', 'rf'])
def test_impute_run_hands_strand_to_map_multiple_samples(tmp_path, monkeypatch, strand):
    from seekmer_amd import common, impute, mapper
    seen = {}

    def record(*args, **kwargs):
        seen.update(kwargs)
        raise _Stop()

    class _Feeder:
        def __init__(self, *args, **kwargs):
            pass

        @staticmethod
        def eligible(paths):
            return True

    paths = [tmp_path / 'c_1.fastq', tmp_path / 'c_2.fastq']
    for path in paths:
        path.write_text('')
    monkeypatch.setattr(mapper, 'map_multiple_samples', record)
    monkeypatch.setattr(common.KMerIndex, 'load', staticmethod(lambda path: _Index()))
    monkeypatch.setattr(common, 'PackedReadFeeder', _Feeder)
    with pytest.raises(_Stop):
        impute.run(tmp_path / 'i.npz', tmp_path / 'out', paths, 1, False, False, 16, strand=strand)
    assert seen['strand'] == strand


def test_an_unknown_mode_is_refused(tmp_path):
    from seekmer_amd import infer, mapper
    with pytest.raises(ValueError):
        mapper.strand_mode('both')
    with pytest.raises(ValueError):
        infer._run(None, None, tmp_path / 'i.npz', tmp_path / 'out', [], 1, False, True, 0, False, 0, None, None,
                   strand='sense')


@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('mode', ['fr', 'rf'])
def test_the_antisense_fixture_with_the_oracle(oracle, paired, mode):
    """The antisense fixture does what the GPU tests rely on: unstranded, a class holds the decoy;
    filtered in the library's own orientation, no class does, every unit keeps its origin, none
    becomes unaligned and the decoy's TPM is exactly 0; filtered in the wrong orientation, most
    units become unaligned."""
    ids, seqs = antisense_transcriptome()
    oindex = oracle.build_index(seqs, ids)
    reads, origin = stranded_reads(seqs, np.random.default_rng(3), 3000, paired, mode)
    bases, offsets = oracle.pack_reads(reads)
    n_units = origin.size
    fld = np.zeros(2000, dtype=np.int64)
    result = oracle.map_batch(oindex, bases, offsets, n_units, paired, fld)
    assert any(DECOY in t for t in result.tuples())
    eff = oracle.effective_lengths(fld, oindex.lengths)

    filtered = filter_result(result, mode)
    tuples = filtered.tuples()
    assert all(DECOY not in t for t in tuples)
    assert all(origin[u] in tuples[u] for u in range(n_units))
    assert (filtered.count > 0).all()
    classes = oracle.Classes()
    classes.update(filtered)
    class_map, class_count = classes.summarize()
    assert DECOY not in class_map[1]
    tpm, _ = oracle.quantify(eff, class_map, class_count)
    assert tpm[DECOY] == 0.0

    wrong = filter_result(result, 'rf' if mode == 'fr' else 'fr')
    assert (wrong.count == 0).sum() > n_units // 2


def test_the_reference_pairs_split_by_strand(oracle, chr21_oracle_index, pairs21):
    """The reference's 21 pairs: 11 units lie in the transcripts' orientation, 10 antisense."""
    bases, offsets = oracle.pack_reads(pairs21)
    result = oracle.map_batch(chr21_oracle_index, bases, offsets, 21, True)
    assert (filter_result(result, 'fr').count > 0).sum() == 11
    assert (filter_result(result, 'rf').count > 0).sum() == 10
