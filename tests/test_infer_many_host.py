"""`infer-many` without a GPU: the command line, the samples' names and grouping, the rule that routes samples
through a sample set, and the harmonic means of many histograms."""
import pathlib

import numpy as np
import pytest


def _parse(argv):
    import argparse
    from seekmer_amd import infer
    parser = argparse.ArgumentParser()
    infer.add_many_subcommand_parser(parser.add_subparsers(dest='subcommand'))
    return vars(parser.parse_args(['infer-many'] + argv))


def test_parser_has_the_flags_of_the_command():
    opts = _parse(['ix', 'out', 'a_1.fq', 'a_2.fq'])
    assert opts['index_path'] == pathlib.Path('ix') and opts['output_path'] == pathlib.Path('out')
    assert opts['fastq_paths'] == [pathlib.Path('a_1.fq'), pathlib.Path('a_2.fq')]
    assert (opts['job_count'], opts['single_ended'], opts['bootstrap'], opts['seed'], opts['device'], opts['strand'],
            opts['names']) == (1, False, 0, None, 0, None, None)
    opts = _parse(['ix', 'out', 'a.fq', 'b.fq', '-s', '-j', '4', '-b', '3', '--seed', '9', '--device', '1',
                   '--rf-stranded', '--names', 'x,y'])
    assert (opts['job_count'], opts['single_ended'], opts['bootstrap'], opts['seed'], opts['device'], opts['strand'],
            opts['names']) == (4, True, 3, 9, 1, 'rf', 'x,y')
    assert _parse(['ix', 'out', 'a.fq', '--fr-stranded'])['strand'] == 'fr'
    with pytest.raises(SystemExit):
        _parse(['ix', 'out', 'a.fq', '--fr-stranded', '--rf-stranded'])
    with pytest.raises(SystemExit):
        _parse(['ix', 'out', 'a.fq', '-m'])          # (a set has no readmap)
    assert 'save_readmap' not in opts


def test_the_command_is_wired_into_the_program(monkeypatch):
    from seekmer_amd import infer
    from seekmer_amd.__main__ import main
    seen = {}
    monkeypatch.setattr(infer, 'run_many', lambda **opts: seen.update(opts))
    assert main(['infer-many', 'ix', 'out', 'a.fq', 'b.fq', '-s', '--names', 'p,q']) == 0
    assert seen['names'] == 'p,q' and seen['single_ended'] and seen['fastq_paths'] == [pathlib.Path('a.fq'), pathlib.Path('b.fq')]


def test_grouping_follows_impute():
    from seekmer_amd import infer
    paths = [pathlib.Path(name) for name in ('a_1.fq', 'a_2.fq', 'b_1.fq', 'b_2.fq', 'c_1.fq')]
    assert infer.sample_groups(paths[:4], False) == [(paths[0], paths[1]), (paths[2], paths[3])]
    assert infer.sample_groups(paths, True) == [(path,) for path in paths]
    assert infer.sample_groups([], False) == []
    for odd in (paths, paths[:1]):                  # a file that would end up in no sample
        with pytest.raises(ValueError, match='every two files'):
            infer.sample_groups(odd, False)


def test_names():
    from seekmer_amd import infer
    groups = [('/data/plate1/A01.R1.fastq.gz', '/data/plate1/A01.R2.fastq.gz'), (pathlib.Path('x/B02_1.fq'), pathlib.Path('x/B02_2.fq'))]
    assert infer.sample_names(groups) == ['A01', 'B02_1']
    assert infer.sample_names(groups, 'left,right') == ['left', 'right']
    assert infer.sample_names(groups, ['l', 'r']) == ['l', 'r']
    for names in ('one', 'a,b,c', 'same,same', 'a,', 'a,b/c', 'a,..'):
        with pytest.raises(ValueError):
            infer.sample_names(groups, names)
    with pytest.raises(ValueError, match='A01'):
        infer.sample_names([('p/A01.fq',), ('q/A01.fq',)])


def test_bad_names_are_refused_before_anything_is_opened(tmp_path):
    """Paths that do not exist: a ValueError about the names, not about the files or the index."""
    from seekmer_amd import infer
    missing = [tmp_path / 'no' / 'A.fq', tmp_path / 'no' / 'B.fq', tmp_path / 'nowhere' / 'A.fq', tmp_path / 'nowhere' / 'C.fq']
    common = dict(index_path=tmp_path / 'no_index.npz', output_path=tmp_path / 'out', job_count=1, bootstrap=0, debug=False)
    with pytest.raises(ValueError, match='not unique'):
        infer.run_many(fastq_paths=missing, single_ended=True, **common)
    with pytest.raises(ValueError, match='3 names for 2 samples'):
        infer.run_many(fastq_paths=missing, single_ended=False, names='a,b,c', **common)
    with pytest.raises(ValueError):
        infer.run_many(fastq_paths=missing, single_ended=False, strand='sideways', **common)
    assert not (tmp_path / 'out').exists()


def test_several_ranks_are_refused(tmp_path, monkeypatch):
    from seekmer_amd import infer, parallel
    monkeypatch.setattr(parallel.Ranks, 'from_env', classmethod(lambda cls: cls(rank=0, world=2, local_rank=0)))
    with pytest.raises(ValueError, match='one process'):
        infer.run_many(index_path=tmp_path / 'no_index.npz', output_path=tmp_path / 'out', fastq_paths=[tmp_path / 'a.fq', tmp_path / 'b.fq'],
                       job_count=1, single_ended=True, bootstrap=0, debug=False)
    assert not (tmp_path / 'out').exists()


def test_routing_rule(monkeypatch):
    from seekmer_amd import impute, infer
    limit = impute.SAMPLE_SET_MAX_CELL_BYTES
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    assert infer.sample_set_members([10, 20, 30], limit) == [0, 1, 2]
    assert infer.sample_set_members([limit, limit + 1, 0], limit) == [0, 2]
    assert infer.sample_set_members([limit + 1, 5, limit + 2], limit) == []        # one small sample: no set
    assert infer.sample_set_members([5], limit) == [] and infer.sample_set_members([], limit) == []
    assert infer.sample_set_members([limit + 1, limit + 1], limit) == []
    assert infer.sample_set_members([10, 20], limit, per_sample=True) == []
    for value, members in (('1', []), ('0', [0, 1]), ('true', [0, 1]), ('', [0, 1])):   # exactly "1", looked up at every call
        monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', value)
        assert infer.sample_set_members([10, 20], limit) == members


def test_harmonic_means_of_many_histograms(oracle):
    from seekmer_amd import mapper
    rng = np.random.default_rng(3)
    counts = np.zeros((5, 2000), dtype=np.int64)
    counts[0, 150:400] = rng.integers(0, 50, 250)
    counts[1, 1999] = 7
    counts[2, 1] = 1
    counts[4, 25:1999] = rng.integers(0, 1 << 40, 1974)
    means = mapper.harmonic_mean_fragment_lengths(counts)
    assert len(means) == 5 and means[3] == 0 and means[1] == 1999.0 and means[2] == 1.0
    for row, mean in zip(counts, means):
        assert mean == oracle.harmonic_mean_fragment_length(row)
    assert mapper.harmonic_mean_fragment_lengths(counts[:0]) == []
    # the arithmetic of MapResult.harmonic_mean_fragment_length, spelled out
    fld = counts[0]
    assert means[0] == fld.sum() / (fld[1:].astype('f8') / np.arange(1, 2000)).sum()
