"""`seekmer_amd infer-many`: many samples against one resident index.  Every sample's folder holds the files
that `seekmer_amd infer` writes for that sample alone -- abundance.tsv byte for byte, run_info.json and the
arrays of abundance.npz equal but for the start time and the call -- whether the samples share launches in a
sample set (the default for small samples) or are mapped one by one (SKM_INFER_MANY_PER_SAMPLE=1)."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

READ_LEN = 75


@pytest.fixture(scope='module')
def synthetic(native_libs, tmp_path_factory):
    """(index path, transcriptome) of synth.transcriptome(5, 30), saved once."""
    from seekmer_amd import index_builder, synth
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    index_path = tmp_path_factory.mktemp('index') / 'index.npz'
    index.save(index_path)
    return index_path, pool, tx_offsets


def _write_samples(folder, pool, tx_offsets, units, paired):
    """One sample per entry of `units` as FASTQ files s<i>_1.fastq (+ s<i>_2.fastq); synth.reads has no
    fragment-length setting, so the samples differ by seed and by where their units begin."""
    from seekmer_amd import synth
    paths = []
    for sample, n_units in enumerate(units):
        bases, _ = synth.reads(100 + sample % 2, pool, tx_offsets, sample * 8000, n_units, READ_LEN, paired)
        names = [folder / ('s%d_%d.fastq' % (sample, mate + 1)) for mate in range(2 if paired else 1)]
        synth.write_fastq(bases, n_units, READ_LEN, paired, *names)
        paths += names
    return paths


def _assert_same_outputs(ours, theirs, everything=True):
    one, other = (ours / 'abundance.tsv').read_bytes(), (theirs / 'abundance.tsv').read_bytes()
    assert len(one) > 1000 and one == other, ours.name
    if not everything:
        return
    info = [json.loads((folder / 'run_info.json').read_text()) for folder in (ours, theirs)]
    for run_info in info:
        del run_info['start_time'], run_info['call']
    assert info[0] == info[1]
    with np.load(ours / 'abundance.npz') as a, np.load(theirs / 'abundance.npz') as b:
        assert sorted(a.files) == sorted(b.files) and 'bootstrap/bs1' in a.files
        for name in a.files:
            if name not in ('aux/call', 'aux/start_time'):
                np.testing.assert_array_equal(a[name], b[name], err_msg=name)


@pytest.fixture(scope='module')
def paired_runs(synthetic, tmp_path_factory):
    """Five paired samples, and `infer -b 2 --seed 7` of each: (index path, files, unit counts, folder)."""
    from seekmer_amd.__main__ import main
    index_path, pool, tx_offsets = synthetic
    folder = tmp_path_factory.mktemp('paired')
    units = (2000, 3500, 4000, 2500, 3000)
    paths = _write_samples(folder, pool, tx_offsets, units, True)
    for sample in range(len(units)):
        assert main(['infer', str(index_path), str(folder / 'alone' / ('s%d_1' % sample)),
                     *map(str, paths[2 * sample:2 * sample + 2]), '-b', '2', '--seed', '7']) == 0
    return index_path, paths, units, folder


def test_every_sample_gets_the_files_of_infer(paired_runs, monkeypatch):
    from seekmer_amd import mapper
    from seekmer_amd.__main__ import main
    index_path, paths, units, folder = paired_runs
    calls = []
    through_set = mapper.map_sample_set
    monkeypatch.setattr(mapper, 'map_sample_set',
                        lambda *a, **k: calls.append(k.get('per_sample_lengths')) or through_set(*a, **k))
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    out = folder / 'many'
    assert main(['infer-many', str(index_path), str(out), *map(str, paths), '-b', '2', '--seed', '7', '-j', '3']) == 0
    assert calls == [True], 'small samples must be mapped through one sample set that keeps their histograms'
    for sample in range(len(units)):
        _assert_same_outputs(out / ('s%d_1' % sample), folder / 'alone' / ('s%d_1' % sample))
    lines = [line.split('\t') for line in (out / 'samples.tsv').read_text().splitlines()]
    assert [line[0] for line in lines] == ['s%d_1' % sample for sample in range(len(units))]
    assert [int(line[1]) for line in lines] == list(units)
    for sample, line in enumerate(lines):
        info = json.loads((out / line[0] / 'run_info.json').read_text())
        assert int(line[2]) == info['n_pseudoaligned'] > 0 and float(line[3]) > READ_LEN
    # the samples' own lengths, not pooled ones: two samples' eff_length columns differ
    columns = [np.load(out / ('s%d_1' % sample) / 'abundance.npz')['aux/eff_lengths'] for sample in (0, 1)]
    assert not np.array_equal(columns[0], columns[1])


def test_both_routes_write_the_same_files(paired_runs, monkeypatch):
    from seekmer_amd import mapper
    from seekmer_amd.__main__ import main
    index_path, paths, units, folder = paired_runs
    calls = []
    through_set = mapper.map_sample_set
    monkeypatch.setattr(mapper, 'map_sample_set', lambda *a, **k: calls.append('set') or through_set(*a, **k))
    monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', '1')
    out = folder / 'one_by_one'
    names = ','.join('n%d' % sample for sample in range(len(units)))
    assert main(['infer-many', str(index_path), str(out), *map(str, paths), '-b', '2', '--seed', '7', '--names', names]) == 0
    assert calls == []
    for sample in range(len(units)):
        _assert_same_outputs(out / ('n%d' % sample), folder / 'alone' / ('s%d_1' % sample))


class _MixedRoute:
    """The mixed route for the five samples of `paired_runs`: impute.SAMPLE_SET_MAX_CELL_BYTES between the third
    and the fourth smallest sample, so that samples 0, 3 and 4 (2000, 2500 and 3000 units) share a sample set and
    samples 1 and 2 get a mapper each -- position k in the set is not sample number i.  `set_calls` holds the
    number of feeders of every mapper.map_sample_set call, `alone_calls` one entry per mapper.map_reads call."""

    def __init__(self, monkeypatch, paths):
        from seekmer_amd import impute, mapper
        sizes = [impute.cell_text_bytes(tuple(paths[2 * sample:2 * sample + 2])) for sample in range(len(paths) // 2)]
        assert len(set(sizes)) == len(sizes) == 5, sizes
        order = sorted(range(len(sizes)), key=sizes.__getitem__)
        assert sorted(order[:3]) == [0, 3, 4], sizes
        assert sizes[order[2]] + 1 < sizes[order[3]], sizes
        monkeypatch.setattr(impute, 'SAMPLE_SET_MAX_CELL_BYTES', (sizes[order[2]] + sizes[order[3]]) // 2)
        monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
        self.set_calls, self.alone_calls = [], []
        through_set, alone = mapper.map_sample_set, mapper.map_reads
        monkeypatch.setattr(mapper, 'map_sample_set',
                            lambda index, feeders, *a, **k: self.set_calls.append(len(feeders)) or through_set(index, feeders, *a, **k))
        monkeypatch.setattr(mapper, 'map_reads', lambda *a, **k: self.alone_calls.append(1) or alone(*a, **k))

    def assert_mixed(self):
        assert self.set_calls == [3] and self.alone_calls == [1, 1], (self.set_calls, self.alone_calls)


def _files(root):
    return sorted(str(path.relative_to(root)) for path in root.rglob('*') if path.is_file())


def _assert_same_trees(ours, theirs):
    """Every file of two output trees byte for byte, but run_info.json as JSON without its start time and call and
    abundance.npz array by array without those two; and the same relative paths."""
    assert _files(ours) == _files(theirs)
    for name in _files(ours):
        if name.endswith('run_info.json'):
            info = [json.loads((root / name).read_text()) for root in (ours, theirs)]
            for run_info in info:
                del run_info['start_time'], run_info['call']
            assert info[0] == info[1], name
        elif name.endswith('abundance.npz'):
            with np.load(ours / name) as a, np.load(theirs / name) as b:
                assert sorted(a.files) == sorted(b.files), name
                for array in a.files:
                    if array not in ('aux/call', 'aux/start_time'):
                        np.testing.assert_array_equal(a[array], b[array], err_msg=name + ': ' + array)
        else:
            assert (ours / name).read_bytes() == (theirs / name).read_bytes(), name


def test_mixed_route_writes_the_files_of_infer(paired_runs, monkeypatch):
    from seekmer_amd.__main__ import main
    index_path, paths, units, folder = paired_runs
    route = _MixedRoute(monkeypatch, paths)
    out = folder / 'mixed'
    assert main(['infer-many', str(index_path), str(out), *map(str, paths), '-b', '2', '--seed', '7', '-j', '3']) == 0
    route.assert_mixed()
    for sample in range(len(units)):
        _assert_same_outputs(out / ('s%d_1' % sample), folder / 'alone' / ('s%d_1' % sample))
    lines = [line.split('\t') for line in (out / 'samples.tsv').read_text().splitlines()]
    assert [line[0] for line in lines] == ['s%d_1' % sample for sample in range(len(units))]
    assert [int(line[1]) for line in lines] == list(units)


EVERY_TABLE = ['--bias', '--genes', '--count-matrix', '-b', '2', '--seed', '7']


@pytest.fixture(scope='module')
def mixed_tables(paired_runs):
    """`infer-many --bias --genes --gene-map FILE --count-matrix -b 2 --seed 7` on the mixed route:
    (output tree, gene-map file with transcript t in gene t // 4)."""
    from seekmer_amd import common
    from seekmer_amd.__main__ import main
    index_path, paths, units, folder = paired_runs
    ids = np.asarray(common.KMerIndex.load(index_path).transcripts['transcript_id'])
    assert ids.size > 100
    map_path = folder / 'gene_map.tsv'
    map_path.write_bytes(b''.join(b'%s\tG%03d\n' % (id_, t // 4) for t, id_ in enumerate(ids.tolist())))
    with pytest.MonkeyPatch.context() as monkeypatch:
        route = _MixedRoute(monkeypatch, paths)
        out = folder / 'mixed_tables'
        assert main(['infer-many', str(index_path), str(out), *map(str, paths), '--gene-map', str(map_path), *EVERY_TABLE]) == 0
        route.assert_mixed()
    return out, map_path


def test_mixed_route_with_every_table(paired_runs, mixed_tables, monkeypatch):
    from seekmer_amd.__main__ import main
    index_path, paths, units, folder = paired_runs
    mixed, map_path = mixed_tables
    monkeypatch.setenv('SKM_INFER_MANY_PER_SAMPLE', '1')
    out = folder / 'one_by_one_tables'
    assert main(['infer-many', str(index_path), str(out), *map(str, paths), '--gene-map', str(map_path), *EVERY_TABLE]) == 0
    names = ['s%d_1' % sample for sample in range(len(units))]
    per_sample = ['abundance.genes.tsv', 'abundance.npz', 'abundance.tsv', 'run_info.json']
    assert _files(out) == sorted(['genes.tpm.tsv', 'genes.unique_counts.tsv', 'samples.tsv']
                                 + ['counts/' + name for name in ('cells.tsv', 'genes.tsv', 'matrix.mtx', 'matrix.npz')]
                                 + [sample + '/' + name for sample in names for name in per_sample])
    _assert_same_trees(mixed, out)


def test_mixed_route_matrix_only(paired_runs, mixed_tables, monkeypatch):
    from seekmer_amd.__main__ import main
    index_path, paths, units, folder = paired_runs
    full, map_path = mixed_tables
    route = _MixedRoute(monkeypatch, paths)
    out = folder / 'mixed_matrix_only'
    assert main(['infer-many', str(index_path), str(out), *map(str, paths), '--gene-map', str(map_path), '--matrix-only']) == 0
    route.assert_mixed()
    assert sorted(path.name for path in out.iterdir()) == ['counts', 'samples.tsv']          # no folder per sample
    wanted = [name for name in _files(full) if name == 'samples.tsv' or name.startswith('counts/')]
    assert _files(out) == wanted and len(wanted) == 5
    for name in wanted:
        assert (out / name).read_bytes() == (full / name).read_bytes(), name


def test_single_ended_samples(synthetic, tmp_path, monkeypatch):
    from seekmer_amd.__main__ import main
    index_path, pool, tx_offsets = synthetic
    monkeypatch.delenv('SKM_INFER_MANY_PER_SAMPLE', raising=False)
    units = (2000, 3100, 2600)
    paths = _write_samples(tmp_path, pool, tx_offsets, units, False)
    assert main(['infer-many', str(index_path), str(tmp_path / 'many'), *map(str, paths), '-s', '-j', '2']) == 0
    for sample, path in enumerate(paths):
        alone = tmp_path / 'alone' / ('s%d_1' % sample)
        assert main(['infer', str(index_path), str(alone), str(path), '-s']) == 0
        _assert_same_outputs(tmp_path / 'many' / ('s%d_1' % sample), alone, everything=False)
    assert [int(line.split('\t')[1]) for line in (tmp_path / 'many' / 'samples.tsv').read_text().splitlines()] == list(units)


def test_a_sample_without_reads_is_refused_before_anything_is_written(synthetic, tmp_path):
    from seekmer_amd.__main__ import main
    index_path, pool, tx_offsets = synthetic
    paths = _write_samples(tmp_path, pool, tx_offsets, (300, 200), False)
    empty = tmp_path / 'nothing.fastq'
    empty.write_bytes(b'')
    with pytest.raises(ValueError, match='nothing'):
        main(['infer-many', str(index_path), str(tmp_path / 'out'), str(paths[0]), str(empty), str(paths[1]), '-s'])
    assert not (tmp_path / 'out' / 's0_1').exists() and not (tmp_path / 'out' / 'samples.tsv').exists()
