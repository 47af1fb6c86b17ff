"""The HIP mapper against RECORDINGS of the compiled reference (tests/golden/reference_mapper.npz;
cases: tests/reference_cases.py; recorder: tests/golden/make_reference_recordings.py).  Reads only
tests/golden/.

The index is the product's host builder's on the golden chr21 FASTA, which
tests/test_reference_recordings.py pins to the reference's arrays bit for bit.  For every case the
reads are regenerated (their SHA-256 is the recorded one) and mapped with keep_spans=True; every
unit's count and unsigned entries, the histogram, the unaligned and total counts and the class table
(classes, targets and counts in first-seen order) must be what the reference's ReadMapper returned
into a collections.Counter (seekmer/mapper.py:54, 60-104).

NOT pinned here, because the reference's Python surface shows none of them (_get_ids drops the sign,
seekmer/_mapper.pyx:528-537; map_read is a cdef method): the signs of the entries, the spans and the
anchors.  Neither are reads shorter than 25 bases, which the reference reads past the end of
(SURVEY.md).  The oracle tests (tests/test_gpu_parity.py) keep all of these.
"""
import collections
import os

import numpy as np
import pytest

import reference_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MAPPER_CASES = ('pairs21', 'single33', 'single100', 'single251', 'paired33', 'paired100', 'paired251', 'long')


@pytest.fixture(scope='module')
def recording():
    with np.load(os.path.join(GOLDEN, 'reference_mapper.npz')) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def inputs(chr21, pairs21, recording):
    out = {}
    for name, paired, reads in cases.mapper_cases(chr21[1], pairs21):
        assert cases.reads_digest(reads) == str(recording[name + '/sha256']), name
        out[name] = (paired, reads)
    assert tuple(out) == MAPPER_CASES == tuple(recording['cases'].tolist())
    return out


@pytest.fixture(scope='module')
def index(native_libs, chr21):
    from seekmer_amd import index_builder
    return index_builder.build(*chr21)


def _expected_table(recording, name):
    """(classes in first-seen order, their counts, unaligned units) as the reference's Counter holds them."""
    counter = collections.Counter(cases.recorded_tuples(recording, name))
    unaligned = counter.pop((), 0)
    return list(counter.keys()), list(counter.values()), unaligned


def _compare_table(export, sizes, recording, name, fld=True):
    offsets, targets, counts = export[0], export[1], export[2]
    classes, class_counts, unaligned = _expected_table(recording, name)
    flat = targets.tolist()
    got = [tuple(flat[a:b]) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
    assert len(got) == len(classes)
    assert got == classes
    assert counts.tolist() == class_counts
    n_classes, _, n_unaligned, total = (int(v) for v in sizes)
    assert n_classes == len(classes)
    assert n_unaligned == unaligned
    assert total == int(recording[name + '/units']) == unaligned + sum(class_counts)
    if fld:
        np.testing.assert_array_equal(export[4], recording[name + '/fld'])


@pytest.mark.parametrize('name', MAPPER_CASES)
def test_units_and_tables_are_the_recorded_ones(oracle, index, recording, inputs, name):
    from seekmer_amd import common, mapper
    paired, reads = inputs[name]
    n_units = len(reads) // 2 if paired else len(reads)
    bases, offsets = oracle.pack_reads(reads)
    result = mapper.MapResult(index, keep_spans=True)
    rm = mapper.ReadMapper(index, result)
    rm.map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    _, _, _, _, counts, entries = rm.last_batch(n_units)
    assert counts.size == n_units == recording[name + '/counts'].size            # every unit is compared
    np.testing.assert_array_equal(counts, recording[name + '/counts'])
    entries = np.asarray(entries).astype(np.int64)
    np.testing.assert_array_equal(np.where(entries < 0, ~entries, entries), recording[name + '/ids'])
    _compare_table(result.export(), result.sizes(), recording, name)


def test_fastq_text_through_the_packed_reader(index, recording, inputs, tmp_path):
    """The paired 100-base case a second way: FASTQ text, parsed and packed by the one-pass reader
    (tests/test_gpu_parity.py::test_packed_reads_give_the_same_tables pins that path to the oracle)."""
    from seekmer_amd import common, mapper
    name = 'paired100'
    paired, reads = inputs[name]
    n_units = len(reads) // 2
    files = [tmp_path / ('r_%d.fastq' % s) for s in range(2)]
    for s, path in enumerate(files):
        with open(path, 'wb') as f:
            for u in range(n_units):
                read = reads[2 * u + s]
                f.write(b'@u%d\n' % u + read + b'\n+\n' + b'I' * len(read) + b'\n')
    feeder = common.PackedReadFeeder(files, True)
    result = mapper.map_reads(index, feeder, job_count=1)
    assert feeder.stats['units'] == n_units
    _compare_table(result.export(), result.sizes(), recording, name)


@pytest.mark.parametrize('names', [('single100', 'single33'), ('paired33', 'paired100')],
                         ids=['single', 'paired'])
def test_two_samples_of_one_sample_set(oracle, index, recording, inputs, names):
    """The single 100-base case and the paired 33-base case, each as one of two samples of a
    SampleSet: a set has one layout (a paired batch for a single-ended set is refused), so each is
    mapped in shared launches beside another case of its own layout.  Every sample's table is the
    Counter of its own recorded tuples."""
    from seekmer_amd import common, mapper
    paired = inputs[names[0]][0]
    sample_set = mapper.SampleSet(index, paired)
    for sample, name in enumerate(names):
        assert inputs[name][0] == paired
        reads = inputs[name][1]
        bases, offsets = oracle.pack_reads(reads)
        n_units = len(reads) // 2 if paired else len(reads)
        sample_set.add_batch(sample, 0, common.ReadBatch(n_units, bases, offsets, paired))
    sizes, tables = sample_set.sizes(), sample_set.export()
    assert len(sample_set) == len(tables) == 2
    total = np.zeros(2000, dtype=np.int64)
    for sample, name in enumerate(names):
        _compare_table(tables[sample], sizes[sample], recording, name, fld=False)
        total += recording[name + '/fld']
    np.testing.assert_array_equal(sample_set.fragment_length_counts, total)
