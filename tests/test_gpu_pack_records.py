"""The read records the packing kernels leave (pack_reads_staged_kernel, and pack_reads_kernel for reads
too long for its stage) against tests/pack_record_reference.py, bit for bit: ReadMapper.map_batch on a small
index, skm_mapper_copy_records, array_equal.  The reference itself is pinned to the host packer by
tests/test_pack_record_reference.py, on the same inputs."""
import ctypes

import numpy as np
import pytest

import pack_record_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def index(native_libs):
    from seekmer_amd import index_builder, synth
    ids, pool, tx_offsets = synth.transcriptome(3, 40)
    return index_builder.build_pooled(ids, pool, tx_offsets)


def _stage_reads(native_libs, words):
    reads = ctypes.c_int32(-1)
    assert native_libs.hip().skm_pack_stage_reads(words, ctypes.byref(reads)) == 0
    return reads.value


def _device_records(native_libs, index, bases, offsets, paired):
    """The records of the batch as the map kernel read them, and W"""
    from seekmer_amd import common, mapper
    n_reads = offsets.size - 1
    result = mapper.MapResult(index)
    held = np.ascontiguousarray(bases) if bases.size else np.zeros(1, dtype=np.uint8)
    mapper.ReadMapper(index, result).map_batch(common.ReadBatch(n_reads // (2 if paired else 1), held, offsets, paired))
    hip = native_libs.hip()
    record_words, words = ctypes.c_int32(), ctypes.c_int32()
    native_libs.check(hip.skm_mapper_copy_records(result._handle, 0, n_reads, None, ctypes.byref(record_words),
                                                  ctypes.byref(words)))
    out = np.full((n_reads, record_words.value), 0xa5a5a5a5, dtype=np.uint32)
    native_libs.check(hip.skm_mapper_copy_records(result._handle, 0, n_reads, native_libs.ptr(out, native_libs.c_u32p),
                                                  None, None))
    # a slice of the batch is the same rows
    if n_reads > 2:
        part = np.zeros((n_reads - 2, record_words.value), dtype=np.uint32)
        native_libs.check(hip.skm_mapper_copy_records(result._handle, 1, n_reads - 2,
                                                      native_libs.ptr(part, native_libs.c_u32p), None, None))
        np.testing.assert_array_equal(part, out[1:-1])
    assert hip.skm_mapper_copy_records(result._handle, 1, n_reads, None, None, None) == native_libs.SKM_ERR_ARG
    return out, words.value


def _check(native_libs, index, bases, offsets, paired, staged=None):
    want = ref.records(bases, offsets)
    got, words = _device_records(native_libs, index, bases, offsets, paired)
    assert words == ref.words_per_read(int(np.diff(offsets).max()))
    if staged is not None:
        assert (_stage_reads(native_libs, words) > 0) == staged
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


_LENGTH_CASES = list(ref.length_cases())


@pytest.mark.parametrize('paired', [False, True], ids=['single', 'paired'])
@pytest.mark.parametrize('name,lengths', _LENGTH_CASES, ids=[c[0] for c in _LENGTH_CASES])
def test_records_by_read_length(native_libs, index, name, lengths, paired):
    """Uniform batches of every length of the list, the ragged batch, the batch in which no read starts at a
    multiple of 16, a 250-base read before 50-base reads (pad words and their flags are zero) and a batch of
    reads beyond the stage (the kernel with a lane per word)."""
    bases, offsets = ref.batch_of(lengths, seed=len(lengths) + sum(lengths))
    _check(native_libs, index, bases, offsets, paired, staged=name != 'fallback')


def test_a_handle_without_a_batch_has_no_records(native_libs, index):
    from seekmer_amd import mapper
    result = mapper.MapResult(index)
    words = ctypes.c_int32()
    assert native_libs.hip().skm_mapper_copy_records(result._handle, 0, 0, None, None,
                                                     ctypes.byref(words)) == native_libs.SKM_ERR_STATE


@pytest.mark.parametrize('length', [100, 150, 250])
def test_records_around_the_block(native_libs, index, length):
    """1, 2, R - 1, R, R + 1 and 2 R + 1 reads, R the library's reads per block for this words_per_read"""
    reads = _stage_reads(native_libs, ref.words_per_read(length))
    assert reads > 0
    for name, lengths in ref.block_cases(reads, length):
        bases, offsets = ref.batch_of(lengths, seed=len(lengths))
        _check(native_libs, index, bases, offsets, False, staged=True)


@pytest.mark.parametrize('byte', ref.ODD_BYTES, ids=[repr(b) for b in ref.ODD_BYTES])
def test_records_of_odd_bytes(native_libs, index, byte):
    """N, n, a, c, g, t, U, '.' and 0xe9 at positions 0, 15, 16, 31, 32 and the last base of the first read, the
    last read and a read that straddles 16-byte chunks"""
    bases, offsets = ref.odd_byte_batch(byte)
    _check(native_libs, index, bases, offsets, False, staged=True)


def test_records_of_the_benchmark_shape(native_libs, index):
    """3000 pairs of 2 x 100 bases"""
    rng = np.random.default_rng(11)
    bases, offsets = ref.random_reads(rng, [100] * 6000)
    _check(native_libs, index, ref.damage(bases, rng, 0.01), offsets, True, staged=True)


def test_sample_set_with_text_parts_at_different_offsets(native_libs, index):
    """Two samples whose reads lie in ONE host buffer, the second from an odd offset on: a sample set packs each
    from its own place (an offsets pointer into the middle of a larger array, bases that do not start at their
    block's beginning); the tables are those of the samples mapped alone."""
    from seekmer_amd import common, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(3, 40)
    n_units = 700
    first, first_offsets = synth.reads(3, pool, tx_offsets, 0, n_units, 75, True)
    second, second_offsets = synth.reads(3, pool, tx_offsets, n_units, n_units, 75, True)
    gap = np.frombuffer(b'NNNNNNN', dtype=np.uint8)                     # 7 bytes that belong to no read
    first = np.asarray(first, dtype=np.uint8)[int(first_offsets[0]):int(first_offsets[-1])]
    second = np.asarray(second, dtype=np.uint8)[int(second_offsets[0]):int(second_offsets[-1])]
    bases = np.concatenate([first, gap, second])
    offsets = [np.asarray(first_offsets, dtype=np.int64) - first_offsets[0],
               np.asarray(second_offsets, dtype=np.int64) - second_offsets[0] + first.size + gap.size]
    assert offsets[1][0] % 16 != 0
    alone = []
    for sample in range(2):
        result = mapper.MapResult(index)
        mapper.ReadMapper(index, result).map_batch(common.ReadBatch(
            n_units, bases[int(offsets[sample][0]):int(offsets[sample][-1])].copy(), offsets[sample] - offsets[sample][0], True))
        alone.append((result.sizes(), result.export()))
        assert alone[-1][0][0] > 10                                     # (classes: the reads do map)
    sample_set = mapper.SampleSet(index, True)
    for sample in range(2):
        sample_set.add_batch(sample, 0, common.ReadBatch(n_units, bases, offsets[sample], True))
    sizes = sample_set.sizes()
    tables = sample_set.export()
    for sample in range(2):
        assert tuple(int(v) for v in sizes[sample]) == alone[sample][0]
        for got, want in zip(tables[sample], alone[sample][1][:4]):
            np.testing.assert_array_equal(got, want)
