"""Strand-specific quantification (--fr-stranded / --rf-stranded) on the GPU against the oracle.

The reference for every check is the oracle's signed tuples filtered on the host by the rule of
skm_mapper_set_strand (tests/strand_reference.py); the spans and the fragment-length histogram are
those of the unfiltered oracle run.  Integer outputs are bit-identical; TPM and est_count have the
tolerance of test_cli_end_to_end (1e-4 relative + 1e-6 absolute)."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_product_index
from strand_reference import (DECOY, antisense_transcriptome, emptied_units, filter_result, filter_units,
                              mixed_units, reverse_complement, stranded_reads)

pytestmark = pytest.mark.gpu

MODES = {'fr': 1, 'rf': 2}


def _damaged_chr21_units(seqs, rng, n_units, paired, read_len=100):
    """Unstranded units of random chr21 fragments (either mate may come first), and among their
    reads the quirks: Ns, lower case, substitutions, indels, reads shorter than k, garbage."""
    long_tx = [s.upper() for s in seqs if len(s) > 450]
    reads = []
    for u in range(n_units):
        s = long_tx[int(rng.integers(len(long_tx)))]
        frag = int(rng.integers(150, 401))
        p = int(rng.integers(0, len(s) - frag + 1))
        f = s[p:p + frag]
        mates = [f[:read_len], reverse_complement(f[-read_len:])]
        if rng.integers(2):
            mates.reverse()
        for j, read in enumerate(mates if paired else mates[:1]):
            r = bytearray(read)
            kind = (2 * u + j) % 13
            if kind == 1:
                for _ in range(3):
                    r[int(rng.integers(len(r)))] = ord('N')
            elif kind == 2:
                q = int(rng.integers(len(r) - 10))
                r[q:q + 10] = bytes(r[q:q + 10]).lower()
            elif kind == 3:
                for _ in range(int(rng.integers(1, 6))):
                    r[int(rng.integers(len(r)))] = b'ACGT'[int(rng.integers(4))]
            elif kind == 4:
                del r[int(rng.integers(5, len(r) - 5))]
            elif kind == 5:
                r.insert(int(rng.integers(5, len(r) - 5)), b'ACGT'[int(rng.integers(4))])
            elif kind == 6:
                r = r[:int(rng.integers(0, 25))]
            elif kind == 7:
                r = bytearray(bytes(r).lower())
            elif kind == 8:
                r = bytearray(bytes(b'ACGT'[int(c)] for c in rng.integers(0, 4, read_len)))
            reads.append(bytes(r))
    return reads


@pytest.fixture(scope='module')
def antisense(oracle):
    ids, seqs = antisense_transcriptome()
    return ids, seqs, oracle.build_index(seqs, ids)


def _case(oracle, chr21, chr21_oracle_index, pairs21, antisense, source, mode, paired):
    """(oracle index, product index, bases, offsets, n_units) of one input; the antisense fixture's
    reads come from a library of orientation `mode`."""
    if source == 'antisense':
        ids, seqs, oindex = antisense
        reads, _ = stranded_reads(seqs, np.random.default_rng(3), 3000, paired, mode)
    else:
        ids, oindex = chr21[0], chr21_oracle_index
        if source == 'pairs21':
            reads = list(pairs21)
        else:
            reads = _damaged_chr21_units(chr21[1], np.random.default_rng(2024), 10_000, paired)
    bases, offsets = oracle.pack_reads(reads)
    n_units = len(reads) // 2 if paired else len(reads)
    return oindex, make_product_index(oindex, ids), bases, offsets, n_units


def _expected_table(oracle, units):
    classes = oracle.Classes()
    classes.update(units)
    return classes


def _same_table(oracle, result, filtered, fld):
    classes = _expected_table(oracle, filtered)
    offs, ids, counts = classes.export()
    g_offs, g_ids, g_counts, _, g_fld = result.export()
    np.testing.assert_array_equal(g_fld, fld)
    np.testing.assert_array_equal(g_offs, offs)
    np.testing.assert_array_equal(g_ids, ids)
    np.testing.assert_array_equal(g_counts, counts)
    assert result.sizes()[2] == classes.unaligned
    return classes


@pytest.mark.parametrize('paired', [True, False])
@pytest.mark.parametrize('mode', ['fr', 'rf'])
@pytest.mark.parametrize('source', ['antisense', 'pairs21', 'chr21'])
def test_units_and_tables_equal_the_filtered_oracle(oracle, native_libs, chr21, chr21_oracle_index, pairs21,
                                                    antisense, source, mode, paired):
    from seekmer_amd import common, mapper
    oindex, index, bases, offsets, n_units = _case(oracle, chr21, chr21_oracle_index, pairs21, antisense,
                                                   source, mode, paired)
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(oindex, bases, offsets, n_units, paired, fld)
    filtered = filter_result(expected, mode)
    if source == 'chr21':
        # the input must keep exercising the partial case and the emptied one
        print('chr21', mode, 'paired' if paired else 'single', 'mixed units', int(mixed_units(expected).sum()),
              'emptied', int(emptied_units(expected, mode).sum()), 'of', n_units)
        assert mixed_units(expected).any()
        assert emptied_units(expected, mode).any()
    result = mapper.MapResult(index, keep_spans=True, strand=mode)
    rm = mapper.ReadMapper(index, result)
    rm.map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    begin, end, a_entry, a_offset, counts, entries = rm.last_batch(n_units)
    np.testing.assert_array_equal(counts, filtered.count)
    np.testing.assert_array_equal(entries, filtered.entries)
    np.testing.assert_array_equal(begin, expected.begin)
    np.testing.assert_array_equal(end, expected.end)
    np.testing.assert_array_equal(a_entry, expected.anchor_entry)
    np.testing.assert_array_equal(a_offset, expected.anchor_offset)
    _same_table(oracle, result, filtered, fld)
    if source == 'antisense':
        assert all(DECOY not in t for t in filtered.tuples())
    if source == 'pairs21' and paired:
        assert (filtered.count > 0).sum() == {'fr': 11, 'rf': 10}[mode]


def _upload(native, array):
    pointer = ctypes.c_void_p()
    native.check(native.hip().skm_device_malloc(0, array.nbytes, ctypes.byref(pointer)))
    native.check(native.hip().skm_device_upload(0, pointer, array.ctypes.data, array.nbytes))
    return pointer


@pytest.mark.parametrize('paired', [True, False])
def test_every_ingest_path_gives_the_same_stranded_table(oracle, native_libs, chr21, chr21_oracle_index, paired,
                                                         tmp_path):
    """map_batch, map_batch_async with first_unit in shuffled order, the uniform async path, the
    device-resident batch, packed pieces through PackedReadFeeder from FASTQ (drained natively and
    pushed one by one), and -m through the ASCII reader: the filtered oracle's table, class order
    included."""
    from seekmer_amd import common, mapper
    mode = 'fr'
    read_len = 100
    reads = _damaged_chr21_units(chr21[1], np.random.default_rng(99), 6000, paired, read_len)
    uniform = [r for r in reads if len(r) == read_len]
    mates = 2 if paired else 1
    index = make_product_index(chr21_oracle_index, chr21[0])
    bases, offsets = oracle.pack_reads(reads)
    n_units = len(reads) // mates
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(chr21_oracle_index, bases, offsets, n_units, paired, fld)
    filtered = filter_result(expected, mode)
    assert mixed_units(expected).any() and emptied_units(expected, mode).any()

    whole = mapper.MapResult(index, strand=mode)
    mapper.ReadMapper(index, whole).map_batch(common.ReadBatch(n_units, bases, offsets, paired))
    _same_table(oracle, whole, filtered, fld)
    reference = whole.export()

    def same(result):
        for got, want in zip(result.export(), reference):
            np.testing.assert_array_equal(got, want)
        assert result.sizes() == whole.sizes()

    cut = [0, 900, 901, 2500, 4100, n_units]
    pieces = [common.ReadBatch(cut[k + 1] - cut[k], bases, offsets[mates * cut[k]:mates * cut[k + 1] + 1], paired,
                               first_unit=cut[k]) for k in range(len(cut) - 1)]
    one = mapper.MapResult(index, strand=mode)
    rm = mapper.ReadMapper(index, one)
    for k in np.random.default_rng(5).permutation(len(pieces)):
        rm.map_batch_async(pieces[k])
    one.sync()
    same(one)

    # the uniform form: reads of one length only, against their own filtered oracle table
    u_units = len(uniform) // mates
    u_bases, u_offsets = oracle.pack_reads(uniform[:mates * u_units])
    u_fld = np.zeros(2000, dtype=np.int64)
    u_filtered = filter_result(oracle.map_batch(chr21_oracle_index, u_bases, u_offsets, u_units, paired, u_fld), mode)
    one.reset()
    for k in np.random.default_rng(6).permutation(2):
        lo, hi = (0, u_units // 3) if k == 0 else (u_units // 3, u_units)
        piece = common.ReadBatch(hi - lo, u_bases, u_offsets[mates * lo:mates * hi + 1], paired, first_unit=lo)
        piece.uniform_len = read_len
        rm.map_batch_async(piece)
    _same_table(oracle, one, u_filtered, u_fld)

    # a batch already in HBM
    one.reset()
    d_bases, d_offsets = _upload(native_libs, bases), _upload(native_libs, offsets)
    try:
        one.map_resident(d_bases, d_offsets, n_units, paired, int(np.diff(offsets).max()))
        same(one)
    finally:
        native_libs.hip().skm_device_free(0, d_bases)
        native_libs.hip().skm_device_free(0, d_offsets)

    files = [tmp_path / ('r_%d.fastq' % s) for s in range(mates)]
    names = [b'u%d' % u for u in range(n_units)]
    for s, path in enumerate(files):
        with open(path, 'wb') as f:
            for u in range(n_units):
                read = reads[mates * u + s]
                f.write(b'@' + names[u] + b'\n' + read + b'\n+\n' + b'@' * len(read) + b'\n')
    feeder = common.PackedReadFeeder(files, paired, threads=2, chunk_bytes=50_000)
    same(mapper.map_reads(index, feeder, strand=mode))
    one.reset()
    rm(common.PackedReadFeeder(files, paired, threads=2, chunk_bytes=50_000))
    same(one)
    one.reset()
    for piece in common.PackedReadFeeder(files, paired, threads=2, chunk_bytes=50_000):
        rm.push_packed(piece)                                 # piece by piece through Python
    same(one)

    # -m: the ASCII reader's batches, readmap.txt from the filtered tuples
    readmap = tmp_path / 'readmap.txt'
    text = mapper.map_reads(index, common.NativeReadFeeder(files, paired=paired), readmap=readmap.open('wt'),
                            strand=mode)
    same(text)
    lines = readmap.read_text().splitlines()
    assert len(lines) == n_units
    for line, name, t in zip(lines, names, filtered.tuples()):
        assert line.split('\t') == [name.decode()] + [chr21[0][i].decode() for i in t]


def test_two_wave_class_insertion_at_full_size(native_libs):
    """A batch of 2^21 pairs on an empty table goes in two waves of class insertion: in mode fr its
    table equals the unstranded run's tuples, filtered on the host and counted by MapResult.update
    (the unstranded mapping is pinned to the oracle at this scale by the parity suite)."""
    from seekmer_amd import common, index_builder, mapper, synth
    ids, pool, tx_offsets = synth.transcriptome(9, 400)
    index = index_builder.build_pooled(ids, pool, tx_offsets)
    n_units = 1 << 21
    bases, offsets = synth.reads(9, pool, tx_offsets, 0, n_units, 100, True)
    batch = common.ReadBatch(n_units, bases, offsets, True)
    plain = mapper.MapResult(index)
    rm = mapper.ReadMapper(index, plain)
    rm.map_batch(batch)
    counts, entries = rm.last_tuples(n_units)
    filtered = filter_units(counts, entries, 'fr')
    assert (filtered.count == 0).sum() > n_units // 4        # unstranded reads: about half emptied

    stranded = mapper.MapResult(index, strand='fr')
    srm = mapper.ReadMapper(index, stranded)
    srm.map_batch(batch)
    s_counts, s_entries = srm.last_tuples(n_units)
    np.testing.assert_array_equal(s_counts, filtered.count)
    np.testing.assert_array_equal(s_entries, filtered.entries)
    expected = mapper.MapResult(index)
    expected.update([None] * n_units, filtered.tuples())
    got, want = stranded.export(), expected.export()
    for k in range(4):                                        # offsets, ids, counts, first_seen
        np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(got[4], plain.export()[4])  # the unstranded histogram
    assert stranded.sizes() == expected.sizes()


def test_state_rules(oracle, native_libs, antisense):
    from seekmer_amd import _native, common, mapper
    ids, seqs, oindex = antisense
    index = make_product_index(oindex, ids)
    reads, _ = stranded_reads(seqs, np.random.default_rng(8), 2000, True, 'fr')
    bases, offsets = oracle.pack_reads(reads)
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(oindex, bases, offsets, 2000, True, fld)
    batch = common.ReadBatch(2000, bases, offsets, True)
    hip = _native.hip()

    result = mapper.MapResult(index)
    h = result._handle
    assert hip.skm_mapper_set_strand(h, 1) == _native.SKM_OK          # a new handle
    assert hip.skm_mapper_set_strand(h, 3) == _native.SKM_ERR_ARG
    assert hip.skm_mapper_set_strand(h, -1) == _native.SKM_ERR_ARG
    rm = mapper.ReadMapper(index, result)
    rm.map_batch(batch)
    _same_table(oracle, result, filter_result(expected, 'fr'), fld)
    assert hip.skm_mapper_set_strand(h, 2) == _native.SKM_ERR_STATE    # the handle holds units
    assert hip.skm_mapper_set_strand(h, 1) == _native.SKM_ERR_STATE
    assert hip.skm_mapper_set_strand(h, 3) == _native.SKM_ERR_ARG
    result.reset()                                                      # the mode survives reset
    rm.map_batch(batch)
    _same_table(oracle, result, filter_result(expected, 'fr'), fld)
    result.clear()                                                      # ... and clear (which keeps the FLD)
    rm.map_batch(batch)
    _same_table(oracle, result, filter_result(expected, 'fr'), 2 * fld)
    result.clear()
    assert hip.skm_mapper_set_strand(h, 2) == _native.SKM_OK
    rm.map_batch(batch)
    _same_table(oracle, result, filter_result(expected, 'rf'), 3 * fld)      # (three batches since the reset)
    result.reset()
    assert hip.skm_mapper_set_strand(h, 0) == _native.SKM_OK            # back to unstranded
    rm.map_batch(batch)
    classes = oracle.Classes()
    classes.update(expected)
    assert result.sizes()[:3] == (classes.export()[2].size, classes.export()[1].size, classes.unaligned)
    # a queued batch: the mode cannot change under it
    result.reset()
    rm.map_batch_async(batch)
    assert hip.skm_mapper_set_strand(h, 1) == _native.SKM_ERR_STATE
    result.sync()
    with pytest.raises(ValueError):
        mapper.MapResult(index, strand='both')


def _write_fastq(path, names, reads):
    with open(path, 'wb') as f:
        for name, read in zip(names, reads):
            f.write(b'@' + name + b'\n' + read + b'\n+\n' + b'I' * len(read) + b'\n')


def _check_abundance(path, ids, lengths, eff, tpm, est):
    rows = [line.rstrip('\n').split('\t') for line in open(path)]
    assert rows[0] == ['target_id', 'length', 'eff_length', 'est_count', 'tpm']
    assert len(rows) == 1 + len(ids)
    for i, row in enumerate(rows[1:]):
        assert row[0] == ids[i].decode()
        assert row[1] == '%g' % lengths[i]
        assert row[2] == '%g' % np.float32(eff[i])
        assert abs(float(row[3]) - est[i]) <= 1e-4 * max(est[i], 1e-300) + 1e-6
        assert abs(float(row[4]) - tpm[i]) <= 1e-4 * max(tpm[i], 1e-300) + 1e-6
    return rows


@pytest.mark.parametrize('flag,mode,aligned', [('--fr-stranded', 'fr', 11), ('--rf-stranded', 'rf', 10)])
def test_cli_end_to_end(oracle, native_libs, chr21, chr21_oracle_index, pairs21, tmp_path, flag, mode, aligned):
    """`seekmer_amd infer <flag> -m -b 2` on the reference's own 21 pairs: run_info, abundance.tsv,
    readmap.txt and aux/fld against the oracle's filtered table and its unstranded histogram."""
    from seekmer_amd import __main__ as cli
    gtf = tmp_path / 'empty.gtf'
    gtf.write_text('')
    index_path = tmp_path / 'index.npz'
    assert cli.main(['index', '-t', os.path.join(GOLDEN, 'human.cdna.21.fa.bz2'), str(gtf), str(index_path)]) == 0
    out = tmp_path / 'out'
    assert cli.main(['infer', str(index_path), str(out), os.path.join(GOLDEN, '20_1.fastq'),
                     os.path.join(GOLDEN, '20_2.fastq'), flag, '-m', '-b', '2', '--seed', '7']) == 0

    bases, offsets = oracle.pack_reads(pairs21)
    fld = np.zeros(2000, dtype=np.int64)
    expected = oracle.map_batch(chr21_oracle_index, bases, offsets, 21, True, fld)
    filtered = filter_result(expected, mode)
    classes = _expected_table(oracle, filtered)
    class_map, class_count = classes.summarize()
    eff = oracle.effective_lengths(fld, chr21_oracle_index.lengths)
    tpm, _ = oracle.quantify(eff, class_map, class_count)
    est = oracle.est_counts(tpm, chr21_oracle_index.lengths, class_count.sum())
    _check_abundance(out / 'abundance.tsv', chr21[0], [len(s) for s in chr21[1]], eff, tpm, est)
    info = json.load((out / 'run_info.json').open())
    assert info['n_processed'] == 21 and info['n_pseudoaligned'] == aligned and info['n_bootstraps'] == 2
    readmap = (out / 'readmap.txt').read_text().splitlines()
    names = [line.strip()[1:].decode() for i, line in
             enumerate(open(os.path.join(GOLDEN, '20_1.fastq'), 'rb')) if i & 3 == 0]
    assert len(readmap) == 21
    for line, name, t in zip(readmap, names, filtered.tuples()):
        assert line.split('\t') == [name] + [chr21[0][i].decode() for i in t]
    arrays = np.load(out / 'abundance.npz')
    np.testing.assert_array_equal(arrays['aux/fld'], fld.astype('i4'))


def test_antisense_decoy_through_the_cli(oracle, native_libs, antisense, tmp_path):
    """A transcript that is the reverse complement of a stretch of another and has no reads of its
    own: unstranded it gets a class (and abundance); --fr-stranded gives it a TPM of exactly 0."""
    from seekmer_amd import __main__ as cli
    ids, seqs, oindex = antisense
    fasta = tmp_path / 'tx.fa'
    fasta.write_bytes(b''.join(b'>' + i + b'\n' + s + b'\n' for i, s in zip(ids, seqs)))
    gtf = tmp_path / 'empty.gtf'
    gtf.write_text('')
    index_path = tmp_path / 'index.npz'
    assert cli.main(['index', '-t', str(fasta), str(gtf), str(index_path)]) == 0
    reads, _ = stranded_reads(seqs, np.random.default_rng(21), 3000, True, 'fr')
    names = [b'p%d' % u for u in range(3000)]
    files = [tmp_path / 'r_1.fastq', tmp_path / 'r_2.fastq']
    for s in range(2):
        _write_fastq(files[s], names, reads[s::2])
    stranded, plain = tmp_path / 'stranded', tmp_path / 'plain'
    assert cli.main(['infer', str(index_path), str(stranded), *map(str, files), '--fr-stranded']) == 0
    assert cli.main(['infer', str(index_path), str(plain), *map(str, files), '-m']) == 0
    rows = [line.rstrip('\n').split('\t') for line in (stranded / 'abundance.tsv').open()]
    assert rows[1 + DECOY][0] == ids[DECOY].decode() and float(rows[1 + DECOY][4]) == 0.0
    readmap = [line.split('\t') for line in (plain / 'readmap.txt').read_text().splitlines()]
    assert any(ids[DECOY].decode() in line[1:] for line in readmap)
    rows = [line.rstrip('\n').split('\t') for line in (plain / 'abundance.tsv').open()]
    assert float(rows[1 + DECOY][4]) > 0


def test_impute_cells_are_stranded(oracle, native_libs, antisense, tmp_path):
    """map_multiple_samples(..., strand='fr'), as impute.run calls it: every cell's table is its
    filtered oracle table."""
    from seekmer_amd import common, mapper
    ids, seqs, oindex = antisense
    index = make_product_index(oindex, ids)
    feeders, expected = [], []
    for cell in range(2):
        reads, _ = stranded_reads(seqs, np.random.default_rng(40 + cell), 2500, True, 'fr')
        names = [b'c%d_%d' % (cell, u) for u in range(2500)]
        files = [tmp_path / ('c%d_%d.fastq' % (cell, s)) for s in (1, 2)]
        for s in range(2):
            _write_fastq(files[s], names, reads[s::2])
        feeders.append(common.PackedReadFeeder(files, paired=True))
        bases, offsets = oracle.pack_reads(reads)
        fld = np.zeros(2000, dtype=np.int64)
        result = oracle.map_batch(oindex, bases, offsets, 2500, True, fld)
        expected.append((filter_result(result, 'fr'), fld))
    results = mapper.map_multiple_samples(index, feeders, job_count=2, strand='fr')
    for result, (filtered, fld) in zip(results, expected):
        _same_table(oracle, result, filtered, fld)
        assert all(DECOY not in t for t in filtered.tuples())
