"""UMI collapse on the GPU ("UMI collapse") against tests/umi_reference.py, exactly.

The classes the reference collapses by come from the oracle (oracle.map_batch on the oracle index of the same
sequences, strand_reference.filter_result for the stranded cases), never from the code under test.  A sample set
that keeps UMIs must give, bit for bit, what a plain set gives that is fed the reference's survivors alone; and
`infer-many --barcodes ... --umi-length L` on pooled files must write, for every cell, what `infer-many` writes for
FASTQ files that hold exactly the cell's surviving units in order."""
import ctypes
import json

import numpy as np
import pytest

import umi_reference as ref
from conftest import make_product_index
from strand_reference import filter_result

pytestmark = pytest.mark.gpu

BASES = 'ACGT'


# ---- the generator of tests/test_gpu_barcodes.py (a copy: that file is free to change) ----------------------------
def _random_barcodes(rng, n, length):
    """n distinct barcodes of `length` bases"""
    seen = set()
    while len(seen) < n:
        seen.update(''.join(row) for row in rng.choice(list(BASES), size=(n - len(seen), length)))
    return sorted(seen, key=lambda _: rng.random())


def _substitute(rng, barcode, places):
    out = list(barcode)
    for p in rng.choice(len(barcode), size=places, replace=False):
        out[p] = rng.choice([b for b in BASES if b != out[p]])
    return ''.join(out)


def _barcode_reads(rng, whitelist, start, n):
    """n barcode reads around the whitelist: exact entries, every kind of damage, every kind of length"""
    length = len(whitelist[0])
    text = lambda k: ''.join(rng.choice(list(BASES), size=k))
    reads = []
    kinds = rng.choice(11, size=n, p=[.22, .12, .14, .08, .08, .06, .08, .08, .05, .04, .05])
    for kind in kinds:
        entry = whitelist[rng.integers(len(whitelist))]
        window, prefix, suffix = entry, text(start), text(rng.integers(0, 11))
        if kind == 1:
            window = _substitute(rng, entry, 1)
        elif kind == 2:
            window = _substitute(rng, entry, min(2, length))
        elif kind == 3 or (kind == 4 and length == 1):
            p = rng.integers(length)
            window = entry[:p] + 'N' + entry[p + 1:]
        elif kind == 4:
            p, q = rng.choice(length, size=2, replace=False)
            window = ''.join('N' if i in (p, q) else c for i, c in enumerate(entry))
        elif kind == 5:
            p = rng.integers(length)
            window = entry[:p] + entry[p].lower() + entry[p + 1:]
        elif kind == 6:           # a base that is not clean just outside the window: it must not matter
            if start and rng.random() < 0.5:
                prefix = prefix[:-1] + 'N'
            else:
                suffix = 'n' + suffix
        elif kind == 7:
            suffix, window = '', entry[:-1]                           # start + L - 1 bases
        elif kind == 8:
            suffix = ''                                                 # start + L bases
        elif kind == 9:
            prefix = window = suffix = ''                               # no bases at all
        elif kind == 10:
            window = text(length)
        reads.append(prefix + window + suffix)
    return reads


def _piece(reads, stride_extra=0):
    """the reads (str) as a packed piece; stride_extra > 0: its codes lie `stride_extra` words further apart"""
    from seekmer_amd import _native
    from seekmer_amd.common import PackedReads
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    bases = np.frombuffer((''.join(reads) + 'A').encode(), dtype=np.uint8)
    piece = PackedReads.from_ascii(bases, offsets)
    if not stride_extra or not reads:
        return piece
    codes, lengths, exception_reads, exception_masks = piece._keep
    stride = codes.shape[1] + stride_extra
    wide = np.full((len(reads), stride), 0x5555555555555555, dtype=np.uint64)
    wide[:, :codes.shape[1]] = codes
    raw = _native.PackedReads()
    ctypes.memmove(ctypes.byref(raw), ctypes.byref(piece.raw), ctypes.sizeof(raw))
    raw.read_stride, raw.codes = stride, wide.ctypes.data
    return PackedReads(raw, keep=(wide, lengths, exception_reads, exception_masks))


# ---- windows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_reads', [0, 1, 255, 256, 257, 3000])
@pytest.mark.parametrize('length, start', [(1, 0), (12, 16), (12, 28), (16, 0), (16, 17)])
def test_windows_are_the_reference(native_libs, length, start, n_reads):
    """every kind of read the barcode generator makes, around the UMI window; strided codes; cell passed or not"""
    from seekmer_amd import mapper
    rng = np.random.default_rng(1000 * length + 10 * start + n_reads)
    reads = _barcode_reads(rng, _random_barcodes(rng, 4 if length == 1 else 200, length), start, n_reads)
    umi, readable = ref.windows(reads, start, length)
    if n_reads >= 255:
        assert 0.5 < readable.mean() < 0.8 and len(set(umi[readable].tolist())) >= min(4, 4 ** length)
    piece = _piece(reads, stride_extra=3)
    got, unreadable = mapper.umi_windows(piece, start, length)
    np.testing.assert_array_equal(got, umi)
    assert got.dtype == np.uint32 and unreadable == int((~readable).sum())
    cell = rng.integers(-1, 7, size=n_reads).astype(np.int32)
    want_cell = np.where(readable, cell, -1)
    got, unreadable = mapper.umi_windows(piece, start, length, cell=cell)
    np.testing.assert_array_equal(got, umi)
    np.testing.assert_array_equal(cell, want_cell)
    assert unreadable == int((~readable).sum())


def test_windows_refuse_what_cannot_be(native_libs):
    from seekmer_amd import mapper
    piece = _piece(['ACGTACGT'] * 3)
    for start, length in ((0, 0), (0, 17), (-1, 4)):
        with pytest.raises(ValueError):
            mapper.umi_windows(piece, start, length)


# ---- the set, directly --------------------------------------------------------------------------------------------
READ_LEN = 75
UMI_ZERO, UMI_ONES = 0, 2 ** 32 - 1


@pytest.fixture(scope='module')
def transcriptome(oracle, native_libs):
    """synth.transcriptome(5, 30): (ids, pool, tx_offsets, oracle index, product index over the same arrays)"""
    from seekmer_amd import synth
    ids, pool, tx_offsets = synth.transcriptome(5, 30)
    oindex = oracle.build_index(synth.sequences_of(pool, tx_offsets), ids)
    return ids, pool, tx_offsets, oindex, make_product_index(oindex, ids)


def _pairs(pool, tx_offsets, seed, first, n):
    from seekmer_amd import synth
    raw = synth.reads(seed, pool, tx_offsets, first, n, READ_LEN, True)[0][:-1].tobytes()
    return [(raw[2 * u * READ_LEN:(2 * u + 1) * READ_LEN], raw[(2 * u + 1) * READ_LEN:(2 * u + 2) * READ_LEN]) for u in range(n)]


@pytest.fixture(scope='module')
def molecules(oracle, transcriptome):
    """Three samples of units (pair, UMI) in which pairs are repeated verbatim, and the reference's answer for the
    unstranded and the rf library.  Everything the set has to get right lies in samples 0 and 1:
      A  copies next to each other            B  copies more than 1024 units apart
      C  2000 copies (sample 0 only)          D  the same (UMI, class) in samples 0 and 1
      E  one UMI with two classes             F  200 unaligned random reads that share one UMI
      G  UMI 0 and UMI 2^32 - 1, both with copies"""
    ids, pool, tx_offsets, oindex, index = transcriptome
    rng = np.random.default_rng(99)
    samples, named = [], None
    for s in range(3):
        distinct = _pairs(pool, tx_offsets, 40 + s, s * 5000, 960)
        # the named molecules are aligned ones, E's two of different classes: by the oracle
        classes = oracle.map_batch(oindex, *oracle.pack_reads([read for pair in distinct[:60] for read in pair]), 60, True).tuples()
        aligned = [i for i, t in enumerate(classes) if t]
        other = next(i for i in aligned[7:] if classes[i] != classes[aligned[6]])
        chosen = aligned[:7] + [other]
        filler = []
        for pair in distinct[60:]:            # every filler molecule 1 to 4 times (mean 2), all over the sample
            filler += [(pair, int(rng.integers(1, 2 ** 32 - 1)))] * int(rng.choice([1, 2, 3, 4], p=[.4, .3, .2, .1]))
        filler = [filler[i] for i in rng.permutation(len(filler))]
        if s == 2:
            samples.append(filler)
            continue
        a, b, c, d, g0, g1, e1, e2 = [distinct[i] for i in chosen]
        if s == 1:
            d = named[3]
        noise = [(bytes(b'ACGT'[int(x)] for x in rng.integers(0, 4, READ_LEN)), bytes(b'ACGT'[int(x)] for x in rng.integers(0, 4, READ_LEN)))
                 for _ in range(200)]
        units = [(a, 11), (a, 11), (a, 11), (b, 12), (c, 13)] + filler[:40] + [(d, 14), (e1, 15), (e2, 15), (g0, UMI_ZERO), (g1, UMI_ONES)]
        units += filler[40:1080] + [(b, 12), (d, 14), (g0, UMI_ZERO), (g1, UMI_ONES), (g1, UMI_ONES)] + filler[1080:]
        late = [(c, 13)] * (1999 if s == 0 else 0) + [(pair, 16) for pair in noise]
        for item, at in zip(late, np.sort(rng.integers(5, len(units), size=len(late)))[::-1]):
            units.insert(int(at), item)
        if s == 0:
            named = (a, b, c, d, e1, e2, g0, g1)
        samples.append(units)
    reads = [read for units in samples for pair, _ in units for read in pair]
    sample = np.repeat(np.arange(3), [len(units) for units in samples]).astype(np.int32)
    umi = np.asarray([m for units in samples for _, m in units], dtype=np.uint32)
    bases, offsets = oracle.pack_reads(reads)
    mapped = oracle.map_batch(oindex, bases, offsets, sample.size, True)
    tuples = {None: mapped.tuples(), 'rf': filter_result(mapped, 'rf').tuples()}
    stay = {strand: ref.survivors(sample, umi, t) for strand, t in tuples.items()}
    return dict(samples=samples, sample=sample, umi=umi, tuples=tuples, stay=stay, index=index, named=named)


def test_the_molecules_are_not_trivial(molecules):
    """the reference alone: what the set is asked is in the input"""
    samples, sample, umi, tuples, stay = (molecules[k] for k in ('samples', 'sample', 'umi', 'tuples', 'stay'))
    a, b, c, d, e1, e2, g0, g1 = molecules['named']
    first = samples[0]
    of = lambda pair, m: [u for u, item in enumerate(first) if item == (pair, m)]
    klass = lambda pair: tuples[None][next(u for u, item in enumerate(first) if item[0] == pair)]
    for pair in (a, b, c, d, e1, e2, g0, g1):
        assert klass(pair), 'the named molecules are aligned'
        assert all(tuples[None][u] == klass(pair) for u, item in enumerate(first) if item[0] == pair), 'verbatim repeats share a class'
    assert of(a, 11)[:3] == [0, 1, 2]
    assert np.diff(of(b, 12)).max() > 1024
    assert len(of(c, 13)) == 2000 and stay[None][of(c, 13)].tolist() == [True] + [False] * 1999
    assert klass(e1) != klass(e2) and stay[None][of(e1, 15)].all() and stay[None][of(e2, 15)].all()
    second = np.flatnonzero(sample == 1)[0]
    in_second = [int(second) + u for u, item in enumerate(samples[1]) if item == (d, 14)]
    assert stay[None][of(d, 14)[0]] and stay[None][in_second[0]] and not stay[None][in_second[1]]
    noise = [u for u, item in enumerate(first) if item[1] == 16]
    assert len(noise) == 200 and all(not tuples[None][u] for u in noise) and stay[None][noise].all()
    assert len(of(g0, UMI_ZERO)) == 2 and len(of(g1, UMI_ONES)) == 3
    assert stay[None][of(g0, UMI_ZERO)].tolist() == [True, False] and stay[None][of(g1, UMI_ONES)].tolist() == [True, False, False]
    for strand in (None, 'rf'):
        aligned = np.asarray([bool(t) for t in tuples[strand]])
        assert 0.25 <= (aligned & ~stay[strand]).sum() / aligned.sum() <= 0.75, strand
        assert not (~aligned & ~stay[strand]).any(), 'an unaligned unit is never removed'
        for s in range(3):
            mine = sample == s
            assert (mine & aligned & ~stay[strand]).sum() >= 100 and mine.sum() >= 1100


def _add_sample(sample_set, s, units, umis=None, cuts=()):
    """the units (pair, umi) of sample s as packed segments cut at `cuts`"""
    from seekmer_amd import common
    from oracle import oracle
    bounds = [0] + list(cuts) + [len(units)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        pieces = [common.PackedReads.from_ascii(*oracle.pack_reads([pair[mate] for pair, _ in units[lo:hi]]), stream=mate)
                  for mate in (0, 1)]
        if umis is None:
            sample_set.add_packed(s, lo, *pieces)
        else:
            sample_set.add_packed(s, lo, *pieces, umis=np.asarray(umis[lo:hi], dtype=np.uint32))


def _state(sample_set):
    summaries = sample_set.summarize()
    fields = ('aligned', 'unaligned', 'total', 'class_map', 'class_count', 'fragment_length_frequencies', 'effective_lengths',
              'class_offsets', 'class_targets')
    out = {'summary %d %s' % (i, f): np.asarray(getattr(s, f)) for i, s in enumerate(summaries) for f in fields}
    out.update(fld=sample_set.sample_fragment_length_counts, bias=sample_set.bias_observed(), sizes=sample_set.sizes())
    out.update({'first seen %d' % i: table[3] for i, table in enumerate(sample_set.export())})
    return out


@pytest.fixture(scope='module')
def expected(molecules):
    """a plain set fed the reference's survivors alone, per strand: computed once"""
    from seekmer_amd import mapper
    out = {}
    for strand in (None, 'rf'):
        plain = mapper.SampleSet(molecules['index'], True, strand=strand, per_sample_lengths=True, bias=True)
        at = 0
        for s, units in enumerate(molecules['samples']):
            stay = molecules['stay'][strand][at:at + len(units)]
            _add_sample(plain, s, [unit for unit, keep in zip(units, stay) if keep])
            at += len(units)
        assert plain.umi_removed().tolist() == [0, 0, 0]
        out[strand] = _state(plain)
        del plain
    return out


def _collapsed_state(molecules, strand=None, cuts=()):
    from seekmer_amd import mapper
    sample_set = mapper.SampleSet(molecules['index'], True, strand=strand, per_sample_lengths=True, bias=True, umi_bases=16)
    order = [1, 0, 2]                         # (the samples in any order; sample 0's segments in theirs)
    for s in order:
        units = molecules['samples'][s]
        _add_sample(sample_set, s, units, umis=[m for _, m in units], cuts=cuts if s == 0 else ())
    state = _state(sample_set)
    state['removed'] = sample_set.umi_removed()
    return state


def _assert_collapsed(molecules, expected, strand=None, cuts=()):
    got = _collapsed_state(molecules, strand, cuts)
    sample, stay = molecules['sample'], molecules['stay'][strand]
    want_removed = [int(((sample == s) & ~stay).sum()) for s in range(3)]
    print('removed', got['removed'].tolist(), 'reference', want_removed, 'units', np.bincount(sample).tolist())
    np.testing.assert_array_equal(got.pop('removed'), want_removed)
    assert sorted(got) == sorted(expected[strand])
    for s in range(3):                        # first-seen units count the units as added: here, as the survivors' numbers
        rank = np.cumsum(stay[sample == s]) - 1
        assert stay[sample == s][got['first seen %d' % s]].all(), 'a removed unit is no class\'s first'
        got['first seen %d' % s] = rank[got['first seen %d' % s]]
    for name, want in expected[strand].items():
        np.testing.assert_array_equal(got[name], want, err_msg=name)


@pytest.mark.parametrize('hook', [None, 'SKM_SAMPLE_SET_MAX_UNITS=500', 'SKM_TEST_UMI_SLOTS=2', 'SKM_TEST_MAP_BLOCKS=1'])
def test_a_set_with_umis_is_the_plain_set_of_the_survivors(molecules, expected, monkeypatch, hook):
    """launches of 500 units: molecules straddle launches; 2 slots: the molecule set grows under every launch"""
    for name in ('SKM_SAMPLE_SET_MAX_UNITS', 'SKM_TEST_UMI_SLOTS', 'SKM_TEST_MAP_BLOCKS'):
        monkeypatch.delenv(name, raising=False)
    if hook:
        monkeypatch.setenv(*hook.split('='))
    _assert_collapsed(molecules, expected)


def test_a_segment_split_in_the_middle_of_a_molecule(molecules, expected, monkeypatch):
    monkeypatch.delenv('SKM_TEST_UMI_SLOTS', raising=False)
    _assert_collapsed(molecules, expected, cuts=(2, 1700))          # between the copies of A; among the copies of C


def test_collapse_follows_the_strand_filter(molecules, expected, monkeypatch):
    monkeypatch.setenv('SKM_SAMPLE_SET_MAX_UNITS', '500')
    assert any(a != b for a, b in zip(molecules['tuples'][None], molecules['tuples']['rf']))
    _assert_collapsed(molecules, expected, strand='rf')


def test_refusals(molecules, native_libs):
    from seekmer_amd import mapper
    index, units = molecules['index'], molecules['samples'][2][:10]
    with pytest.raises(native_libs.NativeError) as error:            # without histograms per sample
        mapper.SampleSet(index, True, umi_bases=12)
    assert error.value.code == native_libs.SKM_ERR_STATE
    plain = mapper.SampleSet(index, True, per_sample_lengths=True)
    _add_sample(plain, 0, units)
    assert native_libs.hip().skm_sample_set_keep_umis(plain._handle, 12) == native_libs.SKM_ERR_STATE     # after a segment
    with pytest.raises(ValueError):                                   # UMIs for a set that keeps none
        _add_sample(plain, 1, units, umis=[1] * 10)
    with_umis = mapper.SampleSet(index, True, per_sample_lengths=True, umi_bases=4)
    with pytest.raises(ValueError, match='takes its reads with them'):
        _add_sample(with_umis, 0, units)
    with pytest.raises(ValueError, match='does not fit'):
        _add_sample(with_umis, 0, units, umis=[256] * 10)
    with pytest.raises(ValueError):
        mapper.SampleSet(index, True, per_sample_lengths=True, umi_bases=17)
    _add_sample(with_umis, 0, units, umis=[255] * 10)
    assert with_umis.sizes()[0, 3] + with_umis.umi_removed()[0] == 10


# ---- end to end ---------------------------------------------------------------------------------------------------
CELL_PAIRS = (2000, 3500, 4000, 0, 2500, 3000)          # original pairs; cell 3 is on the whitelist and has no reads
BARCODE_LENGTH = 12


def _write_fastq(path, reads):
    with open(path, 'w') as f:
        for i, read in enumerate(reads):
            f.write('@r%d\n%s\n+\n%s\n' % (i, read, 'I' * len(read)))


def _pooled(oracle, transcriptome, folder, umi_length):
    """The pooled fixture of tests/test_gpu_barcodes.py with duplication: every original pair is written k times with
    one UMI, k from {1, 2, 3, 4} with probabilities (.4, .3, .2, .1); barcode reads = GGA + barcode (start 3) + UMI
    (start 15) + a tail; 2 % of them carry an N or a lower-case letter in the UMI; everything shuffled.  The
    reference's answer for the paired, the single-ended and the rf library, and one FASTQ pair per cell and library
    with the survivors (plus one of all the cell's units, uncollapsed)."""
    from seekmer_amd import index_builder, synth
    import barcode_reference
    ids, pool, tx_offsets, oindex, _ = transcriptome
    index_path = folder / 'index.npz'
    index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    rng = np.random.default_rng(2024 + umi_length)
    while True:                    # barcodes at distance >= 3 from each other: a substitution never reaches another cell
        whitelist = _random_barcodes(rng, len(CELL_PAIRS), BARCODE_LENGTH)
        if all(sum(a != b for a, b in zip(x, y)) >= 3 for i, x in enumerate(whitelist) for y in whitelist[:i]):
            break
    names = ['cell%d' % c for c in range(len(CELL_PAIRS))]
    (folder / 'whitelist.tsv').write_text(''.join('%s\t%s\n' % row for row in zip(whitelist, names)))
    mates, truth, umis = ([], []), [], []
    for c, n_pairs in enumerate(CELL_PAIRS):
        if not n_pairs:
            continue
        raw = synth.reads(100 + c % 2, pool, tx_offsets, c * 8000, n_pairs, READ_LEN, True)[0][:-1].tobytes().decode()
        shared = ''.join(rng.choice(list(BASES), size=umi_length))
        for u in range(n_pairs):
            k = int(rng.choice([1, 2, 3, 4], p=[.4, .3, .2, .1]))
            # (the first 20 pairs of a cell share one UMI: one UMI, many classes)
            molecule = shared if u < 20 else ''.join(rng.choice(list(BASES), size=umi_length))
            pair = [raw[(2 * u + mate) * READ_LEN:(2 * u + mate + 1) * READ_LEN] for mate in (0, 1)]
            # (pairs 20 .. 39 of cell 0 are also in cell 1 with their UMI, twice: one (UMI, class), two cells)
            for cell_, copies in ((c, k), (1, 2)) if c == 0 and 20 <= u < 40 else ((c, k),):
                for mate in (0, 1):
                    mates[mate].extend([pair[mate]] * copies)
                truth += [cell_] * copies
                umis += [molecule] * copies
    shuffle = rng.permutation(len(truth))
    mates = [[mate[u] for u in shuffle] for mate in mates]
    barcodes = []
    for u in shuffle:
        barcode, molecule, chance = whitelist[truth[u]], umis[u], rng.random()
        if 0.85 <= chance < 0.95:
            barcode = _substitute(rng, barcode, 1)
        elif chance >= 0.95:
            barcode = [_substitute(rng, barcode, 2), ''.join(rng.choice(list(BASES), size=BARCODE_LENGTH)),
                       'N' + barcode[1:], barcode[:4] + 'NN' + barcode[6:]][rng.integers(4)]
        if rng.random() < 0.02:
            p = rng.integers(umi_length)
            molecule = molecule[:p] + ('N' if rng.random() < 0.5 else molecule[p].lower()) + molecule[p + 1:]
        barcodes.append('GGA' + barcode + molecule + ''.join(rng.choice(list(BASES), size=8)))
    _write_fastq(folder / 'pool_1.fastq', mates[0])
    _write_fastq(folder / 'pool_2.fastq', mates[1])
    _write_fastq(folder / 'barcodes.fastq', barcodes)
    cell, cell_assigned, stats = barcode_reference.assign(whitelist, barcodes, start=3, mismatches=1)
    umi, readable = ref.windows(barcodes, 3 + BARCODE_LENGTH, umi_length)
    cell = np.where(readable, cell, -1)
    cell_units = np.bincount(cell[cell >= 0], minlength=len(whitelist))
    n = len(barcodes)
    paired = oracle.map_batch(oindex, *oracle.pack_reads([m.encode() for pair in zip(*mates) for m in pair]), n, True)
    single = oracle.map_batch(oindex, *oracle.pack_reads([m.encode() for m in mates[0]]), n, False)
    tuples = {'paired': paired.tuples(), 'single': single.tuples(), 'rf': filter_result(paired, 'rf').tuples()}
    stay = {library: ref.survivors(cell, umi, t) for library, t in tuples.items()}
    stay['uncollapsed'] = cell >= 0
    for library, mask in stay.items():
        for c in np.flatnonzero(cell_units):
            for mate in (0, 1):
                _write_fastq(folder / ('%s_%s_%d.fastq' % (library, names[c], mate + 1)),
                             [mates[mate][u] for u in np.flatnonzero(mask & (cell == c))])
    return dict(folder=folder, index=index_path, whitelist=whitelist, names=names, cell=cell, umi=umi, cell_assigned=cell_assigned,
                cell_units=cell_units, stats=stats, unreadable=int((~readable).sum()), tuples=tuples, stay=stay,
                umi_length=umi_length, ids=ids)


@pytest.fixture(scope='module')
def pooled(oracle, transcriptome, tmp_path_factory):
    return _pooled(oracle, transcriptome, tmp_path_factory.mktemp('pooled_umi12'), 12)


@pytest.fixture(scope='module')
def pooled_short(oracle, transcriptome, tmp_path_factory):
    """UMIs of 4 bases: different molecules of a cell share UMIs by chance"""
    return _pooled(oracle, transcriptome, tmp_path_factory.mktemp('pooled_umi4'), 4)


@pytest.mark.parametrize('which', ['pooled', 'pooled_short'])
def test_the_pooled_fixtures_are_not_trivial(request, which):
    """the reference alone: a do-nothing and a drop-everything implementation both fail what follows"""
    fixture = request.getfixturevalue(which)
    cell, umi, kept = fixture['cell'], fixture['umi'], np.flatnonzero(fixture['cell_units'])
    assert fixture['unreadable'] > 0 and len(kept) == 5
    for library in ('paired', 'single', 'rf'):
        tuples, stay = fixture['tuples'][library], fixture['stay'][library]
        aligned = np.asarray([bool(t) for t in tuples]) & (cell >= 0)
        removed = aligned & ~stay
        assert 0.25 <= removed.sum() / aligned.sum() <= 0.75, library
        assert all((removed & (cell == c)).sum() >= 100 for c in kept), library
        molecules = {}
        for u in np.flatnonzero(aligned):
            molecules.setdefault((int(cell[u]), int(umi[u]), tuples[u]), []).append(int(u))
        assert any(units[0] // 1000 != units[-1] // 1000 for units in molecules.values()), 'copies in different chunks'
        by_umi, by_class = {}, {}
        for c, m, t in molecules:
            by_umi.setdefault((c, m), set()).add(t)
            by_class.setdefault((m, t), set()).add(c)
        assert any(len(classes) > 1 for classes in by_umi.values()), 'a UMI shared by two classes of a cell'
        assert any(len(cells) > 1 for cells in by_class.values()), 'a (UMI, class) shared by two cells'
        if which == 'pooled_short':           # 256 UMIs: a cell's UMIs are shared by many classes, not by the planted ones alone
            assert sum(len(classes) > 1 for classes in by_umi.values()) > 500


def _run(fixture, out, files, extra, names=None):
    from seekmer_amd.__main__ import main
    assert main(['infer-many', str(fixture['index']), str(out), *map(str, files), '-b', '2', '--seed', '7', *extra,
                 *(['--names', ','.join(names)] if names else [])]) == 0
    return out


def _per_cell_run(fixture, out, library, single=False, extra=()):
    """infer-many on the reference's per-cell files of `library`"""
    folder = fixture['folder']
    kept = [fixture['names'][c] for c in np.flatnonzero(fixture['cell_units'])]
    files = [folder / ('%s_%s_%d.fastq' % (library, name, mate)) for name in kept for mate in ((1,) if single else (1, 2))]
    return _run(fixture, out, files, [*(['-s'] if single else []), *extra], names=kept)


def _pooled_run(fixture, out, single=False, extra=()):
    folder = fixture['folder']
    files = [folder / 'pool_1.fastq'] + ([] if single else [folder / 'pool_2.fastq'])
    return _run(fixture, out, files, ['--barcodes', str(folder / 'whitelist.tsv'), '--barcode-file', str(folder / 'barcodes.fastq'),
                                      '--barcode-start', '3', '--umi-start', str(3 + BARCODE_LENGTH), '--umi-length',
                                      str(fixture['umi_length']), *(['-s'] if single else []), *extra])


def _assert_same_run(fixture, ours, theirs, library):
    from test_gpu_infer_many import _assert_same_outputs
    kept = np.flatnonzero(fixture['cell_units'])
    for c in kept:
        _assert_same_outputs(ours / fixture['names'][c], theirs / fixture['names'][c])
    assert (ours / 'samples.tsv').read_bytes() == (theirs / 'samples.tsv').read_bytes()
    stay, cell = fixture['stay'][library], fixture['cell']
    survivors = [int((stay & (cell == c)).sum()) if fixture['cell_units'][c] else 0 for c in range(len(fixture['names']))]
    rows = [line.split('\t') for line in (ours / 'barcodes.tsv').read_text().splitlines()]
    assert [row[0] for row in rows] == fixture['whitelist'] and [row[1] for row in rows] == fixture['names']
    assert [int(row[2]) for row in rows] == fixture['cell_assigned'].tolist()
    assert [int(row[3]) for row in rows] == [int(n >= 1) for n in fixture['cell_units']]
    assert [int(row[4]) for row in rows] == fixture['cell_units'].tolist()
    assert [int(row[5]) for row in rows] == survivors and all(len(row) == 6 for row in rows)
    summary = json.loads((ours / 'barcodes.json').read_text())
    assert [summary[k] for k in ('exact', 'corrected', 'ambiguous', 'no_match', 'unreadable')] == fixture['stats'].tolist()
    assert (summary['umi_start'], summary['umi_length']) == (3 + BARCODE_LENGTH, fixture['umi_length'])
    assert summary['umi_unreadable'] == fixture['unreadable']
    assert summary['umi_duplicates'] == int(fixture['cell_units'].sum()) - sum(survivors) > 0
    assert sorted(p.name for p in ours.iterdir() if p.is_dir()) == sorted(fixture['names'][c] for c in kept)


@pytest.fixture(scope='module')
def per_cell(pooled):
    return _per_cell_run(pooled, pooled['folder'] / 'per_cell', 'paired')


def test_pooled_run_writes_the_files_of_the_survivors(pooled, per_cell, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    out = _pooled_run(pooled, pooled['folder'] / 'collapsed')
    _assert_same_run(pooled, out, per_cell, 'paired')
    # and not those of the cell's units as they were read: collapse changes every cell's abundances
    uncollapsed = _per_cell_run(pooled, pooled['folder'] / 'per_cell_uncollapsed', 'uncollapsed')
    for c in np.flatnonzero(pooled['cell_units']):
        name = pooled['names'][c]
        assert (per_cell / name / 'abundance.tsv').read_bytes() != (uncollapsed / name / 'abundance.tsv').read_bytes(), name


def test_molecules_spread_over_many_chunks(pooled, per_cell, monkeypatch):
    monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', '1000')
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'collapsed_chunks'), per_cell, 'paired')


def test_short_umis_shared_by_chance(pooled_short, monkeypatch):
    monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', '1000')
    theirs = _per_cell_run(pooled_short, pooled_short['folder'] / 'per_cell', 'paired')
    _assert_same_run(pooled_short, _pooled_run(pooled_short, pooled_short['folder'] / 'collapsed'), theirs, 'paired')


def test_with_bias(pooled):
    theirs = _per_cell_run(pooled, pooled['folder'] / 'per_cell_bias', 'paired', extra=['--bias'])
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'collapsed_bias', extra=['--bias']), theirs, 'paired')


def test_single_ended(pooled):
    theirs = _per_cell_run(pooled, pooled['folder'] / 'per_cell_single', 'single', single=True)
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'collapsed_single', single=True), theirs, 'single')


def test_rf_stranded(pooled):
    theirs = _per_cell_run(pooled, pooled['folder'] / 'per_cell_rf', 'rf', extra=['--rf-stranded'])
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'collapsed_rf', extra=['--rf-stranded']), theirs, 'rf')


def test_with_gene_tables(pooled):
    from seekmer_amd import common
    folder = pooled['folder']
    if (np.asarray(common.KMerIndex.load(pooled['index']).transcripts['gene_id']) != b'').any():
        extra = ['--genes']
    else:                                     # the fixture's index was built without genes: a map of three transcripts a gene
        with open(folder / 'genes.tsv', 'wb') as f:
            for t, id_ in enumerate(pooled['ids']):
                f.write(bytes(id_).split(b'.')[0] + b'\tG%04d\n' % (t // 3))
        extra = ['--gene-map', str(folder / 'genes.tsv')]
    theirs = _per_cell_run(pooled, folder / 'per_cell_genes', 'paired', extra=extra)
    ours = _pooled_run(pooled, folder / 'collapsed_genes', extra=extra)
    _assert_same_run(pooled, ours, theirs, 'paired')
    for name in ('genes.tpm.tsv', 'genes.unique_counts.tsv'):
        assert (ours / name).read_bytes() == (theirs / name).read_bytes(), name
    for c in np.flatnonzero(pooled['cell_units']):
        name = pooled['names'][c]
        assert (ours / name / 'abundance.genes.tsv').read_bytes() == (theirs / name / 'abundance.genes.tsv').read_bytes()
