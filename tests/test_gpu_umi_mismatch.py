"""`--umi-mismatches 1` on the GPU ("UMI mismatches") against tests/umi_mismatch_reference.py,
exactly.

The classes the reference collapses by come from the oracle (oracle.map_batch on the oracle index of the same
sequences, strand_reference.filter_result for the stranded cases), never from the code under test.  A sample set made
with umi_mismatches=1 must give, bit for bit, what a plain set gives that is fed the reference's survivors alone; and
`infer-many --barcodes ... --umi-length 12 --umi-mismatches 1` on pooled files must write, for every cell, what
`infer-many` writes for FASTQ files that hold exactly the cell's surviving units in order."""
import json

import numpy as np
import pytest

import umi_mismatch_reference as near
import umi_reference as exact
from conftest import make_product_index
from strand_reference import filter_result

pytestmark = pytest.mark.gpu

BASES = 'ACGT'
READ_LEN = 75
HOOKS = ('SKM_SAMPLE_SET_MAX_UNITS', 'SKM_TEST_UMI_SLOTS', 'SKM_TEST_MAP_BLOCKS')


# ---- helpers of tests/test_gpu_umi.py (copies: that file is free to change) ---------------------------------------
def _random_barcodes(rng, n, length):
    """n distinct barcodes of `length` bases"""
    seen = set()
    while len(seen) < n:
        seen.update(''.join(row) for row in rng.choice(list(BASES), size=(n - len(seen), length)))
    return sorted(seen, key=lambda _: rng.random())


def _substitute(rng, text, places):
    out = list(text)
    for p in rng.choice(len(text), size=places, replace=False):
        out[p] = rng.choice([b for b in BASES if b != out[p]])
    return ''.join(out)


def _write_fastq(path, reads):
    with open(path, 'w') as f:
        for i, read in enumerate(reads):
            f.write('@r%d\n%s\n+\n%s\n' % (i, read, 'I' * len(read)))


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


# ---- the set, directly --------------------------------------------------------------------------------------------
def _noise(rng, n):
    text = lambda: bytes(b'ACGT'[int(x)] for x in rng.integers(0, 4, READ_LEN))
    return [(text(), text()) for _ in range(n)]


def _aligned_pairs(oracle, oindex, distinct, n):
    """the first n of `distinct` that the oracle aligns, the last of them of another class than the first, and the
    number of pairs looked at"""
    look = 80
    classes = oracle.map_batch(oindex, *oracle.pack_reads([read for pair in distinct[:look] for read in pair]), look, True).tuples()
    aligned = [i for i, t in enumerate(classes) if t]
    other = next(i for i in aligned[n - 1:] if classes[i] != classes[aligned[0]])
    return [distinct[i] for i in aligned[:n - 1] + [other]], look


def _filler(rng, pairs, length, near_share):
    """every pair 1 to 4 times (mean 2) under one random UMI, every copy after the first with one substituted base
    with probability near_share; shuffled"""
    out = []
    for pair in pairs:
        umi = int(rng.integers(0, 4 ** length))
        for copy in range(int(rng.choice([1, 2, 3, 4], p=[.4, .3, .2, .1]))):
            flip = int(rng.integers(1, 4)) << (2 * int(rng.integers(0, length))) if copy and rng.random() < near_share else 0
            out.append((pair, umi ^ flip))
    return [out[i] for i in rng.permutation(len(out))]


def _reference(oracle, oindex, samples, length, strands=(None,)):
    """the samples' units (pair, umi) -> everything the assertions need, the answers from the reference"""
    reads = [read for units in samples for pair, _ in units for read in pair]
    sample = np.repeat(np.arange(len(samples)), [len(units) for units in samples]).astype(np.int32)
    umi = np.asarray([m for units in samples for _, m in units], dtype=np.uint32)
    mapped = oracle.map_batch(oindex, *oracle.pack_reads(reads), sample.size, True)
    tuples = {strand: (mapped if strand is None else filter_result(mapped, strand)).tuples() for strand in strands}
    stay = {strand: near.survivors(sample, umi, t, length, 1) for strand, t in tuples.items()}
    by_definition = {strand: near.survivors_by_definition(sample, umi, t, length, 1) for strand, t in tuples.items()}
    stay_exact = {strand: exact.survivors(sample, umi, t) for strand, t in tuples.items()}
    return dict(samples=samples, sample=sample, umi=umi, tuples=tuples, stay=stay, by_definition=by_definition,
                stay_exact=stay_exact, length=length)


U = dict(a=0x9E3779B9, b=0x7F4A7C15, c=0x1B873593, d=0xCC9E2D51, e=0x85EBCA6B, f=0xC2B2AE35, g=0x27D4EB2F, h=0x165667B1,
         j=0xD3A2646C, k=0xFD7046C5, noise=0x00000010)
UMI_ONES = 2 ** 32 - 1


@pytest.fixture(scope='module')
def molecules(oracle, transcriptome):
    """Three samples of units (pair, UMI of 16 bases): filler molecules 1 to 4 times, a third of the later copies with
    one substituted base, and in samples 0 and 1 the named situations:
      A  a near copy next to its original            B  a near copy more than 1024 units after its original
      C  the chain m0, m1, m2 (one stays)            D  the chain m0, m2, m1 (two stay)
      E  a near UMI with another class (both stay)   F  a near pair across samples 0 and 1 (both stay)
      G  distance 2 (both stay)                      H  a substitution in the first base, and one in the last
      I  UMI 0 and UMI 4^16 - 1, each with a neighbour
      J  a near UMI that itself appears twice (one near removal, one exact removal)
      K  200 unaligned reads that share neighbouring UMIs (all stay)"""
    ids, pool, tx_offsets, oindex, index = transcriptome
    rng = np.random.default_rng(1999)
    samples, named = [], None
    for s in range(3):
        distinct = _pairs(pool, tx_offsets, 60 + s, s * 5000, 1480)
        chosen, look = _aligned_pairs(oracle, oindex, distinct, 12)
        filler = _filler(rng, distinct[look:], 16, 0.35)
        if s == 2:
            samples.append(filler)
            continue
        e1, a, b, c, d, f, g, h, i0, i1, j, e2 = chosen      # (e2: of another class than e1)
        if s == 1:
            f = named['f']
        units = [(a, U['a']), (a, U['a'] ^ 1), (b, U['b']), (c, U['c']), (c, U['c'] ^ (1 << 6)), (c, U['c'] ^ (1 << 6) ^ (2 << 20)),
                 (d, U['d']), (d, U['d'] ^ (3 << 8) ^ (1 << 12)), (d, U['d'] ^ (3 << 8)), (e1, U['e']), (e2, U['e'] ^ 2)]
        units += filler[:40] + [(f, U['f'] ^ (s << 14)), (g, U['g']), (g, U['g'] ^ 1 ^ (1 << 2)), (h, U['h']), (h, U['h'] ^ (2 << 30)),
                                (h, U['h'] ^ 3), (i0, 0), (i1, UMI_ONES), (j, U['j'])]
        units += filler[40:1200] + [(b, U['b'] ^ (2 << 10)), (i0, 1 << 30), (i1, UMI_ONES ^ (3 << 4)), (j, U['j'] ^ 4), (j, U['j'] ^ 4)]
        units += filler[1200:]
        late = [(pair, U['noise'] ^ (int(rng.integers(0, 4)) << 2)) for pair in _noise(rng, 200)]
        for item, at in zip(late, np.sort(rng.integers(12, len(units), size=len(late)))[::-1]):
            units.insert(int(at), item)
        if s == 0:
            named = dict(a=a, b=b, c=c, d=d, e1=e1, e2=e2, f=f, g=g, h=h, i0=i0, i1=i1, j=j)
        samples.append(units)
    out = _reference(oracle, oindex, samples, 16, strands=(None, 'rf'))
    out.update(index=index, named=named)
    return out


def _short(oracle, transcriptome, length, seed):
    """One sample of UMIs of 5 bases (filler, the first and the last base, UMI 0 and UMI 4^5 - 1) or of 4 bases (all
    256 UMIs on six pairs, so that most molecules have a neighbour)"""
    ids, pool, tx_offsets, oindex, index = transcriptome
    rng = np.random.default_rng(seed)
    distinct = _pairs(pool, tx_offsets, 70 + length, 20000, 400)
    chosen, look = _aligned_pairs(oracle, oindex, distinct, 6)
    if length == 4:
        units = [(chosen[int(rng.integers(6))], int(rng.integers(0, 256))) for _ in range(700)]
        units += [(pair, int(rng.integers(0, 256))) for pair in _noise(rng, 40)]
        units = [units[i] for i in rng.permutation(len(units))]
    else:
        h, i0, i1 = chosen[:3]
        ones = 4 ** length - 1
        units = [(h, 0b0110110001), (h, 0b0110110001 ^ (1 << 8)), (h, 0b0110110001 ^ 2), (i0, 0), (i1, ones)]
        units += _filler(rng, distinct[look:], length, 0.35) + [(i0, 3 << 8), (i1, ones ^ 1), (h, 0b0110110001 ^ (1 << 8) ^ 2)]
    out = _reference(oracle, oindex, [units], length)
    out.update(index=index, named=chosen)
    return out


@pytest.fixture(scope='module')
def short5(oracle, transcriptome):
    return _short(oracle, transcriptome, 5, 55)


@pytest.fixture(scope='module')
def short4(oracle, transcriptome):
    return _short(oracle, transcriptome, 4, 44)


def _near_only(fixture, strand=None):
    """per sample: the units that are the first of their exact molecule and go all the same"""
    gone = fixture['stay_exact'][strand] & ~fixture['stay'][strand]
    return [int((gone & (fixture['sample'] == s)).sum()) for s in range(len(fixture['samples']))]


def test_the_molecules_are_not_trivial(molecules, short5, short4):
    """the reference alone: what the set is asked is in the input"""
    samples, sample, tuples, stay, stay_exact = (molecules[k] for k in ('samples', 'sample', 'tuples', 'stay', 'stay_exact'))
    # the rule as it is stated (every pair of units of a cell and class) gives what the two passes give, on every fixture
    for fixture in (molecules, short5, short4):
        assert set(fixture['by_definition']) == set(fixture['stay'])
        for strand, want in fixture['by_definition'].items():
            assert want.dtype == bool and want.shape == fixture['stay'][strand].shape
            np.testing.assert_array_equal(fixture['stay'][strand], want, err_msg='length %d, strand %s' % (fixture['length'], strand))
    assert set(molecules['by_definition']) == {None, 'rf'}
    n = molecules['named']
    first = samples[0]
    all_of = lambda pair: [u for u, item in enumerate(first) if item[0] == pair]
    klass = lambda pair: tuples[None][all_of(pair)[0]]
    for pair in n.values():
        assert klass(pair) and all(tuples[None][u] == klass(pair) for u in all_of(pair)), 'aligned; verbatim repeats share a class'
    answer = lambda pair: stay[None][all_of(pair)].tolist()
    assert all_of(n['a']) == [0, 1] and answer(n['a']) == [True, False]
    assert np.diff(all_of(n['b'])).max() > 1024 and all_of(n['b'])[0] < 500 and answer(n['b']) == [True, False]
    assert answer(n['c']) == [True, False, False] and answer(n['d']) == [True, True, False]
    assert klass(n['e1']) != klass(n['e2']) and answer(n['e1']) == [True] and answer(n['e2']) == [True]
    second = int(np.flatnonzero(sample == 1)[0])
    in_second = [second + u for u, item in enumerate(samples[1]) if item[0] == n['f']]
    assert len(all_of(n['f'])) == len(in_second) == 1 and answer(n['f']) == [True] and stay[None][in_second[0]]
    assert bin(first[all_of(n['f'])[0]][1] ^ samples[1][in_second[0] - second][1]).count('1') == 1
    assert answer(n['g']) == [True, True]
    assert answer(n['h']) == [True, False, False] and answer(n['i0']) == [True, False] and answer(n['i1']) == [True, False]
    assert answer(n['j']) == [True, False, False] and stay_exact[None][all_of(n['j'])].tolist() == [True, True, False]
    noise = [u for u, item in enumerate(first) if (item[1] | 12) == (U['noise'] | 12) and item[0] not in n.values()]
    assert len(noise) >= 200 and sum(not tuples[None][u] for u in noise) >= 200
    assert all(stay[None][u] for u in noise if not tuples[None][u])
    for strand in (None, 'rf'):
        aligned = np.asarray([bool(t) for t in tuples[strand]])
        assert not (~aligned & ~stay[strand]).any(), 'an unaligned unit is never removed'
        assert not (stay[strand] & ~stay_exact[strand]).any(), 'one mismatch only removes more'
        assert all(count >= 100 for count in _near_only(molecules, strand)), _near_only(molecules, strand)
        for s in range(3):
            mine = sample == s
            assert (stay[strand] != stay_exact[strand])[mine].any() and (mine & ~stay_exact[strand]).sum() >= 100
            assert 2400 <= mine.sum() <= 3600
    assert any(a != b for a, b in zip(tuples[None], tuples['rf']))
    # UMIs of 5 bases: the first base, the last base, UMI 0 and UMI 4^5 - 1; filler with neighbours
    units, answer5 = short5['samples'][0], short5['stay'][None]
    h, i0, i1 = short5['named'][:3]
    for pair, want in ((h, [True, False, False, False]), (i0, [True, False]), (i1, [True, False])):
        assert answer5[[u for u, item in enumerate(units) if item[0] == pair]].tolist() == want
    assert _near_only(short5)[0] >= 40 and all(m < 4 ** 5 for _, m in units)
    # UMIs of 4 bases: most molecules have a neighbour, so most first units go
    first_units = short4['stay_exact'][None] & np.asarray([bool(t) for t in short4['tuples'][None]])
    assert _near_only(short4)[0] > 0.5 * first_units.sum() > 100
    assert len({m for _, m in short4['samples'][0]}) > 240 and (short4['stay'][None] & first_units).sum() >= 20


def _expected(fixture, strand=None):
    """a plain set fed the reference's survivors alone"""
    from seekmer_amd import mapper
    plain = mapper.SampleSet(fixture['index'], True, strand=strand, per_sample_lengths=True, bias=True)
    at = 0
    for s, units in enumerate(fixture['samples']):
        stay = fixture['stay'][strand][at:at + len(units)]
        _add_sample(plain, s, [unit for unit, keep in zip(units, stay) if keep])
        at += len(units)
    assert plain.umi_removed().tolist() == [0] * len(fixture['samples']) and plain.umi_near_removed() == 0
    return _state(plain)


@pytest.fixture(scope='module')
def expected(molecules):
    """per strand: computed once"""
    return {strand: _expected(molecules, strand) for strand in (None, 'rf')}


def _collapsed_state(fixture, strand=None, cuts=(), order=None, **how):
    from seekmer_amd import mapper
    sample_set = mapper.SampleSet(fixture['index'], True, strand=strand, per_sample_lengths=True, bias=True,
                                  umi_bases=fixture['length'], **how)
    for s in order or range(len(fixture['samples'])):
        units = fixture['samples'][s]
        _add_sample(sample_set, s, units, umis=[m for _, m in units], cuts=cuts if s == 0 else ())
    state = _state(sample_set)
    state['removed'], state['near removed'] = sample_set.umi_removed(), sample_set.umi_near_removed()
    return state


def _assert_collapsed(fixture, expected, strand=None, cuts=(), order=None):
    got = _collapsed_state(fixture, strand, cuts, order, umi_mismatches=1)
    sample, stay = fixture['sample'], fixture['stay'][strand]
    n_samples = len(fixture['samples'])
    want_removed = [int(((sample == s) & ~stay).sum()) for s in range(n_samples)]
    want_near = sum(_near_only(fixture, strand))
    print('removed', got['removed'].tolist(), 'reference', want_removed, 'by a neighbour alone', got['near removed'], 'reference',
          want_near, 'units', np.bincount(sample).tolist())
    np.testing.assert_array_equal(got.pop('removed'), want_removed)
    assert got.pop('near removed') == want_near
    assert sorted(got) == sorted(expected)
    for s in range(n_samples):                # first-seen units count the units as added: here, as the survivors' numbers
        rank = np.cumsum(stay[sample == s]) - 1
        assert stay[sample == s][got['first seen %d' % s]].all(), 'a removed unit is no class\'s first'
        got['first seen %d' % s] = rank[got['first seen %d' % s]]
    for name, want in expected.items():
        np.testing.assert_array_equal(got[name], want, err_msg=name)


def _hook(monkeypatch, hook):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    if hook:
        monkeypatch.setenv(*hook.split('='))


@pytest.mark.parametrize('hook', [None, 'SKM_SAMPLE_SET_MAX_UNITS=500', 'SKM_TEST_UMI_SLOTS=2', 'SKM_TEST_MAP_BLOCKS=1'])
def test_a_set_with_one_mismatch_is_the_plain_set_of_the_survivors(molecules, expected, monkeypatch, hook):
    """launches of 500 units: near pairs straddle launches; 2 slots: the molecule set grows under every launch"""
    _hook(monkeypatch, hook)
    _assert_collapsed(molecules, expected[None])


def test_a_segment_cut_between_a_near_pair(molecules, expected, monkeypatch):
    _hook(monkeypatch, None)
    _assert_collapsed(molecules, expected[None], cuts=(1, 1700))      # between A and its near copy


def test_the_samples_in_another_order(molecules, expected, monkeypatch):
    _hook(monkeypatch, 'SKM_SAMPLE_SET_MAX_UNITS=500')
    _assert_collapsed(molecules, expected[None], order=(1, 0, 2))


def test_neighbours_follow_the_strand_filter(molecules, expected, monkeypatch):
    _hook(monkeypatch, 'SKM_SAMPLE_SET_MAX_UNITS=500')
    _assert_collapsed(molecules, expected['rf'], strand='rf')


@pytest.mark.parametrize('which, hook', [('short5', None), ('short4', 'SKM_SAMPLE_SET_MAX_UNITS=100'), ('short4', 'SKM_TEST_UMI_SLOTS=2')])
def test_short_umis(request, monkeypatch, which, hook):
    """5 bases: the neighbours stay inside the UMI's 10 bits; 4 bases: nearly every molecule has a neighbour"""
    _hook(monkeypatch, hook)
    fixture = request.getfixturevalue(which)
    _assert_collapsed(fixture, _expected(fixture))


def test_no_mismatch_is_the_set_it_was(short5, monkeypatch):
    _hook(monkeypatch, None)
    without, with_zero = _collapsed_state(short5), _collapsed_state(short5, umi_mismatches=0)
    assert sorted(without) == sorted(with_zero) and with_zero['near removed'] == without['near removed'] == 0
    for name, want in without.items():
        np.testing.assert_array_equal(with_zero[name], want, err_msg=name)
    stay = short5['stay_exact'][None]
    assert with_zero['removed'].tolist() == [int((~stay).sum())] and (stay != short5['stay'][None]).any()


def test_refusals(short5, native_libs):
    from seekmer_amd import mapper
    index, units = short5['index'], short5['samples'][0][:10]
    hip = native_libs.hip()
    with_umis = mapper.SampleSet(index, True, per_sample_lengths=True, umi_bases=5)
    for bad in (2, -1):
        assert hip.skm_sample_set_set_umi_mismatches(with_umis._handle, bad) == native_libs.SKM_ERR_ARG
    assert hip.skm_sample_set_set_umi_mismatches(with_umis._handle, 1) == native_libs.SKM_OK
    assert hip.skm_sample_set_set_umi_mismatches(with_umis._handle, 0) == native_libs.SKM_OK
    _add_sample(with_umis, 0, units, umis=[m for _, m in units])
    assert hip.skm_sample_set_set_umi_mismatches(with_umis._handle, 1) == native_libs.SKM_ERR_STATE       # after a segment
    plain = mapper.SampleSet(index, True, per_sample_lengths=True)
    assert hip.skm_sample_set_set_umi_mismatches(plain._handle, 1) == native_libs.SKM_ERR_STATE           # keeps no UMIs
    assert plain.umi_near_removed() == 0 and with_umis.umi_near_removed() == 0
    for how in (dict(umi_mismatches=1), dict(umi_bases=5, umi_mismatches=2)):
        with pytest.raises(ValueError):
            mapper.SampleSet(index, True, per_sample_lengths=True, **how)


# ---- end to end ---------------------------------------------------------------------------------------------------
CELL_PAIRS = (500, 350, 450, 300, 400, 250, 380, 420, 330, 280, 360, 310)          # original pairs of the twelve cells
BARCODE_LENGTH, START, UMI_LENGTH = 12, 3, 12


@pytest.fixture(scope='module')
def pooled(oracle, transcriptome, tmp_path_factory):
    """Twelve cells (barcodes at distance >= 3 from each other): every original pair is written k times with one UMI of
    12 bases, k from {1, 2, 3, 4} with probabilities (.4, .3, .2, .1), and a fifth of all copies carries one
    substituted UMI base; barcode reads = GGA + barcode (start 3) + UMI (start 15) + a tail; 10 % of the barcodes
    carry a substitution, 2 % of the UMIs an N or a lower-case letter; everything shuffled.  The reference's answer
    for the paired and the single-ended library, and one FASTQ pair per cell and library with the survivors."""
    from seekmer_amd import index_builder, synth
    import barcode_reference
    ids, pool, tx_offsets, oindex, _ = transcriptome
    folder = tmp_path_factory.mktemp('pooled_umi_mismatch')
    index_path = folder / 'index.npz'
    index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    rng = np.random.default_rng(4242)
    while True:                    # a substitution never reaches another cell
        whitelist = _random_barcodes(rng, len(CELL_PAIRS), BARCODE_LENGTH)
        if all(sum(a != b for a, b in zip(x, y)) >= 3 for i, x in enumerate(whitelist) for y in whitelist[:i]):
            break
    names = ['cell%d' % c for c in range(len(CELL_PAIRS))]
    (folder / 'whitelist.tsv').write_text(''.join('%s\t%s\n' % row for row in zip(whitelist, names)))
    mates, truth, umis = ([], []), [], []
    for c, n_pairs in enumerate(CELL_PAIRS):
        raw = synth.reads(200 + c % 2, pool, tx_offsets, c * 8000, n_pairs, READ_LEN, True)[0][:-1].tobytes().decode()
        for u in range(n_pairs):
            molecule = ''.join(rng.choice(list(BASES), size=UMI_LENGTH))
            for _ in range(int(rng.choice([1, 2, 3, 4], p=[.4, .3, .2, .1]))):
                for mate in (0, 1):
                    mates[mate].append(raw[(2 * u + mate) * READ_LEN:(2 * u + mate + 1) * READ_LEN])
                truth.append(c)
                umis.append(_substitute(rng, molecule, 1) if rng.random() < 0.2 else molecule)
    shuffle = rng.permutation(len(truth))
    mates = [[mate[u] for u in shuffle] for mate in mates]
    barcodes = []
    for u in shuffle:
        barcode, molecule = whitelist[truth[u]], umis[u]
        if rng.random() < 0.1:
            barcode = _substitute(rng, barcode, 1)
        if rng.random() < 0.02:
            p = rng.integers(UMI_LENGTH)
            molecule = molecule[:p] + ('N' if rng.random() < 0.5 else molecule[p].lower()) + molecule[p + 1:]
        barcodes.append('GGA' + barcode + molecule + ''.join(rng.choice(list(BASES), size=8)))
    _write_fastq(folder / 'pool_1.fastq', mates[0])
    _write_fastq(folder / 'pool_2.fastq', mates[1])
    _write_fastq(folder / 'barcodes.fastq', barcodes)
    cell, cell_assigned, stats = barcode_reference.assign(whitelist, barcodes, start=START, mismatches=1)
    umi, readable = exact.windows(barcodes, START + BARCODE_LENGTH, UMI_LENGTH)
    cell = np.where(readable, cell, -1)
    cell_units = np.bincount(cell[cell >= 0], minlength=len(whitelist))
    n = len(barcodes)
    paired = oracle.map_batch(oindex, *oracle.pack_reads([m.encode() for pair in zip(*mates) for m in pair]), n, True)
    single = oracle.map_batch(oindex, *oracle.pack_reads([m.encode() for m in mates[0]]), n, False)
    tuples = {'paired': paired.tuples(), 'single': single.tuples()}
    stay = {library: near.survivors(cell, umi, t, UMI_LENGTH, 1) for library, t in tuples.items()}
    by_definition = {library: near.survivors_by_definition(cell, umi, t, UMI_LENGTH, 1) for library, t in tuples.items()}
    stay_exact = {library: exact.survivors(cell, umi, t) for library, t in tuples.items()}
    for library, mask in stay.items():
        for c in range(len(whitelist)):
            for mate in (0, 1):
                _write_fastq(folder / ('%s_%s_%d.fastq' % (library, names[c], mate + 1)),
                             [mates[mate][u] for u in np.flatnonzero(mask & (cell == c))])
    return dict(folder=folder, index=index_path, whitelist=whitelist, names=names, cell=cell, umi=umi, cell_assigned=cell_assigned,
                cell_units=cell_units, stats=stats, unreadable=int((~readable).sum()), tuples=tuples, stay=stay,
                by_definition=by_definition, stay_exact=stay_exact, barcodes=barcodes)


def test_the_pooled_run_is_not_trivial(pooled):
    """the reference alone"""
    import discover_reference
    cell = pooled['cell']
    assert pooled['unreadable'] > 0 and (pooled['cell_units'] > 300).all() and 6000 < len(cell) < 12000
    for library in ('paired', 'single'):
        stay, stay_exact = pooled['stay'][library], pooled['stay_exact'][library]
        np.testing.assert_array_equal(stay, pooled['by_definition'][library], err_msg=library)      # the rule as it is stated
        assert not (stay & ~stay_exact).any()
        for c in range(len(CELL_PAIRS)):
            mine = cell == c
            assert (mine & stay_exact & ~stay).sum() >= 20 and (mine & ~stay_exact).sum() >= 50, (library, c)
    picked, candidates, info = discover_reference.discover(pooled['barcodes'], BARCODE_LENGTH, 12, start=START)
    assert sorted(barcode for barcode, _ in picked) == sorted(pooled['whitelist'])


def _run(fixture, out, files, extra, names=None):
    from seekmer_amd.__main__ import main
    assert main(['infer-many', str(fixture['index']), str(out), *map(str, files), '-b', '2', '--seed', '7', *extra,
                 *(['--names', ','.join(names)] if names else [])]) == 0
    return out


def _per_cell_run(fixture, out, library, single=False):
    """infer-many on the reference's per-cell files of `library`"""
    folder = fixture['folder']
    files = [folder / ('%s_%s_%d.fastq' % (library, name, mate)) for name in fixture['names'] for mate in ((1,) if single else (1, 2))]
    return _run(fixture, out, files, ['-s'] if single else [], names=fixture['names'])


UMIS = ['--umi-start', str(START + BARCODE_LENGTH), '--umi-length', str(UMI_LENGTH)]


def _pooled_run(fixture, out, single=False, extra=('--umi-mismatches', '1'), cells=None):
    folder = fixture['folder']
    files = [folder / 'pool_1.fastq'] + ([] if single else [folder / 'pool_2.fastq'])
    cells = cells or ['--barcodes', str(folder / 'whitelist.tsv')]
    return _run(fixture, out, files, [*cells, '--barcode-file', str(folder / 'barcodes.fastq'), '--barcode-start', str(START), *UMIS,
                                      *(['-s'] if single else []), *extra])


def _assert_same_outputs(ours, theirs):
    """one sample's folder of two runs (a copy of the helper of tests/test_gpu_infer_many.py)"""
    one, other = (ours / 'abundance.tsv').read_bytes(), (theirs / 'abundance.tsv').read_bytes()
    assert len(one) > 1000 and one == other, ours.name
    info = [json.loads((folder / 'run_info.json').read_text()) for folder in (ours, theirs)]
    for run_info in info:
        del run_info['start_time'], run_info['call']
    assert info[0] == info[1]
    with np.load(ours / 'abundance.npz') as a, np.load(theirs / 'abundance.npz') as b:
        assert sorted(a.files) == sorted(b.files) and 'bootstrap/bs1' in a.files
        for name in a.files:
            if name not in ('aux/call', 'aux/start_time'):
                np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def _assert_same_run(fixture, ours, theirs, library, discovered=False):
    rows = [line.split('\t') for line in (ours / 'barcodes.tsv').read_text().splitlines()]
    if discovered:                            # the cells in ranked order, named by their barcodes
        order = [fixture['whitelist'].index(row[0]) for row in rows]
        assert sorted(order) == list(range(len(fixture['names']))) and [row[1] for row in rows] == [row[0] for row in rows]
    else:
        order = list(range(len(fixture['names'])))
        assert [row[0] for row in rows] == fixture['whitelist'] and [row[1] for row in rows] == fixture['names']
        assert (ours / 'samples.tsv').read_bytes() == (theirs / 'samples.tsv').read_bytes()
    for row, c in zip(rows, order):
        _assert_same_outputs(ours / row[1], theirs / fixture['names'][c])
    stay, stay_exact, cell = fixture['stay'][library], fixture['stay_exact'][library], fixture['cell']
    survivors = [int((stay & (cell == c)).sum()) for c in order]
    assert [int(row[2]) for row in rows] == fixture['cell_assigned'][order].tolist()
    assert [int(row[3]) for row in rows] == [1] * len(order)
    assert [int(row[4]) for row in rows] == fixture['cell_units'][order].tolist()
    assert [int(row[5]) for row in rows] == survivors and all(len(row) == 6 for row in rows)
    summary = json.loads((ours / 'barcodes.json').read_text())
    assert [summary[k] for k in ('exact', 'corrected', 'ambiguous', 'no_match', 'unreadable')] == fixture['stats'].tolist()
    assert (summary['umi_start'], summary['umi_length']) == (START + BARCODE_LENGTH, UMI_LENGTH)
    assert summary['umi_unreadable'] == fixture['unreadable'] and summary['umi_mismatches'] == 1
    assert summary['umi_duplicates'] == int(fixture['cell_units'].sum()) - sum(survivors) > 0
    assert summary['umi_near_duplicates'] == int((stay_exact & ~stay).sum()) > 0
    assert sorted(p.name for p in ours.iterdir() if p.is_dir()) == sorted(row[1] for row in rows)


@pytest.fixture(scope='module')
def per_cell(pooled):
    return _per_cell_run(pooled, pooled['folder'] / 'per_cell', 'paired')


def test_pooled_run_writes_the_files_of_the_survivors(pooled, per_cell, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'near'), per_cell, 'paired')


def test_near_pairs_spread_over_many_chunks(pooled, per_cell, monkeypatch):
    monkeypatch.setenv('SKM_DEMUX_CHUNK_UNITS', '1000')
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'near_chunks'), per_cell, 'paired')


def test_single_ended(pooled, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    theirs = _per_cell_run(pooled, pooled['folder'] / 'per_cell_single', 'single', single=True)
    _assert_same_run(pooled, _pooled_run(pooled, pooled['folder'] / 'near_single', single=True), theirs, 'single')


def test_with_discovered_cells(pooled, per_cell, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    out = _pooled_run(pooled, pooled['folder'] / 'near_discovered',
                      cells=['--discover-cells', '12', '--barcode-length', str(BARCODE_LENGTH)])
    _assert_same_run(pooled, out, per_cell, 'paired', discovered=True)


def test_no_mismatch_writes_what_no_option_writes(pooled, monkeypatch):
    monkeypatch.delenv('SKM_DEMUX_CHUNK_UNITS', raising=False)
    folder = pooled['folder']
    plain = _pooled_run(pooled, folder / 'exact', extra=())
    zero = _pooled_run(pooled, folder / 'exact_zero', extra=('--umi-mismatches', '0'))
    files = lambda root: sorted(str(p.relative_to(root)) for p in root.rglob('*') if p.is_file())
    assert files(plain) == files(zero) and len(files(plain)) > 3 * len(CELL_PAIRS)
    for name in files(plain):
        if name.endswith('run_info.json') or name.endswith('abundance.npz'):          # (they hold the call and its time)
            continue
        assert (plain / name).read_bytes() == (zero / name).read_bytes(), name
    for c in range(len(CELL_PAIRS)):
        one, other = plain / pooled['names'][c], zero / pooled['names'][c]
        info = [json.loads((cell / 'run_info.json').read_text()) for cell in (one, other)]
        for run_info in info:
            del run_info['start_time'], run_info['call']
        assert info[0] == info[1]
        with np.load(one / 'abundance.npz') as a, np.load(other / 'abundance.npz') as b:
            assert sorted(a.files) == sorted(b.files)
            for name in a.files:
                if name not in ('aux/call', 'aux/start_time'):
                    np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    summary = json.loads((zero / 'barcodes.json').read_text())
    assert 'umi_mismatches' not in summary and 'umi_near_duplicates' not in summary
    assert summary['umi_duplicates'] == int(pooled['cell_units'].sum()) - int((pooled['stay_exact']['paired'] & (pooled['cell'] >= 0)).sum())
