"""The target-list fixture (tests/target_list_reference.py) reaches what it was built to reach.  The oracle alone:
no GPU, no product code.  tests/test_gpu_target_lists.py holds the map kernel to the oracle on this input, and that
is worth what these conditions are worth: every list size of SIZES met, every pattern kept exactly, in both
orientations, single-ended and paired."""
import numpy as np
import pytest

import target_list_reference as lists
from test_gpu_parity import _adversarial_reads


@pytest.fixture(scope='module')
def mapped(oracle):
    """(fixture, oracle index, the oracle's result for the single-ended units, for the pairs)."""
    fixture = lists.fixture()
    index = oracle.build_index(fixture.sequences, fixture.ids)
    results = []
    for paired, units in ((False, fixture.singles), (True, fixture.pairs)):
        bases, offsets = oracle.pack_reads(lists.reads_of(units))
        results.append(oracle.map_batch(index, bases, offsets, len(units), paired))
    return fixture, index, results[0], results[1]


def test_the_fixture_is_the_stated_one(mapped):
    fixture = mapped[0]
    sized = [f for f in fixture.families if f.kind == 'sized']
    assert tuple(f.size for f in sized) == lists.SIZES and sum(lists.SIZES) == 1312
    assert 3.2e6 < fixture.sized_bases < 3.4e6
    n_patterns = sum(len(f.patterns) for f in sized)
    assert n_patterns == 147
    # five windows, both strands; three fragments, both mate orders
    assert sum(u.family.kind == 'sized' and u.targets is not None for u in fixture.singles) == 10 * n_patterns == 1470
    assert sum(u.family.kind == 'sized' and u.targets != () for u in fixture.pairs) == 6 * n_patterns == 882
    # the units that refill the contexts of one or two blocks (tests/test_gpu_target_lists.py, SKM_TEST_MAP_BLOCKS)
    assert len(fixture.singles) > 2 * 480 and len(fixture.pairs) > 2 * 240


def test_list_positions_and_sizes_on_the_built_index(mapped):
    fixture, index = mapped[0], mapped[1]
    met = lists.check_list_positions(fixture, index.contigs, index.targets)
    for size in lists.SIZES:
        assert size in met, size
    for size in lists.TWICE_SIZES:                 # every member listed twice by its core's contig
        assert 2 * size in met, size
    assert lists.MIXED_SIZE in met
    assert max(met) == 300                         # four extension words, and no more


def test_every_pattern_is_kept_exactly(mapped):
    """Every (family, pattern), both strands, every window, single-ended and paired in both mate orders: the unit
    keeps the pattern's transcripts and nothing else; core-only reads keep the family."""
    fixture, _, singles, pairs = mapped
    for units, result in ((fixture.singles, singles), (fixture.pairs, pairs)):
        kept = result.tuples()
        seen = set()
        for unit, got in zip(units, kept):
            if unit.targets is None:
                continue
            where = (unit.family.kind, unit.family.size, unit.pattern, unit.note)
            assert tuple(sorted(got)) == lists.wanted_entries(unit), where
            seen.add((unit.family.first_id, unit.pattern, unit.note, len(got) == unit.family.size))
        paired = units is fixture.pairs
        notes = ('long list first', 'long list second') if paired else ('forward', 'reverse')
        for family in fixture.families:
            if family.kind == 'other':
                continue
            for name, chosen in family.patterns.items():
                for note in notes:
                    assert (family.first_id, name, note, len(chosen) == family.size) in seen, (family.size, name, note)
    # every size of SIZES is a final list of some single-ended unit, and every family is kept whole by one
    final = set(int(c) for c in singles.count)
    for size in lists.SIZES:
        assert size in final, size
    for family in fixture.families:
        if family.kind == 'other':
            continue
        copies = 2 if family.kind == 'twice' else 1
        assert any(u.family is family and c == copies * family.size for u, c in zip(fixture.singles, singles.count))
    # ... and long lists meet in the intersection of mates: five words against four
    assert int(pairs.count.max()) == 292


def test_the_mixed_family_lists_both_signs(mapped):
    fixture, _, singles, _ = mapped
    whole = [t for u, t in zip(fixture.singles, singles.tuples_signed()) if u.family is fixture.mixed and len(t) == 129]
    assert whole
    for entries in whole:
        negative = sum(e < 0 for e in entries)
        assert sorted((negative, 129 - negative)) == [64, 65]
    part = [c for u, c in zip(fixture.singles, singles.count)
            if u.family is fixture.mixed and u.listed == 43]
    assert len(part) == 6 and all(c == 43 for c in part)


def test_units_that_belong_nowhere(mapped):
    """Chimeras of two families keep nothing or a single transcript, mates of two families nothing; a read with Ns
    inside a core still keeps the family."""
    fixture, _, singles, pairs = mapped
    chimeras = [int(c) for u, c in zip(fixture.singles, singles.count) if u.note == 'chimera']
    assert len(chimeras) == 9 and set(chimeras) <= {0, 1} and 0 in chimeras
    assert [int(c) for u, c in zip(fixture.singles, singles.count) if u.note == 'Ns'] == [300, 300]
    strangers = [int(c) for u, c in zip(fixture.pairs, pairs.count) if u.note == 'mates of two families']
    assert len(strangers) == 8 and not any(strangers)


def test_the_relaunch_batches_keep_whole_lists(oracle, mapped):
    fixture, index = mapped[0], mapped[1]
    for size in (128, 300):
        units = fixture.whole_list_units(size, 2000, seed=size)
        bases, offsets = oracle.pack_reads(lists.reads_of(units))
        result = oracle.map_batch(index, bases, offsets, len(units), False)
        assert (result.count == size).all()


@pytest.mark.parametrize('paired', [True, False])
def test_chr21_hardly_leaves_the_short_forms(oracle, chr21, chr21_oracle_index, paired):
    """What tests/test_gpu_parity.py::test_chr21_adversarial puts through the kernel: no final list above 24
    entries, none in a mask extension word.  If this ever changes, say so here."""
    rng = np.random.default_rng(7)
    reads = _adversarial_reads(chr21[1], rng, 6000, 100)
    bases, offsets = oracle.pack_reads(reads)
    n_units = len(reads) // 2 if paired else len(reads)
    result = oracle.map_batch(chr21_oracle_index, bases, offsets, n_units, paired)
    assert int(result.count.max()) <= 24
    assert int(result.count.max()) == (9 if paired else 24)
    counts = chr21_oracle_index.contigs['target_count']
    assert counts.size == 8356 and (counts > 16).sum() == 105 and (counts > 64).sum() == 2
