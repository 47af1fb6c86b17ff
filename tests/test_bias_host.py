"""The sequence-bias model (--bias) on the host: the numpy yardstick of tests/bias_reference.py against a plain
Python loop, the rule that rebuilds the transcripts from the index arrays, and the command line.  No GPU."""
import numpy as np
import pytest

import bias_reference as ref


def _host_index(seqs):
    """(contigs, sequences, targets) of the product's host builder"""
    from seekmer_amd import index_builder
    _, contigs, sequences, targets = index_builder.ContigAssembler().assemble(list(seqs))
    return contigs, sequences, targets


def _check_rebuilt(seqs, bases, known):
    """Every known base is the transcript's own; a base is unknown only where the builder has no k-mer: in a
    transcript shorter than k, or within k - 1 bases of something that is not A, C, G or T."""
    assert len(bases) == len(seqs)
    for seq, got, mask in zip(seqs, bases, known):
        seq = seq.upper()
        assert len(got) == len(seq) == mask.size
        want = np.frombuffer(seq, dtype='S1')
        np.testing.assert_array_equal(np.frombuffer(bytes(got), dtype='S1')[mask], want[mask])
        assert bytes(np.frombuffer(bytes(got), dtype='S1')[~mask]) == b'N' * int((~mask).sum())
        clean = np.isin(want, [b'A', b'C', b'G', b'T'])
        covered = np.zeros(len(seq), dtype=bool)              # bases inside a k-mer of clean bases
        run = 0
        for p in range(len(seq)):
            run = run + 1 if clean[p] else 0
            if run >= ref.K:
                covered[p - ref.K + 1:p + 1] = True
        np.testing.assert_array_equal(mask, covered)


def test_reconstruction_rebuilds_chr21(native_libs, chr21):
    ids, seqs = chr21
    assert len(seqs) == 1704
    contigs, sequences, targets = _host_index(seqs)
    bases, known = ref.rebuild_transcripts(contigs, sequences, targets, [len(s) for s in seqs])
    _check_rebuilt(seqs, bases, known)
    whole = [t for t, s in enumerate(seqs) if len(s) >= ref.K and set(s.upper()) <= set(b'ACGT')]
    assert len(whole) > 1600
    for t in whole:
        assert bytes(bases[t]) == seqs[t].upper() and known[t].all()


def test_reconstruction_rebuilds_the_synthetic_transcriptome(native_libs, oracle):
    ids, seqs = ref.synthetic_transcriptome()
    assert len(seqs[4]) == 25 and len(seqs[5]) == 10
    for contigs, sequences, targets in (_host_index(seqs),
                                        (lambda ix: (ix.contigs, ix.sequences, ix.targets))(oracle.build_index(seqs, ids))):
        bases, known = ref.rebuild_transcripts(contigs, sequences, targets, [len(s) for s in seqs])
        _check_rebuilt(seqs, bases, known)
        assert not known[5].any() and known[4].all()
        # the cases the transcriptome was made for are in the index: a contig with rows of both signs (the
        # segment shared in both orientations) and a contig with two rows of one transcript (crossed twice)
        both = twice = False
        for contig in contigs:
            rows = targets[int(contig['target_offset']):int(contig['target_offset']) + int(contig['target_count'])]
            entries = [int(e) for e in rows['entry']]
            both |= any(e >= 0 for e in entries) and any(e < 0 for e in entries)
            plain = [e if e >= 0 else ~e for e in entries]
            twice |= len(set(plain)) < len(plain)
        assert both and twice
    with pytest.raises(ValueError):                           # lengths that are not the index's
        ref.rebuild_transcripts(contigs, sequences, targets, [len(s) - 30 for s in seqs])


@pytest.mark.parametrize('strand', [None, 'fr', 'rf'])
def test_reference_equals_the_plain_loop(strand):
    rng = np.random.default_rng(5)
    ids, seqs = ref.synthetic_transcriptome(seed=3)
    seqs = [bytearray(s) for s in seqs] + [bytearray(b'ACGTAC'), bytearray(b'ACGTA'), bytearray()]
    knowns = [np.ones(len(s), dtype=bool) for s in seqs]
    knowns[0][17:21] = False                                  # unknown bases inside a transcript
    knowns[1][:3] = False
    knowns[5][:] = False                                      # a transcript without windows
    seqs[2][40] = ord('N')                                    # (a base the pool could never hold: not a window)
    n_tx = len(seqs)
    tx_windows = [ref.windows(s, k) for s, k in zip(seqs, knowns)]
    assert tx_windows[5].size == 0 and tx_windows[7].size == 1 and tx_windows[8].size == 0 and tx_windows[9].size == 0
    assert tx_windows[0].size == len(seqs[0]) - 5 - 9
    eff = rng.uniform(1.0, 500.0, n_tx)
    cases = []
    tpm = rng.uniform(0.0, 100.0, n_tx)
    tpm[3] = 0.0
    cases.append((rng.integers(0, 50, ref.BINS), tpm))
    cases.append((np.zeros(ref.BINS, dtype=np.int64), tpm))   # nothing observed: every weight 1
    single = np.zeros(n_tx)
    single[6] = 1e6
    cases.append((rng.integers(0, 50, ref.BINS), single))     # one transcript expressed: most E[h] = 0
    cases.append((rng.integers(0, 50, ref.BINS), np.zeros(n_tx)))    # nothing expected
    for observed, tpm in cases:
        expected, b, corrected = ref.correct(tx_windows, observed, tpm, eff, strand)
        want_e, want_b, want_eff = ref.brute_force(seqs, knowns, observed, tpm, eff, strand)
        np.testing.assert_allclose(expected, want_e, rtol=1e-14, atol=0)     # (one rounding per transcript against none)
        np.testing.assert_array_equal(expected == 0, want_e == 0)
        np.testing.assert_allclose(b, want_b, rtol=1e-14, atol=0)
        np.testing.assert_allclose(corrected, want_eff, rtol=1e-14, atol=0)
        assert corrected[5] == eff[5] and corrected[8] == eff[8] and corrected[9] == eff[9]
        if observed.sum() == 0 or tpm.sum() == 0:
            assert (b == 1).all()
            np.testing.assert_allclose(corrected, eff, rtol=1e-15, atol=0)
        else:
            assert (b[expected == 0] == 1).all() and (expected == 0).any()
    assert (ref.correct(tx_windows, cases[2][0], single, eff, strand)[0] == 0).sum() > 3000


def test_hexamer_codes_and_observed_counts():
    assert ref.hexamer_code(b'AAAAAA') == 0 and ref.hexamer_code(b'TTTTTT') == 4095
    assert ref.hexamer_code(b'CAAAAA') == 1 << 10 and ref.hexamer_code(b'AAAAAG') == 2
    assert ref.hexamer_code(b'ACGTNA') == -1 and ref.hexamer_code(b'acgtac') == -1
    for six in (b'ACGTAC', b'GGGTCA', b'TTTAAA'):
        assert int(ref.revcomp_code(ref.hexamer_code(six))) == ref.hexamer_code(ref.reverse_complement(six))
    reads = [b'ACGTACNNNN', b'ACGTAcGGGG', b'ACGTANGGGG', b'ACGTACGGGG', b'ACGTA', b'TTTTTTN']
    counts = ref.observed_counts(reads, [True, True, True, False, True, True])
    assert counts.sum() == 2 and counts[ref.hexamer_code(b'ACGTAC')] == 1 and counts[4095] == 1


def test_command_line():
    from seekmer_amd import __main__ as cli
    assert cli.parse_args(['infer', 'index', 'out', 'a.fq', 'b.fq'])['bias'] is False
    assert cli.parse_args(['infer', 'index', 'out', 'a.fq', 'b.fq', '--bias'])['bias'] is True
    opts = cli.parse_args(['infer-many', 'index', 'out', 'a.fq', 'b.fq', '--bias', '--rf-stranded'])
    assert opts['bias'] is True and opts['strand'] == 'rf'
    assert cli.parse_args(['infer-many', 'index', 'out', 'a.fq', 'b.fq'])['bias'] is False
    assert 'bias' not in cli.parse_args(['impute', 'index', 'out', 'a.fq', 'b.fq'])
    with pytest.raises(SystemExit):
        cli.parse_args(['impute', 'index', 'out', 'a.fq', 'b.fq', '--bias'])


def test_several_ranks_refuse_bias(tmp_path, monkeypatch):
    """A run on more than one rank says that --bias is for one GPU, before it touches a file or a device."""
    from seekmer_amd import infer

    class TwoRanks:
        world, rank, local_rank, shard = 2, 0, 0, (0, 2)

    with pytest.raises(ValueError, match='--bias runs in one process'):
        infer._run(TwoRanks(), None, tmp_path / 'index.npz', tmp_path / 'out', [], 1, False, False, 0, False, 0, None,
                   None, bias=True)
    assert not (tmp_path / 'out').exists()


def test_bias_correct_checks_its_arguments_before_any_device_work(native_libs):
    import ctypes
    hip = native_libs.hip()
    zeros = np.zeros(4096, dtype=np.int64)
    one = np.ones(1)
    args = (native_libs.ptr(zeros, native_libs.c_i64p), native_libs.ptr(one, native_libs.c_f64p),
            native_libs.ptr(one, native_libs.c_f64p), 1, None, None, native_libs.ptr(one, native_libs.c_f64p))
    assert hip.skm_bias_correct(None, 0, *args) == native_libs.SKM_ERR_ARG
    assert hip.skm_index_build_transcripts(None, native_libs.ptr(one, native_libs.c_f64p), 1) == native_libs.SKM_ERR_ARG
    assert hip.skm_index_transcript_bases(None, None, None) == native_libs.SKM_ERR_ARG
    assert hip.skm_mapper_set_bias(None, 1) == native_libs.SKM_ERR_ARG
    assert hip.skm_mapper_bias_observed(None, native_libs.ptr(zeros, native_libs.c_i64p)) == native_libs.SKM_ERR_ARG
    assert ctypes.c_char_p(hip.skm_last_error()).value
