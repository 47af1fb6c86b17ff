"""The fragment-length model (--fragment-length / --sd) as far as it goes without a GPU: the weights, the
exported symbols and the command line."""
import numpy as np
import pytest

import length_model_reference as reference


@pytest.mark.parametrize('model', reference.MODELS)
def test_weights(model):
    from seekmer_amd import mapper
    p = mapper.fragment_length_weights(*model)
    assert p.shape == (2000,) and p.dtype == np.float64
    assert p[0] == 0 and (p >= 0).all() and np.isfinite(p).all()
    assert abs(p.sum() - 1.0) <= 2000 * np.finfo('f8').eps
    np.testing.assert_array_equal(p, reference.weights(*model))


@pytest.mark.parametrize('mean, sd', [(0, 20), (-3, 20), (2000, 20), (2500.5, 20), (float('nan'), 20), (float('inf'), 20),
                                      (200, 0), (200, -1), (200, float('inf')), (200, float('nan')), (100.5, 1e-3)])
def test_weights_that_cannot_be(mean, sd):
    from seekmer_amd import mapper
    with pytest.raises(ValueError):
        mapper.fragment_length_weights(mean, sd)


def test_the_numpy_rule_on_a_point_mass():
    """One bin of weight 1 at i: eff = max(len - i, 1), so the rule's clamp is where it should be."""
    p = np.zeros(2000)
    p[200] = 1.0
    np.testing.assert_array_equal(reference.effective_lengths(p, [1, 200, 201, 202, 1000]), [1, 1, 1, 2, 800])


def test_the_symbols_are_exported_and_fail_without_a_gpu(native_libs):
    hip = native_libs.hip()
    for name in ('skm_effective_lengths_weights', 'skm_mapper_set_length_weights', 'skm_sample_set_set_length_weights'):
        assert name in native_libs.HIP_SYMBOLS and hasattr(hip, name)
    if native_libs.device_count() > 0:
        return
    p = np.ascontiguousarray(reference.weights(200, 20))
    lengths, out = np.ones(4), np.zeros(4)
    f64 = native_libs.c_f64p
    assert hip.skm_effective_lengths_weights(0, 1, native_libs.ptr(p, f64), native_libs.ptr(lengths, f64), 4,
                                             native_libs.ptr(out, f64)) == native_libs.SKM_ERR_NO_DEVICE
    assert hip.skm_mapper_set_length_weights(None, native_libs.ptr(p, f64)) == native_libs.SKM_ERR_NO_DEVICE
    assert hip.skm_sample_set_set_length_weights(None, native_libs.ptr(p, f64)) == native_libs.SKM_ERR_NO_DEVICE
    assert b'no HIP device' in hip.skm_last_error()


def test_bad_weights_are_refused_before_any_device_work(native_libs):
    """SKM_ERR_ARG whether or not there is a GPU: the check comes first."""
    hip = native_libs.hip()
    f64 = native_libs.c_f64p
    lengths, out = np.ones(4), np.zeros(4)
    for bad in (-1e-300, float('nan'), float('inf')):
        p = np.ascontiguousarray(np.stack([reference.weights(200, 20)] * 2))
        p[1, 1999] = bad
        assert hip.skm_effective_lengths_weights(0, 2, native_libs.ptr(p, f64), native_libs.ptr(lengths, f64), 4,
                                                 native_libs.ptr(out, f64)) == native_libs.SKM_ERR_ARG
    p = np.ascontiguousarray(reference.weights(200, 20))
    assert hip.skm_effective_lengths_weights(0, -1, native_libs.ptr(p, f64), native_libs.ptr(lengths, f64), 4,
                                             native_libs.ptr(out, f64)) == native_libs.SKM_ERR_ARG
    assert hip.skm_effective_lengths_weights(0, 1, native_libs.ptr(p, f64), native_libs.ptr(lengths, f64), -4,
                                             native_libs.ptr(out, f64)) == native_libs.SKM_ERR_ARG
    for args in ((None, native_libs.ptr(lengths, f64), native_libs.ptr(out, f64)),
                 (native_libs.ptr(p, f64), None, native_libs.ptr(out, f64)),
                 (native_libs.ptr(p, f64), native_libs.ptr(lengths, f64), None)):
        assert hip.skm_effective_lengths_weights(0, 1, args[0], args[1], 4, args[2]) == native_libs.SKM_ERR_ARG


COMMANDS = (['infer', 'ix', 'out', 'a.fq'], ['infer-many', 'ix', 'out', 'a.fq', 'b.fq'], ['impute', 'ix', 'out', 'a.fq', 'b.fq'])


@pytest.mark.parametrize('command', COMMANDS, ids=[command[0] for command in COMMANDS])
def test_the_options_go_together(command, capsys):
    from seekmer_amd.__main__ import parse_args
    for alone in (['--fragment-length', '200'], ['-l', '200'], ['--sd', '20']):
        with pytest.raises(SystemExit) as error:
            parse_args(command + ['-s'] + alone)
        assert error.value.code == 2 and 'go together' in capsys.readouterr().err
    for both in (['-l', '200', '--sd', '20'], ['--fragment-length', '187.5', '--sd', '12.25']):
        for single in ([], ['-s']):                 # (allowed for paired reads too)
            opts = parse_args(command + single + both)
            assert opts['length_model'] == (float(both[1]), float(both[3])) and opts['single_ended'] == bool(single)
            assert 'fragment_length' not in opts and 'sd' not in opts
    assert parse_args(command)['length_model'] is None
    with pytest.raises(SystemExit):                 # a model that cannot be is said at the command line
        parse_args(command + ['-l', '2000', '--sd', '20'])


def test_run_info_names_the_model_only_when_there_is_one():
    import datetime
    import types
    from seekmer_amd import infer
    index = types.SimpleNamespace(transcripts=np.zeros(3))
    results = dict(class_map=np.asarray([[0, 1], [0, 2]]), class_count=np.asarray([2.0, 3.0]), total=6, aligned=5)
    start = datetime.datetime(2020, 1, 1)
    plain = infer._generate_run_info([], index, types.SimpleNamespace(**results), start)
    assert 'fragment_length_model' not in plain
    assert infer._generate_run_info([], index, types.SimpleNamespace(length_model=None, **results), start) == plain
    with_model = infer._generate_run_info([], index, types.SimpleNamespace(length_model=(200.0, 20.0), **results), start)
    assert with_model.pop('fragment_length_model') == {'mean': 200.0, 'sd': 20.0} and with_model == plain
