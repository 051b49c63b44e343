"""Interaction weights (slk_bilinear_train_weighted) on the real gfx950 library: the checks of tests/weights_checks.py that
tests/test_emu_interaction_weights.py runs on the emulator build, and the model-level cases on the device."""
import numpy as np
import pytest

import weights_checks as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('kind', wc.KINDS)
@pytest.mark.parametrize('loss', wc.LOSSES)
def test_closed_loop_matches_torch_float64(be, loss, kind):
    for D in wc.DIMS:
        wc.check_closed_loop(be, loss, kind, D)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_closed_loop_over_an_item_bloom_table(be, loss):
    wc.check_closed_loop(be, loss, 'adagrad', 32, item_bloom=4)


@pytest.mark.parametrize('loss', ['bpr', 'pointwise'])
def test_integer_weights_equal_repetition(be, loss):
    wc.check_integer_weights_equal_repetition(be, loss)


@pytest.mark.parametrize('kind', wc.KINDS)
@pytest.mark.parametrize('loss', wc.LOSSES)
def test_all_ones_is_the_unweighted_call(be, loss, kind):
    wc.check_all_ones_is_the_unweighted_call(be, loss, kind)


@pytest.mark.parametrize('loss', wc.LOSSES)
def test_a_power_of_two_on_every_weight_changes_no_bit(be, loss):
    wc.check_power_of_two_scaling(be, loss)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge', 'regression'])
def test_chunking_is_bit_neutral_and_the_call_deterministic(be, loss):
    wc.check_chunking_and_determinism(be, loss)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge', 'poisson'])
def test_tiny_calls(be, loss):
    wc.check_tiny_calls(be, loss)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge', 'regression'])
def test_one_user_holds_half_the_minibatch(be, loss):
    wc.check_long_user(be, loss)


def test_refusals_and_the_pingpong_scope_afterwards(be):
    wc.check_refusals(be)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_inside_an_item_bias_shadow_scope(be, loss):
    wc.check_inside_bias_shadow(be, loss)


# ---- model level, on the device -------------------------------------------------------------------------------------------------------
def _interactions(seed=3, U=60, I=40, N=1500, ratings=False):
    from spotlight_amd.interactions import Interactions
    rs = np.random.RandomState(seed)
    return Interactions(rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32),
                        ratings=rs.randint(1, 6, N).astype(np.float32) if ratings else None,
                        weights=(2.0 ** rs.uniform(-3, 3, N)).astype(np.float32), num_users=U, num_items=I)


def test_implicit_model_trains_on_the_weights():
    import torch
    from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
    data = _interactions()
    fit = lambda use: ImplicitFactorizationModel(loss='bpr', embedding_dim=16, n_iter=3, batch_size=256, use_weights=use,
                                                 optimizer_func=lambda p: torch.optim.Adagrad(p, lr=0.05), sparse=True,
                                                 random_state=np.random.RandomState(7))
    a, b = fit(True), fit(False)
    a.fit(data)
    b.fit(data)
    sa, sb = a.predict(3), b.predict(3)
    assert np.isfinite(sa).all() and not np.array_equal(sa, sb)
    assert all(np.array_equal(x, y) for x, y in zip(a._random_state.get_state()[1:3], b._random_state.get_state()[1:3]))


# The model-level cases of tests/test_host_interaction_weights.py, one of each on the device (their bodies do not touch the emulator
# fixture they name: it only points the models' device hooks at the emulator, and here the hooks stay the real ones).
def test_weighted_fit_consumes_the_unweighted_stream_on_the_device(monkeypatch):
    import test_host_interaction_weights as hw
    hw.test_weighted_fit_differs_and_consumes_the_unweighted_stream(None, monkeypatch, 'adaptive_hinge')
    hw.test_weighted_explicit_fit_differs_and_consumes_the_unweighted_stream(None, monkeypatch, 'regression')


def test_weighted_fit_matches_the_autograd_route_on_the_device():
    import test_host_interaction_weights as hw
    hw.test_weighted_fit_matches_the_weighted_autograd_route(None, 'bpr')
    hw.test_weighted_explicit_fit_matches_a_torch_loop_on_the_weighted_losses(None, 'regression')


def test_validation_pickling_and_the_default_on_the_device():
    import test_host_interaction_weights as hw
    hw.test_bad_weights_raise_before_anything_is_drawn(None, 'nan', False)
    hw.test_bad_weights_raise_before_anything_is_drawn(None, 'none', True)
    hw.test_a_weighted_model_pickles_and_resumes(None, False)
    hw.test_without_the_keyword_a_weights_array_is_ignored_bit_for_bit(None, False)


def test_explicit_model_trains_on_the_weights():
    from spotlight_amd.factorization.explicit import ExplicitFactorizationModel
    data = _interactions(ratings=True)
    fit = lambda use: ExplicitFactorizationModel(loss='regression', embedding_dim=16, n_iter=3, batch_size=256, use_weights=use,
                                                 random_state=np.random.RandomState(7))
    a, b = fit(True), fit(False)
    a.fit(data)
    b.fit(data)
    sa, sb = a.predict(3), b.predict(3)
    assert np.isfinite(sa).all() and not np.array_equal(sa, sb)
    assert all(np.array_equal(x, y) for x, y in zip(a._random_state.get_state()[1:3], b._random_state.get_state()[1:3]))
