"""The models' `negative_sampling` keyword on the real gfx950 library: the checks of tests/test_host_negative_sampling.py."""
import pytest

import negative_sampling_checks as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_hand_in_is_exact(loss):
    nc.check_hand_in_is_exact(loss)


def test_uniform_and_none_change_nothing():
    nc.check_uniform_is_untouched()


def test_large_epochs_take_the_hand_in_schedule_and_never_prefetch(monkeypatch):
    nc.check_large_epochs_take_the_hand_in_schedule(monkeypatch)


def test_popularity_weights_and_absent_items(monkeypatch):
    nc.check_popularity_weights(monkeypatch)


@pytest.mark.parametrize('loss,representation', [('bpr', 'pooling'), ('adaptive_hinge', 'pooling'), ('bpr', 'lstm')])
def test_sequence_model_replays_choice_per_minibatch(monkeypatch, loss, representation):
    nc.check_sequence_model(monkeypatch, loss, representation=representation)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_fold_in_draws_from_the_distribution_of_the_last_fit(loss):
    nc.check_fold_in(loss)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_autograd_route_consumes_the_same_stream(loss):
    nc.check_autograd_route(loss)


@pytest.mark.parametrize('which', sorted(nc.BAD_WEIGHTS))
def test_bad_weights_raise_before_anything_is_drawn(which):
    nc.check_validation_errors(which)


def test_sampling_module_host_and_device_forms():
    import torch
    from spotlight_amd.factorization import implicit as host
    device = host._model_device()
    nc.check_sampling_module(host._engine_for(device), device)


def test_repr_and_pickle():
    nc.check_repr_and_pickle()
