"""The models' `negative_sampling` keyword through the emulator build of the kernels (no GPU).  The same checks run on the
gfx950 library in tests/test_gpu_negative_sampling.py."""
import pytest
import torch

import negative_sampling_checks as nc
from emu_backend import emu_lib
from spotlight_amd import _native
from spotlight_amd.factorization import implicit as host


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_hand_in_is_exact(emu_device, loss):
    nc.check_hand_in_is_exact(loss)


def test_uniform_and_none_change_nothing(emu_device):
    nc.check_uniform_is_untouched()


def test_large_epochs_take_the_hand_in_schedule_and_never_prefetch(emu_device, monkeypatch):
    nc.check_large_epochs_take_the_hand_in_schedule(monkeypatch)


def test_popularity_weights_and_absent_items(emu_device, monkeypatch):
    nc.check_popularity_weights(monkeypatch)


@pytest.mark.parametrize('loss,representation', [('bpr', 'pooling'), ('adaptive_hinge', 'pooling'), ('bpr', 'lstm')])
def test_sequence_model_replays_choice_per_minibatch(emu_device, monkeypatch, loss, representation):
    nc.check_sequence_model(monkeypatch, loss, representation=representation)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_fold_in_draws_from_the_distribution_of_the_last_fit(emu_device, loss):
    nc.check_fold_in(loss)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_autograd_route_consumes_the_same_stream(emu_device, loss):
    nc.check_autograd_route(loss)


@pytest.mark.parametrize('which', sorted(nc.BAD_WEIGHTS))
def test_bad_weights_raise_before_anything_is_drawn(emu_device, which):
    nc.check_validation_errors(which)


def test_sharded_model_refuses_the_keyword():
    nc.check_sharded_model_refuses()


def test_sampling_module_host_and_device_forms(emu_device):
    nc.check_sampling_module(emu_device, torch.device('cpu'))


def test_repr_and_pickle(emu_device):
    nc.check_repr_and_pickle()
