"""The models' `verify_negatives` keyword through the emulator build of the kernels (no GPU), the numpy restatement of the
rule against a loop over Python sets, and the refusals.  The model checks run on the gfx950 library in
tests/test_gpu_verify_negatives.py."""
import pytest
import torch

import verify_negatives_checks as vc
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


def test_restatement_equals_a_loop_over_sets():
    vc.check_restatement_against_sets()


def test_seen_items_csr_and_validation():
    vc.check_seen_items_class()


def test_seen_items_bind_builds_the_host_csr_on_the_device(emu_device):
    vc.check_seen_items_bind(emu_device, torch.device('cpu'))


@pytest.mark.parametrize('variant', vc.VARIANTS)
@pytest.mark.parametrize('loss', vc.LOSSES)
def test_fit_equals_the_restated_hand_in(emu_device, monkeypatch, loss, variant):
    vc.check_fit_equals_restated_hand_in(monkeypatch, loss, variant)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_one_try_is_the_unverified_fit(emu_device, loss):
    vc.check_one_try_is_the_unverified_fit(loss)


def test_candidate_cap_changes_nothing(emu_device, monkeypatch):
    vc.check_candidate_cap_changes_nothing(monkeypatch)


@pytest.mark.parametrize('loss', ['bpr', 'warp'])
def test_autograd_route_uses_the_same_negatives(emu_device, monkeypatch, loss):
    vc.check_autograd_route_uses_the_same_negatives(monkeypatch, loss)


def test_verify_tries_is_checked_at_construction():
    vc.check_constructor_refusals()


def test_sharded_and_sequence_models_refuse_before_anything_is_drawn():
    vc.check_models_that_do_not_verify()


def test_fold_in_stays_unverified(emu_device):
    vc.check_fold_in_stays_unverified()


def test_pickle_drops_the_device_csr_and_fit_rebuilds_it(emu_device):
    vc.check_pickle_drops_the_device_csr()
