"""Verified negatives on the real gfx950 library: the kernel checks of tests/test_emu_verify_negatives.py and the model
checks of tests/test_host_verify_negatives.py."""
import pytest

import verify_negatives_checks as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('bm', vc.BATCHES)
def test_ids_and_counters_equal_the_restatement(be, bm):
    vc.check_kernel_equals_restatement(be, bm)


def test_dense_case_every_attempt_and_both_counters(be):
    vc.check_dense_case(be)


def test_empty_call_and_batch_size_beyond_n(be):
    vc.check_empty_call_and_batch_beyond_n(be)


def test_refusals_leave_the_ctx_usable(be):
    vc.check_refusals(be)


@pytest.mark.parametrize('weighted', [False, True], ids=['uniform', 'weighted'])
def test_draw_then_verify_leaves_numpys_state(be, weighted):
    vc.check_draw_then_verify_leaves_numpys_state(be, weighted)


def test_profiled_as_sample(be):
    vc.check_profiled_as_sample(be)


def test_seen_items_bind_builds_the_host_csr_on_the_device():
    from spotlight_amd.factorization import implicit as host
    device = host._model_device()
    vc.check_seen_items_bind(host._engine_for(device), device)


@pytest.mark.parametrize('variant', vc.VARIANTS)
@pytest.mark.parametrize('loss', vc.LOSSES)
def test_fit_equals_the_restated_hand_in(monkeypatch, loss, variant):
    vc.check_fit_equals_restated_hand_in(monkeypatch, loss, variant)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_one_try_is_the_unverified_fit(loss):
    vc.check_one_try_is_the_unverified_fit(loss)


def test_candidate_cap_changes_nothing(monkeypatch):
    vc.check_candidate_cap_changes_nothing(monkeypatch)


@pytest.mark.parametrize('loss', ['bpr', 'warp'])
def test_autograd_route_uses_the_same_negatives(monkeypatch, loss):
    vc.check_autograd_route_uses_the_same_negatives(monkeypatch, loss)


def test_fold_in_stays_unverified():
    vc.check_fold_in_stays_unverified()


def test_pickle_drops_the_device_csr_and_fit_rebuilds_it():
    vc.check_pickle_drops_the_device_csr()
