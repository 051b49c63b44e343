"""slk_als_gram / slk_als_solve / slk_als_loss and ALSFactorizationModel on the real gfx950 library: the checks of
tests/test_emu_als.py over the full grid of dims and table sizes, and the model-level checks of tests/test_host_als.py."""
import pytest

import als_checks as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('n', ac.TABLES)
@pytest.mark.parametrize('D', ac.DS)
def test_gram(be, D, n):
    ac.check_gram(be, D, n)


def test_gram_at_the_cap_of_partial_tiles(be):
    """300 000 rows: more row chunks than 1024 partial tiles of 256 rows hold, so workgroups walk chunks a grid apart."""
    ac.check_gram(be, 6, 300000)


def test_gram_of_no_rows(be):
    ac.check_gram_empty(be)


@pytest.mark.parametrize('I', ac.TABLES)
@pytest.mark.parametrize('D', ac.DS)
def test_half_step_against_float64(be, D, I):
    ac.check_half_step(be, D, I)


@pytest.mark.parametrize('I', ac.TABLES)
@pytest.mark.parametrize('D', ac.DS)
def test_composition_invariance(be, D, I):
    ac.check_composition(be, D, I)


def test_failed_rows_are_counted_and_left_untouched(be):
    ac.check_failure(be)


@pytest.mark.parametrize('D', [24, 72])
def test_objective(be, D):
    ac.check_loss(be, D)


def test_refusals(be):
    ac.check_refusals(be)


def test_profile_classes(be):
    ac.check_profile_classes(be)


# ---- model level ------------------------------------------------------------------------------------------------------------------
def test_fit_against_the_float64_restatement():
    ac.check_model_fit_against_float64()


def test_determinism_and_weights():
    ac.check_model_determinism_and_weights()


def test_fold_in_recommend_evaluation_pickle():
    ac.check_model_serving()


def test_a_representation_of_another_dim_than_the_keyword():
    ac.check_model_representation_dim_wins()


def test_failed_rows_and_open_scopes():
    import torch
    from spotlight_amd.factorization import implicit as host
    device = host._model_device()
    ac.check_model_failure_and_scope(host._engine_for(device), torch.cuda.current_stream(device).cuda_stream)
