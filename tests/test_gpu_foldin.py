"""slk_bilinear_foldin and the models' fold_in() / recommend_vectors() on the real gfx950 library: the checks of
tests/test_emu_foldin.py and tests/test_host_foldin.py, the closed loop over every (loss, kind) pair at every dim."""
import pytest

import foldin_checks as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


PAIRS = [(loss, opt) for loss in fc.LOSSES for opt in fc.KINDS]


@pytest.mark.parametrize('D,n,opt', fc.WIDE)
def test_adaptive_hinge_over_many_candidates_against_the_oracle(be, D, n, opt):
    fc.check_wide_adaptive(be, D, n, opt)


@pytest.mark.parametrize('D', fc.DS)
@pytest.mark.parametrize('i', range(len(PAIRS)))
def test_closed_loop_against_the_oracle(be, i, D):
    loss, opt = PAIRS[i]
    j = i + fc.DS.index(D)  # (I, H) rotate with the pair and the dim: every combination of the two occurs at every dim
    fc.check_closed_loop(be, loss, opt, D, fc.ITEMS[j % 2], fc.USERS[(j // 2) % 3])


@pytest.mark.parametrize('loss,opt', [('bpr', 'adagrad'), ('adaptive_hinge', 'adam_dense')])
def test_item_side_is_frozen(be, loss, opt):
    fc.check_frozen(be, loss, opt)


@pytest.mark.parametrize('I', fc.ITEMS)
@pytest.mark.parametrize('loss,opt,D', [('bpr', 'adagrad', 64), ('pointwise', 'sparse_adam', 6), ('adaptive_hinge', 'adagrad_dense', 72),
                                        ('hinge', 'sgd', 24), ('bpr', 'adam_dense', 24)])
def test_batch_composition_invariance(be, loss, opt, D, I):
    fc.check_batch_composition(be, loss, opt, D, I)


@pytest.mark.parametrize('I', fc.ITEMS)
@pytest.mark.parametrize('loss,opt,D', [('bpr', 'adam_dense', 64), ('pointwise', 'adagrad_dense', 24), ('adaptive_hinge', 'sparse_adam', 6),
                                        ('hinge', 'adagrad', 72), ('bpr', 'sgd', 64)])
def test_step_composition(be, loss, opt, D, I):
    fc.check_step_composition(be, loss, opt, D, I)


def test_step_composition_across_chained_launches(be):
    fc.check_step_composition(be, 'bpr', 'adam_dense', 24, 333, H=3, T=17, lengths=[3, 0, 9])


def test_empty_histories(be):
    fc.check_empty(be)


def test_refusals(be):
    fc.check_refusals(be)


def test_profiled_as_user_pass(be):
    fc.check_profiled_as_user_pass(be)


# ---- model level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,loss', [('adagrad', 'bpr'), ('sgd', 'hinge'), ('sparse_adam', 'pointwise'), ('adam_dense', 'adaptive_hinge'),
                                       ('adagrad_dense', 'bpr'), ('adam_dense', 'pointwise'), ('adagrad', 'adaptive_hinge')])
def test_fused_fold_in_equals_the_generic_route(kind, loss):
    fc.check_model_fused_equals_generic(kind, loss)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_fold_in_consumes_the_random_state_as_sample_items_would(loss):
    fc.check_model_random_state(loss)


def test_recommend_vectors_over_trained_rows_is_recommend():
    fc.check_recommend_vectors()


def test_routes_and_refusals():
    fc.check_model_routes_and_refusals()


def test_refused_inside_an_open_fit_scope():
    import torch
    from spotlight_amd.factorization import implicit as host
    device = host._model_device()
    fc.check_fold_in_refused_inside_an_open_fit_scope(host._engine_for(device), torch.cuda.current_stream(device).cuda_stream)
