"""loss='softmax' (SLK_LOSS_SOFTMAX) on the real gfx950 library: the checks of tests/softmax_checks.py that
tests/test_emu_softmax.py runs on the emulator build, and the model-level cases of tests/test_host_softmax.py on the device."""
import pytest

import softmax_checks as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('kind,D,n,I', sm.CLOSED)
def test_closed_loop_matches_the_float64_restatement(be, kind, D, n, I):
    sm.check_closed_loop(be, kind, D, n, I)


@pytest.mark.parametrize('kind', sm.KINDS)
def test_weighted_closed_loop_matches_the_float64_restatement(be, kind):
    sm.check_closed_loop(be, kind, 24, 3, 333, weights='case')


@pytest.mark.parametrize('kind', ['adagrad', 'sparse_adam'])
def test_closed_loop_over_a_bloom_item_table(be, kind):
    sm.check_closed_loop(be, kind, 24, 3, 333, item_bloom=2)


def test_each_positive_meets_its_own_users_draws(be):
    sm.check_own_user_layout(be)


@pytest.mark.parametrize('n', sm.NS)
def test_all_zero_tables_give_log_n_plus_one_and_uniform_gradients(be, n):
    sm.check_all_zero_tables(be, n)


def test_one_negative_is_softplus(be):
    sm.check_one_negative_is_softplus(be)


@pytest.mark.parametrize('opposite', [False, True])
@pytest.mark.parametrize('bias', [100.0, -100.0])
def test_score_gaps_of_a_hundred_stay_finite_and_exact(be, bias, opposite):
    sm.check_stability(be, bias, opposite)


def test_a_plain_call_takes_the_launch_path(be):
    sm.check_route(be)


@pytest.mark.parametrize('weights', [None, 'case'])
def test_chunking_is_bit_neutral_and_the_call_deterministic(be, weights):
    sm.check_chunking_and_determinism(be, weights)


def test_inside_the_training_scopes(be):
    sm.check_scopes(be)


@pytest.mark.parametrize('kind', sm.KINDS)
def test_all_ones_is_the_unweighted_call(be, kind):
    sm.check_all_ones_is_the_unweighted_call(be, kind)


def test_a_power_of_two_on_every_weight_changes_no_bit(be):
    sm.check_power_of_two_scaling(be)


def test_refusals_through_the_c_abi(be):
    sm.check_refusals(be)


# ---- model level, on the device: the bodies of tests/test_host_softmax.py (their emulator fixture only points the models' device
# hooks at the emulator; here the hooks stay the real ones)
@pytest.mark.parametrize('kw', [{}, dict(use_weights=True), dict(negative_sampling='popularity')],
                         ids=lambda kw: '+'.join(sorted(kw)) or 'plain')
def test_fit_trains_and_consumes_the_random_state_as_adaptive_hinge_does(kw):
    import test_host_softmax as hs
    hs.test_fit_trains_and_consumes_the_random_state_as_adaptive_hinge_does(None, kw)


def test_verified_negatives_fit_and_count():
    import test_host_softmax as hs
    hs.test_verified_negatives_fit_and_count(None)


def test_one_minibatch_matches_softmax_loss_through_autograd():
    import test_host_softmax as hs
    hs.test_one_minibatch_matches_softmax_loss_through_autograd(None)


def test_generic_routes_train_through_softmax_loss():
    import test_host_softmax as hs
    hs.test_custom_representation_and_unfused_optimizer_train_through_softmax_loss(None)


def test_fold_in_runs_the_generic_route():
    import test_host_softmax as hs
    hs.test_fold_in_runs_the_generic_route_and_draws_num_negative_samples_per_position(None)
