"""loss='softmax' (SLK_LOSS_SOFTMAX) on the emulator build: tests/softmax_checks.py.  The same checks run on the gfx950 library in
tests/test_gpu_softmax.py; the model level is tests/test_host_softmax.py."""
import pytest

import softmax_checks as sm


@pytest.fixture(scope='module')
def be():
    from emu_backend import EmuBackend
    b = EmuBackend()
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
