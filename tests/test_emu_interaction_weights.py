"""Interaction weights (slk_bilinear_train_weighted) on the emulator build: tests/weights_checks.py.  The same checks run on the
gfx950 library in tests/test_gpu_interaction_weights.py."""
import pytest

import weights_checks as wc


@pytest.fixture(scope='module')
def be():
    from emu_backend import EmuBackend
    b = EmuBackend()
    yield b
    b.close()


# ---- the bound itself (no engine) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', wc.KINDS)
@pytest.mark.parametrize('loss', wc.LOSSES)
def test_fp32_restatement_meets_the_bounds_with_no_element_left_out(loss, kind):
    wc.check_fp32_restatement_within_bounds(loss, kind)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', wc.KINDS)
@pytest.mark.parametrize('loss', wc.LOSSES)
def test_closed_loop_matches_torch_float64(be, loss, kind):
    for D in wc.DIMS:
        wc.check_closed_loop(be, loss, kind, D)


@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_closed_loop_over_an_item_bloom_table(be, loss):
    wc.check_closed_loop(be, loss, 'adagrad', 32, item_bloom=4)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['bpr', 'pointwise'])
def test_integer_weights_equal_repetition(be, loss):
    wc.check_integer_weights_equal_repetition(be, loss)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', wc.KINDS)
@pytest.mark.parametrize('loss', wc.LOSSES)
def test_all_ones_is_the_unweighted_call(be, loss, kind):
    wc.check_all_ones_is_the_unweighted_call(be, loss, kind)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', wc.LOSSES)
def test_a_power_of_two_on_every_weight_changes_no_bit(be, loss):
    wc.check_power_of_two_scaling(be, loss)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge', 'regression'])
def test_chunking_is_bit_neutral_and_the_call_deterministic(be, loss):
    wc.check_chunking_and_determinism(be, loss)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
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
