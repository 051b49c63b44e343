"""loss='warp' (SLK_LOSS_WARP) on the emulator build: tests/warp_checks.py.  The same checks run on the gfx950 library in
tests/test_gpu_warp.py; the model level is tests/test_host_warp.py."""
import pytest

import foldin_checks as fc
import warp_checks as wk


@pytest.fixture(scope='module')
def be():
    from emu_backend import EmuBackend
    b = EmuBackend()
    yield b
    b.close()


# ---- the guard's seeds (no engine) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,D,n,I', wk.CLOSED)
def test_the_seeds_keep_the_restatement_away_from_ties(kind, D, n, I):
    wk.check_seed_meets_the_guard(kind, D, n, I)


@pytest.mark.parametrize('kind', wk.KINDS)
def test_the_weighted_seeds_keep_the_restatement_away_from_ties(kind):
    wk.check_seed_meets_the_guard(kind, 24, 3, 333, weights='case')


@pytest.mark.parametrize('D,I,H,n', wk.FOLD_CLOSED + wk.FOLD_CLOSED_7)
def test_the_fold_in_seeds_keep_the_restatement_away_from_ties(D, I, H, n):
    wk.check_fold_seed_meets_the_guard(D, I, H, n)


# ---- 1 + 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', wk.ROUTES)
@pytest.mark.parametrize('kind,D,n,I', wk.CLOSED)
def test_closed_loop_matches_the_float64_restatement(be, kind, D, n, I, route):
    wk.check_closed_loop(be, kind, D, n, I, route)


@pytest.mark.parametrize('kind', wk.KINDS)
def test_weighted_closed_loop_matches_the_float64_restatement(be, kind):
    wk.check_closed_loop(be, kind, 24, 3, 333, 'launch', weights='case')


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', wk.KINDS)
def test_persistent_route_is_the_launch_path_bit_for_bit(be, kind):
    for D, n in zip(wk.DS, (5, 3, 1, 5)):
        wk.check_routes_agree(be, kind, D, n)
    wk.check_routes_agree(be, kind, 24, 5, I=7)


@pytest.mark.parametrize('weights', [None, 'case'])
def test_chunking_is_bit_neutral_and_the_call_deterministic(be, weights):
    wk.check_chunking_and_determinism(be, weights)


def test_inside_the_training_scopes(be):
    wk.check_scopes(be)


@pytest.mark.parametrize('kind', wk.KINDS)
def test_all_ones_is_the_unweighted_staged_call(be, kind):
    wk.check_all_ones_is_the_unweighted_staged_call(be, kind)


def test_a_power_of_two_on_every_weight_changes_no_bit(be):
    wk.check_power_of_two_scaling(be)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', wk.ROUTES)
@pytest.mark.parametrize('how', ['two_items', 'no_violator'])
@pytest.mark.parametrize('kind', wk.SPARSE)
def test_a_step_without_a_live_column_changes_no_bit(be, kind, how, route):
    wk.check_nothing_is_live(be, kind, route, how)


@pytest.mark.parametrize('route', wk.ROUTES)
def test_every_column_violating_at_row_zero(be, route):
    wk.check_every_column_violates_at_row_zero(be, route)


@pytest.mark.parametrize('route', wk.ROUTES)
def test_a_nan_candidate_is_skipped(be, route):
    wk.check_nan_candidate_is_skipped(be, route)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('opt', wk.KINDS)
def test_fold_in_closed_loop(be, opt):
    for D, I, H, n in wk.FOLD_CLOSED + [wk.FOLD_CLOSED_7[wk.KINDS.index(opt) % 4]]:
        wk.check_fold_closed_loop(be, opt, D, I, H, n)


@pytest.mark.parametrize('D,n,opt', wk.FOLD_WIDE)
def test_the_wide_fold_in_seeds_keep_the_restatement_away_from_ties(D, n, opt):
    for o in ('sgd', opt):
        wk.check_fold_seed_meets_the_guard(D, 333, 5, n, opt=o, pr=wk.wide_problem(D, n))


@pytest.mark.parametrize('D,n,opt', wk.FOLD_WIDE)
def test_fold_in_closed_loop_over_many_candidates(be, D, n, opt):
    wk.check_fold_closed_loop(be, opt, D, 333, 5, n, pr=wk.wide_problem(D, n))


@pytest.mark.parametrize('D', wk.DS)
def test_fold_in_batch_and_step_composition(be, D):
    for I, n in ((333, 3), (7, 5)):
        wk.check_fold_batch_composition(be, 'adagrad', D, I, n)
        wk.check_fold_step_composition(be, 'adam_dense', D, I, n)


def test_fold_in_item_side_is_frozen(be):
    wk.check_fold_frozen(be, 'sparse_adam')


def test_fold_in_degenerate_columns(be):
    wk.check_fold_degenerate(be)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(be):
    wk.check_refusals(be)
