"""Neighbour entries (slk_rows_inv_norm / slk_neighbors_topk / slk_neighbors_scores) on the real gfx950 library: the checks of
tests/test_emu_neighbors.py over the full grid of shapes."""
import pytest

import neighbors_checks as nc

pytestmark = pytest.mark.gpu
K_MAX = nc.K_MAX


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('k', nc.KS)
@pytest.mark.parametrize('n_q', nc.ROWS)
@pytest.mark.parametrize('I', nc.ITEMS)
@pytest.mark.parametrize('D', nc.DS)
def test_random_tables(be, D, I, n_q, k):
    nc.check_random(be, D, I, n_q, k)


@pytest.mark.parametrize('D', nc.DS)
def test_inverse_norms(be, D):
    nc.check_inverse_norms(be, D)


@pytest.mark.parametrize('D', nc.DS)
def test_cosine_and_dot_values(be, D):
    nc.check_cosine_values(be, D)


def test_ties_across_the_k_boundary(be):
    nc.check_ties(be)


def test_zero_rows_and_zero_queries(be):
    nc.check_zero_rows(be)


def test_nan_orders_last(be):
    nc.check_nan(be)


def test_signed_zero_pair(be):
    nc.check_signed_zero_pair(be)


def test_exclusion_cases(be):
    nc.check_exclusion_cases(be)


def test_k_above_the_row_count(be):
    nc.check_k_above_rows(be)


@pytest.mark.parametrize('k', nc.KS)
def test_chunking_invariance(be, k):
    nc.check_chunking_invariance(be, k)


def test_existing_sweeps_untouched(be):
    nc.check_existing_sweeps_untouched(be)


def test_refusals(be):
    nc.check_refusals(be)
