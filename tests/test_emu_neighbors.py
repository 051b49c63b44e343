"""Neighbour entries (slk_rows_inv_norm / slk_neighbors_topk / slk_neighbors_scores) on the emulator build of the engine sources.
The same checks run on the gfx950 library in tests/test_gpu_neighbors.py, there over the full grid of shapes; here every value
of every axis occurs at least once."""
import pytest

import neighbors_checks as nc
from emu_backend import EmuBackend

K_MAX = nc.K_MAX


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('D,I,n_q,k', [(6, 7, 1, 1), (6, 333, 33, 10), (6, 1500, 65, K_MAX), (24, 7, 150, 10), (24, 333, 65, 1),
                                       (24, 1500, 33, 10), (72, 7, 33, K_MAX), (72, 333, 150, K_MAX), (72, 1500, 1, 10)])
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


@pytest.mark.parametrize('k', [10, K_MAX])
def test_chunking_invariance(be, k):
    nc.check_chunking_invariance(be, k)


def test_existing_sweeps_untouched(be):
    nc.check_existing_sweeps_untouched(be)


def test_refusals(be):
    nc.check_refusals(be)
