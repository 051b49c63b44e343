"""Top-k entries (slk_bilinear_topk / slk_poolnet_topk / slk_shard_topk) on the emulator build of the engine sources.  The same
checks run on the gfx950 library in tests/test_gpu_topk.py, there over the full grid of shapes; here every value of every axis
occurs at least once."""
import pytest

import topk_checks as tc
from emu_backend import EmuBackend

K_MAX = tc.K_MAX


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('D,I,n_rows,k', [(6, 7, 1, 1), (6, 333, 33, 10), (6, 1500, 65, K_MAX), (24, 7, 150, 10), (24, 333, 65, 1),
                                          (24, 1500, 33, 10), (72, 7, 33, K_MAX), (72, 333, 150, K_MAX), (72, 1500, 1, 10),
                                          (24, 333, 150, 1)])
def test_random_tables(be, D, I, n_rows, k):
    tc.check_random(be, D, I, n_rows, k)


@pytest.mark.parametrize('user_bloom', [0, 2])
def test_bloom_tables(be, user_bloom):
    tc.check_bloom(be, user_bloom=user_bloom)


@pytest.mark.parametrize('D,I,n_seq,k,bloom', [(6, 333, 33, 10, 0), (24, 1500, 65, K_MAX, 0), (72, 7, 1, 1, 0), (24, 333, 65, 10, 2)])
def test_poolnet(be, D, I, n_seq, k, bloom):
    tc.check_poolnet(be, D, I, n_seq, k, bloom)


@pytest.mark.parametrize('k', tc.KS)
def test_ties_across_the_k_boundary(be, k):
    tc.check_ties(be, k)


@pytest.mark.parametrize('k', tc.KS)
def test_all_zero_tables(be, k):
    tc.check_all_zero(be, k)


def test_signed_zero_pair(be):
    tc.check_signed_zero_pair(be)


@pytest.mark.parametrize('descending', [False, True])
@pytest.mark.parametrize('k', tc.KS)
def test_worst_case_insertion(be, k, descending):
    tc.check_worst_case_insertion(be, k, descending)


@pytest.mark.parametrize('k', [10, K_MAX])
def test_chunking_invariance(be, k):
    tc.check_chunking_invariance(be, k)


def test_exclusion_cases(be):
    tc.check_exclusion_cases(be)


def test_k_above_the_item_count(be):
    tc.check_k_above_items(be)


def test_nan_orders_last(be):
    tc.check_nan(be)


@pytest.mark.parametrize('W', [2, 3])
@pytest.mark.parametrize('D,I,n_rows,k', [(6, 7, 33, 10), (24, 333, 65, K_MAX), (72, 1500, 150, 10), (24, 7, 1, 1)])
def test_shards_merge_to_the_one_device_result(be, D, I, n_rows, k, W):
    tc.check_shards(be, D, I, n_rows, k, W)


def test_refusals(be):
    tc.check_refusals(be)


def test_profile_survives_a_refusal(be):
    tc.check_profile_survives_refusal(be)
