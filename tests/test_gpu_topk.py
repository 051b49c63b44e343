"""Top-k entries (slk_bilinear_topk / slk_poolnet_topk / slk_shard_topk) on the real gfx950 library: the checks of
tests/test_emu_topk.py over the full grid of shapes."""
import pytest

import topk_checks as tc

pytestmark = pytest.mark.gpu
K_MAX = tc.K_MAX


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('n_rows', tc.ROWS)
@pytest.mark.parametrize('I', tc.ITEMS)
@pytest.mark.parametrize('D', tc.DS)
def test_random_tables(be, D, I, n_rows, k):
    tc.check_random(be, D, I, n_rows, k)


@pytest.mark.parametrize('user_bloom', [0, 2])
def test_bloom_tables(be, user_bloom):
    tc.check_bloom(be, user_bloom=user_bloom)


@pytest.mark.parametrize('bloom', [0, 2])
@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('D,I,n_seq', [(6, 333, 33), (24, 1500, 65), (72, 7, 1), (72, 1500, 150)])
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


@pytest.mark.parametrize('k', tc.KS)
def test_chunking_invariance(be, k):
    tc.check_chunking_invariance(be, k)


def test_exclusion_cases(be):
    tc.check_exclusion_cases(be)


def test_k_above_the_item_count(be):
    tc.check_k_above_items(be)


def test_nan_orders_last(be):
    tc.check_nan(be)


@pytest.mark.parametrize('W', [2, 3])
@pytest.mark.parametrize('k', tc.KS)
@pytest.mark.parametrize('D,I,n_rows', [(6, 7, 33), (24, 333, 65), (72, 1500, 150), (24, 7, 1), (6, 1500, 65)])
def test_shards_merge_to_the_one_device_result(be, D, I, n_rows, k, W):
    tc.check_shards(be, D, I, n_rows, k, W)


def test_refusals(be):
    tc.check_refusals(be)


def test_profile_survives_a_refusal(be):
    tc.check_profile_survives_refusal(be)
