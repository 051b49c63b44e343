"""The scoring sweep with several item blocks per workgroup (tests/sweep_checks.py) on the real gfx950 library: the full grid
under every cut "eval_items_per_wg" offers, the device's own cut at a table sized from its CU count, and the capacity of the
packed rank counters at more than 2^23 items."""
import pytest

import sweep_checks as sw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.fixture(scope='module')
def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize('n_rows', sw.WRITE_ROWS)
@pytest.mark.parametrize('D', sw.DS)
def test_scores_under_every_cut(be, D, n_rows):
    sw.check_write(be, D, n_rows)


@pytest.mark.parametrize('D', sw.DS)
def test_predict_all_under_every_cut(be, D):
    sw.check_predict_all(be, D)


def test_scores_bloom_item_table(be):
    sw.check_write(be, 24, 65, item_bloom=True)


def test_scores_bloom_user_table(be):
    sw.check_write(be, 24, 33, user_bloom=True)


@pytest.mark.parametrize('D', [6, 72])
def test_poolnet_scores_under_every_cut(be, D):
    sw.check_poolnet_write(be, D, 65)


@pytest.mark.parametrize('n_rows', sw.COUNT_ROWS)
@pytest.mark.parametrize('D', sw.DS)
def test_bilinear_ranks_under_every_cut(be, D, n_rows):
    sw.check_bilinear_ranks(be, D, n_rows)


@pytest.mark.parametrize('n_rows', sw.COUNT_ROWS)
@pytest.mark.parametrize('D', sw.DS)
def test_poolnet_ranks_under_every_cut(be, D, n_rows):
    sw.check_poolnet_ranks(be, D, n_rows)


def test_ranks_bloom_item_table(be):
    sw.check_bilinear_ranks(be, 24, 65, item_bloom=True)


def test_shard_entries_under_a_fixed_cut(be):
    sw.check_shard_entries(be)


def test_option(be):
    sw.check_option(be)


def test_device_cut_matrix_core_sweep(be, num_cus):
    sw.check_device_cut_gemm(be, num_cus)


def test_device_cut_streaming_form(be, num_cus):
    sw.check_device_cut_rows(be, num_cus)


def test_packed_counter_capacity(be):
    sw.check_counter_capacity(be)
