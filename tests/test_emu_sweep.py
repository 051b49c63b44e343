"""The scoring sweep with several item blocks per workgroup (tests/sweep_checks.py) on the emulator build of the engine sources:
the block loop, the hand-over of the prefetch, the re-staged representations and the ragged last chunk under every cut
"eval_items_per_wg" offers.  The same checks run on the gfx950 library in tests/test_gpu_sweep.py, where the matrix-core branch
and real barriers are under test; the device-sized tables (the device's own cut, the packed counters' capacity) run only there."""
import pytest

import sweep_checks as sw
from emu_backend import EmuBackend


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


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
