"""Sharded evaluation entries (slk_shard_target_scores / _rank_counts / _scores) on the emulator build of the engine sources:
W shards swept one by one in this process against the one-device fused ranking.  The same checks run on the gfx950 library in
tests/test_gpu_shard_eval.py."""
import pytest

import shard_eval_checks as sc
from emu_backend import EmuBackend


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('n_rows', [1, 33, 65, 150])
@pytest.mark.parametrize('I', [7, 333, 1500])
@pytest.mark.parametrize('D', [6, 24, 72])
def test_shard_ranks_equal_one_device_ranks(be, D, I, n_rows):
    # D: scalar loads (6), vec4 with the operand in registers (24), more than one staged chunk (72); I: unequal shards, no
    # multiple of the 128-item block, 7 items over 3 shards; n_rows: a 32-row tile, a 64-row tile, more than one row tile
    sc.check_shard_ranks(be, D, I, n_rows)


@pytest.mark.parametrize('D,I', [(6, 7), (24, 333), (72, 1500)])
def test_shard_scores_interleave_to_one_device_rows(be, D, I):
    sc.check_shard_scores(be, D, I)  # 1, 2, 8 rows: the streaming form; 9: the sweep


def test_shard_eval_refusals(be):
    sc.check_shard_eval_refusals(be)
