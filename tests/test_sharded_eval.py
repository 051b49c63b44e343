"""Ranking metrics and predict(user) of the row-sharded model, shard by shard (spotlight_amd/factorization/sharded.py:
_fused_ranks, _batch_scores, predict): `world` processes run tests/shard_eval_worker.py, rank 0 compares with the
one-device model -- bit for bit -- and every rank checks that only user rows travel."""
import os

import pytest

from test_sharded import run_world

HERE = os.path.dirname(os.path.abspath(__file__))
EVAL_WORKER = os.path.join(HERE, 'shard_eval_worker.py')


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_eval_matches_single_device_model(world):
    run_world(world, [], worker=EVAL_WORKER, token='SHARD_EVAL_OK', timeout=240)


@pytest.mark.gpu
def test_gpu_sharded_eval_remote_peers_on_one_gpu_over_gloo():
    run_world(2, [], backend='hipgloo', worker=EVAL_WORKER, token='SHARD_EVAL_OK', timeout=240)


@pytest.mark.gpu
def test_gpu_sharded_eval_world1_nccl():
    run_world(1, [], backend='hip', worker=EVAL_WORKER, token='SHARD_EVAL_OK', timeout=240)
