"""recommend() of the models on the gfx950 library (the checks of tests/test_host_recommend.py), the row-sharded model at world
1, and the memory a large call takes."""
import os

import numpy as np
import pytest
import torch

import recommend_checks as rc
from test_sharded import run_world

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOPK_WORKER = os.path.join(HERE, 'shard_topk_worker.py')


def test_bilinear_recommend():
    rc.check_bilinear_recommend()


def test_poolnet_recommend():
    rc.check_poolnet_recommend()


def test_sharded_recommend_world1_nccl():
    run_world(1, [], backend='hip', worker=TOPK_WORKER, token='SHARD_TOPK_OK', timeout=240)


def test_recommend_allocates_no_score_tile():
    """4096 users x 10^6 items: the torch allocator's peak grows by the call's own arrays only -- the ids (8 B per user), the two
    outputs (12 B per user and k) -- each rounded up to the allocator's 512-B granule, times two for the host copies' staging;
    one score tile of evaluation.py would be 256 MB, the score matrix 16 GB.  (The candidate scratch is the ctx's, outside the
    torch allocator and bounded by 64 MB: include/spotlight_hip.h.)"""
    U, I, D, n, k = 4096, 1000000, 64, 4096, 10
    model, _ = rc.bilinear_model(U=U, I=I, D=D)
    users = np.arange(n)
    model.recommend(users[:64], k=k)  # first use: the engine, the library's scratch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    items, scores = model.recommend(users, k=k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    granule = lambda b: (b + 511) // 512 * 512
    bound = 2 * (granule(8 * n) + granule(8 * n * k) + granule(4 * n * k))
    assert grown <= bound, (grown, bound)
    assert bound < (256 << 20) // 100
    assert items.shape == (n, k) and np.all(items >= 0) and np.all(np.diff(scores, axis=1) <= 0)
