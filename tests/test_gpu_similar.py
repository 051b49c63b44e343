"""similar_items() / similar_users() of the models on the gfx950 library (the checks of tests/test_host_similar.py), the
row-sharded model at world 1 (RCCL) and 2 (gloo), and the memory a large call takes."""
import os

import numpy as np
import pytest
import torch

import similar_checks as sc
from test_sharded import run_world

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'shard_neighbors_worker.py')


def test_implicit_model():
    sc.check_factorization()


def test_explicit_model():
    sc.check_factorization(cls=sc.ExplicitFactorizationModel, loss='regression')


def test_ties_in_the_model():
    sc.check_ties_in_the_model()


def test_bloom_item_table():
    sc.check_bloom_item_table()


def test_custom_representation_is_refused():
    sc.check_custom_representation()


def test_sequence_model_never_returns_the_padding_item():
    sc.check_sequence_model()


def test_refused_inside_a_fit_scope():
    from spotlight_amd.factorization import implicit as host
    device = torch.device('cuda', torch.cuda.current_device())
    sc.check_refused_inside_a_fit_scope(host._engine_for(device), host._stream_for(device))


def test_sharded_similar_items_world1_nccl():
    run_world(1, [], backend='hip', worker=WORKER, token='SHARD_NEIGHBORS_OK', timeout=240)


def test_sharded_similar_items_world2_gloo():
    run_world(2, [], backend='hipgloo', worker=WORKER, token='SHARD_NEIGHBORS_OK', timeout=240)


def test_similar_items_allocates_no_score_tile():
    """4096 queries x 10^6 items x dim 64, k = 10, cosine: the torch allocator's peak grows by the call's own arrays only -- the
    ids (8 B per query), the gathered query rows (n * dim * 4), the table's inverse-norm vector (I * 4), the per-row exclusion CSR
    (n + 1 offsets, one self entry per query), the two outputs (12 B per query and k) -- each rounded up to the allocator's 512-B
    granule, times two for the host copies' staging: 11.3 MB, 8 MB of it the inverse-norm vector's term, 2 MB the query rows'.
    One score tile of the generic route would be 256 MB, the score matrix 16 GB.  (The candidate scratch is the ctx's, outside
    the torch allocator and bounded by 64 MB: include/spotlight_hip.h.)"""
    U, I, D, n, k = 64, 1000000, 64, 4096, 10
    model, _ = sc.bilinear_model(U=U, I=I, D=D)
    ids = np.arange(n) * 7
    model.similar_items(ids[:64], k=k)  # first use: the engine, the library's scratch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    items, scores = model.similar_items(ids, k=k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    granule = lambda b: (b + 511) // 512 * 512
    bound = 2 * (granule(8 * n) + granule(4 * n * D) + granule(4 * I) + granule(8 * (n + 1)) + granule(8 * n)
                 + granule(8 * n * k) + granule(4 * n * k))
    print('similar_items peak growth %d B, bound %d B' % (grown, bound))
    assert grown <= bound, (grown, bound)
    assert bound < (256 << 20) // 20  # a twentieth of ONE score tile
    assert items.shape == (n, k) and np.all(items >= 0) and np.all(np.diff(scores, axis=1) <= 0) and not np.any(items == ids[:, None])
