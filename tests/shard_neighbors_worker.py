"""TEST HARNESS: one rank of the sharded similar_items() check (tests/test_host_similar.py, tests/test_gpu_similar.py).

As tests/shard_topk_worker.py: no training, every rank builds the same full random tables from one numpy seed (duplicated item
rows: exact ties that live on different shards, one all-zero row) and copies rows rank::world into a
ShardedImplicitFactorizationModel; rank 0 also loads the full tables into a one-device ImplicitFactorizationModel.
similar_items() of the sharded model must return the one-device model's arrays on every rank, and only the query rows may travel.
argv[2] (optional): the number of items -- 2 puts fewer items than ranks on a world of 3.
Backend 'emu' (gloo + emulator), 'hipgloo' (the gfx950 library, every rank on GPU 0, gloo) or 'hip' (nccl)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from spotlight_amd import _native  # noqa: E402
from spotlight_amd.factorization import implicit as host  # noqa: E402
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel  # noqa: E402
from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel, local_rows  # noqa: E402
from spotlight_amd.interactions import Interactions  # noqa: E402
from topk_checks import assert_same  # noqa: E402


def main():
    backend = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    if backend == 'emu':
        from emu_backend import emu_lib
        dist.init_process_group('gloo')
        eng = _native.Engine(0, lib=emu_lib())
        host._engine_for = lambda device: eng
        host._stream_for = lambda device: 0
        host._model_device = lambda: torch.device('cpu')
    elif backend == 'hipgloo':
        torch.cuda.set_device(0)
        dist.init_process_group('gloo')
    else:
        torch.cuda.set_device(rank)
        dist.init_process_group('nccl', device_id=torch.device('cuda', rank))

    U, D = 61, 16
    I = int(sys.argv[2]) if len(sys.argv) > 2 else 47
    rs = np.random.RandomState(11)
    full = [rs.randn(U, D).astype(np.float32), rs.randn(I, D).astype(np.float32),
            rs.randn(U, 1).astype(np.float32), rs.randn(I, 1).astype(np.float32)]
    if I > 40:
        for dup in (9, 22, 40):  # three copies of item 3, on different shards at world 2 and 3
            full[1][dup] = full[1][3]
        full[1][13] = 0.0
    train = Interactions(rs.randint(0, U, 400).astype(np.int32), rs.randint(0, I, 400).astype(np.int32), num_users=U, num_items=I)
    ids = np.concatenate([np.arange(I), [3 % I, 3 % I, 0]]).astype(np.int64)
    lists = [rs.randint(0, I, rs.randint(0, 9)).astype(np.int64) for _ in ids]

    def load(model, rows):
        model._initialize(train)
        with torch.no_grad():
            for loc, whole in zip(model._net.tables(), full):
                assert tuple(loc.shape) == tuple(whole[rows].shape)
                loc.copy_(torch.from_numpy(np.ascontiguousarray(whole[rows])))
        return model

    kw = dict(loss='bpr', embedding_dim=D, n_iter=1, batch_size=96)
    model = load(ShardedImplicitFactorizationModel(random_state=np.random.RandomState(42), **kw), slice(rank, None, world))
    assert model._net.tables()[1].shape[0] == local_rows(I, world, rank)

    fetched = []
    fetch_rows = model._fetch_rows

    def counting_fetch(t_emb, t_bias, ids_, device):
        fetched.append((t_emb, len(ids_)))
        return fetch_rows(t_emb, t_bias, ids_, device)
    model._fetch_rows = counting_fetch

    K = _native.TOPK_K_MAX
    cases = [dict(k=1), dict(k=10), dict(k=10, metric='dot'), dict(k=10, exclude_self=False), dict(k=10, exclude=lists),
             dict(k=5, metric='dot', exclude_self=False, exclude=lists), dict(k=K, exclude=lists), dict(k=K + 30, metric='dot')]
    got = []
    for case in cases:
        del fetched[:]
        got.append(model.similar_items(ids, **case))
        assert fetched == [(1, len(ids))], fetched  # the query rows only
    assert model.similar_items(np.zeros(0, np.int64), k=3)[0].shape == (0, 3)
    try:
        model.similar_users([1])
        raise AssertionError('similar_users() of the sharded model answered')
    except NotImplementedError:
        pass

    # every rank holds the same arrays
    device = model._net.tables()[0].device
    for items, scores in got:
        mine = torch.from_numpy(np.concatenate([items.ravel().astype(np.float64), scores.view(np.uint32).ravel().astype(np.float64)]))
        gathered = [torch.empty_like(mine).to(device) for _ in range(world)]
        dist.all_gather(gathered, mine.to(device))
        for g in gathered:
            assert torch.equal(g.cpu(), mine)

    if rank == 0:
        ref = load(ImplicitFactorizationModel(random_state=np.random.RandomState(42), **kw), slice(None))
        for case, g in zip(cases, got):
            assert_same(g, ref.similar_items(ids, **case), ('sharded', world, I, sorted(case)))
        print('SHARD_NEIGHBORS_OK world=%d backend=%s items=%d' % (world, backend, I))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
