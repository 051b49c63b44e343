"""TEST HARNESS: one rank of the sharded recommend() check (tests/test_host_recommend.py, tests/test_gpu_recommend.py).

As tests/shard_eval_worker.py: no training, every rank builds the same full random tables from one numpy seed (duplicated item
rows: exact ties that live on different shards) and copies rows rank::world into a ShardedImplicitFactorizationModel; rank 0
also loads the full tables into a one-device ImplicitFactorizationModel.  recommend() of the sharded model must return the
one-device model's arrays on every rank, and only user rows may travel.
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

    U, I, D = 61, 47, 16
    rs = np.random.RandomState(11)
    full = [rs.randn(U, D).astype(np.float32), rs.randn(I, D).astype(np.float32),
            rs.randn(U, 1).astype(np.float32), rs.randn(I, 1).astype(np.float32)]
    for dup in (9, 22, 40):  # three copies of item 3, on different shards at world 2 and 3
        full[1][dup] = full[1][3]
        full[3][dup] = full[3][3]
    train = Interactions(rs.randint(0, U, 400).astype(np.int32), rs.randint(0, I, 400).astype(np.int32), num_users=U, num_items=I)
    users = np.concatenate([np.arange(U), [7, 7]]).astype(np.int64)

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

    def counting_fetch(t_emb, t_bias, ids, device):
        fetched.append((t_emb, len(ids)))
        return fetch_rows(t_emb, t_bias, ids, device)
    model._fetch_rows = counting_fetch

    cases = [(1, None), (10, None), (10, train), (_native.TOPK_K_MAX, train), (5, train)]  # K_MAX > I: padded
    got = []
    for k, exclude in cases:
        del fetched[:]
        got.append(model.recommend(users, k=k, exclude=exclude))
        assert fetched == [(0, len(users))], fetched  # user rows only

    # every rank holds the same arrays
    device = model._net.tables()[0].device
    for items, scores in got:
        mine = torch.from_numpy(np.concatenate([items.ravel().astype(np.float64), scores.ravel().astype(np.float64)]))
        gathered = [torch.empty_like(mine).to(device) for _ in range(world)]
        dist.all_gather(gathered, mine.to(device))
        for g in gathered:
            assert torch.equal(g.cpu(), mine)

    if rank == 0:
        ref = load(ImplicitFactorizationModel(random_state=np.random.RandomState(42), **kw), slice(None))
        for (k, exclude), g in zip(cases, got):
            assert_same(g, ref.recommend(users, k=k, exclude=exclude), ('sharded', world, k, exclude is not None))
        print('SHARD_TOPK_OK world=%d backend=%s' % (world, backend))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
