"""TEST HARNESS: one rank of the sharded-evaluation check (tests/test_sharded_eval.py).

No training: every rank builds the same full random tables from one numpy seed (non-zero biases, three duplicated item rows:
exact ties that live on different shards) and copies rows rank::world into an initialised
ShardedImplicitFactorizationModel; rank 0 also loads the full tables into a one-device ImplicitFactorizationModel.
mrr_score, precision_recall_score and predict(user) of the sharded model must equal the one-device model's bit for bit, on
every rank alike, and no _fetch_rows call may fetch more ids than the call has users (only user rows travel).
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
from spotlight_amd.evaluation import mrr_score, precision_recall_score  # noqa: E402
from spotlight_amd.factorization import implicit as host  # noqa: E402
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel  # noqa: E402
from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel, local_rows  # noqa: E402
from spotlight_amd.interactions import Interactions  # noqa: E402


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
    test_u = np.concatenate([rs.randint(0, 30, 80), np.arange(4)]).astype(np.int32)
    test_i = np.concatenate([rs.randint(0, I, 80), [3, 9, 22, 40]]).astype(np.int32)  # held-out items among the ties too
    test = Interactions(test_u, test_i, num_users=U, num_items=I)
    n_test_users = len(np.unique(test_u))

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

    mrr = mrr_score(model, test, train=train)
    assert fetched and all(t == 0 and n <= n_test_users for t, n in fetched), fetched  # user rows only, a row per test user
    del fetched[:]
    prec, rec = precision_recall_score(model, test, train=train, k=[1, 5])
    assert fetched and all(t == 0 and n <= n_test_users for t, n in fetched), fetched
    del fetched[:]
    pred = model.predict(5)
    assert fetched == [(0, 1)], fetched

    # every rank holds the same arrays
    mine = torch.from_numpy(np.concatenate([mrr.ravel(), prec.ravel(), rec.ravel(), pred.astype(np.float64)]))
    device = model._net.tables()[0].device
    gathered = [torch.empty_like(mine).to(device) for _ in range(world)]
    dist.all_gather(gathered, mine.to(device))
    for g in gathered:
        assert torch.equal(g.cpu(), mine)

    if rank == 0:
        ref = load(ImplicitFactorizationModel(random_state=np.random.RandomState(42), **kw), slice(None))
        want_mrr = mrr_score(ref, test, train=train)
        want_prec, want_rec = precision_recall_score(ref, test, train=train, k=[1, 5])
        want_pred = ref.predict(5)
        assert mrr.shape == (n_test_users,) and np.array_equal(mrr, want_mrr), (mrr, want_mrr)
        assert np.array_equal(prec, want_prec) and np.array_equal(rec, want_rec)
        assert pred.dtype == np.float32 and pred.shape == (I,) and np.array_equal(pred, want_pred)
        # (the one-device fast path is itself the per-user reference route: tests/test_host_model.py)
        print('SHARD_EVAL_OK world=%d backend=%s' % (world, backend))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
