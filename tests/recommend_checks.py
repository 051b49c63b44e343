"""Shared model-level checks of recommend() (ImplicitFactorizationModel, ImplicitSequenceModel), run through the emulator build
(tests/test_host_recommend.py) and on the gfx950 library (tests/test_gpu_recommend.py).  No training: the tables are filled
with random values (non-zero biases, duplicated item rows: exact ties).  The fused route must equal the model's own generic
route (score rows sorted on the host) and, per user, the lexsort of predict(user)."""
import numpy as np
import torch

from spotlight_amd import _native
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.interactions import Interactions, SequenceInteractions
from spotlight_amd.sequence.implicit import ImplicitSequenceModel
from topk_checks import assert_same, host_topk

K_MAX = _native.TOPK_K_MAX


def fill(model, rs, ties=(3, 9, 22, 40)):
    with torch.no_grad():
        for t in model._net.tables():
            a = rs.randn(*t.shape).astype(np.float32)
            t.copy_(torch.from_numpy(a))
        for t in model._net.tables():  # item-side tables: duplicated rows
            if t.shape[0] == model._num_items:
                for d in ties[1:]:
                    t[d] = t[ties[0]]
    return model


def bilinear_model(U=61, I=147, D=16, seed=11, cls=ImplicitFactorizationModel, **kw):
    rs = np.random.RandomState(seed)
    train = Interactions(rs.randint(0, U, 900).astype(np.int32), rs.randint(0, I, 900).astype(np.int32), num_users=U, num_items=I)
    model = cls(loss='bpr', embedding_dim=D, n_iter=1, batch_size=96, random_state=np.random.RandomState(42), **kw)
    model._initialize(train)
    return fill(model, rs), train


def check_bilinear_recommend():
    model, train = bilinear_model()
    U, I = model._num_users, model._num_items
    users = np.concatenate([np.arange(U), [5, 5, 0]])
    lists = [np.unique(train.tocsr()[u].indices) for u in users]
    for k in (1, 10, K_MAX):
        for exclude, exc in ((None, None), (train, lists), (train.tocsr(), lists), (lists, lists)):
            got = model.recommend(users, k=k, exclude=exclude)
            assert got[0].shape == (len(users), k) and got[0].dtype == np.int64 and got[1].dtype == np.float32
            rec_lists = None if exc is None else [np.asarray(x, dtype=np.int64) for x in exc]
            assert_same(got, model._recommend_generic(users.astype(np.int64), k, rec_lists), ('generic route', k))
            rows = np.stack([model.predict(int(u)) for u in users[:7]])
            assert_same((got[0][:7], got[1][:7]), host_topk(rows, None if exc is None else exc[:7], k), ('predict rows', k))
    # k > K_MAX: the generic route, the same order (k > I: padded)
    k = K_MAX + 40
    got = model.recommend(users[:9], k=k, exclude=train)
    rows = np.stack([model.predict(int(u)) for u in users[:9]])
    assert_same(got, host_topk(rows, lists[:9], k), 'k > K_MAX')
    assert np.all(got[0][:, I:] == -1)
    # a scalar user, no user, bad arguments
    one = model.recommend(5, k=3)
    assert one[0].shape == (1, 3) and np.array_equal(one[0], model.recommend([5], k=3)[0])
    assert model.recommend(np.zeros(0, np.int64), k=4)[0].shape == (0, 4)
    for bad_k in (0, -1, 2.5):
        try:
            model.recommend([1], k=bad_k)
            raise AssertionError('k = %r accepted' % (bad_k,))
        except ValueError:
            pass
    for call, err in ((lambda: model.recommend([U]), ValueError), (lambda: model.recommend([-1]), IndexError),
                      (lambda: model.recommend([1], exclude=[[I]]), IndexError), (lambda: model.recommend([1, 2], exclude=[[1]]), ValueError)):
        try:
            call()
            raise AssertionError('accepted')
        except err:
            pass
    try:
        model.predict(np.array([U]))
    except ValueError as e:
        try:
            model.recommend(np.array([U]))
        except ValueError as e2:
            assert str(e) == str(e2)  # predict()'s check, predict()'s message


def check_poolnet_recommend():
    rs = np.random.RandomState(19)
    I, L, n = 131, 6, 70
    seqs = rs.randint(0, I, (n, L)).astype(np.int64)
    seqs[::5, :2] = 0  # padded sequences
    model = ImplicitSequenceModel(loss='bpr', representation='pooling', embedding_dim=24, n_iter=1, batch_size=32,
                                  random_state=np.random.RandomState(7))
    model._initialize(SequenceInteractions(seqs, num_items=I))
    fill(model, rs)
    for k in (1, 10, K_MAX, K_MAX + 9):
        for preceding in (False, True):
            got = model.recommend(seqs, k=k, exclude_preceding=preceding)
            exc = [np.unique(s) for s in seqs] if preceding else None
            rows = np.stack([model.predict(s) for s in seqs])
            assert_same(got, host_topk(rows, exc, k), ('poolnet predict rows', k, preceding))
            from spotlight_amd import recommend as rec
            generic = rec.generic_topk(lambda s: model._batch_scores(s).cpu().numpy(), seqs, I, k, exc)
            assert_same(got, generic, ('poolnet generic', k, preceding))
            if preceding:
                assert not any(np.intersect1d(got[0][r], seqs[r]).size for r in range(n))
    one = model.recommend(seqs[3], k=5)
    assert one[0].shape == (1, 5) and np.array_equal(one[0][0], model.recommend(seqs, k=5)[0][3])
