"""Shared model-level checks of similar_items() / similar_users() (ImplicitFactorizationModel, ExplicitFactorizationModel,
ImplicitSequenceModel), run through the emulator build (tests/test_host_similar.py) and on the gfx950 library
(tests/test_gpu_similar.py).  No training: the tables are filled with random values (recommend_checks.fill: item rows 3, 9, 22
and 40 are copies: exact ties).  The fused route must equal the generic route (score rows ordered on the host) bit for bit, and
the score values the float64 cosine of the same rows within the bound of tests/neighbors_checks.py."""
import numpy as np
import pytest
import torch

from neighbors_checks import EPS
from recommend_checks import fill
from spotlight_amd import _native
from spotlight_amd.factorization.explicit import ExplicitFactorizationModel
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.factorization.representations import BilinearNet
from spotlight_amd.interactions import Interactions, SequenceInteractions
from spotlight_amd.layers import BloomEmbedding
from spotlight_amd.sequence.implicit import ImplicitSequenceModel
from topk_checks import assert_same

K_MAX = _native.TOPK_K_MAX


def bilinear_model(U=61, I=147, D=16, seed=11, cls=ImplicitFactorizationModel, loss='bpr', **kw):
    """An initialised, untrained model with random tables (as recommend_checks.bilinear_model, for either feedback kind)."""
    rs = np.random.RandomState(seed)
    train = Interactions(rs.randint(0, U, 900).astype(np.int32), rs.randint(0, I, 900).astype(np.int32),
                         ratings=rs.randint(1, 6, 900).astype(np.float32), num_users=U, num_items=I)
    model = cls(loss=loss, embedding_dim=D, n_iter=1, batch_size=96, random_state=np.random.RandomState(42), **kw)
    model._initialize(train)
    return (fill(model, rs) if hasattr(model._net, 'tables') else model), train


def generic(model, attr, num_rows, ids, k, metric, exclude_self, exclude, always=None):
    """The model's generic route: slk_neighbors_scores rows a tile at a time, ordered on the host."""
    return ImplicitFactorizationModel._similar(model, attr, num_rows, ids, k, metric, exclude_self, exclude, always=always, generic=True)


def cosine64(table, ids):
    t = table.astype(np.float64)
    norm = np.sqrt((t ** 2).sum(axis=1))
    return (t[ids] @ t.T) / np.outer(norm[ids], norm)


def check_side(model, call, attr, num_rows, ids, always=None):
    """One table of a model: fused == generic for k <= K_MAX; k = K_MAX == the first K_MAX columns of k = K_MAX + 72; values."""
    rs = np.random.RandomState(3)
    lists = [rs.randint(0, num_rows, rs.randint(0, 12)).astype(np.int64) for _ in ids]
    for metric in ('cosine', 'dot'):
        for k in (1, 10, K_MAX):
            for exclude_self, exclude in ((True, None), (False, None), (True, lists), (False, lists)):
                got = call(ids, k=k, metric=metric, exclude_self=exclude_self, exclude=exclude)
                assert got[0].shape == (len(ids), k) and got[0].dtype == np.int64 and got[1].dtype == np.float32
                assert_same(got, generic(model, attr, num_rows, ids, k, metric, exclude_self, exclude, always),
                            (attr, metric, k, exclude_self, exclude is not None))
                if exclude_self:
                    assert not np.any(got[0] == np.asarray(ids)[:, None])
                if exclude is not None:
                    assert not any(np.intersect1d(got[0][r], lists[r]).size for r in range(len(ids)))
                if always is not None:
                    assert not np.any(np.isin(got[0], always))
        big = call(ids, k=K_MAX + 72, metric=metric, exclude=lists)
        assert_same(call(ids, k=K_MAX, metric=metric, exclude=lists), (big[0][:, :K_MAX].copy(), big[1][:, :K_MAX].copy()), (attr, metric, 'k = 200'))
        if K_MAX + 72 > num_rows:
            assert np.all(big[0][:, num_rows:] == -1) and np.all(np.isneginf(big[1][:, num_rows:]))
    # the values: the float64 cosine of the table's own rows
    table = model._embedding_table(attr, num_rows).detach().cpu().numpy()
    D = table.shape[1]
    live = np.asarray([i for i in ids if np.any(table[i] != 0)], dtype=np.int64)
    got = call(live, k=10, metric='cosine', exclude_self=False)
    want = cosine64(table, live)
    ok = got[0] >= 0
    err = np.abs(got[1].astype(np.float64) - np.take_along_axis(want, np.where(ok, got[0], 0), axis=1))[ok]
    assert err.max() <= (2 * D + 16) * EPS, (attr, err.max())
    if always is None:  # a row is its own nearest neighbour (or ties with its copies: the smaller id first)
        assert np.all(np.take_along_axis(want, got[0][:, :1], axis=1)[:, 0] >= 1 - (2 * D + 16) * EPS)


def check_arguments(model, call, num_rows):
    one = call(5, k=3)
    assert one[0].shape == (1, 3) and np.array_equal(one[0], call([5], k=3)[0])
    empty = call(np.zeros(0, np.int64), k=4)
    assert empty[0].shape == (0, 4) and empty[0].dtype == np.int64 and empty[1].shape == (0, 4) and empty[1].dtype == np.float32
    for bad_k in (0, -1, 2.5):
        with pytest.raises(ValueError):
            call([1], k=bad_k)
    with pytest.raises(ValueError, match='metric'):
        call([1], metric='euclid')
    with pytest.raises(ValueError, match='Maximum'):
        call([num_rows])
    with pytest.raises(IndexError):
        call([-1])
    with pytest.raises(IndexError):
        call([1], exclude=[[num_rows]])
    with pytest.raises(ValueError):
        call([1, 2], exclude=[[1]])


def check_factorization(cls=ImplicitFactorizationModel, **kw):
    model, _ = bilinear_model(cls=cls, **kw)
    U, I = model._num_users, model._num_items
    items = np.concatenate([np.arange(I), [5, 5, 0]]).astype(np.int64)
    users = np.concatenate([np.arange(U), [7, 7]]).astype(np.int64)
    check_side(model, model.similar_items, 'item_embeddings', I, items)
    check_side(model, model.similar_users, 'user_embeddings', U, users)
    check_arguments(model, model.similar_items, I)
    check_arguments(model, model.similar_users, U)
    # recommend()'s messages for recommend()'s mistakes
    for bad, call in ((np.array([U]), model.similar_users), (np.array([-1]), model.similar_users)):
        with pytest.raises((ValueError, IndexError)) as e1:
            model.recommend(bad)
        with pytest.raises(type(e1.value)) as e2:
            call(bad)
        assert str(e1.value) == str(e2.value)
    return model


def check_ties_in_the_model():
    """Item rows 3, 9, 22 and 40 are copies (recommend_checks.fill): queried with one of them they come first, in ascending id,
    the query itself left out."""
    model, _ = bilinear_model()
    got = model.similar_items([9, 3], k=2)
    assert np.array_equal(got[0], [[3, 22], [9, 22]]) and np.all(np.abs(got[1] - 1) <= (2 * 16 + 16) * EPS)
    got = model.similar_items([9], k=4, exclude_self=False)
    assert np.array_equal(got[0][0], [3, 9, 22, 40]) and len(set(got[1][0].view(np.uint32).tolist())) == 1


def check_bloom_item_table():
    """A BloomEmbedding item table (the representation of id j: the sum of its hashed rows, materialised once per call) beside a
    plain user table."""
    U, I, D = 61, 147, 16
    net = BilinearNet(U, I, D, item_embedding_layer=BloomEmbedding(I, D, compression_ratio=0.4, num_hash_functions=4))
    model = check_factorization(representation=net)
    table = model._embedding_table('item_embeddings', I)
    assert tuple(table.shape) == (I, D) and tuple(model._net.item_embeddings.weight.shape) == (int(0.4 * I), D)
    ids = torch.arange(I, dtype=torch.int64, device=table.device)
    with torch.no_grad():
        assert torch.equal(table, model._net.item_embeddings(ids).reshape(I, D))


class _NoTables(torch.nn.Module):
    def __init__(self, U, I, D):
        super(_NoTables, self).__init__()
        self.users, self.items = torch.nn.Embedding(U, D), torch.nn.Embedding(I, D)

    def forward(self, user_ids, item_ids):
        return (self.users(user_ids) * self.items(item_ids)).sum(1)


def check_custom_representation():
    model, _ = bilinear_model(representation=_NoTables(61, 147, 16))
    with pytest.raises(TypeError, match='item_embeddings'):
        model.similar_items([1])
    with pytest.raises(TypeError, match='user_embeddings'):
        model.similar_users([1])


def check_sequence_model():
    rs = np.random.RandomState(19)
    I, L, n = 131, 6, 70
    seqs = rs.randint(0, I, (n, L)).astype(np.int64)
    model = ImplicitSequenceModel(loss='bpr', representation='pooling', embedding_dim=24, n_iter=1, batch_size=32,
                                  random_state=np.random.RandomState(7))
    model._initialize(SequenceInteractions(seqs, num_items=I))
    fill(model, rs)
    ids = np.concatenate([np.arange(I), [5, 5]]).astype(np.int64)  # (the padding item may be asked about; it is never an answer)
    check_side(model, model.similar_items, 'item_embeddings', I, ids, always=[0])
    check_arguments(model, model.similar_items, I)
    got = model.similar_items(ids, k=K_MAX + 9, exclude_self=False)  # more than the table holds: 130 answers, then padding
    assert np.all(np.sort(got[0][:, :I - 1], axis=1) == np.arange(1, I)) and np.all(got[0][:, I - 1:] == -1)


def check_refused_inside_a_fit_scope(engine, stream):
    """Inside the user-row ping-pong scope fit() opens for large minibatches the user tensor is a mix of rows: similar_users() is
    refused as predict() is; the item table is whole."""
    model, _ = bilinear_model(optimizer_func=lambda p: torch.optim.Adagrad(list(p), lr=0.05))
    before = model.similar_users([3, 4], k=5)
    with engine.user_pingpong(model._slk_tables(), model._bind().as_struct(), stream=stream):
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            model.predict(3)
        for metric in ('cosine', 'dot'):
            with pytest.raises(_native.SlkError, match='ping-ponged'):
                model.similar_users([3, 4], k=5, metric=metric)
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            model.similar_users([3, 4], k=K_MAX + 1)
        model.similar_items([3, 4], k=5)
    assert_same(model.similar_users([3, 4], k=5), before, 'after the scope')
