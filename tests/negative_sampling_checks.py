"""Shared checks of the models' `negative_sampling` keyword (popularity-weighted negatives: spotlight_amd/sampling.py,
ItemDistribution).  They run through the emulator build of the kernels in tests/test_host_negative_sampling.py (which points the
three device hooks of factorization/implicit.py at it) and on the gfx950 library in tests/test_gpu_negative_sampling.py.

Every comparison is bit for bit: a weighted draw is RandomState.choice(num_items, size=..., p=p) on the model's RandomState, and
the replays below make exactly those calls on a host copy of it, in the reference's order (shuffle, then one draw per minibatch)."""
import io

import numpy as np
import pytest
import torch

from spotlight_amd import _native
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.interactions import Interactions, SequenceInteractions
from spotlight_amd.sampling import ItemDistribution, sample_items, sample_items_device
from spotlight_amd.sequence import implicit as seq_host
from spotlight_amd.sequence.implicit import ImplicitSequenceModel
from spotlight_amd.torch_utils import shuffle

U, I, N, B, EPOCHS, NN = 40, 30, 300, 64, 3, 3
ABSENT = (3, 17, 29)  # items of the catalogue that no interaction names


def _adagrad(params):
    return torch.optim.Adagrad(params, lr=0.05)


def _rmsprop(params):
    return torch.optim.RMSprop(params, lr=0.01)


def dataset(seed=0):
    """40 users, 30 items, 300 interactions; the items of ABSENT never occur."""
    rs = np.random.RandomState(seed)
    present = np.setdiff1d(np.arange(I), ABSENT)
    items = present[rs.zipf(1.5, N) % present.size]
    return Interactions(rs.randint(0, U, N).astype(np.int32), items.astype(np.int32), num_users=U, num_items=I)


def popularity_p(item_ids, num_items, power=0.75, zero=()):
    w = np.bincount(item_ids.reshape(-1), minlength=num_items).astype(np.float64)
    for item in zero:
        w[item] = 0.0
    w = w ** power
    return w / w.sum()


def model_for(loss, seed, **kw):
    kw.setdefault('optimizer_func', _adagrad)
    return ImplicitFactorizationModel(loss=loss, embedding_dim=16, n_iter=EPOCHS, batch_size=B, num_negative_samples=NN,
                                      random_state=np.random.RandomState(seed), **kw)


def tables_of(model):
    return [t.detach().cpu().numpy().copy() for t in model._net.tables()]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_state(a, b):
    a, b = a.get_state(), b.get_state()
    return (a[1] == b[1]).all() and a[2] == b[2]


def assert_same_fit(a, b, what):
    for t, (x, y) in enumerate(zip(tables_of(a), tables_of(b))):
        assert same_bits(x, y), (what, 'table', t)
    assert same_state(a._random_state, b._random_state), (what, 'RandomState')


class Recorded(object):
    """Copies of the negatives every training call of a fit() was handed (the epoch's hand-in buffer, read when the call is
    enqueued)."""

    def __init__(self, monkeypatch, cls, buffer_of):
        self.epochs = []
        inner = cls.train

        def train(job, engine, stream, epoch_num):
            self.epochs.append(buffer_of(job, epoch_num).detach().cpu().numpy().copy())
            return inner(job, engine, stream, epoch_num)
        monkeypatch.setattr(cls, 'train', train)


# ---- 1. the hand-in is exact -------------------------------------------------------------------------------------------------------
def check_hand_in_is_exact(loss, seed=21):
    inter = dataset()
    nn = NN if loss == 'adaptive_hinge' else 1
    model = model_for(loss, seed, negative_sampling='popularity')
    model.fit(inter)

    # the stream, replayed on the host: the constructor's draw, then per epoch the reference's shuffle and one choice() per
    # minibatch in the reference's minibatch order
    p = popularity_p(inter.item_ids, I)
    rs = np.random.RandomState(seed)
    rs.randint(-10**8, 10**8)
    epochs = []
    for _ in range(EPOCHS):
        users, items = shuffle(inter.user_ids, inter.item_ids, random_state=rs)
        negs = [rs.choice(I, size=len(users[lo:lo + B]) * nn, p=p) for lo in range(0, N, B)]
        epochs.append((users.astype(np.int64), items.astype(np.int64), np.concatenate(negs).astype(np.int64)))

    # a twin of the model (same seed: bit-identical initial tables) trained by slk_bilinear_train with those negatives handed in
    twin = model_for(loss, seed, negative_sampling='popularity')
    twin._initialize(inter)
    fresh = model_for(loss, seed, negative_sampling='popularity')
    fresh._initialize(inter)
    for x, y in zip(tables_of(twin), tables_of(fresh)):
        assert same_bits(x, y)
    binding = twin._bind()
    device = twin._net.tables()[0].device
    engine, stream = host._engine_for(device), host._stream_for(device)
    mb_loss = torch.empty((N + B - 1) // B, dtype=torch.float32, device=device)
    with host.fit_scope(twin):
        for users, items, negs in epochs:
            d_u, d_i, d_n = [torch.from_numpy(a).to(device) for a in (users, items, negs)]
            ostruct = binding.as_struct()
            engine.bilinear_train(twin._slk_tables(), ostruct, d_u.data_ptr(), d_i.data_ptr(), N, B, loss, NN, mb_loss.data_ptr(),
                                  d_neg_in=d_n.data_ptr(), stream=stream)
            binding.store_steps(ostruct.step)
            engine.check()
    for t, (x, y) in enumerate(zip(tables_of(model), tables_of(twin))):
        assert same_bits(x, y), (loss, 'table', t)
        assert not same_bits(x, tables_of(fresh)[t]) or t == 2  # (training moved the table; bpr leaves the user biases at zero)
    assert same_state(model._random_state, rs)


# ---- 2. no behaviour change ----------------------------------------------------------------------------------------------------------
def check_uniform_is_untouched(loss='bpr', seed=5):
    inter = dataset()
    base = model_for(loss, seed)
    base.fit(inter)
    for value in ('uniform', None):
        other = model_for(loss, seed, negative_sampling=value)
        other.fit(inter)
        assert other._item_distribution is None
        assert_same_fit(base, other, value)


# ---- 3. the same path above the two-lane threshold -----------------------------------------------------------------------------------
def check_large_epochs_take_the_hand_in_schedule(monkeypatch, loss='bpr', seed=9):
    inter = dataset()
    calls = []
    inner = _native.Engine.bilinear_prefetch

    def counted(self, *a, **kw):
        calls.append(1)
        return inner(self, *a, **kw)
    monkeypatch.setattr(_native.Engine, 'bilinear_prefetch', counted)
    small = model_for(loss, seed, negative_sampling='popularity')
    small.fit(inter)
    assert not calls
    monkeypatch.setattr(host, '_PIPELINE_MAX_DRAWS', 128)  # 300 draws per epoch now count as a large epoch
    large = model_for(loss, seed, negative_sampling='popularity')
    large.fit(inter)
    assert not calls, 'slk_bilinear_prefetch draws uniform negatives: a weighted fit() must never reach it'
    assert_same_fit(small, large, 'above the threshold')
    uniform = model_for(loss, seed)  # (the wrapper does see the pipeline's calls: a uniform fit() of this size prefetches)
    uniform.fit(inter)
    assert calls


# ---- 4. popularity weights -----------------------------------------------------------------------------------------------------------
def check_popularity_weights(monkeypatch, loss='adaptive_hinge', seed=13):
    inter = dataset()
    rec = Recorded(monkeypatch, host._ImplicitEpochs, lambda job, e: job.slots[e % len(job.slots)][2])
    model = model_for(loss, seed, negative_sampling='popularity')
    model.fit(inter)
    dist = model._item_distribution
    assert isinstance(dist, ItemDistribution) and same_bits(dist.p, popularity_p(inter.item_ids, I))
    assert len(rec.epochs) == EPOCHS
    drawn = np.concatenate(rec.epochs)
    assert drawn.size == EPOCHS * N * NN and drawn.min() >= 0 and drawn.max() < I
    assert not np.isin(drawn, ABSENT).any(), 'an item absent from training was drawn as a negative'
    # another power, and weights given as an array
    half = model_for(loss, seed, negative_sampling='popularity', negative_sampling_power=0.5)
    half.fit(inter)
    assert same_bits(half._item_distribution.p, popularity_p(inter.item_ids, I, power=0.5))
    w = np.arange(I, dtype=np.float32)  # item 0 has weight 0
    given = model_for(loss, seed, negative_sampling=w)
    del rec.epochs[:]
    given.fit(inter)
    assert same_bits(given._item_distribution.p, w.astype(np.float64) / w.astype(np.float64).sum())
    assert (np.concatenate(rec.epochs) != 0).all()


# ---- 5. sequence model ---------------------------------------------------------------------------------------------------------------
def sequences(seed=2, n_seq=40, seq_len=6, num_items=30):
    rs = np.random.RandomState(seed)
    seqs = rs.randint(1, num_items - 2, (n_seq, seq_len)).astype(np.int32)  # (the last two items never occur)
    seqs[rs.rand(n_seq, seq_len) < np.linspace(0.6, 0.0, seq_len)] = 0  # left-heavy padding
    return SequenceInteractions(seqs, num_items=num_items)


def check_sequence_model(monkeypatch, loss, seed=31, representation='pooling'):
    inter = sequences()
    seqs = inter.sequences
    n_seq, seq_len = seqs.shape
    batch, n_iter = 16, 2
    nn = NN if loss == 'adaptive_hinge' else 1
    rec = Recorded(monkeypatch, seq_host._SequenceEpochs, lambda job, e: job.negs[e % 2])
    model = ImplicitSequenceModel(loss=loss, representation=representation, embedding_dim=8, n_iter=n_iter, batch_size=batch,
                                  optimizer_func=_adagrad, num_negative_samples=NN, negative_sampling='popularity',
                                  random_state=np.random.RandomState(seed))
    model.fit(inter)
    p = popularity_p(seqs, I, zero=(0,))
    assert same_bits(model._item_distribution.p, p) and p[0] == 0.0
    rs = np.random.RandomState(seed)
    rs.randint(-10**8, 10**8)
    first = None
    cur = seqs
    for _ in range(n_iter):
        cur = shuffle(cur, random_state=rs)  # (the reference rebinds `sequences`: the shuffles compose)
        for lo in range(0, n_seq, batch):
            rows = len(cur[lo:lo + batch])
            block = rs.choice(I, size=(nn * rows, seq_len), p=p)  # sequence/implicit.py: one draw per minibatch
            first = block if first is None else first
    assert same_state(model._random_state, rs)
    if representation == 'pooling':
        assert len(rec.epochs) == n_iter
        assert np.array_equal(rec.epochs[0][:first.size], first.reshape(-1))
        assert all((e != 0).all() for e in rec.epochs), 'the padding item was drawn as a negative'
    return model


# ---- 6. fold_in ----------------------------------------------------------------------------------------------------------------------
def check_fold_in(loss, seed=17):
    inter = dataset()
    model = model_for(loss, seed, negative_sampling='popularity')
    model.fit(inter)
    p = popularity_p(inter.item_ids, I)
    rs = np.random.RandomState(3)
    lengths = (0, 1, 5, 37, 2)
    users = np.repeat(np.arange(len(lengths)), lengths)
    new = Interactions(users.astype(np.int32), rs.randint(0, I, users.size).astype(np.int32), num_users=len(lengths), num_items=I)
    n, H, T = users.size, len(lengths), 3
    nn = NN if loss == 'adaptive_hinge' else 1
    init = (np.full((H, 16), 0.05, np.float32), np.zeros(H, np.float32))
    copy = np.random.RandomState()
    copy.set_state(model._random_state.get_state())
    drawn = model.fold_in(new, n_iter=T, init=init)
    want_neg = np.stack([copy.choice(I, size=(nn, n), p=p) for _ in range(T)])
    assert same_state(model._random_state, copy)
    given = model.fold_in(new, n_iter=T, init=init, negatives=want_neg)
    assert same_bits(drawn[0], given[0]) and same_bits(drawn[1], given[1])
    assert same_state(model._random_state, copy)  # negatives given: the stream is left alone
    assert not same_bits(drawn[0], init[0])


# ---- 7. autograd route ---------------------------------------------------------------------------------------------------------------
def check_autograd_route(loss, seed=19):
    inter = dataset()
    fused = model_for(loss, seed, negative_sampling='popularity')
    fused.fit(inter)
    auto = model_for(loss, seed, negative_sampling='popularity', optimizer_func=_rmsprop)
    auto.fit(inter)
    assert auto._autograd_route and not fused._autograd_route
    assert same_state(fused._random_state, auto._random_state)
    plain = model_for(loss, seed, optimizer_func=_rmsprop)  # (and the keyword does change what the route draws)
    plain.fit(inter)
    assert not same_state(plain._random_state, auto._random_state)


# ---- 8. validation -------------------------------------------------------------------------------------------------------------------
BAD_WEIGHTS = {'wrong length': np.ones(I + 1), 'negative': np.where(np.arange(I) == 4, -1.0, 1.0),
               'nan': np.where(np.arange(I) == 4, np.nan, 1.0), 'all zero': np.zeros(I)}


def check_validation_errors(which):
    w = BAD_WEIGHTS[which]
    inter = dataset()
    model = model_for('bpr', 3, negative_sampling=w)
    before = np.random.RandomState()
    before.set_state(model._random_state.get_state())
    with pytest.raises(ValueError, match='negative_sampling weights'):
        model.fit(inter)
    assert same_state(model._random_state, before)
    seq = ImplicitSequenceModel(loss='bpr', embedding_dim=8, n_iter=1, batch_size=16, negative_sampling=w,
                                random_state=np.random.RandomState(3))
    before.set_state(seq._random_state.get_state())
    with pytest.raises(ValueError, match='negative_sampling weights'):
        seq.fit(sequences())
    assert same_state(seq._random_state, before)
    rs = np.random.RandomState(8)
    before.set_state(rs.get_state())
    with pytest.raises(ValueError, match='negative_sampling weights'):
        sample_items(I, 10, random_state=rs, p=w)
    assert same_state(rs, before)
    with pytest.raises(ValueError, match='negative_sampling must be'):
        ImplicitFactorizationModel(negative_sampling='popular')
    with pytest.raises(ValueError, match='negative_sampling must be'):
        ImplicitSequenceModel(negative_sampling='popular')


def check_sharded_model_refuses():
    """The row-sharded model draws uniform negatives and does not gain the keyword: it says so instead of ignoring it."""
    from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel
    for value in ('popularity', np.ones(I)):
        with pytest.raises(NotImplementedError, match='negative_sampling'):
            ShardedImplicitFactorizationModel(negative_sampling=value)
    for value in ('uniform', None):
        ShardedImplicitFactorizationModel(negative_sampling=value, random_state=np.random.RandomState(1))


# ---- 9. the sampling module, repr and pickling ---------------------------------------------------------------------------------------
def check_sampling_module(engine, device):
    w = (1.0 / np.arange(1, I + 1)) ** 0.75
    w[::7] = 0.0
    p = w / w.sum()
    a, b = np.random.RandomState(4), np.random.RandomState(4)
    assert np.array_equal(sample_items(I, (5, 7), random_state=a, p=w), b.choice(I, size=(5, 7), p=p)) and same_state(a, b)
    assert np.array_equal(sample_items(I, (5, 7), random_state=a), b.randint(0, I, (5, 7), dtype=np.int64)) and same_state(a, b)
    for given in (w, ItemDistribution(w, I)):
        got = sample_items_device(I, (4, 9), a, engine=engine, device=device, p=given)
        assert got.dtype == torch.int64 and tuple(got.shape) == (4, 9)
        assert np.array_equal(got.cpu().numpy(), b.choice(I, size=(4, 9), p=p)) and same_state(a, b)
    got = sample_items_device(I, (4, 9), a, engine=engine, device=device)
    assert np.array_equal(got.cpu().numpy(), b.randint(0, I, (4, 9), dtype=np.int64)) and same_state(a, b)


def check_repr_and_pickle():
    inter = dataset()
    model = model_for('bpr', 23, negative_sampling='popularity')
    assert repr(model) == '<ImplicitFactorizationModel: [uninitialised]>'
    model.fit(inter)
    assert 'BilinearNet' in repr(model) and model._item_distribution.d_cdf is not None
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    clone = torch.load(buf, weights_only=False)
    dist = clone._item_distribution
    assert dist.d_cdf is None and dist.d_guide is None and same_bits(dist.p, model._item_distribution.p)
    assert np.array_equal(clone.predict(2), model.predict(2))
    model.fit(inter)
    clone.fit(inter)  # the device side is rebuilt
    assert clone._item_distribution.d_cdf is not None
    assert_same_fit(model, clone, 'after the pickle round trip')
