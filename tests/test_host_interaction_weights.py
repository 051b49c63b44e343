"""The models' `use_weights` keyword (fit() on Interactions.weights) through the emulator build of the kernels (no GPU): the
schedule, the validation, the autograd route and pickling.  The engine entry itself is tests/weights_checks.py."""
import io

import numpy as np
import pytest
import torch

import engine_checks as ec
from emu_backend import emu_lib
from spotlight_amd import _native, losses
from spotlight_amd.factorization import explicit as explicit_host
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.explicit import ExplicitFactorizationModel
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.interactions import Interactions
from spotlight_amd.torch_utils import minibatch, shuffle

U, I, N, B, EPOCHS, NN = 40, 30, 300, 64, 3, 3


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


def _adagrad(params):
    return torch.optim.Adagrad(params, lr=0.05)


def dataset(weights=True, ratings=False, seed=0):
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32)
    r = rs.randint(1, 6, N).astype(np.float32)
    w = (2.0 ** rs.uniform(-4, 4, N)).astype(np.float32)
    return Interactions(users, items, ratings=r if ratings else None, weights=w if weights else None, num_users=U, num_items=I)


def implicit_model(loss, seed, **kw):
    kw.setdefault('optimizer_func', _adagrad)
    return ImplicitFactorizationModel(loss=loss, embedding_dim=16, n_iter=EPOCHS, batch_size=B, num_negative_samples=NN,
                                      random_state=np.random.RandomState(seed), **kw)


def explicit_model(loss, seed, **kw):
    kw.setdefault('optimizer_func', _adagrad)
    return ExplicitFactorizationModel(loss=loss, embedding_dim=16, n_iter=EPOCHS, batch_size=B,
                                      random_state=np.random.RandomState(seed), **kw)


def tables_of(model):
    return [t.detach().cpu().numpy().copy() for t in model._net.tables()]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_state(a, b):
    a, b = a.get_state(), b.get_state()
    return (a[1] == b[1]).all() and a[2] == b[2]


class Recorded(object):
    """Copies of the epoch buffers every training call of a fit() was handed, read when the call is enqueued."""

    def __init__(self, monkeypatch, cls):
        self.epochs = []
        inner = cls.train

        def train(job, engine, stream, epoch_num):
            self.epochs.append([x.detach().cpu().numpy().copy() for x in job.slots[epoch_num % len(job.slots)]])
            return inner(job, engine, stream, epoch_num)
        monkeypatch.setattr(cls, 'train', train)


# ---- the weights change what is learned, and nothing else ------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['bpr', 'adaptive_hinge'])
def test_weighted_fit_differs_and_consumes_the_unweighted_stream(emu_device, monkeypatch, loss):
    inter = dataset()
    rec = Recorded(monkeypatch, host._ImplicitEpochs)
    plain = implicit_model(loss, 5)
    plain.fit(inter)
    plain_epochs, rec.epochs = rec.epochs, []
    weighted = implicit_model(loss, 5, use_weights=True)
    weighted.fit(inter)
    assert not same_bits(tables_of(plain)[0], tables_of(weighted)[0])
    assert same_state(plain._random_state, weighted._random_state)
    # ids and negatives of every epoch are the unweighted fit's; the weights went through the same permutation as their ids
    rs = np.random.RandomState(5)
    rs.randint(-10**8, 10**8)
    nn = NN if loss == 'adaptive_hinge' else 1
    assert len(rec.epochs) == len(plain_epochs) == EPOCHS
    for a, b in zip(plain_epochs, rec.epochs):
        assert len(a) == 3 and len(b) == 5
        for k in range(3):
            assert np.array_equal(a[k], b[k]), ('users', 'items', 'negatives')[k]
        users, items, w = shuffle(inter.user_ids, inter.item_ids, inter.weights, random_state=rs)
        for lo in range(0, N, B):
            rs.randint(0, I, len(users[lo:lo + B]) * nn, dtype=np.int64)
        assert np.array_equal(b[0], users) and np.array_equal(b[1], items) and same_bits(b[4], w)
    assert same_state(weighted._random_state, rs)


@pytest.mark.parametrize('loss', ['regression', 'poisson', 'logistic'])
def test_weighted_explicit_fit_differs_and_consumes_the_unweighted_stream(emu_device, monkeypatch, loss):
    inter = dataset(ratings=True)
    rec = Recorded(monkeypatch, explicit_host._ExplicitEpochs)
    plain = explicit_model(loss, 5)
    plain.fit(inter)
    weighted = explicit_model(loss, 5, use_weights=True)
    weighted.fit(inter)
    assert not same_bits(tables_of(plain)[0], tables_of(weighted)[0])
    assert same_state(plain._random_state, weighted._random_state)
    rs = np.random.RandomState(5)
    rs.randint(-10**8, 10**8)
    for a, b in zip(rec.epochs[:EPOCHS], rec.epochs[EPOCHS:]):
        users, items, r, w = shuffle(inter.user_ids, inter.item_ids, inter.ratings, inter.weights, random_state=rs)
        assert len(a) == 4 and len(b) == 6
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[3], b[4])
        assert np.array_equal(b[0], users) and same_bits(b[4], r) and same_bits(b[5], w)
    assert same_state(weighted._random_state, rs)


def test_large_epochs_take_the_two_lane_schedule(emu_device, monkeypatch):
    """Above _PIPELINE_MAX_DRAWS an unweighted fit runs the three-stage pipeline and opens its scopes; a weighted one hands its
    negatives in (two-lane) at every size and opens neither scope."""
    monkeypatch.setattr(host, '_PIPELINE_MAX_DRAWS', 100)
    inter = dataset()
    calls = []
    inner = host._epochs.run_three_stage
    monkeypatch.setattr(host._epochs, 'run_three_stage', lambda *a, **k: calls.append('three') or inner(*a, **k))
    small = implicit_model('bpr', 5, use_weights=True)
    small.fit(inter)
    assert calls == []
    assert emu_device.get_stat('shadowed_calls') == 0 and emu_device.get_stat('pingpong_calls') == 0
    plain = implicit_model('bpr', 5)
    plain.fit(inter)
    assert calls == ['three']  # (the unweighted fit of this size does take the pipeline)
    monkeypatch.setattr(host, '_PIPELINE_MAX_DRAWS', 1 << 22)
    ref = implicit_model('bpr', 5, use_weights=True)
    ref.fit(inter)
    for x, y in zip(tables_of(small), tables_of(ref)):
        assert same_bits(x, y)


# ---- against the autograd route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['pointwise', 'bpr', 'hinge', 'adaptive_hinge'])
def test_weighted_fit_matches_the_weighted_autograd_route(emu_device, loss):
    inter = dataset()
    fused = implicit_model(loss, 11, use_weights=True)
    fused.fit(inter)
    auto = implicit_model(loss, 11, use_weights=True)
    auto._initialize(inter)
    auto._autograd_route = True  # the same optimizer through the reference's loop and losses.py's weighted forms
    auto.fit(inter)
    assert not fused._autograd_route
    assert same_state(fused._random_state, auto._random_state)
    for t, (x, y) in enumerate(zip(tables_of(fused), tables_of(auto))):
        ec.assert_open_loop_drift(x, y, (loss, 'table', t))
    plain = implicit_model(loss, 11)
    plain._initialize(inter)
    plain._autograd_route = True
    plain.fit(inter)
    assert not same_bits(tables_of(plain)[0], tables_of(auto)[0])  # (and the route does read the weights)


@pytest.mark.parametrize('loss', ['regression', 'poisson', 'logistic'])
def test_weighted_explicit_fit_matches_a_torch_loop_on_the_weighted_losses(emu_device, loss):
    """The explicit model has no autograd route of its own: the reference's loop (explicit.py:213-236) is written out here over
    the model's own net, with losses.py's weighted forms."""
    inter = dataset(ratings=True)
    if loss == 'logistic':
        inter.ratings = np.where(inter.ratings > 3, 1.0, -1.0).astype(np.float32)
    fused = explicit_model(loss, 11, use_weights=True)
    fused.fit(inter)
    twin = explicit_model(loss, 11, use_weights=True)
    twin._initialize(inter)
    loss_func = {'regression': losses.regression_loss, 'poisson': losses.poisson_loss, 'logistic': losses.logistic_loss}[loss]
    rs = twin._random_state
    for _ in range(EPOCHS):
        arrays = shuffle(inter.user_ids, inter.item_ids, inter.ratings, inter.weights, random_state=rs)
        device = next(twin._net.parameters()).device
        tensors = [torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(device) for a in arrays[:2]] + \
                  [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays[2:]]
        for bu, bi, br, bw in minibatch(*tensors, batch_size=B):
            pred = twin._net(bu, bi)
            if loss == 'poisson':
                pred = torch.exp(pred)
            twin._optimizer.zero_grad()
            loss_func(br, pred, weights=bw).backward()
            twin._optimizer.step()
    assert same_state(fused._random_state, rs)
    for t, (x, y) in enumerate(zip(tables_of(fused), tables_of(twin))):
        ec.assert_open_loop_drift(x, y, (loss, 'table', t))


# ---- validation, before anything is drawn ------------------------------------------------------------------------------------------------
def _bad(which):
    w = np.ones(N, np.float32)
    w[7] = {'zero': 0.0, 'negative': -1.0, 'nan': np.nan, 'inf': np.inf}[which]
    return w


@pytest.mark.parametrize('which', ['none', 'zero', 'negative', 'nan', 'inf', 'length'])
@pytest.mark.parametrize('explicit', [False, True])
def test_bad_weights_raise_before_anything_is_drawn(emu_device, which, explicit):
    inter = dataset(ratings=explicit)
    inter.weights = None if which == 'none' else (np.ones(N + 1, np.float32) if which == 'length' else _bad(which))
    model = explicit_model('regression', 3, use_weights=True) if explicit else implicit_model('bpr', 3, use_weights=True)
    before = np.random.RandomState()
    before.set_state(model._random_state.get_state())
    with pytest.raises(ValueError, match='interactions.weights'):
        model.fit(inter)
    assert same_state(model._random_state, before)
    # the autograd route checks alike
    if not explicit:
        model = implicit_model('bpr', 3, use_weights=True, optimizer_func=lambda p: torch.optim.RMSprop(p, lr=0.01))
        before.set_state(model._random_state.get_state())
        with pytest.raises(ValueError, match='interactions.weights'):
            model.fit(inter)
        assert same_state(model._random_state, before)


def test_sharded_model_refuses_the_keyword():
    from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel
    with pytest.raises(ValueError, match='use_weights'):
        ShardedImplicitFactorizationModel(use_weights=True)
    ShardedImplicitFactorizationModel(use_weights=False, random_state=np.random.RandomState(1))


# ---- pickling and resuming ---------------------------------------------------------------------------------------------------------------------
def _round_trip(model):
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize('explicit', [False, True])
def test_a_weighted_model_pickles_and_resumes(emu_device, explicit):
    inter = dataset(ratings=explicit)
    model = explicit_model('regression', 23, use_weights=True) if explicit else implicit_model('bpr', 23, use_weights=True)
    model.fit(inter)
    clone = _round_trip(model)
    assert clone._use_weights and np.array_equal(clone.predict(2), model.predict(2))
    model.fit(inter)
    clone.fit(inter)
    for x, y in zip(tables_of(model), tables_of(clone)):
        assert same_bits(x, y)
    assert same_state(model._random_state, clone._random_state)


def test_a_model_pickled_before_the_keyword_loads_unweighted(emu_device):
    inter = dataset()
    old = implicit_model('bpr', 29)
    old.fit(inter)
    del old.__dict__['_use_weights']  # what such a pickle holds
    old = _round_trip(old)
    assert not hasattr(old, '_use_weights')
    old.fit(inter)  # resumes, unweighted
    new = implicit_model('bpr', 29)
    new.fit(inter)
    new.fit(inter)
    for x, y in zip(tables_of(old), tables_of(new)):
        assert same_bits(x, y)


# ---- the default is the reference's: weights ignored -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('explicit', [False, True])
def test_without_the_keyword_a_weights_array_is_ignored_bit_for_bit(emu_device, explicit):
    make = (lambda: explicit_model('regression', 31)) if explicit else (lambda: implicit_model('bpr', 31))
    a = make()  # (constructed and fitted in turn: the constructor seeds torch's generator, which initialises the tables)
    a.fit(dataset(weights=True, ratings=explicit))
    b = make()
    b.fit(dataset(weights=False, ratings=explicit))
    for x, y in zip(tables_of(a), tables_of(b)):
        assert same_bits(x, y)
    assert same_state(a._random_state, b._random_state)
