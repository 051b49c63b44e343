"""ImplicitFactorizationModel(loss='softmax') through the emulator build of the kernels (no GPU): the constructor, the draws, the
fused fit against losses.softmax_loss + autograd, use_weights / negative_sampling / verify_negatives, the generic routes,
fold_in(), and the models that refuse the loss.  The engine entries themselves are tests/softmax_checks.py;
tests/test_gpu_softmax.py runs these bodies on the device."""
import numpy as np
import pytest
import torch

import engine_checks as ec
import foldin_checks as fc
import optim_checks as oc
from emu_backend import emu_lib
from spotlight_amd import _native, losses
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.sampling import sample_items
from spotlight_amd.torch_utils import shuffle
from test_host_warp import dataset, same_state, tables_of

NN = 5


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


def model_of(loss, seed=7, **kw):
    kw.setdefault('optimizer_func', lambda p: torch.optim.Adagrad(p, lr=0.05))
    kw.setdefault('n_iter', 3)
    kw.setdefault('batch_size', 256)
    return ImplicitFactorizationModel(loss=loss, embedding_dim=16, num_negative_samples=NN, random_state=np.random.RandomState(seed), **kw)


# ---- fit(): it trains, and draws as adaptive hinge does -------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [{}, dict(use_weights=True), dict(negative_sampling='popularity')],
                         ids=lambda kw: '+'.join(sorted(kw)) or 'plain')
def test_fit_trains_and_consumes_the_random_state_as_adaptive_hinge_does(emu_device, kw):
    """The last epoch's loss is below the first epoch's and below log(n + 1), where small initial embeddings start; the
    RandomState ends bit-exactly where an adaptive_hinge fit with the same n leaves it."""
    inter = dataset(weights=True)
    soft = model_of('softmax', **kw)
    seen = []
    orig = host._epochs.end_epoch
    host._epochs.end_epoch = lambda num, loss, verbose: (seen.append(float(loss)), orig(num, loss, verbose))[1]
    try:
        soft.fit(inter)
    finally:
        host._epochs.end_epoch = orig
    assert len(seen) == 3 and np.isfinite(seen).all(), seen
    assert seen[-1] < seen[0] and seen[-1] < np.log(NN + 1.0), seen
    assert seen[0] < 1.05 * np.log(NN + 1.0), seen  # (the first epoch's mean starts at log(n + 1) and only falls)
    adaptive = model_of('adaptive_hinge', **kw)
    adaptive.fit(inter)
    assert not soft._autograd_route
    assert same_state(soft._random_state, adaptive._random_state)
    s, a = tables_of(soft), tables_of(adaptive)
    assert all(np.isfinite(x).all() for x in s) and not np.array_equal(s[1], a[1])
    assert np.isfinite(soft.predict(3)).all()


def test_verified_negatives_fit_and_count(emu_device):
    """verify_negatives=True fits and fills negative_verification_; the fused route's selection is the numpy rule applied to
    each draw's OWN user (flat slot f of a minibatch belongs to user f // n): both routes count the same slots."""
    inter = dataset()
    fused = model_of('softmax', verify_negatives=True, n_iter=2)
    fused.fit(inter)
    v = fused.negative_verification_
    n = len(inter.user_ids)
    assert v['candidates'] == 2 * n * NN * 4 and 0 < v['replaced'] <= 2 * n * NN and 0 <= v['unresolved'] <= v['replaced'] + 2 * n * NN
    assert all(np.isfinite(x).all() for x in tables_of(fused))
    auto = model_of('softmax', verify_negatives=True, n_iter=2)
    auto._initialize(inter)
    auto._autograd_route = True
    auto.fit(inter)
    assert same_state(fused._random_state, auto._random_state)
    # (the draws do not depend on the tables: the two routes see the same candidates and must pick the same ones)
    assert auto.negative_verification_ == v


def test_one_minibatch_matches_softmax_loss_through_autograd(emu_device):
    """One epoch of one minibatch with the fused Adagrad against losses.softmax_loss + autograd in float64 + torch's optimizer:
    every element within engine_checks.step_update_bounds at rel_delta = 1e-5 plus 1e-5 of the tensor's largest magnitude."""
    inter = dataset(seed=3, N=300)
    n = len(inter.user_ids)
    model = model_of('softmax', seed=3, n_iter=1, batch_size=n,
                     optimizer_func=lambda p: torch.optim.Adagrad(p, lr=0.05, initial_accumulator_value=0.1))
    model._initialize(inter)
    pre = tables_of(model)
    rs = np.random.RandomState()
    rs.set_state(model._random_state.get_state())
    model.fit(inter)
    users, items = shuffle(inter.user_ids, inter.item_ids, random_state=rs)
    negs = sample_items(inter.num_items, n * NN, random_state=rs)
    assert same_state(model._random_state, rs)
    tl = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    P = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in pre]
    score = lambda us, its: (P[0][tl(us)] * P[1][tl(its)]).sum(1) + P[2][tl(us)].squeeze(-1) + P[3][tl(its)].squeeze(-1)
    pos = score(users, items)
    neg = score(np.repeat(users, NN), negs).view(n, NN).t()  # each positive against its own draws
    losses.softmax_loss(pos, neg).backward()
    g = [p.grad.numpy() for p in P]
    hp = dict(lr=0.05)
    zeros, sums = [np.zeros_like(x) for x in pre], [np.full_like(x, 0.1) for x in pre]
    tu, ti = np.unique(users), np.unique(np.concatenate([items, negs]))
    post = [oc.torch_step64('adagrad', hp, pre[t], sums[t], zeros[t], 0, g[t], touched) for t, touched in enumerate((tu, ti, tu, ti))]
    bounds = ec.step_update_bounds('adagrad', hp, pre, sums, zeros, g, 1, rel_delta=1e-5)
    got = tables_of(model)
    for t in range(4):
        w64 = np.asarray(post[t][0], np.float64)
        d = np.abs(got[t].astype(np.float64) - w64)
        tol = 1e-5 * np.abs(w64).max() + bounds[t][0].reshape(w64.shape)
        assert not (d > tol).any(), ('table', t, float((d / tol).max()))
    assert not np.array_equal(got[0], pre[0])


def test_custom_representation_and_unfused_optimizer_train_through_softmax_loss(emu_device):
    """The generic routes: an optimizer without a fused update (RMSprop) and a custom representation run the reference's loop
    on losses.softmax_loss and consume the stream as the fused fit does; the fused fit's own optimizer through that loop ends
    within the open-loop drift bound."""
    from spotlight_amd.factorization.representations import BilinearNet
    inter = dataset()
    fused = model_of('softmax', n_iter=2)
    fused.fit(inter)
    auto = model_of('softmax', n_iter=2, optimizer_func=lambda p: torch.optim.RMSprop(p, lr=0.01))
    auto.fit(inter)
    assert auto._autograd_route and same_state(fused._random_state, auto._random_state)
    assert all(np.isfinite(x).all() for x in tables_of(auto))

    class Custom(torch.nn.Module):
        def __init__(self, U, I):
            super().__init__()
            self.inner = BilinearNet(U, I, 16)

        def forward(self, user_ids, item_ids):
            return self.inner(user_ids, item_ids)

    custom = model_of('softmax', n_iter=2, representation=Custom(inter.num_users, inter.num_items))
    custom.fit(inter)
    assert custom._autograd_route and same_state(fused._random_state, custom._random_state)
    assert all(np.isfinite(p.detach().cpu().numpy()).all() for p in custom._net.parameters())
    twin = model_of('softmax', n_iter=2)
    twin._initialize(inter)
    twin._autograd_route = True
    twin.fit(inter)
    got, ref = tables_of(fused), tables_of(twin)
    for t in (0, 1, 3):
        ec.assert_open_loop_drift(got[t], ref[t], ('softmax', 'table', t))
    # The user biases: every pair of an interaction is the same user's, so their gradient is 0 in exact arithmetic.  The fused
    # route applies exactly 0 (include/spotlight_hip.h) and the ZeroEmbedding stays zero; autograd's fp32 sum leaves a residue
    # of 1e-9 per step, which Adagrad from a zero accumulator turns into steps of lr -- noise, bounded by lr per step taken.
    assert not got[2].any()
    assert np.abs(ref[2]).max() <= 0.05 * 2 * ((len(inter.user_ids) + 255) // 256)


def test_softmax_loss_is_the_definition():
    pos = torch.tensor([0.3, -1.0, 2.0], dtype=torch.float64, requires_grad=True)
    neg = torch.tensor([[0.1, 0.5, -3.0], [-0.2, 1.5, 0.0]], dtype=torch.float64, requires_grad=True)  # [n = 2, B = 3]
    s = np.array([[0.3, -1.0, 2.0], [0.1, 0.5, -3.0], [-0.2, 1.5, 0.0]])
    p = np.exp(s) / np.exp(s).sum(0)
    per = -np.log(p[0])
    loss = losses.softmax_loss(pos, neg)
    assert abs(float(loss.detach()) - per.mean()) < 1e-12
    loss.backward()
    assert np.allclose(neg.grad.numpy(), p[1:] / 3, atol=1e-15) and np.allclose(pos.grad.numpy(), (p[0] - 1) / 3, atol=1e-15)
    w = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
    assert abs(float(losses.softmax_loss(pos, neg, weights=w).detach()) - (per * [1, 2, 4]).sum() / 7.0) < 1e-12
    mask = torch.tensor([1, 1, 0], dtype=torch.bool)
    assert abs(float(losses.softmax_loss(pos, neg, mask=mask).detach()) - per[:2].mean()) < 1e-12
    # n = 1 is softplus(neg - pos); a score of +-1000 does not overflow
    one = losses.softmax_loss(pos.detach(), neg.detach()[:1])
    assert abs(float(one) - float(torch.nn.functional.softplus(neg.detach()[0] - pos.detach()).mean())) < 1e-12
    big = losses.softmax_loss(torch.tensor([1000.0, -1000.0], dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64))
    assert abs(float(big) - (1000.0 + np.log(2.0)) / 2) < 1e-9


# ---- fold_in() ---------------------------------------------------------------------------------------------------------------------------------
def test_fold_in_runs_the_generic_route_and_draws_num_negative_samples_per_position(emu_device):
    from spotlight_amd import foldin
    model, _ = fc.trained_like_model('adagrad', 'softmax')
    twin, _ = fc.trained_like_model('adagrad', 'adaptive_hinge')
    new = fc.new_users(model._num_items)
    init = (np.full((new.num_users, 16), 0.05, np.float32), np.zeros(new.num_users, np.float32))
    calls = []
    orig = foldin.generic_steps
    foldin.generic_steps = lambda *a, **k: (calls.append(a[5].shape), orig(*a, **k))[1]
    try:
        a = model.fold_in(new, n_iter=2, init=init)
    finally:
        foldin.generic_steps = orig
    b = twin.fold_in(new, n_iter=2, init=init)
    assert calls == [(2, model._num_negative_samples, len(new.user_ids))], calls  # (the generic route, nn draws per position)
    assert same_state(model._random_state, twin._random_state)
    assert np.isfinite(a[0]).all() and not fc.same_bits(a[0], b[0]) and not fc.same_bits(a[0], init[0])
    # ... and so does the route asked for by name, over negatives that are handed in
    g = model._fold_in_generic(new, n_iter=2, init=init, negatives=np.random.RandomState(1).randint(
        0, model._num_items, (2, model._num_negative_samples, len(new.user_ids))).astype(np.int64))
    assert np.isfinite(g[0]).all()


# ---- the models that do not have it ------------------------------------------------------------------------------------------------------------
def test_the_sharded_model_refuses_before_drawing():
    from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel
    rs = np.random.RandomState(3)
    before = np.random.RandomState()
    before.set_state(rs.get_state())
    for args, kw in (((), dict(loss='softmax')), (('softmax',), {})):
        with pytest.raises(NotImplementedError, match='softmax is not built on the row-sharded path'):
            ShardedImplicitFactorizationModel(*args, random_state=rs, **kw)
    assert same_state(rs, before)


def test_the_sequence_model_refuses_before_drawing():
    from spotlight_amd.sequence.implicit import ImplicitSequenceModel
    rs = np.random.RandomState(3)
    before = np.random.RandomState()
    before.set_state(rs.get_state())
    with pytest.raises(AssertionError):
        ImplicitSequenceModel(loss='softmax', random_state=rs)
    assert same_state(rs, before)


def test_the_constructor_accepts_softmax_and_the_loss_id_is_eight():
    ImplicitFactorizationModel(loss='softmax', random_state=np.random.RandomState(1))
    with pytest.raises(AssertionError):
        ImplicitFactorizationModel(loss='infonce')
    assert _native.LOSS_KINDS['softmax'] == 8
    assert 'softmax' in host.MULTI_NEGATIVE_LOSSES and 'softmax' not in host.COLUMN_LOSSES
