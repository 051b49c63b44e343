"""ImplicitFactorizationModel(loss='warp') through the emulator build of the kernels (no GPU): the constructor, the draws, the fused
fit against losses.warp_loss + autograd, use_weights / negative_sampling, fold_in(), and the models that refuse the loss.  The
engine entries themselves are tests/warp_checks.py; tests/test_gpu_warp.py runs these bodies on the device."""
import numpy as np
import pytest
import torch

import engine_checks as ec
import foldin_checks as fc
import optim_checks as oc
import warp_checks as wk
from emu_backend import emu_lib
from spotlight_amd import _native, foldin, losses
from spotlight_amd.datasets import synthetic
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.interactions import Interactions
from spotlight_amd.sampling import sample_items
from spotlight_amd.torch_utils import shuffle

NN = 5
ONE_STEP_SEED = 3  # the seed of test_one_minibatch_matches_warp_loss_through_autograd (its restatement meets the guard: asserted)


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


def dataset(seed=0, U=60, I=80, N=1500, weights=False):
    """spotlight_amd.datasets.synthetic data, far smaller than MovieLens-100K's test split."""
    inter = synthetic.generate_sequential(num_users=U, num_items=I, num_interactions=N, concentration_parameter=0.1,
                                          order=2, random_state=np.random.RandomState(seed))
    if weights:
        inter.weights = (2.0 ** np.random.RandomState(seed + 1).uniform(-3, 3, len(inter.user_ids))).astype(np.float32)
    return inter


def model_of(loss, seed=7, **kw):
    kw.setdefault('optimizer_func', _adagrad)
    kw.setdefault('n_iter', 2)
    kw.setdefault('batch_size', 256)
    return ImplicitFactorizationModel(loss=loss, embedding_dim=16, num_negative_samples=NN, random_state=np.random.RandomState(seed), **kw)


def same_state(a, b):
    a, b = a.get_state(), b.get_state()
    return (a[1] == b[1]).all() and a[2] == b[2]


def tables_of(model):
    return [t.detach().cpu().numpy().copy() for t in model._net.tables()]


# ---- fit(): it trains, and draws as adaptive hinge does -------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [{}, dict(use_weights=True), dict(negative_sampling='popularity'),
                                dict(use_weights=True, negative_sampling='popularity')], ids=lambda kw: '+'.join(sorted(kw)) or 'plain')
def test_fit_trains_and_consumes_the_random_state_as_adaptive_hinge_does(emu_device, kw):
    inter = dataset(weights=True)
    warp = model_of('warp', **kw)
    warp.fit(inter)
    adaptive = model_of('adaptive_hinge', **kw)
    adaptive.fit(inter)
    assert not warp._autograd_route
    assert same_state(warp._random_state, adaptive._random_state)
    w, a = tables_of(warp), tables_of(adaptive)
    assert all(np.isfinite(x).all() for x in w) and not np.array_equal(w[1], a[1])
    fresh = model_of('warp', **kw)
    fresh._initialize(inter)
    assert not np.array_equal(w[0], tables_of(fresh)[0])
    assert np.isfinite(warp.predict(3)).all()


def test_one_minibatch_matches_warp_loss_through_autograd(emu_device):
    """One epoch of one minibatch with the fused Adagrad against losses.warp_loss + autograd in float64 + torch's optimizer,
    within warp_checks' bounds, the hinge arguments of the float64 side at least GUARD away from 0."""
    inter = dataset(seed=ONE_STEP_SEED, N=300)
    n = len(inter.user_ids)
    # (a non-zero initial accumulator keeps Adagrad's first step well-conditioned: from sum = 0 it is lr * sign(g), which turns
    # the 1e-9 residue of a user's exactly cancelling bias terms into a step of lr -- the smoke test's reason for the same value)
    model = model_of('warp', seed=ONE_STEP_SEED, n_iter=1, batch_size=n,
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
    neg = score(np.repeat(users, NN), negs).view(NN, n)
    wk.assert_guard(float((neg - pos + 1.0).detach().abs().min()), 'model level')
    losses.warp_loss(pos, neg, inter.num_items).backward()
    g = [p.grad.numpy() for p in P]
    hp = dict(lr=0.05)
    zeros, sums = [np.zeros_like(x) for x in pre], [np.full_like(x, 0.1) for x in pre]
    tu, ti = np.unique(users), np.unique(np.concatenate([items, negs]))
    post = [oc.torch_step64('adagrad', hp, pre[t], sums[t], zeros[t], 0, g[t], touched) for t, touched in enumerate((tu, ti, tu, ti))]
    bounds = ec.step_update_bounds('adagrad', hp, pre, sums, zeros, g, 1, rel_delta=1e-5)
    got = [[x] for x in tables_of(model)]
    for t in range(4):
        w64 = np.asarray(post[t][0], np.float64)
        d = np.abs(got[t][0].astype(np.float64) - w64)
        tol = 1e-5 * np.abs(w64).max() + bounds[t][0].reshape(w64.shape)
        assert not (d > tol).any(), ('table', t, float((d / tol).max()))
    assert not np.array_equal(got[0][0], pre[0])


def test_custom_representation_and_unfused_optimizer_train_through_warp_loss(emu_device):
    """The generic routes: an optimizer without a fused update (RMSprop) runs the reference's loop on losses.warp_loss and consumes
    the stream as the fused fit does; the fused fit's own optimizer through that loop ends within the open-loop drift bound."""
    inter = dataset()
    fused = model_of('warp')
    fused.fit(inter)
    auto = model_of('warp', optimizer_func=lambda p: torch.optim.RMSprop(p, lr=0.01))
    auto.fit(inter)
    assert auto._autograd_route and same_state(fused._random_state, auto._random_state)
    assert all(np.isfinite(x).all() for x in tables_of(auto))
    # the same optimizer through both routes: the open-loop drift bound of the weighted-fit checks
    twin = model_of('warp')
    twin._initialize(inter)
    twin._autograd_route = True
    twin.fit(inter)
    for t, (x, y) in enumerate(zip(tables_of(fused), tables_of(twin))):
        ec.assert_open_loop_drift(x, y, ('warp', 'table', t))


def test_warp_loss_is_the_definition():
    """I = 7, n = 5: the weights log 6, log 3, log 2, 0, 0 across t = 0 .. 4; no violator and a NaN candidate give 0; the mask and
    the weights enter as in the other losses."""
    pos = torch.zeros(7, dtype=torch.float64, requires_grad=True)
    neg = torch.full((5, 7), -5.0, dtype=torch.float64)
    for c in range(5):
        neg[c, c] = 0.5 + c  # column c first violates at row c: x = 1.5 + c
    neg[4, 0] = 9.0          # a later, larger violator is not the first
    neg[0, 6] = float('nan')  # column 6: a NaN and no violator
    neg = neg.requires_grad_(True)
    per_column = [np.log(6) * 1.5, np.log(3) * 2.5, np.log(2) * 3.5, 0.0, 0.0, 0.0, 0.0]
    loss = losses.warp_loss(pos, neg, 7)
    assert abs(float(loss) - sum(per_column) / 7) < 1e-12
    loss.backward()
    want = np.zeros((5, 7))
    want[0, 0], want[1, 1], want[2, 2] = np.log(6) / 7, np.log(3) / 7, np.log(2) / 7
    assert np.allclose(neg.grad.numpy(), want, atol=1e-15) and np.allclose(pos.grad.numpy(), -want.sum(0), atol=1e-15)
    w = torch.tensor([1.0, 2.0, 4.0, 1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    assert abs(float(losses.warp_loss(pos, neg, 7, weights=w)) - (per_column[0] + 2 * per_column[1] + 4 * per_column[2]) / 11.0) < 1e-12
    mask = torch.tensor([1, 1, 0, 0, 0, 0, 0], dtype=torch.bool)
    assert abs(float(losses.warp_loss(pos, neg, 7, mask=mask)) - (per_column[0] + per_column[1]) / 2.0) < 1e-12
    assert float(losses.warp_loss(pos, neg, 2)) == 0.0


# ---- fold_in() ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adagrad', 'sgd'])
def test_fused_fold_in_equals_the_generic_route(emu_device, kind):
    """foldin_checks.check_model_fused_equals_generic for warp: one step of both routes from the same rows, the fused route's rows
    starting the next; the bound is check 1's from the float64 restatement's gradient of that step.
    Under warp a user's bias gradient is a sum of terms -w_c / m + w_c / m with another w_c per column: exactly 0 in the fused
    kernel (it adds column by column), a residue of 1e-9 on the generic route (autograd adds the positives' and the candidates'
    shares separately, in fp32).  From a ZERO state Adagrad and Adam turn that residue into a step of lr or lr / 10, so the two
    routes are compared where the step is well-conditioned: SGD, and Adagrad with the smoke test's initial accumulator of 0.1."""
    acc = 0.1 if kind == 'adagrad' else 0.0
    func = (lambda p: torch.optim.Adagrad(p, lr=0.05, initial_accumulator_value=acc)) if kind == 'adagrad' else None
    model, _ = fc.trained_like_model(kind, 'warp', D=16, optimizer_func=func)
    hp = fc.MODEL_KINDS[kind][2]
    I, D, steps = model._num_items, 16, 3
    new = fc.new_users(I)
    off, items, H = foldin.history_csr(model, new)
    n, nn = int(off[-1]), model._num_negative_samples
    rs = np.random.RandomState(8)
    neg = rs.randint(0, I, (steps, nn, n)).astype(np.int64)
    E, b = rs.normal(0, 0.25, (H, D)).astype(np.float32), rs.normal(0, 0.1, H).astype(np.float32)
    before, state = fc.snapshot(model), model._random_state.get_state()
    pr = wk.Problem.__new__(wk.Problem)
    pr.D, pr.I, pr.H, pr.nn, pr.off, pr.items = D, I, H, nn, off, items
    pr.V, pr.bi = model._net.tables()[1].detach().cpu().numpy(), model._net.tables()[3].detach().cpu().numpy().reshape(-1)
    z = lambda x: np.zeros(np.shape(x), np.float32)
    for t in range(steps):
        fused = model.fold_in(new, n_iter=1, init=(E, b), negatives=neg[t:t + 1])
        generic = model._fold_in_generic(new, n_iter=1, init=(E, b), negatives=neg[t:t + 1])
        pr.neg = neg[t:t + 1]
        pre = [E, b, z(E), z(b), z(E), z(b)]
        for u in range(H):
            o0, o1 = int(off[u]), int(off[u + 1])
            if o0 == o1:
                for got in (fused, generic):
                    assert fc.same_bits(got[0][u], E[u]) and fc.same_bits(got[1][u:u + 1], b[u:u + 1])
                continue
            _, _, g, xmin = wk.restate_fold_user(kind, hp, pr, pre, u, 0, 0)
            wk.assert_guard(xmin, (kind, 'step', t, 'user', u))
            pre_p = [E[u:u + 1], pr.V, b[u:u + 1], pr.bi]
            gs = [g[0], np.zeros(pr.V.shape), g[2], np.zeros(pr.bi.shape)]
            bounds = ec.step_update_bounds(kind, hp, pre_p, [z(x) + np.float32(acc) for x in pre_p], [z(x) for x in pre_p], gs, 1,
                                           rel_delta=1e-5)
            for tab, got, want in ((0, fused[0][u], generic[0][u]), (2, fused[1][u:u + 1], generic[1][u:u + 1])):
                w64 = np.asarray(want, np.float64).ravel()
                d = np.abs(np.asarray(got, np.float64).ravel() - w64)
                tol = 1e-5 * max(np.abs(w64).max(), 1e-30) + np.asarray(bounds[tab][0], np.float64).ravel()
                assert not (d > tol).any(), (kind, 'step', t, 'user', u, tab, float(d.max()))
        assert not fc.same_bits(fused[0], E)
        E, b = fused
    for x, y in zip(fc.snapshot(model), before):
        assert fc.same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y)
    after = model._random_state.get_state()
    assert (after[1] == state[1]).all() and after[2] == state[2]


def test_fold_in_draws_num_negative_samples_per_position(emu_device):
    model, _ = fc.trained_like_model('adagrad', 'warp')
    twin, _ = fc.trained_like_model('adagrad', 'adaptive_hinge')
    new = fc.new_users(model._num_items)
    init = (np.full((new.num_users, 16), 0.05, np.float32), np.zeros(new.num_users, np.float32))
    a, b = model.fold_in(new, n_iter=2, init=init), twin.fold_in(new, n_iter=2, init=init)
    assert same_state(model._random_state, twin._random_state)
    assert np.isfinite(a[0]).all() and not fc.same_bits(a[0], b[0])


def test_fold_in_over_an_item_bloom_table_takes_the_generic_route(emu_device):
    bloom, _ = fc.trained_like_model('adagrad', 'warp', item_bloom=True)
    new = fc.new_users(bloom._num_items)
    rs = np.random.RandomState(4)
    H, n = new.num_users, len(new.user_ids)
    init = (rs.normal(0, 0.25, (H, 16)).astype(np.float32), rs.normal(0, 0.1, H).astype(np.float32))
    neg = rs.randint(0, bloom._num_items, (2, bloom._num_negative_samples, n)).astype(np.int64)
    got = bloom.fold_in(new, n_iter=2, init=init, negatives=neg)
    assert np.isfinite(got[0]).all() and not fc.same_bits(got[0], init[0])


# ---- the models that do not have it ------------------------------------------------------------------------------------------------------------
def test_the_sharded_model_refuses_before_drawing():
    from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel
    rs = np.random.RandomState(3)
    before = np.random.RandomState()
    before.set_state(rs.get_state())
    for args, kw in (((), dict(loss='warp')), (('warp',), {})):
        with pytest.raises(NotImplementedError, match='warp is not built on the row-sharded path'):
            ShardedImplicitFactorizationModel(*args, random_state=rs, **kw)
    assert same_state(rs, before)
    ShardedImplicitFactorizationModel(loss='adaptive_hinge', random_state=rs)  # (the other losses construct, and draw the seed)
    assert not same_state(rs, before)


def test_the_sequence_model_keeps_its_assertion():
    from spotlight_amd.sequence.implicit import ImplicitSequenceModel
    with pytest.raises(AssertionError):
        ImplicitSequenceModel(loss='warp')


def test_the_constructor_accepts_warp_and_nothing_new_besides():
    ImplicitFactorizationModel(loss='warp', random_state=np.random.RandomState(1))
    with pytest.raises(AssertionError):
        ImplicitFactorizationModel(loss='wsabie')
    assert _native.LOSS_KINDS['warp'] == 7
