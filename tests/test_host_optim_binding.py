"""_OptimizerBinding (spotlight_amd/factorization/implicit.py) fed every torch optimizer option it must either carry into slk_optim
or refuse: for each row of MATRIX a small model is fit() as bound, then again with the binding forced to refuse (the autograd route
with the real torch optimizer); the route must be the one the row names, and a fused run must end where the generic one does.

U = 15, I = 25, D = 8, 200 interactions, minibatches of 64, 2 epochs, bpr, the same RandomState: the same initial tables, shuffles
and negatives on both routes.

TOLERANCE of "fused agrees with generic" (relative inf-norm per table): the largest difference over the rows that are bound
correctly, measured on the emulator build, is 1.5e-6 (the Adam rows at default betas and eps; the others
6e-8 .. 5e-7); TOL is 10 times that.  It must be, and is checked to be
(test_tolerance_separates_what_the_matrix_tells_apart), at least 10 times below the difference between the two GENERIC runs of every
pair of optimizers the matrix exists to tell apart -- the smallest of those gaps is 2.7e-4 (amsgrad against plain Adam; the next is
Adagrad's eps, 3.1e-3; coupled against decoupled weight decay at wd = 0.1: 7.2)."""
import numpy as np
import pytest
import torch

from emu_backend import emu_lib
from spotlight_amd import _native
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.explicit import ExplicitFactorizationModel
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.interactions import Interactions, SequenceInteractions
from spotlight_amd.sequence.implicit import ImplicitSequenceModel

TOL = 1.5e-5

O = torch.optim
FUSED, GENERIC = 'fused', 'generic'
# name -> (optimizer_func, sparse gradients, the route fit() must take)
MATRIX = {
    'adam_off': (lambda p: O.Adam(p, lr=.05, betas=(.5, .9), eps=1e-3, weight_decay=.1), False, FUSED),
    'adam_tensor_lr': (lambda p: O.Adam(p, lr=torch.tensor(.05)), False, FUSED),
    'adam_neutral_keys': (lambda p: O.Adam(p, lr=.05, foreach=False, differentiable=False), False, FUSED),
    'adam_decoupled_wd': (lambda p: O.Adam(p, lr=.05, weight_decay=.1, decoupled_weight_decay=True), False, GENERIC),
    'adam_decoupled_no_wd': (lambda p: O.Adam(p, lr=.05, decoupled_weight_decay=True), False, FUSED),  # (nothing to decouple)
    'adamw': (lambda p: O.AdamW(p, lr=.05, weight_decay=.1), False, GENERIC),
    'adam_amsgrad': (lambda p: O.Adam(p, lr=.05, amsgrad=True), False, GENERIC),
    'adam_maximize': (lambda p: O.Adam(p, lr=.05, maximize=True), False, GENERIC),
    'adagrad_off_sparse': (lambda p: O.Adagrad(p, lr=.05, lr_decay=.1, eps=1e-3, initial_accumulator_value=.1), True, FUSED),
    'adagrad_off_dense': (lambda p: O.Adagrad(p, lr=.05, lr_decay=.1, eps=1e-3, initial_accumulator_value=.1), False, FUSED),
    'adagrad_wd': (lambda p: O.Adagrad(p, lr=.05, weight_decay=.1, lr_decay=.1), False, FUSED),
    'sparse_adam_off': (lambda p: O.SparseAdam(list(p), lr=.05, betas=(.5, .9), eps=1e-3), True, FUSED),
    'sgd_dampening': (lambda p: O.SGD(p, lr=.05, dampening=.5), False, FUSED),
    'sgd_wd': (lambda p: O.SGD(p, lr=.05, weight_decay=.1), False, GENERIC),
    'sgd_momentum': (lambda p: O.SGD(p, lr=.05, momentum=.9), False, GENERIC),
}
# what the matrix exists to tell apart: (a row, the optimizer a wrong binding would have run instead, sparse gradients)
PAIRS = {
    'coupled_vs_decoupled_wd': ('adam_decoupled_wd', lambda p: O.Adam(p, lr=.05, weight_decay=.1)),
    'adam_betas_eps': ('adam_off', lambda p: O.Adam(p, lr=.05, weight_decay=.1)),
    'adam_wd': ('adam_off', lambda p: O.Adam(p, lr=.05, betas=(.5, .9), eps=1e-3)),
    'adagrad_lr_decay': ('adagrad_off_dense', lambda p: O.Adagrad(p, lr=.05, eps=1e-3, initial_accumulator_value=.1)),
    'adagrad_eps': ('adagrad_off_dense', lambda p: O.Adagrad(p, lr=.05, lr_decay=.1, initial_accumulator_value=.1)),
    'adagrad_accumulator': ('adagrad_off_dense', lambda p: O.Adagrad(p, lr=.05, lr_decay=.1, eps=1e-3)),
    'adagrad_wd': ('adagrad_wd', lambda p: O.Adagrad(p, lr=.05, lr_decay=.1)),
    'sparse_adam_betas_eps': ('sparse_adam_off', lambda p: O.SparseAdam(list(p), lr=.05)),
    'sgd_wd': ('sgd_wd', lambda p: O.SGD(p, lr=.05)),
    'amsgrad': ('adam_amsgrad', lambda p: O.Adam(p, lr=.05)),
}


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


def _refuse(self, optimizer, params, sparse):
    raise NotImplementedError('the binding is forced to refuse: the autograd route with the real torch optimizer')


def _interactions():
    rs = np.random.RandomState(3)
    return Interactions(rs.randint(0, 15, 200).astype(np.int32), rs.randint(0, 25, 200).astype(np.int32), num_users=15, num_items=25)


def _fit(func, sparse):
    model = ImplicitFactorizationModel(loss='bpr', embedding_dim=8, n_iter=2, batch_size=64, optimizer_func=func, sparse=sparse,
                                       random_state=np.random.RandomState(7))
    model.fit(_interactions())
    return model, [w.detach().numpy().copy() for w in model._net.tables()]


_GENERIC = {}


def _generic(monkeypatch, key, func, sparse):
    """The forced-generic run of an optimizer_func (computed once: it does not depend on the binding under test)."""
    if key not in _GENERIC:
        with monkeypatch.context() as m:
            m.setattr(host._OptimizerBinding, '__init__', _refuse)
            model, tables = _fit(func, sparse)
        assert model._autograd_route and model._binding is None
        _GENERIC[key] = tables
    return _GENERIC[key]


def _rel(a, b):
    # (bpr leaves the user biases at zero on every route: 0 against 0)
    return max(float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30)) for x, y in zip(a, b))


@pytest.mark.parametrize('name', sorted(MATRIX))
def test_route_and_result(emu_device, monkeypatch, name):
    func, sparse, route = MATRIX[name]
    model, tables = _fit(func, sparse)
    assert model._autograd_route == (route == GENERIC), (name, 'ran', GENERIC if model._autograd_route else FUSED)
    assert (model._binding is None) == (route == GENERIC)
    generic = _generic(monkeypatch, name, func, sparse)
    for t in tables:
        assert np.isfinite(t).all()
    if route == FUSED:
        print('BINDING_REL %s %.3e' % (name, _rel(tables, generic)))
        assert _rel(tables, generic) <= TOL, (name, _rel(tables, generic))
    else:  # the same route twice: the same tables
        assert _rel(tables, generic) == 0.0


def test_tolerance_separates_what_the_matrix_tells_apart(emu_device, monkeypatch):
    for key, (row, other) in sorted(PAIRS.items()):
        func, sparse, _ = MATRIX[row]
        gap = _rel(_generic(monkeypatch, row, func, sparse), _generic(monkeypatch, 'pair/' + key, other, sparse))
        print('BINDING_GAP %s %.3e' % (key, gap))
        assert gap >= 10 * TOL, (key, gap, TOL)


def test_adagrad_weight_decay_with_sparse_gradients_raises_torchs_message(emu_device):
    with pytest.raises(RuntimeError, match='weight_decay option is not compatible with sparse gradients'):
        _fit(MATRIX['adagrad_wd'][0], True)


def test_an_option_the_binding_does_not_know_is_refused():
    """A param-group key that is neither read nor arithmetic-neutral, away from the class's default: NotImplementedError (the
    generic route), not silence -- here a key a later torch might add, on a subclass that declares its default."""
    class FutureAdagrad(O.Adagrad):
        def __init__(self, params, lr=1e-2, centered=False):
            O.Adagrad.__init__(self, params, lr=lr)
            for g in self.param_groups:
                g['centered'] = centered

    for centered, refused in ((False, False), (True, True)):
        p = [torch.zeros(4, 3, requires_grad=True)]
        opt = FutureAdagrad(p, centered=centered)
        if refused:
            with pytest.raises(NotImplementedError, match='centered'):
                host._OptimizerBinding(opt, p, False)
        else:
            assert host._OptimizerBinding(opt, p, False).kind == 'adagrad'
    # a key without a class default (a scheduler's 'initial_lr') has nothing to differ from
    p = [torch.zeros(4, 3, requires_grad=True)]
    opt = O.Adagrad(p, lr=.05)
    torch.optim.lr_scheduler.StepLR(opt, 10)
    assert 'initial_lr' in opt.param_groups[0] and host._OptimizerBinding(opt, p, False).kind == 'adagrad'


# ---- the two other models share the binding; for their fused networks (PoolNet, BilinearNet) there is no generic route: a refusal of
# the binding is fit()'s NotImplementedError, never a silently different rule
def _seq_data():
    rs = np.random.RandomState(4)
    seqs = rs.randint(1, 25, (40, 6)).astype(np.int32)
    seqs[::3, :2] = 0
    return SequenceInteractions(seqs, num_items=25)


def test_sequence_model_binds_and_refuses(emu_device):
    def fit(func):
        m = ImplicitSequenceModel(loss='bpr', embedding_dim=8, n_iter=2, batch_size=16, optimizer_func=func,
                                  random_state=np.random.RandomState(7))
        m.fit(_seq_data())
        return m, [w.detach().numpy().copy() for w in m._net.tables()]

    m, tables = fit(MATRIX['adam_off'][0])
    assert m._binding.kind == 'adam_dense'
    assert m._binding.hp == dict(lr=.05, eps=1e-3, betas=(.5, .9), weight_decay=.1)
    assert m._binding.steps_taken() == 2 * 3
    # the hyper-parameters reached the kernels: the run is reproducible, and far from the runs with one of them at its default
    assert _rel(fit(MATRIX['adam_off'][0])[1], tables) == 0.0
    for other in (lambda p: O.Adam(p, lr=.05, weight_decay=.1), lambda p: O.Adam(p, lr=.05, betas=(.5, .9), eps=1e-3)):
        assert _rel(fit(other)[1], tables) >= 10 * TOL
    with pytest.raises(NotImplementedError, match='decoupled_weight_decay'):
        fit(MATRIX['adam_decoupled_wd'][0])


def test_explicit_model_binds_and_refuses(emu_device):
    """The fused row is held to the real torch optimizer: three epochs of ONE minibatch each (batch_size = the 200 interactions, so
    the shuffle only reorders a sum), against three steps of optimizer_func on float64 copies of the initial tables under the
    reference's regression loss, mean((rating - score)^2) -- within TOL.  lr_decay shows from the second step on."""
    rs = np.random.RandomState(3)
    users, items = rs.randint(0, 15, 200).astype(np.int32), rs.randint(0, 25, 200).astype(np.int32)
    ratings = rs.randint(1, 6, 200).astype(np.float32)
    inter = Interactions(users, items, ratings=ratings, num_users=15, num_items=25)
    mk = lambda func: ExplicitFactorizationModel(loss='regression', embedding_dim=8, n_iter=3, batch_size=200, optimizer_func=func,
                                                 random_state=np.random.RandomState(7))
    func = MATRIX['adagrad_wd'][0]
    m = mk(func)
    m._initialize(inter)
    P, Q, bu, bi = [torch.nn.Parameter(w.detach().clone().double()) for w in m._net.tables()]
    m.fit(inter)
    assert m._binding.kind == 'adagrad_dense'
    assert m._binding.hp == dict(lr=.05, eps=1e-10, weight_decay=.1, lr_decay=.1)
    assert m._binding.steps_taken() == 3
    opt = func([P, Q, bu, bi])
    u, i, r = torch.from_numpy(users.astype(np.int64)), torch.from_numpy(items.astype(np.int64)), torch.from_numpy(ratings).double()
    for _ in range(3):
        opt.zero_grad()
        score = (P[u] * Q[i]).sum(1) + bu[u].reshape(-1) + bi[i].reshape(-1)
        ((r - score) ** 2).mean().backward()
        opt.step()
    got = [w.detach().numpy() for w in m._net.tables()]
    want = [w.detach().numpy().reshape(g.shape) for w, g in zip((P, Q, bu, bi), got)]
    print('BINDING_REL explicit %.3e' % _rel(got, want))
    assert _rel(got, want) <= TOL, _rel(got, want)
    with pytest.raises(NotImplementedError, match='decoupled_weight_decay'):
        mk(MATRIX['adam_decoupled_wd'][0]).fit(inter)
