"""Shared checks of slk_bilinear_foldin (include/spotlight_hip.h: rows for unseen users against frozen item tables), run on the
emulator build (tests/test_emu_foldin.py) and on the gfx950 library (tests/test_gpu_foldin.py).

The reference is the CPU oracle: ONE fold-in step of user u is one BilinearOracle.step() on a one-user model (u's row, bias and
optimizer state + the item tables) over u's interactions as the minibatch.  Everything else is a bit-for-bit statement of the
engine against itself (batch composition, step composition, empty histories, frozen item side).

Every check runs under "foldin_wg_min_len" = 0 (the default crossover, 64: both routes in a call with a long history), 1 (every
non-empty user on the workgroup route), 2^40 (every user on the wave route) and 20 (both routes among the short histories too)."""
import numpy as np
import pytest

from engine_checks import step_update_bounds
from oracle.oracle import BilinearOracle
from spotlight_amd import _native

LOSSES = ('bpr', 'hinge', 'pointwise', 'adaptive_hinge')
KINDS = ('adagrad', 'sgd', 'sparse_adam', 'adam_dense', 'adagrad_dense')
DS = (6, 24, 64, 72)       # row layouts (VEC, G) = (1, 8), (4, 8), (4, 16), (4, 32)
ITEMS = (7, 333)           # 7: a history is full of duplicates and negatives equal positives
USERS = (1, 5, 70)
ROUTES = (0, 1, 1 << 40, 20)   # "foldin_wg_min_len": default, all-workgroup, all-wave, and a crossover inside every mix of lengths
NN = 3                     # negatives per interaction under adaptive hinge
# adaptive hinge (and, in warp_checks, warp) at wide n: the gather takes a position's candidates SLK_FOLDIN_NEG_BATCH = 4 at a
# time -- n = 7 is one full batch and a ragged one, n = 64 sixteen.  Short histories (both routes under "foldin_wg_min_len" = 20,
# an empty one, a single interaction): the closed loop's cost, and under warp the number of hinge arguments its guard has to keep
# away from 0, grow with n * m.  (D, n, optimizer): every row layout, every n
WIDE_NS = (7, 64)
WIDE_LENGTHS = (37, 0, 3, 1, 9)
WIDE = [(6, 7, 'adagrad'), (24, 64, 'sgd'), (72, 7, 'sparse_adam'), (64, 64, 'adam_dense')]
SENTINEL = np.float32(-7.25)


def hparams(opt):
    hp = dict(lr=0.05)
    if opt.endswith('dense'):
        hp['weight_decay'] = 1e-3
    if opt == 'adagrad_dense':
        hp['lr_decay'] = 1e-2
    return hp


def group_lanes(D):
    """G of slk_pick_layout: lanes that share one embedding row."""
    need = D // 4 if D % 4 == 0 else D
    g = 1
    while g < need:
        g <<= 1
    return g


def history_lengths(D, H):
    """0, 1, the wave's group count 64 / G and its neighbours, 37, 300 -- plus, where H has room, the neighbours of the
    workgroup's group count 256 / G and of one unrolled trip of the wave (2 * 64 / G)."""
    ng = 64 // group_lanes(D)
    if H == 1:
        return [ng + 1]
    if H == 5:
        return [37, 0, ng, 300, 1]
    base = [0, 1, ng - 1, ng, ng + 1, 37, 300, 2 * ng + 1, 4 * ng - 1, 4 * ng, 4 * ng + 1, 2 * ng]
    out = [base[i % len(base)] for i in range(H)]
    for i in range(len(base), H):  # one long history is enough: the rest of the 300s become short ones
        if out[i] == 300:
            out[i] = 2 + i % 7
    return out


class Problem(object):
    """Histories (CSR), negatives [T][nn][n], frozen item tables and initial rows for H new users."""

    def __init__(self, D, I, H, loss, T, seed=0, lengths=None, nn=NN):
        rs = np.random.RandomState(1000 + 7 * D + 3 * I + H + seed)
        self.D, self.I, self.H, self.loss, self.T = D, I, H, loss, T
        self.nn = nn if loss == 'adaptive_hinge' else 1
        lens = np.asarray(history_lengths(D, H) if lengths is None else lengths, dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.n = int(self.off[-1])
        self.items = rs.randint(0, I, self.n).astype(np.int64)
        self.neg = rs.randint(0, I, (T, self.nn, self.n)).astype(np.int64)
        sc = min(0.3, 1.0 / np.sqrt(D))  # scores O(1): no saturated sigmoid
        self.V = rs.normal(0, sc, (I, D)).astype(np.float32)
        self.bi = rs.normal(0, 0.1, I).astype(np.float32)
        self.U = rs.normal(0, sc, (H, D)).astype(np.float32)
        self.b = rs.normal(0, 0.1, H).astype(np.float32)

    def subset(self, users):
        """The same problem for `users` (in that order), each with their slice of the negatives."""
        q = Problem.__new__(Problem)
        q.D, q.I, q.loss, q.T, q.nn, q.V, q.bi = self.D, self.I, self.loss, self.T, self.nn, self.V, self.bi
        q.H = len(users)
        cols = [np.arange(self.off[u], self.off[u + 1]) for u in users]
        q.off = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
        cols = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
        q.n = int(q.off[-1])
        q.items = self.items[cols]
        q.neg = np.ascontiguousarray(self.neg[:, :, cols])
        q.U, q.b = self.U[list(users)], self.b[list(users)]
        return q


class Fold(object):
    """Device side of a Problem: the new rows + their state in slots 0 / 2, the model's item tables in 1 / 3, and
    sentinel-filled buffers as optimizer state of the item tables (never read, never written)."""

    def __init__(self, be, pr, opt, state=None, step=0, hp=None):
        f32 = lambda x: be.alloc(np.array(x, dtype=np.float32, order='C'))
        self.be = be
        self.p = [f32(pr.U), f32(pr.V), f32(pr.b), f32(pr.bi)]
        z = lambda x: np.zeros(np.shape(x), np.float32)
        s = state if state is not None else (z(pr.U), z(pr.b), z(pr.U), z(pr.b))
        sent = lambda: f32(np.full(64, SENTINEL))
        self.s1 = [f32(s[0]), sent(), f32(s[1]), sent()]
        self.s2 = [f32(s[2]), sent(), f32(s[3]), sent()]
        self.tables = _native.make_tables([be.ptr(x) for x in self.p], pr.H, pr.I, pr.D)
        self.optim = _native.make_optim(opt, [be.ptr(x) for x in self.s1], [be.ptr(x) for x in self.s2], step=step,
                                        **(hparams(opt) if hp is None else hp))
        self.d_off, self.d_items = be.alloc(pr.off), be.alloc(pr.items if pr.n else np.zeros(1, np.int64))
        self.pr = pr

    def run(self, n_steps, t0=0, want_loss=True):
        """Steps t0 .. t0 + n_steps of the problem's negatives; returns the losses [n_steps][H].  The frozen side is checked
        on every call."""
        be, pr = self.be, self.pr
        neg = pr.neg[t0:t0 + n_steps]
        d_neg = be.alloc(neg if neg.size else np.zeros(1, np.int64))
        d_loss = be.alloc(np.full((n_steps, pr.H), np.nan, dtype=np.float32)) if want_loss else None
        be.engine.bilinear_foldin(self.tables, self.optim, be.ptr(self.d_off), be.ptr(self.d_items), pr.H, pr.n, pr.loss,
                                  pr.nn if pr.loss == 'adaptive_hinge' else NN, n_steps, be.ptr(d_neg), be.ptr(d_loss), be.stream)
        self.assert_frozen()
        return be.get(d_loss).copy() if want_loss else None

    def assert_frozen(self):
        be, pr = self.be, self.pr
        assert np.array_equal(be.get(self.p[1]).view(np.uint32), pr.V.view(np.uint32)), 'item embeddings changed'
        assert np.array_equal(be.get(self.p[3]).view(np.uint32), pr.bi.view(np.uint32)), 'item biases changed'
        for s in (self.s1[1], self.s1[3], self.s2[1], self.s2[3]):
            assert (be.get(s) == SENTINEL).all(), 'optimizer state of an item table was written'

    def result(self):
        """(row, bias, state1 row, state1 bias, state2 row, state2 bias) as host copies."""
        g = lambda x: self.be.get(x).copy()
        return [g(self.p[0]), g(self.p[2]), g(self.s1[0]), g(self.s1[2]), g(self.s2[0]), g(self.s2[2])]


def routed(be, value):
    return be.engine.options(foldin_wg_min_len=value)


def cancellation_floor(pr):
    """abs_delta of step_update_bounds for the 7-ITEM problems only; every other problem (and the model-level check) is held to
    the bare bound, 1e-5 * |want|inf + step_update_bounds(rel_delta=1e-5).

    With 7 items a history is full of duplicates and negatives equal positives, so a user's gradient is often a sum of terms
    that cancel EXACTLY in exact arithmetic (interaction 0 pushes item 5 away, interaction 1 pulls it in; under bpr / hinge the
    bias terms +g and -g).  The oracle (sparse_grads=True) accumulates the user's gradient interaction by interaction in history
    order; the engine gives interaction j to row group j mod (groups of the route), sums per group and then combines the groups,
    and sums the bias terms the same way.  Where the exact sum is 0, one order ends at 0.0 and the other at a rounding residue of
    1e-9, and Adam / Adagrad from a near-zero accumulator turn that residue into a step of lr: the bare bound, which scales with
    |g|inf ~ 1e-9 there, fails (seen on the emulator and on the GPU: adaptive_hinge / sparse_adam, dim 72, a row; adaptive_hinge /
    adagrad, the bias).  The fp32 rounding of such a sum does not scale with the sum but with its terms: their magnitudes add up
    to at most S = 2 max(1, |V|max) per element (m interactions, two terms each, every |dL/dscore| <= 1 / m), and the floor is
    2 ulp of S = S * 2^-22 -- the precedent of engine_checks.check_train_matches_oracle for its degenerate runs, from the number
    format alone.  It decides only where the gradient itself is ~0: those elements are identified by their gradient magnitude,
    there is no quota."""
    if pr.I != ITEMS[0]:
        return 0.0
    return 2.0 ** -22 * 2.0 * max(1.0, float(np.abs(pr.V).max()))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. closed loop against the oracle, per step ---------------------------------------------------------------------------------
def closed_loop_one_route(be, pr, opt, route, steps):
    hp = hparams(opt)
    adam = opt in ('sparse_adam', 'adam_dense')
    with routed(be, route):
        fold = Fold(be, pr, opt)
        for t in range(steps):
            pre = fold.result()
            got_loss = fold.run(1, t0=t)[0]
            assert fold.optim.step == t + 1
            got = fold.result()
            for u in range(pr.H):
                o0, o1 = int(pr.off[u]), int(pr.off[u + 1])
                m = o1 - o0
                what = (pr.loss, opt, pr.D, pr.I, pr.H, 'route', route, 'step', t, 'user', u, 'm', m)
                if m == 0:
                    assert got_loss[u] == 0.0, what
                    for x, y in zip(got, pre):
                        assert same_bits(x[u], y[u]), what
                    continue
                zV, zb = np.zeros_like(pr.V), np.zeros_like(pr.bi)
                pre_p = [pre[0][u:u + 1], pr.V, pre[1][u:u + 1], pr.bi]
                pre_s1 = [pre[2][u:u + 1], zV, pre[3][u:u + 1], zb]
                pre_s2 = [pre[4][u:u + 1], zV, pre[5][u:u + 1], zb]
                ora = BilinearOracle(*pre_p, opt=opt, sparse_grads=True, state1=pre_s1, state2=pre_s2, step=t, **hp)
                want_loss, g = ora.step(np.zeros(m, np.int64), pr.items[o0:o1], pr.neg[t, :, o0:o1].ravel(), loss=pr.loss,
                                        n_neg=pr.nn, want_grads=True)
                assert abs(float(got_loss[u]) - want_loss) <= 1e-5 * abs(want_loss), (what, float(got_loss[u]), want_loss)
                bounds = step_update_bounds(opt, hp, pre_p, pre_s1, pre_s2, g, t + 1, rel_delta=1e-5, abs_delta=cancellation_floor(pr))
                for tab, (ip, i1, i2) in ((0, (0, 2, 4)), (2, (1, 3, 5))):
                    dp, ds1, ds2 = bounds[tab]
                    for nm, gi, want, bound in (('param', ip, ora.p[tab], dp), ('state1', i1, ora.s1[tab], ds1),
                                                ('state2', i2, ora.s2[tab], ds2)):
                        if (nm == 'state2' and not adam) or (nm == 'state1' and opt == 'sgd'):
                            continue
                        w64 = np.asarray(want, np.float64).ravel()
                        d = np.abs(got[gi][u].astype(np.float64).ravel() - w64)
                        tol = 1e-5 * max(np.abs(w64).max(), 1e-30) + np.asarray(bound, np.float64).ravel()
                        assert not (d > tol).any(), (what, tab, nm, float(d.max()), float(tol.min()))


def check_closed_loop(be, loss, opt, D, I, H, steps=2):
    pr = Problem(D, I, H, loss, steps)
    for route in ROUTES:
        closed_loop_one_route(be, pr, opt, route, steps)


def check_wide_adaptive(be, D, n, opt, I=ITEMS[1], steps=2):
    """Adaptive hinge over n candidates per position (WIDE), every route, against the oracle's one-user step."""
    pr = Problem(D, I, len(WIDE_LENGTHS), 'adaptive_hinge', steps, lengths=WIDE_LENGTHS, nn=n)
    assert pr.neg.shape == (steps, n, sum(WIDE_LENGTHS))
    for route in ROUTES:
        closed_loop_one_route(be, pr, opt, route, steps)


# ---- 2. the item side is frozen ------------------------------------------------------------------------------------------------
def check_frozen(be, loss, opt, D=24, I=333, H=5):
    pr = Problem(D, I, H, loss, 3)
    for route in ROUTES:
        with routed(be, route):
            fold = Fold(be, pr, opt)
            fold.run(3)  # (asserts the frozen side)
            assert not same_bits(fold.result()[0], pr.U), 'nothing was trained'


# ---- 3. batch composition ---------------------------------------------------------------------------------------------------------
def check_batch_composition(be, loss, opt, D, I, H=5, T=2):
    pr = Problem(D, I, H, loss, T)
    perm = list(np.random.RandomState(5).permutation(H))
    for route in ROUTES:
        with routed(be, route):
            whole = Fold(be, pr, opt)
            whole_loss = whole.run(T)
            want = whole.result()
            for u in range(H):
                one = Fold(be, pr.subset([u]), opt)
                one_loss = one.run(T)
                assert same_bits(one_loss[:, 0], whole_loss[:, u]), ('loss of user alone', u, route)
                for x, y in zip(one.result(), want):
                    assert same_bits(x[0], y[u]), ('user alone', u, route)
            mixed = Fold(be, pr.subset(perm), opt)
            mixed_loss = mixed.run(T)
            assert same_bits(mixed_loss, whole_loss[:, perm]), ('loss, permuted users', route)
            for x, y in zip(mixed.result(), want):
                assert same_bits(x, y[perm]), ('permuted users', route)


# ---- 4. step composition ----------------------------------------------------------------------------------------------------------
def check_step_composition(be, loss, opt, D, I, H=5, T=3, lengths=None):
    pr = Problem(D, I, H, loss, T, lengths=lengths)
    for route in ROUTES:
        with routed(be, route):
            once = Fold(be, pr, opt)
            once_loss = once.run(T)
            assert once.optim.step == T
            stepwise = Fold(be, pr, opt)
            losses = [stepwise.run(1, t0=t)[0] for t in range(T)]
            assert stepwise.optim.step == T
            assert same_bits(np.stack(losses), once_loss), ('losses', route)
            for x, y in zip(stepwise.result(), once.result()):
                assert same_bits(x, y), ('T calls of one step against one call of T', route)


# ---- 5. empty histories -----------------------------------------------------------------------------------------------------------
def check_empty(be, loss='bpr', opt='sparse_adam', D=24, I=333):
    rs = np.random.RandomState(2)
    for lengths in ([0, 5, 0, 0, 40], [0, 0, 0]):
        pr = Problem(D, I, len(lengths), loss, 2, lengths=lengths)
        state = tuple(rs.rand(*np.shape(x)).astype(np.float32) for x in (pr.U, pr.b, pr.U, pr.b))
        for route in ROUTES:
            with routed(be, route):
                fold = Fold(be, pr, opt, state=state, step=4)
                pre = fold.result()
                loss_out = fold.run(2)
                assert fold.optim.step == 6
                post = fold.result()
                for u, m in enumerate(lengths):
                    if m == 0:
                        assert (loss_out[:, u] == 0.0).all() and not np.signbit(loss_out[:, u]).any()
                        for x, y in zip(post, pre):
                            assert same_bits(x[u], y[u]), ('empty history', u, route)
                    else:
                        assert (loss_out[:, u] > 0).all() and not same_bits(post[0][u], pre[0][u])
                fold.run(1, want_loss=False)  # d_loss is optional


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def check_refusals(be):
    pr = Problem(24, 333, 5, 'bpr', 1)
    fold = Fold(be, pr, 'adagrad')
    P = be.ptr
    d_neg = be.alloc(pr.neg)
    d_loss = be.alloc(np.zeros((1, pr.H), np.float32))

    def call(match, tables=fold.tables, optim=fold.optim, off=fold.d_off, items=fold.d_items, H=pr.H, n=pr.n, loss='bpr', n_neg=NN,
             n_steps=1, neg=d_neg):
        with pytest.raises(_native.SlkError, match=match) as e:
            be.engine.bilinear_foldin(tables, optim, P(off), P(items), H, n, loss, n_neg, n_steps, P(neg), P(d_loss), be.stream)
        assert e.value.code == _native.SLK_EINVAL

    ptrs = lambda: [P(x) for x in fold.p]
    tab = lambda ptrs_=None, H=pr.H, I=pr.I, D=pr.D, **kw: _native.make_tables(ptrs_ or ptrs(), H, I, D, **kw)
    call('NULL', off=None)
    call('NULL', items=None)
    call('NULL', neg=None)
    for t in range(4):
        q = ptrs()
        q[t] = None
        call(r'd_param\[%d\] is NULL' % t, tables=tab(q))
    s1 = [P(x) for x in fold.s1]
    s1[2] = None
    call(r'd_state1\[2\] is NULL', optim=_native.make_optim('adagrad', s1, [P(x) for x in fold.s2]))
    s2 = [P(x) for x in fold.s2]
    s2[0] = None
    call(r'd_state2\[0\] is NULL', optim=_native.make_optim('adam_dense', [P(x) for x in fold.s1], s2))
    call('must be at least 1', n_steps=0)
    call('must be at least 1', H=0, tables=tab(H=0))
    call('is negative', n=-1)
    for explicit in ('regression', 'poisson', 'logistic'):
        call('not an implicit-feedback loss', loss=explicit)
    call('adaptive hinge needs n_neg >= 1', loss='adaptive_hinge', n_neg=0)
    call('embedding dim 65 unsupported', tables=tab(D=65))
    call('BloomEmbedding table on the user side', tables=tab(user_bloom=_native.make_bloom(pr.H, 2)))
    call('BloomEmbedding table on the item side', tables=tab(item_bloom=_native.make_bloom(pr.I, 2)))
    call('num_users', tables=tab(H=pr.H + 1))
    # item biases inside an open bias-shadow scope (as slk_shard_scores refuses them)
    full = be.model([pr.U, pr.V, pr.b, pr.bi], opt='adagrad')
    with be.engine.bias_shadow(full.tables, full.optim, stream=be.stream):
        q = ptrs()
        q[3] = P(full.p[3])
        call('shadowed', tables=tab(q))
    assert fold.optim.step == 0 and same_bits(fold.result()[0], pr.U)  # no refused call trained anything
    fold.run(1)  # ... and the same arguments, made good, are answered
    assert fold.optim.step == 1


def check_profiled_as_user_pass(be):
    pr = Problem(24, 333, 5, 'bpr', 1)
    fold = Fold(be, pr, 'adagrad')
    be.engine.profile_enable(True)
    try:
        be.engine.profile_reset()
        fold.run(1)
        prof = be.engine.profile_read()
    finally:
        be.engine.profile_enable(False)
    assert prof['user_pass'][0] == 1 and all(v[0] == 0 for k, v in prof.items() if k != 'user_pass'), prof


# ---- 7. model level: ImplicitFactorizationModel.fold_in() / recommend_vectors() ---------------------------------------------------
# (tests/test_host_foldin.py through the emulator build, tests/test_gpu_foldin.py on the gfx950 library)
MODEL_KINDS = {
    # kind -> (optimizer_func, constructor arguments, the hyper-parameters step_update_bounds is told)
    'adagrad': (lambda p: __import__('torch').optim.Adagrad(p, lr=0.05), {}, dict(lr=0.05)),
    'sgd': (lambda p: __import__('torch').optim.SGD(p, lr=0.05), {}, dict(lr=0.05)),
    'sparse_adam': (lambda p: __import__('torch').optim.SparseAdam(p, lr=0.05), dict(sparse=True), dict(lr=0.05)),
    'adam_dense': (None, dict(l2=1e-3, learning_rate=0.05), dict(lr=0.05, weight_decay=1e-3)),
    'adagrad_dense': (lambda p: __import__('torch').optim.Adagrad(p, lr=0.05, weight_decay=1e-3, lr_decay=1e-2), {},
                      dict(lr=0.05, weight_decay=1e-3, lr_decay=1e-2)),
}


def trained_like_model(kind='adagrad', loss='bpr', D=16, U=61, I=147, seed=11, item_bloom=False, user_bloom=False, optimizer_func=None,
                       **kw):
    """An initialised ImplicitFactorizationModel whose tables hold random values of a trained model's scale (scores O(1))."""
    import torch
    from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
    from spotlight_amd.factorization.representations import BilinearNet
    from spotlight_amd.interactions import Interactions
    from spotlight_amd.layers import BloomEmbedding
    rs = np.random.RandomState(seed)
    train = Interactions(rs.randint(0, U, 900).astype(np.int32), rs.randint(0, I, 900).astype(np.int32), num_users=U, num_items=I)
    func, ctor, _ = MODEL_KINDS[kind]
    ctor = dict(ctor, **kw)
    rep = None
    if item_bloom or user_bloom:
        mk = lambda n: BloomEmbedding(n, D, compression_ratio=0.5, num_hash_functions=2)
        rep = BilinearNet(U, I, D, user_embedding_layer=mk(U) if user_bloom else None, item_embedding_layer=mk(I) if item_bloom else None)
    model = ImplicitFactorizationModel(loss=loss, embedding_dim=D, n_iter=3, batch_size=96, random_state=np.random.RandomState(42),
                                       optimizer_func=optimizer_func or func, representation=rep, **ctor)
    model._initialize(train)
    sc = min(0.3, 1.0 / np.sqrt(D))
    with torch.no_grad():
        for t in model._net.tables():
            t.copy_(torch.from_numpy(rs.normal(0, sc if t.shape[1] > 1 else 0.1, tuple(t.shape)).astype(np.float32)))
    return model, train


def new_users(I, lengths=(0, 1, 3, 4, 5, 37, 300, 2, 0, 9), seed=3):
    """Interactions of H new users, in shuffled order (the CSR comes from a stable sort), with duplicates."""
    from spotlight_amd.interactions import Interactions
    rs = np.random.RandomState(seed)
    users = np.repeat(np.arange(len(lengths)), lengths)
    items = rs.randint(0, I, users.size)
    order = rs.permutation(users.size)
    return Interactions(users[order].astype(np.int32), items[order].astype(np.int32), num_users=len(lengths), num_items=I)


def snapshot(model):
    import torch
    out = [p.detach().cpu().numpy().copy() for p in model._net.parameters()]
    for st in model._optimizer.state.values():
        out += [v.detach().cpu().numpy().copy() for v in st.values() if torch.is_tensor(v)]
    return out


def check_model_fused_equals_generic(kind, loss, D=16, steps=3):
    """Closed loop through init= / negatives=: from the same rows both routes take ONE step (fresh state); the fused route's rows
    start the next step.  Bound: check 1's, from the oracle's gradient of that step."""
    from spotlight_amd import foldin
    model, _ = trained_like_model(kind, loss, D=D)
    hp = MODEL_KINDS[kind][2]
    I = model._num_items
    new = new_users(I)
    off, items, H = foldin.history_csr(model, new)
    n = int(off[-1])
    nn = model._num_negative_samples if loss == 'adaptive_hinge' else 1
    rs = np.random.RandomState(8)
    neg = rs.randint(0, I, (steps, nn, n)).astype(np.int64)
    E, b = rs.normal(0, 0.25, (H, D)).astype(np.float32), rs.normal(0, 0.1, H).astype(np.float32)
    before = snapshot(model)
    state = model._random_state.get_state()
    V, _, bi = [t.detach().cpu().numpy() for t in model._net.tables()[1:]]
    bi = bi.reshape(-1)
    for t in range(steps):
        fused = model.fold_in(new, n_iter=1, init=(E, b), negatives=neg[t:t + 1])
        generic = model._fold_in_generic(new, n_iter=1, init=(E, b), negatives=neg[t:t + 1])
        assert fused[0].shape == (H, D) and fused[1].shape == (H,) and fused[0].dtype == fused[1].dtype == np.float32
        for u in range(H):
            o0, o1 = int(off[u]), int(off[u + 1])
            if o0 == o1:
                for got in (fused, generic):
                    assert same_bits(got[0][u], E[u]) and same_bits(got[1][u:u + 1], b[u:u + 1]), ('empty history', u)
                continue
            z = lambda x: np.zeros_like(x)
            pre_p = [E[u:u + 1], V, b[u:u + 1], bi]
            ora = BilinearOracle(*pre_p, opt=kind, sparse_grads=True, **hp)
            _, g = ora.step(np.zeros(o1 - o0, np.int64), items[o0:o1], neg[t, :, o0:o1].ravel(), loss=loss, n_neg=nn, want_grads=True)
            bounds = step_update_bounds(kind, hp, pre_p, [z(x) for x in pre_p], [z(x) for x in pre_p], g, 1, rel_delta=1e-5)
            for tab, got, want in ((0, fused[0][u], generic[0][u]), (2, fused[1][u:u + 1], generic[1][u:u + 1])):
                w64 = np.asarray(want, np.float64).ravel()
                d = np.abs(np.asarray(got, np.float64).ravel() - w64)
                tol = 1e-5 * max(np.abs(w64).max(), 1e-30) + np.asarray(bounds[tab][0], np.float64).ravel()
                assert not (d > tol).any(), (kind, loss, 'step', t, 'user', u, tab, float(d.max()))
        assert not same_bits(fused[0], E)
        E, b = fused
    # the model itself: every parameter and optimizer-state tensor byte-identical, the RandomState untouched (negatives given)
    for x, y in zip(snapshot(model), before):
        assert same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y)
    after = model._random_state.get_state()
    assert (after[1] == state[1]).all() and after[2] == state[2]


def check_model_random_state(loss):
    from spotlight_amd.sampling import sample_items
    model, _ = trained_like_model('adagrad', loss)
    I, D = model._num_items, 16
    new = new_users(I)
    n, H = len(new.user_ids), new.num_users
    nn = model._num_negative_samples if loss == 'adaptive_hinge' else 1
    init = (np.full((H, D), 0.05, np.float32), np.zeros(H, np.float32))
    copy = np.random.RandomState()
    copy.set_state(model._random_state.get_state())
    drawn = model.fold_in(new, n_iter=3, init=init)
    want_neg = np.stack([sample_items(I, (nn, n), random_state=copy) for _ in range(3)])
    got, ref = model._random_state.get_state(), copy.get_state()
    assert (got[1] == ref[1]).all() and got[2] == ref[2]
    given = model.fold_in(new, n_iter=3, init=init, negatives=want_neg)  # the same negatives, handed in: the same bits
    assert same_bits(drawn[0], given[0]) and same_bits(drawn[1], given[1])
    got2 = model._random_state.get_state()
    assert (got2[1] == ref[1]).all() and got2[2] == ref[2]  # negatives given: the stream is left alone
    # init=None: the rows are drawn first (fit()'s distributions), then the negatives
    model.fold_in(new)  # n_iter: the model's (3)
    copy.normal(0, 1.0 / D, (H, D))
    for _ in range(3):
        sample_items(I, (nn, n), random_state=copy)
    got, ref = model._random_state.get_state(), copy.get_state()
    assert (got[1] == ref[1]).all() and got[2] == ref[2]


def check_recommend_vectors():
    import recommend_checks as rc
    model, train = rc.bilinear_model()  # random tables with exact ties
    U, I = model._num_users, model._num_items
    E, _, b, _ = [t.detach().cpu().numpy() for t in model._net.tables()]
    b = b.reshape(-1)
    users = np.concatenate([np.arange(U), [5, 5, 0]])
    lists = [np.unique(train.tocsr()[u].indices) for u in users]
    for k in (1, 10, 128, 200):
        for exclude in (None, lists):
            want = model.recommend(users, k=k, exclude=exclude)
            got = model.recommend_vectors(E[users], b[users], k=k, exclude=exclude)
            assert got[0].dtype == np.int64 and got[1].dtype == np.float32
            assert np.array_equal(got[0], want[0]), ('items', k, exclude is not None)
            assert same_bits(got[1], want[1]), ('scores', k, exclude is not None)
    # a sparse matrix: row r of the matrix hides row r's items
    got = model.recommend_vectors(E[:U], b[:U], k=10, exclude=train)
    want = model.recommend(np.arange(U), k=10, exclude=train)
    assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1])
    one = model.recommend_vectors(E[5], k=3)  # one vector, no bias
    assert one[0].shape == (1, 3) and model.recommend_vectors(np.zeros((0, E.shape[1]), np.float32), k=4)[0].shape == (0, 4)
    for call, err in ((lambda: model.recommend_vectors(E[:2], k=0), ValueError), (lambda: model.recommend_vectors(E[:2, :3]), ValueError),
                      (lambda: model.recommend_vectors(E[:2], b[:3]), ValueError),
                      (lambda: model.recommend_vectors(E[:2], exclude=[[I], []]), IndexError)):
        with pytest.raises(err):
            call()


def check_model_routes_and_refusals():
    import torch
    from spotlight_amd.factorization.explicit import ExplicitFactorizationModel
    from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel
    from spotlight_amd.interactions import Interactions
    I, D = 147, 16
    new = new_users(I)
    H, n = new.num_users, len(new.user_ids)
    rs = np.random.RandomState(4)
    init = (rs.normal(0, 0.25, (H, D)).astype(np.float32), rs.normal(0, 0.1, H).astype(np.float32))
    neg = rs.randint(0, I, (2, 1, n)).astype(np.int64)
    empty = np.nonzero(np.bincount(new.user_ids, minlength=H) == 0)[0]
    # an item BloomEmbedding: the generic route on the materialised table == the generic route of a plain model holding that table
    bloom, _ = trained_like_model('adagrad', 'bpr', item_bloom=True)
    got = bloom.fold_in(new, n_iter=2, init=init, negatives=neg)
    plain, _ = trained_like_model('adagrad', 'bpr')
    with torch.no_grad():
        plain._net.item_embeddings.weight.copy_(bloom._embedding_table('item_embeddings', I))
        plain._net.item_biases.weight.copy_(bloom._net.item_biases.weight)
    want = plain._fold_in_generic(new, n_iter=2, init=init, negatives=neg)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert not same_bits(got[0], init[0]) and same_bits(got[0][empty], init[0][empty])
    rv = bloom.recommend_vectors(got[0], got[1], k=5)
    rv_plain = plain.recommend_vectors(got[0], got[1], k=5)
    assert np.array_equal(rv[0], rv_plain[0]) and same_bits(rv[1], rv_plain[1])
    # any other optimizer_func: the generic route trains with it; a user without a history keeps their row
    rms, _ = trained_like_model('adagrad', 'bpr', optimizer_func=lambda p: torch.optim.RMSprop(p, lr=0.01))
    before = snapshot(rms)
    got = rms.fold_in(new, n_iter=2, init=init, negatives=neg)
    assert np.isfinite(got[0]).all() and not same_bits(got[0], init[0])
    assert same_bits(got[0][empty], init[0][empty]) and same_bits(got[1][empty], init[1][empty])
    for x, y in zip(snapshot(rms), before):
        assert np.array_equal(x, y)
    # bad arguments
    for call, err in ((lambda: plain.fold_in(new, n_iter=0), ValueError),
                      (lambda: plain.fold_in(new, n_iter=2, negatives=neg[:1]), ValueError),
                      (lambda: plain.fold_in(new, n_iter=2, negatives=neg + I), ValueError),
                      (lambda: plain.fold_in(Interactions(np.array([0, 1]), np.array([1, I]), num_users=2, num_items=I + 1)), ValueError),
                      (lambda: plain.fold_in(Interactions(np.array([0, 1]), np.array([1, -1]), num_users=2, num_items=I)), IndexError)):
        with pytest.raises(err):
            call()
    # refusals
    ubloom, _ = trained_like_model('adagrad', 'bpr', user_bloom=True)
    with pytest.raises(TypeError, match='BloomEmbedding'):
        ubloom.fold_in(new)

    class Custom(torch.nn.Module):
        def __init__(self):
            super(Custom, self).__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))

        def forward(self, user_ids, item_ids):
            return self.w[0] + 0.0 * user_ids.float()
    custom, _ = trained_like_model('adagrad', 'bpr')
    custom._representation = Custom()
    custom._initialize(Interactions(np.array([0, 1]), np.array([1, 2]), num_users=61, num_items=I))
    with pytest.raises(TypeError, match='item_embeddings'):
        custom.fold_in(new)
    with pytest.raises(TypeError, match='item_embeddings'):
        custom.recommend_vectors(init[0])
    for cls in (ExplicitFactorizationModel, ShardedImplicitFactorizationModel):
        with pytest.raises(NotImplementedError, match='INTEGRATION.md 2m'):
            cls.fold_in(None, new)
        with pytest.raises(NotImplementedError, match='INTEGRATION.md 2m'):
            cls.recommend_vectors(None, init[0])


def check_fold_in_refused_inside_an_open_fit_scope(engine, stream=0):
    """Item biases shadowed by a training scope: fold_in() and recommend_vectors() are refused as predict() is."""
    model, _ = trained_like_model('adagrad', 'bpr', optimizer_func=lambda p: __import__('torch').optim.Adagrad(p, lr=0.05), sparse=False)
    new = new_users(model._num_items)
    binding = model._bind()
    with engine.bias_shadow(model._slk_tables(), binding.as_struct(), stream=stream):
        with pytest.raises(_native.SlkError, match='shadowed'):
            model.predict(0)
        state = model._random_state.get_state()
        with pytest.raises(_native.SlkError, match='shadowed'):
            model.fold_in(new, n_iter=1)
        with pytest.raises(_native.SlkError, match='shadowed'):
            model._fold_in_generic(new, n_iter=1)  # the generic route is refused too
        after = model._random_state.get_state()
        assert (after[1] == state[1]).all() and after[2] == state[2], 'a refused call consumed the RandomState'
        with pytest.raises(_native.SlkError, match='shadowed'):
            model.recommend_vectors(np.zeros((2, 16), np.float32))
    model.fold_in(new, n_iter=1)
