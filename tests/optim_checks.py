"""ONE optimizer step of the engine (csrc/slk_optim.h: slk_opt_coef_at, slk_opt_hyper_of, slk_opt_step<KIND>) against torch's own
optimizer classes in float64, off the default hyper-parameters -- shared by tests/test_emu_optim.py (emulator build) and
tests/test_gpu_optim.py (the gfx950 library).

The reference (torch_step64) is torch.optim.Adagrad / SparseAdam / Adam / SGD on float64 leaves, state preloaded, `.grad` in the
optimizer's own form.  It is neither the oracle nor a copy of slk_opt_step.  The gradient handed to it is the engine's OWN summed
gradient (read out through ADAM_DENSE with lr = 0, beta1 = 0, as engine_checks.check_single_step_gradients reads it), so the
gradient's error -- pinned elsewhere -- is not part of the comparison: only the roundings of the rule remain.  That the read-out
is bit for bit the gradient the fused kinds see is a check of its own per route (check_readout_is_the_gradient).

THE BOUND (step_error_bound) is derived, not tuned.  u = 2^-24.  A first-order running error is carried through the float64
formulas in the order of slk_opt_step<KIND>'s fp32 operations (class Err): every fp32 operation adds one rounding u * |result|
(`fl`), every coefficient that slk_opt_coef_at / slk_opt_hyper_of cast from double to fp32 enters with u * |coefficient| (`coef`),
and the errors propagate through +, -, *, /, sqrt at the operands' magnitudes -- so the two Adam lerps are charged at
|s1| + |g| + |wd p| and s2 + gv^2, and the step at dD/dm, dD/dv.  The counts stand beside each rule below.  2^-149 per rounding
covers a subnormal result (g * g of a 1e-21 gradient; every route has such elements, and elements whose square is exactly 0).  The assertion is |engine - torch64| <= 2 * bound: one slack factor of 2,
nothing else.  The numpy fp32 restatement of the rules (numpy_step32; only the bound's own sanity check uses it) stays inside the
bound at slack 1 on 2 * 10^5 random elements of the tests' dynamic range, every kind, both hyper-parameter sets
(check_bound_holds_for_fp32_restatement).

fp32 divide and sqrt: spotlight_amd/build.py compiles with -O3 -ffp-contract=off and neither -ffast-math nor
-fno-hip-fp32-correctly-rounded-divide-sqrt nor -fgpu-flush-denormals-to-zero, i.e. hipcc's defaults: correctly rounded
divide and sqrt, subnormals kept (a build that flushed them would miss the bound at the tiny gradients: a flushed g * g is 1e-41
from torch's, the bound there is ~1e-45).  Both are therefore counted as one rounding like every other operation."""
import numpy as np
import torch

import engine_checks as ec
import foldin_checks as fc

U_ROUND = 2.0 ** -24
ETA = 2.0 ** -149     # a rounding whose result is subnormal
SLACK = 2.0

KINDS = ('adagrad', 'sparse_adam', 'adam_dense', 'adagrad_dense', 'sgd')
SPARSE_KINDS = ('adagrad', 'sparse_adam', 'sgd')
STEP0S = (0, 1, 999, 2 ** 31 + 5)  # the last: slk_optim.step is an int64, pow(beta, step) underflows to bc = 1
DEFAULT_LR = 1e-2  # _native.make_optim's
WHICH = ('default', 'off')
# (route, dim): the launch path at the four row layouts of foldin_checks.DS, every other route at 24
ROUTES = [('launch', D) for D in fc.DS] + [(name, 24) for name in ('epoch', 'pingpong', 'explicit', 'poolnet', 'foldin')]
ROUTE_KINDS = [(name, D, kind) for name, D in ROUTES for kind in (SPARSE_KINDS if name == 'pingpong' else KINDS)]


def hyper(kind, which):
    """'default': what _native.make_optim fills in.  'off': every hyper-parameter the kind reads, away from its default."""
    if which == 'default':
        return dict(lr=DEFAULT_LR)
    hp = dict(lr=0.03)
    if kind != 'sgd':
        hp['eps'] = 1e-3
    if kind in ('sparse_adam', 'adam_dense'):
        hp['betas'] = (0.5, 0.9)
    if kind.endswith('dense'):
        hp['weight_decay'] = 0.1
    if kind.startswith('adagrad'):
        hp['lr_decay'] = 0.1
    return hp


def resolved(kind, hp):
    eps = hp.get('eps')
    if eps is None:
        eps = 1e-10 if kind.startswith('adagrad') else 1e-8
    return dict(lr=float(hp.get('lr', DEFAULT_LR)), eps=float(eps), betas=tuple(hp.get('betas', (0.9, 0.999))),
                weight_decay=float(hp.get('weight_decay', 0.0)), lr_decay=float(hp.get('lr_decay', 0.0)))


# ---- the reference: torch's optimizer classes, float64 ------------------------------------------------------------------------------
def torch_step64(kind, hp, p, s1, s2, step0, g, touched):
    """One .step() of the real torch optimizer on float64 leaves built from the fp32 pre-step values.  `g`: the summed gradient
    (any float dtype, p's shape); `touched`: the rows of the minibatch (the sparse kinds' .grad is a sparse_coo_tensor over exactly
    those rows, all-zero rows included).  Returns float64 (p', s1', s2')."""
    h = resolved(kind, hp)
    t64 = lambda x: torch.from_numpy(np.array(x, dtype=np.float64, copy=True))
    P = t64(p).requires_grad_(True)
    G = t64(g)
    step_t = torch.tensor(float(step0), dtype=torch.float64)
    if kind in ('adagrad', 'adagrad_dense'):
        opt = torch.optim.Adagrad([P], lr=h['lr'], lr_decay=h['lr_decay'], eps=h['eps'], weight_decay=h['weight_decay'], foreach=False)
        opt.state[P] = {'step': step_t, 'sum': t64(s1)}
    elif kind == 'sparse_adam':
        opt = torch.optim.SparseAdam([P], lr=h['lr'], betas=h['betas'], eps=h['eps'])
        opt.state[P] = {'step': int(step0), 'exp_avg': t64(s1), 'exp_avg_sq': t64(s2)}
    elif kind == 'adam_dense':
        opt = torch.optim.Adam([P], lr=h['lr'], betas=h['betas'], eps=h['eps'], weight_decay=h['weight_decay'], foreach=False)
        opt.state[P] = {'step': step_t, 'exp_avg': t64(s1), 'exp_avg_sq': t64(s2)}
    elif kind == 'sgd':
        opt = torch.optim.SGD([P], lr=h['lr'], foreach=False)
    else:
        raise ValueError(kind)
    if kind in SPARSE_KINDS:
        rows = torch.from_numpy(np.asarray(touched, dtype=np.int64))
        P.grad = torch.sparse_coo_tensor(rows.reshape(1, -1), G[rows], size=tuple(P.shape))
    else:
        P.grad = G
    opt.step()
    st = opt.state[P] if kind != 'sgd' else {}
    out1 = st.get('sum', st.get('exp_avg'))
    out2 = st.get('exp_avg_sq')
    as_np = lambda x: None if x is None else x.detach().numpy().copy()
    return as_np(P), as_np(out1), as_np(out2)


# ---- the bound: a first-order running error through the rule's fp32 operations ----------------------------------------------------------
class Err(object):
    """A float64 value `v` and a bound `e` on how far its fp32 counterpart in the engine may be from it."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)

    def __add__(self, o):
        return Err(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return Err(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return Err(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        with np.errstate(divide='ignore', invalid='ignore'):
            return Err(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def sqrt(self):
        # the farther end of [sqrt(v - e), sqrt(v + e)] from sqrt(v): e / (2 sqrt v) to first order, finite at v = 0
        r = np.sqrt(self.v)
        return Err(r, np.maximum(np.sqrt(self.v + self.e) - r, r - np.sqrt(np.maximum(self.v - self.e, 0.0))))


def fl(x):
    """One fp32 rounding of the engine."""
    return Err(x.v, x.e + U_ROUND * np.abs(x.v) + ETA)


def coef(c):
    """A double of slk_optim that slk_opt_coef_at / slk_opt_hyper_of cast to fp32 (torch keeps the double)."""
    return Err(c, U_ROUND * abs(c))


def coefficients(kind, hp, step_no):
    """slk_opt_coef_at's doubles, as torch forms them: (c0, c1)."""
    h = resolved(kind, hp)
    if kind == 'sgd':
        return h['lr'], 0.0
    if kind.startswith('adagrad'):
        return h['lr'] / (1.0 + (step_no - 1.0) * h['lr_decay']), 0.0
    bc1, bc2 = 1.0 - h['betas'][0] ** float(step_no), 1.0 - h['betas'][1] ** float(step_no)
    if kind == 'sparse_adam':
        return h['lr'] * np.sqrt(bc2) / bc1, 0.0
    return h['lr'] / bc1, np.sqrt(bc2)


def step_error_bound(kind, hp, step_no, p, s1, s2, g):
    """(ep, es1, es2) per element, BEFORE the slack factor: the roundings of slk_opt_step<KIND> carried to first order."""
    h = resolved(kind, hp)
    c0v, c1v = coefficients(kind, hp, step_no)
    P, G = Err(p), Err(g)
    S1 = Err(s1) if s1 is not None else None
    S2 = Err(s2) if s2 is not None else None
    c0, eps, wd = coef(c0v), coef(h['eps']), coef(h['weight_decay'])
    zero = np.zeros(P.v.shape)
    if kind == 'sgd':
        # p += -c0 * g                                              2 roundings, 1 coefficient (c0)
        return fl(P - fl(c0 * G)).e, zero, zero
    if kind == 'adagrad':
        # s1 += g * g                                               2 roundings
        # p += -c0 * (g / (sqrtf(s1) + eps))                        5 roundings, 2 coefficients (c0, eps)
        s = fl(S1 + fl(G * G))
        return fl(P - fl(c0 * fl(G / fl(fl(s.sqrt()) + eps)))).e, s.e, zero
    if kind == 'adagrad_dense':
        # gv = g + wd * p                                           2 roundings, 1 coefficient (wd)
        # s = s1 + gv * gv                                          2 roundings
        # p += -c0 * (gv / (sqrtf(s) + eps))                        5 roundings, 2 coefficients (c0, eps)
        gv = fl(G + fl(wd * P))
        s = fl(S1 + fl(gv * gv))
        return fl(P - fl(c0 * fl(gv / fl(fl(s.sqrt()) + eps)))).e, s.e, zero
    omb1, omb2, beta2 = coef(1.0 - h['betas'][0]), coef(1.0 - h['betas'][1]), coef(h['betas'][1])
    if kind == 'sparse_adam':
        # mu = (g - s1) * omb1; s1 = mu + s1                        3 roundings, 1 coefficient (omb1)
        # vu = (g * g - s2) * omb2; s2 = vu + s2                    4 roundings, 1 coefficient (omb2)
        # p += -c0 * (s1 / (sqrtf(s2) + eps))                       5 roundings, 2 coefficients (c0, eps)
        m = fl(fl(fl(G - S1) * omb1) + S1)
        v = fl(fl(fl(fl(G * G) - S2) * omb2) + S2)
        return fl(P - fl(c0 * fl(m / fl(fl(v.sqrt()) + eps)))).e, m.e, v.e
    assert kind == 'adam_dense'
    # gv = g + wd * p                                               2 roundings, 1 coefficient (wd)
    # m = s1 + omb1 * (gv - s1)                                     3 roundings, 1 coefficient (omb1)
    # v = s2 * beta2 + omb2 * (gv * gv)                             4 roundings, 2 coefficients (beta2, omb2)
    # p += -c0 * (m / (sqrtf(v) / c1 + eps))                        6 roundings, 3 coefficients (c0, c1, eps)
    gv = fl(G + fl(wd * P))
    m = fl(S1 + fl(omb1 * fl(gv - S1)))
    v = fl(fl(S2 * beta2) + fl(omb2 * fl(gv * gv)))
    return fl(P - fl(c0 * fl(m / fl(fl(fl(v.sqrt()) / coef(c1v)) + eps)))).e, m.e, v.e


def numpy_step32(kind, hp, step_no, p, s1, s2, g):
    """The rules in numpy fp32, one rounding per operation -- used ONLY to check that the bound is wide enough for a faithful fp32
    implementation (check_bound_holds_for_fp32_restatement), never as a reference for the engine."""
    f = np.float32
    h = resolved(kind, hp)
    c0, c1 = [f(x) for x in coefficients(kind, hp, step_no)]
    eps, wd = f(h['eps']), f(h['weight_decay'])
    omb1, omb2, beta2 = f(1.0 - h['betas'][0]), f(1.0 - h['betas'][1]), f(h['betas'][1])
    p, g = np.asarray(p, f), np.asarray(g, f)
    if kind == 'sgd':
        return p + -c0 * g, None, None
    if kind == 'adagrad':
        s = s1 + g * g
        return p + -c0 * (g / (np.sqrt(s) + eps)), s, None
    if kind == 'adagrad_dense':
        gv = g + wd * p
        s = s1 + gv * gv
        return p + -c0 * (gv / (np.sqrt(s) + eps)), s, None
    if kind == 'sparse_adam':
        m = (g - s1) * omb1 + s1
        v = (g * g - s2) * omb2 + s2
        return p + -c0 * (m / (np.sqrt(v) + eps)), m, v
    gv = g + wd * p
    m = s1 + omb1 * (gv - s1)
    v = s2 * beta2 + omb2 * (gv * gv)
    return p + -c0 * (m / (np.sqrt(v) / c1 + eps)), m, v


def compare_with_torch(kind, hp, step0, pre, got, g, touched, what, slack=SLACK):
    """`pre`, `got`: (p, s1, s2) fp32 before / after the step.  Every element of the rows torch updates within slack * bound of
    torch's float64 step; under the row-sparse kinds every other row bit-unchanged.  Returns the largest error / bound."""
    sparse = kind in SPARSE_KINDS
    has1, has2 = kind != 'sgd', kind in ('sparse_adam', 'adam_dense')
    p, s1, s2 = [np.asarray(x, np.float32) for x in pre]
    want = torch_step64(kind, hp, p, s1 if has1 else None, s2 if has2 else None, step0, g, touched)
    bound = step_error_bound(kind, hp, step0 + 1, p, s1 if has1 else None, s2 if has2 else None, np.asarray(g, np.float64))
    rows = np.zeros(p.shape[0], dtype=bool)
    rows[np.asarray(touched, dtype=np.int64)] = True
    worst = 0.0
    for nm, have, a, b, w, e in (('param', True, pre[0], got[0], want[0], bound[0]), ('state1', has1, pre[1], got[1], want[1], bound[1]),
                                 ('state2', has2, pre[2], got[2], want[2], bound[2])):
        if not have:
            continue
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        assert np.isfinite(b).all(), (what, nm, 'not finite')
        if sparse:
            assert fc.same_bits(a[~rows], b[~rows]), (what, nm, 'a row outside the minibatch changed')
        sel = rows if sparse else np.ones_like(rows)
        d = np.abs(b.astype(np.float64) - w)[sel]
        ratio = float((d / e[sel]).max()) if d.size else 0.0
        assert ratio <= slack, (what, nm, 'error / bound', ratio, 'worst element', int(np.argmax(d / e[sel])))
        worst = max(worst, ratio)
    return worst


RATIOS = {}  # (backend class, kind) -> the largest error / bound seen (DESIGN.md section 5 records them)


def note_ratio(be, kind, ratio):
    key = (type(be).__name__, kind)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print('OPTIM_RATIO %s %s %.4f' % (key[0], kind, ratio))


# ---- pre-state ----------------------------------------------------------------------------------------------------------------------------
def make_state(kind, g, seed):
    """Optimizer state of one table before the step, by row (row r is of class r % 4):
       0  s1 = s2 = 0: a first step;
       1  moments 1e4 times the gradient (Adam: m = 1e4 g, v = 1e8 g^2; Adagrad: sum = 1e8 g^2): the cancellation of the lerps;
       2, 3  accumulators spread over six decades, independent of the gradient."""
    rs = np.random.RandomState(seed)
    g = np.asarray(g, np.float64)
    cls = (np.arange(g.shape[0]) % 4).reshape((-1,) + (1,) * (g.ndim - 1))
    v = 10.0 ** rs.uniform(-10.0, -4.0, g.shape)
    m = rs.choice([-1.0, 1.0], g.shape) * 10.0 ** rs.uniform(-6.0, 0.0, g.shape) * 1e-2
    if kind.startswith('adagrad'):
        s1, s2 = v, np.zeros(g.shape)
        s1 = np.where(cls == 1, 1e8 * g * g, s1)
    else:
        s1, s2 = np.where(cls == 1, 1e4 * g, m), np.where(cls == 1, 1e8 * g * g, v)
    s1, s2 = np.where(cls == 0, 0.0, s1), np.where(cls == 0, 0.0, s2)
    return s1.astype(np.float32), s2.astype(np.float32)


def put(be, buf, a):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(tuple(buf.shape))
    if isinstance(buf, np.ndarray):
        buf[...] = a
    else:
        buf.copy_(torch.from_numpy(a))


READOUT_HP = dict(lr=0.0, betas=(0.0, 0.999), weight_decay=0.0)  # ADAM_DENSE, from zero state: exp_avg' = 0 + 1 * (g - 0) = g


# ---- routes -------------------------------------------------------------------------------------------------------------------------------
TINY_SUBNORMAL, TINY_ZERO = 1e-18, 1e-22  # embeddings scaled so that a gradient's fp32 square is subnormal / exactly zero


def start(be, dev, n, state, step0):
    """Pre-state and step count into a backend model of n tables."""
    for t in range(n if state is not None else 0):
        put(be, dev.s1[t], state[t][0])
        put(be, dev.s2[t], state[t][1])
    dev.optim.step = step0


def finish(be, dev, n, step0):
    assert dev.optim.step == step0 + 1
    return [[be.get(x[t]).copy() for x in (dev.p, dev.s1, dev.s2)] for t in range(n)]


class BilinearRoute(object):
    """One call over ONE minibatch of 64 with repeated ids, U = 37, I = 53.
    `how`: 'launch' (slk_bilinear_train, epoch_kernel = 0), 'epoch' (the persistent kernel, its four gates opened), 'pingpong'
    (inside the user-row ping-pong scope) or 'explicit' (slk_bilinear_train_explicit, regression against ratings, no negatives).
      items 0-2    embeddings scaled by 1e-18: the gradients of users 0-1, who see only these, are ~1e-21, g * g is SUBNORMAL;
      items 3-5    embeddings scaled by 1e-22: the gradients of users 2-3 are ~1e-25 and g * g is exactly 0 in fp32;
      items 12-16, users 7-10   never in the minibatch.
    The three implicit routes use the hinge loss, so that some rows are TOUCHED WITH AN EXACTLY ZERO GRADIENT (the margin holds):
      items 6-8    bias +4, the positives of users 4-6;  items 9-11  bias -4, their negatives."""
    U, I, B = 37, 53, 64
    tables = 4
    tiny_table = 0

    def __init__(self, how, D):
        self.how, self.D = how, D
        explicit = how == 'explicit'
        self.loss = 'regression' if explicit else 'hinge'
        self.name = 'bilinear/%s/D%d' % (how, D)
        rs = np.random.RandomState(100 + D)
        sc = min(0.3, 1.0 / np.sqrt(D))
        P, Q = rs.normal(0, sc, (self.U, D)), rs.normal(0, sc, (self.I, D))
        bu, bi = rs.normal(0, 0.1, self.U), rs.normal(0, 0.1, self.I)
        Q[0:3] *= TINY_SUBNORMAL
        Q[3:6] *= TINY_ZERO
        bi[6:9] += 4.0
        bi[9:12] -= 4.0
        self.params = [x.astype(np.float32) for x in (P, Q, bu, bi)]
        # (every row of the two margin groups occurs: twice, so that the ids repeat)
        users = np.concatenate([rs.randint(0, 2, 4), rs.randint(2, 4, 4), np.repeat(np.arange(4, 7), 2), rs.randint(11, self.U, 50)])
        items = np.concatenate([rs.randint(0, 3, 4), rs.randint(3, 6, 4), np.tile(np.arange(6, 9), 2), rs.randint(17, self.I, 50)])
        negs = np.concatenate([rs.randint(0, 3, 4), rs.randint(3, 6, 4), np.tile(np.arange(9, 12), 2), rs.randint(17, self.I, 50)])
        perm = rs.permutation(self.B)
        self.users, self.items, self.negs = [x[perm].astype(np.int64) for x in (users, items, negs)]
        self.ratings = ec._ratings_for(np.random.RandomState(7), 'regression', self.B) if explicit else None
        tu = np.unique(self.users)
        ti = np.unique(self.items if explicit else np.concatenate([self.items, self.negs]))
        self.touched = [tu, ti, tu, ti]
        self.zero_rows = None if explicit else [np.arange(4, 7), np.arange(6, 12), tu, np.arange(6, 12)]

    def call(self, be, kind, hp, step0=0, state=None, how=None):
        how = how or self.how
        eng = be.engine
        dev = be.model(self.params, opt=kind, **hp)
        start(be, dev, 4, state, step0)
        d_u, d_i = be.alloc(self.users), be.alloc(self.items)
        mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
        opts = dict(epoch_kernel=0)
        if how == 'epoch':
            opts = dict(epoch_kernel=1, epoch_max_batch=1 << 20, epoch_adaptive_max_batch=1 << 20, epoch_dense_elems=1 << 40)
        with eng.options(**opts):
            n0 = eng.get_stat('pingpong_calls')
            eng.profile_reset()
            eng.profile_enable(True)
            if how == 'explicit':
                d_r = be.alloc(self.ratings)
                eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), be.ptr(d_r), self.B, self.B, self.loss,
                                            be.ptr(mb_loss), stream=be.stream)
            else:
                d_n = be.alloc(self.negs)
                with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream, enabled=how == 'pingpong'):
                    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), self.B, self.B, self.loss, 1, be.ptr(mb_loss),
                                       d_neg_in=be.ptr(d_n), stream=be.stream)
            eng.profile_enable(False)
            prof = eng.profile_read()
        # the route under test really ran
        if how == 'epoch':
            assert prof['epoch'][0] == 1 and prof['user_pass'][0] == 0, prof
        else:
            assert prof['epoch'][0] == 0 and prof['user_pass'][0] == 1, prof
        assert (eng.get_stat('pingpong_calls') - n0) == (1 if how == 'pingpong' else 0)
        return finish(be, dev, 4, step0)

    def readout(self, be):  # (the ping-pong scope takes no dense kind: its read-out is the launch path's, and the SGD check holds it to it)
        return [r[1] for r in self.call(be, 'adam_dense', READOUT_HP, how='explicit' if self.how == 'explicit' else 'launch')]


class PoolNetRoute(object):
    """slk_poolnet_train: I = 31, ONE minibatch of 16 left-padded sequences of L = 9, hinge loss.  Ids 25-30 never occur; the
    padding row 0 receives no gradient and is not a row of the minibatch.  Embedding COLUMNS 0-1 are scaled by 1e-18 and columns
    2-3 by 1e-22: a row's gradient in a column is a sum of dL/dscore times other rows' values in that column, so every row's
    gradient there has a subnormal, respectively an exactly zero, fp32 square."""
    I, N, L = 31, 16, 9
    tables = 2
    tiny_table = 0

    def __init__(self, D):
        self.D, self.loss = D, 'hinge'
        self.name = 'poolnet/D%d' % D
        rs = np.random.RandomState(300 + D)
        self.seqs = ec.make_sequences(rs, self.N, self.L, 25)
        self.negs = rs.randint(1, 25, self.N * self.L).astype(np.int64)
        self.params = ec._seq_params(rs, self.I, D)
        self.params[0][:, 0:2] *= np.float32(TINY_SUBNORMAL)
        self.params[0][:, 2:4] *= np.float32(TINY_ZERO)
        ids = np.unique(np.concatenate([self.seqs.ravel(), self.negs]))
        ids = ids[ids != 0]
        self.touched = [ids, ids]
        self.zero_rows = None

    def call(self, be, kind, hp, step0=0, state=None, how=None):
        eng = be.engine
        dev = be.seq_model(self.params, opt=kind, **hp)
        start(be, dev, 2, state, step0)
        d_seqs, d_negs = be.alloc(self.seqs), be.alloc(self.negs)
        mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
        eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), self.N, self.L, self.N, self.loss, 1, be.ptr(mb_loss),
                          d_neg_in=be.ptr(d_negs), stream=be.stream)
        return finish(be, dev, 2, step0)

    def readout(self, be):
        return [r[1] for r in self.call(be, 'adam_dense', READOUT_HP)]


class FoldinRoute(object):
    """slk_bilinear_foldin, ONE step for 5 new users with histories of 37, 3, 9, 300 and 1 interactions (the default crossover:
    the wave route and the workgroup route in one call) against 53 frozen items, pointwise loss.  The two trained tables are the
    new users' rows and biases.  Columns 0-1 / 2-3 of the item embeddings are scaled by 1e-18 / 1e-22: the new rows' gradients in
    those columns have a subnormal / an exactly zero fp32 square."""
    tables = 2
    tiny_table = 0

    def __init__(self, D):
        self.D = D
        self.name = 'foldin/D%d' % D
        self.pr = fc.Problem(D, 53, 5, 'pointwise', 1, seed=3, lengths=[37, 3, 9, 300, 1])
        self.pr.V[:, 0:2] *= np.float32(TINY_SUBNORMAL)
        self.pr.V[:, 2:4] *= np.float32(TINY_ZERO)
        self.params = [self.pr.U, self.pr.b]
        self.touched = [np.arange(5), np.arange(5)]
        self.zero_rows = None

    def call(self, be, kind, hp, step0=0, state=None, how=None):
        st = None
        if state is not None:
            st = (state[0][0], state[1][0], state[0][1], state[1][1])
        fold = fc.Fold(be, self.pr, kind, state=st, step=step0, hp=hp)
        fold.run(1, want_loss=False)
        assert fold.optim.step == step0 + 1
        r = fold.result()
        return [[r[0], r[2], r[4]], [r[1], r[3], r[5]]]

    def readout(self, be):
        return [r[1] for r in self.call(be, 'adam_dense', READOUT_HP)]


_ROUTES = {}


def route(name, D=24):
    """The problems are built once per process; the engine's gradient of each once per backend (gradient_of)."""
    key = (name, D)
    if key not in _ROUTES:
        _ROUTES[key] = PoolNetRoute(D) if name == 'poolnet' else FoldinRoute(D) if name == 'foldin' else BilinearRoute(name, D)
    return _ROUTES[key]


def gradient_of(be, rt):
    cache = be.__dict__.setdefault('_optim_gradients', {})
    if rt.name not in cache:
        g = rt.readout(be)
        for x in g:
            x.setflags(write=False)
        cache[rt.name] = g
    return cache[rt.name]


# ---- the checks -----------------------------------------------------------------------------------------------------------------------------
def check_readout_is_the_gradient(be, rt):
    """The precondition of every comparison below: SGD with lr = 1 from the same tables (and negatives) ends at fl(p - g), bit for
    bit, in every element of every table -- so the ADAM_DENSE read-out IS the gradient the fused kinds of this route apply."""
    g = gradient_of(be, rt)
    got = rt.call(be, 'sgd', dict(lr=1.0))
    for t in range(rt.tables):
        p = np.asarray(rt.params[t], np.float32).reshape(g[t].shape)
        assert fc.same_bits(got[t][0].reshape(g[t].shape), p - g[t]), (rt.name, 'table', t)
        if t == 0:
            assert np.abs(g[t]).max() > 0, 'nothing was trained'
    # the tiny gradients are there: non-zero elements whose fp32 square is subnormal, and non-zero elements whose square is 0
    gt = g[rt.tiny_table].astype(np.float32)
    sq = gt * gt
    assert ((gt != 0) & (sq > 0) & (sq < np.float32(2.0 ** -126))).any(), (rt.name, 'no gradient with a subnormal square')
    assert ((gt != 0) & (sq == 0)).any(), (rt.name, 'no non-zero gradient whose square underflows to zero')
    if rt.zero_rows is not None:  # the rows built to be touched with a zero gradient are
        for t in range(rt.tables):
            assert (g[t][rt.zero_rows[t]] == 0).all(), (rt.name, 'table', t, 'a margin row has a gradient')
            assert np.isin(rt.zero_rows[t], rt.touched[t]).all(), (rt.name, 'table', t, 'a margin row is not in the minibatch')


def check_rule_against_torch(be, rt, kind, which, step0):
    """One step of `kind` on route `rt` from the pre-state of make_state, every table against torch_step64 within the derived
    bound; rows outside the minibatch bit-unchanged under the row-sparse kinds; a row touched with a zero gradient moves under
    SparseAdam (torch decays its moments) and is bit-unchanged under Adagrad / SGD (as in torch: sum += 0, p -= 0)."""
    hp = hyper(kind, which)
    g = gradient_of(be, rt)
    state = [make_state(kind, g[t], seed=17 + t) for t in range(rt.tables)]
    got = rt.call(be, kind, hp, step0=step0, state=state)
    worst = 0.0
    for t in range(rt.tables):
        shape = g[t].shape
        pre = (np.asarray(rt.params[t], np.float32).reshape(shape), state[t][0], state[t][1])
        post = [x.reshape(shape) for x in got[t]]
        what = (rt.name, kind, which, 'step0', step0, 'table', t)
        worst = max(worst, compare_with_torch(kind, hp, step0, pre, post, g[t], rt.touched[t], what))
        if rt.zero_rows is not None and kind in SPARSE_KINDS:
            z = rt.zero_rows[t]
            if kind == 'sparse_adam':
                live = z[(z % 4) >= 2]  # (rows of class 0 and 1 have zero moments here: nothing to decay)
                assert live.size and not fc.same_bits(post[1][live], pre[1][live]), (what, 'SparseAdam did not decay a zero-gradient row')
                assert not fc.same_bits(post[0][live], pre[0][live]), (what, 'SparseAdam did not move a zero-gradient row')
            else:
                assert fc.same_bits(post[0][z], pre[0][z]) and (kind == 'sgd' or fc.same_bits(post[1][z], pre[1][z])), \
                    (what, 'a zero gradient is not a no-op')
    note_ratio(be, kind, worst)
    return worst


def check_bound_holds_for_fp32_restatement(kind, which, n=200000, seed=1):
    """The bound is wide enough: the numpy fp32 restatement of the rule stays inside it at slack ONE against torch float64, on
    2 * 10^5 random elements of the dynamic range the engine tests use, at every step0."""
    rs = np.random.RandomState(seed)
    hp = hyper(kind, which)
    p = (rs.normal(0, 0.3, n) * 10.0 ** rs.uniform(-3, 0, n)).astype(np.float32)
    g = (rs.normal(0, 1.0, n) * 10.0 ** rs.uniform(-18, -1, n)).astype(np.float32)
    g[rs.rand(n) < 0.02] = 0.0
    s1, s2 = make_state(kind, g, seed + 1)
    worst = 0.0
    for step0 in STEP0S:
        want = torch_step64(kind, hp, p, s1, s2, step0, g, np.arange(n))
        have = numpy_step32(kind, hp, step0 + 1, p, s1, s2, g)
        bound = step_error_bound(kind, hp, step0 + 1, p, s1, s2, g.astype(np.float64))
        for k in range(3):
            if have[k] is None:
                continue
            ratio = float((np.abs(have[k].astype(np.float64) - want[k]) / bound[k]).max())
            assert ratio <= 1.0, (kind, which, step0, ('param', 'state1', 'state2')[k], ratio)
            worst = max(worst, ratio)
    return worst


def check_bound_is_tight_enough(kind):
    """... and narrow enough to see a wrong hyper-parameter: the fp32 restatement run with the DEFAULT eps (or beta2, lr_decay,
    weight_decay) against torch at the 'off' set is outside slack * bound."""
    rs = np.random.RandomState(5)
    n = 20000
    hp = hyper(kind, 'off')
    p = rs.normal(0, 0.3, n).astype(np.float32)
    g = (rs.normal(0, 1.0, n) * 10.0 ** rs.uniform(-5, -1, n)).astype(np.float32)
    s1, s2 = make_state(kind, g, 6)
    step0 = 999
    want = torch_step64(kind, hp, p, s1, s2, step0, g, np.arange(n))
    bound = step_error_bound(kind, hp, step0 + 1, p, s1, s2, g.astype(np.float64))
    for key in hp:
        if key == 'lr':
            continue
        wrong = dict(hp)
        del wrong[key]
        have = numpy_step32(kind, wrong, step0 + 1, p, s1, s2, g)
        ratio = max(float((np.abs(have[k].astype(np.float64) - want[k]) / bound[k]).max()) for k in range(3) if have[k] is not None)
        assert ratio > 10 * SLACK, (kind, key, 'a default in place of the set value passes the bound', ratio)


# ---- multi-step closed loop -----------------------------------------------------------------------------------------------------------------
def check_closed_loop_against_torch(be, kind, which, D=24, U=37, I=53, N=200, B=64, loss='bpr', step0=999, seed=5):
    """N = 200, B = 64: four minibatches.  Each step is a single-minibatch call checked as in check_rule_against_torch (its
    gradient read out from the tables that step starts from); ONE call over all four minibatches must end bit-identical to the
    four calls, on the launch path and on the persistent kernel (whose per-minibatch coefficient table hc[m] is what differs
    between the four steps under lr_decay and the bias corrections)."""
    eng = be.engine
    hp = hyper(kind, which)
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    negs = rs.randint(0, I, N).astype(np.int64)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    params = [x.astype(np.float32) for x in params]
    state0 = [make_state(kind, 1e-3 * params[t], seed=23 + t) for t in range(4)]  # (class 1 rows: moments of a plausible gradient size)
    n_mb = (N + B - 1) // B

    def fresh(opt, hp_, tabs, state, step):
        dev = be.model(tabs, opt=opt, **hp_)
        for t in range(4):
            put(be, dev.s1[t], state[t][0])
            put(be, dev.s2[t], state[t][1])
        dev.optim.step = step
        return dev

    def train(dev, lo, hi):
        d_u, d_i, d_n = be.alloc(users[lo:hi]), be.alloc(items[lo:hi]), be.alloc(negs[lo:hi])
        mb_loss = be.alloc(np.zeros((hi - lo + B - 1) // B, dtype=np.float32))
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), hi - lo, B, loss, 1, be.ptr(mb_loss),
                           d_neg_in=be.ptr(d_n), stream=be.stream)

    read = lambda dev: [[be.get(x[t]).copy() for x in (dev.p, dev.s1, dev.s2)] for t in range(4)]
    launch = dict(epoch_kernel=0)
    persistent = dict(epoch_kernel=1, epoch_max_batch=1 << 20, epoch_adaptive_max_batch=1 << 20, epoch_dense_elems=1 << 40)
    zeros = [(np.zeros_like(x), np.zeros_like(x)) for x in params]
    worst = 0.0
    with eng.options(**launch):
        dev = fresh(kind, hp, params, state0, step0)
        for m in range(n_mb):
            lo, hi = m * B, min((m + 1) * B, N)
            pre = read(dev)
            gdev = fresh('adam_dense', READOUT_HP, [pre[t][0] for t in range(4)], zeros, 0)
            train(gdev, lo, hi)
            g = [be.get(gdev.s1[t]).copy() for t in range(4)]
            train(dev, lo, hi)
            assert dev.optim.step == step0 + m + 1
            post = read(dev)
            tu, ti = np.unique(users[lo:hi]), np.unique(np.concatenate([items[lo:hi], negs[lo:hi]]))
            for t, touched in enumerate((tu, ti, tu, ti)):
                what = ('closed loop', kind, which, 'minibatch', m, 'table', t)
                worst = max(worst, compare_with_torch(kind, hp, step0 + m, pre[t], post[t], g[t].reshape(pre[t][0].shape), touched, what))
        stepwise = read(dev)
    note_ratio(be, kind, worst)
    for name, opts in (('launch path', launch), ('persistent kernel', persistent)):
        with eng.options(**opts):
            dev = fresh(kind, hp, params, state0, step0)
            eng.profile_reset()
            eng.profile_enable(True)
            train(dev, 0, N)
            eng.profile_enable(False)
            prof = eng.profile_read()
            assert (prof['epoch'][0] >= 1 and prof['user_pass'][0] == 0) if opts is persistent else \
                (prof['epoch'][0] == 0 and prof['user_pass'][0] == n_mb), prof
            assert dev.optim.step == step0 + n_mb
            whole = read(dev)
        for t in range(4):
            for k in range(3):
                assert fc.same_bits(whole[t][k], stepwise[t][k]), ('one call over %d minibatches on the %s differs from %d calls'
                                                                   % (n_mb, name, n_mb), kind, which, 'table', t, ('param', 'state1', 'state2')[k])
    return worst


def check_routes_agree_off_the_defaults(be, what, kind):
    """The bit-for-bit route checks of engine_checks at the 'off' hyper-parameters, 999 steps in, at the smallest shapes the
    suite already runs them at.  'epoch': 300 interactions in minibatches of 64 are FIVE minibatches in one chunk -- with
    lr_decay (and bias corrections still moving) every entry hc[m] of the persistent kernel's coefficient table is another number."""
    hp = hyper(kind, 'off')
    if what == 'epoch':
        ec.check_epoch_kernel_is_bit_identical(be, 'bpr', kind, 8, U=40, I=30, N=300, B=64, hp=hp, step0=999)
    elif what == 'chunking':
        ec.check_chunking_is_bit_neutral(be, 'bpr', kind, 8, U=40, I=30, N=500, B=32, chunk=100, hp=hp, step0=999)
    else:
        ec.check_user_pingpong_is_bit_neutral(be, 'bpr', kind, 16, U=400, I=300, N=3000, B=512, hp=hp, step0=999)


def check_foldin_steps_compose_off_the_defaults(be, kind, D=24, T=3, step0=999):
    """slk_bilinear_foldin has a per-step coefficient table of its own (c[t], at step + t + 1).  T steps in ONE call must end bit
    for bit where T one-step calls end -- whose single step (c[0]) check_rule_against_torch holds to torch at every step0 --, at the
    'off' hyper-parameters 999 steps in: with lr_decay every c[t] is another number."""
    hp = hyper(kind, 'off')
    pr = fc.Problem(D, 53, 5, 'pointwise', T, seed=4, lengths=[37, 3, 9, 300, 1])
    state = [make_state(kind, 1e-3 * x, seed=31 + k) for k, x in enumerate((pr.U, pr.b))]
    st = (state[0][0], state[1][0], state[0][1], state[1][1])
    whole = fc.Fold(be, pr, kind, state=st, step=step0, hp=hp)
    whole.run(T, want_loss=False)
    steps = fc.Fold(be, pr, kind, state=st, step=step0, hp=hp)
    for t in range(T):
        steps.run(1, t0=t, want_loss=False)
    assert whole.optim.step == steps.optim.step == step0 + T
    for k, (a, b) in enumerate(zip(whole.result(), steps.result())):
        assert fc.same_bits(a, b), ('one fold-in call of %d steps differs from %d calls' % (T, T), kind, k)
    assert not fc.same_bits(whole.result()[0], pr.U), 'nothing was trained'
