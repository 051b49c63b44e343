"""The multi-negative losses (softmax, adaptive hinge, warp) at wide n, with EXACT scores and dL/dscore read pair by pair --
backend-agnostic checks, run on the emulator build by tests/test_emu_wide_negatives.py and on the gfx950 library by
tests/test_gpu_wide_negatives.py.  softmax_checks / warp_checks / engine_checks compare with a reference at n <= 5 (one closed
loop at n = 130); their bounds scale with the tensor, and at n = 1024 one dropped pair (1 / ((n + 1) B)) is of the order of the
bound.  Here every pair's gradient is read on its own.

THE INPUTS (make_case).
  dyadic tables   every entry of U and V is a multiple of 1/4 with |u|, |v| <= 1 (softmax's planted rows: +-32), all four bias
                  tables start at 0.  Every product is a multiple of 1/16 and every partial sum far below 2^20, so a score is exact
                  in float32 under ANY summation order: the test knows sk to the bit without assuming how k_score_pass reduces.
                  assert_scores_exact checks it on the case's own tables -- engine_checks.f32_chain_dot, a float32 sum in reversed
                  order and the float64 product agree exactly.
  once            negatives are handed in (d_neg_in); the N (1 + n) items of a call are distinct (a permutation of a catalogue of
                  I = N (1 + n) + 1 items) and so are its N users (of N + 2).
  SGD, lr = 1     confirmed in csrc/slk_optim.h: c0 = (float)lr = 1.0f and the rule is p += -c0 * g (slk_opt_step<SLK_OPT_SGD>, no
                  state, no weight decay), with g the item pass's sum over the item's occurrences -- here one.  From a bias of 0 the
                  item bias of pair (k, j) ends at 0 + -(1 * g) = -g: the kernel's own gk entry, to the bit, for every one of the
                  1 + n pairs.  An item ROW ends at fl32(V - fl32(g * u)): the product g * u is formed in fp32 first (it is the
                  summed gradient the rule takes), so there are TWO roundings where |u| = 3/4 (g * 3 needs two more bits) and one
                  otherwise; item_rows_follow restates exactly that in numpy float32 and compares BITS.
  two minibatches N = B + 5: the second is short and has k0 = B != 0.  Their users and items are disjoint, so each row of the
                  result belongs to one minibatch and the second minibatch's scores are exact too.

SOFTMAX.  The reference is float64 from the exact scores: g_j = e^(s_j - m) / Z / bm, g_0 = -(sum_{j>0} e^(s_j - m)) / Z / bm,
l = log Z - (s_0 - m).  The tolerance is MEASURED, as als_checks has it: a float32 numpy restatement of the same formulas
(np.float32 exponentials, the sum taken sequentially in pair order -- the last element of a float32 cumsum, no more accurate than
the kernel's per-lane-then-butterfly order) is the yardstick; its worst error against float64 on the case's own scores is
measured on every run and the kernel passes at max(FACTOR x that, 2^-22).
  spread    random dyadic rows, score gaps asserted within 16: nothing underflows, every pair's g is held RELATIVELY.
  planted   pair j*(k) of interaction k -- cycled through {0, 1, G - 1, G, G + 1, 63, 64, 65, NP - 1} below NP -- has the item row
            32 sign(u) (zeros -> +32): its score 32 sum|u_d| lies more than 88 above every other pair's (user rows carry four
            entries of magnitude >= 3/4, so sum|u| >= 3 and the gap is >= 31 * 3; asserted).  A max reduction that misses it
            gives inf / NaN, not a quietly equal number.  `mirrored`: the positive's score the LOWEST by that gap.  Held
            ABSOLUTELY per interaction at max(FACTOR x yardstick, 2^-22) x max_j|g_j| (the other pairs underflow) + 2^-126, the
            smallest normal float32 (softmax_checks.FP32_TINY's rule: where j* = 0 every g of the interaction lies below the
            normal range, in which the format holds no relative precision).  Every value must be finite.
  Measured, spread regime, B = 37, D = 8 (worst pair of both minibatches, relative; recorded for the reader -- the tests measure
  the yardstick again on every run and print all three with `pytest -s`):
        n      G   yardstick   emulator kernel   gfx950 kernel          n      G   yardstick   emulator kernel   gfx950 kernel
        1      2   9.5e-8      9.7e-8            9.7e-8                63     64   3.7e-7      2.0e-7            2.0e-7
        3      4   2.0e-7      2.0e-7            2.0e-7                64     64   4.1e-7      1.9e-7            2.1e-7
        7      8   2.4e-7      2.0e-7            2.0e-7                65     64   5.5e-7      2.4e-7            2.0e-7
        8     16   2.4e-7      1.8e-7            1.8e-7               127     64   5.7e-7      2.7e-7            2.8e-7
       15     16   3.2e-7      2.3e-7            2.3e-7               128     64   4.9e-7      2.4e-7            2.5e-7
       16     32   2.8e-7      2.1e-7            2.1e-7               200     64   6.5e-7      2.2e-7            2.2e-7
       31     32   3.4e-7      2.4e-7            2.4e-7              1024     64   2.6e-6      2.5e-7            2.1e-7
       32     64   3.4e-7      2.6e-7            2.6e-7
  B = 1 (n = 3, 31, 200), B = 300 (n = 63, 64) and D = 24 (n = 65) lie inside these ranges (yardstick 8.8e-8 .. 5.9e-7, either
  kernel 7.5e-8 .. 2.4e-7).  The kernel is at most 1.03 x the yardstick (n = 1, where both are one or two roundings) and 0.1 x at
  n = 1024: its butterfly adds n terms in n / G + log2 G steps, the yardstick in n.  Planted and mirrored, per interaction over
  max_j|g_j|: yardstick 2.4e-8 .. 1.3e-7, either kernel 2.4e-8 .. 1.2e-7 -- the rounding of 1 / bm and little else, so the floor
  2^-22 decides there; what these regimes test is the max reduction (inf / NaN otherwise), not the last bits.

ADAPTIVE HINGE, WARP.  The reference is computed on the host from the exact scores through the reference's view(n, B) layout (a
numpy reshape of the flat draws -- not the kernels' f / n, f % n arithmetic): adaptive hinge the first maximum, g = fl32(1 / bm)
where x = s_best - s_p + 1 >= 0; warp the first row with x > 0, g = fl32(log(max(1, (I - 1) // (r + 1)))) fl32(1 / bm).  With
exact scores there is no guard: x is exact in fp32 and in float64.  Adaptive hinge is compared by BITS (-g, +g, exact zeros),
warp within 2^-22 relative (logf against log, one product).  Both routes run (the persistent kernel, the launch path) and the
engine's profile says which one did.  PLANTED columns (plant_columns): an exact tie of the maximum at rows (0, n - 1) and at two
rows of different interactions; x == 0 exactly; warp's first violator at row 0 and at row n - 1 behind rows at x == 0; no
violator at all; a selected draw of another interaction than the positive.  In every other column the maximum is made unique
(a later holder of a tied maximum gets a fresh row) and that is asserted.

EVERY CASE also holds: the returned loss within 1e-5 of float64; user rows and user biases against float64 U - sum_j g_j V_j under
engine_checks.step_update_bounds (rel_delta = 1e-5, weights_checks.assert_within) -- the user pass's sum over 1 + n pairs; a pair
with zero gradient, and every row outside the call, keeps its bits; softmax's user biases stay exactly 0."""
import types

import numpy as np

import engine_checks as ec
import warp_checks as wk
import weights_checks as wc

FACTOR = 4.0
FLOOR = 2.0 ** -22
FP32_TINY = 2.0 ** -126
HP = dict(lr=1.0)
LAUNCH = dict(epoch_kernel=0)

SOFTMAX_NS = (1, 3, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 200, 1024)
COLUMN_NS = (2, 7, 16, 33, 64, 65, 200, 1024)
REGIMES = ('spread', 'planted', 'mirrored')
# (n, B, D, regime)
SOFTMAX_CASES = [(n, 37, 8, r) for n in SOFTMAX_NS for r in REGIMES] + \
                [(n, 1, 8, r) for n in (3, 31, 200) for r in ('spread', 'planted')] + \
                [(n, 300, 8, r) for n in (63, 64) for r in ('spread', 'planted')] + [(65, 37, 24, 'spread'), (65, 37, 24, 'planted')]
# (n, B, D)
COLUMN_CASES = [(n, 37, 8) for n in COLUMN_NS] + [(n, 1, 8) for n in (2, 33, 200)] + [(64, 300, 8), (33, 37, 24)]
COLUMN_LOSSES = ('adaptive_hinge', 'warp')
ROUTES = wk.ROUTES  # ('persistent', 'launch')
EDGES = ('tie_ends', 'tie_split', 'x_zero', 'warp_row0', 'warp_last', 'no_violator', 'other_interaction')


def softmax_group(NP):
    """csrc/slk_bilinear.hip: slk_softmax_group -- the lane-group width of k_softmax_loss, a function of n alone."""
    g = 2
    while g < NP and g < 64:
        g <<= 1
    return g


def check_grid_covers_the_kernel():
    """No engine: the softmax grid takes every instantiation; each with all its lanes on (NP == G) and, from G = 16, with one lane
    past the width below (NP == G / 2 + 1); G = 64 with one pair per lane, one pair past it (NP = 65: the strided form's
    shortest second trip), one and two full strides with and without a pair past them, a ragged stride and the cap."""
    nps = [n + 1 for n in SOFTMAX_NS]
    assert {softmax_group(NP) for NP in nps} == {2, 4, 8, 16, 32, 64}
    for G in (2, 4, 8, 16, 32, 64):
        assert G in nps and softmax_group(G) == G, G
    for G in (16, 32, 64):
        assert G // 2 + 1 in nps and softmax_group(G // 2 + 1) == G, G
    assert 65 in nps and 128 in nps and 129 in nps and 201 in nps and 1025 in nps


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def dyadic(rs, shape):
    return rs.randint(-4, 5, shape) / 4.0


def planted_pairs(NP):
    G = softmax_group(NP)
    return sorted({j for j in (0, 1, G - 1, G, G + 1, 63, 64, 65, NP - 1) if 0 <= j < NP})


def make_case(loss, n, B, D=8, regime='spread', seed=3):
    rs = np.random.RandomState(1000 * seed + 7 * n + B + D)
    N, NP = B + 5, n + 1
    I, NU = N * NP + 1, N + 2
    users = rs.permutation(NU)[:N].astype(np.int64)
    pair_item = rs.permutation(I)[:N * NP].reshape(N, NP).astype(np.int64)  # the item of pair j of interaction k
    Ut, Vt = dyadic(rs, (NU, D)), dyadic(rs, (I, D))
    case = types.SimpleNamespace(loss=loss, n=n, nn=n, B=B, D=D, N=N, NP=NP, I=I, NU=NU, users=users, pair_item=pair_item,
                                 items=pair_item[:, 0].copy(), negs=pair_item[:, 1:].reshape(-1).copy(), regime=regime, idesc=None,
                                 ratings=None, weights=None, planted={})
    if loss == 'softmax':
        if regime != 'spread':
            # four entries of magnitude >= 3/4: sum|u| >= 3
            Ut[:, :4] = rs.choice([-1.0, -0.75, 0.75, 1.0], (NU, 4))
            big = 32.0 * np.where(Ut[users] < 0, -1.0, 1.0)
            if regime == 'planted':
                js = planted_pairs(NP)
                case.jstar = np.array([js[k % len(js)] for k in range(N)])
                Vt[pair_item[np.arange(N), case.jstar]] = big
            else:
                case.jstar = np.zeros(N, np.int64)
                Vt[pair_item[:, 0]] = -big
    else:
        Ut[:, 0] = rs.choice([-1.0, 1.0], NU)  # a row t * u_0 e_0 scores exactly t against this user
    case.params = [Ut, Vt, np.zeros(NU), np.zeros(I)]
    if loss != 'softmax':
        plant_columns(case, rs)
        make_maxima_unique(case, rs)
    return case


def minibatches(case):
    return [(lo, min(lo + case.B, case.N)) for lo in range(0, case.N, case.B)]


def exact_scores(case):
    """[N, 1 + n] float64, exact: S[k, j] = U[user k] . V[item of pair (k, j)]."""
    Ut, Vt = case.params[0], case.params[1]
    return np.einsum('kd,kjd->kj', Ut[case.users], Vt[case.pair_item])


def assert_scores_exact(case):
    """The precondition, on the CPU: the float32 fma chain, a float32 sum in reversed order and the float64 product agree
    exactly on the case's own tables, pair by pair."""
    u32 = case.params[0][case.users].astype(np.float32)[:, None, :]
    v32 = case.params[1][case.pair_item].astype(np.float32)
    assert np.array_equal(u32.astype(np.float64)[:, 0], case.params[0][case.users]) and np.array_equal(v32.astype(np.float64), case.params[1][case.pair_item])
    S = exact_scores(case)
    chain = ec.f32_chain_dot(np.broadcast_to(u32, v32.shape), v32)
    rev = np.zeros(S.shape, np.float32)
    for d in range(case.D - 1, -1, -1):
        rev = (rev + (u32[..., d] * v32[..., d]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(chain.astype(np.float64), S) and np.array_equal(rev.astype(np.float64), S)
    assert len(np.unique(case.pair_item)) == case.N * case.NP and len(np.unique(case.users)) == case.N
    return S


# ---- the column losses' planted edges ------------------------------------------------------------------------------------------------
def _set_score(case, k, j, t):
    """Pair j of interaction k (of the call) scores exactly t: its item's row is t * u_0 e_0, |u_0| = 1."""
    row = np.zeros(case.D)
    row[0] = t * case.params[0][case.users[k], 0]
    case.params[1][case.pair_item[k, j]] = row


def _draw(case, lo, bm, c, r):
    """Row r of column c of the minibatch at lo, in the reference's view(n, bm): flat draw r * bm + c -> (interaction, pair)."""
    f = r * bm + c
    return lo + f // case.n, 1 + f % case.n


def plant_columns(case, rs):
    """Edge e in column c of minibatch m where (c + 3 m) % 7 == e, c < 14: each edge twice in a minibatch of 37, five of them in
    the short one, one per minibatch at B = 1.  An edge a column cannot hold (bm = 1: every draw is the positive's own) gives
    way to warp_last.  case.planted[(m, c)] = edge."""
    n = case.n
    for m, (lo, hi) in enumerate(minibatches(case)):
        bm = hi - lo
        for c in range(min(bm, 14)):
            edge = EDGES[(c + 3 * m) % 7]
            if bm == 1 and edge in ('tie_split', 'other_interaction'):
                edge = 'warp_last'
            own = lambda r: _draw(case, lo, bm, c, r)[0]
            cand = None
            if edge == 'tie_ends':
                sp, cand = 0.25, np.full(n, -0.75)
                cand[[0, n - 1]] = 0.5
            elif edge == 'tie_split':  # (n = 2: rows 0 and 1, the only pair there is)
                r1 = 1 if n >= 3 else 0
                r2 = [r for r in range(r1 + 1, n) if own(r) != own(r1)]
                if r2:
                    sp, cand = 0.5, np.full(n, -1.0)
                    cand[[r1, r2[0]]] = 0.75
            elif edge == 'x_zero':
                sp, cand = 0.5, np.full(n, -1.0)
                cand[n // 2] = -0.5
            elif edge == 'warp_row0':
                sp, cand = 0.5, np.full(n, -0.5)
                cand[0] = -0.25
            elif edge == 'warp_last':
                sp, cand = 0.5, np.full(n, -0.5)
                cand[n - 1] = -0.25
            elif edge == 'no_violator':
                sp, cand = 1.0, -0.25 - 0.25 * (np.arange(n) % 3)
            else:
                rr = [r for r in range(n) if own(r) != lo + c]
                if rr:
                    sp, cand = 0.25, np.full(n, -1.0)
                    cand[rr[0]] = 0.75
            if cand is None:
                continue
            _set_score(case, lo + c, 0, sp)
            for r in range(n):
                _set_score(case, *_draw(case, lo, bm, c, r), cand[r])
            case.planted[(m, c)] = edge


def candidate_matrix(S_mb):
    """The reference's layout: the minibatch's draws, flat in (interaction, pair) order, viewed as [n, bm]."""
    bm, n = S_mb.shape[0], S_mb.shape[1] - 1
    return S_mb[:, 1:].reshape(-1).reshape(n, bm)


def make_maxima_unique(case, rs):
    """Every column that is not planted: a later holder of a tied maximum gets a fresh random row, until the two largest
    candidates differ."""
    for _ in range(200):
        S, again = exact_scores(case), False
        for m, (lo, hi) in enumerate(minibatches(case)):
            bm = hi - lo
            cand = candidate_matrix(S[lo:hi])
            for c in np.nonzero((cand == cand.max(0)).sum(0) > 1)[0]:
                if (m, int(c)) in case.planted:
                    continue
                for r in np.nonzero(cand[:, c] == cand[:, c].max())[0][1:]:
                    k, j = _draw(case, lo, bm, int(c), int(r))
                    case.params[1][case.pair_item[k, j]] = dyadic(rs, case.D)
                again = True
        if not again:
            return
    raise AssertionError('tied maxima remain')


def assert_column_preconditions(case, S):
    seen = set(case.planted.values())
    for m, (lo, hi) in enumerate(minibatches(case)):
        bm = hi - lo
        cand = candidate_matrix(S[lo:hi])
        top2 = np.sort(cand, axis=0)[-2:] if case.n > 1 else None
        for c in range(bm):
            if (m, c) not in case.planted:
                assert top2[1, c] > top2[0, c], ('a tied maximum in a column that is not planted', m, c)
    # (bm = 1: every draw is the positive's own -- no second interaction to tie with or to select from)
    assert seen == set(EDGES) - ({'tie_split', 'other_interaction'} if case.B == 1 else set()), seen


# ---- the references ------------------------------------------------------------------------------------------------------------------
def softmax_ref64(S, bm):
    m = S.max(1, keepdims=True)
    e = np.exp(S - m)
    zn = e[:, 1:].sum(1)
    Z = e[:, 0] + zn
    G = e / Z[:, None] / bm
    G[:, 0] = -zn / Z / bm
    return G, np.log(Z) - (S[:, 0] - m[:, 0])


def softmax_f32(S, bm):
    """The yardstick: the same formulas in np.float32, the sum sequential in pair order."""
    S = S.astype(np.float32)
    m = S.max(1, keepdims=True)
    e = np.exp((S - m).astype(np.float32)).astype(np.float32)
    zn = np.cumsum(e[:, 1:], axis=1, dtype=np.float32)[:, -1]
    Z = (e[:, 0] + zn).astype(np.float32)
    inv_b = np.float32(1.0) / np.float32(bm)
    G = ((e / Z[:, None]).astype(np.float32) * inv_b).astype(np.float32)
    G[:, 0] = -((zn / Z).astype(np.float32) * inv_b)
    return G


def column_ref(loss, S, bm, I):
    """(G [bm, 1 + n] float64 holding float32 values, l [bm] float64) of one minibatch's columns through view(n, bm)."""
    n = S.shape[1] - 1
    cand, sp = candidate_matrix(S), S[:, 0]
    inv_b = np.float64(np.float32(1.0) / np.float32(bm))
    cols = np.arange(bm)
    if loss == 'adaptive_hinge':
        best = cand.argmax(0)  # the first maximum
        x = cand[best, cols] - sp + 1.0
        g = np.where(x >= 0, inv_b, 0.0)
        l = np.maximum(x, 0.0)
    else:
        viol = cand - sp[None, :] + 1.0 > 0
        hit = viol.any(0)
        best = viol.argmax(0)  # the first violator
        w = np.log(np.maximum(1, (I - 1) // (best + 1)).astype(np.float64))
        x = cand[best, cols] - sp + 1.0
        g = np.where(hit, np.float64(1.0) * w.astype(np.float32) * inv_b, 0.0)
        l = np.where(hit, w * x, 0.0)
    flat = np.zeros(n * bm)
    flat[best * bm + cols] = g
    G = np.empty((bm, n + 1))
    G[:, 0] = -g
    G[:, 1:] = flat.reshape(bm, n)
    return G, l, best


# ---- one call, read back -------------------------------------------------------------------------------------------------------------
def _profiled(be, case, route, fn):
    if case.loss != 'softmax':
        return wk._profiled_route(be, route, fn)
    eng = be.engine
    eng.profile_reset()
    eng.profile_enable(True)
    try:
        out = fn()
    finally:
        eng.profile_enable(False)
    prof = eng.profile_read()
    # the launch path by itself: no persistent launch, and per minibatch one score stage (k_score_pass + k_softmax_loss<G>,
    # G = slk_softmax_group(n + 1)), one user pass
    n_mb = len(minibatches(case))
    assert prof['epoch'][0] == 0 and prof['score'][0] == n_mb and prof['user_pass'][0] >= n_mb, prof
    return out


def run_case(be, case, route=None):
    """The call; returns (losses, pre, post, g_read [N, 1 + n] float32: dL/dscore of every pair, read from the item biases)."""
    with be.engine.options(**(LAUNCH if route == 'launch' else {})):
        dev = wc.fresh(be, case, 'sgd', HP)
        pre = wc.read(be, dev)
        losses = _profiled(be, case, route, lambda: wc.train(be, dev, case, 0, case.N, case.B, weights=None))
    assert dev.optim.step == len(minibatches(case))
    post = wc.read(be, dev)
    return losses, pre, post, post[3][0].ravel()[case.pair_item]


def assert_rows_follow(case, pre, post, bias, Gs, what):
    """What every case holds once its per-pair gradients are known (the module docstring, EVERY CASE).  bias: [N, 1 + n] item
    biases after the call; Gs: per minibatch the float64 reference G."""
    G = np.concatenate(Gs)
    g32 = (np.float32(0.0) - bias).astype(np.float32)
    U32, V32 = pre[0][0], pre[1][0]
    # item rows: fl32(V - fl32(g u)) with the g that was read, by bits; a zero gradient leaves the row and the bias as they were
    want_rows = (V32[case.pair_item] - (g32[:, :, None] * U32[case.users][:, None, :]).astype(np.float32)).astype(np.float32)
    got_rows = post[1][0][case.pair_item]
    assert wc.same_bits(got_rows, want_rows), (what, 'item rows: %d differ' % int((got_rows.view(np.uint32) != want_rows.view(np.uint32)).any(2).sum()))
    zero = G == 0
    assert wc.same_bits(bias[zero], np.zeros(int(zero.sum()), np.float32)), (what, 'the bias of a pair without gradient moved')
    assert wc.same_bits(got_rows[zero], V32[case.pair_item][zero]), (what, 'the row of a pair without gradient moved')
    # rows outside the call
    out_i = np.setdiff1d(np.arange(case.I), case.pair_item)
    out_u = np.setdiff1d(np.arange(case.NU), case.users)
    assert out_i.size == 1 and out_u.size == 2
    for t, rows in ((0, out_u), (2, out_u), (1, out_i), (3, out_i)):
        assert wc.same_bits(post[t][0][rows], pre[t][0][rows]), (what, 'table', t, 'a row outside the call moved')
    if case.loss == 'softmax':
        assert wc.same_bits(post[2][0], np.zeros(case.NU, np.float32)), (what, 'a user bias moved')
    # user rows and user biases: float64 U - sum_j g_j V_j, bounds minibatch by minibatch (each row belongs to one)
    V64, U64 = V32.astype(np.float64), U32.astype(np.float64)
    want = [U64.copy(), None, np.zeros(case.NU), None]
    bounds = [np.zeros((case.NU, case.D)), None, np.zeros(case.NU), None]
    for (lo, hi), Gm in zip(minibatches(case), Gs):
        g = [np.zeros((case.NU, case.D)), np.zeros((case.I, case.D)), np.zeros(case.NU), np.zeros(case.I)]
        g[0][case.users[lo:hi]] = np.einsum('kj,kjd->kd', Gm, V64[case.pair_item[lo:hi]])
        g[2][case.users[lo:hi]] = 0.0 if case.loss == 'softmax' else Gm.sum(1)
        g[1][case.pair_item[lo:hi]] = Gm[:, :, None] * U64[case.users[lo:hi]][:, None, :]
        g[3][case.pair_item[lo:hi]] = Gm
        b = ec.step_update_bounds('sgd', HP, [x[0] for x in pre], [None] * 4, [None] * 4, g, 1, rel_delta=1e-5)
        for t in (0, 2):
            want[t] -= g[t]
            bounds[t] += b[t][0]
    for t in (0, 2):
        d = np.abs(post[t][0].astype(np.float64).reshape(want[t].shape) - want[t])
        tol = 1e-5 * max(np.abs(want[t]).max(), 1e-30) + bounds[t]
        assert not (d > tol).any(), (what, 'table', t, '%d elements beyond the bound' % int((d > tol).sum()), float((d / np.maximum(tol, 1e-300)).max()))


def assert_losses(case, losses, ls, what):
    for m, l in enumerate(ls):
        got, want = float(losses[m]), float(l.mean())
        assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want) + FP32_TINY, (what, 'minibatch', m, got, want)


# ---- softmax -------------------------------------------------------------------------------------------------------------------------
def check_softmax(be, n, B, D, regime):
    """Returns (yardstick, the kernel's own worst figure): relative per pair (spread), per interaction over max_j|g_j| (planted)."""
    case = make_case('softmax', n, B, D, regime)
    S = assert_scores_exact(case)
    others = S.copy()
    if regime == 'spread':
        assert (S.max(1) - S.min(1)).max() <= 16.0
    else:
        rows = np.arange(case.N)
        others[rows, case.jstar] = np.nan
        gap = (S[rows, case.jstar] - np.nanmax(others, 1)) if regime == 'planted' else (np.nanmin(others, 1) - S[:, 0])
        assert gap.min() > 88.0, gap.min()
        assert (np.abs(case.params[0][case.users]) > 0).sum(1).min() >= 4
    what = ('softmax', n, B, D, regime)
    losses, pre, post, bias = run_case(be, case)
    assert np.isfinite(bias).all() and np.isfinite(losses).all(), what
    for t in range(4):
        assert np.isfinite(post[t][0]).all(), (what, 'table', t)
    g_read = -bias.astype(np.float64)
    Gs, ls, yard, worst = [], [], 0.0, 0.0
    refs = []
    for lo, hi in minibatches(case):
        G, l = softmax_ref64(S[lo:hi], hi - lo)
        Gs.append(G)
        ls.append(l)
        refs.append((lo, hi, G, softmax_f32(S[lo:hi], hi - lo).astype(np.float64)))
    # the yardstick over the whole case first, then the kernel against it
    if regime == 'spread':
        yard = max(float((np.abs(g32 - G) / np.abs(G)).max()) for _, _, G, g32 in refs)
        bound = max(FACTOR * yard, FLOOR)
        for lo, hi, G, _ in refs:
            rel = np.abs(g_read[lo:hi] - G) / np.abs(G)
            worst = max(worst, float(rel.max()))
            k, j = np.unravel_index(rel.argmax(), rel.shape)
            assert rel.max() <= bound, (what, 'interaction', lo + int(k), 'pair', int(j), float(rel.max()), 'bound', bound,
                                        '%d pairs beyond it' % int((rel > bound).sum()))
    else:
        normal = lambda G: np.abs(G).max(1) >= 2.0 ** -100  # (where j* = 0 every g of the interaction is below the normal range)
        yard = max(float((np.abs(g32 - G).max(1) / np.abs(G).max(1))[normal(G)].max()) for _, _, G, g32 in refs if normal(G).any())
        bound = max(FACTOR * yard, FLOOR)
        for lo, hi, G, _ in refs:
            assert np.array_equal(normal(G), (case.jstar[lo:hi] != 0) | (regime == 'mirrored'))
        for lo, hi, G, _ in refs:
            err, scale = np.abs(g_read[lo:hi] - G).max(1), np.abs(G).max(1)
            ok = normal(G)
            if ok.any():
                worst = max(worst, float((err / scale)[ok].max()))
            assert (err <= bound * scale + FP32_TINY).all(), (what, 'interaction', lo + int((err - bound * scale).argmax()),
                                                              float((err / np.maximum(scale, 1e-300)).max()), 'bound', bound)
    print('WIDE softmax n %d B %d D %d %s G %d: yardstick %.3g, bound %.3g, kernel %.3g' % (n, B, D, regime, softmax_group(n + 1), yard, bound, worst))
    assert_losses(case, losses, ls, what)
    assert_rows_follow(case, pre, post, bias, Gs, what)
    return yard, worst


# ---- adaptive hinge, warp ------------------------------------------------------------------------------------------------------------
def check_column(be, loss, n, B, D, route):
    case = make_case(loss, n, B, D)
    S = assert_scores_exact(case)
    assert_column_preconditions(case, S)
    what = (loss, n, B, D, route)
    losses, pre, post, bias = run_case(be, case, route)
    Gs, ls, rows_hit = [], [], set()
    for m, (lo, hi) in enumerate(minibatches(case)):
        G, l, best = column_ref(loss, S[lo:hi], hi - lo, case.I)
        Gs.append(G)
        ls.append(l)
        rows_hit |= set(best[G[:, 0] != 0].tolist())
        want_bias = (np.float32(0.0) - G.astype(np.float32)).astype(np.float32)  # (G holds float32 values under adaptive hinge)
        got = bias[lo:hi]
        if loss == 'adaptive_hinge':
            bad = got.view(np.uint32) != want_bias.view(np.uint32)
            assert not bad.any(), (what, 'minibatch', m, '%d pairs differ' % int(bad.sum()), 'first (interaction, pair)', np.argwhere(bad)[0].tolist(),
                                   [case.planted.get((m, c)) for c in np.unique(np.argwhere(bad)[:, 0])[:4].tolist()])
        else:
            live = G != 0
            assert wc.same_bits(got[~live], want_bias[~live]), (what, 'minibatch', m, 'a pair outside the selection carries a gradient')
            rel = np.abs(-got[live].astype(np.float64) - G[live]) / np.abs(G[live])
            assert (rel <= FLOOR).all(), (what, 'minibatch', m, float(rel.max()))
        # the planted edges did what they were planted for
        for c in range(hi - lo):
            edge = case.planted.get((m, c))
            x0 = edge == 'x_zero'
            if edge == 'no_violator' or (x0 and loss == 'warp'):
                assert G[c, 0] == 0 and l[c] == 0
            elif edge is not None:
                assert G[c, 0] < 0 and (l[c] > 0) != x0, (edge, c)
            if edge in ('tie_ends', 'warp_row0'):
                assert best[c] == 0
            if edge == 'warp_last':
                assert best[c] == n - 1
            if edge == 'other_interaction':
                assert lo + (best[c] * (hi - lo) + c) // n != lo + c
    if B > 1:
        assert 0 in rows_hit and n - 1 in rows_hit
    print('WIDE', what, 'losses', losses.tolist())
    assert_losses(case, losses, ls, what)
    assert_rows_follow(case, pre, post, bias, Gs, what)
