"""loss='warp' (include/spotlight_hip.h: SLK_LOSS_WARP) -- backend-agnostic checks, run on the emulator build by
tests/test_emu_warp.py and on the gfx950 library by tests/test_gpu_warp.py; the model level is tests/test_host_warp.py.

THE REFERENCE (restate_loss / restate_step) is a float64 torch restatement of the definition written here, in the manner of
weights_checks.restate_step: the BilinearNet forward on float64 leaves, the candidates in the reference's view(n, B) layout, the
first violating row per column, the weight log(max(1, (I - 1) // (t + 1))) as a constant of the backward pass, autograd, and
torch's own optimizer classes for the step (optim_checks.torch_step64).  Closed loop: before each minibatch the engine's tables
and state go to torch, which takes that one step.

THE BOUNDS are the project's: loss within 1e-5 relative; every element of every table / state tensor within
engine_checks.step_update_bounds at rel_delta = 1e-5 plus 1e-5 of the tensor's largest magnitude (weights_checks.assert_within);
the 7-item cases alone add the project's floor for exactly cancelling sums (cancellation_floor, here and in foldin_checks).

THE GUARD.  The selection is discontinuous: a hinge argument x_r within rounding of 0 selects another row in fp32 than in float64.
Every compared step therefore first ASSERTS, on the float64 restatement, |x_r| >= GUARD = 1e-4 over all (column, r) -- with scores
O(1) about a hundred fp32 roundings of x.  No case is left out or skipped: the seeds below are chosen so that the restatement
alone (an open loop in float64, no engine: check_seed_meets_the_guard) stays 2 * GUARD away, which the engine's closed loop -- its
tables differ from the open loop's by fp32 roundings -- then cannot undercut."""
import types

import numpy as np
import pytest
import torch

import engine_checks as ec
import foldin_checks as fc
import optim_checks as oc
import weights_checks as wc
from spotlight_amd import _native

LOSS = 'warp'
KINDS = ('adagrad', 'sgd', 'sparse_adam', 'adam_dense', 'adagrad_dense')
SPARSE = ('adagrad', 'sgd', 'sparse_adam')
DS = fc.DS                 # (6, 24, 64, 72): the four row layouts
NS = (1, 3, 5)
U, N, B = 37, 300, 64      # five minibatches, the last of 44: bm != B in the view(n, bm) indexing
ITEMS = (333, 7, 2)        # generic; duplicates, negatives equal to positives, weights log 6, log 3, log 2, 0, 0; weight 0 everywhere
GUARD = 1e-4
LAUNCH = dict(epoch_kernel=0)
ROUTES = ('persistent', 'launch')
STEP0 = 7

# (D, n, I) of the closed loop, and who takes them: adagrad every (D, n) at I = 333; the other kinds every D once with n
# rotating; every kind the 7-item and the 2-item catalogue at n = 5 (all five weights of t = 0 .. 4), D rotating.
CLOSED = [('adagrad', D, n, 333) for D in DS for n in NS] + \
         [(k, D, NS[(i + j) % 3], 333) for j, k in enumerate(KINDS[1:]) for i, D in enumerate(DS)] + \
         [(k, DS[j % 4], 5, 7) for j, k in enumerate(KINDS)] + [(k, DS[(j + 1) % 4], 5, 2) for j, k in enumerate(KINDS)]
# The seed of a case's data where the default's restatement comes within 2 * GUARD of a tie (check_seed_meets_the_guard finds them)
DEFAULT_SEED = 5
SEEDS = {}
# fold-in's closed loop, (D, I, H, n): every row layout and every n; 70 users hold every history length of
# foldin_checks.history_lengths; the 7-item catalogue at n = 5
FOLD_CLOSED = [(6, 333, 5, 1), (24, 333, 70, 3), (64, 333, 5, 5), (72, 333, 5, 3)]
FOLD_CLOSED_7 = [(D, 7, 5, 5) for D in DS]
FOLD_SEEDS = {}
# fold-in at wide n, (D, n, optimizer): foldin_checks.WIDE's shapes over foldin_checks.WIDE_LENGTHS (59 positions, n * 59 hinge
# arguments per step for the guard to hold off 0 -- the histories of FOLD_CLOSED, with 300 interactions in one of them, would
# leave no seed at n = 64)
FOLD_WIDE = fc.WIDE
FOLD_WIDE_SEEDS = {}


def hyper(kind):
    return fc.hparams(kind)


def case_seed(kind, D, n, I):
    return SEEDS.get((kind, D, n, I), DEFAULT_SEED)


def make_case(D, n, I, seed=DEFAULT_SEED, U=U, N=N):
    case = wc.make_case('adaptive_hinge', D, U=U, I=I, N=N, seed=seed, nn=n)  # (the draws and their layout are adaptive hinge's)
    case.loss = LOSS
    return case


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def warp_terms(pos, neg, num_items):
    """Per column: (l_c, x) from the positive scores [bm] and the candidates [n, bm] -- the definition, in the tensors' dtype."""
    x = neg - pos.unsqueeze(0) + 1.0
    n = x.shape[0]
    rows = torch.arange(n).view(n, 1).expand_as(x)
    first = torch.where(x > 0, rows, torch.full_like(rows, n)).min(0)[0]  # (NaN > 0 is False: a NaN does not violate)
    hit = first < n
    t = first.clamp(max=n - 1)
    rank = torch.clamp((num_items - 1) // (t + 1), min=1)
    w = torch.log(rank.to(x.dtype))
    x_t = x.gather(0, t.unsqueeze(0)).squeeze(0)
    return torch.where(hit, w * x_t, torch.zeros_like(x_t)), x


def restate_loss(P, users, items, negs, weights, nn, num_items, keep=None):
    """(the minibatch loss on torch leaves P, min |x_r| over the step).  weights None: the plain mean.  `keep` (a list): the
    score tensors (positives [bm], candidates [n, bm]) are appended to it and keep their gradients."""
    dt = P[0].dtype
    tl = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    score = lambda us, its: (P[0][tl(us)] * P[1][tl(its)]).sum(1) + P[2][tl(us)] + P[3][tl(its)]
    pos = score(users, items)
    bm = len(users)
    # the reference's layout: users repeated user-major, ONE draw of B * n, scores viewed as [n, B]
    neg = score(np.repeat(users, nn), negs).view(nn, bm)
    if keep is not None:
        pos.retain_grad()
        neg.retain_grad()
        keep += [pos, neg]
    l, x = warp_terms(pos, neg, num_items)
    finite = x.detach()[torch.isfinite(x.detach())]
    xmin = float(finite.abs().min()) if finite.numel() else float('inf')
    if weights is None:
        return l.mean(), xmin
    w = torch.from_numpy(np.asarray(weights, np.float64)).to(dt)
    return (w * l).sum() / w.sum(), xmin


def restate_step(kind, hp, pre, step0, users, items, negs, weights, nn, num_items):
    """ONE step from pre = [(p, s1, s2)] * 4 (fp32): (loss, post [(p, s1, s2)] * 4, dense gradients [g] * 4, min |x|), float64."""
    P = [torch.from_numpy(np.array(pre[t][0], dtype=np.float64)).requires_grad_(True) for t in range(4)]
    L, xmin = restate_loss(P, users, items, negs, weights, nn, num_items)
    L.backward()
    g = [P[t].grad.numpy().copy() for t in range(4)]
    tu, ti = np.unique(users), np.unique(np.concatenate([items, negs]))  # every looked-up row is touched (SparseAdam decays it)
    post = [oc.torch_step64(kind, hp, pre[t][0], pre[t][1], pre[t][2], step0, g[t].reshape(pre[t][0].shape), touched)
            for t, touched in enumerate((tu, ti, tu, ti))]
    return float(L.item()), post, g, xmin


def cancellation_floor(case, pre):
    """abs_delta of step_update_bounds for the 7-ITEM cases only (foldin_checks.cancellation_floor's rule on the training routes);
    every other case is held to the bare bound.

    With 7 items a minibatch is full of duplicates and negatives equal to positives: an item is pulled in as a positive of one
    column and pushed away as the selected draw of another with the SAME weight, so elements of its gradient are sums that cancel
    EXACTLY in exact arithmetic.  The float64 restatement ends at 0.0 there (step_update_bounds then grants that element no
    allowance at all: `touched` is False), the engine's fp32 sum in another order at a residue of 1e-9, and Adagrad / Adam from a
    zero accumulator turn the residue into a step of lr (seen on the GPU: adagrad, dim 6, n = 5, the persistent route, ONE item
    bias 0.11 off; the emulator's order happened to cancel).  The fp32 rounding of such a sum scales with its terms, not with
    the sum: at most two live occurrences per column, each |dL/dscore| <= log(I - 1) / bm times a factor of magnitude
    <= max(1, |table|max), so the terms' magnitudes add up to at most S = 2 log(I - 1) max(1, |U|max, |V|max) per element; the
    floor is 2 ulp of S = S * 2^-22 -- engine_checks.check_train_matches_oracle's floor for its degenerate runs, from the number
    format alone.  It decides only where the gradient itself is ~0: there is no quota."""
    if case.I != 7:
        return 0.0
    return 2.0 ** -22 * 2.0 * np.log(case.I - 1.0) * max(1.0, float(np.abs(pre[0][0]).max()), float(np.abs(pre[1][0]).max()))


def bounds_for(case, kind, hp, pre, g, step):
    return ec.step_update_bounds(kind, hp, [x[0] for x in pre], [x[1] for x in pre], [x[2] for x in pre],
                                 [g[t].reshape(pre[t][0].shape) for t in range(4)], step, rel_delta=1e-5,
                                 abs_delta=cancellation_floor(case, pre))


def assert_guard(xmin, what, guard=GUARD):
    assert xmin >= guard, ('a hinge argument within %g of 0: the comparison is not defined here, pick another seed' % guard, what, xmin)


def start_pre(case, kind):
    st = wc.start_state(case, kind)
    return [(np.asarray(case.params[t], np.float32).reshape(np.asarray(case.params[t]).shape), st[t][0], st[t][1]) for t in range(4)]


def check_seed_meets_the_guard(kind, D, n, I, weights=None):
    """No engine: the float64 restatement alone, open loop over the case's five minibatches, stays 2 * GUARD away from a tie."""
    case = make_case(D, n, I, seed=case_seed(kind, D, n, I))
    hp = hyper(kind)
    pre = start_pre(case, kind)
    w = case.weights if weights == 'case' else None
    worst = float('inf')
    for k, lo in enumerate(range(0, case.N, B)):
        hi = min(lo + B, case.N)
        _, post, _, xmin = restate_step(kind, hp, pre, STEP0 + k, case.users[lo:hi], case.items[lo:hi], case.negs[lo * n:hi * n],
                                        None if w is None else w[lo:hi], n, I)
        worst = min(worst, xmin)
        pre = [tuple(np.zeros_like(pre[t][0]) if x is None else np.asarray(x, np.float32).reshape(pre[t][0].shape) for x in post[t])
               for t in range(4)]
    assert_guard(worst, (kind, D, n, I), 2 * GUARD)
    return worst


# ---- 1 + 2. closed loop against the float64 restatement, both routes, behind the guard -------------------------------------------------------
def _profiled_route(be, route, fn):
    eng = be.engine
    eng.profile_reset()
    eng.profile_enable(True)
    try:
        out = fn()
    finally:
        eng.profile_enable(False)
    prof = eng.profile_read()
    if route == 'persistent':
        assert prof['epoch'][0] >= 1 and prof['user_pass'][0] == 0, prof
    else:
        assert prof['epoch'][0] == 0 and prof['user_pass'][0] >= 1, prof
    return out


def check_closed_loop(be, kind, D, n, I, route, weights=None):
    """weights None: slk_bilinear_train (the persistent kernel from a plain call at these sizes; the launch path forced as
    engine_checks forces it, epoch_kernel = 0).  weights 'case': slk_bilinear_train_weighted (always staged)."""
    case = make_case(D, n, I, seed=case_seed(kind, D, n, I))
    hp = hyper(kind)
    w = case.weights if weights == 'case' else None
    with be.engine.options(**(LAUNCH if route == 'launch' else {})):
        dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
        step = STEP0
        for lo in range(0, case.N, B):
            hi = min(lo + B, case.N)
            pre = wc.read(be, dev)
            want_loss, post, g, xmin = restate_step(kind, hp, pre, step, case.users[lo:hi], case.items[lo:hi],
                                                    case.negs[lo * n:hi * n], None if w is None else w[lo:hi], n, I)
            what = (kind, D, n, I, route, 'minibatch at', lo)
            assert_guard(xmin, what)
            run = lambda: wc.train(be, dev, case, lo, hi, B, weights=w)
            got_loss = _profiled_route(be, route, run) if w is None else run()
            step += 1
            assert dev.optim.step == step
            print('WARP closed loop', what, 'loss', float(got_loss[0]), want_loss, 'min|x|', xmin)
            assert abs(float(got_loss[0]) - want_loss) <= 1e-5 * abs(want_loss), (what, float(got_loss[0]), want_loss)
            wc.assert_within(wc.read(be, dev), post, bounds_for(case, kind, hp, pre, g, step), kind, what)


# ---- 3. bit for bit, engine against itself -----------------------------------------------------------------------------------------------
def check_routes_agree(be, kind, D, n, I=333):
    """One call over all five minibatches: the persistent kernel's tables and state are the launch path's, bit for bit (the
    losses to summation order: 2e-6, engine_checks.check_epoch_kernel_is_bit_identical)."""
    case = make_case(D, n, I)
    hp = hyper(kind)
    out = []
    for route in ROUTES:
        with be.engine.options(**(LAUNCH if route == 'launch' else {})):
            dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
            losses = _profiled_route(be, route, lambda: wc.train(be, dev, case, 0, case.N, B, weights=None))
            assert dev.optim.step == STEP0 + 5
            out.append((losses, wc.read(be, dev)))
    assert np.abs(out[0][0] - out[1][0]).max() <= 2e-6 * np.abs(out[1][0]).max()
    wc.assert_same_tables(out[0][1], out[1][1], ('persistent route against the launch path', kind, D, n))


def check_chunking_and_determinism(be, weights, kind='adagrad', D=16, U=3000, I=1000, N=30000, B=1000, n=5, chunk=4096, seed=21):
    """weights_checks.check_chunking_and_determinism's shapes and settings: one chunk against chunks of 4096 interactions with the
    prep in line and on the second stream, and the same call twice -- unweighted (weights None) and weighted ('case')."""
    eng = be.engine
    case = make_case(D, n, I, seed=seed, U=U, N=N)
    hp = hyper(kind)
    results = []
    for chunk_i, overlap_i in ((1 << 23, 0), (1 << 23, 0), (chunk, 0), (chunk, 1)):
        eng.set_option('chunk_interactions', chunk_i)
        eng.set_option('overlap_prep', overlap_i)
        eng.set_option('overlap_min_batch', 0)
        try:
            dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
            losses = [wc.train(be, dev, case, 0, N, B, weights=weights) for _ in range(2)]
            assert dev.optim.step == STEP0 + 2 * ((N + B - 1) // B)
            results.append((np.concatenate(losses), wc.read(be, dev)))
        finally:
            eng.set_option('chunk_interactions', 1 << 23)
            eng.set_option('overlap_prep', 0)
            eng.set_option('overlap_min_batch', 1 << 16)
    assert (results[0][0] > 0).all()
    for k, what in ((1, 'the same call again'), (2, 'chunks of %d, prep in line' % chunk), (3, 'chunks of %d, prep beside the passes' % chunk)):
        assert wc.same_bits(results[0][0], results[k][0]), ('mb_loss differs:', what)
        wc.assert_same_tables(results[0][1], results[k][1], what)


def check_scopes(be, D=16, n=3, I=333):
    """Inside an open item-bias shadow scope (Adagrad) a call gives the tables of the same call outside it, bit for bit, weighted
    or not.  A user-row ping-pong scope serves the pair losses only: warp is refused there in adaptive hinge's words, nothing is
    trained, and the scope still closes."""
    case = make_case(D, n, I)
    hp = hyper('adagrad')
    for weights in (None, 'case'):
        a, b = (wc.fresh(be, case, 'adagrad', hp, state=wc.start_state(case, 'adagrad'), step=STEP0) for _ in range(2))
        with be.engine.options(**LAUNCH):  # (a shadowed call takes the launches: so does the one outside)
            la = wc.train(be, a, case, 0, case.N, B, weights=weights)
            with be.engine.bias_shadow(b.tables, b.optim, stream=be.stream):
                lb = wc.train(be, b, case, 0, case.N, B, weights=weights)
        assert wc.same_bits(la, lb)
        wc.assert_same_tables(wc.read(be, a), wc.read(be, b), ('inside the item-bias shadow', weights))
    dev = wc.fresh(be, case, 'adagrad', hp)
    pre = wc.read(be, dev)
    with be.engine.options(**LAUNCH):
        with be.engine.user_pingpong(dev.tables, dev.optim, stream=be.stream):
            for loss in ('adaptive_hinge', LOSS):
                case.loss = loss
                with pytest.raises(_native.SlkError, match='ping-ponged'):
                    wc.train(be, dev, case, 0, case.N, B, weights=None)
            case.loss = LOSS
    assert dev.optim.step == 0
    wc.assert_same_tables(pre, wc.read(be, dev), 'a call refused inside the ping-pong scope')


def check_all_ones_is_the_unweighted_staged_call(be, kind, D=24, n=3, I=333):
    case = make_case(D, n, I)
    hp = hyper(kind)
    ones = np.ones(case.N, np.float32)
    with be.engine.options(**LAUNCH):
        a, b = (wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0) for _ in range(2))
        la, lb = wc.train(be, a, case, 0, case.N, B, weights=ones), wc.train(be, b, case, 0, case.N, B, weights=None)
    wc.assert_same_tables(wc.read(be, a), wc.read(be, b), ('all ones', kind))
    np.testing.assert_allclose(la, lb, rtol=1e-6)
    assert (lb > 0).all()


def check_power_of_two_scaling(be, kind='adagrad', D=24, n=3, I=333):
    case = make_case(D, n, I)
    hp = hyper(kind)
    out = []
    for scale in (1.0, 4.0):
        dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
        out.append((wc.train(be, dev, case, 0, case.N, B, scale=scale), wc.read(be, dev)))
    wc.assert_same_tables(out[0][1], out[1][1], 'weights and 4 * weights')
    assert wc.same_bits(out[0][0], out[1][0])


# ---- 4. degenerate columns -------------------------------------------------------------------------------------------------------------------
def _zero_state(case):
    return [(np.zeros(np.shape(case.params[t]), np.float32), np.zeros(np.shape(case.params[t]), np.float32)) for t in range(4)]


def check_nothing_is_live(be, kind, route, how, D=24, n=5):
    """how 'two_items': I = 2, the weight is log(max(1, 1 // (t + 1))) = 0 everywhere.  how 'no_violator': the candidates' item
    biases at -100 (candidates disjoint from the positives).  After a step every table and state array holds its bits and the
    reported loss is 0 -- from a zero state under SparseAdam (which decays the moments of a looked-up row whatever its gradient)."""
    I = 2 if how == 'two_items' else 333
    case = make_case(D, n, I)
    if how == 'no_violator':
        case.items %= I // 2
        case.negs = I // 2 + case.negs % (I - I // 2)
        case.params[3] = np.array(case.params[3], np.float64)
        case.params[3][I // 2:] = -100.0
    hp = hyper(kind)
    with be.engine.options(**(LAUNCH if route == 'launch' else {})):
        dev = wc.fresh(be, case, kind, hp, state=_zero_state(case) if kind == 'sparse_adam' else wc.start_state(case, kind), step=STEP0)
        pre = wc.read(be, dev)
        losses = _profiled_route(be, route, lambda: wc.train(be, dev, case, 0, case.N, B, weights=None))
    assert dev.optim.step == STEP0 + 5
    assert (losses == 0.0).all(), losses
    wc.assert_same_tables(pre, wc.read(be, dev), (how, kind, route))


def _all_violate_case(D, n, I, nan_row0=False):
    """Positives among the lower half of the catalogue with item biases -100, candidates among the upper half: x_0 ~ 101 > 0 in
    every column, so t = 0 everywhere."""
    case = make_case(D, n, I)
    case.items %= I // 2
    case.negs = I // 2 + case.negs % (I - I // 2)
    case.params[3] = np.array(case.params[3], np.float64)
    case.params[3][:I // 2] = -100.0
    return case


def check_every_column_violates_at_row_zero(be, route, D=24, n=5, I=333):
    """One minibatch of SGD at lr = 1 through the training route: g is +-logf(I - 1) / bm on exactly the positive and row 0 of each
    column.  Read from the item biases: a positive's moves by +count * g, a row-0 draw's by -count * g (flat draws 0 .. bm - 1 are
    row 0), and an item that is only drawn in rows >= 1 keeps every bit of its bias AND its embedding row."""
    case = _all_violate_case(D, n, I)
    bm = B
    with be.engine.options(**(LAUNCH if route == 'launch' else {})):
        dev = wc.fresh(be, case, 'sgd', dict(lr=1.0))
        pre = wc.read(be, dev)
        loss = _profiled_route(be, route, lambda: wc.train(be, dev, case, 0, bm, B, weights=None))
    post = wc.read(be, dev)
    g = np.log(np.float64(I - 1)) / bm
    pos, row0, later = case.items[:bm], case.negs[:bm], case.negs[bm:bm * n]
    want = pre[3][0].astype(np.float64).ravel() + g * np.bincount(pos, minlength=I) - g * np.bincount(row0, minlength=I)
    got = post[3][0].astype(np.float64).ravel()
    # fp32: the bias and each of its <= count updates round once, at the magnitude of the bias (|b| <= 101)
    tol = 1e-5 * np.maximum(np.abs(want), g)
    assert (np.abs(got - want) <= tol).all(), float(np.abs(got - want).max())
    idle = np.setdiff1d(later, np.concatenate([row0, pos]))
    assert idle.size > 0
    assert wc.same_bits(post[3][0].ravel()[idle], pre[3][0].ravel()[idle]) and wc.same_bits(post[1][0][idle], pre[1][0][idle])
    assert not wc.same_bits(post[1][0][np.unique(row0)], pre[1][0][np.unique(row0)])
    # the loss: mean over the columns of log(I - 1) * x_0 in float64 from the pre-step tables
    P = [torch.from_numpy(np.asarray(pre[t][0], np.float64)) for t in range(4)]
    want_loss, _ = restate_loss(P, case.users[:bm], case.items[:bm], case.negs[:bm * n], None, n, I)
    assert abs(float(loss[0]) - float(want_loss)) <= 1e-5 * float(want_loss)


def check_nan_candidate_is_skipped(be, route, D=24, n=3, I=333):
    """An item whose bias is NaN scores NaN wherever it is drawn: it does not violate, is never selected, and the call ends where
    the same call ends with that bias at -100 (never a violator either) -- every bit but that one bias."""
    out = []
    for bias in (np.nan, -100.0):
        case = make_case(D, n, I)
        z = I - 1
        case.items[case.items == z] = 0
        case.negs[::4] = z  # every row of the [n, bm] matrix holds it somewhere, row 0 included
        case.params[3] = np.array(case.params[3], np.float64)
        case.params[3][z] = bias
        with be.engine.options(**(LAUNCH if route == 'launch' else {})):
            dev = wc.fresh(be, case, 'adagrad', hyper('adagrad'), state=wc.start_state(case, 'adagrad'), step=STEP0)
            losses = wc.train(be, dev, case, 0, case.N, B, weights=None)
        tabs = wc.read(be, dev)
        assert np.isfinite(losses).all() and (losses > 0).all()
        for t in range(4):
            for k in range(3):
                x = tabs[t][k].ravel().copy()
                if t == 3:
                    x[z] = 0.0
                assert np.isfinite(x).all(), ('a NaN spread', t, k)
                tabs[t][k] = x
        out.append((losses, tabs))
    assert wc.same_bits(out[0][0], out[1][0])
    wc.assert_same_tables(out[0][1], out[1][1], ('NaN candidate', route))


# ---- 5. fold-in ---------------------------------------------------------------------------------------------------------------------------------
class Problem(fc.Problem):
    """foldin_checks.Problem under warp with n candidates per position."""

    def __init__(self, D, I, H, T, n=3, seed=0, lengths=None):
        rs = np.random.RandomState(2000 + 7 * D + 3 * I + H + 11 * n + seed)
        self.D, self.I, self.H, self.loss, self.T, self.nn = D, I, H, LOSS, T, n
        lens = np.asarray(fc.history_lengths(D, H) if lengths is None else lengths, dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.n = int(self.off[-1])
        self.items = rs.randint(0, I, self.n).astype(np.int64)
        self.neg = rs.randint(0, I, (T, n, self.n)).astype(np.int64)
        sc = min(0.3, 1.0 / np.sqrt(D))
        self.V = rs.normal(0, sc, (I, D)).astype(np.float32)
        self.bi = rs.normal(0, 0.1, I).astype(np.float32)
        self.U = rs.normal(0, sc, (H, D)).astype(np.float32)
        self.b = rs.normal(0, 0.1, H).astype(np.float32)


class Fold(fc.Fold):
    def run(self, n_steps, t0=0, want_loss=True):
        be, pr = self.be, self.pr
        neg = pr.neg[t0:t0 + n_steps]
        d_neg = be.alloc(neg if neg.size else np.zeros(1, np.int64))
        d_loss = be.alloc(np.full((n_steps, pr.H), np.nan, dtype=np.float32)) if want_loss else None
        be.engine.bilinear_foldin(self.tables, self.optim, be.ptr(self.d_off), be.ptr(self.d_items), pr.H, pr.n, pr.loss, pr.nn,
                                  n_steps, be.ptr(d_neg), be.ptr(d_loss), be.stream)
        self.assert_frozen()
        return be.get(d_loss).copy() if want_loss else None


def restate_fold_user(opt, hp, pr, pre, u, t, step0):
    """ONE step of user u alone (a one-user minibatch over the frozen item tables): (loss, post of the row and the bias, g, min |x|)."""
    o0, o1 = int(pr.off[u]), int(pr.off[u + 1])
    m = o1 - o0
    full = [(pre[0][u:u + 1], pre[2][u:u + 1], pre[4][u:u + 1]), (pr.V, None, None), (pre[1][u:u + 1], pre[3][u:u + 1], pre[5][u:u + 1]),
            (pr.bi, None, None)]
    P = [torch.from_numpy(np.array(full[k][0], dtype=np.float64)).requires_grad_(k in (0, 2)) for k in range(4)]
    # neg[t] is [n, m] row-major: flat entry r * m + c is row r of column c, the view(n, m) of the reference
    scores = []
    L, xmin = restate_loss(P, np.zeros(m, np.int64), pr.items[o0:o1], pr.neg[t, :, o0:o1].ravel(), None, pr.nn, pr.I, keep=scores)
    L.backward()
    g = {k: P[k].grad.numpy().copy() for k in (0, 2)}
    # The user's bias enters every score of the one-user minibatch, so its gradient is the sum of dL/dscore over the positives and
    # the candidates: column by column -w_c / m + w_c / m, exactly 0.  Autograd adds the positives' and the candidates' shares
    # as two separate sums and leaves a residue of 1e-17, which Adagrad and Adam from a zero state turn into a step of lr / 10:
    # the sum is restated here in the order in which it cancels (per column first), as the CPU oracle adds it for the other losses
    g[2] = (scores[0].grad + scores[1].grad.sum(0)).sum().reshape(1).numpy().copy()
    post = {k: oc.torch_step64(opt, hp, full[k][0], full[k][1], full[k][2], step0, g[k], np.zeros(1, np.int64)) for k in (0, 2)}
    return float(L.item()), post, g, xmin


def fold_closed_loop(be, pr, opt, route, steps):
    hp = hyper(opt)
    adam = opt in ('sparse_adam', 'adam_dense')
    with fc.routed(be, route):
        fold = Fold(be, pr, opt)
        for t in range(steps):
            pre = fold.result()
            got_loss = fold.run(1, t0=t)[0]
            assert fold.optim.step == t + 1
            got = fold.result()
            # Every user against their own one-user step; |want|inf of "1e-5 of the tensor's largest magnitude" is taken over the
            # TENSOR the call updates -- all users' rows, all users' biases -- as weights_checks.assert_within takes it over a
            # table.  (Per user it would be one bias: where two Adagrad steps of lr nearly cancel, that element's own magnitude
            # is below half an ulp of its operands, and no fp32 evaluation can meet 1e-5 of it.)
            cases = []
            for u in range(pr.H):
                m = int(pr.off[u + 1] - pr.off[u])
                what = (opt, pr.D, pr.I, pr.H, pr.nn, 'route', route, 'step', t, 'user', u, 'm', m)
                if m == 0:
                    assert got_loss[u] == 0.0, what
                    for x, y in zip(got, pre):
                        assert fc.same_bits(x[u], y[u]), what
                    continue
                want_loss, post, g, xmin = restate_fold_user(opt, hp, pr, pre, u, t, t)
                assert_guard(xmin, what)
                assert abs(float(got_loss[u]) - want_loss) <= 1e-5 * abs(want_loss), (what, float(got_loss[u]), want_loss)
                zV, zb = np.zeros_like(pr.V), np.zeros_like(pr.bi)
                pre_p = [pre[0][u:u + 1], pr.V, pre[1][u:u + 1], pr.bi]
                pre_s1 = [pre[2][u:u + 1], zV, pre[3][u:u + 1], zb]
                pre_s2 = [pre[4][u:u + 1], zV, pre[5][u:u + 1], zb]
                gs = [g[0], zV.astype(np.float64), g[2], zb.astype(np.float64)]
                bounds = ec.step_update_bounds(opt, hp, pre_p, pre_s1, pre_s2, gs, t + 1, rel_delta=1e-5, abs_delta=fc.cancellation_floor(pr))
                cases.append((u, what, post, bounds))
            slots = [(tab, k, nm, gi) for tab, idx in ((0, (0, 2, 4)), (2, (1, 3, 5))) for k, (nm, gi) in enumerate(zip(('param', 'state1', 'state2'), idx))
                     if not ((nm == 'state2' and not adam) or (nm == 'state1' and opt == 'sgd'))]
            for tab, k, nm, gi in slots:
                norm = max([np.abs(np.asarray(post[tab][k], np.float64)).max() for _, _, post, _ in cases] + [1e-30])
                for u, what, post, bounds in cases:
                    w64 = np.asarray(post[tab][k], np.float64).ravel()
                    d = np.abs(got[gi][u].astype(np.float64).ravel() - w64)
                    tol = 1e-5 * norm + np.asarray(bounds[tab][k], np.float64).ravel()
                    assert not (d > tol).any(), (what, tab, nm, float(d.max()), float(tol.min()))


def wide_problem(D, n, steps=2, I=333):
    return Problem(D, I, len(fc.WIDE_LENGTHS), steps, n=n, seed=FOLD_WIDE_SEEDS.get((D, n), 0), lengths=fc.WIDE_LENGTHS)


def check_fold_closed_loop(be, opt, D, I, H, n, steps=2, pr=None):
    pr = pr or Problem(D, I, H, steps, n=n, seed=FOLD_SEEDS.get((D, I, H, n), 0))
    for route in fc.ROUTES:
        fold_closed_loop(be, pr, opt, route, steps)


def check_fold_seed_meets_the_guard(D, I, H, n, steps=2, opt='sgd', pr=None):
    """No engine: every user's hinge arguments over the steps of the float64 restatement alone, 2 * GUARD away from 0 (SGD's
    trajectory; the closed loop asserts GUARD on every step of every optimizer's own)."""
    pr = pr or Problem(D, I, H, steps, n=n, seed=FOLD_SEEDS.get((D, I, H, n), 0))
    z = lambda x: np.zeros(np.shape(x), np.float32)
    pre = [pr.U.copy(), pr.b.copy(), z(pr.U), z(pr.b), z(pr.U), z(pr.b)]
    for t in range(steps):
        nxt = [x.copy() for x in pre]
        for u in range(pr.H):
            if pr.off[u + 1] > pr.off[u]:
                _, post, _, xmin = restate_fold_user(opt, hyper(opt), pr, pre, u, t, t)
                assert_guard(xmin, (D, I, H, n, 'step', t, 'user', u), 2 * GUARD)
                nxt[0][u], nxt[1][u] = post[0][0][0], post[2][0][0]
        pre = nxt


def check_fold_batch_composition(be, opt, D, I, n, H=5, T=2):
    pr = Problem(D, I, H, T, n=n)
    perm = list(np.random.RandomState(5).permutation(H))
    for route in fc.ROUTES:
        with fc.routed(be, route):
            whole = Fold(be, pr, opt)
            whole_loss = whole.run(T)
            want = whole.result()
            for u in range(H):
                one = Fold(be, pr.subset([u]), opt)
                one_loss = one.run(T)
                assert fc.same_bits(one_loss[:, 0], whole_loss[:, u]), ('loss of user alone', u, route)
                for x, y in zip(one.result(), want):
                    assert fc.same_bits(x[0], y[u]), ('user alone', u, route)
            mixed = Fold(be, pr.subset(perm), opt)
            mixed_loss = mixed.run(T)
            assert fc.same_bits(mixed_loss, whole_loss[:, perm]), ('loss, permuted users', route)
            for x, y in zip(mixed.result(), want):
                assert fc.same_bits(x, y[perm]), ('permuted users', route)
            assert not fc.same_bits(want[0], pr.U)


def check_fold_step_composition(be, opt, D, I, n, H=5, T=3):
    pr = Problem(D, I, H, T, n=n)
    for route in fc.ROUTES:
        with fc.routed(be, route):
            once = Fold(be, pr, opt)
            once_loss = once.run(T)
            stepwise = Fold(be, pr, opt)
            losses = [stepwise.run(1, t0=t)[0] for t in range(T)]
            assert stepwise.optim.step == once.optim.step == T
            assert fc.same_bits(np.stack(losses), once_loss), ('losses', route)
            for x, y in zip(stepwise.result(), once.result()):
                assert fc.same_bits(x, y), ('T calls of one step against one call of T', route)


def check_fold_frozen(be, opt, D=24, I=333, H=5, n=5):
    pr = Problem(D, I, H, 3, n=n)
    for route in fc.ROUTES:
        with fc.routed(be, route):
            fold = Fold(be, pr, opt)
            fold.run(3)  # (asserts the frozen side)
            assert not fc.same_bits(fold.result()[0], pr.U), 'nothing was trained'


def check_fold_degenerate(be, D=24, n=5):
    """The fold-in gather's latch: I = 2 and no violator anywhere leave row, bias and state bit-unchanged with loss 0; every
    candidate violating at r = 0 gives g = +-logf(I - 1) / m on the positive and row 0 -- read from the loss and from one SGD
    step at lr = 1 on the row; a NaN candidate is skipped."""
    lengths = [37, 0, 3, 300, 1]
    for route in fc.ROUTES:
        with fc.routed(be, route):
            for how in ('two_items', 'no_violator'):
                I = 2 if how == 'two_items' else 333
                pr = Problem(D, I, len(lengths), 2, n=n, lengths=lengths)
                if how == 'no_violator':
                    pr.items %= I // 2
                    pr.neg = I // 2 + pr.neg % (I - I // 2)
                    pr.bi[I // 2:] = -100.0
                for opt in ('adagrad', 'sgd', 'sparse_adam'):
                    fold = Fold(be, pr, opt)
                    pre = fold.result()
                    loss = fold.run(2)
                    assert (loss == 0.0).all(), (how, opt, route, loss)
                    for x, y in zip(fold.result(), pre):
                        assert fc.same_bits(x, y), (how, opt, route)
            # every candidate violates at r = 0
            I = 333
            pr = Problem(D, I, len(lengths), 1, n=n, lengths=lengths)
            pr.items %= I // 2
            pr.neg = I // 2 + pr.neg % (I - I // 2)
            pr.bi[:I // 2] = -100.0
            fold = Fold(be, pr, 'sgd', hp=dict(lr=1.0))
            loss = fold.run(1)[0]
            row, bias = fold.result()[:2]
            V, bi, Uu = pr.V.astype(np.float64), pr.bi.astype(np.float64), pr.U.astype(np.float64)
            w = np.log(np.float64(I - 1))
            for u, m in enumerate(lengths):
                if m == 0:
                    continue
                o0 = int(pr.off[u])
                ip, i0 = pr.items[o0:o0 + m], pr.neg[0, 0, o0:o0 + m]
                x0 = (V[i0] - V[ip]) @ Uu[u] + bi[i0] - bi[ip] + 1.0
                assert abs(float(loss[u]) - w * x0.mean()) <= 1e-5 * w * x0.mean(), (route, u)
                want_row = Uu[u] - (w / m) * (V[i0] - V[ip]).sum(0)
                # a sum of 2 m fp32 products of magnitude <= (w / m) |V|max, and the row itself: 1e-5 of the larger
                tol = 1e-5 * max(np.abs(want_row).max(), w * np.abs(V).max())
                assert np.abs(row[u].astype(np.float64) - want_row).max() <= tol, (route, u)
                assert abs(float(bias[u]) - float(pr.b[u])) <= 1e-5 * w  # (+g and -g on the user's bias)
            # a NaN candidate
            out = []
            for value in (np.nan, -100.0):
                pr = Problem(D, I, len(lengths), 2, n=3, lengths=lengths)
                z = I - 1
                pr.items[pr.items == z] = 0
                pr.neg.reshape(-1)[::4] = z
                pr.bi[z] = value
                fold = Fold(be, pr, 'adagrad')
                loss = fold.run(2)
                assert np.isfinite(loss).all()
                out.append([loss] + fold.result())
            for x, y in zip(*out):
                assert np.isfinite(x).all() and fc.same_bits(x, y), ('NaN candidate', route)


# ---- 7. refusals through the C ABI ------------------------------------------------------------------------------------------------------------
def check_refusals(be):
    eng = be.engine
    case = make_case(8, 3, 40, N=200)
    dev = wc.fresh(be, case, 'adagrad', hyper('adagrad'))
    d_u, d_i, d_n = be.alloc(case.users), be.alloc(case.items), be.alloc(case.negs)
    d_r, d_w = be.alloc(np.ones(case.N, np.float32)), be.alloc(case.weights)
    mb_loss = be.alloc(np.zeros(4, dtype=np.float32))
    pre = wc.read(be, dev)
    P = be.ptr

    def refused(match, fn):
        with pytest.raises(_native.SlkError, match=match) as e:
            fn()
        assert e.value.code == _native.SLK_EINVAL
        assert dev.optim.step == 0
        wc.assert_same_tables(pre, wc.read(be, dev), match)

    for n_neg in (0, -1):
        refused('num_negative_samples', lambda: eng.bilinear_train(dev.tables, dev.optim, P(d_u), P(d_i), case.N, 64, LOSS, n_neg, P(mb_loss),
                                                                  d_neg_in=P(d_n), stream=be.stream))
        refused('num_negative_samples', lambda: eng.bilinear_train_weighted(dev.tables, dev.optim, P(d_u), P(d_i), P(d_w), case.N, 64, LOSS,
                                                                           n_neg, P(mb_loss), d_neg_in=P(d_n), stream=be.stream))
    refused('warp', lambda: eng.bilinear_train_explicit(dev.tables, dev.optim, P(d_u), P(d_i), P(d_r), case.N, 64, LOSS, P(mb_loss),
                                                        stream=be.stream))
    refused('ratings go with', lambda: eng.bilinear_train_weighted(dev.tables, dev.optim, P(d_u), P(d_i), P(d_w), case.N, 64, LOSS, 3,
                                                                  P(mb_loss), d_ratings=P(d_r), d_neg_in=P(d_n), stream=be.stream))
    # the sequence entry: PoolNet tables over the same buffers (item embeddings, item biases)
    seq = be.seq_model([case.params[1], case.params[3]], opt='adagrad')
    d_s = be.alloc(np.random.RandomState(1).randint(1, case.I, (8, 5)).astype(np.int64))
    seq_pre = [be.get(x).copy() for x in seq.p]
    with pytest.raises(_native.SlkError, match='warp') as e:
        eng.poolnet_train(seq.tables, seq.optim, 0, P(d_s), 8, 5, 4, LOSS, 3, P(mb_loss), stream=be.stream)
    assert e.value.code == _native.SLK_EINVAL and seq.optim.step == 0
    assert all(wc.same_bits(be.get(x), y) for x, y in zip(seq.p, seq_pre))
    # the row-sharded train entry: warp is answered before anything else of the call is looked at
    with pytest.raises(_native.SlkError, match='warp') as e:
        eng._check(eng._lib.slk_shard_user_pass(eng._ctx, None, None, None, 0, 64, _native.LOSS_KINDS[LOSS], None, None, None, 0, None))
    assert e.value.code == _native.SLK_EINVAL
    # fold-in: n_neg < 1
    pr = Problem(24, 333, 5, 1)
    fold = Fold(be, pr, 'adagrad')
    pr.nn = 0
    with pytest.raises(_native.SlkError, match='warp needs n_neg >= 1') as e:
        fold.run(1)
    assert e.value.code == _native.SLK_EINVAL and fold.optim.step == 0 and fc.same_bits(fold.result()[0], pr.U)
    pr.nn = 3
    # ... and the same arguments, made good, are answered
    fold.run(1)
    eng.bilinear_train(dev.tables, dev.optim, P(d_u), P(d_i), case.N, 64, LOSS, 3, P(mb_loss), d_neg_in=P(d_n), stream=be.stream)
    assert dev.optim.step == 4 and fold.optim.step == 1
