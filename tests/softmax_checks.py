"""loss='softmax' (include/spotlight_hip.h: SLK_LOSS_SOFTMAX) -- backend-agnostic checks, run on the emulator build by
tests/test_emu_softmax.py and on the gfx950 library by tests/test_gpu_softmax.py; the model level is tests/test_host_softmax.py.

THE REFERENCE (restate_loss / restate_step) is a float64 torch restatement of the definition written here, in the manner of
warp_checks.restate_step: the BilinearNet forward on float64 leaves, each positive against ITS OWN n draws (flat draw f of a
minibatch is negative f % n of interaction f // n), torch.logsumexp, autograd, and torch's own optimizer classes for the step
(optim_checks.torch_step64).  Closed loop: before each minibatch the engine's tables and state go to torch, which takes that
one step.

THE BOUNDS are the project's: loss within 1e-5 relative; every element of every table / state tensor within
engine_checks.step_update_bounds at rel_delta = 1e-5 plus 1e-5 of the tensor's largest magnitude (weights_checks.assert_within).
The loss is smooth: there is no tie guard.  The 7-item cases alone add the project's floor for exactly cancelling sums by
warp_checks.cancellation_floor's rule: per interaction sum_j |dL/ds_j| = 2 (1 - p_0) / bm <= 2 / bm, each times a factor of
magnitude <= max(1, |table|max), so the terms of an element's gradient add up to at most S = 2 max(1, |U|max, |V|max) and the
floor is 2 ulp of S = S * 2^-22."""
import numpy as np
import pytest
import torch

import engine_checks as ec
import optim_checks as oc
import warp_checks as wk
import weights_checks as wc
from spotlight_amd import _native

LOSS = 'softmax'
KINDS = wk.KINDS           # ('adagrad', 'sgd', 'sparse_adam', 'adam_dense', 'adagrad_dense')
DS = wk.DS                 # (6, 24, 64, 72): the four row layouts
NS = (1, 3, 5)
U, N, B = 37, 300, 64      # five minibatches, the last of 44
STEP0 = 7
LAUNCH = dict(epoch_kernel=0)
SEED = 5

# (kind, D, n, I) of the closed loop, rotated as warp_checks.CLOSED rotates them: adagrad every (D, n) at I = 333; the other kinds
# every D once with n rotating; every kind the 7-item catalogue at n = 5, D rotating; one case at n = 130: NP = 131 takes
# k_softmax_loss<64> alone, in its strided form (two full trips of the wavefront and three pairs of a third).  NS takes G = 2, 4, 8;
# G = 16, 32, 64 with one pair per lane, NP a multiple of 64 and the cap are in tests/wide_negatives_checks.py
CLOSED = [('adagrad', D, n, 333) for D in DS for n in NS] + \
         [(k, D, NS[(i + j) % 3], 333) for j, k in enumerate(KINDS[1:]) for i, D in enumerate(DS)] + \
         [(k, DS[j % 4], 5, 7) for j, k in enumerate(KINDS)] + [('adagrad', 24, 130, 333)]


def hyper(kind):
    return wk.hyper(kind)


def make_case(D, n, I, seed=SEED, U=U, N=N, item_bloom=0):
    case = wc.make_case('adaptive_hinge', D, U=U, I=I, N=N, seed=seed, nn=n, item_bloom=item_bloom)  # (the draws are adaptive hinge's: N * n values)
    case.loss = LOSS
    return case


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _scores(P, users, items, negs, nn, own_user=True, idesc=None):
    tl = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))

    def emb_items(ids):  # (idesc: a BloomEmbedding item table -- an item's embedding is the sum of its hashed rows)
        rows = wc._item_rows(idesc, P[1].shape[0], ids)
        return P[1][tl(ids)] if rows is None else P[1][tl(rows)].sum(1)
    score = lambda us, its: (P[0][tl(us)] * emb_items(its)).sum(1) + P[2][tl(us)] + P[3][tl(its)]
    bm = len(users)
    flat = score(np.repeat(users, nn), negs)  # flat draw f is scored with user f // nn, whichever the layout
    # own_user: row r of column c is draw c * nn + r, the c-th user's own.  Else the reference's view(n, B): draw r * bm + c
    return score(users, items), (flat.view(bm, nn).t() if own_user else flat.view(nn, bm))


def restate_loss(P, users, items, negs, weights, nn, own_user=True, idesc=None):
    """The minibatch loss on torch leaves P.  weights None: the plain mean."""
    pos, neg = _scores(P, users, items, negs, nn, own_user, idesc)
    l = torch.logsumexp(torch.cat([pos.unsqueeze(0), neg], 0), 0) - pos
    if weights is None:
        return l.mean()
    w = torch.from_numpy(np.asarray(weights, np.float64)).to(P[0].dtype)
    return (w * l).sum() / w.sum()


def restate_step(kind, hp, pre, step0, users, items, negs, weights, nn, idesc=None):
    """ONE step from pre = [(p, s1, s2)] * 4 (fp32): (loss, post [(p, s1, s2)] * 4, dense gradients [g] * 4), float64."""
    P = [torch.from_numpy(np.array(pre[t][0], dtype=np.float64)).requires_grad_(True) for t in range(4)]
    L = restate_loss(P, users, items, negs, weights, nn, idesc=idesc)
    L.backward()
    g = [P[t].grad.numpy().copy() for t in range(4)]
    irows = np.concatenate([items, negs])
    tu, ti = np.unique(users), np.unique(irows)  # every looked-up row is touched (SparseAdam decays it)
    trows = ti
    if idesc is not None:  # (weights_checks.restate_step: the padding row takes no gradient, the touched rows are the hashed ones)
        g[1][idesc['padding_idx']] = 0.0
        trows = np.setdiff1d(np.unique(wc._item_rows(idesc, P[1].shape[0], irows)), [idesc['padding_idx']])
    post = [oc.torch_step64(kind, hp, pre[t][0], pre[t][1], pre[t][2], step0, g[t].reshape(pre[t][0].shape), touched)
            for t, touched in enumerate((tu, trows, tu, ti))]
    return float(L.item()), post, g


def cancellation_floor(case, pre):
    """abs_delta of step_update_bounds for the 7-ITEM cases only (the module docstring); every other case the bare bound."""
    if case.I != 7:
        return 0.0
    return 2.0 ** -22 * 2.0 * max(1.0, float(np.abs(pre[0][0]).max()), float(np.abs(pre[1][0]).max()))


def bounds_for(case, kind, hp, pre, g, step):
    return ec.step_update_bounds(kind, hp, [x[0] for x in pre], [x[1] for x in pre], [x[2] for x in pre],
                                 [g[t].reshape(pre[t][0].shape) for t in range(4)], step, rel_delta=1e-5,
                                 abs_delta=cancellation_floor(case, pre))


def _profiled_launch(be, fn):
    """fn() with the engine's profile on: it ran on the launch path -- no persistent launch, at least one user pass."""
    eng = be.engine
    eng.profile_reset()
    eng.profile_enable(True)
    try:
        out = fn()
    finally:
        eng.profile_enable(False)
    prof = eng.profile_read()
    assert prof['epoch'][0] == 0 and prof['user_pass'][0] >= 1, prof
    return out


# ---- 1. closed loop against the float64 restatement ---------------------------------------------------------------------------------------
def check_closed_loop(be, kind, D, n, I, weights=None, item_bloom=0):
    """A plain call, no option forced (it must take the launches by itself); weights 'case': slk_bilinear_train_weighted.
    item_bloom: the item table is a BloomEmbedding of that many hash functions -- its bias pass over the occurrence list of all
    1 + n occurrences, its row pass over the hashed one (never the late live list)."""
    case = make_case(D, n, I, item_bloom=item_bloom)
    hp = hyper(kind)
    w = case.weights if weights == 'case' else None
    dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
    step = STEP0
    for lo in range(0, case.N, B):
        hi = min(lo + B, case.N)
        pre = wc.read(be, dev)
        want_loss, post, g = restate_step(kind, hp, pre, step, case.users[lo:hi], case.items[lo:hi], case.negs[lo * n:hi * n],
                                          None if w is None else w[lo:hi], n, idesc=case.idesc)
        what = (kind, D, n, I, weights, item_bloom, 'minibatch at', lo)
        run = lambda: wc.train(be, dev, case, lo, hi, B, weights=w)
        got_loss = _profiled_launch(be, run) if w is None else run()
        step += 1
        assert dev.optim.step == step
        print('SOFTMAX closed loop', what, 'loss', float(got_loss[0]), want_loss)
        assert abs(float(got_loss[0]) - want_loss) <= 1e-5 * abs(want_loss), (what, float(got_loss[0]), want_loss)
        wc.assert_within(wc.read(be, dev), post, bounds_for(case, kind, hp, pre, g, step), kind, what)


def check_own_user_layout(be, D=8, n=2, I=40, bm=64):
    """Two users with opposite rows, every item row along the first user's: user 0 scores the upper half of the catalogue high,
    user 1 low.  Draws alternate between the halves so that an interaction's OWN draws and the draws the reference's view(n, B)
    puts in its column lie in different halves for half of the interactions: the two layouts' losses differ visibly, and the
    engine must give the own-user one."""
    rs = np.random.RandomState(11)
    case = make_case(D, n, I, U=2, N=bm)
    a = np.full(D, 0.7)
    bump = np.where(np.arange(I) >= I // 2, 1.0, -1.0)
    case.params = [np.stack([a, -a]), bump[:, None] * np.abs(rs.normal(0.7, 0.05, (I, D))), np.zeros(2), np.zeros(I)]
    case.users = (np.arange(bm) % 2).astype(np.int64)
    case.items = rs.randint(0, I, bm).astype(np.int64)
    # flat draw f: the upper half for the first bm draws, the lower half for the rest -- under own-user the first bm / n
    # interactions meet only upper-half items, under view(n, B) every column meets one of each
    case.negs = np.where(np.arange(bm * n) < bm, I // 2 + rs.randint(0, I // 2, bm * n), rs.randint(0, I // 2, bm * n)).astype(np.int64)
    P = [torch.from_numpy(np.asarray(p, np.float64).astype(np.float32).astype(np.float64)) for p in case.params]
    own = float(restate_loss(P, case.users, case.items, case.negs, None, n, own_user=True))
    col = float(restate_loss(P, case.users, case.items, case.negs, None, n, own_user=False))
    assert abs(own - col) > 0.05 * own, (own, col)
    hp = hyper('adagrad')
    dev = wc.fresh(be, case, 'adagrad', hp, state=wc.start_state(case, 'adagrad'), step=STEP0)
    pre = wc.read(be, dev)
    want_loss, post, g = restate_step('adagrad', hp, pre, STEP0, case.users, case.items, case.negs, None, n)
    got = wc.train(be, dev, case, 0, bm, bm, weights=None)
    assert abs(float(got[0]) - want_loss) <= 1e-5 * want_loss, (float(got[0]), want_loss, 'view(n, B) would give', col)
    assert abs(want_loss - own) <= 1e-12 * own
    wc.assert_within(wc.read(be, dev), post, bounds_for(case, 'adagrad', hp, pre, g, STEP0 + 1), 'adagrad', 'own-user layout')


# ---- 2. closed forms: one SGD step at lr = 1, read from the item biases -------------------------------------------------------------------
def check_all_zero_tables(be, n, D=24, I=333, bm=B):
    """All tables zero: every score is 0, every probability 1 / (n + 1).  The loss is log(n + 1); a negative occurrence moves its
    item's bias by -1 / ((n + 1) bm), a positive by +n / ((n + 1) bm)."""
    case = make_case(D, n, I)
    case.params = [np.zeros_like(np.asarray(p, np.float64)) for p in case.params]
    dev = wc.fresh(be, case, 'sgd', dict(lr=1.0))
    loss = wc.train(be, dev, case, 0, bm, B, weights=None)
    assert abs(float(loss[0]) - np.log(n + 1.0)) <= 1e-5 * np.log(n + 1.0), (float(loss[0]), np.log(n + 1.0))
    unit = 1.0 / ((n + 1.0) * bm)
    want = n * unit * np.bincount(case.items[:bm], minlength=I) - unit * np.bincount(case.negs[:bm * n], minlength=I)
    got = wc.read(be, dev)[3][0].astype(np.float64).ravel()
    # fp32: dL/dscore and each of an item's <= count additions round once, at the magnitude of the running sum
    tol = 1e-5 * np.maximum(np.abs(want), unit)
    assert (np.abs(got - want) <= tol).all(), float(np.abs(got - want).max())
    assert (want > 0).any() and (want < 0).sum() > bm // 2


def check_one_negative_is_softplus(be, kind='adagrad', D=24, I=333):
    """n = 1: l = log(e^s0 + e^s1) - s0 = softplus(s1 - s0), in float64 from the pre-step tables, within 1e-5."""
    case = make_case(D, 1, I)
    dev = wc.fresh(be, case, kind, hyper(kind), state=wc.start_state(case, kind), step=STEP0)
    pre = wc.read(be, dev)
    losses = wc.train(be, dev, case, 0, case.N, case.N, weights=None)
    P = [torch.from_numpy(np.asarray(pre[t][0], np.float64)) for t in range(4)]
    pos, neg = _scores(P, case.users, case.items, case.negs, 1)
    want = float(torch.nn.functional.softplus(neg[0] - pos).mean())
    assert abs(float(losses[0]) - want) <= 1e-5 * want, (float(losses[0]), want)


# ---- 3. stability ------------------------------------------------------------------------------------------------------------------------------
FP32_TINY = 2.0 ** -126


def check_stability(be, bias, opposite, kind='adagrad', D=24, n=5, I=333):
    """Positives among the lower half of the catalogue, whose item biases are set to `bias` (+100, then -100); candidates among
    the upper half -- as they are, or (`opposite`) at -bias: score gaps of 100 and of 200, either of which overflows expf without
    the max subtraction (e^88.8 is fp32's largest).  Every loss and every table element stays finite and the loss is within 1e-5
    relative of the float64 value: ~0 (n e^-100, n e^-200) and ~100 + log n, ~200 + log n.  The ~0 values lie below fp32's normal
    range, where the format itself cannot hold 1e-5 relative: there the comparison has the absolute floor 2^-126, the smallest
    normal fp32 -- from the number format alone."""
    case = make_case(D, n, I)
    case.items %= I // 2
    case.negs = I // 2 + case.negs % (I - I // 2)
    case.params[3] = np.array(case.params[3], np.float64)
    case.params[3][:I // 2] = bias
    if opposite:
        case.params[3][I // 2:] = -bias
    hp = hyper(kind)
    dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
    for lo in range(0, case.N, B):
        hi = min(lo + B, case.N)
        pre = wc.read(be, dev)
        P = [torch.from_numpy(np.asarray(pre[t][0], np.float64)) for t in range(4)]
        want = float(restate_loss(P, case.users[lo:hi], case.items[lo:hi], case.negs[lo * n:hi * n], None, n))
        got = float(wc.train(be, dev, case, lo, hi, B, weights=None)[0])
        print('SOFTMAX stability', bias, opposite, 'minibatch at', lo, 'loss', got, want)
        assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want) + FP32_TINY, (bias, opposite, lo, got, want)
        assert (want < 1e-30) if bias > 0 else (want > 99.0 * (2 if opposite else 1))
    for t, tab in enumerate(wc.read(be, dev)):
        for k in range(3):
            assert np.isfinite(tab[k]).all(), ('table', t, k)


# ---- 4. route, chunking, scopes, weights: bit for bit, engine against itself ---------------------------------------------------------------
def check_route(be, kind='adagrad', D=24, n=5, I=333):
    """A plain call at B = 64 -- where adaptive hinge takes the persistent kernel -- takes the launches with no option forced, and
    gives the bits of the same call with the persistent route switched off."""
    case = make_case(D, n, I)
    hp = hyper(kind)
    out = []
    for opts in ({}, LAUNCH):
        with be.engine.options(**opts):
            dev = wc.fresh(be, case, kind, hp, state=wc.start_state(case, kind), step=STEP0)
            losses = _profiled_launch(be, lambda: wc.train(be, dev, case, 0, case.N, B, weights=None))
            assert dev.optim.step == STEP0 + 5
            out.append((losses, wc.read(be, dev)))
    assert wc.same_bits(out[0][0], out[1][0])
    wc.assert_same_tables(out[0][1], out[1][1], 'plain call against epoch_kernel = 0')
    assert (out[0][0] > 0).all()


def check_chunking_and_determinism(be, weights, kind='adagrad', D=16, U=3000, I=1000, N=30000, B=1000, n=5, chunk=4096, seed=21):
    """warp_checks.check_chunking_and_determinism's shapes and settings: one chunk against chunks of 4096 interactions with the
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
    or not.  A user-row ping-pong scope serves the pair losses only: softmax is refused there in adaptive hinge's words, nothing
    is trained, and the scope still closes."""
    case = make_case(D, n, I)
    hp = hyper('adagrad')
    for weights in (None, 'case'):
        a, b = (wc.fresh(be, case, 'adagrad', hp, state=wc.start_state(case, 'adagrad'), step=STEP0) for _ in range(2))
        la = wc.train(be, a, case, 0, case.N, B, weights=weights)
        with be.engine.bias_shadow(b.tables, b.optim, stream=be.stream):
            lb = wc.train(be, b, case, 0, case.N, B, weights=weights)
        assert wc.same_bits(la, lb)
        wc.assert_same_tables(wc.read(be, a), wc.read(be, b), ('inside the item-bias shadow', weights))
    dev = wc.fresh(be, case, 'adagrad', hp)
    pre = wc.read(be, dev)
    with be.engine.user_pingpong(dev.tables, dev.optim, stream=be.stream):
        for loss in ('adaptive_hinge', LOSS):
            case.loss = loss
            with pytest.raises(_native.SlkError, match='ping-ponged'):
                wc.train(be, dev, case, 0, case.N, B, weights=None)
        case.loss = LOSS
    assert dev.optim.step == 0
    wc.assert_same_tables(pre, wc.read(be, dev), 'a call refused inside the ping-pong scope')
    # ... and the scope has closed: the same call now trains
    wc.train(be, dev, case, 0, case.N, B, weights=None)
    assert dev.optim.step == 5


def check_all_ones_is_the_unweighted_call(be, kind, D=24, n=3, I=333):
    case = make_case(D, n, I)
    hp = hyper(kind)
    ones = np.ones(case.N, np.float32)
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


# ---- 5. refusals through the C ABI -----------------------------------------------------------------------------------------------------------
def check_refusals(be):
    eng = be.engine
    case = make_case(8, 3, 40, N=200)
    dev = wc.fresh(be, case, 'adagrad', hyper('adagrad'))
    big = np.random.RandomState(2).randint(0, case.I, case.N * 1025).astype(np.int64)  # (n_neg = 1025 over buffers that hold it)
    d_u, d_i, d_n = be.alloc(case.users), be.alloc(case.items), be.alloc(big)
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

    for n_neg in (0, -1, 1025):
        refused('num_negative_samples', lambda: eng.bilinear_train(dev.tables, dev.optim, P(d_u), P(d_i), case.N, 64, LOSS, n_neg, P(mb_loss),
                                                                  d_neg_in=P(d_n), stream=be.stream))
        refused('num_negative_samples', lambda: eng.bilinear_train_weighted(dev.tables, dev.optim, P(d_u), P(d_i), P(d_w), case.N, 64, LOSS,
                                                                           n_neg, P(mb_loss), d_neg_in=P(d_n), stream=be.stream))
    refused('softmax', lambda: eng.bilinear_train_explicit(dev.tables, dev.optim, P(d_u), P(d_i), P(d_r), case.N, 64, LOSS, P(mb_loss),
                                                           stream=be.stream))
    refused('ratings go with', lambda: eng.bilinear_train_weighted(dev.tables, dev.optim, P(d_u), P(d_i), P(d_w), case.N, 64, LOSS, 3,
                                                                  P(mb_loss), d_ratings=P(d_r), d_neg_in=P(d_n), stream=be.stream))
    # the sequence entry keeps its answer for an id it does not know: PoolNet tables over the same buffers
    seq = be.seq_model([case.params[1], case.params[3]], opt='adagrad')
    d_s = be.alloc(np.random.RandomState(1).randint(1, case.I, (8, 5)).astype(np.int64))
    seq_pre = [be.get(x).copy() for x in seq.p]
    with pytest.raises(_native.SlkError, match='unknown loss kind 8') as e:
        eng.poolnet_train(seq.tables, seq.optim, 0, P(d_s), 8, 5, 4, LOSS, 3, P(mb_loss), stream=be.stream)
    assert e.value.code == _native.SLK_EINVAL and seq.optim.step == 0
    assert all(wc.same_bits(be.get(x), y) for x, y in zip(seq.p, seq_pre))
    # the row-sharded train entry: softmax is answered before anything else of the call is looked at
    with pytest.raises(_native.SlkError, match='softmax') as e:
        eng._check(eng._lib.slk_shard_user_pass(eng._ctx, None, None, None, 0, 64, _native.LOSS_KINDS[LOSS], None, None, None, 0, None))
    assert e.value.code == _native.SLK_EINVAL
    # fold-in: by name, before the histories are read
    pr = wk.Problem(24, 333, 5, 1)
    fold = wk.Fold(be, pr, 'adagrad')
    pr.loss = LOSS
    with pytest.raises(_native.SlkError, match='softmax') as e:
        fold.run(1)
    assert e.value.code == _native.SLK_EINVAL and fold.optim.step == 0 and wc.same_bits(fold.result()[0], pr.U)
    # ... and the same arguments, made good, are answered
    pr.loss = 'adaptive_hinge'
    fold.run(1)
    eng.bilinear_train(dev.tables, dev.optim, P(d_u), P(d_i), case.N, 64, LOSS, 3, P(mb_loss), d_neg_in=P(d_n), stream=be.stream)
    assert dev.optim.step == 4 and fold.optim.step == 1
