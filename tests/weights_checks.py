"""Interaction weights (include/spotlight_hip.h: slk_bilinear_train_weighted) -- backend-agnostic checks, run on the emulator build
by tests/test_emu_interaction_weights.py and on the gfx950 library by tests/test_gpu_interaction_weights.py.

THE ORACLE (restate_step) is a float64 torch restatement written here: the BilinearNet forward on float64 leaves, the weighted
loss  L = sum_i(w_i l_i) / sum_i(w_i)  through autograd, and torch's own optimizer classes for the step
(optim_checks.torch_step64).  It runs closed loop: before each minibatch the engine's tables and state go to torch, which takes
that one step.  With weights=None it is the reference's unweighted .mean() -- what the repetition check compares against, so that
check does not lean on the weighted formula at all.

THE BOUNDS are the project's: loss within 1e-5 relative; every element of every table / state tensor within
engine_checks.step_update_bounds at rel_delta = 1e-5 (+ 1e-5 of the tensor's largest magnitude, as assert_step_within_bounds has
it).  The optimizer state starts NON-ZERO (optim_checks.make_state), and no element is masked out.  That an fp32 evaluation of
the restatement itself stays inside these bounds is a check of its own (check_fp32_restatement_within_bounds: no engine)."""
import types

import numpy as np
import pytest
import torch

import engine_checks as ec
import optim_checks as oc

PAIR = ('pointwise', 'bpr', 'hinge')
EXPLICIT = ('regression', 'poisson', 'logistic')
LOSSES = PAIR + ('adaptive_hinge',) + EXPLICIT
KINDS = ('adagrad', 'sparse_adam', 'adam_dense', 'sgd')
DIMS = (12, 32, 64)
NN = 3
LAUNCH = dict(epoch_kernel=0, explicit_fused=0)  # the unweighted call on the launch path, staged where it can be


def hyper(kind):
    return dict(lr=0.05, weight_decay=1e-3) if kind.endswith('dense') else dict(lr=0.05)


def n_neg_of(loss, nn=NN):
    return nn if loss == 'adaptive_hinge' else (0 if loss in EXPLICIT else 1)


def make_weights(rs, n):
    return (2.0 ** rs.uniform(-6, 6, n)).astype(np.float32)


def make_case(loss, D, U=37, I=29, N=300, seed=5, item_bloom=0, nn=NN):
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    negs = rs.randint(0, I, N * max(n_neg_of(loss, nn), 1)).astype(np.int64)
    params, _, idesc = ec._bloom_setup(rs, U, I, D, 0, item_bloom, 0.5)
    ratings = ec._ratings_for(rs, loss, N).astype(np.float32) if loss in EXPLICIT else None
    return types.SimpleNamespace(loss=loss, D=D, U=U, I=I, N=N, users=users, items=items, negs=negs, params=params, idesc=idesc,
                                 ratings=ratings, weights=make_weights(rs, N), nn=n_neg_of(loss, nn))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _item_rows(case_idesc, rows, items):
    """[len(items), H] rows of the (compressed) item table behind each item id; None: a plain table."""
    if case_idesc is None:
        return None
    from oracle.oracle import bloom_indices
    return bloom_indices(items, case_idesc['seeds'], rows, case_idesc['padding_idx'])


def restate_loss(P, users, items, negs, weights, loss, nn, ratings=None, idesc=None):
    """The minibatch loss on torch leaves P (any float dtype): weights None -> the reference's .mean()."""
    dt = P[0].dtype
    tl = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))

    def emb_items(ids):
        rows = _item_rows(idesc, P[1].shape[0], ids)
        return P[1][tl(ids)] if rows is None else P[1][tl(rows)].sum(1)

    def score(us, its):
        return (P[0][tl(us)] * emb_items(its)).sum(1) + P[2][tl(us)] + P[3][tl(its)]
    pos = score(users, items)
    bm = len(users)
    if loss in EXPLICIT:
        r = torch.from_numpy(np.asarray(ratings, np.float64)).to(dt)
        if loss == 'regression':
            l = (r - pos) ** 2
        elif loss == 'poisson':
            p = torch.exp(pos)
            l = p - r * torch.log(p)
        else:
            l = torch.nn.functional.binary_cross_entropy_with_logits(pos, r.clamp(0, 1), reduction='none')
    elif loss == 'adaptive_hinge':
        # the reference's layout: users repeated user-major, ONE draw of B * n, scores viewed as [n, B]; column c keeps c's weight
        neg = score(np.repeat(users, nn), negs).view(nn, bm)
        l = torch.clamp(neg.max(0)[0] - pos + 1.0, min=0.0)
    else:
        neg = score(users, negs)
        if loss == 'pointwise':
            l = (1.0 - torch.sigmoid(pos)) + torch.sigmoid(neg)
        elif loss == 'bpr':
            l = 1.0 - torch.sigmoid(pos - neg)
        else:
            l = torch.clamp(neg - pos + 1.0, min=0.0)
    if weights is None:
        return l.mean()
    w = torch.from_numpy(np.asarray(weights, np.float64)).to(dt)
    return (w * l).sum() / w.sum()


def restate_step(kind, hp, pre, step0, users, items, negs, weights, loss, nn, ratings=None, idesc=None, dtype=torch.float64):
    """ONE step from pre = [(p, s1, s2)] * 4 (fp32): (loss, post [(p, s1, s2)] * 4, dense gradients [g] * 4), float64 numpy.
    dtype=torch.float32 evaluates forward, loss and backward in fp32 (the optimizer step stays torch's, in float64)."""
    P = [torch.from_numpy(np.array(pre[t][0], dtype=np.float64)).to(dtype).requires_grad_(True) for t in range(4)]
    L = restate_loss(P, users, items, negs, weights, loss, nn, ratings, idesc)
    L.backward()
    g = [P[t].grad.double().numpy().copy() for t in range(4)]
    if idesc is not None:
        g[1][idesc['padding_idx']] = 0.0  # nn.Embedding(padding_idx=...): the padding row takes no gradient
    irows = np.concatenate([items, negs]) if loss not in EXPLICIT else np.asarray(items)
    tu, ti = np.unique(users), np.unique(irows)
    trows = ti if idesc is None else np.setdiff1d(np.unique(_item_rows(idesc, P[1].shape[0], irows)), [idesc['padding_idx']])
    post = []
    for t, touched in enumerate((tu, trows, tu, ti)):
        p, s1, s2 = oc.torch_step64(kind, hp, pre[t][0], pre[t][1], pre[t][2], step0, g[t].reshape(pre[t][0].shape), touched)
        post.append((p, s1, s2))
    return float(L.item()), post, g


def assert_within(got, want, bounds, kind, what):
    """|got - want| <= 1e-5 * max|want| + step_update_bounds, every element of every tensor (engine_checks.assert_step_within_bounds)."""
    adam = kind in ('sparse_adam', 'adam_dense')
    for t in range(4):
        for k, nm in enumerate(('param', 'state1', 'state2')):
            if kind == 'sgd' and k > 0 or (k == 2 and not adam):
                continue
            w64 = np.asarray(want[t][k], np.float64)
            d = np.abs(np.asarray(got[t][k], np.float64).reshape(w64.shape) - w64)
            tol = 1e-5 * max(np.abs(w64).max(), 1e-30) + bounds[t][k].reshape(w64.shape)
            assert not (d > tol).any(), (what, 'table', t, nm, '%d elements beyond the bound' % int((d > tol).sum()),
                                         float((d / np.maximum(tol, 1e-300)).max()))


def bounds_for(kind, hp, pre, g, step):
    return ec.step_update_bounds(kind, hp, [x[0] for x in pre], [x[1] for x in pre], [x[2] for x in pre],
                                 [g[t].reshape(pre[t][0].shape) for t in range(4)], step)


# ---- engine plumbing ------------------------------------------------------------------------------------------------------------------------
def read(be, dev):
    return [[be.get(x[t]).copy() for x in (dev.p, dev.s1, dev.s2)] for t in range(4)]


def fresh(be, case, kind, hp, tabs=None, state=None, step=0):
    dev = be.model(case.params if tabs is None else tabs, opt=kind, item_bloom=case.idesc, **hp)
    for t in range(4 if state is not None else 0):
        oc.put(be, dev.s1[t], state[t][0])
        oc.put(be, dev.s2[t], state[t][1])
    dev.optim.step = step
    return dev


def start_state(case, kind):
    return [oc.make_state(kind, 1e-3 * np.asarray(case.params[t], np.float64), seed=23 + t) for t in range(4)]


def train(be, dev, case, lo, hi, B, weights='case', scale=1.0, n=None):
    """One engine call over interactions [lo, hi): weights 'case' / an array -> the weighted entry, None -> the unweighted ones.
    `n`: the call's n where it is not hi - lo (n = 0 over real buffers: an empty device buffer has a NULL pointer)."""
    n, nn = hi - lo if n is None else n, case.nn
    keep = [be.alloc(case.users[lo:hi]), be.alloc(case.items[lo:hi])]
    mb_loss = be.alloc(np.zeros(max((n + B - 1) // B, 1), dtype=np.float32))
    d_r = be.alloc(case.ratings[lo:hi]) if case.ratings is not None else None
    d_n = be.alloc(case.negs[lo * nn:hi * nn]) if nn else None
    if weights is None:
        if d_r is not None:
            be.engine.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(keep[0]), be.ptr(keep[1]), be.ptr(d_r), n, B, case.loss,
                                              be.ptr(mb_loss), stream=be.stream)
        else:
            be.engine.bilinear_train(dev.tables, dev.optim, be.ptr(keep[0]), be.ptr(keep[1]), n, B, case.loss, nn, be.ptr(mb_loss),
                                     d_neg_in=be.ptr(d_n), stream=be.stream)
    else:
        w = case.weights if isinstance(weights, str) else weights
        d_w = be.alloc((np.asarray(w[lo:hi], np.float32) * np.float32(scale)).astype(np.float32))
        be.engine.bilinear_train_weighted(dev.tables, dev.optim, be.ptr(keep[0]), be.ptr(keep[1]), be.ptr(d_w), n, B, case.loss, nn,
                                          be.ptr(mb_loss), d_ratings=be.ptr(d_r), d_neg_in=be.ptr(d_n), stream=be.stream)
    return be.get(mb_loss).copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_same_tables(x, y, what):
    for t in range(4):
        for k in range(3):
            assert same_bits(x[t][k], y[t][k]), (what, 'table', t, ('param', 'state1', 'state2')[k])


# ---- 1. closed loop against torch float64 -----------------------------------------------------------------------------------------------
def check_closed_loop(be, loss, kind, D, B=64, item_bloom=0, case=None, step0=7, weights='case'):
    case = case or make_case(loss, D, item_bloom=item_bloom)
    hp = hyper(kind)
    w = case.weights if isinstance(weights, str) else weights
    dev = fresh(be, case, kind, hp, state=start_state(case, kind), step=step0)
    step = step0
    for lo in range(0, case.N, B):
        hi = min(lo + B, case.N)
        pre = read(be, dev)
        want_loss, post, g = restate_step(kind, hp, pre, step, case.users[lo:hi], case.items[lo:hi],
                                          case.negs[lo * case.nn:hi * case.nn], w[lo:hi], loss, case.nn,
                                          case.ratings[lo:hi] if case.ratings is not None else None, case.idesc)
        got_loss = train(be, dev, case, lo, hi, B, weights=w)
        step += 1
        assert dev.optim.step == step
        assert abs(float(got_loss[0]) - want_loss) <= 1e-5 * abs(want_loss), (loss, kind, D, lo, float(got_loss[0]), want_loss)
        assert_within(read(be, dev), post, bounds_for(kind, hp, pre, g, step), kind, (loss, kind, D, 'minibatch at', lo))
    return dev


def check_fp32_restatement_within_bounds(loss, kind, D=32, B=64):
    """No engine: forward, loss and backward of the restatement in fp32 against float64, from the checks' own start state --
    the bound is one an fp32 evaluation meets with no element left out."""
    case = make_case(loss, D)
    hp = hyper(kind)
    st = start_state(case, kind)
    pre = [(np.asarray(case.params[t], np.float32).reshape(np.asarray(case.params[t]).shape), st[t][0], st[t][1]) for t in range(4)]
    args = (case.users[:B], case.items[:B], case.negs[:B * case.nn], case.weights[:B], loss, case.nn,
            case.ratings[:B] if case.ratings is not None else None)
    l64, post64, g = restate_step(kind, hp, pre, 7, *args)
    l32, post32, _ = restate_step(kind, hp, pre, 7, *args, dtype=torch.float32)
    assert abs(l32 - l64) <= 1e-5 * abs(l64)
    assert_within(post32, post64, bounds_for(kind, hp, pre, g, 8), kind, ('fp32 restatement', loss, kind))


# ---- 2. integer weights equal repetition ------------------------------------------------------------------------------------------------
def check_integer_weights_equal_repetition(be, loss, kind='adagrad', D=32, N=200, seed=13):
    """One minibatch (B = N), weights in {1, 2, 3}: the tables of the UNWEIGHTED float64 restatement on the list with interaction i
    repeated w_i times, its negative with it."""
    case = make_case(loss, D, N=N, seed=seed)
    rs = np.random.RandomState(seed + 1)
    w = rs.randint(1, 4, N)
    rep = np.repeat(np.arange(N), w)
    hp = hyper(kind)
    dev = fresh(be, case, kind, hp, state=start_state(case, kind), step=7)
    pre = read(be, dev)
    want_loss, post, g = restate_step(kind, hp, pre, 7, case.users[rep], case.items[rep], case.negs[rep], None, loss, 1)
    got_loss = train(be, dev, case, 0, N, N, weights=w.astype(np.float32))
    assert abs(float(got_loss[0]) - want_loss) <= 1e-5 * abs(want_loss)
    assert_within(read(be, dev), post, bounds_for(kind, hp, pre, g, 8), kind, ('repetition', loss))


# ---- 3. all ones is the unweighted call ---------------------------------------------------------------------------------------------------
def check_all_ones_is_the_unweighted_call(be, loss, kind, D=32, B=64):
    """Adaptive hinge and explicit feedback: the unweighted call is staged too (LAUNCH), and weights of 1.0 give its tables and
    state bit for bit.  The pair losses' unweighted call forms dL/dscore inside the user pass and adds a pair's two rows as
    gu += gp * vi + gn * vj (csrc/slk_bilinear.hip, k_user_pass, UMODE 0), the staged route row by row (UMODE 1: slk_vaxpy per live
    pair) -- another association of the same sum; they are held to the closed loop's bounds against each other instead."""
    case = make_case(loss, D)
    hp = hyper(kind)
    ones = np.ones(case.N, np.float32)
    with be.engine.options(**LAUNCH):
        if loss not in PAIR:
            a, b = (fresh(be, case, kind, hp, state=start_state(case, kind), step=7) for _ in range(2))
            la, lb = train(be, a, case, 0, case.N, B, weights=ones), train(be, b, case, 0, case.N, B, weights=None)
            assert_same_tables(read(be, a), read(be, b), ('all ones', loss, kind))
            np.testing.assert_allclose(la, lb, rtol=1e-6)
            return
        a = fresh(be, case, kind, hp, state=start_state(case, kind), step=7)
        step = 7
        for lo in range(0, case.N, B):
            hi = min(lo + B, case.N)
            pre = read(be, a)
            b = fresh(be, case, kind, hp, tabs=[x[0] for x in pre], state=[(x[1], x[2]) for x in pre], step=step)
            _, _, g = restate_step(kind, hp, pre, step, case.users[lo:hi], case.items[lo:hi], case.negs[lo:hi], None, loss, 1)
            la, lb = train(be, a, case, lo, hi, B, weights=ones), train(be, b, case, lo, hi, B, weights=None)
            step += 1
            np.testing.assert_allclose(la, lb, rtol=1e-6)
            assert_within(read(be, a), read(be, b), bounds_for(kind, hp, pre, g, step), kind, ('all ones', loss, kind, lo))


# ---- 4. power-of-two scaling ------------------------------------------------------------------------------------------------------------------
def check_power_of_two_scaling(be, loss, kind='adagrad', D=32, B=64):
    case = make_case(loss, D)
    hp = hyper(kind)
    out = []
    for scale in (1.0, 4.0):
        dev = fresh(be, case, kind, hp, state=start_state(case, kind), step=7)
        out.append((train(be, dev, case, 0, case.N, B, scale=scale), read(be, dev)))
    assert_same_tables(out[0][1], out[1][1], ('weights and 4 * weights', loss, kind))
    assert same_bits(out[0][0], out[1][0]), ('mb_loss under weights and 4 * weights', loss)


# ---- 5. chunking and determinism ------------------------------------------------------------------------------------------------------------
def check_chunking_and_determinism(be, loss, kind='adagrad', D=16, U=3000, I=1000, N=30000, B=1000, nn=5, chunk=4096, seed=21):
    """The shapes of engine_checks.check_chunking_is_bit_neutral: one chunk against chunks of 4096 interactions (4 minibatches)
    with the prep in line and on the second stream; and the same call twice from the same state."""
    eng = be.engine
    case = make_case(loss, D, U=U, I=I, N=N, seed=seed, nn=nn)
    hp = hyper(kind)
    results = []
    for chunk_i, overlap_i in ((1 << 23, 0), (1 << 23, 0), (chunk, 0), (chunk, 1)):
        eng.set_option('chunk_interactions', chunk_i)
        eng.set_option('overlap_prep', overlap_i)
        eng.set_option('overlap_min_batch', 0)
        try:
            dev = fresh(be, case, kind, hp, state=start_state(case, kind), step=7)
            losses = [train(be, dev, case, 0, N, B) for _ in range(2)]
            assert dev.optim.step == 7 + 2 * ((N + B - 1) // B)
            results.append((np.concatenate(losses), read(be, dev)))
        finally:
            eng.set_option('chunk_interactions', 1 << 23)
            eng.set_option('overlap_prep', 0)
            eng.set_option('overlap_min_batch', 1 << 16)
    for k, what in ((1, 'the same call again'), (2, 'chunks of %d, prep in line' % chunk), (3, 'chunks of %d, prep beside the passes' % chunk)):
        assert same_bits(results[0][0], results[k][0]), ('mb_loss differs:', what, loss)
        assert_same_tables(results[0][1], results[k][1], (what, loss))


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------------------
def check_tiny_calls(be, loss, kind='adagrad', D=12):
    """B = 1 (every minibatch one interaction: L = l_i whatever w_i), N = 1, and n = 0 (a no-op), against the restatement."""
    check_closed_loop(be, loss, kind, D, B=1, case=make_case(loss, D, N=5, seed=3))
    check_closed_loop(be, loss, kind, D, B=64, case=make_case(loss, D, N=1, seed=4))
    case = make_case(loss, D, N=4, seed=6)
    dev = fresh(be, case, kind, hyper(kind), state=start_state(case, kind), step=7)
    pre = read(be, dev)
    train(be, dev, case, 0, 4, 64, n=0)
    assert dev.optim.step == 7
    assert_same_tables(pre, read(be, dev), 'n = 0')


def check_long_user(be, loss, kind='adagrad', D=16, U=37, I=29, N=4096, seed=9):
    """One user holds half of a 4096-interaction minibatch: the user pass's long-run form and its stitch, against the restatement."""
    case = make_case(loss, D, U=U, I=I, N=N, seed=seed)
    case.users[np.random.RandomState(seed).permutation(N)[:N // 2]] = 3
    before = be.engine.get_stat('user_long_launches')
    check_closed_loop(be, loss, kind, D, B=N, case=case)
    assert be.engine.get_stat('user_long_launches') > before, 'the minibatch did not take the long-run form'


def check_refusals(be):
    from spotlight_amd import _native
    eng = be.engine
    case = make_case('bpr', 8, N=200)
    dev = fresh(be, case, 'adagrad', hyper('adagrad'))
    d_u, d_i, d_n = be.alloc(case.users), be.alloc(case.items), be.alloc(case.negs)
    d_w, d_r = be.alloc(case.weights), be.alloc(np.ones(case.N, np.float32))
    mb_loss = be.alloc(np.zeros(4, dtype=np.float32))
    call = lambda w, loss='bpr', r=None: eng.bilinear_train_weighted(
        dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), w, case.N, 64, loss, 1, be.ptr(mb_loss), d_ratings=r, d_neg_in=be.ptr(d_n),
        stream=be.stream)
    pre = read(be, dev)
    with pytest.raises(_native.SlkError, match='d_weights is NULL'):
        call(None)
    with pytest.raises(_native.SlkError, match='ratings go with'):
        call(be.ptr(d_w), 'bpr', be.ptr(d_r))
    with pytest.raises(_native.SlkError, match='ratings go with'):
        call(be.ptr(d_w), 'regression', None)
    # inside a user-row ping-pong scope: refused in so many words, nothing trained, and the scope still serves its own calls
    ref = fresh(be, case, 'adagrad', hyper('adagrad'))
    with eng.options(epoch_kernel=0):
        eng.bilinear_train(ref.tables, ref.optim, be.ptr(d_u), be.ptr(d_i), case.N, 64, 'bpr', 1, be.ptr(mb_loss), d_neg_in=be.ptr(d_n),
                           stream=be.stream)
        with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream):
            with pytest.raises(_native.SlkError, match='interaction weights'):
                call(be.ptr(d_w))
            assert dev.optim.step == 0
            eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), case.N, 64, 'bpr', 1, be.ptr(mb_loss),
                               d_neg_in=be.ptr(d_n), stream=be.stream)
    assert_same_tables(read(be, dev), read(be, ref), 'the ping-pong scope after a refused weighted call')
    assert not same_bits(pre[0][0], read(be, dev)[0][0])
    call(be.ptr(d_w))  # and outside the scope the call trains
    assert dev.optim.step == 8


def check_inside_bias_shadow(be, loss='bpr', D=16, B=64):
    """A weighted call inside an open item-bias shadow scope (Adagrad) gives the tables of the same call outside it, bit for bit."""
    case = make_case(loss, D)
    hp = hyper('adagrad')
    a, b = (fresh(be, case, 'adagrad', hp, state=start_state(case, 'adagrad'), step=7) for _ in range(2))
    la = train(be, a, case, 0, case.N, B)
    with be.engine.bias_shadow(b.tables, b.optim, stream=be.stream):
        lb = train(be, b, case, 0, case.N, B)
    assert same_bits(la, lb)
    assert_same_tables(read(be, a), read(be, b), ('inside the item-bias shadow', loss))
