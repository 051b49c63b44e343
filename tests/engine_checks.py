"""Backend-agnostic parity checks of the engine's C ABI against the CPU oracle / numpy /
the golden vectors.  `be` is a backend: tests/emu_backend.EmuBackend (fiber emulator, numpy
memory; runs anywhere) or tests/hip_backend.HipBackend (the real gfx950 library, torch device
memory; `-m gpu`)."""
import os

import numpy as np

from oracle.oracle import BilinearOracle, Rng
from oracle.replay import ORACLE_OPT, oracle_hparams

# open-loop drift bounds (assert_open_loop_drift): relative 2-NORM bounds, a coarse "no wrong update rule, no missed row" statement --
# NOT the parity pin (that is the closed loop: check_train_closed_loop / check_replays_reference_fixture, per element under
# step_update_bounds).  Measured over the 45 recordings (emulator build): embedding tables <= 6.5e-4, bias tables (a few hundred
# elements, where one sign-flipped first step shows) <= 6.7e-2
OPEN_LOOP_DRIFT_ROWS = 5e-3
OPEN_LOOP_DRIFT_BIAS = 0.2  # (20 % of the bias table's norm: coarse by design, see above)


def rel_inf(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def adagrad_well_conditioned(state_sum, rel=1e-6):
    """Elements whose Adagrad update is well-posed: the accumulator sum of g^2 is not ~0 next to the table's largest.  Where
    the only gradient an element ever saw is a residual of cancelling terms (|g| below `rel` of the table's gradient scale --
    often exactly 0 in one summation order and 1e-11 in another), lr * g / (sqrt(g^2) + 1e-10) turns that noise into
    anything up to lr: those elements are identified here BY THEIR GRADIENT MAGNITUDE and only bounded, not compared."""
    g = np.sqrt(np.asarray(state_sum, np.float64).ravel())
    return g > rel * max(g.max(), 1e-30)


def assert_open_loop_drift(got, ref, what, bound=None):
    """Open-loop replays (several epochs from zero accumulators, one engine call per epoch) are chaotic at the 1e-3 level element
    by element (see check_replays_reference_fixture), so what they pin is the loss trajectory; for the tables themselves this is a
    quota-free NORM statement: ||got - ref||_2 <= bound * ||ref||_2 (a handful of sign-flipped lr-sized steps are invisible in it,
    a wrong update rule or a missed row is not).  The element-wise statement is the closed loop."""
    is_bias = np.ndim(ref) < 2 or np.shape(ref)[-1] == 1
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    if os.environ.get('SLK_PRINT_DRIFT'):
        print('DRIFT', what, rel)
    if bound is None:
        bound = OPEN_LOOP_DRIFT_BIAS if is_bias else OPEN_LOOP_DRIFT_ROWS
    assert rel <= bound, ('open-loop drift', what, rel, bound)


def assert_close_table(got, want, tol, what, cond=None, loose=None):
    """Multi-step OPEN-LOOP comparison of a table against the oracle's, without an outlier quota:
      * tables of up to 10 000 elements: ||got - want||inf <= tol * ||want||inf, every element;
      * larger tables: ||got - want||_2 <= tol * ||want||_2 AND every element within 20 * tol * ||want||inf.  Several
        optimizer steps from zero accumulators amplify 1-ulp differences (a different expf, a different summation
        association) chaotically in a handful of elements -- torch's own dense and sparse paths end 6e-4 apart on one of
        the recordings -- so the element-wise statement at `tol` is the CLOSED-loop one (check_train_closed_loop,
        check_replays_reference_fixture); here no element may be arbitrarily wrong (the 20x cap) and the table as a whole
        must be within `tol` (the norm).
    Adagrad callers whose runs start from zero accumulators pass `cond` (adagrad_well_conditioned): elements whose
    accumulated gradient is a residual of cancelling terms are bounded by `loose` (identified by their gradient magnitude)."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    d = np.abs(got - want)
    scale = max(np.abs(want).max(), 1e-30)
    if cond is not None:  # ill-conditioned elements: within `loose` absolute, not compared
        assert (d[~cond] <= loose).all(), (what, 'ill-conditioned element moved by more than lr * steps')
        d = np.where(cond, d, 0.0)
    if want.size <= 10000:
        bad = d > tol * scale
        assert not bad.any(), (what, int(bad.sum()), float(d.max()))
        return
    assert d.max() <= 20.0 * tol * scale, (what, 'an element beyond 20 x tol', float(d.max() / scale))
    rel2 = np.linalg.norm(d) / max(np.linalg.norm(want), 1e-30)
    assert rel2 <= tol, (what, 'relative 2-norm', float(rel2))


def check_sampler_bit_exact(be, num_items, counts=(1, 5, 700, 3000)):
    eng = be.engine
    rs = np.random.RandomState(1234)
    rs.randint(0, 10, 77)  # start mid-block
    eng.rng_set_state(rs.get_state())
    for count in counts:
        out = be.alloc(np.full(count, -1, dtype=np.int64))
        eng.sample_items(num_items, count, be.ptr(out), be.stream)
        want = rs.randint(0, num_items, count, dtype=np.int64)
        assert (be.get(out) == want).all()
        got, ref = eng.rng_get_state(), rs.get_state()
        assert (got[1] == ref[1]).all() and got[2] == ref[2]


def check_sampler_block_boundaries(be):
    eng = be.engine
    rs = np.random.RandomState(42)  # pos == 624: regenerate-on-first-draw
    eng.rng_set_state(rs.get_state())
    for count in (624, 1, 623, 1248):
        out = be.alloc(np.empty(count, dtype=np.int64))
        eng.sample_items(2 ** 32, count, be.ptr(out), be.stream)  # every word accepted
        assert (be.get(out) == rs.randint(0, 2 ** 32, count, dtype=np.int64)).all()
        got, ref = eng.rng_get_state(), rs.get_state()
        assert (got[1] == ref[1]).all() and got[2] == ref[2]


def check_train_matches_oracle(be, loss, opt, D, U=37, I=29, N=150, B=64, nn=3, epochs=2, tol=2e-5,
                               seed=5, degenerate=False):
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    # keep scores O(1): a saturated fp32 sigmoid (|x| > 16.6) makes s*(1-s) flip between 0 and
    # 6e-8 on a 1-ulp difference of expf, which Adagrad then amplifies to lr
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    ora = BilinearOracle(*params, opt=opt, sparse_grads=True, **hp)
    dev = be.model(params, opt=opt, **hp)
    state = np.random.RandomState(9).get_state()
    orng = Rng(state=state)
    eng.rng_set_state(state)
    n_mb = (N + B - 1) // B
    d_users, d_items = be.alloc(users), be.alloc(items)
    for epoch in range(epochs):
        want_loss, want_neg = ora.train(orng, users, items, B, loss=loss, n_neg=nn, want_negs=True)
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.full(want_neg.size, -1, dtype=np.int64))
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn,
                           be.ptr(mb_loss), d_neg_out=be.ptr(neg_out), stream=be.stream)
        assert (be.get(neg_out) == want_neg).all()
        got_loss = be.get(mb_loss)
        if degenerate:
            # rows hit ~64x by cancelling +g/-g terms: what is left is summation-order noise
            # that Adagrad/Adam normalise to O(lr); only the first minibatch is well-posed
            if epoch == 0:
                assert abs(got_loss[0] - want_loss[0]) / abs(want_loss[0]) < 1e-5
            assert np.abs(got_loss - want_loss).max() / np.abs(want_loss).max() < 5e-2
        else:
            assert np.abs(got_loss - want_loss).max() / np.abs(want_loss).max() < 1e-5
    assert dev.optim.step == ora.step_count == epochs * n_mb
    if degenerate:
        #  the open-loop tables of such a run are noise-dominated and are not compared; the UPDATE is pinned
        # the closed-loop way instead: the same run one minibatch per call, before every minibatch the engine's tables go to the
        # oracle, which takes that one step -- loss within 1e-5, every element of every table and state tensor within
        # step_update_bounds, and the one-call run above must equal the per-minibatch run bit for bit
        # (a row's gradient here is a sum of hundreds of cancelling +g / -g terms: the fp32 summation order alone moves it by
        # percents of its own size, so the gradient allowance carried through the update formulas is the 5e-2 of the loss
        # statement above, not 1e-5 -- still a per-element statement on every table and state tensor: a missed row, a wrong
        # update rule or a double-applied gradient is far outside it.  The exact (float64) gradients of such rows are pinned by
        # check_long_run_gradients_against_exact.)
        check_train_closed_loop(be, loss, opt, D, U, I, N, B, nn=nn, epochs=epochs, seed=seed, open_loss_tol=5e-2, open_drift_bound=None,
                                grad_rel_delta=5e-2, grad_abs_delta=2.0 ** -22)  # (+ 2 ulp of a sum whose terms add up to <= 1 in magnitude)
    for t in range(0 if degenerate else 4):
        assert_close_table(be.get(dev.p[t]), ora.p[t], tol, ('param', t))
        assert_close_table(be.get(dev.s1[t]), ora.s1[t], tol, ('state1', t))
        if opt in ('sparse_adam', 'adam_dense'):
            assert_close_table(be.get(dev.s2[t]), ora.s2[t], tol, ('state2', t))
    got, ref = eng.rng_get_state(), orng.get_state()
    assert (got[1] == ref[1]).all() and got[2] == ref[2]
    # predict on the engine's own tables: scalar user vs all items, and explicit pairs
    # (factorization/implicit.py:277-311)
    P = [be.get(x).astype(np.float64) for x in dev.p]
    score = lambda u, i: (P[0][u] * P[1][i]).sum(-1) + P[2][u] + P[3][i]
    uq = min(3, U - 1)
    out = be.alloc(np.empty(I, dtype=np.float32))
    d_u = be.alloc(np.array([uq], dtype=np.int64))
    eng.bilinear_predict(dev.tables, be.ptr(d_u), 1, None, I, be.ptr(out), be.stream)
    assert rel_inf(be.get(out), score(np.full(I, uq), np.arange(I))) < 1e-5
    m = min(50, N)
    pu, pi = users[:m].copy(), items[:m].copy()
    out = be.alloc(np.empty(m, dtype=np.float32))
    d_pu, d_pi = be.alloc(pu), be.alloc(pi)
    eng.bilinear_predict(dev.tables, be.ptr(d_pu), m, be.ptr(d_pi), m, be.ptr(out), be.stream)
    assert rel_inf(be.get(out), score(pu, pi)) < 1e-5


def check_single_step_gradients(be, loss, D, U=50, I=40, B=128, nn=3, seed=11, bias_tol=1e-5, emb_tol=1e-5):
    """Identical minibatch, identical parameters: loss within 1e-5 rel, summed gradients
    within 1e-5 of each table's inf-norm (bias tables: of their joint norm, the user-bias
    gradient being a sum of cancelling +g/-g terms).  The engine's gradient is read back
    through the ADAM_DENSE accumulate-only mode with lr = 0 (parameters stay put).
    bias_tol / emb_tol: for tables of a handful of rows, where a bias gradient is a sum of thousands of cancelling +g/-g terms and the
    oracle's own sequential fp32 sum is that far from the exact one."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, B).astype(np.int64)
    items = rs.randint(0, I, B).astype(np.int64)
    n_draw = B * (nn if loss == 'adaptive_hinge' else 1)
    negs = rs.randint(0, I, n_draw).astype(np.int64)
    params = [rs.normal(0, 0.5, (U, D)), rs.normal(0, 0.5, (I, D)), rs.normal(0, 0.2, U), rs.normal(0, 0.2, I)]
    ora = BilinearOracle(*params, opt='adagrad', sparse_grads=True)
    want_loss, want_g = ora.step(users, items, negs, loss=loss, n_neg=nn, want_grads=True)
    # beta1 = 0 => exp_avg after one step == the gradient itself
    dev = be.model(params, opt='adam_dense', lr=0.0, betas=(0.0, 0.999))
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_users, d_items, d_negs = be.alloc(users), be.alloc(items), be.alloc(negs)
    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), B, B, loss, nn,
                       be.ptr(mb_loss), d_neg_in=be.ptr(d_negs), stream=be.stream)
    assert abs(float(be.get(mb_loss)[0]) - want_loss) / abs(want_loss) < 1e-5
    got = [be.get(dev.s1[t]) for t in range(4)]
    bscale = max(np.abs(want_g[2]).max(), np.abs(want_g[3]).max())
    for t in range(4):
        scale = np.abs(want_g[t]).max() if t < 2 else bscale
        assert np.abs(got[t].ravel() - want_g[t].ravel()).max() <= (emb_tol if t < 2 else bias_tol) * scale, t
    for t in range(4):  # lr = 0: parameters untouched
        assert np.array_equal(be.get(dev.p[t]).ravel(), np.asarray(params[t], np.float32).ravel())


def check_long_run_gradients_against_exact(be, loss, D, U, I, B, seed=11, tol=2e-6):
    """Item rows that collect thousands of occurrences in one minibatch (k_item_pass partials + k_item_stitch): the engine's
    summed item gradients against the EXACT ones (the pair losses' closed-form backward in float64, numpy), to 2e-6 of the
    table's norm -- an order of magnitude inside the 1e-5 bar.  The oracle restates the reference's SEQUENTIAL fp32 sums
    (index_add / coalesce on the CPU), which at thousands of cancelling terms per row are themselves 1e-5..1e-4 from exact: it
    is held to 1e-3 here only as a sanity check of the comparison itself."""
    assert loss in ('bpr', 'pointwise')
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, B).astype(np.int64)
    items = rs.randint(0, I, B).astype(np.int64)
    negs = rs.randint(0, I, B).astype(np.int64)
    params = [rs.normal(0, 0.5, (U, D)), rs.normal(0, 0.5, (I, D)), rs.normal(0, 0.2, U), rs.normal(0, 0.2, I)]
    P, Q, bu, bi = [np.asarray(p, np.float32).astype(np.float64) for p in params]
    sp = (P[users] * Q[items]).sum(1) + bu[users] + bi[items]
    sn = (P[users] * Q[negs]).sum(1) + bu[users] + bi[negs]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    if loss == 'bpr':  # losses.py:53-90: mean(1 - sigmoid(pos - neg))
        s = sig(sp - sn)
        gp = -(s * (1.0 - s)) / B
        gn = -gp
        want_loss = float((1.0 - s).mean())
    else:              # losses.py:18-50: mean((1 - sigmoid(pos)) + sigmoid(neg))
        a, b = sig(sp), sig(sn)
        gp, gn = -(a * (1.0 - a)) / B, (b * (1.0 - b)) / B
        want_loss = float(((1.0 - a) + b).mean())
    exact = np.zeros_like(Q)
    np.add.at(exact, items, gp[:, None] * P[users])
    np.add.at(exact, negs, gn[:, None] * P[users])
    _, ora_g = BilinearOracle(*params, opt='adagrad', sparse_grads=True).step(users, items, negs, loss=loss, n_neg=1,
                                                                             want_grads=True)
    dev = be.model(params, opt='adam_dense', lr=0.0, betas=(0.0, 0.999))  # exp_avg after one step == the gradient
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_users, d_items, d_negs = be.alloc(users), be.alloc(items), be.alloc(negs)
    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), B, B, loss, 1, be.ptr(mb_loss),
                       d_neg_in=be.ptr(d_negs), stream=be.stream)
    assert abs(float(be.get(mb_loss)[0]) - want_loss) / abs(want_loss) < 1e-5
    got = be.get(dev.s1[1]).astype(np.float64).reshape(exact.shape)
    scale = np.abs(exact).max()
    ours, theirs = np.abs(got - exact).max() / scale, np.abs(np.asarray(ora_g[1], np.float64).reshape(exact.shape) - exact).max() / scale
    assert ours <= tol, (ours, theirs)
    assert theirs <= 1e-3, (ours, theirs)
    return ours, theirs


def check_long_user_run_gradients_against_exact(be, loss, D, U, I, B, seed=12, tol=2e-6):
    """USER rows that collect hundreds or thousands of occurrences in one minibatch (k_user_pass<ULONG> partials +
    k_user_stitch): the engine's summed user-embedding and user-bias gradients against the EXACT ones (closed-form backward
    in float64), to 2e-6 of the table's norm; the oracle's sequential fp32 sums are held to 1e-3 as a sanity check only."""
    assert loss in ('bpr', 'pointwise')
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, B).astype(np.int64)
    items = rs.randint(0, I, B).astype(np.int64)
    negs = rs.randint(0, I, B).astype(np.int64)
    params = [rs.normal(0, 0.5, (U, D)), rs.normal(0, 0.5, (I, D)), rs.normal(0, 0.2, U), rs.normal(0, 0.2, I)]
    P, Q, bu, bi = [np.asarray(p, np.float32).astype(np.float64) for p in params]
    sp = (P[users] * Q[items]).sum(1) + bu[users] + bi[items]
    sn = (P[users] * Q[negs]).sum(1) + bu[users] + bi[negs]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    if loss == 'bpr':
        s = sig(sp - sn)
        gp = -(s * (1.0 - s)) / B
        gn = -gp
        want_loss = float((1.0 - s).mean())
    else:
        a, b = sig(sp), sig(sn)
        gp, gn = -(a * (1.0 - a)) / B, (b * (1.0 - b)) / B
        want_loss = float(((1.0 - a) + b).mean())
    exact = np.zeros_like(P)
    np.add.at(exact, users, gp[:, None] * Q[items] + gn[:, None] * Q[negs])
    exact_b = np.zeros_like(bu)
    np.add.at(exact_b, users, gp + gn)
    _, ora_g = BilinearOracle(*params, opt='adagrad', sparse_grads=True).step(users, items, negs, loss=loss, n_neg=1,
                                                                             want_grads=True)
    dev = be.model(params, opt='adam_dense', lr=0.0, betas=(0.0, 0.999))  # exp_avg after one step == the gradient
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_users, d_items, d_negs = be.alloc(users), be.alloc(items), be.alloc(negs)
    long_before = eng.get_stat('user_long_launches')
    eng.set_option('epoch_kernel', 0)  # the launch path's hot-user form is what is under test
    try:
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), B, B, loss, 1, be.ptr(mb_loss),
                           d_neg_in=be.ptr(d_negs), stream=be.stream)
    finally:
        eng.set_option('epoch_kernel', 1)
    if B // U >= 96:  # every run then covers a tile of 32 positions
        assert eng.get_stat('user_long_launches') == long_before + 1, 'the long-run form of the user pass was not taken'
    assert abs(float(be.get(mb_loss)[0]) - want_loss) / abs(want_loss) < 1e-5
    got = be.get(dev.s1[0]).astype(np.float64).reshape(exact.shape)
    scale = np.abs(exact).max()
    ours = np.abs(got - exact).max() / scale
    theirs = np.abs(np.asarray(ora_g[0], np.float64).reshape(exact.shape) - exact).max() / scale
    assert ours <= tol, (ours, theirs)
    assert theirs <= 1e-3, (ours, theirs)
    if loss == 'pointwise':  # (bpr: the user-bias gradient is a sum of exactly cancelling +g / -g pairs)
        got_b = be.get(dev.s1[2]).astype(np.float64).ravel()
        assert np.abs(got_b - exact_b).max() <= tol * np.abs(exact_b).max(), (np.abs(got_b - exact_b).max(), np.abs(exact_b).max())
    else:
        assert (be.get(dev.s1[2]) == 0).all()
    return ours, theirs


def step_update_bounds(opt, hp, pre_p, pre_s1, pre_s2, g, step, rel_delta=1e-5, bias_tables=(2, 3), abs_delta=0.0):
    """Per element: how far ONE optimizer step may move a parameter / its state when the summed gradient is perturbed by
    delta = rel_delta * ||g||inf (per embedding table, the bias tables against their joint norm; touched rows only) --
    the north star's gradient tolerance carried through the update formulas:
        Adagrad (+wd)      dp <= lr * delta / (sqrt(sum_pre + g^2) + eps)          dsum <= 2 |g| delta
        Adam / SparseAdam  dp <= (lr / bc1) * delta / (sqrt(v_new / bc2) + eps)    dm <= (1-b1) delta, dv <= 2 (1-b2) |g| delta
    The parameter bound is only large where the accumulator is ~0 and the gradient itself is ~0 (the update is then
    lr * sign(g)): the ill-conditioned elements are identified by their gradient magnitude, not by a quota."""
    lr, wd = float(hp.get('lr', 1e-2)), float(hp.get('weight_decay', 0.0))
    b1, b2 = hp.get('betas', (0.9, 0.999))
    eps = hp.get('eps') or (1e-10 if opt.startswith('adagrad') else 1e-8)
    bscale = max(np.abs(g[t]).max() for t in bias_tables)
    out = []
    for t in range(len(g)):
        gt = np.asarray(g[t], np.float64)
        scale = bscale if t in bias_tables else np.abs(gt).max()
        touched = (gt != 0).any(axis=1, keepdims=True) if gt.ndim == 2 else (gt != 0)
        # abs_delta (degenerate runs only): an absolute floor of the gradient perturbation -- the fp32 rounding of a sum of
        # hundreds of cancelling terms does not scale with the (arbitrarily small) sum
        # (the floor also covers rows whose oracle gradient is EXACTLY zero -- a user whose occurrences cancel term by term in
        # the oracle's summation order and leave a 1e-11 residue in another: Adagrad from a zero accumulator moves such an
        # element by lr * g / (|g| + eps) whatever |g| is)
        delta = np.broadcast_to(rel_delta * scale * touched + abs_delta, gt.shape)
        geff = gt + wd * np.asarray(pre_p[t], np.float64).reshape(gt.shape) if opt.endswith('dense') else gt
        if opt == 'sgd':  # p -= lr * g: a gradient perturbation moves the parameter by lr * delta, there is no state
            dp, ds1, ds2 = lr * delta, np.zeros_like(gt), np.zeros_like(gt)
        elif opt.startswith('adagrad'):
            dp = lr * delta / (np.sqrt(np.asarray(pre_s1[t], np.float64).reshape(gt.shape) + geff * geff) + eps)
            ds1, ds2 = 2.0 * np.abs(geff) * delta, np.zeros_like(gt)
        else:
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            v_new = b2 * np.asarray(pre_s2[t], np.float64).reshape(gt.shape) + (1.0 - b2) * geff * geff
            dp = (lr / bc1) * delta / (np.sqrt(v_new / bc2) + eps)
            ds1, ds2 = (1.0 - b1) * delta, 2.0 * (1.0 - b2) * np.abs(geff) * delta
        out.append((dp, ds1, ds2))
    return out


def assert_step_within_bounds(be, dev, ora, pre_p, pre_s1, pre_s2, g, step, opt, hp, bias_tables=(2, 3), what='', rel_delta=1e-5, abs_delta=0.0):
    """After ONE engine step and ONE oracle step from the same tables / state: every element of every parameter and
    optimizer-state tensor within 1e-5 * ||.||inf + step_update_bounds (no quota)."""
    bounds = step_update_bounds(opt, hp, pre_p, pre_s1, pre_s2, g, step, rel_delta=rel_delta, bias_tables=bias_tables, abs_delta=abs_delta)
    adam = opt in ('sparse_adam', 'adam_dense')
    for t in range(len(g)):
        dp, ds1, ds2 = bounds[t]
        for got, want, bound, nm in ((dev.p[t], ora.p[t], dp, 'param'), (dev.s1[t], ora.s1[t], ds1, 'state1'),
                                     (dev.s2[t], ora.s2[t], ds2, 'state2')):
            if nm == 'state2' and not adam:
                continue
            w64 = np.asarray(want, np.float64)
            d = np.abs(be.get(got).astype(np.float64).reshape(w64.shape) - w64)
            tol = 1e-5 * max(np.abs(w64).max(), 1e-30) + bound.reshape(w64.shape)
            assert not (d > tol).any(), ('%s step %d table %d %s: %d elements beyond the conditioned bound'
                                         % (what, step, t, nm, int((d > tol).sum())), float(d.max()))


def check_train_closed_loop(be, loss, opt, D, U, I, N, B, nn=3, epochs=1, seed=5, open_loss_tol=1e-3, open_drift_bound=0.25,
                            grad_rel_delta=1e-5, grad_abs_delta=0.0):
    """Multi-minibatch training against the oracle WITHOUT an outlier allowance: one engine call over the whole run (open
    loop: negatives and RNG state bit-exact against the host stream, the first minibatch's loss within 1e-5, later losses
    within 1e-3 -- from zero accumulators a trajectory is chaotic element by element, see check_replays_reference_fixture),
    then the same run one minibatch per call (closed loop): before every minibatch the engine's tables and state go to the
    oracle, which takes that one step with the same negatives; loss within 1e-5, every element of every table / state
    tensor within the bound a 1e-5-relative gradient perturbation implies for that step (step_update_bounds).  The two
    runs must end bit-identical (chunking is value-neutral), so the per-step statement covers the one-call tables."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    state = np.random.RandomState(9).get_state()
    n_mb = (N + B - 1) // B
    NN = nn if loss == 'adaptive_hinge' else 1
    # ---- open loop
    ora = BilinearOracle(*params, opt=opt, sparse_grads=True, **hp)
    dev = be.model(params, opt=opt, **hp)
    orng = Rng(state=state)
    eng.rng_set_state(state)
    d_users, d_items = be.alloc(users), be.alloc(items)
    all_negs = []
    for epoch in range(epochs):
        want_loss, want_neg = ora.train(orng, users, items, B, loss=loss, n_neg=nn, want_negs=True)
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.full(want_neg.size, -1, dtype=np.int64))
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn, be.ptr(mb_loss),
                           d_neg_out=be.ptr(neg_out), stream=be.stream)
        assert (be.get(neg_out) == want_neg).all()
        all_negs.append(want_neg)
        got_loss = be.get(mb_loss)
        if epoch == 0:
            assert abs(got_loss[0] - want_loss[0]) <= 1e-5 * abs(want_loss[0])
        assert np.abs(got_loss - want_loss).max() / np.abs(want_loss).max() < open_loss_tol
    got, ref = eng.rng_get_state(), orng.get_state()
    assert (got[1] == ref[1]).all() and got[2] == ref[2]
    open_tables = [be.get(x).copy() for x in dev.p + dev.s1 + dev.s2]
    for t in range(4 if open_drift_bound is not None else 0):
        # coarse sanity only (a wrong update rule or a missed row shows; the element-wise statement is the closed loop below):
        # random data from zero accumulators at lr 0.05 drifts further than the recordings the default bounds were measured on --
        # adaptive hinge's arg-max flips on 1-ulp score differences, a handful of users collect every gradient
        assert_open_loop_drift(open_tables[t], ora.p[t], ('closed-loop check, open-loop run', t), bound=open_drift_bound)
    # ---- closed loop
    dev2 = be.model(params, opt=opt, **hp)
    step = 0
    for epoch in range(epochs):
        for off in range(0, N, B):
            hi = min(off + B, N)
            neg = all_negs[epoch][off * NN:hi * NN]
            pre_p = [be.get(x).copy() for x in dev2.p]
            pre_s1 = [be.get(x).copy() for x in dev2.s1]
            pre_s2 = [be.get(x).copy() for x in dev2.s2]
            o1 = BilinearOracle(*pre_p, opt=opt, sparse_grads=True, state1=pre_s1, state2=pre_s2, step=step, **hp)
            want_loss, g = o1.step(users[off:hi], items[off:hi], neg, loss=loss, n_neg=nn, want_grads=True)
            step += 1
            d_su, d_si, d_neg = be.alloc(users[off:hi]), be.alloc(items[off:hi]), be.alloc(neg)
            mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
            eng.bilinear_train(dev2.tables, dev2.optim, be.ptr(d_su), be.ptr(d_si), hi - off, B, loss, nn, be.ptr(mb_loss),
                               d_neg_in=be.ptr(d_neg), stream=be.stream)
            assert dev2.optim.step == step
            assert abs(float(be.get(mb_loss)[0]) - want_loss) <= 1e-5 * abs(want_loss), (epoch, off)
            assert_step_within_bounds(be, dev2, o1, pre_p, pre_s1, pre_s2, g, step, opt, hp, what='%s/%s' % (loss, opt), rel_delta=grad_rel_delta,
                                      abs_delta=grad_abs_delta)
    for k, x in enumerate(dev2.p + dev2.s1 + dev2.s2):
        assert np.array_equal(be.get(x), open_tables[k]), ('closed-loop run differs from the open-loop one', k)


def check_replays_reference_fixture(be, golden_dir, name):
    """A run recorded from the live reference (same init tables, same shuffled ids, same RandomState), replayed twice:

    OPEN LOOP (one engine call per epoch, as fit() makes them): negatives and the RandomState afterwards bit-exact, the first
    minibatch's loss within 1e-5, its summed gradients within 1e-5 of the reference's recorded p.grad, every later loss within
    1e-3.  Final tables: a bounded deviation only -- from zero accumulators the trajectory is chaotic at the 1e-3 level (an
    element whose first gradient is ~1e-10 moves by lr * sign(g); the moved parameter perturbs every later gradient; torch's
    own dense and sparse paths, which differ in summation association only, end 6e-4 apart on `d64_bpr_adagrad`), so an
    element-wise open-loop comparison pins nothing.

    CLOSED LOOP (one engine call per minibatch): before EVERY minibatch the engine's tables and optimizer state are handed
    to the oracle, which takes that one step with the recorded negatives; the engine's loss must agree within 1e-5 and every
    element of every table / state tensor within the bound the north star's gradient tolerance (1e-5 relative) implies for
    that step's update (step_update_bounds) -- no quota of outliers.  The closed-loop run must end bit-identical to the
    open-loop one (chunking is value-neutral), so the per-step statement covers the tables fit() produces.
    Returns the final tables."""
    from oracle.replay import case_from_rec
    eng = be.engine
    rec = np.load(os.path.join(golden_dir, name + '.npz'))
    case = case_from_rec(rec)
    hp = oracle_hparams(case)
    hp.pop('sparse_grads')
    opt = ORACLE_OPT[case['opt']]
    nn = int(case.get('n_neg', 5)) if case['loss'] == 'adaptive_hinge' else 1
    N, B = int(case['N']), int(case['B'])
    n_mb = (N + B - 1) // B
    loss_kind = str(case['loss'])
    rng0 = ('MT19937', rec['rng_key_before_fit'], int(rec['rng_pos_before_fit']))

    # ---- open loop
    dev = be.model([rec['init_%d' % t] for t in range(4)], opt=opt, **hp)
    eng.rng_set_state(rng0)
    host = Rng(state=rng0)
    losses, negs = [], []
    for e in range(int(case['n_iter'])):
        # the shuffle stays on the host (torch_utils.py:35-52) and shares the stream
        host.set_state(eng.rng_get_state())
        perm = host.shuffle_perm(N)
        eng.rng_set_state(host.get_state())
        su = rec['users'].astype(np.int64)[perm]
        si = rec['items'].astype(np.int64)[perm]
        assert (su == rec['shuffled_users'][e]).all()
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.empty(N * nn, dtype=np.int64))
        d_su, d_si = be.alloc(su), be.alloc(si)
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_su), be.ptr(d_si), N, B, loss_kind, nn, be.ptr(mb_loss),
                           d_neg_out=be.ptr(neg_out), stream=be.stream)
        losses.append(be.get(mb_loss))
        negs.append(be.get(neg_out))
    assert (np.concatenate(negs) == rec['negatives']).all()
    losses = np.concatenate(losses)
    assert abs(losses[0] - rec['losses'][0]) / abs(rec['losses'][0]) < 1e-5
    assert np.max(np.abs(losses - rec['losses']) / np.abs(rec['losses'])) < 1e-3
    st = eng.rng_get_state()
    assert (st[1] == rec['rng_key_after_fit']).all() and st[2] == int(rec['rng_pos_after_fit'])
    open_tables = [be.get(dev.p[t]).copy() for t in range(4)]
    for t in range(4):  # coarse drift sanity only (see the docstring): the element-wise statement is the closed loop below
        ref = rec['final_%d' % t]
        assert_open_loop_drift(open_tables[t], ref, (name, t))

    # ---- the first minibatch's summed gradients against the reference's recorded p.grad: ADAM_DENSE accumulate-only mode
    # (lr = 0, beta1 = 0 => exp_avg == the gradient), the recorded negatives
    B0 = min(B, N)
    gdev = be.model([rec['init_%d' % t] for t in range(4)], opt='adam_dense', lr=0.0, betas=(0.0, 0.999))
    su0 = rec['shuffled_users'][0].astype(np.int64)[:B0]
    si0 = rec['shuffled_items'][0].astype(np.int64)[:B0]
    d_su, d_si, d_neg = be.alloc(su0), be.alloc(si0), be.alloc(rec['negatives'][:B0 * nn].astype(np.int64))
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    eng.bilinear_train(gdev.tables, gdev.optim, be.ptr(d_su), be.ptr(d_si), B0, B0, loss_kind, nn, be.ptr(mb_loss),
                       d_neg_in=be.ptr(d_neg), stream=be.stream)
    assert abs(float(be.get(mb_loss)[0]) - rec['losses'][0]) <= 1e-5 * abs(rec['losses'][0])
    bscale = max(np.abs(rec['grad0_2']).max(), np.abs(rec['grad0_3']).max())
    for t in range(4):
        ref = rec['grad0_%d' % t]
        scale = np.abs(ref).max() if t < 2 else bscale
        err = np.abs(be.get(gdev.s1[t]).reshape(ref.shape) - ref).max()
        assert err <= 1e-5 * scale, ('first-step gradient vs the reference', t, float(err), float(scale))

    # ---- closed loop
    dev2 = be.model([rec['init_%d' % t] for t in range(4)], opt=opt, **hp)
    step = 0
    for e in range(int(case['n_iter'])):
        su = rec['shuffled_users'][e].astype(np.int64)
        si = rec['shuffled_items'][e].astype(np.int64)
        for off in range(0, N, B):
            hi = min(off + B, N)
            neg = rec['negatives'][(e * N + off) * nn:(e * N + hi) * nn].astype(np.int64)
            pre_p = [be.get(x).copy() for x in dev2.p]
            pre_s1 = [be.get(x).copy() for x in dev2.s1]
            pre_s2 = [be.get(x).copy() for x in dev2.s2]
            ora = BilinearOracle(*pre_p, opt=opt, sparse_grads=True, state1=pre_s1, state2=pre_s2, step=step, **hp)
            want_loss, g = ora.step(su[off:hi], si[off:hi], neg, loss=loss_kind, n_neg=nn, want_grads=True)
            step += 1
            d_su, d_si, d_neg = be.alloc(su[off:hi]), be.alloc(si[off:hi]), be.alloc(neg)
            mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
            eng.bilinear_train(dev2.tables, dev2.optim, be.ptr(d_su), be.ptr(d_si), hi - off, B, loss_kind, nn,
                               be.ptr(mb_loss), d_neg_in=be.ptr(d_neg), stream=be.stream)
            assert dev2.optim.step == step
            assert abs(float(be.get(mb_loss)[0]) - want_loss) <= 1e-5 * abs(want_loss), (e, off)
            assert_step_within_bounds(be, dev2, ora, pre_p, pre_s1, pre_s2, g, step, opt, hp)
    # chunking is value-neutral: the per-minibatch calls end where the per-epoch calls did, bit for bit
    for t in range(4):
        assert np.array_equal(be.get(dev2.p[t]), open_tables[t]), ('closed-loop run differs from the open-loop one', t)
    return open_tables


ALL_LOSSES = ('pointwise', 'bpr', 'hinge', 'adaptive_hinge')
ALL_OPTS = ('adagrad', 'sparse_adam', 'adam_dense', 'adagrad_dense', 'sgd')
FIXTURES = ['adaptive_hinge_adagrad', 'adaptive_hinge_adagrad_sparse', 'adaptive_hinge_adam_default', 'adaptive_hinge_sparse_adam',
            'bpr_adagrad', 'bpr_adagrad_sparse', 'bpr_adam_default', 'bpr_sparse_adam', 'c1_bpr_adagrad', 'c1_bpr_adam',
            'd12_pointwise_adagrad_wd', 'd64_adaptive_sparse_adam', 'd64_bpr_adagrad', 'hinge_adagrad', 'hinge_adagrad_sparse',
            'hinge_adam_default', 'hinge_sparse_adam', 'pointwise_adagrad', 'pointwise_adagrad_sparse', 'pointwise_adam_default',
            'pointwise_sparse_adam', 'bpr_sgd', 'adaptive_hinge_sgd_sparse', 'd64_pointwise_sgd']  # every BilinearNet run recorded from the live reference (oracle/make_golden.py)


# ---------------------------------------------------------------------------------------
# PoolNet / ImplicitSequenceModel (slk_poolnet_*)
# ---------------------------------------------------------------------------------------
def make_sequences(rs, n_seq, L, num_items, pad_frac=0.5):
    seqs = rs.randint(1, num_items, (n_seq, L)).astype(np.int64)
    for b in range(n_seq):
        if L > 1 and rs.rand() < pad_frac:
            seqs[b, :rs.randint(1, L)] = 0  # left padding, at least one real item
    return seqs


def _seq_params(rs, I, D, rows=None):
    """`rows`: compressed rows when the item embedding layer is a BloomEmbedding."""
    sc = min(0.3, 1.0 / np.sqrt(D))
    E = rs.normal(0, sc, (rows or I, D)).astype(np.float32)
    bias = rs.normal(0, 0.1, I).astype(np.float32)
    E[0] = 0.0   # padding row (ScaledEmbedding/ZeroEmbedding with padding_idx=0, layers.py:35-37,54-56)
    bias[0] = 0.0
    return [E, bias]


def check_seq_train_matches_oracle(be, loss, opt, D, I=31, N=40, L=9, B=16, nn=3, epochs=2, tol=2e-5, seed=5,
                                   pad_frac=0.5, bloom=0, ratio=0.4):
    """`bloom` > 0: PoolNet over a BloomEmbedding item layer with that many hash functions."""
    from oracle.oracle import PoolNetOracle, bloom_desc
    eng = be.engine
    rs = np.random.RandomState(seed)
    seqs = make_sequences(rs, N, L, I, pad_frac)
    desc = bloom_desc(n_hash=bloom) if bloom else None
    params = _seq_params(rs, I, D, rows=int(ratio * I) if bloom else None)
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    ora = PoolNetOracle(*params, opt=opt, item_bloom=desc, **hp)
    dev = be.seq_model(params, opt=opt, item_bloom=desc, **hp)
    state = np.random.RandomState(9).get_state()
    orng = Rng(state=state)
    eng.rng_set_state(state)
    n_mb = (N + B - 1) // B
    d_seqs = be.alloc(seqs)
    for epoch in range(epochs):
        want_loss, want_neg = ora.train(orng, seqs, B, loss=loss, n_neg=nn, want_negs=True)
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.full(want_neg.size, -1, dtype=np.int64))
        eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), N, L, B, loss, nn, be.ptr(mb_loss),
                          d_neg_out=be.ptr(neg_out), stream=be.stream)
        assert (be.get(neg_out) == want_neg).all()
        got_loss = be.get(mb_loss)
        # the first minibatch is a pure forward on identical parameters; later ones also see the (Adagrad: up to lr-sized)
        # moves of ill-conditioned elements, see below
        if epoch == 0:
            assert abs(got_loss[0] - want_loss[0]) / abs(want_loss[0]) < 1e-5, (got_loss, want_loss)
        assert np.abs(got_loss - want_loss).max() / np.abs(want_loss).max() < (2e-4 if opt == 'adagrad' else 1e-5), (got_loss, want_loss)
    assert dev.optim.step == ora.step_count == epochs * n_mb
    for t in range(2):
        # Adagrad: an element whose accumulated g^2 is ~0 (a residual of cancelling terms) moves by up to lr per step whatever
        # the summation order; it is bounded, the others are compared
        cond = adagrad_well_conditioned(ora.s1[t]) if opt == 'adagrad' else None
        assert_close_table(be.get(dev.p[t]), ora.p[t], tol, ('param', t), cond=cond, loose=hp['lr'] * epochs * n_mb * 1.01)
        assert_close_table(be.get(dev.s1[t]), ora.s1[t], tol, ('state1', t))
        if opt in ('sparse_adam', 'adam_dense'):
            assert_close_table(be.get(dev.s2[t]), ora.s2[t], tol, ('state2', t))
    assert (be.get(dev.p[0])[0] == 0).all() and be.get(dev.p[1])[0] == 0  # padding row untouched
    got, ref = eng.rng_get_state(), orng.get_state()
    assert (got[1] == ref[1]).all() and got[2] == ref[2]
    # predict on the engine's own tables (sequence/implicit.py:288-340)
    po = PoolNetOracle(be.get(dev.p[0]), be.get(dev.p[1]), item_bloom=desc)
    out = be.alloc(np.empty(I, dtype=np.float32))
    d_seq = be.alloc(seqs[1])
    eng.poolnet_predict(dev.tables, be.ptr(d_seq), L, None, I, be.ptr(out), be.stream)
    assert rel_inf(be.get(out), po.predict(seqs[1])) < 1e-5
    some = np.arange(1, min(I, 12), dtype=np.int64)
    out = be.alloc(np.empty(some.size, dtype=np.float32))
    d_some = be.alloc(some)
    eng.poolnet_predict(dev.tables, be.ptr(d_seq), L, be.ptr(d_some), some.size, be.ptr(out), be.stream)
    assert rel_inf(be.get(out), po.predict(seqs[1], some)) < 1e-5


def check_seq_chunking_is_bit_neutral(be, loss, opt, D, I=2000, N=300, L=24, B=32, nn=3, chunk=2048, overlap=1, bloom=0, seed=17,
                                      option=None, negs_in=False):
    """PoolNet training in ONE prep chunk against the same call cut into several chunks of `chunk` timesteps with the prep of
    chunk c + 1 (negatives, occurrence sort, flags) on the second stream while chunk c trains (slk_seq.hip: the pipeline of
    slk_bilinear_train): losses, negatives, RNG state, tables and optimizer state bit for bit.
    `negs_in`: both runs are HANDED the same negatives (d_neg_in) instead of drawing them: every chunk reads its own window of
    them, d_neg_out echoes them and the RNG state stays where it was set."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    seqs = make_sequences(rs, N, L, I, 0.3)
    params = _seq_params(rs, I, D, rows=int(0.4 * I) if bloom else None)
    from oracle.oracle import bloom_desc
    desc = bloom_desc(n_hash=bloom) if bloom else None
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    n_draw = N * L * (nn if loss == 'adaptive_hinge' else 1)
    given = np.random.RandomState(seed).randint(0, I, n_draw).astype(np.int64) if negs_in else None
    results = []
    for run_i, (chunk_i, overlap_i) in enumerate(((1 << 23, 0), (chunk, overlap))):
        eng.set_option('chunk_interactions', chunk_i)
        eng.set_option('overlap_prep', overlap_i)
        eng.set_option('overlap_min_batch', 0)
        if option:  # (name, value of the first run, value of the second run, default): an option that must not change results
            eng.set_option(option[0], option[1 + run_i])
        try:
            dev = be.seq_model(params, opt=opt, item_bloom=desc, lr=0.05)
            eng.rng_set_state(state)
            d_seqs = be.alloc(seqs)
            mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
            neg_out = be.alloc(np.full(n_draw, -1, dtype=np.int64))
            d_neg_in = be.alloc(given) if negs_in else None
            for _ in range(2):
                eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), N, L, B, loss, nn, be.ptr(mb_loss),
                                  d_neg_in=be.ptr(d_neg_in), d_neg_out=be.ptr(neg_out), stream=be.stream)
            st = eng.rng_get_state()
            if negs_in:
                assert np.array_equal(be.get(neg_out), given), 'd_neg_out is not the negatives the call was handed'
                assert np.array_equal(st[1], state[1]) and st[2] == state[2], 'a call that was handed its negatives moved the RNG'
            results.append([be.get(mb_loss), be.get(neg_out), st[1], np.array(st[2])] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
        finally:
            eng.set_option('chunk_interactions', 1 << 23)
            eng.set_option('overlap_prep', 0)
            eng.set_option('overlap_min_batch', 1 << 16)
            if option:
                eng.set_option(option[0], option[3])
    for k, (a, b) in enumerate(zip(*results)):
        assert np.array_equal(a, b), ('tensor %d differs between one chunk and the pipelined chunks' % k)


def _seq_case(be, opt, D, I, N, L, bloom, seed):
    """sequences, a fresh model and the RNG state of check_seq_chunking_is_bit_neutral's case"""
    from oracle.oracle import bloom_desc
    rs = np.random.RandomState(seed)
    seqs = make_sequences(rs, N, L, I, 0.3)
    params = _seq_params(rs, I, D, rows=int(0.4 * I) if bloom else None)
    dev = be.seq_model(params, opt=opt, item_bloom=bloom_desc(n_hash=bloom) if bloom else None, lr=0.05)
    return seqs, dev, np.random.RandomState(seed + 1).get_state()


def _seq_train_twice(be, dev, seqs, B, loss, nn):
    """two training calls over `seqs`: [losses, negatives, RNG key, RNG position, tables, optimizer state]"""
    eng = be.engine
    N, L = seqs.shape
    d_seqs = be.alloc(seqs)
    mb_loss = be.alloc(np.zeros((N + B - 1) // B, dtype=np.float32))
    neg_out = be.alloc(np.full(N * L * (nn if loss == 'adaptive_hinge' else 1), -1, dtype=np.int64))
    for _ in range(2):
        eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), N, L, B, loss, nn, be.ptr(mb_loss), d_neg_out=be.ptr(neg_out),
                          stream=be.stream)
    st = eng.rng_get_state()
    return [be.get(mb_loss), be.get(neg_out), st[1], np.array(st[2])] + [be.get(x) for x in dev.p + dev.s1 + dev.s2]


def check_seq_reserve_is_neutral(be, loss, opt, D, I=2000, N=300, L=24, B=32, nn=3, chunk=2048, overlap=1, seed=17):
    """slk_poolnet_reserve only allocates: it leaves the RNG state, optim.step and the tables as they were, and the training calls
    behind it give what they give without it, bit for bit."""
    eng = be.engine
    results = []
    with eng.options(chunk_interactions=chunk, overlap_prep=overlap, overlap_min_batch=0):
        for reserve in (True, False):
            seqs, dev, state = _seq_case(be, opt, D, I, N, L, 0, seed)
            eng.rng_set_state(state)
            if reserve:
                before = [be.get(x).copy() for x in dev.p + dev.s1 + dev.s2]
                eng.poolnet_reserve(dev.tables, dev.optim, N, L, B, loss, nn, stream=be.stream)
                st = eng.rng_get_state()
                assert np.array_equal(st[1], state[1]) and st[2] == state[2], 'slk_poolnet_reserve moved the RNG'
                assert dev.optim.step == 0
                for k, (a, b) in enumerate(zip(before, [be.get(x) for x in dev.p + dev.s1 + dev.s2])):
                    assert np.array_equal(a, b), 'slk_poolnet_reserve changed tensor %d' % k
            results.append(_seq_train_twice(be, dev, seqs, B, loss, nn))
    for k, (a, b) in enumerate(zip(*results)):
        assert np.array_equal(a, b), 'tensor %d differs between training behind a reserve and training alone' % k


# slk_poolnet_train's refusals: (what, arguments that differ from a good call, text of the error), in the order the rules are
# checked in.  A good call: 2 sequences of 4 over 5 items at dim 8, minibatches of 2, bpr.  `ptr`: the case is one of a pointer
# or of padding_idx, which slk_poolnet_reserve does not take.
SEQ_REFUSALS = [
    ('warp', dict(loss='warp'), 'slk_poolnet_train: warp (loss kind 7) is not built for the sequence model', False),
    ('loss kind above the range', dict(loss=8), 'unknown loss kind 8', False),
    ('loss kind below the range', dict(loss=-1), 'unknown loss kind -1', False),
    ('adaptive hinge, no negatives', dict(loss='adaptive_hinge', n_neg=0), 'num_negative_samples 0 outside [1, 1024]', False),
    ('adaptive hinge, 1025 negatives', dict(loss='adaptive_hinge', n_neg=1025), 'num_negative_samples 1025 outside [1, 1024]', False),
    ('padding_idx == num_items', dict(padding_idx=5), 'padding_idx 5 outside [-1, num_items)', True),
    ('padding_idx -2', dict(padding_idx=-2), 'padding_idx -2 outside [-1, num_items)', True),
    ('seq_len 0', dict(seq_len=0), 'slk_poolnet_train: n_seq 2 batch_size 2 seq_len 0', False),
    ('batch_size 0', dict(batch_size=0), 'slk_poolnet_train: n_seq 2 batch_size 0 seq_len 4', False),
    ('n_seq < 0', dict(n_seq=-1), 'slk_poolnet_train: n_seq -1 batch_size 2 seq_len 4', False),
    ('NULL d_sequences', dict(seqs=None), 'slk_poolnet_train: NULL pointer', True),
    ('LDS bound', dict(seq_len=100000), 'sequence length 100000 x dim 8 does not fit the 160 KB LDS of a CU', False),
    ('2^31 lookups per minibatch', dict(n_seq=1 << 28, batch_size=1 << 28), 'batch_size * seq_len * lookups per timestep must be < 2^31', False),
    # where a call breaks two rules, the first one answers
    ('warp and a bad padding_idx', dict(loss='warp', padding_idx=5), 'slk_poolnet_train: warp (loss kind 7)', True),
    ('bad padding_idx and NULL pointers', dict(padding_idx=5, seqs=None, mb_loss=None), 'padding_idx 5 outside [-1, num_items)', True),
]


def check_seq_refusals(be):
    """Every refusal of slk_poolnet_train, by its text (SEQ_REFUSALS); an empty call with NULL pointers succeeds; and
    slk_poolnet_reserve refuses what it can be asked with the same code and the same text."""
    from spotlight_amd import _native
    eng = be.engine
    dev = be.seq_model([np.zeros((5, 8)), np.zeros(5)])
    seqs = be.alloc(np.zeros((2, 4), dtype=np.int64))
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))

    def refusal(call, *args, **kwargs):
        try:
            call(*args, **kwargs)
        except _native.SlkError as e:
            return e.code, str(e)
        return None

    for what, change, text, ptr in SEQ_REFUSALS:
        a = dict(padding_idx=0, seqs=seqs, n_seq=2, seq_len=4, batch_size=2, loss='bpr', n_neg=1, mb_loss=mb_loss)
        a.update(change)
        got = refusal(eng.poolnet_train, dev.tables, dev.optim, a['padding_idx'], be.ptr(a['seqs']), a['n_seq'], a['seq_len'],
                      a['batch_size'], a['loss'], a['n_neg'], be.ptr(a['mb_loss']), stream=be.stream)
        assert got is not None, 'slk_poolnet_train accepted: ' + what
        assert got[0] == _native.SLK_EINVAL and text in got[1], (what, got)
        if not ptr:
            again = refusal(eng.poolnet_reserve, dev.tables, dev.optim, a['n_seq'], a['seq_len'], a['batch_size'], a['loss'], a['n_neg'],
                            stream=be.stream)
            assert again == got, (what, again, got)
    assert dev.optim.step == 0
    eng.poolnet_train(dev.tables, dev.optim, 0, None, 0, 4, 2, 'bpr', 1, None, stream=be.stream)  # nothing to do: no pointer is read
    assert dev.optim.step == 0


def check_seq_route_that_was_meant_ran(be, D=16, I=2000, N=300, L=24, B=32, chunk=2048, seed=17):
    """The 5 chunks of check_seq_chunking_is_bit_neutral's call: with "overlap_prep" 1 the prep of 4 of them runs beside the chunk
    before (the statistic counts them, call by call), with 0 none does; either way the call launches the same kernels, class by
    class."""
    eng = be.engine
    launches = []
    for overlap, rise in ((0, 0), (1, 4)):
        with eng.options(chunk_interactions=chunk, overlap_prep=overlap, overlap_min_batch=0):
            seqs, dev, state = _seq_case(be, 'adagrad', D, I, N, L, 0, seed)
            eng.rng_set_state(state)
            d_seqs = be.alloc(seqs)
            mb_loss = be.alloc(np.zeros((N + B - 1) // B, dtype=np.float32))
            eng.profile_reset()
            eng.profile_enable(True)
            try:
                for _ in range(2):
                    before = eng.get_stat('overlapped_chunks')
                    eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), N, L, B, 'bpr', 1, be.ptr(mb_loss), stream=be.stream)
                    assert eng.get_stat('overlapped_chunks') - before == rise, (overlap, eng.get_stat('overlapped_chunks') - before)
                launches.append({name: n for name, (n, _) in eng.profile_read().items()})
            finally:
                eng.profile_enable(False)
                eng.profile_reset()
    assert launches[0] == launches[1], launches
    assert launches[0]['seq_pass'] == 2 * ((N + B - 1) // B)


def check_bilinear_prefetch_behind_a_seq_call(be, D=8, U=60, I=50, N=700, B=128, chunk=256, seed=37):
    """Both training drivers leave the ctx's record of the last pipelined buffer set in the same way, so a
    slk_bilinear_prefetch behind a sequence call -- pipelined or in line -- knows which set it may overwrite: the prefetched
    bilinear call (3 chunks) gives what it gives on a fresh engine, bit for bit.  (Values only: an ordering fault between the
    two streams would not show here.)"""
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), np.zeros(U), np.zeros(I)]
    state = np.random.RandomState(seed + 1).get_state()

    def bilinear(be):
        eng = be.engine
        with eng.options(chunk_interactions=chunk, overlap_prep=1, overlap_min_batch=0, epoch_kernel=0):
            dev = be.model(params, opt='adagrad', lr=0.05)
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros((N + B - 1) // B, dtype=np.float32))
            neg_out = be.alloc(np.full(N, -1, dtype=np.int64))
            eng.rng_set_state(state)
            eng.bilinear_prefetch(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1, stream=be.stream)
            assert eng.get_stat('prefetch_pending') > 0
            eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1, be.ptr(mb_loss),
                               d_neg_out=be.ptr(neg_out), stream=be.stream)
            st = eng.rng_get_state()
            return [be.get(mb_loss), be.get(neg_out), st[1], np.array(st[2])] + [be.get(x) for x in dev.p + dev.s1]

    fresh = type(be)()
    try:
        want = bilinear(fresh)
    finally:
        fresh.close()
    for seq_overlap in (1, 0):
        with be.engine.options(chunk_interactions=2048, overlap_prep=seq_overlap, overlap_min_batch=0):
            seqs, dev, seq_state = _seq_case(be, 'adagrad', 16, 2000, 300, 24, 0, 17)
            be.engine.rng_set_state(seq_state)
            _seq_train_twice(be, dev, seqs, 32, 'bpr', 1)
        for k, (a, b) in enumerate(zip(bilinear(be), want)):
            assert np.array_equal(a, b), ('tensor %d of a prefetched bilinear call differs behind a sequence call (overlap_prep %d)'
                                          % (k, seq_overlap))


def check_seq_single_step_gradients(be, loss, D, I=40, B=24, L=11, nn=3, seed=11, bloom=0, ratio=0.4, tol=1e-5):
    """Identical minibatch and parameters: loss within 1e-5 rel, summed gradients within 1e-5 of
    each table's inf-norm; read back through ADAM_DENSE with lr = 0, beta1 = 0."""
    from oracle.oracle import PoolNetOracle, bloom_desc
    eng = be.engine
    rs = np.random.RandomState(seed)
    seqs = make_sequences(rs, B, L, I)
    n_draw = B * L * (nn if loss == 'adaptive_hinge' else 1)
    negs = rs.randint(0, I, n_draw).astype(np.int64)
    desc = bloom_desc(n_hash=bloom) if bloom else None
    params = _seq_params(rs, I, D, rows=int(ratio * I) if bloom else None)
    want_loss, want_g = PoolNetOracle(*params, opt='adagrad', item_bloom=desc).step(seqs, negs, loss=loss, n_neg=nn,
                                                                                   want_grads=True)
    dev = be.seq_model(params, opt='adam_dense', lr=0.0, betas=(0.0, 0.999), item_bloom=desc)
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_seqs, d_negs = be.alloc(seqs), be.alloc(negs)
    eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), B, L, B, loss, nn, be.ptr(mb_loss),
                      d_neg_in=be.ptr(d_negs), stream=be.stream)
    assert abs(float(be.get(mb_loss)[0]) - want_loss) / abs(want_loss) < 1e-5
    for t in range(2):
        got = be.get(dev.s1[t])
        assert np.abs(got.ravel() - want_g[t].ravel()).max() <= tol * np.abs(want_g[t]).max(), t
        assert np.array_equal(be.get(dev.p[t]).ravel(), np.asarray(params[t], np.float32).ravel())


def check_seq_replays_reference_fixture(be, golden_dir, name):
    """Sequence fixtures recorded from the live reference (oracle/make_golden_seq.py)."""
    from oracle.oracle import bloom_desc
    from oracle.replay import case_from_rec, _oracle_hparams
    eng = be.engine
    rec = np.load(os.path.join(golden_dir, name + '.npz'))
    case = case_from_rec(rec)
    desc = bloom_desc(n_hash=int(case['bloom'])) if int(case.get('bloom', 0)) else None
    dev = be.seq_model([rec['init_0'], rec['init_1']], opt=ORACLE_OPT[str(case['opt'])], item_bloom=desc,
                       **_oracle_hparams(case))
    state = ('MT19937', rec['rng_key_before_fit'], int(rec['rng_pos_before_fit']))
    eng.rng_set_state(state)
    host = Rng(state=state)
    nn = int(case.get('n_neg', 5)) if case['loss'] == 'adaptive_hinge' else 1
    N, L, B = int(case['N']), int(case['L']), int(case['B'])
    n_mb = (N + B - 1) // B
    seqs = rec['sequences'].astype(np.int64)
    losses, negs = [], []
    for e in range(int(case['n_iter'])):
        host.set_state(eng.rng_get_state())
        seqs = seqs[host.shuffle_perm(N)]  # epochs compose (sequence/implicit.py:215-216)
        eng.rng_set_state(host.get_state())
        assert (seqs == rec['shuffled'][e]).all()
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.empty(N * L * nn, dtype=np.int64))
        d_seqs = be.alloc(seqs)
        eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), N, L, B, str(case['loss']), nn, be.ptr(mb_loss),
                          d_neg_out=be.ptr(neg_out), stream=be.stream)
        losses.append(be.get(mb_loss))
        negs.append(be.get(neg_out))
    assert (np.concatenate(negs) == rec['negatives']).all()
    losses = np.concatenate(losses)
    assert abs(losses[0] - rec['losses'][0]) / abs(rec['losses'][0]) < 1e-5
    assert np.max(np.abs(losses - rec['losses']) / np.abs(rec['losses'])) < 1e-3
    st = eng.rng_get_state()
    assert (st[1] == rec['rng_key_after_fit']).all() and st[2] == int(rec['rng_pos_after_fit'])
    for t in range(2):  # coarse open-loop drift sanity; the element-wise statement is the closed loop below
        ref = rec['final_%d' % t]
        assert_open_loop_drift(be.get(dev.p[t]), ref, (name, t))
    open_tables = [be.get(dev.p[t]).copy() for t in range(2)]
    # ---- closed loop (see check_replays_reference_fixture): every minibatch from the engine's own tables, one oracle step
    from oracle.oracle import PoolNetOracle
    opt, hp = ORACLE_OPT[str(case['opt'])], _oracle_hparams(case)
    dev2 = be.seq_model([rec['init_0'], rec['init_1']], opt=opt, item_bloom=desc, **hp)
    step = 0
    for e in range(int(case['n_iter'])):
        sh = rec['shuffled'][e].astype(np.int64)
        base = e * N * L * nn
        for off in range(0, N, B):
            hi = min(off + B, N)
            neg = rec['negatives'][base + off * L * nn:base + hi * L * nn].astype(np.int64)
            pre_p = [be.get(x).copy() for x in dev2.p]
            pre_s1 = [be.get(x).copy() for x in dev2.s1]
            pre_s2 = [be.get(x).copy() for x in dev2.s2]
            ora = PoolNetOracle(pre_p[0], pre_p[1], opt=opt, state1=pre_s1, state2=pre_s2, step=step, item_bloom=desc, **hp)
            want_loss, g = ora.step(sh[off:hi], neg, loss=str(case['loss']), n_neg=nn, want_grads=True)
            step += 1
            d_seqs, d_neg = be.alloc(sh[off:hi]), be.alloc(neg)
            mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
            eng.poolnet_train(dev2.tables, dev2.optim, 0, be.ptr(d_seqs), hi - off, L, B, str(case['loss']), nn, be.ptr(mb_loss),
                              d_neg_in=be.ptr(d_neg), stream=be.stream)
            assert abs(float(be.get(mb_loss)[0]) - want_loss) <= 1e-5 * abs(want_loss), (e, off)
            assert_step_within_bounds(be, dev2, ora, pre_p, pre_s1, pre_s2, g, step, opt, hp, bias_tables=(1,), what='seq')
    for t in range(2):
        assert np.array_equal(be.get(dev2.p[t]), open_tables[t]), ('closed-loop run differs from the open-loop one', t)
    # predictions on the reference's final tables
    fin = be.seq_model([rec['final_0'], rec['final_1']], item_bloom=desc)
    out = be.alloc(np.empty(int(case['I']), dtype=np.float32))
    d_seq = be.alloc(rec['predict_seq'].astype(np.int64))
    eng.poolnet_predict(fin.tables, be.ptr(d_seq), L, None, int(case['I']), be.ptr(out), be.stream)
    assert rel_inf(be.get(out), rec['predict_all']) < 1e-5


SEQ_FIXTURES = ['seq_bpr_adagrad_sparse', 'seq_hinge_sparse_adam', 'seq_pointwise_adam_default',
                'seq_adaptive_hinge_adagrad', 'seq_d64_bpr_adagrad', 'seq_d32_adaptive_adam',
                # PoolNet over a BloomEmbedding item layer (oracle/make_golden_seq.py bloom)
                'seq_bloom_bpr_adagrad', 'seq_bloom_pointwise_adam_default', 'seq_bloom_hinge_adagrad',
                'seq_bloom_adaptive_hinge_adagrad', 'seq_bloom_d64_bpr_adagrad']


# ---------------------------------------------------------------------------------------
# BilinearNet with BloomEmbedding layers
# ---------------------------------------------------------------------------------------
def _bloom_setup(rs, U, I, D, user_bloom, item_bloom, ratio):
    from oracle.oracle import bloom_desc
    sc = min(0.3, 1.0 / np.sqrt(D))
    ud = bloom_desc(n_hash=user_bloom) if user_bloom else None
    idesc = bloom_desc(n_hash=item_bloom) if item_bloom else None
    ru = int(ratio * U) if ud else U
    ri = int(ratio * I) if idesc else I
    params = [rs.normal(0, sc, (ru, D)).astype(np.float32), rs.normal(0, sc, (ri, D)).astype(np.float32),
              rs.normal(0, 0.1, U).astype(np.float32), rs.normal(0, 0.1, I).astype(np.float32)]
    if ud:
        params[0][0] = 0.0  # the compressed table's padding row (layers.py:167-169)
    if idesc:
        params[1][0] = 0.0
    return params, ud, idesc


def check_bloom_train_matches_oracle(be, loss, opt, D, user_bloom=0, item_bloom=4, U=45, I=60, N=170, B=64, nn=3,
                                     epochs=2, ratio=0.4, tol=2e-5, seed=5):
    from oracle.oracle import BloomBilinearOracle
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    params, ud, idesc = _bloom_setup(rs, U, I, D, user_bloom, item_bloom, ratio)
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    ora = BloomBilinearOracle(*params, user_bloom=ud, item_bloom=idesc, opt=opt, **hp)
    dev = be.model(params, opt=opt, user_bloom=ud, item_bloom=idesc, **hp)
    state = np.random.RandomState(9).get_state()
    orng = Rng(state=state)
    eng.rng_set_state(state)
    n_mb = (N + B - 1) // B
    d_users, d_items = be.alloc(users), be.alloc(items)
    for epoch in range(epochs):
        want_loss, want_neg = ora.train(orng, users, items, B, loss=loss, n_neg=nn, want_negs=True)
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.full(want_neg.size, -1, dtype=np.int64))
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn,
                           be.ptr(mb_loss), d_neg_out=be.ptr(neg_out), stream=be.stream)
        assert (be.get(neg_out) == want_neg).all()
        got_loss = be.get(mb_loss)
        assert np.abs(got_loss - want_loss).max() / np.abs(want_loss).max() < 1e-5, (got_loss, want_loss)
    for t in range(4):
        assert_close_table(be.get(dev.p[t]), ora.p[t], tol, ('param', t))
        assert_close_table(be.get(dev.s1[t]), ora.s1[t], tol, ('state1', t))
    if ud:
        assert (be.get(dev.p[0])[0] == 0).all()  # padding rows of the compressed tables stay zero
    if idesc:
        assert (be.get(dev.p[1])[0] == 0).all()
    # predict (scalar user vs all items; pairs) on the engine's own tables
    po = BloomBilinearOracle(*[be.get(x) for x in dev.p], user_bloom=ud, item_bloom=idesc)
    out = be.alloc(np.empty(I, dtype=np.float32))
    d_u = be.alloc(np.array([3], dtype=np.int64))
    eng.bilinear_predict(dev.tables, be.ptr(d_u), 1, None, I, be.ptr(out), be.stream)
    assert rel_inf(be.get(out), po.predict(3)) < 1e-5
    m = min(50, N)
    out = be.alloc(np.empty(m, dtype=np.float32))
    d_pu, d_pi = be.alloc(users[:m].copy()), be.alloc(items[:m].copy())
    eng.bilinear_predict(dev.tables, be.ptr(d_pu), m, be.ptr(d_pi), m, be.ptr(out), be.stream)
    assert rel_inf(be.get(out), po.predict(users[:m], items[:m])) < 1e-5


def check_bloom_single_step_gradients(be, loss, D, user_bloom=0, item_bloom=4, U=50, I=70, B=128, nn=3, seed=11):
    from oracle.oracle import BloomBilinearOracle
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, B).astype(np.int64)
    items = rs.randint(0, I, B).astype(np.int64)
    negs = rs.randint(0, I, B * (nn if loss == 'adaptive_hinge' else 1)).astype(np.int64)
    params, ud, idesc = _bloom_setup(rs, U, I, D, user_bloom, item_bloom, 0.4)
    want_loss, want_g = BloomBilinearOracle(*params, user_bloom=ud, item_bloom=idesc).step(
        users, items, negs, loss=loss, n_neg=nn, want_grads=True)
    dev = be.model(params, opt='adam_dense', lr=0.0, betas=(0.0, 0.999), user_bloom=ud, item_bloom=idesc)
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_users, d_items, d_negs = be.alloc(users), be.alloc(items), be.alloc(negs)
    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), B, B, loss, nn, be.ptr(mb_loss),
                       d_neg_in=be.ptr(d_negs), stream=be.stream)
    assert abs(float(be.get(mb_loss)[0]) - want_loss) / abs(want_loss) < 1e-5
    bscale = max(np.abs(want_g[2]).max(), np.abs(want_g[3]).max())
    for t in range(4):
        scale = np.abs(want_g[t]).max() if t < 2 else bscale
        assert np.abs(be.get(dev.s1[t]).ravel() - want_g[t].ravel()).max() <= 1e-5 * scale, t


def check_bloom_replays_reference_fixture(be, golden_dir, name):
    """Fixtures recorded from the live reference with BloomEmbedding layers (oracle/make_golden_bloom.py)."""
    from oracle.oracle import bloom_desc
    from oracle.replay import case_from_rec, _oracle_hparams
    eng = be.engine
    rec = np.load(os.path.join(golden_dir, name + '.npz'))
    case = case_from_rec(rec)
    mk = lambda on: bloom_desc(n_hash=int(case['H'])) if int(on) else None
    dev = be.model([rec['init_%d' % t] for t in range(4)], opt=ORACLE_OPT[str(case['opt'])],
                   user_bloom=mk(case['user_bloom']), item_bloom=mk(case['item_bloom']), **_oracle_hparams(case))
    state = ('MT19937', rec['rng_key_before_fit'], int(rec['rng_pos_before_fit']))
    eng.rng_set_state(state)
    host = Rng(state=state)
    nn = int(case.get('n_neg', 5)) if case['loss'] == 'adaptive_hinge' else 1
    N, B = int(case['N']), int(case['B'])
    n_mb = (N + B - 1) // B
    losses, negs = [], []
    for e in range(int(case['n_iter'])):
        host.set_state(eng.rng_get_state())
        perm = host.shuffle_perm(N)
        eng.rng_set_state(host.get_state())
        su, si = rec['users'].astype(np.int64)[perm], rec['items'].astype(np.int64)[perm]
        assert (su == rec['shuffled_users'][e]).all()
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        neg_out = be.alloc(np.empty(N * nn, dtype=np.int64))
        d_su, d_si = be.alloc(su), be.alloc(si)
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_su), be.ptr(d_si), N, B, str(case['loss']), nn,
                           be.ptr(mb_loss), d_neg_out=be.ptr(neg_out), stream=be.stream)
        losses.append(be.get(mb_loss))
        negs.append(be.get(neg_out))
    assert (np.concatenate(negs) == rec['negatives']).all()
    losses = np.concatenate(losses)
    assert abs(losses[0] - rec['losses'][0]) / abs(rec['losses'][0]) < 1e-5
    assert np.max(np.abs(losses - rec['losses']) / np.abs(rec['losses'])) < 1e-3
    for t in range(4):  # coarse open-loop drift sanity; the element-wise statement is the closed loop below
        ref = rec['final_%d' % t]
        assert_open_loop_drift(be.get(dev.p[t]), ref, (name, t))
    open_tables = [be.get(dev.p[t]).copy() for t in range(4)]
    # ---- closed loop (see check_replays_reference_fixture)
    from oracle.oracle import BloomBilinearOracle
    opt, hp = ORACLE_OPT[str(case['opt'])], _oracle_hparams(case)
    dev2 = be.model([rec['init_%d' % t] for t in range(4)], opt=opt, user_bloom=mk(case['user_bloom']),
                    item_bloom=mk(case['item_bloom']), **hp)
    step = 0
    for e in range(int(case['n_iter'])):
        su, si = rec['shuffled_users'][e].astype(np.int64), rec['shuffled_items'][e].astype(np.int64)
        for off in range(0, N, B):
            hi = min(off + B, N)
            neg = rec['negatives'][(e * N + off) * nn:(e * N + hi) * nn].astype(np.int64)
            pre_p = [be.get(x).copy() for x in dev2.p]
            pre_s1 = [be.get(x).copy() for x in dev2.s1]
            pre_s2 = [be.get(x).copy() for x in dev2.s2]
            ora = BloomBilinearOracle(*pre_p, user_bloom=mk(case['user_bloom']), item_bloom=mk(case['item_bloom']), opt=opt,
                                      step=step, **hp)
            for t in range(4):
                ora.s1[t][...] = pre_s1[t].reshape(ora.s1[t].shape)
                ora.s2[t][...] = pre_s2[t].reshape(ora.s2[t].shape)
            want_loss, g = ora.step(su[off:hi], si[off:hi], neg, loss=str(case['loss']), n_neg=nn, want_grads=True)
            step += 1
            d_su, d_si, d_neg = be.alloc(su[off:hi]), be.alloc(si[off:hi]), be.alloc(neg)
            mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
            eng.bilinear_train(dev2.tables, dev2.optim, be.ptr(d_su), be.ptr(d_si), hi - off, B, str(case['loss']), nn,
                               be.ptr(mb_loss), d_neg_in=be.ptr(d_neg), stream=be.stream)
            assert abs(float(be.get(mb_loss)[0]) - want_loss) <= 1e-5 * abs(want_loss), (e, off)
            assert_step_within_bounds(be, dev2, ora, pre_p, pre_s1, pre_s2, g, step, opt, hp, what='bloom')
    for t in range(4):
        assert np.array_equal(be.get(dev2.p[t]), open_tables[t]), ('closed-loop run differs from the open-loop one', t)


BLOOM_FIXTURES = ['bloom_item_bpr_adagrad', 'bloom_item_adaptive_hinge_adam_default', 'bloom_both_bpr_adagrad',
                  'bloom_both_adaptive_adam', 'bloom_user_pointwise_adagrad', 'bloom_c3_adaptive_adagrad']


def check_chunking_is_bit_neutral(be, loss, opt, D, U=3000, I=1000, N=30000, B=1000, nn=5, user_bloom=0, item_bloom=0,
                                  chunk=4096, overlap=1, seed=21, nt=None, hp=None, step0=0):
    """The engine is deterministic (sorted ownership, no atomics), and chunking / the prep pipeline
    only change WHEN value-independent work happens: one big chunk on one stream and many small
    chunks with prep on the second stream must agree bit for bit -- losses, negatives, every table,
    every optimizer-state tensor and the final RNG state.
    `hp`: the optimizer's hyper-parameters in place of lr = 0.05 and defaults; `step0`: steps already taken."""
    hp = dict(lr=0.05) if hp is None else hp
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    params, ud, idesc = _bloom_setup(rs, U, I, D, user_bloom, item_bloom, 0.2)
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    n_draw = N * (nn if loss == 'adaptive_hinge' else 1)
    results = []
    for chunk_i, overlap_i in ((1 << 23, 0), (chunk, overlap)):
        eng.set_option('chunk_interactions', chunk_i)
        eng.set_option('overlap_prep', overlap_i)
        eng.set_option('overlap_min_batch', 0)  # (by default only minibatches >= 2^16 overlap their prep)
        if nt is not None and chunk_i == chunk:  # the second run also uses another cache policy
            eng.set_option('nt', nt)
        try:
            dev = be.model(params, opt=opt, user_bloom=ud, item_bloom=idesc, **hp)
            dev.optim.step = step0
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
            neg_out = be.alloc(np.full(n_draw, -1, dtype=np.int64))
            for _ in range(2):
                eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn,
                                   be.ptr(mb_loss), d_neg_out=be.ptr(neg_out), stream=be.stream)
            assert dev.optim.step == step0 + 2 * n_mb
            st = eng.rng_get_state()
            results.append([be.get(mb_loss), be.get(neg_out), st[1], np.array(st[2])] +
                           [be.get(x) for x in dev.p + dev.s1 + dev.s2])
        finally:
            eng.set_option('chunk_interactions', 1 << 23)
            eng.set_option('overlap_prep', 0)
            eng.set_option('overlap_min_batch', 1 << 16)
            if nt is not None:
                eng.set_option('nt', 3)
    for k, (a, b) in enumerate(zip(*results)):
        assert np.array_equal(a, b), ('tensor %d differs between one chunk and the pipelined run' % k,
                                      float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))


def check_user_bias_zero_hint_is_bit_neutral(be, D=16, U=3000, I=1000, N=20000, B=4096, seed=29):
    """include/spotlight_hip.h, SLK_TABLES_USER_BIAS_ZERO: with user biases that ARE identically zero the pair-mode user pass may skip
    fetching them.  Under bpr / hinge (row-sparse Adagrad, plain SGD) a run with the hint equals the run without it bit for bit --
    every table, every state tensor, the losses -- and the user biases are still all zero afterwards (their gradient is exactly
    zero).  Routes the hint does not cover (pointwise: the user bias DOES get a gradient there) ignore it: same equality."""
    from spotlight_amd import _native
    eng = be.engine
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), np.zeros(U), rs.normal(0, 0.1, I)]
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    eng.set_option('epoch_kernel', 0)  # (the launch path; the persistent kernel does not look at the hint)
    try:
        for loss, opt in (('bpr', 'adagrad'), ('hinge', 'sgd'), ('pointwise', 'adagrad'), ('bpr', 'sparse_adam')):
            results = []
            for hinted in (False, True):
                dev = be.model(params, opt=opt, lr=0.05)
                if hinted:
                    dev.tables.flags = _native.TABLES_USER_BIAS_ZERO
                eng.rng_set_state(state)
                d_users, d_items = be.alloc(users), be.alloc(items)
                mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
                for _ in range(2):
                    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, 1, be.ptr(mb_loss),
                                       stream=be.stream)
                results.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
            for k, (a, b) in enumerate(zip(*results)):
                assert np.array_equal(a, b), ('%s / %s: tensor %d differs with the user-bias hint' % (loss, opt, k))
            if loss != 'pointwise':
                assert not results[1][3].any(), 'user biases moved under a loss whose user-bias gradient is zero'
    finally:
        eng.set_option('epoch_kernel', 1)


def check_prefetch_behind_an_inline_draw(be, D=16, U=3000, I=1000, N=30000, B=1000, chunk=4096, seed=23):
    """slk_bilinear_prefetch used to assume that every earlier user of the sampler's scratch and of the RNG state ran on
    the ctx's prep stream.  An in-line slk_sample_items (the caller's stream) followed by a prefetch WITHOUT a host synchronisation
    in between must still draw the stream in order: the sampled ids, the training call's negatives, its tables and the final RNG
    state equal those of the same sequence with nothing prepared ahead, bit for bit.  (Run twice: the second round's prefetch
    follows a PIPELINED training call, the first one an in-line state.)"""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), np.zeros(U), np.zeros(I)]
    state = np.random.RandomState(seed + 1).get_state()
    M = 5000
    results = []
    for ahead in (False, True):
        eng.set_option('chunk_interactions', chunk)
        eng.set_option('overlap_prep', 1)
        eng.set_option('overlap_min_batch', 0)
        eng.set_option('epoch_kernel', 0)  # (the persistent route of small minibatches prepares nothing ahead)
        try:
            dev = be.model(params, opt='adagrad', lr=0.05)
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            n_mb = (N + B - 1) // B
            outs = []
            for _ in range(2):
                drawn = be.alloc(np.full(M, -1, dtype=np.int64))
                mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
                neg_out = be.alloc(np.full(N, -1, dtype=np.int64))
                eng.sample_items(I, M, be.ptr(drawn), be.stream)  # in line, on the caller's stream
                if ahead:
                    eng.bilinear_prefetch(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1, stream=be.stream)
                    assert eng.get_stat('prefetch_pending') > 0
                eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1, be.ptr(mb_loss),
                                   d_neg_out=be.ptr(neg_out), stream=be.stream)
                outs += [be.get(drawn), be.get(mb_loss), be.get(neg_out)]
            st = eng.rng_get_state()
            results.append(outs + [st[1], np.array(st[2])] + [be.get(x) for x in dev.p + dev.s1])
        finally:
            eng.set_option('chunk_interactions', 1 << 23)
            eng.set_option('overlap_prep', 0)
            eng.set_option('overlap_min_batch', 1 << 16)
            eng.set_option('epoch_kernel', 1)
    ref = np.random.RandomState(seed + 1)
    assert np.array_equal(results[0][0], ref.randint(0, I, M, dtype=np.int64))  # and the stream itself is numpy's
    assert np.array_equal(results[0][2], ref.randint(0, I, N, dtype=np.int64))
    for k, (a, b) in enumerate(zip(*results)):
        assert np.array_equal(a, b), ('tensor %d differs between the prefetched and the in-line sequence' % k)


# ---------------------------------------------------------------------------------------
# epoch shuffle on the device (slk_shuffle_perm)
# ---------------------------------------------------------------------------------------
def check_shuffle_matches_numpy(be, n, seed, burn=7, rows=0, band=1):
    """d_perm == numpy's RandomState.shuffle(arange(n)) bit for bit, same RandomState afterwards
    (torch_utils.py:35-52); `rows` > 0 also checks slk_gather_rows_i64 on an [n, rows] array.
    band: 1 = the banded draws (default; no range may fall back to the full sweeps), 0 = the full sweeps only,
    > 1 = a band that many times too narrow, so that ranges DO leave it and are redone (the fall-back path)."""
    eng = be.engine
    eng.set_option('shuffle_band', band)
    try:
        _check_shuffle_matches_numpy(be, n, seed, burn, rows)
        if n > 4096:
            if band == 1:
                assert eng.get_stat('shuffle_fallbacks') == 0 and eng.get_stat('shuffle_sweeps') == 0
            elif band == 0:
                assert eng.get_stat('shuffle_sweeps') > 0 and eng.get_stat('shuffle_fallbacks') == 0
            elif band >= 8:
                assert eng.get_stat('shuffle_fallbacks') > 0 and eng.get_stat('shuffle_sweeps') > 0
    finally:
        eng.set_option('shuffle_band', 1)


def _check_shuffle_matches_numpy(be, n, seed, burn, rows):
    eng = be.engine
    rs = np.random.RandomState(seed)
    if burn:
        rs.randint(0, 1000, burn)  # leave the block start
    eng.rng_set_state(rs.get_state())
    want = np.arange(n)
    rs.shuffle(want)
    d_perm = be.alloc(np.full(max(n, 1), -1, dtype=np.int64))
    eng.shuffle_perm(n, be.ptr(d_perm), stream=be.stream)
    got = be.get(d_perm)[:n]
    st, ref = eng.rng_get_state(), rs.get_state()
    assert np.array_equal(got, want), (n, int((got != want).sum()))
    assert (st[1] == ref[1]).all() and st[2] == ref[2], 'RandomState after the shuffle differs'
    if rows and n:
        src = np.arange(n * rows, dtype=np.int64).reshape(n, rows) * 3 + 1
        d_src, d_dst = be.alloc(src), be.alloc(np.zeros_like(src))
        eng.gather_rows_i64(be.ptr(d_src), be.ptr(d_perm), n, rows, be.ptr(d_dst), stream=be.stream)
        assert np.array_equal(be.get(d_dst), src[want])
    if n:
        # both id arrays of fit() through the permutation from their packed 32-bit form (slk_pack_id_pairs / slk_gather_id_pairs)
        ids = np.random.RandomState(seed + 1)
        users, items = ids.randint(0, 1 << 31, n).astype(np.int64), ids.randint(0, 1 << 31, n).astype(np.int64)
        users[0], items[-1] = (1 << 32) - 1, 0  # the whole 32-bit range survives the narrowing
        d_u, d_i, d_pairs = be.alloc(users), be.alloc(items), be.alloc(np.zeros(2 * n, dtype=np.uint32))
        d_uo, d_io = be.alloc(np.zeros(n, dtype=np.int64)), be.alloc(np.zeros(n, dtype=np.int64))
        eng.pack_id_pairs(be.ptr(d_u), be.ptr(d_i), n, be.ptr(d_pairs), stream=be.stream)
        eng.gather_id_pairs(be.ptr(d_pairs), be.ptr(d_perm), n, be.ptr(d_uo), be.ptr(d_io), stream=be.stream)
        assert np.array_equal(be.get(d_pairs).reshape(n, 2), np.stack([users, items], 1).astype(np.uint32))
        assert np.array_equal(be.get(d_uo), users[want]) and np.array_equal(be.get(d_io), items[want])
    # the negatives drawn next continue the same stream
    d_neg = be.alloc(np.zeros(64, dtype=np.int64))
    eng.sample_items(1000, 64, be.ptr(d_neg), stream=be.stream)
    assert np.array_equal(be.get(d_neg), rs.randint(0, 1000, 64, dtype=np.int64))


# ---------------------------------------------------------------------------------------
# explicit feedback (slk_bilinear_train_explicit)
# ---------------------------------------------------------------------------------------
EXPLICIT_LOSSES = ('regression', 'poisson', 'logistic')
EXPLICIT_FIXTURES = ['explicit_regression_adam_default', 'explicit_regression_adagrad', 'explicit_poisson_adagrad',
                     'explicit_poisson_sparse_adam', 'explicit_logistic_adam_default', 'explicit_logistic_sparse_adam',
                     'explicit_d64_regression_adagrad']


def _ratings_for(rs, loss, n):
    if loss == 'logistic':
        return rs.choice([-1.0, 1.0], n).astype(np.float32)
    if loss == 'poisson':
        return rs.poisson(2.0, n).astype(np.float32)
    return rs.randint(1, 6, n).astype(np.float32)


def check_explicit_train_matches_oracle(be, loss, opt, D, U=37, I=29, N=300, B=64, epochs=2, tol=2e-5, seed=5,
                                        user_bloom=0, item_bloom=0):
    """ExplicitFactorizationModel's minibatch loop (factorization/explicit.py:213-236) against the oracle:
    per-minibatch losses, tables and optimizer state; no RNG draws are made."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    ratings = _ratings_for(rs, loss, N)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)).astype(np.float32), rs.normal(0, sc, (I, D)).astype(np.float32),
              rs.normal(0, 0.1, U).astype(np.float32), rs.normal(0, 0.1, I).astype(np.float32)]
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    ora = BilinearOracle(*params, opt=opt, sparse_grads=True, **hp)
    dev = be.model(params, opt=opt, **hp)
    state = np.random.RandomState(9).get_state()
    eng.rng_set_state(state)
    n_mb = (N + B - 1) // B
    d_users, d_items, d_ratings = be.alloc(users), be.alloc(items), be.alloc(ratings)
    for epoch in range(epochs):
        want = ora.explicit_train(users, items, ratings, B, loss=loss)
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), be.ptr(d_ratings), N, B,
                                    loss, be.ptr(mb_loss), stream=be.stream)
        got = be.get(mb_loss)
        assert np.abs(got - want).max() / np.abs(want).max() < 1e-5, (got, want)
    assert dev.optim.step == ora.step_count == epochs * n_mb
    for t in range(4):
        assert_close_table(be.get(dev.p[t]), ora.p[t], tol, ('param', t))
        assert_close_table(be.get(dev.s1[t]), ora.s1[t], tol, ('state1', t))
    st = eng.rng_get_state()
    assert (st[1] == state[1]).all() and st[2] == state[2]  # the explicit path draws nothing


def check_explicit_single_step_gradients(be, loss, D, U=50, I=40, B=128, seed=11):
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, B).astype(np.int64)
    items = rs.randint(0, I, B).astype(np.int64)
    ratings = _ratings_for(rs, loss, B)
    params = [rs.normal(0, 0.3, (U, D)), rs.normal(0, 0.3, (I, D)), rs.normal(0, 0.2, U), rs.normal(0, 0.2, I)]
    want_loss, want_g = BilinearOracle(*params, opt='adagrad', sparse_grads=True).explicit_step(
        users, items, ratings, loss=loss, want_grads=True)
    dev = be.model(params, opt='adam_dense', lr=0.0, betas=(0.0, 0.999))
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_users, d_items, d_ratings = be.alloc(users), be.alloc(items), be.alloc(ratings)
    eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), be.ptr(d_ratings), B, B, loss,
                                be.ptr(mb_loss), stream=be.stream)
    assert abs(float(be.get(mb_loss)[0]) - want_loss) / abs(want_loss) < 1e-5
    for t in range(4):
        got = be.get(dev.s1[t])
        assert np.abs(got.ravel() - want_g[t].ravel()).max() <= 1e-5 * np.abs(want_g[t]).max(), t


def check_explicit_replays_reference_fixture(be, golden_dir, name):
    """Explicit-feedback fixtures recorded from the live reference (oracle/make_golden_explicit.py)."""
    from oracle.replay import case_from_rec, _oracle_hparams
    eng = be.engine
    rec = np.load(os.path.join(golden_dir, name + '.npz'))
    case = case_from_rec(rec)
    loss = str(case['loss'])
    dev = be.model([rec['init_%d' % t] for t in range(4)], opt=ORACLE_OPT[str(case['opt'])], **_oracle_hparams(case))
    N, B = int(case['N']), int(case['B'])
    n_mb = (N + B - 1) // B
    losses = []
    for e in range(int(case['n_iter'])):
        d_u = be.alloc(rec['shuffled_users'][e].astype(np.int64))
        d_i = be.alloc(rec['shuffled_items'][e].astype(np.int64))
        d_r = be.alloc(rec['shuffled_ratings'][e].astype(np.float32))
        mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
        eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), be.ptr(d_r), N, B, loss,
                                    be.ptr(mb_loss), stream=be.stream)
        losses.append(be.get(mb_loss))
    losses = np.concatenate(losses)
    assert abs(losses[0] - rec['losses'][0]) / abs(rec['losses'][0]) < 1e-5
    assert np.max(np.abs(losses - rec['losses']) / np.abs(rec['losses'])) < 1e-3
    for t in range(4):  # coarse open-loop drift sanity; the element-wise statement is the closed loop below
        ref = rec['final_%d' % t]
        assert_open_loop_drift(be.get(dev.p[t]), ref, (name, t))
    open_tables = [be.get(dev.p[t]).copy() for t in range(4)]
    # ---- closed loop (see check_replays_reference_fixture)
    opt, hp = ORACLE_OPT[str(case['opt'])], _oracle_hparams(case)
    dev2 = be.model([rec['init_%d' % t] for t in range(4)], opt=opt, **hp)
    step = 0
    for e in range(int(case['n_iter'])):
        su, si = rec['shuffled_users'][e].astype(np.int64), rec['shuffled_items'][e].astype(np.int64)
        sr = rec['shuffled_ratings'][e].astype(np.float32)
        for off in range(0, N, B):
            hi = min(off + B, N)
            pre_p = [be.get(x).copy() for x in dev2.p]
            pre_s1 = [be.get(x).copy() for x in dev2.s1]
            pre_s2 = [be.get(x).copy() for x in dev2.s2]
            ora = BilinearOracle(*pre_p, opt=opt, sparse_grads=True, state1=pre_s1, state2=pre_s2, step=step, **hp)
            want_loss, g = ora.explicit_step(su[off:hi], si[off:hi], sr[off:hi], loss=loss, want_grads=True)
            step += 1
            d_u, d_i, d_r = be.alloc(su[off:hi]), be.alloc(si[off:hi]), be.alloc(sr[off:hi])
            mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
            eng.bilinear_train_explicit(dev2.tables, dev2.optim, be.ptr(d_u), be.ptr(d_i), be.ptr(d_r), hi - off, B, loss,
                                        be.ptr(mb_loss), stream=be.stream)
            assert abs(float(be.get(mb_loss)[0]) - want_loss) <= 1e-5 * abs(want_loss), (e, off)
            assert_step_within_bounds(be, dev2, ora, pre_p, pre_s1, pre_s2, g, step, opt, hp, what='explicit')
    for t in range(4):
        assert np.array_equal(be.get(dev2.p[t]), open_tables[t]), ('closed-loop run differs from the open-loop one', t)


def check_high_row_ids(be, U=(1 << 25) + 3, I=(1 << 21) + 1, D=4, N=4000, B=1024, seed=2):
    """Ids near the top of tables with more than 2^24 (users) / 2^21 (items) rows: the (minibatch, row)
    sort keys, the uint32 narrowing and the row addressing must hold beyond 24 bits.  Rows are zero except
    the touched ones, which the check compares with the oracle run on a compacted copy of the tables."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    hot_u = np.concatenate([np.array([0, 1, U - 1, U - 2, min((1 << 24) + 1, U - 3)]), rs.randint(0, U, 200)])
    hot_i = np.concatenate([np.array([0, I - 1, min((1 << 20) + 7, I - 2)]), rs.randint(0, I, 100)])
    users = rs.choice(hot_u, N).astype(np.int64)
    items = rs.choice(hot_i, N).astype(np.int64)
    negs = rs.choice(hot_i, N).astype(np.int64)
    # compacted problem for the oracle: rank of each id among the ids in use
    uu, ui = np.unique(users), np.unique(np.concatenate([items, negs]))
    pu = rs.normal(0, 0.3, (len(uu), D)).astype(np.float32)
    pi = rs.normal(0, 0.3, (len(ui), D)).astype(np.float32)
    bu, bi = rs.normal(0, 0.1, len(uu)).astype(np.float32), rs.normal(0, 0.1, len(ui)).astype(np.float32)
    ora = BilinearOracle(pu, pi, bu, bi, opt='adagrad', lr=0.05, sparse_grads=True)
    want_loss = ora.train(None, np.searchsorted(uu, users), np.searchsorted(ui, items), B, loss='bpr',
                          neg_in=np.searchsorted(ui, negs))
    full = [np.zeros((U, D), np.float32), np.zeros((I, D), np.float32), np.zeros(U, np.float32), np.zeros(I, np.float32)]
    full[0][uu], full[1][ui], full[2][uu], full[3][ui] = pu, pi, bu, bi
    dev = be.model(full, opt='adagrad', lr=0.05)
    del full
    n_mb = (N + B - 1) // B
    mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
    d_users, d_items, d_negs = be.alloc(users), be.alloc(items), be.alloc(negs)
    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1, be.ptr(mb_loss),
                       d_neg_in=be.ptr(d_negs), stream=be.stream)
    assert np.abs(be.get(mb_loss) - want_loss).max() / np.abs(want_loss).max() < 1e-5
    got = [be.get(t) for t in dev.p]
    assert_close_table(got[0][uu], ora.p[0], 2e-5, 'user rows')
    assert_close_table(got[1][ui], ora.p[1], 2e-5, 'item rows')
    assert_close_table(got[2][uu], ora.p[2], 2e-5, 'user bias')
    assert_close_table(got[3][ui], ora.p[3], 2e-5, 'item bias')
    untouched = np.ones(U, dtype=bool)
    untouched[uu] = False
    assert not got[0][untouched].any() and not got[2][untouched].any()
    # predict for the top user row
    out = be.alloc(np.empty(len(ui), dtype=np.float32))
    d_u, d_it = be.alloc(np.array([U - 1], dtype=np.int64)), be.alloc(ui.astype(np.int64))
    eng.bilinear_predict(dev.tables, be.ptr(d_u), 1, be.ptr(d_it), len(ui), be.ptr(out), be.stream)
    k = int(np.searchsorted(uu, U - 1))
    ref = (ora.p[0][k] * ora.p[1]).sum(1) + ora.p[2][k] + ora.p[3]
    assert rel_inf(be.get(out), ref) < 1e-5


# ---------------------------------------------------------------------------------------
# Interactions.to_sequence on the device (slk_to_sequence_plan / slk_to_sequence_fill)
# ---------------------------------------------------------------------------------------
def to_sequence_case(rs, n, num_users, num_items, ts_mode):
    """Synthetic interactions with duplicate timestamps (stability matters) in the flavour `ts_mode`."""
    from spotlight_amd.interactions import Interactions
    users = rs.randint(0, num_users, n).astype(np.int32)
    items = rs.randint(1, num_items, n).astype(np.int32)
    if ts_mode == 'int32':
        ts = rs.randint(0, max(n // 3, 2), n).astype(np.int32)
    elif ts_mode == 'int64_wide':      # range needs more than 32 bits: the 64-bit key sort
        ts = rs.randint(0, 50, n).astype(np.int64) * (1 << 37) - (1 << 40)
    elif ts_mode == 'negative':
        ts = rs.randint(-1000, 1000, n).astype(np.int64)
    elif ts_mode == 'float':
        ts = rs.randint(-40, 40, n).astype(np.float64) / 8.0
        ts[rs.rand(n) < 0.05] = -0.0
        ts[rs.rand(n) < 0.05] = np.inf
    elif ts_mode == 'float32':
        ts = (rs.randint(0, 200, n) * 0.25).astype(np.float32)
    elif ts_mode == 'constant':
        ts = np.full(n, 7, dtype=np.int64)
    else:
        raise ValueError(ts_mode)
    return Interactions(users, items, timestamps=ts, num_users=num_users, num_items=num_items)


def device_to_sequence(be, inter, max_sequence_length, min_sequence_length, step_size):
    """The engine calls Interactions._to_sequence_device makes, through the backend `be`."""
    eng = be.engine
    L = max_sequence_length
    step = L if step_size is None else step_size
    if min_sequence_length is None:
        thr = 1
    else:
        thr = min_sequence_length if min_sequence_length > 0 else L + min_sequence_length
    ts = inter.timestamps
    kind = 0 if ts.dtype.kind in 'iu' else 1
    ts = ts.astype(np.int64 if kind == 0 else np.float64)
    d_u, d_i, d_t = be.alloc(inter.user_ids.astype(np.int64)), be.alloc(inter.item_ids.astype(np.int64)), be.alloc(ts)
    rows = eng.to_sequence_plan(be.ptr(d_u), be.ptr(d_i), be.ptr(d_t), kind, len(inter), inter.num_users, L, step, thr,
                                stream=be.stream)
    d_seq = be.alloc(np.full((max(rows, 1), L), -7, dtype=np.int32))
    d_su = be.alloc(np.full(max(rows, 1), -7, dtype=np.int32))
    eng.to_sequence_fill(be.ptr(d_seq), be.ptr(d_su), stream=be.stream)
    return be.get(d_seq)[:rows], be.get(d_su)[:rows]


def check_to_sequence(be, n, num_users, num_items, ts_mode, max_sequence_length, min_sequence_length, step_size, seed=0):
    """Device to_sequence == the host to_sequence (interactions.py:170-266; the host one is pinned to the
    reference's golden vectors in test_host_api.py / test_interactions.py), cell for cell."""
    rs = np.random.RandomState(seed)
    inter = to_sequence_case(rs, n, num_users, num_items, ts_mode)
    want = inter.to_sequence(max_sequence_length, min_sequence_length, step_size)
    seq, seq_users = device_to_sequence(be, inter, max_sequence_length, min_sequence_length, step_size)
    assert seq.shape == want.sequences.shape, (seq.shape, want.sequences.shape)
    assert np.array_equal(seq, want.sequences)
    assert np.array_equal(seq_users, want.user_ids)
    return seq.shape[0]


def vectorized_to_sequence(inter, L, min_len, step):
    """numpy restatement of interactions.py:170-266 without the Python double loop (so that 10^7 interactions
    can be checked); itself checked against the host loop at small sizes (test_emu_engine.py)."""
    step = L if step is None else step
    order = np.lexsort((inter.timestamps, inter.user_ids))
    users, items = inter.user_ids[order], inter.item_ids[order]
    uniq, starts, counts = np.unique(users, return_index=True, return_counts=True)
    per_user = -(-counts // step)
    seg = np.repeat(np.arange(len(uniq)), per_user)
    first = np.concatenate([[0], np.cumsum(per_user)[:-1]])
    w = np.arange(len(seg)) - first[seg]
    end = counts[seg] - w * step
    pos = end[:, None] - L + np.arange(L)[None, :]
    seq = np.where(pos >= 0, items[np.clip(starts[seg][:, None] + pos, 0, len(items) - 1)], 0).astype(np.int32)
    seq_users = uniq[seg].astype(np.int32)
    if min_len is not None:
        keep = seq[:, -min_len] != 0
        seq, seq_users = seq[keep], seq_users[keep]
    return seq, seq_users


def check_to_sequence_large(be, n, num_users, num_items, ts_mode, L, min_len, step, seed=0):
    rs = np.random.RandomState(seed)
    inter = to_sequence_case(rs, n, num_users, num_items, ts_mode)
    want, want_users = vectorized_to_sequence(inter, L, min_len, step)
    seq, seq_users = device_to_sequence(be, inter, L, min_len, step)
    assert seq.shape == want.shape, (seq.shape, want.shape)
    assert np.array_equal(seq, want) and np.array_equal(seq_users, want_users)
    return seq.shape[0]


def check_explicit_routes_agree(be, loss, opt, D, U=37, I=29, N=300, B=64, seed=5, user_bloom=0, item_bloom=0):
    """The fused explicit route (score + loss inside the user pass) and the staged one (score pass, loss kernel,
    then the user pass) form dL/dscore with the same fp32 operations: identical tables and optimizer state; the
    minibatch losses differ only in summation order."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    ratings = _ratings_for(rs, loss, N)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)).astype(np.float32), rs.normal(0, sc, (I, D)).astype(np.float32),
              rs.normal(0, 0.1, U).astype(np.float32), rs.normal(0, 0.1, I).astype(np.float32)]
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    n_mb = (N + B - 1) // B
    d_users, d_items, d_ratings = be.alloc(users), be.alloc(items), be.alloc(ratings)
    runs = []
    try:
        for fused in (1, 0):
            eng.set_option('explicit_fused', fused)
            dev = be.model(params, opt=opt, **hp)
            mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
            for _ in range(2):
                eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), be.ptr(d_ratings), N,
                                            B, loss, be.ptr(mb_loss), stream=be.stream)
            runs.append(([be.get(t).copy() for t in dev.p], [be.get(t).copy() for t in dev.s1], be.get(mb_loss).copy()))
    finally:
        eng.set_option('explicit_fused', 1)
    for t in range(4):
        assert np.array_equal(runs[0][0][t], runs[1][0][t]), ('param', t)
        assert np.array_equal(runs[0][1][t], runs[1][1][t]), ('state', t)
    assert np.allclose(runs[0][2], runs[1][2], rtol=1e-6)


def check_item_long_gate_is_bit_neutral(be, loss, opt, D, U, I, N, B, seed=41, option='item_long_gate', values=(1, 0), default=1, nn=1):
    """The plain item pass (minibatches in which no run wholly covers a tile, chosen per chunk from k_item_long_flags) against
    the partial-writing pass + k_item_stitch for every minibatch: every table and state tensor bit for bit."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    results = []
    for gate in values:  # (any option that must not change results: `option`, its two `values`, its `default`)
        eng.set_option(option, gate)
        eng.set_option('epoch_kernel', 0)  # the launch path under test
        try:
            dev = be.model(params, opt=opt, **hp)
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
            eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn, be.ptr(mb_loss),
                               stream=be.stream)
            results.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
        finally:
            eng.set_option(option, default)
            eng.set_option('epoch_kernel', 1)
    for k, (a, b) in enumerate(zip(*results)):
        if k == 0:  # the minibatch losses: the two forms of the user pass hand positions to row groups differently, so the fp32
            # per-thread loss sums associate differently (the model state below does not depend on them)
            assert np.abs(a - b).max() <= 2e-6 * np.abs(a).max(), (a, b)
            continue
        assert np.array_equal(a, b), ('tensor %d differs between the gated and the ungated passes' % k)


def check_bias_shadow_is_bit_neutral(be, loss, D, U, I, N, B, nn=1, seed=43, options=None):
    """Training inside a bias-shadow scope (slk_bias_shadow_begin / _end: item biases and their Adagrad accumulator interleaved
    in the ctx for the duration) against plain training: losses, every table and state tensor bit for bit, and inside the scope
    the caller's bias tensors are not what is trained on (the scope's end rewrites them).  Two training calls per scope."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    results = []
    saved = {k: eng.get_option(k) for k in (options or {})}
    for shadow in (False, True):
        for k, v in (options or {}).items():
            eng.set_option(k, v)
        try:
            dev = be.model(params, opt='adagrad', lr=0.05)
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            d_ratings = be.alloc(_ratings_for(np.random.RandomState(seed + 2), loss, N)) if loss in EXPLICIT_LOSSES else None
            mb_loss = be.alloc(np.zeros(2 * n_mb, dtype=np.float32))
            with eng.bias_shadow(dev.tables, dev.optim, stream=be.stream, enabled=shadow):
                for rep in range(2):
                    if d_ratings is not None:  # explicit feedback: the same two passes, one pair per interaction
                        eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), be.ptr(d_ratings), N, B,
                                                    loss, be.ptr(mb_loss) + 4 * rep * n_mb, stream=be.stream)
                        continue
                    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn,
                                       be.ptr(mb_loss) + 4 * rep * n_mb, stream=be.stream)
                if shadow:  # the caller's bias tensor is stale inside the scope: still the initial values
                    assert np.array_equal(be.get(dev.p[3]).ravel(), params[3].astype(np.float32).ravel())
            results.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
        finally:
            for k, v in saved.items():
                eng.set_option(k, v)
    for k, (a, b) in enumerate(zip(*results)):
        if k == 0 and B <= 1024:  # the plain run of a small minibatch takes the persistent kernel, the shadowed one the launches:
            # the same tables bit for bit, the fp32 loss sums associate differently
            assert np.abs(a - b).max() <= 2e-6 * np.abs(a).max(), (a, b)
            continue
        assert np.array_equal(a, b), ('tensor %d differs between shadowed and plain item biases' % k)
    assert not np.array_equal(results[0][4].ravel(), params[3].astype(np.float32).ravel())  # (the biases did train)


def check_user_pingpong_is_bit_neutral(be, loss, opt, D, U, I, N, B, seed=53, options=None, with_bias_shadow=False, calls=2, sanity=True,
                                       hp=None, step0=0):
    """Training inside a user-row ping-pong scope (slk_user_pingpong_begin / _end: the user table doubled in the ctx, the user
    pass writes updated rows to the other copy and no record, the item pass gathers pre-step rows where they still stand)
    against plain training: losses, every table and state tensor bit for bit.  Inside the scope the caller's user table is a MIX
    of rows (some current rows live in the ctx's copy); the scope's end makes it whole.  `calls` training calls per scope: a
    user's current copy alternates with every minibatch that touches it.  `sanity=False` (the fuzz: one-item tables, single
    interactions): the "something did train" asserts are skipped, the bit-for-bit ones are not.
    `hp`: the optimizer's hyper-parameters in place of lr = 0.05 and defaults; `step0`: steps already taken."""
    hp = dict(lr=0.05) if hp is None else hp
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    results = []
    saved = {k: eng.get_option(k) for k in (options or {})}
    for pingpong in (False, True):
        for k, v in (options or {}).items():
            eng.set_option(k, v)
        try:
            dev = be.model(params, opt=opt, **hp)
            dev.optim.step = step0
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros(calls * n_mb, dtype=np.float32))
            n0 = eng.get_stat('pingpong_calls')
            with eng.bias_shadow(dev.tables, dev.optim, stream=be.stream, enabled=with_bias_shadow):
                with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream, enabled=pingpong):
                    for rep in range(calls):
                        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, 1,
                                           be.ptr(mb_loss) + 4 * rep * n_mb, stream=be.stream)
                    if pingpong:
                        assert eng.get_stat('pingpong_calls') == n0 + calls, 'a call of the scope did not run on the two copies'
                        mixed = be.get(dev.p[0]).copy()
            assert dev.optim.step == step0 + calls * n_mb
            results.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
        finally:
            for k, v in saved.items():
                eng.set_option(k, v)
    for k, (a, b) in list(enumerate(zip(*results)))[1:]:
        assert np.array_equal(a, b), ('tensor %d differs between ping-ponged and plain user rows' % k)
    # the minibatch losses: the scope's user pass is another kernel (its own occupancy, hence its own grid: the fp32 per-thread
    # loss sums associate differently -- a hot user's thousand terms by 2-3e-6; small minibatches take the persistent kernel
    # outside the scope): the path's 1e-5 loss tolerance
    assert np.abs(results[0][0] - results[1][0]).max() <= 1e-5 * np.abs(results[0][0]).max(), (results[0][0], results[1][0])
    # inside the scope the caller's array holds the current row of exactly the users that were updated an EVEN number of times
    # (a user's current copy alternates with every minibatch that touches it); the others' current rows were in the ctx's copy
    times = np.zeros(U, dtype=np.int64)
    for m in range(n_mb):
        times[np.unique(users[m * B:(m + 1) * B])] += calls
    home = times % 2 == 0
    assert np.array_equal(mixed[home], results[1][1][home]), 'a user updated an even number of times is not at home in the caller\'s table'
    if sanity and (~home).any():
        assert not np.array_equal(mixed[~home], results[1][1][~home])
    if sanity:
        assert not np.array_equal(results[0][1], params[0].astype(np.float32))  # (the user rows did train)


def check_prefetch_before_pingpong_begin(be, loss, D=8, U=60, I=2000, N=700, B=128, seed=71):
    """A first chunk prepared ahead (slk_bilinear_prefetch) BEFORE slk_user_pingpong_begin was sorted without the single-occurrence
    flags that the training call inside the scope reads (option "item_single_min_items"): the call that adopts it makes them
    itself.  Both orders -- prefetch, then the scope; the scope, then the prefetch -- against plain training (no scope, nothing
    prepared ahead): every table and its first state tensor bit for bit, the chunk was adopted, the fast path did run.  Three
    chunks of two minibatches."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    options = dict(chunk_interactions=256, overlap_prep=1, overlap_min_batch=0, epoch_kernel=0, item_single_min_items=1, user_lat_max_batch=0)
    saved = {k: eng.get_option(k) for k in options}
    results = {}
    for k, v in options.items():
        eng.set_option(k, v)
    try:
        for order in ('plain', 'prefetch_then_scope', 'scope_then_prefetch'):
            dev = be.model(params, opt='adagrad', lr=0.05)
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
            eng.rng_set_state(state)
            prefetched, single = eng.get_stat('prefetched_chunks'), eng.get_stat('single_minibatches')

            def prefetch():
                eng.bilinear_prefetch(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, 1, stream=be.stream)
                assert eng.get_stat('prefetch_pending') > 0

            if order == 'prefetch_then_scope':
                prefetch()
            with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream, enabled=order != 'plain'):
                if order == 'scope_then_prefetch':
                    prefetch()
                eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, 1, be.ptr(mb_loss), stream=be.stream)
            if order != 'plain':
                assert eng.get_stat('prefetched_chunks') == prefetched + 1, order
                assert eng.get_stat('single_minibatches') > single, order  # (every one of the 6 minibatches at the default shape)
            results[order] = [be.get(x).copy() for x in dev.p + dev.s1]
    finally:
        for k, v in saved.items():
            eng.set_option(k, v)
    for order in ('prefetch_then_scope', 'scope_then_prefetch'):
        for t, (a, b) in enumerate(zip(results[order], results['plain'])):
            assert np.array_equal(a, b), ('tensor %d of %s differs from plain training' % (t, order))


def check_user_pingpong_contract(be):
    """include/spotlight_hip.h, slk_user_pingpong_begin: what the scope covers and refuses, and its lifetime rules -- one scope per
    ctx, plain tables + row-sparse optimizers; calls that would read the caller's (mixed) user table are refused inside it; so
    are adaptive hinge, explicit feedback and another model's tables; _end makes the table whole, _abort does not."""
    import pytest
    from spotlight_amd import _native
    rs = np.random.RandomState(5)
    U, I, D, N, B = 40, 30, 8, 600, 128
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    d_u, d_i = be.alloc(users), be.alloc(items)
    nmb = (N + B - 1) // B
    loss = be.alloc(np.zeros(nmb, dtype=np.float32))
    eng = be.engine

    def train(dev, kind='bpr', nn=1):
        eng.rng_set_state(np.random.RandomState(9).get_state())
        eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), N, B, kind, nn, be.ptr(loss), stream=be.stream)

    dense = be.model(params, opt='adam_dense', lr=0.05)
    with pytest.raises(_native.SlkError, match='row-sparse'):
        with eng.user_pingpong(dense.tables, dense.optim, stream=be.stream):
            pass
    dev = be.model(params, opt='adagrad', lr=0.05)
    other = be.model(params, opt='adagrad', lr=0.05)
    ref = be.model(params, opt='adagrad', lr=0.05)
    train(ref)
    want = be.get(ref.p[0]).copy()
    out, one = be.alloc(np.empty(I, dtype=np.float32)), be.alloc(np.array([3], dtype=np.int64))
    with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream):
        with pytest.raises(_native.SlkError, match='already active'):  # one scope per ctx
            with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream):
                pass
        train(dev)
        # the caller's user table is a mix of rows inside the scope: a call that would read it is refused, not answered
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            eng.bilinear_predict(dev.tables, be.ptr(one), 1, None, I, be.ptr(out), be.stream)
        # losses the scope does not cover, on ITS tables: refused (the scope belongs to this model's pair-loss training)
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            train(dev, 'adaptive_hinge', 3)
        ratings = be.alloc(np.ones(N, dtype=np.float32))
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_u), be.ptr(d_i), be.ptr(ratings), N, B, 'regression',
                                        be.ptr(loss), stream=be.stream)
        with pytest.raises(_native.SlkError, match='OTHER'):  # another model's tables while the scope is open
            train(other)
        eng.bilinear_reserve(other.tables, other.optim, N, B, 'bpr', 1, stream=be.stream)  # (allocating is not training)
        assert not np.array_equal(be.get(dev.p[0]), want)  # some current rows are in the ctx's copy
    assert np.array_equal(be.get(dev.p[0]), want)  # _end made the table whole: the plain run's table bit for bit
    eng.bilinear_predict(dev.tables, be.ptr(one), 1, None, I, be.ptr(out), be.stream)  # (and answered again outside it)
    assert np.isfinite(be.get(out)).all()
    train(other)  # the ctx is free again
    # _abort: the scope closes, nothing is copied back
    scope = eng.user_pingpong(dev.tables, dev.optim, stream=be.stream)
    scope.__enter__()
    train(dev)
    mixed = be.get(dev.p[0]).copy()
    scope.abort()
    assert np.array_equal(be.get(dev.p[0]), mixed)
    with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream):  # and a new scope can open
        pass
    scope.__exit__(None, None, None)  # (a closed scope's exit is a no-op)


# ---------------------------------------------------------------------------------------
# persistent epoch kernel (csrc/slk_epoch.hip) against the per-minibatch launches
# ---------------------------------------------------------------------------------------
def check_epoch_kernel_is_bit_identical(be, loss, opt, D, U=300, I=170, N=2500, B=256, seed=31, chunk=None, epochs=2,
                                        max_grid=None, barrier=-1, cooperative=0, nn=None, hp=None, step0=0):
    """The persistent route (option epoch_kernel = 1: every minibatch of a chunk in one cooperative launch) performs the
    launch path's arithmetic in the launch path's order: losses to fp32 summation-order noise, negatives, RNG state and
    EVERY table / optimizer-state tensor bit for bit -- including the dense optimizers, whose full-table sweep the
    persistent route folds into the gaps between the owned rows.
    `hp`: the optimizer's hyper-parameters in place of lr = 0.05 (dense kinds: weight_decay = 1e-3) and defaults; `step0`: steps
    already taken (with lr_decay, or bias corrections that have not converged, every minibatch of a chunk has its own
    coefficients: the persistent kernel's table hc[m])."""
    eng = be.engine
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, N).astype(np.int64)
    items = rs.randint(0, I, N).astype(np.int64)
    sc = min(0.3, 1.0 / np.sqrt(D))
    params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    if hp is None:
        hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
    state = np.random.RandomState(seed + 1).get_state()
    n_mb = (N + B - 1) // B
    # explicit feedback (ExplicitFactorizationModel.fit, factorization/explicit.py:213-236): one pair per interaction,
    # the loss against a rating, no negatives
    explicit = loss in ('regression', 'poisson', 'logistic')
    ratings = _ratings_for(rs, loss, N) if explicit else None
    # adaptive hinge (implicit.py:266-275): nn draws per interaction, the persistent route's score phase + in-phase selection
    nn = (nn or 5) if loss == 'adaptive_hinge' else 1
    results = []
    for route in (0, 1):
        eng.set_option('epoch_kernel', route)
        eng.set_option('epoch_max_batch', 1 << 20)      # the persistent route for every size / optimizer under test,
        eng.set_option('epoch_adaptive_max_batch', 1 << 20)
        eng.set_option('epoch_dense_elems', 1 << 40)     # not only where it is the default
        if chunk:
            eng.set_option('chunk_interactions', chunk)
        if max_grid:
            eng.set_option('epoch_max_grid', max_grid)
        eng.set_option('epoch_barrier', barrier)
        eng.set_option('epoch_cooperative', cooperative)
        try:
            dev = be.model(params, opt=opt, **hp)
            dev.optim.step = step0
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            d_ratings = be.alloc(ratings) if explicit else None
            losses = []
            neg_out = be.alloc(np.full(N * nn, -1, dtype=np.int64))
            eng.profile_reset()
            eng.profile_enable(True)
            for _ in range(epochs):
                mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
                if explicit:
                    eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), be.ptr(d_ratings), N,
                                                B, loss, be.ptr(mb_loss), stream=be.stream)
                else:
                    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn,
                                       be.ptr(mb_loss), d_neg_out=be.ptr(neg_out), stream=be.stream)
                losses.append(be.get(mb_loss).copy())
            eng.profile_enable(False)
            prof = eng.profile_read()
            # the route under test really ran: the persistent kernel or the two passes, never both
            if route:
                assert prof['epoch'][0] >= epochs and prof['user_pass'][0] == 0, prof
            else:
                assert prof['epoch'][0] == 0 and prof['user_pass'][0] == epochs * n_mb, prof
            st = eng.rng_get_state()
            assert dev.optim.step == step0 + epochs * n_mb
            results.append((np.concatenate(losses), [be.get(neg_out), st[1], np.array(st[2])] +
                            [be.get(x) for x in dev.p + dev.s1 + dev.s2]))
        finally:
            eng.set_option('epoch_kernel', 1)
            eng.set_option('epoch_max_batch', 1024)
            eng.set_option('epoch_adaptive_max_batch', 1024)
            eng.set_option('epoch_dense_elems', 1 << 18)
            eng.set_option('chunk_interactions', 1 << 23)
            eng.set_option('epoch_max_grid', 256)
            eng.set_option('epoch_barrier', -1)
            eng.set_option('epoch_cooperative', 0)
    (la, ta), (lb, tb) = results
    assert np.abs(la - lb).max() <= 2e-6 * np.abs(la).max(), (la, lb)
    for k, (a, b) in enumerate(zip(ta, tb)):
        assert np.array_equal(a, b), ('tensor %d differs between the persistent kernel and the launch path' % k,
                                      float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))



def f32_chain_dot(a, b):
    """The package's score dot product in numpy: acc = fmaf(a_d, b_d, acc) over d ascending, in float32 (an fma = the
    exactly rounded float64 product-sum of float32 operands: 24 + 24-bit products and a 24-bit addend fit a double)."""
    acc = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, np.float32)
    for d in range(a.shape[-1]):
        acc = (a[..., d].astype(np.float64) * b[..., d].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def check_scores_are_the_fma_chain(be, D, U=70, I=700, seed=3):
    """predict(user) over EVERY item (the matrix-core sweep, csrc/slk_eval.hip), predict over explicit pairs (the vector-unit
    chain) and the numpy chain give the same bits; the batched score rows too."""
    rng = np.random.RandomState(seed)
    params = [rng.randn(U, D).astype(np.float32), rng.randn(I, D).astype(np.float32), rng.randn(U).astype(np.float32),
              rng.randn(I).astype(np.float32)]
    dev = be.model(params)
    eng = be.engine
    users = np.array([0, U - 1, U // 2], dtype=np.int64)
    want = {int(u): ((f32_chain_dot(params[0][u][None, :], params[1]) + params[2][u]) + params[3]).astype(np.float32) for u in users}
    for u in users:
        out = be.alloc(np.empty(I, dtype=np.float32))
        d_u = be.alloc(np.array([u], dtype=np.int64))
        eng.bilinear_predict(dev.tables, be.ptr(d_u), 1, None, I, be.ptr(out), be.stream)
        got_all = be.get(out).copy()
        d_pu, d_pi = be.alloc(np.full(I, u, dtype=np.int64)), be.alloc(np.arange(I, dtype=np.int64))
        eng.bilinear_predict(dev.tables, be.ptr(d_pu), I, be.ptr(d_pi), I, be.ptr(out), be.stream)
        got_pairs = be.get(out).copy()
        assert np.array_equal(got_all, got_pairs), (D, int(u), np.abs(got_all - got_pairs).max())
        assert np.array_equal(got_all, want[int(u)]), (D, int(u), np.abs(got_all - want[int(u)]).max())
    rows = be.alloc(np.empty((len(users), I), dtype=np.float32))
    d_users = be.alloc(users)
    eng.bilinear_scores(dev.tables, be.ptr(d_users), len(users), be.ptr(rows), be.stream)
    for r, u in enumerate(users):
        assert np.array_equal(be.get(rows)[r], want[int(u)])
    # every row count's kernel: the streaming form for a handful of rows (1, 2, <= 4, <= 8), one and two matrix-core tiles above
    for n_rows in (2, 5, 8, 9, 40):
        batch = rng.randint(0, U, n_rows).astype(np.int64)
        rows = be.alloc(np.full((n_rows, I), np.nan, dtype=np.float32))
        d_batch = be.alloc(batch)
        eng.bilinear_scores(dev.tables, be.ptr(d_batch), n_rows, be.ptr(rows), be.stream)
        got = be.get(rows)
        for r, u in enumerate(batch):
            w = ((f32_chain_dot(params[0][u][None, :], params[1]) + params[2][u]) + params[3]).astype(np.float32)
            assert np.array_equal(got[r], w), (D, n_rows, r)


def check_fused_ranks(be, D=24, U=90, I=333, n_rows=150, seed=5, ties=True):
    """slk_bilinear_rank against scipy-style average ranks of the chain scores: targets on and off their group's exclusion
    list, exact ties (duplicated item rows), groups without exclusions, several rows per group."""
    rng = np.random.RandomState(seed)
    V = rng.randn(I, D).astype(np.float32)
    bi = rng.randn(I).astype(np.float32)
    if ties:
        V[5] = V[6] = V[7]
        bi[5] = bi[6] = bi[7]
    params = [rng.randn(U, D).astype(np.float32), V, rng.randn(U).astype(np.float32), bi]
    dev = be.model(params)
    groups = rng.choice(U, size=40, replace=False).astype(np.int64)
    row_group = np.sort(rng.randint(0, len(groups), n_rows)).astype(np.int64)
    row_target = rng.randint(0, I, n_rows).astype(np.int64)
    row_target[:6] = [5, 6, 7, 5, 6, 7]
    exc = [np.unique(rng.randint(0, I, rng.randint(0, 30))) if g % 3 else np.zeros(0, np.int64) for g in range(len(groups))]
    for r in range(0, n_rows, 7):  # some targets are excluded themselves
        g = row_group[r]
        if len(exc[g]):
            exc[g] = np.unique(np.append(exc[g], row_target[r]))
    exc_off = np.concatenate([[0], np.cumsum([len(x) for x in exc])]).astype(np.int64)
    exc_items = np.concatenate(exc).astype(np.int64)
    ranks = be.alloc(np.zeros(n_rows, dtype=np.float64))
    d_g, d_rg, d_rt, d_eo, d_ei = be.alloc(groups), be.alloc(row_group), be.alloc(row_target), be.alloc(exc_off), be.alloc(exc_items)
    be.engine.bilinear_rank(dev.tables, be.ptr(d_g), len(groups), be.ptr(d_rg), be.ptr(d_rt), n_rows, be.ptr(d_eo), be.ptr(d_ei),
                            be.ptr(ranks), be.stream)
    got = be.get(ranks)
    for r in range(n_rows):
        u = groups[row_group[r]]
        s = ((f32_chain_dot(params[0][u][None, :], V) + params[2][u]) + bi).astype(np.float32)
        s[exc[row_group[r]]] = -np.finfo(np.float32).max
        t = s[row_target[r]]
        want = float((s > t).sum()) + (float((s == t).sum()) + 1.0) * 0.5
        assert got[r] == want, (r, got[r], want)
    # no exclusion lists at all
    be.engine.bilinear_rank(dev.tables, be.ptr(d_g), len(groups), be.ptr(d_rg), be.ptr(d_rt), n_rows, None, None, be.ptr(ranks), be.stream)
    got = be.get(ranks)
    for r in range(0, n_rows, 5):
        u = groups[row_group[r]]
        s = ((f32_chain_dot(params[0][u][None, :], V) + params[2][u]) + bi).astype(np.float32)
        t = s[row_target[r]]
        assert got[r] == float((s > t).sum()) + (float((s == t).sum()) + 1.0) * 0.5


def check_bias_shadow_refusals(be):
    """slk_bias_shadow_begin covers the fused row-sparse Adagrad, one scope per ctx; a call that would read the stale bias array
    inside the scope is refused."""
    import pytest
    from spotlight_amd import _native
    rs = np.random.RandomState(3)
    params = [rs.normal(0, 0.1, (30, 8)), rs.normal(0, 0.1, (20, 8)), np.zeros(30), np.zeros(20)]
    dev = be.model(params, opt='sparse_adam', lr=0.05)
    with pytest.raises(_native.SlkError):
        with be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream):
            pass
    dev = be.model(params, opt='adagrad', lr=0.05)
    with be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream):
        with pytest.raises(_native.SlkError):  # one scope per ctx
            with be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream):
                pass
        # the caller's bias array is stale inside the scope: a call that would read it is refused, not answered
        out, d_u = be.alloc(np.empty(20, dtype=np.float32)), be.alloc(np.array([3], dtype=np.int64))
        with pytest.raises(_native.SlkError, match='shadowed'):
            be.engine.bilinear_predict(dev.tables, be.ptr(d_u), 1, None, 20, be.ptr(out), be.stream)
    be.engine.bilinear_predict(dev.tables, be.ptr(d_u), 1, None, 20, be.ptr(out), be.stream)  # (and answered again outside it)
    assert np.isfinite(be.get(out)).all()


def check_bias_shadow_lifetime_contract(be):
    """include/spotlight_hip.h, LIFETIME CONTRACT (ABI 11): inside a scope the ctx holds the caller's bias / accumulator pointers.
    A training call that names the shadowed biases with ANOTHER optimizer-state tensor (swapped inside the scope), or that names
    other tables altogether, is refused; _end closes the scope and writes back; _abort closes it without writing."""
    import pytest
    from spotlight_amd import _native
    rs = np.random.RandomState(5)
    U, I, D, N, B = 40, 30, 8, 600, 128
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    d_u, d_i = be.alloc(users), be.alloc(items)
    nmb = (N + B - 1) // B
    loss = be.alloc(np.zeros(nmb, dtype=np.float32))

    def train(dev, optim=None):
        be.engine.rng_set_state(np.random.RandomState(9).get_state())
        be.engine.bilinear_train(dev.tables, optim if optim is not None else dev.optim, be.ptr(d_u), be.ptr(d_i), N, B, 'bpr', 1,
                                 be.ptr(loss), stream=be.stream)

    dev = be.model(params, opt='adagrad', lr=0.05)
    other = be.model(params, opt='adagrad', lr=0.05)
    bias0 = be.get(dev.p[3]).copy()
    scope = be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream)
    with scope:
        train(dev)  # the scope's own model trains
        # (1) the optimizer state tensor swapped inside the scope (nothing freed): refused, loudly
        swapped_state = be.alloc(np.zeros(I, dtype=np.float32))
        s1 = [dev.optim.d_state1[k] for k in range(4)]
        s1[3] = be.ptr(swapped_state)
        swapped = _native.make_optim('adagrad', s1, lr=0.05)
        with pytest.raises(_native.SlkError, match='another optimizer state'):
            train(dev, swapped)
        # (2) another model's tables while the scope is open: refused
        with pytest.raises(_native.SlkError, match='OTHER'):
            train(other)
        # ... but allocating its scratch is not training
        be.engine.bilinear_reserve(other.tables, other.optim, N, B, 'bpr', 1, stream=be.stream)
        assert np.array_equal(be.get(dev.p[3]), bias0)  # the caller's array is still the stale pre-scope one
    trained = be.get(dev.p[3]).copy()
    assert not np.array_equal(trained, bias0)  # _end wrote the scope's training back
    train(other)  # the ctx is free again
    # (3) _abort: the scope closes, nothing is written
    scope = be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream)
    scope.__enter__()
    train(dev)
    scope.abort()
    assert np.array_equal(be.get(dev.p[3]), trained)
    with be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream):  # and a new scope can open
        pass
    scope.__exit__(None, None, None)  # (a closed scope's exit is a no-op)


# ---------------------------------------------------------------------------------------
# every engine option is result-neutral (include/spotlight_hip.h: slk_ctx_set_option "tuning knobs that never change results")
# ---------------------------------------------------------------------------------------
# option -> values to try against the defaults.  Two debug switches are measurement modes whose results are declared meaningless
# (sort_debug, epoch_debug) and are excluded by name.
OPTION_VALUES = {
    'chunk_interactions': (300, 2048), 'overlap_prep': (1, 2), 'overlap_min_batch': (0,), 'prefetch_wait': (1,),
    'mt_long_min_blocks': (2, 40), 'sort_big_min': (1, 1 << 40), 'item_grid_mult': (1, 64), 'user_grid_mult': (1, 3, 64),
    'seq_variant': (0, 1), 'explicit_fused': (0,), 'epoch_kernel': (0,), 'item_lat_max_tiles': (0, 1 << 30),
    'epoch_adaptive': (0,), 'epoch_adaptive_max_batch': (1, 1 << 20), 'epoch_max_batch': (1, 1 << 20), 'epoch_max_grid': (1, 3, 64),
    'epoch_barrier': (0, 1), 'epoch_cooperative': (1,), 'epoch_dense_elems': (0, 1 << 40), 'user_lat_max_batch': (0, 1 << 30),
    'item_long_gate': (0,), 'shuffle_band': (0, 64), 'nt': (1, 6, 15, 48, 63), 'record_nt_min_bytes': (0, 1), 'user_bias_zero_hint': (0,),
    'user_grid_own_occ': (1,), 'item_single_min_items': (0, 1),
}
OPTIONS_NOT_RESULT_NEUTRAL = ('sort_debug', 'epoch_debug')
# adaptive hinge's item side in its two forms (all 1 + n occurrences sorted per chunk / the live ones re-sorted per minibatch): the
# same sums in a different order -- neutral to fp32 rounding, not bit for bit (include/spotlight_hip.h says so); one minibatch, so
# that nothing amplifies the 1-ulp differences
OPTIONS_NEUTRAL_TO_SUMMATION_ORDER = {'adaptive_late_min_batch': (0, 1 << 30)}


def option_names_of_the_library():
    """The names in csrc/slk_api.hip's option table (the C ABI has a getter per name, no enumeration)."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'spotlight_amd', 'csrc', 'slk_api.hip')).read()
    return re.findall(r'SLK_OPT\("([a-z_]+)"', src)


def check_option_is_result_neutral(be, name, values):
    """Training under `name` = each of `values` against the defaults, on a launch-path shape (several chunks when the option says so,
    hot items), a persistent-route shape and an adaptive-hinge one: negatives, every table and state tensor bit for bit; the
    minibatch losses to fp32 summation order."""
    eng = be.engine
    shapes = [('bpr', 'adagrad', 16, 400, 30, 6000, 2048, 1), ('pointwise', 'sparse_adam', 8, 300, 170, 2500, 256, 1),
              ('adaptive_hinge', 'adagrad', 8, 120, 90, 1500, 512, 3), ('hinge', 'adam_dense', 8, 60, 50, 700, 256, 1)]
    default = eng.get_option(name)
    for loss, opt, D, U, I, N, B, nn in shapes:
        rs = np.random.RandomState(77)
        users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
        sc = min(0.3, 1.0 / np.sqrt(D))
        params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
        hp = dict(lr=0.05, weight_decay=1e-3 if opt.endswith('dense') else 0.0)
        state = np.random.RandomState(78).get_state()
        n_mb = (N + B - 1) // B
        results = []
        for v in (default,) + tuple(values):
            eng.set_option(name, v)
            try:
                dev = be.model(params, opt=opt, **hp)
                eng.rng_set_state(state)
                d_users, d_items = be.alloc(users), be.alloc(items)
                mb_loss = be.alloc(np.zeros(n_mb, dtype=np.float32))
                neg_out = be.alloc(np.full(N * nn, -1, dtype=np.int64))
                eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, loss, nn, be.ptr(mb_loss),
                                   d_neg_out=be.ptr(neg_out), stream=be.stream)
                st = eng.rng_get_state()
                results.append([be.get(mb_loss)] + [be.get(x) for x in [neg_out] + dev.p + dev.s1 + dev.s2] + [st[1], np.array(st[2])])
            finally:
                eng.set_option(name, default)
        for r in results[1:]:
            assert np.abs(r[0] - results[0][0]).max() <= 2e-6 * np.abs(results[0][0]).max(), (name, loss)
            for k, (a, b) in enumerate(zip(results[0][1:], r[1:])):
                assert np.array_equal(a, b), ('option %s: tensor %d differs (%s, %s)' % (name, k, loss, opt))
    # the other training entry points: bloom layers on both sides, explicit feedback, PoolNet (plain and over a bloom item layer)
    from oracle.oracle import bloom_desc

    def run_all(v):
        out = []
        eng.set_option(name, v)
        try:
            rs = np.random.RandomState(79)
            U, I, D, N, B = 150, 200, 16, 1800, 512
            users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
            params, ud, idesc = _bloom_setup(rs, U, I, D, 2, 4, 0.4)
            dev = be.model(params, opt='adagrad', user_bloom=ud, item_bloom=idesc, lr=0.05)
            eng.rng_set_state(np.random.RandomState(80).get_state())
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros((N + B - 1) // B, dtype=np.float32))
            eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1, be.ptr(mb_loss), stream=be.stream)
            out.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1])
            ratings = _ratings_for(rs, 'regression', N)
            sc = 1.0 / np.sqrt(D)
            params = [rs.normal(0, sc, (U, D)), rs.normal(0, sc, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
            for B2 in (256, 2048):  # the persistent route and the launches
                dev = be.model(params, opt='sparse_adam', lr=0.05)
                mb_loss = be.alloc(np.zeros((N + B2 - 1) // B2, dtype=np.float32))
                d_r = be.alloc(ratings)
                eng.bilinear_train_explicit(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), be.ptr(d_r), N, B2, 'regression',
                                            be.ptr(mb_loss), stream=be.stream)
                out.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
            for bloom in (0, 3):
                NS, L, BS, IS = 90, 20, 32, 400
                seqs = make_sequences(rs, NS, L, IS, 0.3)
                sp = _seq_params(rs, IS, D, rows=int(0.4 * IS) if bloom else None)
                dev = be.seq_model(sp, opt='adagrad', item_bloom=bloom_desc(n_hash=bloom) if bloom else None, lr=0.05)
                eng.rng_set_state(np.random.RandomState(81).get_state())
                d_seqs = be.alloc(seqs)
                mb_loss = be.alloc(np.zeros((NS + BS - 1) // BS, dtype=np.float32))
                eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), NS, L, BS, 'bpr', 1, be.ptr(mb_loss), stream=be.stream)
                st = eng.rng_get_state()
                out.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1] + [st[1], np.array(st[2])])
        finally:
            eng.set_option(name, default)
        return out
    base = run_all(default)
    for v in values:
        for j, (ra, rb) in enumerate(zip(base, run_all(v))):
            assert np.abs(ra[0] - rb[0]).max() <= 2e-6 * np.abs(ra[0]).max(), (name, j)
            for k, (a, b) in enumerate(zip(ra[1:], rb[1:])):
                assert np.array_equal(a, b), ('option %s = %r: run %d, tensor %d differs' % (name, v, j, k))


def check_option_is_neutral_to_summation_order(be, name, values, tol=2e-6):
    """ONE adaptive-hinge minibatch on the launch path under `name` = each of `values`: the same negatives, every table within
    `tol` of its largest element (a different association of the same fp32 sums), Adagrad from a non-zero accumulator."""
    eng = be.engine
    default = eng.get_option(name)
    loss, opt, D, U, I, B, nn = 'adaptive_hinge', 'adagrad', 8, 120, 90, 512, 3
    rs = np.random.RandomState(77)
    users, items = rs.randint(0, U, B).astype(np.int64), rs.randint(0, I, B).astype(np.int64)
    params = [rs.normal(0, 0.3, (U, D)), rs.normal(0, 0.3, (I, D)), rs.normal(0, 0.1, U), rs.normal(0, 0.1, I)]
    state = np.random.RandomState(78).get_state()
    results = []
    with eng.options(epoch_kernel=0):
        for v in values:
            eng.set_option(name, v)
            try:
                dev = be.model(params, opt=opt, lr=0.05)
                eng.rng_set_state(state)
                d_users, d_items = be.alloc(users), be.alloc(items)
                mb_loss, neg_out = be.alloc(np.zeros(1, dtype=np.float32)), be.alloc(np.full(B * nn, -1, dtype=np.int64))
                eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), B, B, loss, nn, be.ptr(mb_loss),
                                   d_neg_out=be.ptr(neg_out), stream=be.stream)
                results.append([be.get(neg_out)] + [be.get(x) for x in [mb_loss] + dev.p + dev.s1])
            finally:
                eng.set_option(name, default)
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0])
        for a, b in zip(results[0][1:], r[1:]):
            assert np.abs(a - b).max() <= tol * max(np.abs(a).max(), 1e-30), name

