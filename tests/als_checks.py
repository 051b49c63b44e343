"""Shared checks of slk_als_gram / slk_als_solve / slk_als_loss (include/spotlight_hip.h: implicit-feedback ALS), run on the
emulator build (tests/test_emu_als.py) and on the gfx950 library (tests/test_gpu_als.py), and of ALSFactorizationModel
(spotlight_amd/factorization/als.py) on the GPU.

The reference is a float64 numpy restatement of the half-step, of the objective L and of a whole fit() (half_step / objective
/ fit below with dtype=np.float64).  The YARDSTICK of every tolerance is the same restatement in float32 (numpy float32
accumulation, LAPACK's float32 Cholesky solve): its worst per-row relative error against the float64 result is measured on
the test's own inputs, every time the test runs, and the kernel passes at FACTOR times that figure.  Both are backward-stable
factorizations of the same systems at the same unit round-off; they differ in summation order and blocking only, which a
small constant covers.  Everything else is a bit-for-bit statement of the engine against itself.

Every half-step check runs under "als_wg_min_len" = 0 (the default crossover, 32: both routes in a call), 1 (every non-empty row on the workgroup route) and 2^40 (every row on the light route)."""
import numpy as np
import pytest
import scipy.linalg

from spotlight_amd import _native

DS = (6, 24, 64, 72, 128)
TABLES = (7, 333, 2000)        # rows of the fixed table; 2000: several workgroups of the Gram kernel, each with several chunks, 8 partial tiles
ROUTES = (0, 1, 1 << 40)       # "als_wg_min_len": default, all-workgroup, all-light
WG_DEFAULT = 32                # SLK_ALS_WG_MIN_LEN (csrc/slk_als.hip)
LONG = 600                     # a history on the workgroup route at the default crossover (as are D - 1, D, D + 1 and 300 from dim 64 on)
LAMBDA = np.float32(0.5)
SENTINEL = np.float32(-7.25)

# The tolerance of every comparison with float64: FACTOR x the float32 restatement's own worst error on the same inputs.
FACTOR = 4.0
# What the yardstick measured here (worst per-row relative error |x32 - x64| / |x64| of the float32 restatement; recorded for the
# reader, the tests measure it again on every run):
#   half-step, Problem(D, I), fixed tables of 333 and 2000 rows ... 5.4e-7 (D 24, I 2000) .. 7.3e-6 (D 128, I 333); the kernel's
#                                                                   own worst row: 6.1e-7 .. 6.4e-6, at most 1.6 x the yardstick's
#   half-step, fixed tables of 7 rows (G has rank 7: the systems'
#   smallest eigenvalue is lambda itself) ........................... 2.2e-6 (D 6) .. 4.2e-3 (D 128); the kernel 2.0e-6 .. 3.9e-3
#   objective L, loss_problem(24) / (72) ............................ 1.8e-8 / 8.8e-8 relative, so the floor of 2^-22 decides (the
#                                                                   kernel accumulates in float64: 9e-10 / 1.5e-9)
#   fit(n_iter=3) on datasets/synthetic.py's default shape, dim 32 . user rows 1.9e-6, item rows 2.1e-6 (the kernel 2.0e-6 and
#                                                                   2.4e-6); L: 1.2e-3 absolute of 1.4e4 .. 1.8e4
# (DESIGN.md 4b "ALS" quotes the same figures)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def merge_duplicates(rows, cols, r, n_rows):
    """CSR (off, cols, r) of the (row, col, r) triples with duplicate pairs merged into one entry whose r is the sum; columns
    ascending within a row."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    span = int(cols.max()) + 1 if cols.size else 1
    key, inv = np.unique(rows * span + cols, return_inverse=True)
    summed = np.zeros(len(key), np.float64)
    np.add.at(summed, inv, np.asarray(r, np.float64))
    off = np.searchsorted(key // span, np.arange(n_rows + 1)).astype(np.int64)
    return off, (key % span).astype(np.int64), summed


def gram(Y, dtype):
    Y = Y.astype(dtype)
    return Y.T @ Y


def system(Y, G, lam, cols, w, dtype):
    """(A, b) of one row in `dtype`: A = G + lam I + sum w y y^T, b = sum (w + 1) y."""
    Yr = Y[cols].astype(dtype)
    w = w.astype(dtype)
    A = G.astype(dtype) + dtype(lam) * np.eye(Y.shape[1], dtype=dtype) + (Yr * w[:, None]).T @ Yr
    b = ((w + dtype(1))[:, None] * Yr).sum(axis=0, dtype=dtype)
    return A, b


def half_step(Y, G, lam, off, cols, w, dtype, rows=None):
    """(X [len(off) - 1, D] in `dtype`, number of rows whose system is not positive definite in `dtype`): the half-step of
    include/spotlight_hip.h by Cholesky.  A failed row is NaN."""
    n, D = len(off) - 1, Y.shape[1]
    X = np.zeros((n, D), dtype)
    failed = 0
    for u in (range(n) if rows is None else rows):
        o0, o1 = int(off[u]), int(off[u + 1])
        if o0 == o1:
            continue
        A, b = system(Y, G, lam, cols[o0:o1], w[o0:o1], dtype)
        try:
            X[u] = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True, check_finite=False), b, check_finite=False)
        except np.linalg.LinAlgError:
            X[u], failed = np.nan, failed + 1
    return X, failed


def objective_brute(X, Y, lam, off, cols, w):
    """L over ALL pairs in float64, the definition: sum c (p - x.y)^2 + lam (|X|^2 + |Y|^2)."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    S = X @ Y.T
    C = np.ones_like(S)
    P = np.zeros_like(S)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    np.add.at(C, (rows, cols), w.astype(np.float64))
    P[rows, cols] = 1.0
    return float((C * (P - S) ** 2).sum() + float(lam) * ((X ** 2).sum() + (Y ** 2).sum()))


def objective(X, Y, G, lam, off, cols, w, dtype):
    """L through the identity slk_als_loss evaluates, in `dtype`: per row x^T G x + sum_obs [c (1 - s)^2 - s^2] + lam |x|^2, summed,
    plus lam |Y|^2."""
    X, Y, G, w = X.astype(dtype), Y.astype(dtype), G.astype(dtype), w.astype(dtype)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    s = (X[rows] * Y[cols]).sum(axis=1, dtype=dtype)
    per_entry = (w + dtype(1)) * (dtype(1) - s) ** 2 - s ** 2
    total = ((X @ G) * X).sum(dtype=dtype) + per_entry.sum(dtype=dtype) + dtype(lam) * ((X ** 2).sum(dtype=dtype) + (Y ** 2).sum(dtype=dtype))
    return float(total)


def fit(X, Y, lam, by_user, by_item, n_iter, dtype):
    """n_iter iterations (user half-step, item half-step) from the tables X, Y in `dtype`; returns (X, Y, [L per iteration])."""
    X, Y = X.astype(dtype), Y.astype(dtype)
    history = []
    for _ in range(n_iter):
        X, _ = half_step(Y, gram(Y, dtype), lam, *by_user, dtype)
        Y, _ = half_step(X, gram(X, dtype), lam, *by_item, dtype)
        history.append(objective(X, Y, gram(Y, dtype), lam, *by_user, dtype) if dtype is np.float32
                       else objective_brute(X, Y, lam, *by_user))
    return X, Y, history


def row_errors(got, want):
    """Per-row relative error |got - want|_2 / |want|_2 against the float64 rows (0 where both are the zero row)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    num = np.sqrt(((got - want) ** 2).sum(axis=1))
    den = np.sqrt((want ** 2).sum(axis=1))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), num)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def history_lengths(D):
    return [0, 1, D - 1, D, D + 1, 300, LONG, 0, 5]


class Problem(object):
    """A fixed table Y [I, D], its float32 Gram matrix and the histories of history_lengths(D).  Columns are drawn with
    replacement (the engine does not need them distinct; with 7 rows they cannot be); the row of length D + 1 is built from
    D + 2 raw pairs, the last a duplicate of the first, merged into one entry whose value is the sum.  c - 1 spans 0.1 .. 100."""

    def __init__(self, D, I, seed=0):
        rs = np.random.RandomState(500 + 11 * D + I + seed)
        self.D, self.I = D, I
        self.Y = rs.normal(0, 0.2, (I, D)).astype(np.float32)
        self.G = gram(self.Y, np.float32)
        lens = history_lengths(D)
        cols, vals = [], []
        for m in lens:
            c = rs.randint(0, I, m).astype(np.int64)
            v = (10.0 ** rs.uniform(-1, 2, m)).astype(np.float32)
            if m == D + 1:
                extra = np.float32(10.0 ** rs.uniform(-1, 2))
                off, mc, mv = merge_duplicates(np.zeros(2, np.int64), [c[0], c[0]], [v[0], extra], 1)
                assert len(mc) == 1
                v[0] = np.float32(mv[0])
            cols.append(c)
            vals.append(v)
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.cols = np.concatenate(cols)
        self.vals = np.concatenate(vals)
        self.H = len(lens)
        self.want, failed64 = half_step(self.Y, gram(self.Y, np.float64), LAMBDA, self.off, self.cols, self.vals, np.float64)
        self.yard, failed32 = half_step(self.Y, self.G, LAMBDA, self.off, self.cols, self.vals, np.float32)
        assert failed64 == 0 and failed32 == 0, 'the inputs must not fail'
        self.yard_err = float(row_errors(self.yard, self.want).max())


_PROBLEMS = {}


def problem(D, I):
    """One Problem per shape for the whole run (the references are computed once and never modified)."""
    if (D, I) not in _PROBLEMS:
        _PROBLEMS[(D, I)] = Problem(D, I)
    return _PROBLEMS[(D, I)]


class Device(object):
    """Device side of a Problem."""

    def __init__(self, be, pr, out=None):
        self.be, self.pr = be, pr
        self.Y, self.G = be.alloc(pr.Y), be.alloc(pr.G)
        self.off = be.alloc(pr.off)
        self.cols = be.alloc(pr.cols if pr.cols.size else np.zeros(1, np.int64))
        self.vals = be.alloc(pr.vals if pr.vals.size else np.zeros(1, np.float32))
        self.out = be.alloc(np.full((pr.H, pr.D), SENTINEL, np.float32) if out is None else out)
        self.failed = be.alloc(np.zeros(1, np.int32))

    def solve(self, rows=None, lam=LAMBDA):
        be, pr = self.be, self.pr
        d_rows = be.alloc(np.asarray(rows, np.int64)) if rows is not None else None
        be.engine.als_solve(be.ptr(self.Y), be.ptr(self.G), pr.D, lam, be.ptr(self.off), be.ptr(self.cols), be.ptr(self.vals),
                            be.ptr(d_rows), pr.H if rows is None else len(rows), be.ptr(self.out), be.ptr(self.failed), be.stream)
        assert same_bits(be.get(self.Y), pr.Y), 'the fixed table was written'
        assert same_bits(be.get(self.G), pr.G), 'the Gram matrix was written'
        return be.get(self.out).copy(), int(be.get(self.failed)[0])


def routed(be, value):
    return be.engine.options(als_wg_min_len=value)


# ---- 1. Gram ------------------------------------------------------------------------------------------------------------------------
def check_gram(be, D, n, seed=0):
    rs = np.random.RandomState(40 + D + n + seed)
    Y = rs.normal(0, 0.5, (n, D)).astype(np.float32)
    want = Y.astype(np.float64).T @ Y.astype(np.float64)
    yard = np.abs(gram(Y, np.float32).astype(np.float64) - want).max()  # float32 matmul on the same rows
    scale = np.abs(want).max()
    # an entry is a sum of n products, each rounded once more by the kernel's fused chain at the most: the float32 restatement's
    # error, and never less than one rounding of the largest entry
    tol = FACTOR * max(yard, scale * 2.0 ** -24)
    d_Y = be.alloc(Y)
    outs = []
    for _ in range(2):
        d_G = be.alloc(np.full((D, D), SENTINEL, np.float32))
        be.engine.als_gram(be.ptr(d_Y), n, D, be.ptr(d_G), be.stream)
        outs.append(be.get(d_G).copy())
    G = outs[0]
    print('gram D %d n %d: max error %.3g, yardstick %.3g, bound %.3g' % (D, n, np.abs(G - want).max(), yard, tol))
    assert same_bits(be.get(d_Y), Y), 'the table was written'
    assert np.abs(G.astype(np.float64) - want).max() <= tol, (D, n, float(np.abs(G - want).max()), tol)
    assert same_bits(G, np.ascontiguousarray(G.T)), 'not symmetric bit for bit'
    assert same_bits(outs[0], outs[1]), 'two calls differ'


def check_gram_empty(be, D=24):
    d_G = be.alloc(np.full((D, D), SENTINEL, np.float32))
    be.engine.als_gram(None, 0, D, be.ptr(d_G), be.stream)
    assert not be.get(d_G).any()


# ---- 2.-4. the half-step -------------------------------------------------------------------------------------------------------------
def check_half_step(be, D, I):
    """Against float64 at FACTOR x the float32 yardstick; no row fails; the routes give the same bits; empty histories give exact
    zeros; the fixed side is not written (Device.solve)."""
    pr = problem(D, I)
    bound = FACTOR * pr.yard_err
    first = None
    for route in ROUTES:
        with routed(be, route):
            got, failed = Device(be, pr).solve()
        err = row_errors(got, pr.want)
        print('half-step D %d I %d route %d: worst row error %.3g, yardstick %.3g, bound %.3g' % (D, I, route, err.max(), pr.yard_err, bound))
        assert failed == 0, (D, I, route, failed)
        assert np.isfinite(got).all()
        assert err.max() <= bound, (D, I, route, float(err.max()), bound, int(err.argmax()))
        for u in np.nonzero(np.diff(pr.off) == 0)[0]:
            assert same_bits(got[u], np.zeros(D, np.float32)), ('empty history', u)
        if first is None:
            first = got
        assert same_bits(got, first), ('the routes differ', D, I, route)


def check_composition(be, D, I):
    """A subset of the rows through the row list, the same rows in another order, every row alone: each row gets the bits of the
    full call, rows outside the list keep theirs."""
    pr = problem(D, I)
    rs = np.random.RandomState(9)
    for route in ROUTES:
        with routed(be, route):
            whole, _ = Device(be, pr).solve()
            subset = [6, 1, 4, 0]
            got, failed = Device(be, pr).solve(rows=subset)
            assert failed == 0
            for u in range(pr.H):
                if u in subset:
                    assert same_bits(got[u], whole[u]), ('subset', route, u)
                else:
                    assert (got[u] == SENTINEL).all(), ('a row outside the list was written', route, u)
            perm = list(rs.permutation(pr.H))
            got, _ = Device(be, pr).solve(rows=perm)
            assert same_bits(got, whole), ('permuted rows', route)
            for u in (2, 6):
                got, _ = Device(be, pr).solve(rows=[u])
                assert same_bits(got[u], whole[u]) and (np.delete(got, u, axis=0) == SENTINEL).all(), ('alone', route, u)
            # the same segment under another row number and in other company: a CSR holding rows 6 and 3 only
            lens = np.diff(pr.off)
            q = Problem.__new__(Problem)
            q.D, q.I, q.Y, q.G, q.H = pr.D, pr.I, pr.Y, pr.G, 2
            seg = [np.arange(pr.off[u], pr.off[u + 1]) for u in (6, 3)]
            q.off = np.concatenate([[0], np.cumsum([lens[6], lens[3]])]).astype(np.int64)
            q.cols, q.vals = pr.cols[np.concatenate(seg)], pr.vals[np.concatenate(seg)]
            got, _ = Device(be, q).solve()
            assert same_bits(got[0], whole[6]) and same_bits(got[1], whole[3]), ('another CSR', route)


def check_failure(be, D=24, I=7):
    """lambda = 0 and an all-zero fixed table: every non-empty system is the zero matrix.  Those rows are counted and left
    untouched; made indefinite for ONE row only (its columns point at zero rows of an otherwise good table), the others are solved."""
    pr = problem(D, I)
    zero = Problem.__new__(Problem)
    zero.__dict__.update(pr.__dict__)
    zero.Y, zero.G = np.zeros_like(pr.Y), np.zeros_like(pr.G)
    nonempty = int((np.diff(pr.off) > 0).sum())
    for route in ROUTES:
        with routed(be, route):
            got, failed = Device(be, zero).solve(lam=0.0)
            assert failed == nonempty, (route, failed, nonempty)
            for u, m in enumerate(np.diff(pr.off)):
                assert (got[u] == (SENTINEL if m else 0.0)).all(), (route, u)
    # one bad row among good ones: lambda = 0 and G = 0 handed in, so A is the row's own sum of outer products.  Row 1's one entry
    # points at a row of the table that is zero: its system is the zero matrix.  Rows 5 and 6 (300 and 600 entries, dim 24) are
    # positive definite and are held to FACTOR x the float32 restatement's error on these very systems.
    one = Problem.__new__(Problem)
    one.__dict__.update(problem(D, 333).__dict__)
    one.G = np.zeros_like(one.G)
    one.Y = one.Y.copy()
    one.Y[one.cols[one.off[1]]] = 0.0
    want, failed64 = half_step(one.Y, one.G, 0.0, one.off, one.cols, one.vals, np.float64, rows=[5, 6])
    yard, failed32 = half_step(one.Y, one.G, 0.0, one.off, one.cols, one.vals, np.float32, rows=[5, 6])
    assert failed64 == 0 and failed32 == 0
    bound = FACTOR * row_errors(yard[[5, 6]], want[[5, 6]]).max()
    for route in ROUTES:
        with routed(be, route):
            got, failed = Device(be, one).solve(rows=[1, 5, 6], lam=0.0)
            assert failed == 1, (route, failed)
            assert (got[1] == SENTINEL).all()
            assert np.isfinite(got[[5, 6]]).all() and row_errors(got[[5, 6]], want[[5, 6]]).max() <= bound


# ---- 6. the objective ------------------------------------------------------------------------------------------------------------------
def loss_problem(D=24, U=40, I=57, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.normal(0, 0.3, (U, D)).astype(np.float32)
    Y = rs.normal(0, 0.3, (I, D)).astype(np.float32)
    n = 500
    off, cols, r = merge_duplicates(rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(1, 4, n), U)
    w = (2.5 * r).astype(np.float32)
    return X, Y, off, cols, w


def check_loss(be, D=24):
    X, Y, off, cols, w = loss_problem(D)
    lam = np.float32(0.3)
    want = objective_brute(X, Y, lam, off, cols, w)
    G32 = gram(Y, np.float32)
    yard = abs(objective(X, Y, G32, lam, off, cols, w, np.float32) - want) / abs(want)
    # (never below a few roundings of the total: the float32 restatement can land on the float64 value by luck)
    bound = FACTOR * max(yard, 2.0 ** -22)
    d = [be.alloc(a) for a in (X, Y, G32, off, cols, w)]
    out = be.alloc(np.full(X.shape[0], np.nan, np.float64))
    be.engine.als_loss(be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), D, lam, be.ptr(d[3]), be.ptr(d[4]), be.ptr(d[5]), X.shape[0],
                       be.ptr(out), be.stream)
    rows = be.get(out)
    got = float(rows.sum()) + float(lam) * float((Y.astype(np.float64) ** 2).sum())
    print('objective: got %.9g want %.9g relative error %.3g, yardstick %.3g, bound %.3g' % (got, want, abs(got - want) / abs(want), yard, bound))
    assert np.isfinite(rows).all()
    assert abs(got - want) <= bound * abs(want), (got, want, yard)
    for a, h in zip(d[:3], (X, Y, G32)):
        assert same_bits(be.get(a), h), 'an input was written'


# ---- 8. refusals at the ABI ------------------------------------------------------------------------------------------------------------
def check_refusals(be):
    pr = problem(24, 333)
    dev = Device(be, pr)
    P = be.ptr
    d_loss = be.alloc(np.zeros(pr.H, np.float64))

    def refused(match, fn, *args):
        with pytest.raises(_native.SlkError, match=match) as e:
            fn(*args, be.stream)
        assert e.value.code == _native.SLK_EINVAL

    eng = be.engine
    solve = lambda **kw: [kw.get('Y', P(dev.Y)), kw.get('G', P(dev.G)), kw.get('D', pr.D), kw.get('lam', LAMBDA), kw.get('off', P(dev.off)),
                          kw.get('cols', P(dev.cols)), kw.get('vals', P(dev.vals)), None, kw.get('n', pr.H), kw.get('out', P(dev.out)),
                          kw.get('failed', P(dev.failed))]
    loss = lambda **kw: [kw.get('X', P(dev.out)), kw.get('Y', P(dev.Y)), kw.get('G', P(dev.G)), kw.get('D', pr.D), kw.get('lam', LAMBDA),
                         kw.get('off', P(dev.off)), kw.get('cols', P(dev.cols)), kw.get('vals', P(dev.vals)), kw.get('n', pr.H),
                         kw.get('out', P(d_loss))]
    for D in (129, 132, 256, 65, 0, -4):
        refused('embedding dim', eng.als_gram, P(dev.Y), pr.I, D, P(dev.G))
        refused('embedding dim', eng.als_solve, *solve(D=D))
        refused('embedding dim', eng.als_loss, *loss(D=D))
    refused('NULL', eng.als_gram, None, pr.I, pr.D, P(dev.G))
    refused('NULL', eng.als_gram, P(dev.Y), pr.I, pr.D, None)
    refused('negative', eng.als_gram, P(dev.Y), -1, pr.D, P(dev.G))
    for name in ('Y', 'G', 'off', 'cols', 'vals', 'out', 'failed'):
        refused('NULL', eng.als_solve, *solve(**{name: None}))
    for name in ('X', 'Y', 'G', 'off', 'cols', 'vals', 'out'):
        refused('NULL', eng.als_loss, *loss(**{name: None}))
    for n in (-1, 1 << 31):
        refused('n_rows', eng.als_solve, *solve(n=n))
        refused('n_rows', eng.als_loss, *loss(n=n))
    for lam in (-0.5, float('nan'), float('inf')):
        refused('lambda', eng.als_solve, *solve(lam=lam))
        refused('lambda', eng.als_loss, *loss(lam=lam))
    # inside an open fit scope that doubles the user table: the array holds only some of the current rows
    rs = np.random.RandomState(1)
    U, I, D = 9, 7, 24
    full = be.model([rs.rand(U, D), rs.rand(I, D), np.zeros(U), np.zeros(I)], opt='adagrad')
    small = Problem.__new__(Problem)
    small.__dict__.update(problem(D, I).__dict__)
    inner = Device(be, small)
    with eng.user_pingpong(full.tables, full.optim, stream=be.stream) as _:
        refused('ping-ponged', eng.als_gram, P(full.p[0]), U, D, P(inner.G))
        refused('ping-ponged', eng.als_solve, *solve(Y=P(full.p[0]), G=P(inner.G), off=P(inner.off), cols=P(inner.cols), vals=P(inner.vals),
                                                     out=P(inner.out), failed=P(inner.failed)))
        refused('ping-ponged', eng.als_solve, *solve(Y=P(inner.Y), G=P(inner.G), off=P(inner.off), cols=P(inner.cols), vals=P(inner.vals),
                                                     out=P(full.p[0]), failed=P(inner.failed), n=U))
        refused('ping-ponged', eng.als_loss, *loss(X=P(full.p[0]), Y=P(inner.Y), G=P(inner.G), off=P(inner.off), cols=P(inner.cols),
                                                   vals=P(inner.vals), n=U))
    # nothing was written by a refused call, and the same arguments, made good, are answered
    assert (be.get(dev.out) == SENTINEL).all() and int(be.get(dev.failed)[0]) == 0
    got, failed = dev.solve()
    assert failed == 0 and np.isfinite(got).all()
    eng.als_solve(*(solve(n=0) + [be.stream]))  # no rows: nothing to do


def check_profile_classes(be):
    pr = problem(24, 333)
    dev = Device(be, pr)
    d_loss = be.alloc(np.zeros(pr.H, np.float64))
    P = be.ptr
    d_gram = be.alloc(np.zeros((pr.D, pr.D), np.float32))
    be.engine.profile_enable(True)
    try:
        be.engine.profile_reset()
        be.engine.als_gram(P(dev.Y), pr.I, pr.D, P(d_gram), be.stream)
        dev.solve()
        be.engine.als_loss(P(dev.out), P(dev.Y), P(dev.G), pr.D, LAMBDA, P(dev.off), P(dev.cols), P(dev.vals), pr.H, P(d_loss), be.stream)
        prof = be.engine.profile_read()
    finally:
        be.engine.profile_enable(False)
    assert prof['score'][0] == 2 and prof['user_pass'][0] == 1, prof
    assert all(v[0] == 0 for k, v in prof.items() if k not in ('score', 'user_pass')), prof


# ---- 7. model level (tests/test_gpu_als.py; tests/test_host_als.py runs it through the emulator build) -------------------------------
MODEL = dict(embedding_dim=32, n_iter=3, regularization=0.5, alpha=8.0)
_MODEL_DATA = {}


def synthetic():
    """datasets/synthetic.py at its default shape (100 users, 1000 items, 10 000 interactions), generated once."""
    if 'train' not in _MODEL_DATA:
        from spotlight_amd.datasets.synthetic import generate_sequential
        _MODEL_DATA['train'] = generate_sequential(random_state=np.random.RandomState(5))
    return _MODEL_DATA['train']


def new_model(seed=3, **kw):
    from spotlight_amd.factorization.als import ALSFactorizationModel
    return ALSFactorizationModel(random_state=np.random.RandomState(seed), **dict(MODEL, **kw))


def tables_of(model):
    return [t.detach().cpu().numpy().copy() for t in model._net.tables()]


def model_csrs(train, alpha, weights=None):
    r = np.ones(len(train.user_ids)) if weights is None else weights
    by_user = merge_duplicates(train.user_ids, train.item_ids, r, train.num_users)
    by_item = merge_duplicates(train.item_ids, train.user_ids, r, train.num_items)
    f = lambda c: (c[0], c[1], (float(alpha) * c[2]).astype(np.float32))  # c - 1 = alpha * r, formed in float64, rounded once
    return f(by_user), f(by_item)


def fitted():
    """(model after fit(n_iter=3), its initial tables, the float64 and the float32 restatement from those tables), once."""
    from spotlight_amd.factorization import implicit as host
    key = ('fit', host._model_device().type)  # (the emulator's run and the GPU's may share a session)
    if key not in _MODEL_DATA:
        train = synthetic()
        model = new_model()
        model._initialize(train)
        init = tables_of(model)
        state = model._random_state.get_state()
        model.fit(train)
        after = model._random_state.get_state()
        by_user, by_item = model_csrs(train, MODEL['alpha'])
        lam = np.float32(MODEL['regularization'])
        ref64 = fit(init[0], init[1], lam, by_user, by_item, MODEL['n_iter'], np.float64)
        ref32 = fit(init[0], init[1], lam, by_user, by_item, MODEL['n_iter'], np.float32)
        _MODEL_DATA[key] = (model, init, ref64, ref32, (state, after))
    return _MODEL_DATA[key]


def check_model_fit_against_float64():
    """Six half-steps, each fed by the one before.  How the error compounds is MEASURED, not modelled: the float32 restatement
    runs the same six half-steps from the same initial tables, so its final error against the float64 run contains every
    half-step's own rounding carried through the systems of the following ones -- the same systems the kernel solves, whose
    sensitivity to a perturbed fixed table is therefore the same.  The kernel passes at FACTOR x that figure, per table; L per
    iteration likewise, and L never rises by more than FACTOR x the yardstick's own worst absolute error in L."""
    model, init, ref64, ref32, (state, after) = fitted()
    got = tables_of(model)
    for name, t, w64, w32 in (('user', got[0], ref64[0], ref32[0]), ('item', got[1], ref64[1], ref32[1])):
        yard = row_errors(w32, w64).max()
        err = row_errors(t, w64).max()
        print('fit: %s rows worst error %.3g, yardstick %.3g, bound %.3g' % (name, err, yard, FACTOR * yard))
        assert err <= FACTOR * yard, (name, float(err), float(yard))
    assert not got[2].any() and not got[3].any(), 'the biases must stay zero'
    L = np.asarray(model.loss_history_, np.float64)
    L64, L32 = np.asarray(ref64[2]), np.asarray(ref32[2])
    assert L.shape == L64.shape == (MODEL['n_iter'],)
    yard_abs = np.abs(L32 - L64).max()
    slack = FACTOR * max(yard_abs, 2.0 ** -22 * L64.max())
    print('fit: L', L, 'float64', L64, 'float32 restatement', L32, 'slack', slack)
    assert np.abs(L - L64).max() <= slack, (L, L64, slack)
    assert (np.diff(L) <= slack).all(), ('the objective rose', L, slack)
    assert (np.diff(L64) <= 0).all()  # the exact iteration never rises
    # fit() neither reads nor advances the RandomState once the tables are initialised
    assert (after[1] == state[1]).all() and after[2] == state[2]


def check_model_determinism_and_weights():
    train = synthetic()
    model = fitted()[0]
    base = tables_of(model)
    again = new_model()
    again.fit(train)
    for x, y in zip(tables_of(again), base):
        assert same_bits(x, y), 'two fits from one seed differ'
    assert again.loss_history_ == model.loss_history_
    from spotlight_amd.interactions import Interactions
    mk = lambda w: Interactions(train.user_ids, train.item_ids, weights=w, num_users=train.num_users, num_items=train.num_items)
    ones = new_model(use_weights=True)
    ones.fit(mk(np.ones(len(train.user_ids), np.float32)))
    for x, y in zip(tables_of(ones), base):
        assert same_bits(x, y), 'all-ones weights differ from use_weights=False'
    doubled = new_model(use_weights=True)
    doubled.fit(mk(np.full(len(train.user_ids), 2.0, np.float32)))
    twice = new_model(alpha=2 * MODEL['alpha'])
    twice.fit(train)
    for x, y in zip(tables_of(doubled), tables_of(twice)):
        assert same_bits(x, y), 'doubled weights differ from doubled alpha'
    # a second fit() continues from the current tables (and goes on appending to loss_history_)
    more = new_model(n_iter=1)
    for _ in range(MODEL['n_iter']):
        more.fit(train)
    for x, y in zip(tables_of(more), base):
        assert same_bits(x, y), 'three fits of one iteration differ from one fit of three'
    assert more.loss_history_ == model.loss_history_


def check_model_serving():
    """fold_in() of a training user's own history returns that user's row as a user half-step leaves it; recommend_vectors over
    those rows is recommend(); the fast path of mrr_score equals the generic per-user route; pickling."""
    import pickle
    from spotlight_amd import evaluation
    from spotlight_amd.interactions import Interactions
    train = synthetic()
    model = fitted()[0]
    users = np.array([0, 7, 31, 99])
    sel = np.isin(train.user_ids, users)
    relabel = {u: k for k, u in enumerate(users)}
    new = Interactions(np.array([relabel[u] for u in train.user_ids[sel]], np.int32), train.item_ids[sel], num_users=len(users),
                       num_items=train.num_items)
    state = model._random_state.get_state()
    before = tables_of(model)
    rows, biases = model.fold_in(new)
    assert rows.shape == (len(users), MODEL['embedding_dim']) and rows.dtype == np.float32
    assert biases.shape == (len(users),) and biases.dtype == np.float32 and not biases.any()
    for x, y in zip(tables_of(model), before):
        assert same_bits(x, y), 'fold_in() modified the model'
    after = model._random_state.get_state()
    assert (after[1] == state[1]).all() and after[2] == state[2]
    # what a user half-step over the whole training set leaves in those rows: the engine entries over the model's item table and
    # the CSR fit() builds, written into the user table of a copy of the model
    import torch
    from spotlight_amd.factorization import als, implicit as host
    clone = pickle.loads(pickle.dumps(model))
    U, V = [t.detach() for t in clone._net.tables()[:2]]
    engine, stream = host._engine_for(V.device), host._stream_for(V.device)
    by_user, _ = als.build_csrs(train.user_ids, train.item_ids, None, train.num_users, train.num_items, MODEL['alpha'], V.device)
    gram_items = torch.empty((V.shape[1], V.shape[1]), dtype=torch.float32, device=V.device)
    failed = torch.zeros(1, dtype=torch.int32, device=V.device)
    engine.als_gram(V.data_ptr(), V.shape[0], V.shape[1], gram_items.data_ptr(), stream)
    engine.als_solve(V.data_ptr(), gram_items.data_ptr(), V.shape[1], MODEL['regularization'], by_user.off.data_ptr(),
                     by_user.cols.data_ptr(), by_user.vals.data_ptr(), None, by_user.n_rows, U.data_ptr(), failed.data_ptr(), stream)
    assert int(failed.item()) == 0
    assert same_bits(rows, tables_of(clone)[0][users])
    got = clone.recommend_vectors(rows, biases, k=10)
    want = clone.recommend(users, k=10)
    assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1])
    # evaluation: the fused ranking against the per-user route
    test = Interactions(train.user_ids[::7], train.item_ids[::7], num_users=train.num_users, num_items=train.num_items)
    fast = evaluation.mrr_score(model, test, train=train)
    fused = model._fused_ranks
    try:
        model._fused_ranks = None
        model._batch_scores = None
        slow = evaluation.mrr_score(model, test, train=train)
    finally:
        del model._fused_ranks, model._batch_scores
        assert model._fused_ranks == fused
    assert np.array_equal(fast, slow)
    # pickle round trip
    back = pickle.loads(pickle.dumps(model))
    for x, y in zip(tables_of(back), before):
        assert same_bits(x, y)
    assert back.loss_history_ == model.loss_history_
    assert same_bits(back.predict(3), model.predict(3))
    for kw in ('n_iter', 'init', 'negatives'):
        with pytest.raises(TypeError):
            model.fold_in(new, **{kw: 1})


def check_model_representation_dim_wins():
    """A plain BilinearNet handed in as `representation=` whose dim differs from the embedding_dim keyword: as in the parent, the
    net's dim is the model's.  fit(), fold_in() and recommend_vectors() run at the net's dim (fold_in() sizes its rows from the
    item table); a net whose dim the engine does not solve is refused at construction."""
    from spotlight_amd.factorization.als import ALSFactorizationModel
    from spotlight_amd.factorization.representations import BilinearNet
    from spotlight_amd.interactions import Interactions
    rs = np.random.RandomState(13)
    U, I, n = 30, 41, 600
    train = Interactions(rs.randint(0, U, n).astype(np.int32), rs.randint(0, I, n).astype(np.int32), num_users=U, num_items=I)
    for net_dim, keyword in ((24, 8), (8, 24)):  # the net wider than the keyword, and narrower
        model = ALSFactorizationModel(embedding_dim=keyword, n_iter=2, regularization=0.5, alpha=8.0, random_state=np.random.RandomState(2),
                                      representation=BilinearNet(U, I, net_dim))
        model.fit(train)
        tables = tables_of(model)
        assert tables[0].shape == (U, net_dim) and tables[1].shape == (I, net_dim) and len(model.loss_history_) == 2
        users = np.array([3, 17, 29])
        sel = np.isin(train.user_ids, users)
        relabel = {u: k for k, u in enumerate(users)}
        new = Interactions(np.array([relabel[u] for u in train.user_ids[sel]], np.int32), train.item_ids[sel], num_users=len(users),
                           num_items=I)
        rows, biases = model.fold_in(new)
        assert rows.shape == (len(users), net_dim) and biases.shape == (len(users),)
        # against the float64 restatement of that half-step, at FACTOR x the float32 restatement's error
        by_user, _ = model_csrs(new, 8.0)
        want, _ = half_step(tables[1], gram(tables[1], np.float64), 0.5, *by_user, np.float64)
        yard, _ = half_step(tables[1], gram(tables[1], np.float32), 0.5, *by_user, np.float32)
        assert row_errors(rows, want).max() <= FACTOR * row_errors(yard, want).max()
        import types  # (Interactions itself refuses empty id arrays: anything with its four attributes serves)
        empty = model.fold_in(types.SimpleNamespace(user_ids=np.zeros(0, np.int32), item_ids=np.zeros(0, np.int32), weights=None,
                                                    num_users=0, num_items=I))
        assert empty[0].shape == (0, net_dim)
        got = model.recommend_vectors(rows, biases, k=5)
        scores = rows.astype(np.float64) @ tables[1].astype(np.float64).T
        assert got[0].shape == (len(users), 5)
        np.testing.assert_allclose(got[1], np.sort(scores, axis=1)[:, ::-1][:, :5], rtol=1e-5, atol=1e-6)
    for bad in (132, 70, 256):
        with pytest.raises(ValueError, match='embedding dim'):
            ALSFactorizationModel(representation=BilinearNet(U, I, bad))


def check_model_failure_and_scope(engine, stream=0):
    from spotlight_amd.interactions import Interactions
    train = synthetic()
    # an indefinite system: regularization 0 and all-zero tables (the Gram matrix and every outer product vanish)
    import torch
    model = new_model(regularization=0.0)
    model._initialize(train)
    with torch.no_grad():
        for t in model._net.tables():
            t.zero_()
    with pytest.raises(ValueError, match=r'regularization') as e:
        model.fit(train)
    assert str(len(np.unique(train.user_ids))) in str(e.value)  # the count of failed rows: every user with a history
    # inside an open fit scope of another model on the same tables
    model = fitted()[0]
    from spotlight_amd.factorization.implicit import _OptimizerBinding
    binding = _OptimizerBinding(torch.optim.Adagrad(model._net.parameters(), lr=0.05), model._net.tables(), False)
    before = tables_of(model)
    with engine.bias_shadow(model._slk_tables(), binding.as_struct(), stream=stream):
        with pytest.raises(_native.SlkError, match='shadowed'):
            model.fit(train)
        with pytest.raises(_native.SlkError, match='shadowed'):
            model.fold_in(Interactions(np.array([0]), np.array([1]), num_users=1, num_items=train.num_items))
    with engine.user_pingpong(model._slk_tables(), binding.as_struct(), stream=stream):
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            model.fit(train)
    for x, y in zip(tables_of(model), before):
        assert same_bits(x, y), 'a refused fit() modified the model'
