"""Shared checks of the neighbour entries (include/spotlight_hip.h: slk_rows_inv_norm, slk_neighbors_topk, slk_neighbors_scores),
run on the emulator build (tests/test_emu_neighbors.py) and on the gfx950 library (tests/test_gpu_neighbors.py).

Selection is checked against the host selection of tests/topk_checks.py applied to the score rows slk_neighbors_scores returns
on the same backend (items exactly, scores bit for bit); the values of those rows and of the inverse norms against float64,
within bounds derived from the arithmetic the header specifies (see check_inverse_norms / check_cosine_values)."""
import numpy as np
import pytest

from spotlight_amd import _native
from topk_checks import (DS, ITEMS, KS, K_MAX, ROWS, assert_same, bilinear_scores, bilinear_topk, csr, host_topk,  # noqa: F401
                         random_exclusions, random_params)

METRICS = ('cosine', 'dot')
EPS = 2.0 ** -24  # half an ulp of 1.0f: the relative error of one float32 rounding


def inv_norm(be, rows):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    d_rows = be.alloc(rows)
    d_out = be.alloc(np.full(rows.shape[0], 7.5, dtype=np.float32))
    be.engine.rows_inv_norm(be.ptr(d_rows), rows.shape[0], rows.shape[1], be.ptr(d_out), be.stream)
    return be.get(d_out).copy()


class Setup(object):
    """A table and query rows on the device, with their inverse norms (the engine's own) for the cosine calls."""

    def __init__(self, be, table, queries):
        self.be = be
        self.table = np.ascontiguousarray(table, dtype=np.float32)
        self.queries = np.ascontiguousarray(queries, dtype=np.float32)
        self.I, self.D = self.table.shape
        self.n = self.queries.shape[0]
        self.d_table, self.d_q = be.alloc(self.table), be.alloc(self.queries)
        self.d_ts = be.alloc(np.zeros(self.I, np.float32))
        self.d_qs = be.alloc(np.zeros(self.n, np.float32))
        be.engine.rows_inv_norm(be.ptr(self.d_table), self.I, self.D, be.ptr(self.d_ts), be.stream)
        be.engine.rows_inv_norm(be.ptr(self.d_q), self.n, self.D, be.ptr(self.d_qs), be.stream)

    def scales(self, metric):
        P = self.be.ptr
        return (P(self.d_ts), P(self.d_qs)) if metric == 'cosine' else (None, None)

    def topk(self, k, metric, exc=None):
        be = self.be
        ts, qs = self.scales(metric)
        d_eo, d_ei = csr(exc, be)
        d_items = be.alloc(np.full((self.n, k), -7, dtype=np.int64))
        d_scores = be.alloc(np.full((self.n, k), 7.5, dtype=np.float32))
        be.engine.neighbors_topk(be.ptr(self.d_table), self.I, self.D, ts, be.ptr(self.d_q), qs, self.n, k, be.ptr(d_eo), be.ptr(d_ei),
                                 be.ptr(d_items), be.ptr(d_scores), be.stream)
        return be.get(d_items).copy(), be.get(d_scores).copy()

    def scores(self, metric):
        be = self.be
        ts, qs = self.scales(metric)
        out = be.alloc(np.full((self.n, self.I), np.nan, dtype=np.float32))
        be.engine.neighbors_scores(be.ptr(self.d_table), self.I, self.D, ts, be.ptr(self.d_q), qs, self.n, be.ptr(out), be.stream)
        return be.get(out).copy()

    def check(self, k, metric, exc=None, what=''):
        """neighbors_topk == the host selection of the rows neighbors_scores returns"""
        got = self.topk(k, metric, exc)
        assert_same(got, host_topk(self.scores(metric), exc, k), (what, metric, k, exc is not None))
        return got


def check_random(be, D, I, n_q, k, seed=5):
    """Random rows: both metrics, without exclusions and with a different list per query."""
    rng = np.random.RandomState(seed + D + I + n_q + k)
    s = Setup(be, rng.randn(I, D), rng.randn(n_q, D))
    exc = random_exclusions(rng, n_q, I)
    for metric in METRICS:
        s.check(k, metric, None, ('random', D, I, n_q))
        s.check(k, metric, exc, ('random + exclusions', D, I, n_q))


def check_inverse_norms(be, D, n=333):
    """rows_inv_norm against 1 / sqrt in float64: relative error at most (D / 2 + 4) * 2^-24 -- D roundings on a sum of
    non-negative terms (each at most 2^-24 of the running sum, so of the total), halved by the square root, plus the root's and
    the quotient's own roundings and slack for a divide that is not correctly rounded.  An all-zero row gives exactly +0.0f."""
    rng = np.random.RandomState(7 + D)
    rows = rng.randn(n, D).astype(np.float32)
    rows[0::2] *= np.float32(0.1)
    rows[1::2] *= np.float32(10.0)
    rows[17] = 0.0
    rows[n - 1] = -0.0
    got = inv_norm(be, rows)
    assert got.dtype == np.float32 and got.shape == (n,)
    zero = np.array([17, n - 1])
    assert np.all(got[zero].view(np.uint32) == 0), got[zero]
    live = np.setdiff1d(np.arange(n), zero)
    want = 1.0 / np.sqrt((rows[live].astype(np.float64) ** 2).sum(axis=1))
    rel = np.abs(got[live].astype(np.float64) - want) / want
    print('inverse norms: dim %d, worst relative error %.3g, bound %.3g' % (D, rel.max(), (D / 2.0 + 4) * EPS))
    assert rel.max() <= (D / 2.0 + 4) * EPS, (D, rel.max())
    # n_rows == 0: a no-op
    be.engine.rows_inv_norm(None, 0, D, None, be.stream)


def fma_chain_rows(queries, table):
    """[n, I] float32: acc = fma(q_d, v_d, acc) over d ascending from 0.  (The product of two float32 is exact in float64; the
    sum is rounded to double, then to float: a double rounding that differs from the fused one in rare last-bit cases only.)"""
    q, v = queries.astype(np.float64), table.astype(np.float64)
    acc = np.zeros((q.shape[0], v.shape[0]), dtype=np.float32)
    for d in range(q.shape[1]):
        acc = (np.outer(q[:, d], v[:, d]) + acc.astype(np.float64)).astype(np.float32)
    return acc


def check_cosine_values(be, D, I=333, n_q=33):
    """|score - cos64| <= (2 D + 16) * 2^-24 against the float64 cosine of the same float32 rows: D * 2^-24 * |q| |v| from the fma
    chain (Cauchy-Schwarz), twice the inverse-norm bound (D / 2 + 4) * 2^-24, the two products.  'dot' scores against the float32
    fma-ordered chain formed with numpy, within D * 2^-24 * |q| |v|."""
    rng = np.random.RandomState(11 + D)
    table, queries = rng.randn(I, D).astype(np.float32), rng.randn(n_q, D).astype(np.float32)
    table[0::2] *= np.float32(0.1)
    table[1::2] *= np.float32(10.0)
    queries[0::3] *= np.float32(10.0)
    queries[1::3] *= np.float32(0.1)
    s = Setup(be, table, queries)
    q64, v64 = queries.astype(np.float64), table.astype(np.float64)
    nq, nv = np.sqrt((q64 ** 2).sum(axis=1)), np.sqrt((v64 ** 2).sum(axis=1))
    cos64 = (q64 @ v64.T) / np.outer(nq, nv)
    err = np.abs(s.scores('cosine').astype(np.float64) - cos64)
    print('cosine: dim %d, worst error %.3g, bound %.3g' % (D, err.max(), (2 * D + 16) * EPS))
    assert err.max() <= (2 * D + 16) * EPS, (D, err.max())
    dot = s.scores('dot')
    derr = np.abs(dot.astype(np.float64) - fma_chain_rows(queries, table).astype(np.float64)) / np.outer(nq, nv)
    print('dot: dim %d, worst error / (|q||v|) %.3g, bound %.3g' % (D, derr.max(), D * EPS))
    assert derr.max() <= D * EPS, (D, derr.max())


TIES = (3, 9, 22, 40)


def check_ties(be, D=24, I=333):
    """Rows 3, 9, 22 and 40 are copies of one row: equal scores come back in ascending id, for every k at which the copies
    straddle the k boundary -- with the query one of the copies (self-exclusion on and off), and with other rows as queries."""
    rng = np.random.RandomState(13)
    table = rng.randn(I, D).astype(np.float32)
    for t in TIES[1:]:
        table[t] = table[TIES[0]]
    q_ids = np.array([9, 3, 100, 7, 40], dtype=np.int64)
    s = Setup(be, table, table[q_ids])
    self_exc = [np.array([q]) for q in q_ids]
    for metric in METRICS:
        rows = s.scores(metric)
        assert all(np.array_equal(rows[:, t].view(np.uint32), rows[:, TIES[0]].view(np.uint32)) for t in TIES[1:])
        # where the first copy stands in every query's order: k from one copy inside to all of them inside
        full = host_topk(rows, None, I)[0]
        first = [int(np.nonzero(full[r] == TIES[0])[0][0]) for r in range(len(q_ids))]
        for k in sorted(set(min(p + j, K_MAX) for p in first for j in (1, 2, 3, 4, 5))):
            for exc in (None, self_exc):
                got = s.check(k, metric, exc, 'ties')
                for r in range(len(q_ids)):
                    at = [int(np.nonzero(got[0][r] == t)[0][0]) for t in TIES if t in got[0][r]]
                    assert at == list(range(at[0], at[0] + len(at))) if at else True, (r, k, got[0][r])  # adjacent, ascending id
    # cosine, a copy as the query: the copies score highest (the query itself among them unless excluded)
    got = s.topk(2, 'cosine', self_exc)
    assert np.array_equal(got[0][0], [3, 22]) and np.array_equal(got[0][1], [9, 22]) and np.array_equal(got[0][4], [3, 9]), got[0]
    got = s.topk(3, 'cosine')
    for r in (0, 1, 4):
        assert np.array_equal(got[0][r], [3, 9, 22]), got[0]


def check_zero_rows(be, D=6, I=40, k=10):
    """All-zero table rows score exactly 0 under cosine and sort by id among the zeros; an all-zero query returns ids 0 .. k-1
    with score 0."""
    rng = np.random.RandomState(17)
    table = rng.randn(I, D).astype(np.float32)
    zeros = [2, 5, 31]
    table[zeros] = 0.0
    queries = rng.randn(4, D).astype(np.float32)
    queries[2] = 0.0
    s = Setup(be, table, queries)
    rows = s.scores('cosine')
    assert np.all(rows[:, zeros] == 0) and np.all(rows[2] == 0) and not np.any(np.isnan(rows))
    got = s.check(I, 'cosine', None, 'zero rows')
    for r in (0, 1, 3):
        at = [int(np.nonzero(got[0][r] == z)[0][0]) for z in zeros]
        assert at == list(range(at[0], at[0] + 3)) and np.all(got[1][r][at] == 0), (r, got[0][r])
    for metric in METRICS:
        got = s.check(k, metric, None, 'zero query')
        assert np.array_equal(got[0][2], np.arange(k)) and np.all(got[1][2] == 0), got[0][2]


def check_nan(be, D=24):
    """A table row holding a NaN scores NaN for every query under both metrics: it orders after every number and comes back as
    the quiet NaN 0x7fc00000."""
    rng = np.random.RandomState(19)
    for I, k in ((7, 10), (333, 10), (333, K_MAX)):
        table = rng.randn(I, D).astype(np.float32)
        table[5, 1] = np.nan
        s = Setup(be, table, rng.randn(33, D))
        for metric in METRICS:
            got = s.check(k, metric, None, ('nan', I))
            if k >= I:
                assert np.all(got[0][:, I - 1] == 5) and np.all(got[1][:, I - 1].view(np.uint32) == 0x7fc00000) and np.all(got[0][:, I:] == -1)
            else:
                assert not np.any(got[0] == 5) and not np.any(np.isnan(got[1]))
            exc = [np.setdiff1d(np.arange(I), [2, 5, 6]) for _ in range(33)]
            got = s.check(k, metric, exc, ('nan + exclusions', I))
            assert np.all(got[0][:, 2] == 5) and np.all(got[1][:, 2].view(np.uint32) == 0x7fc00000) and np.all(got[0][:, 3:] == -1)


def check_signed_zero_pair(be, D=6, I=40):
    """Row 9 scores -0.0 (every product of its chain underflows to -0), row 4 +0.0, everything else is negative: the two zeros
    tie and the smaller id wins."""
    table = np.full((I, D), -1.0, np.float32)
    table[9] = -1e-30
    table[4] = 0.0
    s = Setup(be, table, np.full((3, D), 1e-30, np.float32))
    rows = s.scores('dot')
    assert np.all(np.signbit(rows[:, 9])) and np.all(rows[:, 9] == 0) and not np.any(np.signbit(rows[:, 4])) and np.all(rows[:, 4] == 0)
    assert np.all(np.delete(rows, [4, 9], axis=1) < 0)
    for k in (1, 2, 10):
        got = s.check(k, 'dot', None, 'signed zeros')
        assert np.array_equal(got[0][:, :2], np.tile([4, 9], (3, 1))[:, :k]), got[0]


def check_exclusion_cases(be, D=24, I=333, n_q=65, k=10):
    """The query's own id never appears; an empty list; a list holding every row (all padding); all but k - 1 rows (tail padding)."""
    rng = np.random.RandomState(23)
    table = rng.randn(I, D).astype(np.float32)
    q_ids = rng.randint(0, I, n_q)
    s = Setup(be, table, table[q_ids])
    for metric in METRICS:
        free = s.check(k, metric, None, 'no exclusions')
        if metric == 'cosine':  # a row is its own nearest neighbour
            assert np.array_equal(free[0][:, 0], q_ids)
        got = s.check(k, metric, [np.array([q]) for q in q_ids], 'self')
        assert not np.any(got[0] == q_ids[:, None]) and np.all(got[0] >= 0)
        assert_same(s.topk(k, metric, [np.zeros(0, np.int64)] * n_q), free, 'empty lists')
        got = s.topk(k, metric, [np.arange(I)] * n_q)
        assert np.all(got[0] == -1) and np.all(np.isneginf(got[1]))
        exc = [np.setdiff1d(np.arange(I), rng.choice(I, k - 1, replace=False)) if r % 2 == 0 else np.array([q_ids[r]])
               for r in range(n_q)]
        got = s.check(k, metric, exc, 'all but k - 1')
        assert np.all(got[0][0::2, k - 1:] == -1) and np.all(np.isneginf(got[1][0::2, k - 1:])) and np.all(got[0][0::2, :k - 1] >= 0)
        assert np.all(got[0][1::2] >= 0)


def check_k_above_rows(be, D=6, I=7, k=10):
    rng = np.random.RandomState(29)
    table = rng.randn(I, D).astype(np.float32)
    for n_q in (1, 33):
        q_ids = rng.randint(0, I, n_q)
        s = Setup(be, table, table[q_ids])
        for metric in METRICS:
            got = s.check(k, metric, None, 'k > rows')
            assert np.all(got[0][:, I:] == -1) and np.all(np.sort(got[0][:, :I], axis=1) == np.arange(I))
            got = s.check(k, metric, [np.array([q]) for q in q_ids], 'k > rows, self excluded')
            assert np.all(got[0][:, I - 1:] == -1) and not np.any(got[0] == q_ids[:, None])


def check_chunking_invariance(be, k, D=24, I=1500, n_q=65):
    """One block per workgroup, two, the automatic cut and one workgroup per row tile: identical arrays (ties included)."""
    rng = np.random.RandomState(31)
    vecs = rng.randn(40, D).astype(np.float32)
    table = vecs[rng.randint(0, 40, I)]
    s = Setup(be, table, rng.randn(n_q, D))
    exc = random_exclusions(rng, n_q, I)
    for metric in METRICS:
        want = host_topk(s.scores(metric), exc, k)
        for per in (0, 128, 256, 1536):
            with be.engine.options(topk_items_per_wg=per):
                assert be.engine.get_option('topk_items_per_wg') == per
                assert_same(s.topk(k, metric, exc), want, ('chunking', metric, per, k))
        assert be.engine.get_option('topk_items_per_wg') == 0


def check_existing_sweeps_untouched(be, D=24, I=333, n_rows=65, k=10):
    """The neighbour calls share the ctx's top-k scratch with slk_*_topk: bilinear_topk / bilinear_scores of a random model
    return after them what they returned before."""
    rng = np.random.RandomState(37)
    params = random_params(rng, 100, I, D)
    users = rng.randint(0, 100, n_rows)
    exc = random_exclusions(rng, n_rows, I)
    dev = be.model(params)
    before = bilinear_topk(be, dev, users, k, exc), bilinear_scores(be, dev, users)
    s = Setup(be, rng.randn(1500, D), rng.randn(150, D))
    for metric in METRICS:
        s.check(K_MAX, metric, random_exclusions(rng, 150, 1500), 'between')
    after = bilinear_topk(be, dev, users, k, exc), bilinear_scores(be, dev, users)
    assert np.array_equal(before[0][0], after[0][0])
    assert np.array_equal(before[0][1].view(np.uint32), after[0][1].view(np.uint32))
    assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    assert_same(after[0], host_topk(after[1], exc, k), 'after the neighbour calls')


def check_refusals(be):
    rng = np.random.RandomState(41)
    I, D, n, k = 20, 8, 4, 5
    s = Setup(be, rng.randn(I, D), rng.randn(n, D))
    P, eng = be.ptr, be.engine
    d_items = be.alloc(np.zeros((n, K_MAX + 1), dtype=np.int64))
    d_scores = be.alloc(np.zeros((n, K_MAX + 1), dtype=np.float32))
    d_out = be.alloc(np.zeros((n, I), dtype=np.float32))
    ok = dict(table=P(s.d_table), I=I, D=D, ts=P(s.d_ts), q=P(s.d_q), qs=P(s.d_qs), n=n, k=k, eo=None, ei=None, items=P(d_items),
              scores=P(d_scores), out=P(d_out))

    def topk(**kw):
        a = dict(ok, **kw)
        eng.neighbors_topk(a['table'], a['I'], a['D'], a['ts'], a['q'], a['qs'], a['n'], a['k'], a['eo'], a['ei'], a['items'],
                           a['scores'], be.stream)

    def scores(**kw):
        a = dict(ok, **kw)
        eng.neighbors_scores(a['table'], a['I'], a['D'], a['ts'], a['q'], a['qs'], a['n'], a['out'], be.stream)

    def refused(match, fns=(topk, scores), **kw):
        for fn in fns:
            with pytest.raises(_native.SlkError, match=match) as e:
                fn(**kw)
            assert e.value.code == _native.SLK_EINVAL

    refused('at least 1', fns=(topk,), k=0)
    refused('at least 1', fns=(topk,), k=-3)
    refused('at most SLK_TOPK_K_MAX', fns=(topk,), k=K_MAX + 1)
    refused('NULL', fns=(topk,), items=None)
    refused('NULL', fns=(topk,), scores=None)
    refused('NULL', fns=(scores,), out=None)
    refused('NULL', table=None)
    refused('bad arguments', q=None)
    refused('no table rows', I=0)
    refused('no table rows', I=-5)
    refused('32 bits', I=2 ** 32 - 1)
    refused('dim', D=0)
    refused('dim', D=-8)
    refused('unsupported', D=70)  # neither a multiple of 4 nor <= 64: no row layout
    refused('go together', ts=None)
    refused('go together', qs=None)
    d_ei = be.alloc(np.arange(8, dtype=np.int64))  # (held in names: the device arrays must outlive the calls)
    d_down, d_neg, d_fine = [be.alloc(np.array(x, dtype=np.int64)) for x in ([0, 3, 2, 4, 4], [-1, 0, 2, 4, 4], [0, 1, 2, 3, 4])]
    refused('not sorted', fns=(topk,), eo=P(d_down), ei=P(d_ei))
    refused('not sorted', fns=(topk,), eo=P(d_neg), ei=P(d_ei))
    refused('bad arguments', fns=(topk,), eo=P(d_fine), ei=None)
    d_norm = be.alloc(np.zeros(I, np.float32))
    for bad, match in (((None, I, D, P(d_norm)), 'NULL'), ((P(s.d_table), I, D, None), 'NULL'), ((P(s.d_table), -1, D, P(d_norm)), 'n_rows'),
                       ((P(s.d_table), I, 0, P(d_norm)), 'dim'), ((P(s.d_table), I, 70, P(d_norm)), 'unsupported')):
        with pytest.raises(_native.SlkError, match=match) as e:
            eng.rows_inv_norm(*bad, be.stream)
        assert e.value.code == _native.SLK_EINVAL
    # the user table of an open ping-pong scope: a mix of current and superseded rows, refused as table and as queries
    U = 30
    dev = be.model(random_params(rng, U, I, D), opt='adagrad', lr=0.05)
    d_un = be.alloc(np.zeros(U, np.float32))
    with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream):
        refused('ping-ponged', table=P(dev.p[0]), I=U, ts=P(d_un))
        refused('ping-ponged', q=P(dev.p[0]))
        with pytest.raises(_native.SlkError, match='ping-ponged'):
            eng.rows_inv_norm(P(dev.p[0]), U, D, P(d_un), be.stream)
        topk(table=P(dev.p[1]), ts=None, qs=None)  # (the item table is whole)
    # ... and answered once the scope is closed, as the good arguments are after all the refusals
    eng.rows_inv_norm(P(dev.p[0]), U, D, P(d_un), be.stream)
    topk(table=P(dev.p[0]), I=U, ts=P(d_un))
    for metric in METRICS:
        s.check(k, metric, None, 'after refusals')
