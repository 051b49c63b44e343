"""Shared checks of the top-k entries (include/spotlight_hip.h: slk_bilinear_topk, slk_poolnet_topk, slk_shard_topk), run on the
emulator build (tests/test_emu_topk.py) and on the gfx950 library (tests/test_gpu_topk.py).

The expected value is always formed on the host: the score rows of the slk_*_scores entries (which predate the top-k entries
and are pinned to the f32 fma chain by their own tests), ordered with np.lexsort by (NaN last, score descending, id ascending),
the row's exclusion list removed, padded with item -1 / score -inf.  Items are compared exactly, scores bit for bit modulo the
sign of a zero (a NaN only has to be a NaN)."""
import numpy as np
import pytest

from spotlight_amd import _native

K_MAX = _native.TOPK_K_MAX
DS = (6, 24, 72)           # scalar loads, the operand in registers, two staged chunks
ITEMS = (7, 333, 1500)     # fewer than k, no multiple of the 128-item block, several blocks
ROWS = (1, 33, 65, 150)    # a 32-row tile, two of them / a 64-row tile, more than one tile
KS = (1, 10, K_MAX)


def order_of(scores):
    """Indices of a score row by THE ORDER of the header: NaN last, score descending (-0.0 == +0.0), id ascending."""
    s = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -(np.where(nan, np.float32(0), s).astype(np.float64) + 0.0), nan))


def host_topk(scores, exc, k, ids=None):
    """scores [n, m] (column j = item ids[j], default j); exc: per row the excluded ITEM ids or None."""
    n, m = scores.shape
    ids = np.arange(m, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    items = np.full((n, k), -1, dtype=np.int64)
    out = np.full((n, k), -np.inf, dtype=np.float32)
    for r in range(n):
        keep = np.ones(m, bool) if exc is None else ~np.isin(ids, exc[r])
        cols = np.nonzero(keep)[0]
        sub = scores[r][cols]
        nan = np.isnan(sub)
        o = np.lexsort((ids[cols], -(np.where(nan, np.float32(0), sub).astype(np.float64) + 0.0), nan))[:k]
        items[r, :len(o)] = ids[cols][o]
        out[r, :len(o)] = sub[o]
    return items, out


def assert_same(got, want, what):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == np.int64 and gs.dtype == np.float32 and gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1))[0]
    assert np.array_equal(gi, wi), (what, 'items differ in rows', bad[:6], gi[bad[:1]], wi[bad[:1]])
    nan = np.isnan(ws)
    assert np.array_equal(np.isnan(gs), nan), (what, 'NaN positions')
    zero = (ws == 0) & ~nan
    assert np.all(gs[zero] == 0), (what, 'zeros')
    rest = ~nan & ~zero
    assert np.array_equal(gs[rest].view(np.uint32), ws[rest].view(np.uint32)), (what, 'score bits')


def csr(exc, be):
    """(d_exc_off, d_exc_items) of per-row lists made sorted and distinct, or (None, None)."""
    if exc is None:
        return None, None
    lists = [np.unique(np.asarray(x, dtype=np.int64)) for x in exc]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.concatenate(lists).astype(np.int64) if off[-1] else np.zeros(1, np.int64)
    return be.alloc(off), be.alloc(flat)


def bilinear_topk(be, dev, users, k, exc=None):
    n = len(users)
    d_users = be.alloc(np.asarray(users, dtype=np.int64))
    d_eo, d_ei = csr(exc, be)
    d_items = be.alloc(np.full((n, k), -7, dtype=np.int64))
    d_scores = be.alloc(np.full((n, k), 7.5, dtype=np.float32))
    be.engine.bilinear_topk(dev.tables, be.ptr(d_users), n, k, be.ptr(d_eo), be.ptr(d_ei), be.ptr(d_items), be.ptr(d_scores),
                            be.stream)
    return be.get(d_items).copy(), be.get(d_scores).copy()


def bilinear_scores(be, dev, users):
    n, I = len(users), dev.tables.num_items
    d_users = be.alloc(np.asarray(users, dtype=np.int64))
    out = be.alloc(np.full((n, I), np.nan, dtype=np.float32))
    be.engine.bilinear_scores(dev.tables, be.ptr(d_users), n, be.ptr(out), be.stream)
    return be.get(out).copy()


def random_exclusions(rng, n, I, frac_empty=0.3, longest=40):
    return [np.zeros(0, np.int64) if rng.rand() < frac_empty else rng.randint(0, I, rng.randint(1, longest)).astype(np.int64)
            for _ in range(n)]


def check_bilinear(be, params, users, k, exc=None, what='', **model_kw):
    dev = be.model(params, **model_kw)
    want = host_topk(bilinear_scores(be, dev, users), exc, k)
    got = bilinear_topk(be, dev, users, k, exc)
    assert_same(got, want, (what, k))
    return got


def random_params(rng, U, I, D):
    return [rng.randn(U, D).astype(np.float32), rng.randn(I, D).astype(np.float32), rng.randn(U).astype(np.float32),
            rng.randn(I).astype(np.float32)]


def check_random(be, D, I, n_rows, k, seed=3):
    """Random plain tables: without exclusions and with a different list per row (rows of one tile in different groups)."""
    rng = np.random.RandomState(seed + D + I + n_rows + k)
    U = 200
    params = random_params(rng, U, I, D)
    users = rng.randint(0, U, n_rows)
    check_bilinear(be, params, users, k, None, ('random', D, I, n_rows))
    check_bilinear(be, params, users, k, random_exclusions(rng, n_rows, I), ('random + exclusions', D, I, n_rows))


def check_bloom(be, D=24, I=333, n_rows=65, k=10, user_bloom=0):
    """A BloomEmbedding item table (the element-by-element loader), and one on the user side (representations from scratch)."""
    from oracle.oracle import bloom_desc
    rng = np.random.RandomState(17)
    U = 90
    ud = bloom_desc(n_hash=user_bloom) if user_bloom else None
    idesc = bloom_desc(n_hash=4)
    params = [rng.randn(int(0.5 * U) if ud else U, D).astype(np.float32), rng.randn(int(0.4 * I), D).astype(np.float32),
              rng.randn(U).astype(np.float32), rng.randn(I).astype(np.float32)]
    users = rng.randint(0, U, n_rows)
    check_bilinear(be, params, users, k, random_exclusions(rng, n_rows, I), ('bloom', D, I), user_bloom=ud, item_bloom=idesc)


def check_poolnet(be, D, I, n_seq, k, bloom=0, L=5):
    """slk_poolnet_topk against the rows of slk_poolnet_scores, excluding each sequence's own items (exclude_preceding)."""
    from oracle.oracle import bloom_desc
    rng = np.random.RandomState(23 + D + I)
    desc = bloom_desc(n_hash=bloom) if bloom else None
    rows = int(0.5 * I) if bloom else I
    E = rng.randn(rows, D).astype(np.float32)
    E[0] = 0.0
    dev = be.seq_model([E, rng.randn(I).astype(np.float32)], item_bloom=desc)
    seqs = rng.randint(0, I, (n_seq, L)).astype(np.int64)
    d_seqs = be.alloc(seqs)
    out = be.alloc(np.full((n_seq, I), np.nan, dtype=np.float32))
    be.engine.poolnet_scores(dev.tables, be.ptr(d_seqs), n_seq, L, be.ptr(out), be.stream)
    scores = be.get(out).copy()
    for exc in (None, [seqs[r] for r in range(n_seq)]):
        d_eo, d_ei = csr(exc, be)
        d_items = be.alloc(np.full((n_seq, k), -7, dtype=np.int64))
        d_scores = be.alloc(np.full((n_seq, k), 7.5, dtype=np.float32))
        be.engine.poolnet_topk(dev.tables, be.ptr(d_seqs), n_seq, L, k, be.ptr(d_eo), be.ptr(d_ei), be.ptr(d_items),
                               be.ptr(d_scores), be.stream)
        assert_same((be.get(d_items).copy(), be.get(d_scores).copy()), host_topk(scores, exc, k), ('poolnet', D, I, bloom, exc is None))


def check_ties(be, k, D=24, I=1500, n_rows=65):
    """Item rows drawn from 5 vectors and 2 biases: hundreds of items share every score, across every k boundary."""
    rng = np.random.RandomState(31)
    U = 80
    vecs, biases = rng.randn(5, D).astype(np.float32), rng.randn(2).astype(np.float32)
    params = random_params(rng, U, I, D)
    params[1] = vecs[rng.randint(0, 5, I)]
    params[3] = biases[rng.randint(0, 2, I)]
    users = rng.randint(0, U, n_rows)
    check_bilinear(be, params, users, k, None, 'ties')
    check_bilinear(be, params, users, k, random_exclusions(rng, n_rows, I, longest=300), 'ties + exclusions')


def check_all_zero(be, k, D=6, I=333, n_rows=33):
    """All-zero tables: every score is +0.0, the answer is the k smallest ids that are not excluded."""
    params = [np.zeros((40, D), np.float32), np.zeros((I, D), np.float32), np.zeros(40, np.float32), np.zeros(I, np.float32)]
    users = np.arange(n_rows) % 40
    exc = [np.arange(0, 2 * (r % 9), 2) for r in range(n_rows)]
    dev = be.model(params)
    items, scores = bilinear_topk(be, dev, users, k, exc)
    for r in range(n_rows):
        want = np.setdiff1d(np.arange(I), exc[r])[:k]
        assert np.array_equal(items[r], want), (r, items[r], want)
    assert np.all(scores == 0)
    assert np.array_equal(bilinear_topk(be, dev, users, k)[0], np.tile(np.arange(k), (n_rows, 1)))


def check_signed_zero_pair(be, D=6, I=40):
    """Item 9 scores -0.0 (every product of its chain underflows to -0, every bias is -0.0), item 4 scores +0.0, everything
    else is negative: the two zeros tie and the smaller id wins."""
    params = [np.zeros((3, D), np.float32), np.zeros((I, D), np.float32), np.full(3, -0.0, np.float32), np.full(I, -1.0, np.float32)]
    params[0][:] = 1e-30
    params[1][9] = -1e-30
    params[3][9] = -0.0
    params[3][4] = 0.0
    dev = be.model(params)
    rows = bilinear_scores(be, dev, [0, 1, 2])
    assert np.all(np.signbit(rows[:, 9])) and np.all(rows[:, 9] == 0) and not np.any(np.signbit(rows[:, 4])) and np.all(rows[:, 4] == 0)
    for k in (1, 2, 10):
        items, scores = bilinear_topk(be, dev, [0, 1, 2], k)
        assert np.array_equal(items[:, :2], np.tile([4, 9], (3, 1))[:, :k]), items
        assert_same((items, scores), host_topk(rows, None, k), 'signed zeros')


def worst_case_params(I, D, descending, U=7):
    """The representation is a multiple of e_0 and V[i][0] = i (or I - i): the scores ascend (descend) with the id."""
    params = [np.zeros((U, D), np.float32), np.zeros((I, D), np.float32), np.zeros(U, np.float32), np.zeros(I, np.float32)]
    params[0][:, 0] = 1.0 + np.arange(U) % 3
    params[1][:, 0] = (I - np.arange(I)) if descending else np.arange(I)
    return params


def check_worst_case_insertion(be, k, descending, D=24, I=1500, n_rows=33):
    """Ascending scores: EVERY item beats its row's threshold, every block fills the candidate buffer; one workgroup sweeps all
    1500 items ("topk_items_per_wg").  Without and with exclusions (the best items among them)."""
    params = worst_case_params(I, D, descending)
    users = np.arange(n_rows) % 7
    rng = np.random.RandomState(41)
    best = (np.arange(30) if descending else I - 1 - np.arange(30))
    exc = [np.concatenate([best[:r % 31], rng.randint(0, I, 25)]) for r in range(n_rows)]
    with be.engine.options(topk_items_per_wg=1536):
        got = check_bilinear(be, params, users, k, None, ('worst case', descending))
        want0 = (np.arange(k) if descending else I - 1 - np.arange(k))
        assert np.array_equal(got[0], np.tile(want0, (n_rows, 1)))
        check_bilinear(be, params, users, k, exc, ('worst case + exclusions', descending))


def check_chunking_invariance(be, k, D=24, I=1500, n_rows=65):
    """One block per workgroup, two, the automatic cut and one workgroup per row tile: identical arrays."""
    rng = np.random.RandomState(53)
    U = 100
    vecs = rng.randn(40, D).astype(np.float32)
    params = random_params(rng, U, I, D)
    params[1] = vecs[rng.randint(0, 40, I)]  # ties, too: their order must not depend on the chunking either
    params[3][:] = 0.25
    users = rng.randint(0, U, n_rows)
    exc = random_exclusions(rng, n_rows, I)
    dev = be.model(params)
    want = host_topk(bilinear_scores(be, dev, users), exc, k)
    for per in (0, 128, 256, 640, 1536):
        with be.engine.options(topk_items_per_wg=per):
            assert be.engine.get_option('topk_items_per_wg') == per
            assert_same(bilinear_topk(be, dev, users, k, exc), want, ('chunking', per, k))
    assert be.engine.get_option('topk_items_per_wg') == 0


def check_exclusion_cases(be, D=24, I=333, n_rows=65, k=10):
    rng = np.random.RandomState(61)
    U = 100
    params = random_params(rng, U, I, D)
    users = rng.randint(0, U, n_rows)
    dev = be.model(params)
    rows = bilinear_scores(be, dev, users)
    free = host_topk(rows, None, k)
    assert_same(bilinear_topk(be, dev, users, k), free, 'no exclusions')
    # every row's whole unexcluded top k excluded: the next k come up
    exc = [free[0][r] for r in range(n_rows)]
    got = bilinear_topk(be, dev, users, k, exc)
    assert_same(got, host_topk(rows, exc, k), 'top k excluded')
    assert not any(np.intersect1d(got[0][r], exc[r]).size for r in range(n_rows))
    # all but 3 items excluded (other rows: nothing, or all but 3 others): padding
    exc = [np.setdiff1d(np.arange(I), rng.choice(I, 3, replace=False)) if r % 2 == 0 else np.zeros(0, np.int64)
           for r in range(n_rows)]
    got = bilinear_topk(be, dev, users, k, exc)
    assert_same(got, host_topk(rows, exc, k), 'all but 3 excluded')
    assert np.all(got[0][0::2, 3:] == -1) and np.all(np.isneginf(got[1][0::2, 3:])) and np.all(got[0][0::2, :3] >= 0)
    # everything excluded
    exc = [np.arange(I) for _ in range(n_rows)]
    got = bilinear_topk(be, dev, users, k, exc)
    assert np.all(got[0] == -1) and np.all(np.isneginf(got[1]))


def check_k_above_items(be, D=6, I=7, k=10):
    rng = np.random.RandomState(67)
    params = random_params(rng, 50, I, D)
    for n_rows in (1, 33):
        users = rng.randint(0, 50, n_rows)
        got = check_bilinear(be, params, users, k, None, 'k > I')
        assert np.all(got[0][:, I:] == -1) and np.all(np.sort(got[0][:, :I], axis=1) == np.arange(I))
        check_bilinear(be, params, users, k, [np.array([r % I]) for r in range(n_rows)], 'k > I + exclusions')


def check_nan(be, D=24):
    """One item row holds a NaN: that item scores NaN for every user and comes after every number, never ahead of one."""
    rng = np.random.RandomState(71)
    for I, k in ((7, 10), (333, 10), (333, K_MAX)):
        params = random_params(rng, 50, I, D)
        params[1][5, 1] = np.nan
        users = rng.randint(0, 50, 33)
        got = check_bilinear(be, params, users, k, None, ('nan', I, k))
        if k >= I:
            assert np.all(got[0][:, I - 1] == 5) and np.all(np.isnan(got[1][:, I - 1])) and np.all(got[0][:, I:] == -1)
        else:
            assert not np.any(got[0] == 5) and not np.any(np.isnan(got[1]))
        # ... and with every number but two excluded it is third
        exc = [np.setdiff1d(np.arange(I), [2, 5, 6]) for _ in range(33)]
        got = check_bilinear(be, params, users, k, exc, ('nan + exclusions', I, k))
        assert np.all(got[0][:, 2] == 5) and np.all(got[0][:, 3:] == -1)


class _Shard(object):
    def __init__(self, be, params, w, W):
        self.V = be.alloc(np.array(params[1][w::W], order='C'))
        self.bi = be.alloc(np.array(params[3][w::W], order='C'))
        self.n = params[1][w::W].shape[0]
        self.tables = _native.make_tables([None, be.ptr(self.V), None, be.ptr(self.bi)], 0, self.n, params[1].shape[1])


def check_shards(be, D, I, n_rows, k, W):
    """slk_shard_topk over the W cyclic shards (rows w::W), one after the other; the candidates merged by the order on the host
    == slk_bilinear_topk on the whole table == the host expectation."""
    rng = np.random.RandomState(79 + D + I + W)
    U = 120
    params = random_params(rng, U, I, D)
    tied = [i for i in (1, 2, 3, 5, 6) if i < I]  # ties that live on different shards
    params[1][tied] = params[1][tied[0]]
    params[3][tied] = params[3][tied[0]]
    users = rng.randint(0, U, n_rows)
    dev = be.model(params)
    for exc in (None, random_exclusions(rng, n_rows, I)):
        whole = bilinear_topk(be, dev, users, k, exc)
        assert_same(whole, host_topk(bilinear_scores(be, dev, users), exc, k), ('one device', D, I, n_rows, k))
        d_rep = be.alloc(np.array(params[0][users], order='C'))
        d_rbias = be.alloc(np.array(params[2][users], order='C'))
        cand_i, cand_s = [], []
        for w in range(W):
            sh = _Shard(be, params, w, W)
            if sh.n == 0:
                continue
            loc = None if exc is None else [np.unique(x)[np.unique(x) % W == w] // W for x in exc]
            d_eo, d_ei = csr(loc, be)
            d_items = be.alloc(np.full((n_rows, k), -7, dtype=np.int64))
            d_scores = be.alloc(np.full((n_rows, k), 7.5, dtype=np.float32))
            be.engine.shard_topk(sh.tables, be.ptr(d_rep), be.ptr(d_rbias), n_rows, k, be.ptr(d_eo), be.ptr(d_ei), be.ptr(d_items),
                                 be.ptr(d_scores), be.stream)
            li = be.get(d_items).copy()
            assert np.all((li >= -1) & (li < sh.n))
            cand_i.append(np.where(li >= 0, li * W + w, -1))
            cand_s.append(be.get(d_scores).copy())
        ci, cs = np.concatenate(cand_i, axis=1), np.concatenate(cand_s, axis=1)
        merged_i = np.full((n_rows, k), -1, dtype=np.int64)
        merged_s = np.full((n_rows, k), -np.inf, dtype=np.float32)
        for r in range(n_rows):
            live = np.nonzero(ci[r] >= 0)[0]
            s = cs[r][live]
            nan = np.isnan(s)
            o = live[np.lexsort((ci[r][live], -(np.where(nan, np.float32(0), s).astype(np.float64) + 0.0), nan))][:k]
            merged_i[r, :len(o)] = ci[r][o]
            merged_s[r, :len(o)] = cs[r][o]
        assert_same((merged_i, merged_s), whole, ('shards', D, I, n_rows, k, W, exc is None))


def check_profile_survives_refusal(be):
    """A call refused AFTER its profile span has opened (decreasing offsets: the check runs on the device) closes the span: the
    profile stays readable, the refused call counts as a call, and the class's time is a time (at most the wall time around
    the two calls; an end event that was never recorded gives an error on HIP and a meaningless difference on the emulator)."""
    import time
    rng = np.random.RandomState(89)
    U, I, D, k = 3, 8, 4, 2
    dev = be.model(random_params(rng, U, I, D))
    users = np.arange(U, dtype=np.int64)
    d_users = be.alloc(users)
    d_eo, d_ei = be.alloc(np.array([0, 2, 1, 3], dtype=np.int64)), be.alloc(np.arange(3, dtype=np.int64))
    d_items, d_scores = be.alloc(np.zeros((U, k), dtype=np.int64)), be.alloc(np.zeros((U, k), dtype=np.float32))
    be.engine.profile_reset()
    be.engine.profile_enable(True)
    t0 = time.perf_counter()
    try:
        with pytest.raises(_native.SlkError, match='not sorted'):
            be.engine.bilinear_topk(dev.tables, be.ptr(d_users), U, k, be.ptr(d_eo), be.ptr(d_ei), be.ptr(d_items), be.ptr(d_scores),
                                    be.stream)
        got = bilinear_topk(be, dev, users, k)  # (reads the results back: the stream is synchronised)
    finally:
        be.engine.profile_enable(False)
    wall_ms = (time.perf_counter() - t0) * 1e3
    calls, ms = be.engine.profile_read()['score']
    print('score class: %d calls, %.6f ms of %.3f ms wall' % (calls, ms, wall_ms))
    assert calls == 2
    assert 0 <= ms <= wall_ms
    assert_same(got, host_topk(bilinear_scores(be, dev, users), None, k), 'after a refusal under the profile')


def check_refusals(be):
    rng = np.random.RandomState(83)
    U, I, D, n, k = 30, 20, 8, 4, 5
    params = random_params(rng, U, I, D)
    dev = be.model(params)
    seq = be.seq_model([params[1], params[3]])
    d_users = be.alloc(np.arange(n, dtype=np.int64))
    d_seqs = be.alloc(np.ones((n, 3), dtype=np.int64))
    d_rep, d_rbias = be.alloc(params[0][:n]), be.alloc(params[2][:n])
    d_items = be.alloc(np.zeros((n, K_MAX + 1), dtype=np.int64))
    d_scores = be.alloc(np.zeros((n, K_MAX + 1), dtype=np.float32))
    item_side = lambda **kw: _native.make_tables([None, be.ptr(dev.p[1]), None, be.ptr(dev.p[3])], 0, I, D, **kw)
    P = be.ptr

    def all_three(match, k=k, eo=None, ei=None, items=d_items, scores=d_scores):
        with pytest.raises(_native.SlkError, match=match):
            be.engine.bilinear_topk(dev.tables, P(d_users), n, k, P(eo), P(ei), P(items), P(scores), be.stream)
        with pytest.raises(_native.SlkError, match=match):
            be.engine.poolnet_topk(seq.tables, P(d_seqs), n, 3, k, P(eo), P(ei), P(items), P(scores), be.stream)
        with pytest.raises(_native.SlkError, match=match):
            be.engine.shard_topk(item_side(), P(d_rep), P(d_rbias), n, k, P(eo), P(ei), P(items), P(scores), be.stream)

    all_three('at least 1', k=0)
    all_three('at least 1', k=-3)
    all_three('at most SLK_TOPK_K_MAX', k=K_MAX + 1)
    all_three('NULL', items=None)
    all_three('NULL', scores=None)
    all_three('not sorted', eo=be.alloc(np.array([0, 3, 2, 4, 4], dtype=np.int64)), ei=be.alloc(np.arange(8, dtype=np.int64)))
    all_three('not sorted', eo=be.alloc(np.array([-1, 0, 2, 4, 4], dtype=np.int64)), ei=be.alloc(np.arange(8, dtype=np.int64)))
    with pytest.raises(_native.SlkError, match='bloom'):
        be.engine.shard_topk(item_side(item_bloom=_native.make_bloom(I, 2)), P(d_rep), P(d_rbias), n, k, None, None, P(d_items),
                             P(d_scores), be.stream)
    with pytest.raises(_native.SlkError, match='NULL'):
        be.engine.shard_topk(item_side(), None, P(d_rbias), n, k, None, None, P(d_items), P(d_scores), be.stream)
    with pytest.raises(_native.SlkError, match='unknown option or bad value'):
        be.engine.set_option('topk_items_per_wg', -1)
    # ... and the same arguments with a good k are answered
    assert_same(bilinear_topk(be, dev, np.arange(n), k), host_topk(bilinear_scores(be, dev, np.arange(n)), None, k), 'after refusals')
