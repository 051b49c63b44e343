"""Shared checks of the scoring sweep where ONE WORKGROUP SWEEPS SEVERAL ITEM BLOCKS (csrc/slk_eval.hip: k_score_gemm in its
WRITE and COUNT modes, k_score_rows), run on the emulator build (tests/test_emu_sweep.py) and on the gfx950 library
(tests/test_gpu_sweep.py).

How many blocks a workgroup sweeps is cut by eval_gemm from the device's CU count; on a large device every small table ends up
with one block per workgroup, and the block loop, the register prefetch across blocks, the re-staging of the representations
at dim > 64 and the ragged last chunk never run.  Option "eval_items_per_wg" fixes the cut, so the same small table is swept
as one block per workgroup, two, five, all of it by one workgroup, and as the device would cut it.

Every expected value is formed on the host and compared EXACTLY (no tolerance anywhere):
  score   engine_checks.f32_chain_dot, then (dot + bu) + bi (BilinearNet) or bi + dot (PoolNet);
  PoolNet representation: the L item vectors summed in sequence order in float32, one float32 division by (non-zero count + 1);
  rank    #{s > t} + (#{s == t} + 1) / 2 after the group's excluded items (the target too, if listed) are set to -FLT_MAX.
Rows are drawn from at most 16 distinct users / sequences and the expectation is formed once per distinct one."""
import numpy as np
import pytest

import shard_eval_checks as sec
import topk_checks as tc
from engine_checks import f32_chain_dot
from spotlight_amd import _native

DS = (6, 24, 72, 128)      # scalar loader; vec4 with the operand in registers; two depth chunks, the second partial; two full ones
ITEMS = 1500               # 11.7 blocks of 128: a ragged end under every cut
PERS = (0, 128, 256, 640, 1536)  # the automatic cut, one block per workgroup, two, five, one workgroup per row tile
WRITE_ROWS = (1, 5, 9, 33, 65, 150)  # k_score_rows (dim % 4 == 0) x 2, a 32-row tile x 2, a 64-row tile, three tiles (one partial)
COUNT_ROWS = (1, 33, 65, 150)
TIES = ((126, 127, 128, 129), (1279, 1280))  # items that share one row and one bias: across a block edge and across 640 | 640
N_DISTINCT = 16
SEQ_LEN = 5
FLT_MAX = np.finfo(np.float32).max
OPTION = 'eval_items_per_wg'

_cases = {}  # (kind, D, I) -> the tables and the host expectation, formed once and never written again


def frozen(a):
    a.setflags(write=False)
    return a


def bilinear_host_scores(rep, rbias, V, bi):
    """[n, I] float32: (chain(rep_r, V_i) + rbias_r) + bi_i."""
    dot = f32_chain_dot(rep[:, None, :], V[None, :, :])
    return ((dot + rbias[:, None]).astype(np.float32) + bi[None, :]).astype(np.float32)


def poolnet_host_scores(rep, V, bi):
    """[n, I] float32: bi_i + chain(rep_r, V_i)."""
    return (bi[None, :] + f32_chain_dot(rep[:, None, :], V[None, :, :])).astype(np.float32)


def bloom_rows(T, desc, ids):
    """BloomEmbedding on the host: the hashed rows of every id summed in hash order, in float32 (slk_emb_vec)."""
    from oracle.oracle import bloom_indices
    idx = bloom_indices(np.asarray(ids, dtype=np.int64), desc['seeds'], T.shape[0], desc['padding_idx'])
    e = T[idx[:, 0]].astype(np.float32)
    for h in range(1, idx.shape[1]):
        e = (e + T[idx[:, h]]).astype(np.float32)
    return e


def pool_representation(E, seqs):
    """k_eval_seq_rows on the host: float32 sum in sequence order / (per-dimension non-zero count + 1)."""
    S = np.zeros((seqs.shape[0], E.shape[1]), np.float32)
    C = np.zeros_like(S)
    for t in range(seqs.shape[1]):
        e = E[seqs[:, t]]
        S = (S + e).astype(np.float32)
        C = (C + (e != 0)).astype(np.float32)
    return (S / (C + np.float32(1))).astype(np.float32)


def tie_items(V, bi, I):
    for group in TIES:
        g = [i for i in group if i < I]
        if g:
            V[g] = V[g[0]]
            bi[g] = bi[g[0]]


def bilinear_case(D, I=ITEMS, item_bloom=False, user_bloom=False, seed=7):
    """Tables, 16 distinct users and their score rows on the host."""
    key = ('bilinear', D, I, item_bloom, user_bloom)
    if key not in _cases:
        from oracle.oracle import bloom_desc
        rng = np.random.RandomState(seed + D)
        U = 60
        ud = bloom_desc(n_hash=2) if user_bloom else None
        idesc = bloom_desc(n_hash=4) if item_bloom else None
        Ut = rng.randn(int(0.5 * U) if ud else U, D).astype(np.float32)
        Vt = rng.randn(int(0.4 * I) if idesc else I, D).astype(np.float32)
        bu, bi = rng.randn(U).astype(np.float32), rng.randn(I).astype(np.float32)
        if not idesc:
            tie_items(Vt, bi, I)
        else:
            for group in TIES:  # (a hashed table ties by chance only: the biases at least)
                bi[list(group)] = bi[group[0]]
        pool = rng.choice(np.arange(1, U), N_DISTINCT, replace=False).astype(np.int64)
        rep = bloom_rows(Ut, ud, pool) if ud else Ut[pool]
        V = bloom_rows(Vt, idesc, np.arange(I)) if idesc else Vt
        want = bilinear_host_scores(rep, bu[pool], V, bi)
        _cases[key] = dict(params=[frozen(Ut), frozen(Vt), frozen(bu), frozen(bi)], pool=frozen(pool), want=frozen(want),
                           kw=dict(user_bloom=ud, item_bloom=idesc), I=I, D=D)
    return _cases[key]


def poolnet_case(D, I=ITEMS, seed=11):
    """PoolNet tables, 16 distinct sequences of SEQ_LEN items (padding among them) and their score rows on the host."""
    key = ('poolnet', D, I)
    if key not in _cases:
        rng = np.random.RandomState(seed + D)
        E = rng.randn(I, D).astype(np.float32)
        bi = rng.randn(I).astype(np.float32)
        tie_items(E, bi, I)
        E[0] = 0.0  # the padding row: it does not count in the mean's denominator
        seqs = rng.randint(1, I, (N_DISTINCT, SEQ_LEN)).astype(np.int64)
        seqs[::3, 0] = 0
        seqs[5, :] = 0  # nothing but padding: the representation is zero, every score is the item's bias
        want = poolnet_host_scores(pool_representation(E, seqs), E, bi)
        _cases[key] = dict(params=[frozen(E), frozen(bi)], seqs=frozen(seqs), want=frozen(want), I=I, D=D)
    return _cases[key]


def assert_rows(got, want, what):
    """got [n + 1, I] with a guard row that must still be NaN; want [n, I]."""
    n = want.shape[0]
    assert np.all(np.isnan(got[n])), (what, 'the guard row behind the output was written')
    if not np.array_equal(got[:n], want):
        bad = np.argwhere(got[:n] != want)
        assert False, (what, 'first of %d wrong scores at (row, item)' % len(bad), bad[:6].tolist(),
                       got[:n][tuple(bad[0])], want[tuple(bad[0])])


def under_every_cut(be, pers, run):
    for per in pers:
        with be.engine.options(**{OPTION: per}):
            assert be.engine.get_option(OPTION) == per
            run(per)
    assert be.engine.get_option(OPTION) == 0


# ---- a. WRITE ---------------------------------------------------------------------------------------------------------------

def check_write(be, D, n_rows, pers=PERS, item_bloom=False, user_bloom=False, I=ITEMS):
    """slk_bilinear_scores under every cut == the host chain, element for element; nothing behind the output is written."""
    case = bilinear_case(D, I, item_bloom, user_bloom)
    rng = np.random.RandomState(100 + n_rows)
    pick = rng.randint(0, N_DISTINCT, n_rows)
    dev = be.model(case['params'], **case['kw'])
    d_users = be.alloc(case['pool'][pick])
    want = case['want'][pick]

    def run(per):
        out = be.alloc(np.full((n_rows + 1, I), np.nan, dtype=np.float32))
        be.engine.bilinear_scores(dev.tables, be.ptr(d_users), n_rows, be.ptr(out), be.stream)
        assert_rows(be.get(out), want, ('bilinear_scores', D, n_rows, per, item_bloom, user_bloom))

    under_every_cut(be, pers, run)


def check_predict_all(be, D, pers=PERS, I=ITEMS):
    """slk_bilinear_predict(user, items = NULL): one row against every item."""
    case = bilinear_case(D, I)
    dev = be.model(case['params'])
    for j in (0, N_DISTINCT - 1):
        d_u = be.alloc(case['pool'][j:j + 1])

        def run(per):
            out = be.alloc(np.full((2, I), np.nan, dtype=np.float32))
            be.engine.bilinear_predict(dev.tables, be.ptr(d_u), 1, None, I, be.ptr(out), be.stream)
            assert_rows(be.get(out), case['want'][j:j + 1], ('bilinear_predict', D, per))

        under_every_cut(be, pers, run)


def check_poolnet_write(be, D, n_rows, pers=PERS, I=ITEMS):
    case = poolnet_case(D, I)
    rng = np.random.RandomState(200 + n_rows)
    pick = rng.randint(0, N_DISTINCT, n_rows)
    dev = be.seq_model(case['params'])
    d_seqs = be.alloc(case['seqs'][pick])
    want = case['want'][pick]

    def run(per):
        out = be.alloc(np.full((n_rows + 1, I), np.nan, dtype=np.float32))
        be.engine.poolnet_scores(dev.tables, be.ptr(d_seqs), n_rows, SEQ_LEN, be.ptr(out), be.stream)
        assert_rows(be.get(out), want, ('poolnet_scores', D, n_rows, per))

    under_every_cut(be, pers, run)


# ---- b. COUNT ---------------------------------------------------------------------------------------------------------------

def rank_rows(rng, I, n_rows, n_groups=N_DISTINCT, ties=TIES):
    """Rows, targets and exclusion lists as engine_checks.check_fused_ranks builds them: several rows per group, groups with
    and without a list, targets among the tied items, some targets on their own group's list, tied items on some lists."""
    row_group = np.sort(rng.randint(0, n_groups, n_rows)).astype(np.int64)
    row_target = rng.randint(0, I, n_rows).astype(np.int64)
    tied = [i for group in ties for i in group]
    k = min(n_rows, len(tied))
    row_target[:k] = tied[:k]
    exc = []
    for g in range(n_groups):
        if g % 3 == 0:
            exc.append(np.zeros(0, np.int64))
            continue
        x = rng.randint(0, I, rng.randint(1, 30))
        if g % 3 == 1:
            x = np.append(x, [ties[0][1], ties[-1][-1]])  # part of a tie pushed last
        exc.append(np.unique(x).astype(np.int64))
    for r in range(0, n_rows, 7):  # some targets are excluded themselves
        g = row_group[r]
        if len(exc[g]):
            exc[g] = np.unique(np.append(exc[g], row_target[r]))
    exc_off = np.concatenate([[0], np.cumsum([len(x) for x in exc])]).astype(np.int64)
    return row_group, row_target, exc, exc_off, np.concatenate(exc).astype(np.int64)


def host_ranks(scores, row_group, row_target, exc):
    """scores [groups, I]; exc: the groups' lists, or None."""
    pushed = {}
    want = np.zeros(len(row_group))
    for r, (g, t) in enumerate(zip(row_group, row_target)):
        if g not in pushed:
            s = scores[g].copy()
            if exc is not None:
                s[exc[g]] = -FLT_MAX
            pushed[g] = s
        s = pushed[g]
        want[r] = float((s > s[t]).sum()) + (float((s == s[t]).sum()) + 1.0) * 0.5
    return want


def _check_ranks(be, call, scores, I, n_rows, pers, what, seed, tied=True):
    rng = np.random.RandomState(seed + n_rows)
    row_group, row_target, exc, exc_off, exc_items = rank_rows(rng, I, n_rows)
    d_rg, d_rt, d_eo, d_ei = be.alloc(row_group), be.alloc(row_target), be.alloc(exc_off), be.alloc(exc_items)
    want = {True: host_ranks(scores, row_group, row_target, exc), False: host_ranks(scores, row_group, row_target, None)}
    if tied:  # the first rows' targets are the tied items (four and two of a kind): an even tie's average rank ends in .5
        assert np.all(want[False][:min(n_rows, 6)] % 1.0 == 0.5)
    seen = {True: [], False: []}

    def run(per):
        for with_exc in (True, False):
            ranks = be.alloc(np.full(n_rows, np.nan, dtype=np.float64))
            call(be.ptr(d_rg), be.ptr(d_rt), n_rows, be.ptr(d_eo) if with_exc else None, be.ptr(d_ei) if with_exc else None,
                 be.ptr(ranks))
            got = be.get(ranks).copy()
            bad = np.nonzero(got != want[with_exc])[0]
            assert bad.size == 0, (what, n_rows, per, with_exc, 'rows', bad[:8].tolist(), got[bad[:8]], want[with_exc][bad[:8]])
            seen[with_exc].append(got)

    under_every_cut(be, pers, run)
    for with_exc in (True, False):
        assert all(np.array_equal(x, seen[with_exc][0]) for x in seen[with_exc])


def check_bilinear_ranks(be, D, n_rows, pers=PERS, item_bloom=False, I=ITEMS):
    case = bilinear_case(D, I, item_bloom)
    dev = be.model(case['params'], **case['kw'])
    d_g = be.alloc(case['pool'])

    def call(rg, rt, n, eo, ei, out):
        be.engine.bilinear_rank(dev.tables, be.ptr(d_g), N_DISTINCT, rg, rt, n, eo, ei, out, be.stream)

    _check_ranks(be, call, case['want'], I, n_rows, pers, ('bilinear_rank', D, item_bloom), 300, tied=not item_bloom)


def check_poolnet_ranks(be, D, n_rows, pers=PERS, I=ITEMS):
    case = poolnet_case(D, I)
    dev = be.seq_model(case['params'])
    d_g = be.alloc(case['seqs'])

    def call(rg, rt, n, eo, ei, out):
        be.engine.poolnet_rank(dev.tables, be.ptr(d_g), N_DISTINCT, SEQ_LEN, rg, rt, n, eo, ei, out, be.stream)

    _check_ranks(be, call, case['want'], I, n_rows, pers, ('poolnet_rank', D), 400)


# ---- c. the sharded entries share eval_gemm ---------------------------------------------------------------------------------

def check_shard_entries(be, D=72, I=ITEMS, n_rows=65, W=2, pers=(0, 256)):
    """slk_shard_rank_counts / slk_shard_scores of W cyclic shards under a fixed cut == the one-device results (== the host)."""
    case = sec.make_case(D, I, n_rows)
    params = case['params']
    dev = be.model(params)
    d_g, d_rg, d_rt = be.alloc(case['groups']), be.alloc(case['row_group']), be.alloc(case['row_target'])
    d_eo, d_ei = be.alloc(case['exc_off']), be.alloc(case['exc_items'])
    whole = {}
    for with_exc in (True, False):
        ranks = be.alloc(np.full(n_rows, np.nan, dtype=np.float64))
        be.engine.bilinear_rank(dev.tables, be.ptr(d_g), len(case['groups']), be.ptr(d_rg), be.ptr(d_rt), n_rows,
                                be.ptr(d_eo) if with_exc else None, be.ptr(d_ei) if with_exc else None, be.ptr(ranks), be.stream)
        whole[with_exc] = be.get(ranks).copy()
        assert np.array_equal(whole[with_exc], sec.expected_ranks(case, with_exc)), ('one device', with_exc)
    users = case['groups'][np.arange(n_rows) % len(case['groups'])]
    d_users = be.alloc(users)
    rows = be.alloc(np.full((n_rows + 1, I), np.nan, dtype=np.float32))
    be.engine.bilinear_scores(dev.tables, be.ptr(d_users), n_rows, be.ptr(rows), be.stream)
    rows = be.get(rows).copy()
    assert_rows(rows, bilinear_host_scores(params[0][users], params[2][users], params[1], params[3]), 'one device')
    d_rep = be.alloc(np.array(params[0][users], order='C'))
    d_rbias = be.alloc(np.array(params[2][users], order='C'))

    def run(per):
        for with_exc in (True, False):
            got = sec.sharded_ranks(be, case, W, with_exc)
            assert np.array_equal(got, whole[with_exc]), ('shard_rank_counts', per, with_exc, np.nonzero(got != whole[with_exc])[0][:8])
        got = np.full((n_rows, I), np.nan, dtype=np.float32)
        for w in range(W):
            sh = sec._Shard(be, params, w, W)
            d_out = be.alloc(np.full((n_rows + 1, sh.n), np.nan, dtype=np.float32))
            be.engine.shard_scores(sh.tables, be.ptr(d_rep), be.ptr(d_rbias), n_rows, be.ptr(d_out), be.stream)
            out = be.get(d_out)
            assert np.all(np.isnan(out[n_rows])), ('shard_scores', per, w, 'guard row')
            got[:, w::W] = out[:n_rows]
        assert np.array_equal(got, rows[:n_rows]), ('shard_scores', per)

    under_every_cut(be, pers, run)


# ---- d. the option itself ---------------------------------------------------------------------------------------------------

def check_option(be, D=24, I=333, n_rows=33, k=10):
    eng = be.engine
    assert eng.get_option(OPTION) == 0
    for v in (1, 128, 1000, 1 << 40):
        with eng.options(**{OPTION: v}):
            assert eng.get_option(OPTION) == v
        assert eng.get_option(OPTION) == 0
    for v in (-1, (1 << 40) + 1):
        with pytest.raises(_native.SlkError, match='unknown option or bad value'):
            eng.set_option(OPTION, v)
        assert eng.get_option(OPTION) == 0
    # the selecting sweep keeps its own option: top-k under a fixed evaluation cut == the order of the host's score rows
    case = bilinear_case(D, I)
    dev = be.model(case['params'])
    rng = np.random.RandomState(500)
    pick = rng.randint(0, N_DISTINCT, n_rows)
    exc = tc.random_exclusions(rng, n_rows, I)
    want = tc.host_topk(case['want'][pick], exc, k)
    free = tc.bilinear_topk(be, dev, case['pool'][pick], k, exc)
    tc.assert_same(free, want, 'top-k, automatic cut')
    with eng.options(**{OPTION: 128}):
        assert eng.get_option('topk_items_per_wg') == 0
        tc.assert_same(tc.bilinear_topk(be, dev, case['pool'][pick], k, exc), want, 'top-k under eval_items_per_wg')


# ---- e. the automatic cut at the device's own size (GPU only) ----------------------------------------------------------------

def gemm_cut(I, n_rows, num_cus):
    """eval_gemm's own formula for k_score_gemm: (items per workgroup, row tiles)."""
    mt = 2 if n_rows > 32 else 1
    row_tiles = (n_rows + 32 * mt - 1) // (32 * mt)
    want = max(1, ((2 if row_tiles == 1 else 4) * num_cus + row_tiles - 1) // row_tiles)
    per = (I + want - 1) // want
    per = (per + 127) // 128 * 128
    return min(per, 1 << 22), want


def rows_cut(I, num_cus):
    """... and for k_score_rows."""
    per = (I + 2 * num_cus - 1) // (2 * num_cus)
    return (per + 255) // 256 * 256


def check_device_cut_gemm(be, num_cus, R=1024, D=72):
    """Option left at 0: R = 1024 rows (16 tiles of 64) and a table sized from the CU count so that the device's own cut makes
    every workgroup sweep three blocks, the last chunk ragged (256 CUs: 20 000 items, 384 per workgroup, 32 in the last)."""
    assert be.engine.get_option(OPTION) == 0
    want_wgs = (4 * num_cus + R // 64 - 1) // (R // 64)
    I = 384 * ((want_wgs * 13) // 16) + 32
    per, _ = gemm_cut(I, R, num_cus)
    assert per >= 3 * 128, ('the device cuts %d items into workgroups of %d: fewer than 3 blocks each' % (I, per), num_cus)
    assert I % per != 0 and (I % per) % 128 != 0, ('the last chunk is not ragged', I, per, num_cus)
    ties = ((per - 2, per - 1, per, per + 1), (127, 128))  # across a workgroup's edge and across a block's
    key = ('device cut', D, I)
    if key not in _cases:
        rng = np.random.RandomState(13)
        U = 60
        Ut, Vt = rng.randn(U, D).astype(np.float32), rng.randn(I, D).astype(np.float32)
        bu, bi = rng.randn(U).astype(np.float32), rng.randn(I).astype(np.float32)
        for group in ties:
            Vt[list(group)] = Vt[group[0]]
            bi[list(group)] = bi[group[0]]
        pool = rng.choice(U, N_DISTINCT, replace=False).astype(np.int64)
        _cases[key] = dict(params=[frozen(Ut), frozen(Vt), frozen(bu), frozen(bi)], pool=frozen(pool),
                           want=frozen(bilinear_host_scores(Ut[pool], bu[pool], Vt, bi)))
    case = _cases[key]
    dev = be.model(case['params'])
    rng = np.random.RandomState(17)
    # ranks
    row_group, row_target, exc, exc_off, exc_items = rank_rows(rng, I, R, ties=ties)
    d_g, d_rg, d_rt, d_eo, d_ei = (be.alloc(x) for x in (case['pool'], row_group, row_target, exc_off, exc_items))
    for with_exc in (True, False):
        ranks = be.alloc(np.full(R, np.nan, dtype=np.float64))
        be.engine.bilinear_rank(dev.tables, be.ptr(d_g), N_DISTINCT, be.ptr(d_rg), be.ptr(d_rt), R, be.ptr(d_eo) if with_exc else None,
                                be.ptr(d_ei) if with_exc else None, be.ptr(ranks), be.stream)
        got, want = be.get(ranks), host_ranks(case['want'], row_group, row_target, exc if with_exc else None)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, ('bilinear_rank at the device cut', I, per, with_exc, bad[:8].tolist(), got[bad[:8]], want[bad[:8]])
    # scores: R x I floats, compared per distinct user
    pick = rng.randint(0, N_DISTINCT, R)
    d_users = be.alloc(case['pool'][pick])
    out = be.alloc(np.full((R + 1, I), np.nan, dtype=np.float32))
    be.engine.bilinear_scores(dev.tables, be.ptr(d_users), R, be.ptr(out), be.stream)
    got = be.get(out)
    assert np.all(np.isnan(got[R])), 'the guard row behind the output was written'
    for j in range(N_DISTINCT):
        rows = np.nonzero(pick == j)[0]
        same = got[rows] == case['want'][j][None, :]
        assert same.all(), ('bilinear_scores at the device cut', I, per, 'user', j, 'first wrong (row, item)',
                            rows[np.argwhere(~same)[0][0]], np.argwhere(~same)[0][1], int((~same).sum()))


def check_device_cut_rows(be, num_cus, R=2, D=24):
    """The streaming form under the device's own cut: a table sized so that a k_score_rows workgroup sweeps at least three
    blocks of 256 items (256 CUs: 400 003 items, 1024 per workgroup)."""
    assert be.engine.get_option(OPTION) == 0
    I = 2 * num_cus * 781 + 131
    per = rows_cut(I, num_cus)
    assert per >= 3 * 256 and I % 256 != 0, ('the device cuts %d items into workgroups of %d' % (I, per), num_cus)
    rng = np.random.RandomState(19)
    U = 5
    params = [rng.randn(U, D).astype(np.float32), rng.randn(I, D).astype(np.float32), rng.randn(U).astype(np.float32),
              rng.randn(I).astype(np.float32)]
    d_p = [be.alloc(x) for x in params]
    tables = _native.make_tables([be.ptr(x) for x in d_p], U, I, D)
    users = np.array([3, 1], dtype=np.int64)[:R]
    d_users = be.alloc(users)
    out = be.alloc(np.full((R + 1, I), np.nan, dtype=np.float32))
    be.engine.bilinear_scores(tables, be.ptr(d_users), R, be.ptr(out), be.stream)
    assert_rows(be.get(out), bilinear_host_scores(params[0][users], params[2][users], params[1], params[3]),
                ('bilinear_scores, streaming form at the device cut', I, per))


# ---- f. capacity of the packed per-lane counters (GPU only) -------------------------------------------------------------------

def check_counter_capacity(be, I=(1 << 23) + 1000, D=4):
    """COUNT keeps (#equal << 16) | #greater per lane and accumulator element; a lane sees one column per 128 items, so a
    workgroup may sweep at most 2^23 items, and eval_gemm clamps the cut to 2^22.  V[i][0] = i and representations e_0, 2 e_0
    and 0: every product is exact, the scores of users 0 and 1 ascend strictly with the id (rank of target t: I - t), user 2's
    all tie at +0.0 (rank (I + 1) / 2).  Under the largest cut the option admits, a lane of an UNclamped workgroup would count
    65 544 greater items for target 0 (a carry into #equal) and 65 544 equal ones for user 2 (a carry out of the word)."""
    V = np.zeros((I, D), np.float32)
    V[:, 0] = np.arange(I, dtype=np.float32)
    assert V[-1, 0] == I - 1 and V[-2, 0] == I - 2
    Ut = np.zeros((3, D), np.float32)
    Ut[0, 0], Ut[1, 0] = 1.0, 2.0
    d_p = [be.alloc(Ut), be.alloc(V), be.alloc(np.zeros(3, np.float32)), be.alloc(np.zeros(I, np.float32))]
    del V
    tables = _native.make_tables([be.ptr(x) for x in d_p], 3, I, D)
    targets = np.array([0, I - 1, (1 << 22) + 77], dtype=np.int64)
    row_group = np.repeat(np.arange(3, dtype=np.int64), len(targets))
    row_target = np.tile(targets, 3)
    want = np.where(row_group < 2, (I - row_target).astype(np.float64), (I + 1) / 2.0)
    d_g, d_rg, d_rt = be.alloc(np.arange(3, dtype=np.int64)), be.alloc(row_group), be.alloc(row_target)
    n = len(row_group)

    def run(per):
        ranks = be.alloc(np.full(n, np.nan, dtype=np.float64))
        be.engine.bilinear_rank(tables, be.ptr(d_g), 3, be.ptr(d_rg), be.ptr(d_rt), n, None, None, be.ptr(ranks), be.stream)
        got = be.get(ranks)
        assert np.array_equal(got, want), ('eval_items_per_wg', per, 'ranks', got.tolist(), 'expected', want.tolist())

    under_every_cut(be, (0, 1 << 40), run)
