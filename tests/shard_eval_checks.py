"""Shared checks of the sharded evaluation entries (include/spotlight_hip.h: slk_shard_target_scores, slk_shard_rank_counts,
slk_shard_scores), run on the emulator build (tests/test_emu_shard_eval.py) and on the gfx950 library
(tests/test_gpu_shard_eval.py) in ONE process: the item side of a whole table is cut into `W` cyclic shards (rows w::W), every
shard is swept on its own, and the host plays the two collectives (elementwise max of the target scores, sum of the counts).
The result must be the one-device fused ranking's / score rows', bit for bit."""
import numpy as np
import pytest

from engine_checks import f32_chain_dot
from spotlight_amd import _native

WORLDS = (1, 2, 3)
FLT_MAX = np.finfo(np.float32).max


def make_case(D, I, n_rows, U=90, seed=5):
    """Random tables with exact ties (items 5, 6, 7 -- as many of them as exist -- are one row with one bias: at world 2 and 3
    they live on different shards), targets among the ties, targets on their own group's exclusion list, groups with an empty
    list, several rows per group.  As engine_checks.check_fused_ranks builds its case."""
    rng = np.random.RandomState(seed)
    V = rng.randn(I, D).astype(np.float32)
    bi = rng.randn(I).astype(np.float32)
    tied = [i for i in (5, 6, 7) if i < I]
    V[tied] = V[tied[0]]
    bi[tied] = bi[tied[0]]
    params = [rng.randn(U, D).astype(np.float32), V, rng.randn(U).astype(np.float32), bi]
    groups = rng.choice(U, size=40, replace=False).astype(np.int64)
    row_group = np.sort(rng.randint(0, len(groups), n_rows)).astype(np.int64)
    row_target = rng.randint(0, I, n_rows).astype(np.int64)
    k = min(n_rows, 6)
    row_target[:k] = (tied * 6)[:k]
    exc = [np.unique(rng.randint(0, I, rng.randint(0, 30))) if g % 3 else np.zeros(0, np.int64) for g in range(len(groups))]
    for r in range(0, n_rows, 7):  # some targets are excluded themselves
        g = row_group[r]
        if len(exc[g]):
            exc[g] = np.unique(np.append(exc[g], row_target[r]))
    exc_off = np.concatenate([[0], np.cumsum([len(x) for x in exc])]).astype(np.int64)
    exc_items = np.concatenate(exc).astype(np.int64)
    return dict(params=params, groups=groups, row_group=row_group, row_target=row_target, exc=exc, exc_off=exc_off,
                exc_items=exc_items)


class _Shard(object):
    """Shard w of W of the item side on the backend's device: tables whose user-side pointers are NULL."""

    def __init__(self, be, params, w, W):
        self.V = be.alloc(np.array(params[1][w::W], order='C'))
        self.bi = be.alloc(np.array(params[3][w::W], order='C'))
        self.n = params[1][w::W].shape[0]
        self.tables = _native.make_tables([None, be.ptr(self.V), None, be.ptr(self.bi)], 0, self.n, params[1].shape[1])


def sharded_ranks(be, case, W, with_exclusions=True):
    """The ranks of the case's rows from W shards, each swept on its own; the host plays the collectives."""
    params, groups = case['params'], case['groups']
    row_group, row_target = case['row_group'], case['row_target']
    n_groups, n_rows = len(groups), len(row_group)
    d_rep = be.alloc(np.array(params[0][groups], order='C'))
    d_rbias = be.alloc(np.array(params[2][groups], order='C'))
    d_rg = be.alloc(row_group)
    shards, lists = [], []
    for w in range(W):
        shards.append(_Shard(be, params, w, W))
        tl = np.where(row_target % W == w, row_target // W, -1).astype(np.int64)
        if with_exclusions:
            here = case['exc_items'] % W == w
            eo = np.concatenate([[0], np.cumsum(here)])[case['exc_off']].astype(np.int64)
            ei = (case['exc_items'][here] // W).astype(np.int64)
            d_eo, d_ei = be.alloc(eo), be.alloc(ei if len(ei) else np.zeros(1, np.int64))
        else:
            d_eo = d_ei = None
        lists.append((be.alloc(tl), d_eo, d_ei))
    st = np.full(n_rows, -np.inf, dtype=np.float32)
    for sh, (d_tl, d_eo, d_ei) in zip(shards, lists):
        d_st = be.alloc(np.full(n_rows, np.nan, dtype=np.float32))
        be.engine.shard_target_scores(sh.tables, be.ptr(d_rep), be.ptr(d_rbias), n_groups, be.ptr(d_rg), be.ptr(d_tl), n_rows,
                                      be.ptr(d_eo), be.ptr(d_ei), be.ptr(d_st), be.stream)
        got = be.get(d_st)
        owned = row_target % W == shards.index(sh)
        assert np.all(np.isneginf(got[~owned])) and np.all(np.isfinite(got[owned]))
        st = np.maximum(st, got)  # all-reduce MAX
    gt, eq = np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64)
    d_stg = be.alloc(st)
    for sh, (d_tl, d_eo, d_ei) in zip(shards, lists):
        d_gt, d_eq = be.alloc(np.full(n_rows, -7, dtype=np.int64)), be.alloc(np.full(n_rows, -7, dtype=np.int64))
        be.engine.shard_rank_counts(sh.tables, be.ptr(d_rep), be.ptr(d_rbias), n_groups, be.ptr(d_rg), be.ptr(d_stg), n_rows,
                                    be.ptr(d_eo), be.ptr(d_ei), be.ptr(d_gt), be.ptr(d_eq), be.stream)
        gt += be.get(d_gt)  # all-reduce SUM
        eq += be.get(d_eq)
    return gt.astype(np.float64) + (eq.astype(np.float64) + 1.0) * 0.5


def expected_ranks(case, with_exclusions=True):
    """numpy: average ranks of the f32 chain scores, the group's exclusion list pushed last."""
    params, groups = case['params'], case['groups']
    want = np.zeros(len(case['row_group']))
    scores = {}
    for r, (g, t) in enumerate(zip(case['row_group'], case['row_target'])):
        if g not in scores:
            u = groups[g]
            s = ((f32_chain_dot(params[0][u][None, :], params[1]) + params[2][u]) + params[3]).astype(np.float32)
            if with_exclusions:
                s[case['exc'][g]] = -FLT_MAX
            scores[g] = s
        s = scores[g]
        want[r] = float((s > s[t]).sum()) + (float((s == s[t]).sum()) + 1.0) * 0.5
    return want


def check_shard_ranks(be, D, I, n_rows):
    """gt + (eq + 1) / 2 from 1, 2 and 3 shards == slk_bilinear_rank on the whole table == the numpy expectation, exactly;
    with the exclusion lists and without any."""
    case = make_case(D, I, n_rows)
    dev = be.model(case['params'])
    d_g, d_rg, d_rt = be.alloc(case['groups']), be.alloc(case['row_group']), be.alloc(case['row_target'])
    d_eo, d_ei = be.alloc(case['exc_off']), be.alloc(case['exc_items'])
    for with_exc in (True, False):
        ranks = be.alloc(np.zeros(n_rows, dtype=np.float64))
        be.engine.bilinear_rank(dev.tables, be.ptr(d_g), len(case['groups']), be.ptr(d_rg), be.ptr(d_rt), n_rows,
                                be.ptr(d_eo) if with_exc else None, be.ptr(d_ei) if with_exc else None, be.ptr(ranks), be.stream)
        whole = be.get(ranks).copy()
        want = expected_ranks(case, with_exc)
        assert np.array_equal(whole, want), (D, I, n_rows, with_exc)
        for W in WORLDS:
            got = sharded_ranks(be, case, W, with_exc)
            assert np.array_equal(got, whole), (D, I, n_rows, W, with_exc, np.nonzero(got != whole)[0][:8])


def check_shard_scores(be, D, I, rows=(1, 2, 8, 9)):
    """slk_shard_scores of every shard, interleaved (out[:, w::W] = shard w), == slk_bilinear_scores on the whole table: the
    streaming form (<= 8 rows of a plain table with dim % 4 == 0) and the matrix-core sweep."""
    case = make_case(D, I, 1)
    params = case['params']
    dev = be.model(params)
    for n in rows:
        users = case['groups'][:n]
        d_users = be.alloc(users)
        whole = be.alloc(np.full((n, I), np.nan, dtype=np.float32))
        be.engine.bilinear_scores(dev.tables, be.ptr(d_users), n, be.ptr(whole), be.stream)
        whole = be.get(whole).copy()
        want = np.stack([((f32_chain_dot(params[0][u][None, :], params[1]) + params[2][u]) + params[3]).astype(np.float32)
                         for u in users])
        assert np.array_equal(whole, want), (D, I, n)
        d_rep = be.alloc(np.array(params[0][users], order='C'))
        d_rbias = be.alloc(np.array(params[2][users], order='C'))
        for W in WORLDS:
            got = np.full((n, I), np.nan, dtype=np.float32)
            for w in range(W):
                sh = _Shard(be, params, w, W)
                d_out = be.alloc(np.full((n, sh.n), np.nan, dtype=np.float32))
                be.engine.shard_scores(sh.tables, be.ptr(d_rep), be.ptr(d_rbias), n, be.ptr(d_out), be.stream)
                got[:, w::W] = be.get(d_out)
            assert np.array_equal(got, whole), (D, I, n, W)


def check_shard_eval_refusals(be):
    """A bloom item table, NULL representations and item biases inside a bias-shadow scope are refused by all three entries."""
    rs = np.random.RandomState(3)
    U, I, D, n = 30, 20, 8, 4
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), np.zeros(U), rs.normal(0, 0.1, I)]
    dev = be.model(params, opt='adagrad', lr=0.05)
    item_side = lambda **kw: _native.make_tables([None, be.ptr(dev.p[1]), None, be.ptr(dev.p[3])], 0, I, D, **kw)
    d_rep = be.alloc(np.asarray(params[0][:n], dtype=np.float32))
    d_rbias = be.alloc(np.zeros(n, dtype=np.float32))
    d_rg = be.alloc(np.arange(n, dtype=np.int64))
    d_tl = be.alloc(np.arange(n, dtype=np.int64))
    d_st = be.alloc(np.zeros(n, dtype=np.float32))
    d_gt, d_eq = be.alloc(np.zeros(n, dtype=np.int64)), be.alloc(np.zeros(n, dtype=np.int64))
    d_out = be.alloc(np.zeros((n, I), dtype=np.float32))

    def all_three(tables, rep, rbias, match):
        with pytest.raises(_native.SlkError, match=match):
            be.engine.shard_target_scores(tables, rep, rbias, n, be.ptr(d_rg), be.ptr(d_tl), n, None, None, be.ptr(d_st), be.stream)
        with pytest.raises(_native.SlkError, match=match):
            be.engine.shard_rank_counts(tables, rep, rbias, n, be.ptr(d_rg), be.ptr(d_st), n, None, None, be.ptr(d_gt),
                                        be.ptr(d_eq), be.stream)
        with pytest.raises(_native.SlkError, match=match):
            be.engine.shard_scores(tables, rep, rbias, n, be.ptr(d_out), be.stream)

    all_three(item_side(item_bloom=_native.make_bloom(I, 2)), be.ptr(d_rep), be.ptr(d_rbias), 'bloom')
    all_three(item_side(), None, be.ptr(d_rbias), 'NULL')
    all_three(item_side(), be.ptr(d_rep), None, 'NULL')
    with be.engine.bias_shadow(dev.tables, dev.optim, stream=be.stream):
        all_three(item_side(), be.ptr(d_rep), be.ptr(d_rbias), 'shadowed')
    # ... and answered outside the scope
    be.engine.shard_scores(item_side(), be.ptr(d_rep), be.ptr(d_rbias), n, be.ptr(d_out), be.stream)
    want = ((f32_chain_dot(be.get(d_rep)[:, None, :], be.get(dev.p[1])[None, :, :]) + 0.0) + be.get(dev.p[3])[None, :]).astype(np.float32)
    assert np.array_equal(be.get(d_out), want)
