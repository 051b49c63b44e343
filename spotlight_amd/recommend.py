"""recommend(): the k best items per user / sequence -- the pieces the models share.

THE ORDER (include/spotlight_hip.h): score descending (-0.0 == +0.0), ties to the smaller item id, a NaN score after every
number; an excluded item never appears; a row with fewer than k eligible items ends in item -1 / score -inf.  The fused route
(slk_*_topk) selects inside the scoring sweep and never forms a score row; the generic route below sorts score rows a tile
at a time and serves what the fused route does not: custom representation modules, models without a fused sweep and
k > TOPK_K_MAX.  It is also what the tests compare the fused route with.
"""
import numpy as np

from spotlight_amd._native import TOPK_K_MAX, merge_topk, topk_order  # noqa: F401  (re-exported)

_SCORE_BYTES = 256 << 20  # one tile of score rows of the generic route (as evaluation.py's)


def check_k(k):
    if int(k) != k or int(k) < 1:
        raise ValueError('k must be an integer >= 1, got {!r}'.format(k))
    return int(k)


def exclusion_lists(exclude, keys, num_items):
    """Per key the sorted, distinct item ids to hide, or None.  `exclude`: None, an Interactions / scipy sparse matrix whose row
    u holds user u's items (keys are then user ids), or one index array per key."""
    if exclude is None:
        return None
    if hasattr(exclude, 'tocsr'):
        m = exclude.tocsr()
        empty = np.zeros(0, np.int64)
        lists = [np.unique(m.indices[m.indptr[u]:m.indptr[u + 1]]).astype(np.int64) if u < m.shape[0] else empty
                 for u in np.asarray(keys).reshape(-1)]
    else:
        if len(exclude) != len(keys):
            raise ValueError('exclude holds {} lists for {} rows'.format(len(exclude), len(keys)))
        lists = [np.unique(np.asarray(x).reshape(-1).astype(np.int64)) for x in exclude]
    for x in lists:
        if x.size and (x[0] < 0 or x[-1] >= num_items):
            raise IndexError('index {} is out of bounds for axis 0 with size {}'.format(int(x[-1] if x[0] >= 0 else x[0]), num_items))
    return lists


def csr_of(lists):
    """(exc_off, exc_items) int64 arrays of per-row lists; exc_items never empty (it is uploaded)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    items = np.concatenate(lists).astype(np.int64) if off[-1] else np.zeros(1, np.int64)
    return off, items


def empty_result(k):
    return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)


def generic_topk(score_rows, keys, num_items, k, lists):
    """The generic route: `score_rows(keys[lo:hi])` -> [hi - lo, num_items] float32 host array (row r == predict(keys[r])); the
    excluded entries are made ineligible, the rest is ordered by a STABLE sort on (NaN last, score descending), so equal scores
    keep ascending id."""
    n = len(keys)
    items = np.full((n, k), -1, dtype=np.int64)
    scores = np.full((n, k), -np.inf, dtype=np.float32)
    per_tile = max(1, _SCORE_BYTES // (4 * num_items))
    for lo in range(0, n, per_tile):
        hi = min(lo + per_tile, n)
        rows = np.asarray(score_rows(keys[lo:hi]), dtype=np.float32).reshape(hi - lo, num_items)
        for r in range(lo, hi):
            row = rows[r - lo]
            if lists is not None and lists[r].size:
                cols = np.setdiff1d(np.arange(num_items), lists[r], assume_unique=True)
            else:
                cols = np.arange(num_items)
            o = cols[topk_order(row[cols], cols)][:k]
            items[r, :len(o)] = o
            scores[r, :len(o)] = row[o]
    return items, scores


# ---- similar_items() / similar_users(): neighbours in the embedding space ------------------------------------------------
# (include/spotlight_hip.h: slk_rows_inv_norm, slk_neighbors_topk, slk_neighbors_scores.)  The score of query q against
# table row j is the k-ordered fma chain of the two rows ('dot'), or (chain * 1/|q|) * 1/|j| ('cosine'); order, padding and
# exclusion lists are recommend()'s.  The fused route selects inside the sweep; the generic route sorts score rows a tile at
# a time (k > TOPK_K_MAX, and what the tests compare the fused route with).
METRICS = ('cosine', 'dot')


def check_metric(metric):
    if metric not in METRICS:
        raise ValueError('metric must be one of {}, got {!r}'.format(METRICS, metric))
    return metric


def neighbor_lists(ids, num_rows, exclude_self=True, exclude=None, always=None):
    """Per query the sorted, distinct table rows to hide, or None: the caller's lists (`exclude`: one index array per query),
    the query's own id (`exclude_self`) and the rows hidden from everyone (`always`)."""
    lists = exclusion_lists(exclude, ids, num_rows)
    always = np.zeros(0, np.int64) if always is None else np.asarray(always, dtype=np.int64).reshape(-1)
    if lists is None and not exclude_self and not always.size:
        return None
    if lists is None:
        lists = [np.zeros(0, np.int64)] * len(ids)
    own = (lambda q: [q]) if exclude_self else (lambda q: [])
    return [np.unique(np.concatenate([x, always, np.asarray(own(q), dtype=np.int64)])).astype(np.int64) for x, q in zip(lists, ids)]


def inverse_norms(engine, stream, rows):
    """float32 [n] device tensor: 1 / |row| by the engine's chain (0 for an all-zero row); `rows`: contiguous [n, dim]."""
    import torch
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    engine.rows_inv_norm(rows.data_ptr(), rows.shape[0], rows.shape[1], out.data_ptr(), stream)
    return out


def _ptr(t):
    return t.data_ptr() if t is not None else None


def neighbors_fused(engine, stream, table, tscale, queries, qscale, k, lists):
    """The k best rows of `table` per row of `queries` (device tensors), selected inside the sweep: device tensors
    (items int64 [n, k], scores float32 [n, k]).  k <= TOPK_K_MAX."""
    import torch
    n, device = queries.shape[0], table.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    d_eo, d_ei = [dev(a) for a in csr_of(lists)] if lists is not None else (None, None)
    items = torch.empty((n, k), dtype=torch.int64, device=device)
    scores = torch.empty((n, k), dtype=torch.float32, device=device)
    engine.neighbors_topk(table.data_ptr(), table.shape[0], table.shape[1], _ptr(tscale), queries.data_ptr(), _ptr(qscale), n, k,
                          _ptr(d_eo), _ptr(d_ei), items.data_ptr(), scores.data_ptr(), stream)
    return items, scores


def neighbors_generic(engine, stream, table, tscale, queries, qscale, k, lists):
    """The same result from score rows (slk_neighbors_scores), a tile of queries at a time, ordered on the host."""
    import torch
    n, num_rows = queries.shape[0], table.shape[0]

    def score_rows(idx):
        lo, m = int(idx[0]), len(idx)
        out = torch.empty((m, num_rows), dtype=torch.float32, device=table.device)
        engine.neighbors_scores(table.data_ptr(), num_rows, table.shape[1], _ptr(tscale), queries[lo:lo + m].data_ptr(),
                                _ptr(qscale[lo:lo + m]) if qscale is not None else None, m, out.data_ptr(), stream)
        return out.cpu().numpy()
    return generic_topk(score_rows, np.arange(n), num_rows, k, lists)


def similar_rows(engine, stream, table, ids, k, metric, lists, generic=False):
    """similar_items() / similar_users() over one dense table (a float32 [n, dim] device tensor): the queries are rows `ids` of
    the table itself, gathered on the device; under 'cosine' the table's inverse norms are computed once and the queries'
    factors are entries of that vector.  Host arrays (items, scores)."""
    import torch
    table = table.detach()
    if not table.is_contiguous() or table.dtype != torch.float32:
        raise RuntimeError('the embedding table must be a contiguous fp32 tensor')
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(table.device)
    queries = table.index_select(0, d_ids)
    tscale = qscale = None
    if metric == 'cosine':
        tscale = inverse_norms(engine, stream, table)
        qscale = tscale.index_select(0, d_ids)
    if generic or k > TOPK_K_MAX:
        return neighbors_generic(engine, stream, table, tscale, queries, qscale, k, lists)
    items, scores = neighbors_fused(engine, stream, table, tscale, queries, qscale, k, lists)
    return items.cpu().numpy(), scores.cpu().numpy()
