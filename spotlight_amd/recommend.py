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
