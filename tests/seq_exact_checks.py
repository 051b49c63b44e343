"""Shared checks of the PoolNet sequence pass (csrc/slk_seq.hip: k_seq_pass / k_seq_pass_reg, and the SLK_ITEM_SEQ item pass of
csrc/slk_kernels.h) and of the prediction side (slk_poolnet_predict / slk_poolnet_scores) against a float64 restatement, per
timestep.  Run on the emulator build (tests/test_emu_seq_exact.py) and on the gfx950 library (tests/test_gpu_seq_exact.py); the
restatement itself is pinned on the CPU in tests/test_host_seq_exact.py (torch.autograd in float64, the live reference's PoolNet
where it exists, PoolNetOracle).

THE REFERENCE is minibatch(..., dtype=np.float64) below on the float32-rounded inputs: plain numpy, the padding-aware running mean
(sequence/representations.py:76-114), the four sequence losses (losses.py, mask = sequence != 0) and the closed-form backward.
THE YARDSTICK of every tolerance is the same function with dtype=np.float32 (sequential float32 cumsums and sums): its worst
error against the float64 result is measured on the test's own inputs, every time the test runs, and the kernel passes at FACTOR
times that figure (floor 2^-22).  The error of an output row is |got - want64|_inf / mag[row], where mag is the float64 sum of the
absolute values of the leaf terms the row is a sum of (largest element), so cancellation inside a row can neither make the bound
unreachable nor make it lax.  Where the restatement's answer is exactly zero (mag == 0: rows never looked up, the padding row and
its bias, an adaptive candidate that was not chosen) the engine's must be exactly zero.

Gradients are read as tests/engine_checks.py reads them: adam_dense, lr = 0, betas = (0, 0.999), so exp_avg after one step is
the gradient; the negatives are handed in (d_neg_in); the parameters must come back bit-unchanged.

Two input families.  ISOLATING: more items than lookups, every real sequence entry and every handed-in negative a distinct id --
every item row then receives exactly ONE term (a negative drawn at (s, t): g_neg(s, t) * rep(s, t), bias g_neg(s, t); the
sequence's item at (s, t): g_pos(s, t) * rep(s, t) + the history gradient of that timestep), so the row-by-row comparison is a
check of every timestep's representation, dL/dscore and history gradient.  SHARED: 4 items, 64 x 64 timesteps at dim 64 -- three
rows that each collect thousands of occurrences (the item pass's per-tile partials + k_item_stitch)."""
import numpy as np

from embed_checks import bloom_of, same_bits
from oracle.oracle import bloom_indices

# The tolerance of every comparison with float64: FACTOR x the float32 restatement's own worst error on the same inputs.
FACTOR = 4.0
FLOOR = 2.0 ** -22
# An input whose float32 yardstick is itself this far from float64 (relative to mag) is ill-chosen: replace the input.
YARD_MAX = 1e-4
# Inputs keep every decision (the adaptive maximum, the hinge's kink) this far from a tie in float64, so that float32 and float64
# take the same branch; exact ties (the same id twice, the deliberate twin rows) are decided by the rule, not by rounding.
# (A float32 score of these inputs is within ~5e-7 of the float64 one; 2e-5 is 40 times that, and small enough that one of the
# first seeds of even the 12 000 timesteps of the grid-stride case on a 256-CU part keeps every decision outside it.)
MARGIN = 2e-5

# What the yardstick and the kernels measured (worst row of a case: item rows / item biases / loss, each relative to its mag;
# recorded for the reader, the tests measure the yardstick again on every run and print both with `pytest -s`):
#   group (worst case of the group)                     yardstick rows / bias / loss     emulator kernels rows / bias / loss
#   scan shapes, 23 (D, L) x bpr, adaptive n = 5 ...... 3.4e-7 / 5.8e-7 / 9.7e-7         3.4e-7 / 5.8e-7 / 5.7e-8
#   the four losses + adaptive n = 1, 4, one term/row . 2.7e-7 / 2.8e-7 / 2.2e-7         2.7e-7 / 2.8e-7 / 3.7e-8
#   shared, 64 x 17, the four losses .................. 3.2e-7 / 2.4e-7 / 5.6e-7         2.6e-8 / 2.8e-8 / 4.6e-8
#   shared, 64 x 64 (4096 timesteps), bpr, pointwise .. 4.6e-7 / 5.6e-7 / 1.5e-7         3.4e-8 / 3.1e-8 / 1.4e-8
#   padding and zeros, plain and bloom ................ 5.2e-7 / 1.0e-6 / 2.0e-7         5.2e-7 / 1.0e-6 / 3.2e-8
#   adaptive tie ...................................... 1.0e-7 / 3.7e-9 / 3.2e-8         1.0e-7 / 3.7e-9 / 5.2e-8
#   grid stride, 35 sequences (2 emulated CUs) ........ 3.1e-7 / 4.7e-7 / 4.6e-7         3.1e-7 / 4.7e-7 / 4.8e-8
#   predict / scores on the padding inputs ............ 1.2e-7                           1.4e-7
# The floor 2^-22 = 2.4e-7 decides about half of the comparisons.  The emulator's kernels are never beyond 0.41 of their
# tolerance; the long runs (per-tile partials, stitched) are ten times closer to float64 than the sequential float32 sums of the
# yardstick, and the loss, accumulated in float64, is rounded once.  The gfx950 column is not recorded yet: run
# `pytest tests/test_gpu_seq_exact.py -m gpu -s` on the device (every case prints its yardstick and kernel figures) and add it here.
# (DESIGN.md 5 quotes the same figures)

LOSSES = ('pointwise', 'bpr', 'hinge', 'adaptive_hinge')

# (D, L) of the scan-shape cases: layout (vec, g) from slk_pick_layout, NG = 256 / g row groups, C = ceil(L / NG) timesteps per
# group; the register-resident form runs up to L = 256 and C = 16 (CMAX = min(g, 16) rows of registers)
SCAN_SHAPES = [(64, 1), (64, 15), (64, 16), (64, 17), (64, 255), (64, 256), (64, 257),   # g 16, NG 16; 257: LDS form only
               (128, 8), (128, 9), (128, 128), (128, 129),                                # g 32, NG 8; C = 17 at 129: LDS form
               (256, 64), (256, 65),                                                      # g 64, NG 4
               (72, 9),                                                                   # g 32 with idle lanes
               (8, 128), (8, 129), (8, 256),                                              # g 2, CMAX 2
               (4, 1), (4, 256), (4, 257),                                                # g 1, CMAX 1
               (6, 33), (6, 256), (3, 65)]                                                # vec 1: g 8, g 4
SCAN_LOSSES = (('bpr', 1), ('adaptive_hinge', 5))
PAD_SHAPES = [(64, 17), (6, 33)]
# adaptive hinge at wide n: the pass indexes its dL/dscore as gsn[(b * L + t) * NP + pair], and everything above stops at NP = 6.
# (D, L) is the grid-stride case's, the smallest shape here that has a running mean (at L = 1 every representation is zero)
WIDE_NS = (7, 64, 200)
WIDE_SHAPE = (8, 3)


def pick_layout(D):
    """slk_pick_layout (csrc/slk_kernels.h)."""
    need = D // 4 if D % 4 == 0 else D
    g = 1
    while g < need:
        g <<= 1
    return (4 if D % 4 == 0 else 1), g


def reg_form_applies(D, L):
    """plan_seq_training: the register-resident pass is taken when L <= 256 and ceil(L / NG) <= 16 (and "seq_variant" != 0)."""
    ng = 256 // pick_layout(D)[1]
    return L <= 256 and (L + ng - 1) // ng <= 16


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def seq_sum(x, axis=-1):
    """Sum along `axis` by sequential accumulation in x's own dtype (np.sum adds pairwise)."""
    return np.take(np.add.accumulate(x, axis=axis), -1, axis=axis)


def excl_cumsum(x, axis=1):
    """Exclusive prefix sum along `axis`, sequential, in x's dtype."""
    out = np.zeros_like(x)
    dst = [slice(None)] * x.ndim
    src = [slice(None)] * x.ndim
    dst[axis], src[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = np.add.accumulate(x[tuple(src)], axis=axis)
    return out


def suffix_sum(x, axis=1):
    """out[t] = sum of x[t'] over t' > t, accumulated from the end, in x's dtype."""
    return np.flip(excl_cumsum(np.flip(x, axis), axis), axis)


def hashed_rows(ids, bloom, rows):
    """[ids.size, n_hash] rows of the compressed table (the hash restatement tests/embed_checks.py uses)."""
    return bloom_indices(np.asarray(ids, np.int64).ravel(), bloom['seeds'], rows, bloom['padding_idx'])


def item_vectors(E, ids, bloom, dtype):
    """(vectors, sum of |leaf rows|) of `ids`: a row of the plain table, or the sum of the n_hash hashed rows in hash order."""
    E = E.astype(dtype)
    ids = np.asarray(ids, np.int64)
    if bloom is None:
        v = E[ids]
        return v, np.abs(v.astype(np.float64))
    idx = hashed_rows(ids, bloom, E.shape[0])
    v = E[idx[:, 0]]
    a = np.abs(v.astype(np.float64))
    for h in range(1, idx.shape[1]):
        v = v + E[idx[:, h]]
        a = a + np.abs(E[idx[:, h]].astype(np.float64))
    return v.reshape(ids.shape + (E.shape[1],)), a.reshape(ids.shape + (E.shape[1],))


def sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def pair_loss(loss, sp, sn):
    """(loss, dloss/dsp, dloss/dsn) per pair, in the scores' dtype (losses.py: pointwise :40-50, bpr :82-90, hinge :115-124)."""
    one = sp.dtype.type(1)
    if loss == 'bpr':
        s = sigmoid(sp - sn)
        return one - s, -(s * (one - s)), s * (one - s)
    if loss in ('hinge', 'adaptive_hinge'):
        x = sn - sp + one
        on = (x >= 0).astype(sp.dtype)  # clamp's backward is inclusive at 0
        return np.maximum(x, 0), -on, on
    a, b = sigmoid(sp), sigmoid(sn)
    return (one - a) + b, -(a * (one - a)), b * (one - b)


class Result(object):
    """What minibatch() returns; every array in the dtype it was asked for, the mag_* always float64."""


def minibatch(E, bias, seqs, negs, loss, n_neg, dtype, bloom=None):
    """One PoolNet minibatch in `dtype`.  E [rows, D] (the compressed table under `bloom`), bias [I], seqs [B, L] (0 = padding),
    negs: the draw, flat, in the (n * B, L) layout of sequence/implicit.py:266-286 (candidate r of (b, t) at (r * B + b, t)).
    IEEE rules throughout: a minibatch without a real entry divides by mask.sum() == 0."""
    E32, bias32 = np.asarray(E, np.float32), np.asarray(bias, np.float32).reshape(-1)
    seqs = np.asarray(seqs, np.int64)
    B, L = seqs.shape
    D, I = E32.shape[1], bias32.size
    nn = n_neg if loss == 'adaptive_hinge' else 1
    cand = np.asarray(negs, np.int64).reshape(nn, B, L)
    one = dtype(1)
    b = bias32.astype(dtype)
    r = Result()
    with np.errstate(all='ignore'):
        # forward: rep_t = S_t / (C_t + 1), S and C the exclusive prefix sums of the rows and of (row != 0) per element
        e, ae = item_vectors(E32, seqs, bloom, dtype)
        nz = (e != 0).astype(dtype)
        S, C = excl_cumsum(e), excl_cumsum(nz)
        rep = S / (C + one)
        arep = excl_cumsum(ae) / (C.astype(np.float64) + 1.0)
        r.rep = rep
        r.rep_final = (S[:, -1] + e[:, -1]) / (C[:, -1] + nz[:, -1] + one)
        r.rep_final_mag = (excl_cumsum(ae)[:, -1] + ae[:, -1]) / (C[:, -1] + nz[:, -1] + one).astype(np.float64)
        sp = b[seqs] + seq_sum(rep * e)
        ce, ace = item_vectors(E32, cand, bloom, dtype)
        sc = b[cand] + seq_sum(rep[None] * ce)
        chosen = np.argmax(sc, axis=0)  # the first maximum wins
        pick = lambda x: np.take_along_axis(x, chosen.reshape((1, B, L) + (1,) * (x.ndim - 3)), 0)[0]
        sn, en, aen, nid = pick(sc), pick(ce), pick(ace), pick(cand)
        r.sp, r.sn, r.sc, r.chosen, r.nid = sp, sn, sc, chosen, nid
        # loss: sum(loss * mask) / mask.sum()
        mask = (seqs != 0).astype(dtype)
        M = dtype(int((seqs != 0).sum()))
        l, up, un = pair_loss(loss, sp, sn)
        r.pair_x = sn - sp + one
        r.loss = seq_sum((l * mask).ravel()) / M
        r.loss_mag = float(np.abs((l * mask).astype(np.float64)).sum() / np.float64(M))
        w = mask / M
        gp, gn = up * w, un * w
        r.gp, r.gn = gp, gn
        # backward: dL/d(prefix sum) per timestep, its suffix sum (the cumsum's backward), the two contributions per timestep
        c1 = C + one
        gs = (gp[..., None] * e + gn[..., None] * en) / c1
        ags = (np.abs(gp.astype(np.float64))[..., None] * ae + np.abs(gn.astype(np.float64))[..., None] * aen) / c1.astype(np.float64)
        own = gp[..., None] * rep + suffix_sum(gs)
        aown = np.abs(gp.astype(np.float64))[..., None] * arep + suffix_sum(ags)
        neg = gn[..., None] * rep
        aneg = np.abs(gn.astype(np.float64))[..., None] * arep
        r.own, r.neg = own, neg
        # embedding backward: duplicate rows summed in occurrence order, the padding row (bloom: the skip row) receives nothing
        ids = np.concatenate([seqs.ravel(), nid.ravel()])
        terms = np.concatenate([own.reshape(-1, D), neg.reshape(-1, D)])
        aterms = np.concatenate([aown.reshape(-1, D), aneg.reshape(-1, D)])
        bterms = np.concatenate([gp.ravel(), gn.ravel()])
        live = ids != 0
        ids, terms, aterms, bterms = ids[live], terms[live], aterms[live], bterms[live]
        r.grad_bias = np.zeros(I, dtype)
        np.add.at(r.grad_bias, ids, bterms)
        r.mag_bias = np.zeros(I, np.float64)
        np.add.at(r.mag_bias, ids, np.abs(bterms.astype(np.float64)))
        rows = E32.shape[0]
        r.grad_rows = np.zeros((rows, D), dtype)
        mag = np.zeros((rows, D), np.float64)
        if bloom is None:
            np.add.at(r.grad_rows, ids, terms)
            np.add.at(mag, ids, aterms)
        else:
            idx = hashed_rows(ids, bloom, rows)
            for h in range(idx.shape[1]):
                np.add.at(r.grad_rows, idx[:, h], terms)
                np.add.at(mag, idx[:, h], aterms)
            skip = bloom['skip_row']
            if skip >= 0:
                r.grad_rows[skip] = 0
                mag[skip] = 0
        r.mag_rows = mag.max(axis=1)
    return r


def scores_of(E, bias, rep, rep_mag, bloom, dtype):
    """(scores [n_seq, I], their mag) of every item against the final representations: bias + rep . e, d-ordered."""
    E32, bias32 = np.asarray(E, np.float32), np.asarray(bias, np.float32).reshape(-1)
    v, av = item_vectors(E32, np.arange(bias32.size, dtype=np.int64), bloom, dtype)
    s = bias32.astype(dtype)[None] + seq_sum(rep.astype(dtype)[:, None, :] * v[None])
    mag = np.abs(bias32.astype(np.float64))[None] + (rep_mag[:, None, :] * av[None]).sum(-1)
    return s, mag


def row_errors(got, want, mag):
    """Per-row |got - want|_inf / mag over the rows with mag > 0 (got, want [rows, D] or [rows])."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    if d.ndim > 1:
        d = d.reshape(d.shape[0], -1).max(axis=1)
    live = mag > 0
    return d[live] / mag[live]


def worst(got, want, mag):
    e = row_errors(got, want, mag)
    return float(e.max()) if e.size else 0.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
class Case(object):
    """Inputs of one minibatch, its float64 reference (`exact`) and float32 yardstick (`yard`), computed once and never modified."""

    def __init__(self, name, E, bias, seqs, negs, loss, n_neg, bloom=None, ties=False, degenerate=False):
        self.name, self.loss, self.n_neg, self.bloom = name, loss, n_neg, bloom
        self.E, self.bias = np.ascontiguousarray(E, np.float32), np.ascontiguousarray(bias, np.float32).reshape(-1)
        self.seqs, self.negs = np.ascontiguousarray(seqs, np.int64), np.ascontiguousarray(negs, np.int64).ravel()
        self.B, self.L = self.seqs.shape
        self.D = self.E.shape[1]
        self.degenerate = degenerate
        self.exact = minibatch(self.E, self.bias, self.seqs, self.negs, loss, n_neg, np.float64, bloom)
        self.yard = minibatch(self.E, self.bias, self.seqs, self.negs, loss, n_neg, np.float32, bloom)
        if degenerate:
            return
        x, y = self.exact, self.yard
        self.well_separated = self._well_separated(ties)
        self.yard_rows = worst(y.grad_rows, x.grad_rows, x.mag_rows)
        self.yard_bias = worst(y.grad_bias, x.grad_bias, x.mag_bias)
        self.yard_loss = abs(float(y.loss) - float(x.loss)) / x.loss_mag

    def _well_separated(self, ties):
        """Every decision of the float64 evaluation is MARGIN from flipping (see MARGIN)."""
        x = self.exact
        real = self.seqs != 0
        if self.loss in ('hinge', 'adaptive_hinge') and (np.abs(x.pair_x[real]) < MARGIN).any():
            return False
        if self.loss == 'adaptive_hinge':
            top = x.sc.max(axis=0)
            below = np.where(x.sc < top[None], x.sc, -np.inf).max(axis=0)
            if ((top - below)[real] < MARGIN).any():
                return False
            if not ties:  # equal scores only where the same id was drawn twice
                cand = self.negs.reshape(self.n_neg, self.B, self.L)
                eq = (x.sc == top[None]) & (cand != x.nid[None])
                if eq[:, real].any():
                    return False
        return True

    def tolerances(self):
        return (max(FACTOR * self.yard_rows, FLOOR), max(FACTOR * self.yard_bias, FLOOR), max(FACTOR * self.yard_loss, FLOOR))


def params_for(rs, rows, I, D):
    """Tables whose scores are O(1): rows ~ N(0, D^-1/4), biases ~ N(0, 0.5); the padding row and its bias are zero
    (ScaledEmbedding / ZeroEmbedding with padding_idx = 0)."""
    E = rs.normal(0, D ** -0.25, (rows, D)).astype(np.float32)
    bias = rs.normal(0, 0.5, I).astype(np.float32)
    E[0] = 0.0
    bias[0] = 0.0
    return E, bias


def distinct_ids(rs, B, L, nn):
    """(I, seqs [B, L], negs [nn * B * L]): every entry a distinct id of 1 .. I - 1, I = B * L * (1 + nn) + 2."""
    I = B * L * (1 + nn) + 2
    ids = rs.permutation(np.arange(1, I, dtype=np.int64))
    return I, ids[:B * L].reshape(B, L).copy(), ids[B * L:B * L * (1 + nn)].copy()


def _first_good(build, what):
    """The first of the seeds 0, 1, .. whose case keeps its decisions MARGIN apart (deterministic: the same seed every run)."""
    for seed in range(64):
        c = build(seed)
        if c.well_separated:
            assert max(c.yard_rows, c.yard_bias, c.yard_loss) <= YARD_MAX, (what, c.yard_rows, c.yard_bias, c.yard_loss)
            c.seed = seed
            return c
    raise AssertionError('no well-separated input for %s' % (what,))


_CASES = {}


def _cached(key, build):
    if key not in _CASES:
        _CASES[key] = _first_good(build, key)
    return _CASES[key]


def isolating_case(D, L, loss, n_neg=1, B=None, left_pad=True):
    """The isolating family: B sequences (4 by default) of distinct ids; one of them left-padded when there is room."""
    B = B or 4
    nn = n_neg if loss == 'adaptive_hinge' else 1

    def build(seed):
        rs = np.random.RandomState(1000 * D + 7 * L + 131 * seed + len(loss) + n_neg)
        I, seqs, negs = distinct_ids(rs, B, L, nn)
        if left_pad and L > 2:
            seqs[1, :rs.randint(1, L - 1)] = 0
        E, bias = params_for(rs, I, I, D)
        return Case(('isolating', D, L, loss, n_neg, B), E, bias, seqs, negs, loss, n_neg)

    return _cached(('isolating', D, L, loss, n_neg, B), build)


def shared_case(loss, n_neg=1, B=64, L=64, D=64, I=4):
    """The shared family: 3 real items, each with thousands of occurrences in the minibatch."""
    nn = n_neg if loss == 'adaptive_hinge' else 1

    def build(seed):
        rs = np.random.RandomState(77 + 13 * L + 131 * seed + len(loss) + n_neg)
        seqs = rs.randint(1, I, (B, L)).astype(np.int64)
        for b in range(0, B, 3):
            seqs[b, :rs.randint(1, L)] = 0
        negs = rs.randint(0, I, nn * B * L).astype(np.int64)
        E, bias = params_for(rs, I, I, D)
        return Case(('shared', D, L, loss, n_neg, B), E, bias, seqs, negs, loss, n_neg)

    return _cached(('shared', D, L, loss, n_neg, B), build)


def padding_case(D, L, loss, n_neg=1, n_hash=0):
    """Padding and zeros, 5 sequences of distinct real ids: (0) padding in the middle, twice, and zero-holding items around it;
    (1) padding at the right end; (2) a single real item at the last position; (3) wholly padded; (4) items whose rows hold 0.0
    and -0.0 in some elements and an item whose whole row is zero, in the middle of the sequence.  Under a bloom layer
    (`n_hash` = 2) the zeros are sums: both hashed rows zero in the elements (0.0 + 0.0, -0.0 + -0.0), and hashed rows that are
    exact negatives of each other in some elements / in every element."""
    B = 5
    nn = n_neg if loss == 'adaptive_hinge' else 1
    assert L >= 12

    def build(seed):
        rs = np.random.RandomState(5000 + 1000 * D + 7 * L + 131 * seed + len(loss) + n_neg + 17 * n_hash)
        I, seqs, negs = distinct_ids(rs, B, L, nn)
        rows = I if not n_hash else max(31, int(0.4 * I) | 1)
        E, bias = params_for(rs, rows, I, D)
        bloom = bloom_of(rows, n_hash)[0] if n_hash else None
        z = [int(seqs[4, 2]), int(seqs[4, 3]), int(seqs[4, L // 2])]  # 0.0 in some elements, -0.0 in others, the whole row
        if not n_hash:
            E[z[0], ::3] = 0.0
            E[z[1], 1::4] = -0.0
            E[z[1], 2::4] = 0.0
            E[z[2]] = 0.0
        else:
            # items of sequence 4 whose two hashed rows are distinct, not the skip row, and not shared among the three
            used, z = set(), []
            for t in range(1, L):
                r0, r1 = hashed_rows([seqs[4, t]], bloom, rows)[0]
                if r0 != r1 and r0 != 0 and r1 != 0 and not ({r0, r1} & used):
                    used |= {r0, r1}
                    z.append((int(seqs[4, t]), int(r0), int(r1)))
                if len(z) == 3:
                    break
            assert len(z) == 3, 'no three items with separate hashed rows'
            (_, a0, a1), (_, b0, b1), (_, c0, c1) = z
            E[a0, ::3] = 0.0
            E[a1, ::3] = 0.0
            E[a0, 1::3] = -0.0
            E[a1, 1::3] = -0.0
            E[b1, 1::4] = -E[b0, 1::4]
            E[c1] = -E[c0]
            z = [i for i, _, _ in z]
        seqs[0, 3] = seqs[0, 4] = seqs[0, L - 4] = 0
        seqs[0, 1], seqs[0, 6], seqs[0, L - 2] = z[0], z[2], z[1]  # the zero-holding items again, around the padding
        seqs[1, L - 5:] = 0
        seqs[2, :L - 1] = 0
        seqs[3, :] = 0
        c = Case(('padding', D, L, loss, n_neg, n_hash), E, bias, seqs, negs, loss, n_neg, bloom=bloom)
        c.zero_items = z
        return c

    return _cached(('padding', D, L, loss, n_neg, n_hash), build)


def tie_case(D=64, L=17, n_neg=5, B=4):
    """Adaptive tie: at every third timestep two distinct items with identical row and bias (the bias high enough to win) are
    drawn as candidates 3 and 1 -- the gradient lands on candidate 1, drawn first; the twin's row stays exactly zero."""
    def build(seed):
        rs = np.random.RandomState(9000 + 131 * seed)
        I, seqs, negs = distinct_ids(rs, B, L, n_neg)
        E, bias = params_for(rs, I, I, D)
        cand = negs.reshape(n_neg, B, L)
        first, twin = cand[1, :, ::3], cand[3, :, ::3]
        E[twin] = E[first]
        bias[first] = bias[twin] = np.float32(4.0)
        c = Case(('tie', D, L, n_neg, B), E, bias, seqs, negs, 'adaptive_hinge', n_neg, ties=True)
        c.first, c.twin, c.twin_real = first.ravel().copy(), twin.ravel().copy(), (seqs[:, ::3] != 0).ravel()
        return c

    return _cached(('tie', D, L, n_neg, B), build)


def no_real_entry_case(D=8, L=5, B=3):
    """A minibatch with no real entry: mask.sum() == 0."""
    rs = np.random.RandomState(3)
    I, _, negs = distinct_ids(rs, B, L, 1)
    E, bias = params_for(rs, I, I, D)
    return Case(('no real entry', D, L, B), E, bias, np.zeros((B, L), np.int64), negs, 'bpr', 1, degenerate=True)


# ---- the engine --------------------------------------------------------------------------------------------------------------------
def run_engine(be, case, variant=1):
    """One training call of `case` under "seq_variant" = variant: (loss, item-row gradients, item-bias gradients)."""
    eng = be.engine
    dev = be.seq_model([case.E, case.bias], opt='adam_dense', lr=0.0, betas=(0.0, 0.999), item_bloom=case.bloom)
    mb_loss = be.alloc(np.zeros(1, dtype=np.float32))
    d_seqs, d_negs = be.alloc(case.seqs), be.alloc(case.negs)
    with eng.options(seq_variant=variant):
        eng.poolnet_train(dev.tables, dev.optim, 0, be.ptr(d_seqs), case.B, case.L, case.B, case.loss, case.n_neg, be.ptr(mb_loss),
                          d_neg_in=be.ptr(d_negs), stream=be.stream)
    got = (be.get(mb_loss).copy()[0], be.get(dev.s1[0]).reshape(case.E.shape).copy(), be.get(dev.s1[1]).ravel().copy())
    if not case.degenerate:
        # lr = 0: the parameters come back as they went in, bit for bit.  (An element that went in as -0.0 comes back as a zero of
        # either sign: Adam's p + (-lr) * m / (sqrt(v) + eps) is -0.0 + 0.0 = +0.0 under a negative m, in torch as here.)
        p_rows = be.get(dev.p[0]).reshape(case.E.shape)
        minus_zero = (case.E == 0) & np.signbit(case.E)
        assert same_bits(p_rows[~minus_zero], case.E[~minus_zero]) and (p_rows[minus_zero] == 0).all(), (case.name, 'the item rows moved at lr = 0')
        assert same_bits(be.get(dev.p[1]).ravel(), case.bias), (case.name, 'the item biases moved at lr = 0')
    return got, dev


def hold_to_float64(case, got, what):
    """The engine's (loss, row gradients, bias gradients) against the float64 restatement by the module's rule."""
    x = case.exact
    loss, rows, bias = got
    tol_rows, tol_bias, tol_loss = case.tolerances()
    err_rows, err_bias = worst(rows, x.grad_rows, x.mag_rows), worst(bias, x.grad_bias, x.mag_bias)
    err_loss = abs(float(loss) - float(x.loss)) / x.loss_mag
    print('%s %s: yardstick rows %.2e bias %.2e loss %.2e | kernel rows %.2e bias %.2e loss %.2e'
          % (case.name, what, case.yard_rows, case.yard_bias, case.yard_loss, err_rows, err_bias, err_loss))
    # exactly zero where the restatement is: rows never looked up, the padding row and its bias, candidates that were not chosen
    assert (rows[x.mag_rows == 0] == 0).all(), (case.name, what, 'a row the restatement leaves at zero was written')
    assert (bias[x.mag_bias == 0] == 0).all(), (case.name, what, 'a bias the restatement leaves at zero was written')
    assert np.isfinite(rows).all() and np.isfinite(bias).all(), (case.name, what)
    assert err_rows <= tol_rows, (case.name, what, 'item rows', err_rows, tol_rows, case.yard_rows)
    assert err_bias <= tol_bias, (case.name, what, 'item biases', err_bias, tol_bias, case.yard_bias)
    assert err_loss <= tol_loss, (case.name, what, 'loss', err_loss, tol_loss, case.yard_loss)


def check_case(be, case):
    """`case` under both forms of the sequence pass where the register form applies ("seq_variant" 1, the default, and 0, the
    LDS-staged form): the same bits, and each held to float64."""
    variants = (1, 0) if reg_form_applies(case.D, case.L) else (1,)
    results = []
    for v in variants:
        got, _ = run_engine(be, case, v)
        hold_to_float64(case, got, 'seq_variant %d' % v)
        results.append(got)
    if len(results) == 2:
        for k, (a, b) in enumerate(zip(*results)):
            assert same_bits(np.asarray(a), np.asarray(b)), (case.name, 'output %d differs between the two forms of the sequence pass' % k)
    return results[0]


def check_isolating(be, D, L, loss, n_neg=1, B=None):
    case = isolating_case(D, L, loss, n_neg, B)
    x = case.exact
    # the family is what it claims: every live id occurs once, so every row is one term of one timestep
    ids = np.concatenate([case.seqs.ravel(), case.negs])
    ids = ids[ids != 0]
    assert len(np.unique(ids)) == len(ids) and case.E.shape[0] > case.B * case.L * (1 + (n_neg if loss == 'adaptive_hinge' else 1)) + 1
    _, rows, bias = check_case(be, case)
    if loss == 'adaptive_hinge' and n_neg > 1:  # the candidates that were not chosen: exactly zero
        cand = case.negs.reshape(n_neg, case.B, case.L)
        idle = cand[cand != x.nid[None]]
        assert (rows[idle] == 0).all() and (bias[idle] == 0).all()


def check_wide_adaptive(be, n_neg):
    """Adaptive hinge over n_neg candidates per timestep (WIDE_NS) at WIDE_SHAPE, both forms of the pass: every timestep's chosen
    candidate, its row and bias against float64; the n_neg - 1 others exactly zero.  The chosen rows are spread over the
    candidates -- from n = 64 not all among the first six, where the other cases end."""
    D, L = WIDE_SHAPE
    case = isolating_case(D, L, 'adaptive_hinge', n_neg)
    real = case.seqs != 0
    assert len(np.unique(case.exact.chosen[real])) >= min(real.sum(), n_neg) // 2 and case.exact.chosen[real].max() >= min(6, n_neg // 2)
    check_isolating(be, D, L, 'adaptive_hinge', n_neg)


def check_shared(be, loss, n_neg=1, L=64):
    """Long runs: the three real rows collect thousands of occurrences (per-tile partials + k_item_stitch in the SEQ mode)."""
    case = shared_case(loss, n_neg, L=L)
    eng = be.engine
    before = eng.get_stat('item_long_launches')
    check_case(be, case)
    assert eng.get_stat('item_long_launches') == before + 2, 'the long-run form of the item pass was not taken'


def check_padding(be, D, L, loss, n_neg=1, n_hash=0):
    case = padding_case(D, L, loss, n_neg, n_hash)
    x = case.exact
    # the inputs hold what they claim: exact zeros in real items' vectors, a real item whose vector is all zero
    v, _ = item_vectors(case.E, np.asarray(case.zero_items), case.bloom, np.float32)
    zeros = np.concatenate([v[0][v[0] == 0], v[1][v[1] == 0]])
    assert np.signbit(zeros).any() and not np.signbit(zeros).all() and (v[2] == 0).all()
    assert all((v[k] == 0).any() and (v[k] != 0).any() for k in (0, 1))
    assert (case.seqs[3] == 0).all() and (case.seqs[0, 3:5] == 0).all() and case.seqs[0, 5] != 0 and case.seqs[1, -1] == 0
    check_case(be, case)


def check_tie(be):
    case = tie_case()
    x = case.exact
    assert (x.chosen[:, ::3] == 1).all(), 'the twins are not the maximum'
    _, rows, bias = check_case(be, case)
    assert (rows[case.twin] == 0).all() and (bias[case.twin] == 0).all(), 'the candidate drawn second received a gradient'
    assert case.twin_real.sum() > 10 and (bias[case.first[case.twin_real]] > 0).all(), 'the candidate drawn first received none'


def check_grid_stride(be, cus, loss='bpr', n_neg=1):
    """2 * (8 * cus) + 3 sequences of length 3 at dim 8: every workgroup of the sequence pass (min(B, 8 * cus) of them) takes a
    second sequence, three of them a third, reusing its LDS; every sequence's rows are held to float64."""
    B = 2 * 8 * cus + 3
    check_isolating(be, 8, 3, loss, n_neg, B=B)


def check_no_real_entry(be):
    """mask.sum() == 0: the loss is NaN, the rows and biases of the sampled negatives are NaN, nothing else is touched -- the
    restatement under IEEE rules, the engine and PoolNetOracle agree on which elements are NaN (no word on payloads)."""
    from oracle.oracle import PoolNetOracle
    case = no_real_entry_case()
    x = case.exact
    nan_rows, nan_bias = np.isnan(x.grad_rows), np.isnan(x.grad_bias)
    assert np.isnan(x.loss) and nan_rows[case.negs].all() and nan_bias[case.negs].all()
    assert nan_rows.sum() == case.negs.size * case.D and nan_bias.sum() == case.negs.size
    assert (x.grad_rows[~nan_rows] == 0).all() and (x.grad_bias[~nan_bias] == 0).all()
    ora_loss, ora_g = PoolNetOracle(case.E, case.bias, opt='adagrad').step(case.seqs, case.negs, loss=case.loss, n_neg=1, want_grads=True)
    assert np.isnan(ora_loss)
    assert np.array_equal(np.isnan(ora_g[0]), nan_rows) and np.array_equal(np.isnan(ora_g[1].ravel()), nan_bias)
    assert (ora_g[0][~nan_rows] == 0).all() and (ora_g[1].ravel()[~nan_bias] == 0).all()
    for variant in (1, 0):
        (loss, rows, bias), dev = run_engine(be, case, variant)
        assert np.isnan(loss), variant
        assert np.array_equal(np.isnan(rows), nan_rows) and np.array_equal(np.isnan(bias), nan_bias), variant
        assert same_bits(rows[~nan_rows], np.zeros_like(rows)[~nan_rows]) and same_bits(bias[~nan_bias], np.zeros_like(bias)[~nan_bias])
        p_rows, p_bias = be.get(dev.p[0]).reshape(case.E.shape), be.get(dev.p[1]).ravel()
        assert same_bits(p_rows[~nan_rows], case.E[~nan_rows]) and same_bits(p_bias[~nan_bias], case.bias[~nan_bias]), variant


def check_prediction(be, D, L, n_hash=0):
    """slk_poolnet_predict (every item, and a list of items) and slk_poolnet_scores on the padding-and-zeros sequences: the
    scores against bias + rep_final . e in float64, rep_final the representation after the last timestep."""
    case = padding_case(D, L, 'bpr', 1, n_hash)
    eng = be.engine
    x, y = case.exact, case.yard
    I = case.bias.size
    want, mag = scores_of(case.E, case.bias, x.rep_final, x.rep_final_mag, case.bloom, np.float64)
    yard, _ = scores_of(case.E, case.bias, y.rep_final, x.rep_final_mag, case.bloom, np.float32)
    dev = be.seq_model([case.E, case.bias], item_bloom=case.bloom)
    d_seqs = be.alloc(case.seqs)
    out = be.alloc(np.full((case.B, I), -7.25, np.float32))
    eng.poolnet_scores(dev.tables, be.ptr(d_seqs), case.B, L, be.ptr(out), be.stream)
    all_scores = be.get(out).reshape(case.B, I)
    some = np.concatenate([np.arange(0, I, 7, dtype=np.int64), np.asarray(case.zero_items, np.int64)])
    d_some = be.alloc(some)
    for s in range(case.B):
        yard_err = worst(yard[s], want[s], mag[s])
        tol = max(FACTOR * yard_err, FLOOR)
        d_seq = be.alloc(case.seqs[s])
        o_all, o_some = be.alloc(np.full(I, -7.25, np.float32)), be.alloc(np.full(some.size, -7.25, np.float32))
        eng.poolnet_predict(dev.tables, be.ptr(d_seq), L, None, I, be.ptr(o_all), be.stream)
        eng.poolnet_predict(dev.tables, be.ptr(d_seq), L, be.ptr(d_some), some.size, be.ptr(o_some), be.stream)
        for what, got, w, m in (('scores', all_scores[s], want[s], mag[s]), ('predict, every item', be.get(o_all), want[s], mag[s]),
                                ('predict, some items', be.get(o_some), want[s][some], mag[s][some])):
            err = worst(got, w, m)
            print('%s sequence %d %s: yardstick %.2e | kernel %.2e' % (case.name, s, what, yard_err, err))
            assert (got[m == 0] == 0).all(), (case.name, s, what)
            assert err <= tol, (case.name, s, what, err, tol)
    assert same_bits(be.get(dev.p[0]).reshape(case.E.shape), case.E) and same_bits(be.get(dev.p[1]).ravel(), case.bias)
