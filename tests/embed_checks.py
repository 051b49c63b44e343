"""Shared checks of the embedding front-end, entry by entry: slk_embedding_forward / slk_embedding_backward_plan /
slk_embedding_backward_fill (csrc/slk_embed.hip; include/spotlight_hip.h), run on the emulator build (tests/test_emu_embed.py)
and on the gfx950 library (tests/test_gpu_embed.py).  `be` is the EmuBackend / HipBackend object; the checks call
be.engine.embedding_forward / embedding_backward_plan / embedding_backward_fill directly, not spotlight_amd.embedding.lookup.

THE REFERENCE IS EXACT.  The table W and the upstream gradient g are integers in [-8, 8] stored as float32, and no run of equal
rows is longer than 2^17 lookups (bloom: occurrences), so every partial sum of every summation order is an integer of magnitude
below 8 * 2^17 = 2^20 < 2^24: float32 addition never rounds, and the expected gradient is a plain int64 np.add.at.  Every
comparison is np.array_equal, element by element, without a tolerance and without a norm: a term that is dropped, added twice or
filed under the wrong row changes the result however small the row is next to a hot one.

The cases are run LAYOUTS, not random ids.  Ids are built from per-row counts and shuffled; the backward's stable sort undoes the
shuffle, so the counts alone fix what k_emb_reduce sees: which runs lie strictly inside a chunk of EM_CHUNK = 16 (stored at
once), which are a chunk's first or last run (entries 2c / 2c + 1 of the next level), which fill a chunk (the explicit zero
entry), and how many levels a run climbs.  The dims 1 / 3 / 4 / 65 / 260 are one lane per row scalar and vector (T = 1), and 64
lanes striding the row scalar and vector (T = 64); 64 and 128 are the shipped ones.

One float case per backend (check_float) bounds every element by the standard bound of a float32 sum in any order, on that
element's own terms."""
import numpy as np
import pytest

from spotlight_amd import _native

EM_CHUNK = 16                          # csrc/slk_embed.hip
SENTINEL = np.float32(-7.25)           # no sum of integers, and never written by the entries
ROW_SENTINEL = np.int64(-77)
MAX_RUN = 1 << 17                      # 8 * 2^17 = 2^20 < 2^24: every partial sum is an exactly representable integer

DIMS = (1, 3, 4, 65, 260)
SHIPPED_DIMS = DIMS + (64, 128)

ONE_ROW_NS = (1, 15, 16, 17, 255, 256, 257, 4096, 4097, 65536, 70001)
ALL_PADDING_NS = tuple(n for n in ONE_ROW_NS if n <= 4097)
UNIFORM_COUNTS = (1, 8, 16, 32, 48)
UNIFORM_TABLES = ((40, None), (40, 0), (64, 63), (64, 5))       # (rows, padding_idx)
NAMED = {                                                          # name -> (per-row counts, padding_idx)
    'cycle': ([1, 15, 16, 17, 31, 33, 2, 0, 300, 1] * 5, 0),
    'padding_first': ([3000] + [1] * 63, 0),
    'padding_last': ([1] * 63 + [3000], 63),
}
KEY_WIDTH_TABLES = ((255, 0), (256, 255), (65536, 0), (65536, 65535), (65537, None), (1 << 20, 7))
KEY_WIDTH_DIMS = (4, 6)
BLOOM_HASHES = (1, 2, 4, 8)
BLOOM_DIMS = (4, 6, 72)
BLOOM_ROWS = (7, 64, 301)
REUSE_DIMS = (4, 65)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def integers(rs, shape):
    """Integers in [-8, 8] as float32."""
    return rs.randint(-8, 9, size=shape, dtype=np.int8).astype(np.float32)


def ids_of_counts(counts, seed=0):
    """counts[r] lookups of row r, shuffled."""
    ids = np.repeat(np.arange(len(counts), dtype=np.int64), np.asarray(counts, dtype=np.int64))
    np.random.RandomState(seed).shuffle(ids)
    return ids


def bloom_of(rows, n_hash):
    """(oracle descriptor, SlkBloom) of a BloomEmbedding with `rows` compressed rows, padding id 0, skip_row 0."""
    from oracle.oracle import bloom_desc
    desc = bloom_desc(n_hash=n_hash, padding_idx=0)
    assert desc['skip_row'] == 0
    return desc, _native.make_bloom(rows, n_hash, padding_idx=0, skip_row=0, seeds=desc['seeds'])


def occurrences(ids, rows, padding_idx, bloom):
    """(table row, lookup) of every occurrence that receives a gradient: one per lookup, or n_hash per lookup of a bloom layer;
    the padding row (bloom: the skip row) receives none."""
    ids = np.asarray(ids, dtype=np.int64)
    if bloom is None:
        occ_rows, occ_k, skip = ids, np.arange(len(ids), dtype=np.int64), padding_idx
    else:
        from oracle.oracle import bloom_indices
        desc = bloom[0]
        idx = bloom_indices(ids, desc['seeds'], rows, desc['padding_idx'])
        occ_rows = idx.reshape(-1)
        occ_k = np.repeat(np.arange(len(ids), dtype=np.int64), idx.shape[1])
        skip = desc['skip_row']
    assert occ_rows.size == 0 or (occ_rows.min() >= 0 and occ_rows.max() < rows)  # the entries do not check ids: feed none outside
    keep = np.ones(occ_rows.shape, bool) if skip is None or skip < 0 else occ_rows != skip
    return occ_rows[keep], occ_k[keep]


def exact_sums(occ_rows, occ_k, g, rows, dtype=np.int64):
    """[rows, D] sums of g[occ_k] filed under occ_rows: np.add.at on the flattened table."""
    D = g.shape[1]
    total = np.zeros(rows * D, dtype)
    cols = np.arange(D, dtype=np.int64)
    np.add.at(total, (occ_rows[:, None] * D + cols).reshape(-1), g[occ_k].astype(dtype).reshape(-1))
    return total.reshape(rows, D)


class Outcome(object):
    """What one case left in the caller's buffers, for bit comparisons between engines."""

    def __init__(self, out, dense, coo_rows, coo_values):
        self.out, self.dense, self.coo_rows, self.coo_values = out, dense, coo_rows, coo_values

    def same_bits(self, other):
        return all(same_bits(getattr(self, k), getattr(other, k)) for k in ('out', 'dense', 'coo_rows', 'coo_values'))


def _guarded(be, n, D):
    """A sentinel-filled [n + 1, D] buffer: n rows for the entry, one guard row behind them."""
    return be.alloc(np.full((n + 1, D), SENTINEL, np.float32))


def _dense_fill(be, rows, D, bloom, padding_idx, d_ids, n, d_g):
    d_dense = _guarded(be, rows, D)
    be.engine.embedding_backward_plan(rows, D, bloom[1] if bloom else None, padding_idx, be.ptr(d_ids), n, stream=be.stream)
    be.engine.embedding_backward_fill(be.ptr(d_g), be.ptr(d_dense), stream=be.stream)
    return be.get(d_dense)


def _coo_fill(be, rows, D, bloom, padding_idx, d_ids, n, d_g):
    n_rows = be.engine.embedding_backward_plan(rows, D, bloom[1] if bloom else None, padding_idx, be.ptr(d_ids), n,
                                               count_rows=True, stream=be.stream)
    assert 0 <= n_rows <= rows
    d_rows = be.alloc(np.full(n_rows + 1, ROW_SENTINEL, np.int64))
    d_vals = _guarded(be, n_rows, D)
    be.engine.embedding_backward_fill(be.ptr(d_g), None, be.ptr(d_rows), be.ptr(d_vals), stream=be.stream)
    return n_rows, be.get(d_rows), be.get(d_vals)


def check_case(be, ids, rows, D, padding_idx, bloom=None, seed=0, data=None):
    """Forward, dense backward, COO backward and determinism of one case against the exact integer sums.  `bloom`: bloom_of().
    `data`: (W, g) to use instead of drawing them.  Returns the Outcome."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n = len(ids)
    rs = np.random.RandomState(1000 + seed)
    W, g = data if data is not None else (integers(rs, (rows, D)), integers(rs, (n, D)))
    assert W.shape == (rows, D) and g.shape == (n, D)
    d_ids = be.alloc(ids if n else np.zeros(1, np.int64))
    d_W, d_g = be.alloc(W), be.alloc(g if n else np.zeros((1, D), np.float32))
    desc = bloom[1] if bloom else None

    # 1. forward
    d_out = _guarded(be, n, D)
    be.engine.embedding_forward(be.ptr(d_W), rows, D, desc, be.ptr(d_ids), n, be.ptr(d_out), stream=be.stream)
    out = be.get(d_out)
    if bloom is None:
        want_out = W[ids]
    else:
        from sweep_checks import bloom_rows
        want_out = bloom_rows(W, bloom[0], ids)
    assert np.array_equal(out[:n], want_out), 'forward'
    assert same_bits(out[:n], want_out.astype(np.float32)), 'forward bits'
    assert np.all(out[n] == SENTINEL), 'forward wrote behind its n rows'

    occ_rows, occ_k = occurrences(ids, rows, padding_idx, bloom)
    distinct, run = np.unique(occ_rows, return_counts=True)
    assert run.size == 0 or run.max() <= MAX_RUN  # the premise of the exact comparison
    want = exact_sums(occ_rows, occ_k, g, rows)
    skip = bloom[0]['skip_row'] if bloom else padding_idx
    if skip is not None and 0 <= skip < rows:
        assert not want[skip].any() and skip not in distinct

    # 2. dense backward
    dense = _dense_fill(be, rows, D, bloom, padding_idx, d_ids, n, d_g)
    assert np.array_equal(dense[:rows], want), 'dense gradient'
    untouched = np.ones(rows, bool)
    untouched[distinct] = False
    assert not dense[:rows][untouched].any(), 'rows without a lookup are exact zeros'
    assert np.all(dense[rows] == SENTINEL), 'the dense fill wrote behind its table'

    # 3. COO backward
    n_rows, coo_rows, coo_vals = _coo_fill(be, rows, D, bloom, padding_idx, d_ids, n, d_g)
    assert n_rows == len(distinct), ('distinct rows with a gradient', n_rows, len(distinct))
    assert np.array_equal(coo_rows[:n_rows], distinct), 'COO rows ascending'
    assert np.array_equal(coo_vals[:n_rows], want[distinct]), 'COO values'
    assert coo_rows[n_rows] == ROW_SENTINEL and np.all(coo_vals[n_rows] == SENTINEL), 'the COO fill wrote behind its outputs'

    # 4. determinism
    assert same_bits(_dense_fill(be, rows, D, bloom, padding_idx, d_ids, n, d_g), dense)
    n_rows2, coo_rows2, coo_vals2 = _coo_fill(be, rows, D, bloom, padding_idx, d_ids, n, d_g)
    assert n_rows2 == n_rows and same_bits(coo_rows2, coo_rows) and same_bits(coo_vals2, coo_vals)
    return Outcome(out, dense, coo_rows, coo_vals)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def check_one_row(be, n, D):
    """One row of a 5-row table owns all n lookups: a single run through every level; n = 16^k is all "first && last" chunks."""
    check_case(be, np.full(n, 3, np.int64), 5, D, None, seed=n)


def check_all_padding(be, n, D):
    """Every lookup is the padding row: the dense gradient is all zeros, the COO one has no rows and its fill leaves the outputs
    alone (check_case's sentinels)."""
    check_case(be, np.zeros(n, np.int64), 5, D, 0, seed=n)


def check_uniform(be, c, rows, padding_idx, D):
    """Every row has exactly c lookups.  c = 1: interior runs only; 8: two runs per chunk, both at its edges; 16: every chunk is one
    whole run; 32, 48: every run spans whole chunks.  With a padding row in the middle, its lookups are re-keyed to `rows` and
    sort to the end, which shifts every later run by c."""
    check_case(be, ids_of_counts([c] * rows, seed=c), rows, D, padding_idx, seed=c)


def check_named(be, name, D):
    counts, padding_idx = NAMED[name]
    check_case(be, ids_of_counts(counts, seed=len(counts)), len(counts), D, padding_idx, seed=len(name))


def check_key_width(be, rows, padding_idx, D):
    """Row counts around the widths of the sort key: the no-gradient key `rows` needs one bit more than any real row when `rows`
    is a power of two.  3000 lookups, 30 % on row 0 and 30 % on the last row."""
    rs = np.random.RandomState(rows % 9973)
    ids = rs.randint(0, rows, 3000).astype(np.int64)
    u = rs.rand(3000)
    ids[u < 0.3] = 0
    ids[u >= 0.7] = rows - 1
    check_case(be, ids, rows, D, padding_idx, seed=rows % 9973)


def check_one_row_table(be, D):
    check_case(be, np.zeros(40, np.int64), 1, D, None, seed=40)


def check_bloom(be, n_hash, D, rows):
    """A bloom layer: the forward is the sum of the hashed rows, the backward files n * n_hash occurrences.  With 7 compressed
    rows several hashes of one id collide on one row, which must receive the gradient once per hash; every hash that lands on the
    skip row 0 -- all of a padding id's, and some of other ids' -- is dropped."""
    rs = np.random.RandomState(7 * n_hash + rows)
    ids = rs.randint(1, 1000, 700).astype(np.int64)
    ids[rs.rand(700) < 0.2] = 0
    bloom = bloom_of(rows, n_hash)
    occ_rows, occ_k = occurrences(ids, rows, None, bloom)
    if rows == 7 and n_hash > 1:  # the case is about collisions: some lookup does hit one row under two hashes
        pair = occ_k * rows + occ_rows
        assert len(np.unique(pair)) < len(pair)
    check_case(be, ids, rows, D, None, bloom=bloom, seed=n_hash)


def check_buffer_reuse(be, D):
    """A large call, a small one and the large one again on ONE engine, each bit-equal to the same case on a fresh engine: the
    scratch buffers keep the size of the large call, so its keys and partial sums lie right behind what the small call uses."""
    big = (np.full(70001, 3, np.int64), 5, D, None)
    small = (ids_of_counts([1, 6, 0, 8], seed=15), 4, D, 0)
    assert len(small[0]) == 15
    shared = [check_case(be, *case, seed=i % 2) for i, case in enumerate((big, small, big))]
    for i, case in enumerate((big, small)):
        other = type(be)()
        try:
            alone = check_case(other, *case, seed=i)
        finally:
            other.close()
        assert shared[i].same_bits(alone)
        if i == 0:
            assert shared[2].same_bits(alone)


def check_state_machine(be):
    """plan -> fill, as include/spotlight_hip.h and csrc/slk_embed.hip state it.  A fill needs a plan and consumes it; a sparse
    fill needs a plan that counted rows, and its refusal leaves the plan in place (the check comes before the plan is taken); a
    plan replaces the one before it, and a refused plan leaves none.  A refusal is SlkError and writes nothing."""
    eng = type(be)()  # a ctx that never planned
    try:
        rows, D, n = 9, 4, 37
        rs = np.random.RandomState(5)
        ids_a, ids_b = rs.randint(0, rows, n).astype(np.int64), rs.randint(0, rows, n).astype(np.int64)
        g = integers(rs, (n, D))
        d_a, d_b, d_g = eng.alloc(ids_a), eng.alloc(ids_b), eng.alloc(g)
        want_a = exact_sums(*occurrences(ids_a, rows, 0, None), g, rows)
        want_b = exact_sums(*occurrences(ids_b, rows, 0, None), g, rows)
        assert not np.array_equal(want_a, want_b)
        e = eng.engine

        def plan(d_ids, count=False, n_=n, dim=D):
            return e.embedding_backward_plan(rows, dim, None, 0, eng.ptr(d_ids), n_, count_rows=count, stream=eng.stream)

        def refused(sparse):
            d_dense, d_rows, d_vals = _guarded(eng, rows, D), eng.alloc(np.full(rows + 1, ROW_SENTINEL, np.int64)), _guarded(eng, rows, D)
            with pytest.raises(_native.SlkError):
                if sparse:
                    e.embedding_backward_fill(eng.ptr(d_g), None, eng.ptr(d_rows), eng.ptr(d_vals), stream=eng.stream)
                else:
                    e.embedding_backward_fill(eng.ptr(d_g), eng.ptr(d_dense), stream=eng.stream)
            assert np.all(eng.get(d_dense) == SENTINEL) and np.all(eng.get(d_vals) == SENTINEL)
            assert np.all(eng.get(d_rows) == ROW_SENTINEL)

        def dense():
            d_dense = _guarded(eng, rows, D)
            e.embedding_backward_fill(eng.ptr(d_g), eng.ptr(d_dense), stream=eng.stream)
            got = eng.get(d_dense)
            assert np.all(got[rows] == SENTINEL)
            return got[:rows]

        refused(sparse=False)  # no plan yet
        refused(sparse=True)
        plan(d_a)
        refused(sparse=True)   # the plan did not count rows; it stays
        assert np.array_equal(dense(), want_a)
        refused(sparse=False)  # the fill consumed it
        refused(sparse=True)
        assert plan(d_a, count=True) == len(np.unique(ids_a[ids_a != 0]))
        assert np.array_equal(dense(), want_a)  # a plan that counted rows serves a dense fill as well
        refused(sparse=True)

        plan(d_a, n_=0)        # no lookups: the dense gradient is all zeros
        got = dense()
        assert got.shape == (rows, D) and not got.any()
        refused(sparse=False)
        assert plan(d_a, count=True, n_=0) == 0
        d_rows, d_vals = eng.alloc(np.full(1, ROW_SENTINEL, np.int64)), _guarded(eng, 0, D)
        e.embedding_backward_fill(eng.ptr(d_g), None, eng.ptr(d_rows), eng.ptr(d_vals), stream=eng.stream)
        assert np.all(eng.get(d_rows) == ROW_SENTINEL) and np.all(eng.get(d_vals) == SENTINEL)
        refused(sparse=True)

        plan(d_a)              # a new plan replaces an unconsumed one
        plan(d_b)
        assert np.array_equal(dense(), want_b)
        refused(sparse=False)

        plan(d_a)              # a refused plan leaves none
        with pytest.raises(_native.SlkError):
            plan(d_b, dim=4097)
        refused(sparse=False)
    finally:
        eng.close()


def check_float(be):
    """Standard-normal gradients: n = 6000 lookups of 50 rows, D = 8, 60 % on row 7, padding_idx 0.  Every element within the bound
    of a float32 sum of c terms in ANY order, c u / (1 - c u) * sum |terms| with u = 2^-24 (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., (4.4) with the term count for the number of additions), c and sum |terms| that element's own:
    per row, not per table.  A row with a single term is that term, bit for bit; row 49 is given exactly one lookup for that, row
    48 none.  (The worst element on the emulator build and on gfx950: 0.016 of its bound.)"""
    n, rows, D = 6000, 50, 8
    rs = np.random.RandomState(6000)
    ids = rs.randint(0, rows - 2, n).astype(np.int64)
    ids[rs.rand(n) < 0.6] = 7
    ids[n // 2] = rows - 1  # row 49: exactly one lookup; row 48: none
    g = rs.normal(size=(n, D)).astype(np.float32)
    d_ids, d_g = be.alloc(ids), be.alloc(g)
    occ_rows, occ_k = occurrences(ids, rows, 0, None)
    distinct, count = np.unique(occ_rows, return_counts=True)
    assert count.max() > 0.55 * n and count.min() == 1
    exact = exact_sums(occ_rows, occ_k, g, rows, np.float64)
    mass = exact_sums(occ_rows, occ_k, np.abs(g), rows, np.float64)
    c = np.zeros(rows)
    c[distinct] = count
    u = 2.0 ** -24
    bound = (c * u / (1 - c * u))[:, None] * mass
    single = distinct[count == 1]

    def verify(got_rows, got):
        """`got`: the sums of `got_rows`."""
        err = np.abs(got.astype(np.float64) - exact[got_rows])
        print('embedding backward, float case: worst error / bound = %.3g' % (err / np.maximum(bound[got_rows], 1e-300)).max())
        assert np.all(err <= bound[got_rows])
        for r in single:
            k = occ_k[occ_rows == r]
            assert same_bits(got[list(got_rows).index(r)], g[k[0]])

    dense = _dense_fill(be, rows, D, None, 0, d_ids, n, d_g)
    assert np.all(dense[rows] == SENTINEL)
    assert not dense[0].any() and not dense[rows - 2].any()  # the padding row and the row nobody looked up: bound 0
    verify(np.arange(rows), dense[:rows])
    n_rows, coo_rows, coo_vals = _coo_fill(be, rows, D, None, 0, d_ids, n, d_g)
    assert n_rows == len(distinct) and np.array_equal(coo_rows[:n_rows], distinct)
    verify(distinct, coo_vals[:n_rows])
    assert same_bits(coo_vals[:n_rows], dense[distinct])  # one reduction, two destinations
    assert same_bits(_dense_fill(be, rows, D, None, 0, d_ids, n, d_g), dense)


def check_grid_wrap(be, cus):
    """Device only (`cus`: the part's compute units).  At D = 65 a row takes 64 lanes, a block of k_emb_reduce holds 4 chunks and a
    block of k_emb_gather 4 lookups, and both grids are capped at 32 blocks per compute unit: with 16 * (4 * 32 * cus) + 53
    lookups level 0 of the reduction needs 32 * cus + 1 blocks, so its grid-stride loop takes a second trip, and the gather's
    takes sixteen.  1000 rows, padding_idx 0, one row with 2^17 lookups and the rest uniform."""
    cap = 32 * cus
    n = EM_CHUNK * (4 * cap) + EM_CHUNK * 3 + 5
    rows, D = 1000, 65
    nchunks = (n + EM_CHUNK - 1) // EM_CHUNK
    assert (nchunks + 3) // 4 > cap, 'level 0 of the reduction no longer wraps its grid'
    assert (n + 3) // 4 > cap, 'the gather no longer wraps its grid'
    rs = np.random.RandomState(cus)
    hot = min(MAX_RUN, n // 2)
    ids = rs.randint(0, rows - 1, n).astype(np.int64)
    ids[ids >= 500] += 1  # uniform over every row but 500 ...
    ids[rs.permutation(n)[:hot]] = 500  # ... which gets exactly `hot` lookups
    assert np.count_nonzero(ids == 500) == hot
    check_case(be, ids, rows, D, 0, seed=cus)
