"""The radix sort's top-digit route (csrc/slk_sort.hip: one scatter on the top digit, then every bucket finished inside
one workgroup) against numpy's stable argsort per segment, on the fiber emulator; tests/test_gpu_sort_finish.py is the
`-m gpu` twin and imports the checks from here.

The route is taken by SEGMENTED sorts of u32 keys with more than 8 bits once `n >= sort_big_min`; every check forces
the hook, states which route it means and asserts it from the statistics: `sort_finish_sorts` counts the sorts enqueued
on the route, `sort_finish_fallbacks` those whose buckets did not fit `sort_finish_cap` pairs (the LSD passes, enqueued
behind, then do the sort)."""
import numpy as np
import pytest

from emu_backend import EmuBackend

KT = {0: (np.uint32, np.uint32), 1: (np.uint32, np.uint64)}
BIG_MIN_DEFAULT = 1 << 20


def payload(kind, n, rng):
    vals = rng.randint(0, 2 ** 31, size=n).astype(KT[kind][1])
    if kind == 1:  # both halves of a u64 payload carry information
        vals = vals | (np.arange(n, dtype=np.uint64) << np.uint64(33))
    return vals


def run_sort(be, kind, keys, bits, seg_len, route, big_min=1, repeat=1):
    """Sorts `keys` (+ a payload) per segment of `seg_len` and compares with numpy, `repeat` times back to back.
    route: 'finish' (top-digit route, buckets fit), 'fallback' (top-digit route enqueued, a bucket did not fit), 'lsd' (the
    route is not taken at all)."""
    kt, vt = KT[kind]
    keys = np.ascontiguousarray(keys, dtype=kt)
    n = keys.size
    vals = payload(kind, n, np.random.RandomState(n % 9973))
    k_in, v_in = be.alloc(keys), be.alloc(vals)
    k_out, v_out = be.alloc(np.zeros(n, kt)), be.alloc(np.zeros(n, vt))
    eng = be.engine
    sorts0, falls0 = eng.get_stat('sort_finish_sorts'), eng.get_stat('sort_finish_fallbacks')
    eng.set_option('sort_big_min', big_min)
    try:
        for _ in range(repeat):
            eng.probe_sort(kind, be.ptr(k_in), be.ptr(k_out), be.ptr(v_in), be.ptr(v_out), n, bits, seg_len=seg_len)
    finally:
        eng.set_option('sort_big_min', BIG_MIN_DEFAULT)
    sorts, falls = eng.get_stat('sort_finish_sorts') - sorts0, eng.get_stat('sort_finish_fallbacks') - falls0
    got_k, got_v = be.get(k_out), be.get(v_out)
    assert np.array_equal(be.get(k_in), keys) and np.array_equal(be.get(v_in), vals)  # inputs intact
    mask = kt((1 << bits) - 1 if bits < 32 else 0xffffffff)
    for s0 in range(0, n, seg_len):
        s1 = min(n, s0 + seg_len)
        order = np.argsort(keys[s0:s1] & mask, kind='stable')
        assert np.array_equal(got_k[s0:s1], keys[s0:s1][order]), (kind, n, bits, seg_len, s0)
        assert np.array_equal(got_v[s0:s1], vals[s0:s1][order]), (kind, n, bits, seg_len, s0)
    want = {'finish': (repeat, 0), 'fallback': (repeat, repeat), 'lsd': (0, 0)}[route]
    assert (sorts, falls) == want, ('route', route, 'sort_finish_sorts / sort_finish_fallbacks moved by', sorts, falls)


def uniform_keys(n, below, seed):
    return np.random.RandomState(seed).randint(0, below, size=n, dtype=np.int64).astype(np.uint32)


# ---- the checks of the emulator suite (sizes <= 30 000 pairs) ----------------------------------------------------------------
def check_segments_and_short_tail(be, kind):
    # three segments of 9000 + a short one of 55, 13 bits (the shape of test_sort_big_tile_shapes_at_small_sizes)
    run_sort(be, kind, uniform_keys(3 * 9000 + 55, 1 << 13, 22), 13, 9000, 'finish')


def check_three_local_rounds(be):
    # 24 bits, u64 payload: whatever top digit is chosen (<= 8 bits) leaves >= 16 bits; keys with all 24 bits in use
    run_sort(be, 1, uniform_keys(20000, 1 << 24, 5), 24, 10000, 'finish')
    # 32 bits: 24 or more bits below the top digit = three or four local rounds
    run_sort(be, 1, uniform_keys(12000, 1 << 32, 6), 32, 6000, 'finish')


def check_uneven_local_digits(be, kind):
    # the bits below the top digit are split into ceil(. / 8) local digits of nearly equal width: for a top digit of 1..8 bits,
    # 19 bits leave 11..18 and 21 bits leave 13..20 -- between them even and uneven splits of two and three digits
    run_sort(be, kind, uniform_keys(2 * 7000 + 333, 1 << 19, 7), 19, 7000, 'finish')
    run_sort(be, kind, uniform_keys(2 * 7000 + 333, 1 << 21, 8), 21, 7000, 'finish')


def bucket_fill_keys(groups, bits, seed):
    """One segment: groups[b] keys whose top byte (of `bits`) is b, low bits random, shuffled.  Top bytes 0, 128 and 255 fall
    into three different buckets of the top digit whatever its width (1..8 bits), and nothing else shares the bucket of 0."""
    rng = np.random.RandomState(seed)
    parts = [(np.uint32(b) << np.uint32(bits - 8)) | rng.randint(0, 1 << (bits - 8), size=s, dtype=np.int64).astype(np.uint32)
             for b, s in sorted(groups.items())]
    keys = np.concatenate(parts)
    rng.shuffle(keys)
    return keys


def check_bucket_at_capacity(be, kind):
    cap = be.engine.get_stat('sort_finish_cap')
    assert cap >= 9120  # mean + 6 sigma of the flagship's item-side buckets
    bits = 16
    # a bucket of EXACTLY cap pairs (the keys with top byte 0), 700 pairs in two other buckets: fits
    run_sort(be, kind, bucket_fill_keys({0: cap, 128: 300, 255: 400}, bits, 11), bits, cap + 700, 'finish')
    # ... and of cap + 1: falls back, result still exact
    run_sort(be, kind, bucket_fill_keys({0: cap + 1, 128: 299, 255: 400}, bits, 12), bits, cap + 700, 'fallback')


def check_empty_and_single_buckets(be, kind):
    # keys whose top byte is 0..2 or 253..255 only: for a top digit of two bits or more the buckets in between are EMPTY
    bits, n = 16, 9000
    rng = np.random.RandomState(13)
    tops = rng.choice(np.array([0, 1, 2, 253, 254, 255], dtype=np.uint32), size=n)
    keys = (tops << np.uint32(bits - 8)) | rng.randint(0, 1 << (bits - 8), size=n, dtype=np.int64).astype(np.uint32)
    run_sort(be, kind, np.concatenate([keys, keys[:100]]), bits, n, 'finish')
    # a last segment of ONE pair: one bucket of one pair, every other bucket of that segment empty
    run_sort(be, kind, uniform_keys(2 * 5000 + 1, 1 << 12, 14), 12, 5000, 'finish')


def check_skew_falls_back(be, kind):
    # 80 % equal keys: one bucket holds most of a segment of 15 000 pairs -- more than the capacity
    rng = np.random.RandomState(15)
    n, seg = 30000, 15000
    keys = uniform_keys(n, 1 << 20, 16)
    keys = np.where(rng.rand(n) < 0.8, np.uint32(12345), keys).astype(np.uint32)
    assert (keys[:seg] == 12345).sum() > be.engine.get_stat('sort_finish_cap')
    run_sort(be, kind, keys, 20, seg, 'fallback')


def check_old_route_untouched(be, kind):
    run_sort(be, kind, uniform_keys(3 * 9000 + 55, 1 << 13, 22), 13, 9000, 'lsd', big_min=1 << 62)
    # not segmented, 8 bits or fewer, u64 keys: the LSD passes whatever the hook says
    eng = be.engine
    s0 = eng.get_stat('sort_finish_sorts')
    from test_emu_sort import check_sort
    try:
        check_sort(be, kind, 9000, 13, seg_len=0, seed=1, cfg=1)
        check_sort(be, kind, 9000, 8, seg_len=4500, seed=2, cfg=1)
        check_sort(be, 2, 9000, 40, seg_len=4500, seed=3, cfg=1)
    finally:
        eng.set_option('sort_big_min', BIG_MIN_DEFAULT)
    assert eng.get_stat('sort_finish_sorts') == s0


def check_repeat(be, kind):
    # the same sort back to back: nothing of one sort's control block leaks into the next (a fitting one behind a fallback too)
    run_sort(be, kind, uniform_keys(2 * 6000, 1 << 14, 17), 14, 6000, 'finish', repeat=3)
    check_skew_falls_back(be, kind)
    run_sort(be, kind, uniform_keys(2 * 6000, 1 << 14, 18), 14, 6000, 'finish')


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('kind', [0, 1])
def test_finish_segments_and_short_tail(be, kind):
    check_segments_and_short_tail(be, kind)


def test_finish_three_local_rounds(be):
    check_three_local_rounds(be)


@pytest.mark.parametrize('kind', [0, 1])
def test_finish_uneven_local_digits(be, kind):
    check_uneven_local_digits(be, kind)


@pytest.mark.parametrize('kind', [0, 1])
def test_finish_bucket_at_capacity(be, kind):
    check_bucket_at_capacity(be, kind)


@pytest.mark.parametrize('kind', [0, 1])
def test_finish_empty_and_single_buckets(be, kind):
    check_empty_and_single_buckets(be, kind)


@pytest.mark.parametrize('kind', [0, 1])
def test_finish_skew_falls_back(be, kind):
    check_skew_falls_back(be, kind)


@pytest.mark.parametrize('kind', [0, 1])
def test_finish_old_route_untouched(be, kind):
    check_old_route_untouched(be, kind)


def test_finish_repeat(be):
    check_repeat(be, 0)
