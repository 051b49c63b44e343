"""`-m gpu` twin of tests/test_emu_sort_finish.py: the radix sort's top-digit route on the device, at the smallest shapes
that still have the flagship's bucket fill (C2: item ids below 10^6 in segments of 2^21 occurrences, 245 of 256 buckets of
~8559 pairs; user ids below 10^7 in segments of 2^20, 153 buckets of ~6854), plus every check of the emulator file."""
import numpy as np
import pytest

import test_emu_sort_finish as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


def test_item_side_fill_takes_the_finish(be):
    # kind 0, 20 bits, keys uniform below 10^6: two segments of 2^21 + one of 300 001; the largest bucket stays under the
    # capacity (8828 here), so the sort must NOT fall back
    seg = 1 << 21
    keys = F.uniform_keys(2 * seg + 300001, 10 ** 6, 31)
    assert np.bincount(keys[:seg] >> 12).max() < be.engine.get_stat('sort_finish_cap')
    F.run_sort(be, 0, keys, 20, seg, 'finish', big_min=1 << 20)


def test_user_side_fill_takes_the_finish(be):
    # kind 1, 24 bits, keys uniform below 10^7: two segments of 2^20 + one of 300 001 (max bucket 7074 here)
    seg = 1 << 20
    keys = F.uniform_keys(2 * seg + 300001, 10 ** 7, 32)
    assert np.bincount(keys[:seg] >> 16).max() < be.engine.get_stat('sort_finish_cap')
    F.run_sort(be, 1, keys, 24, seg, 'finish', big_min=1 << 20)


def test_zipf_items_fall_back(be):
    # Zipf(1.0) item ids of one 2^21 segment: the head items' bucket holds most of it
    seg, items = 1 << 21, 10 ** 6
    w = 1.0 / np.arange(1, items + 1)
    cdf = np.cumsum(w / w.sum())
    keys = np.searchsorted(cdf, np.random.RandomState(33).rand(seg)).clip(0, items - 1).astype(np.uint32)
    assert np.bincount(keys >> 12).max() > be.engine.get_stat('sort_finish_cap')
    F.run_sort(be, 0, keys, 20, seg, 'fallback', big_min=1 << 20)


def test_same_sort_five_times(be):
    seg = 1 << 18
    F.run_sort(be, 0, F.uniform_keys(2 * seg + 4097, 10 ** 6, 34), 20, seg, 'finish', repeat=5)
    F.run_sort(be, 1, F.uniform_keys(2 * seg + 4097, 10 ** 7, 35), 24, seg, 'finish', repeat=5)


@pytest.mark.parametrize('kind', [0, 1])
def test_emulator_checks_on_the_device(be, kind):
    F.check_segments_and_short_tail(be, kind)
    F.check_uneven_local_digits(be, kind)
    F.check_bucket_at_capacity(be, kind)
    F.check_empty_and_single_buckets(be, kind)
    F.check_skew_falls_back(be, kind)
    F.run_sort(be, kind, F.uniform_keys(3 * 9000 + 55, 1 << 13, 22), 13, 9000, 'lsd', big_min=1 << 62)
    F.check_repeat(be, kind)
    if kind == 1:
        F.check_three_local_rounds(be)
