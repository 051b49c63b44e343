"""Shared checks of the weighted sampler (include/spotlight_hip.h: slk_cdf_guide, slk_sample_items_weighted) against numpy's own
definition, RandomState.choice(num_items, size=count, p=p): ids AND the final (key, pos) bit for bit.  `be` is a backend:
tests/emu_backend.EmuBackend (tests/test_emu_weighted_sampler.py) or tests/hip_backend.HipBackend (tests/test_gpu_weighted_sampler.py).
Nothing here has a tolerance."""
import numpy as np
import pytest

from spotlight_amd import _native

NUM_ITEMS = (1, 2, 7, 1000, 70000)  # 70000 needs more than 16 guide bits
COUNTS = (1, 5, 311, 312, 313, 700, 3000)  # 312 values are exactly one state block of 624 words
WEIGHTS = ('constant', 'zipf_zeros', 'one_hot', 'dynamic_range')


def weights(kind, I):
    """The weight vectors of the checks.  'zipf_zeros': zipf ** 0.75 with every 7th item, the first and the last item at zero --
    at num_items 1 and 2 that would leave no item at all (no distribution), so there the vector stays zipf ** 0.75.
    'dynamic_range': 1e-300 .. 1 in shuffled order: most increments vanish against the running sum, the cdf has long flat
    stretches (and a subnormal-sized start)."""
    if kind == 'constant':
        return np.ones(I)
    if kind == 'zipf_zeros':
        w = (1.0 / np.arange(1, I + 1)) ** 0.75
        z = w.copy()
        z[::7] = 0.0
        z[0] = z[-1] = 0.0
        return z if z.sum() > 0 else w
    if kind == 'one_hot':
        w = np.zeros(I)
        w[I // 3] = 1.0
        return w
    if kind == 'dynamic_range':
        return np.random.RandomState(11).permutation(10.0 ** np.linspace(-300.0, 0.0, I)) if I > 1 else np.ones(1)
    raise ValueError(kind)


def cdf_of(w):
    p = w / w.sum()
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return p, cdf


def start_states():
    mid = np.random.RandomState(1234)
    mid.randint(0, 10, 77)  # mid-block
    return [('mid-block', mid.get_state()), ('pos 624', np.random.RandomState(42).get_state())]  # a fresh state: pos == 624


def same_state(got, ref):
    return (got[1] == ref[1]).all() and got[2] == ref[2]


def guide_bits_cases(eng, I):
    """0 (one bucket: a pure binary search), the automatic value, and a value with K > num_items."""
    auto = eng.cdf_guide_bits(I)  # the smallest K >= num_items: one more bit has K > num_items
    return sorted({0, auto, auto + 1})


class Sampler(object):
    """A cdf and its guide in the backend's memory."""

    def __init__(self, be, w, bits):
        self.be, self.I, self.bits = be, len(w), bits
        self.p, self.cdf = cdf_of(np.asarray(w, np.float64))
        self.d_cdf = be.alloc(self.cdf)
        self.d_guide = be.alloc(np.full((1 << bits) + 1, 0x7fffffff, dtype=np.int32))  # (uint32 entries)
        be.engine.cdf_guide(be.ptr(self.d_cdf), self.I, bits, be.ptr(self.d_guide), be.stream)

    def guide(self):
        return self.be.get(self.d_guide).view(np.uint32).astype(np.int64)

    def draw(self, count):
        out = self.be.alloc(np.full(count, -1, dtype=np.int64))
        self.be.engine.sample_items_weighted(self.be.ptr(self.d_cdf), self.be.ptr(self.d_guide), self.bits, self.I, count,
                                             self.be.ptr(out), self.be.stream)
        return self.be.get(out)


def check_auto_guide_bits(be):
    eng = be.engine
    for I, want in ((1, 0), (2, 1), (3, 2), (7, 3), (8, 3), (9, 4), (1000, 10), (65536, 16), (70000, 17), (1 << 24, 24),
                    ((1 << 24) + 1, 24), (1 << 32, 24)):
        assert eng.cdf_guide_bits(I) == want, (I, eng.cdf_guide_bits(I), want)


def check_bit_exact(be, I, kind):
    """Ids, state and guide against numpy for one (num_items, weights) pair: every guide_bits case, both starting states, the
    successive counts."""
    eng = be.engine
    w = weights(kind, I)
    for bits in guide_bits_cases(eng, I):
        s = Sampler(be, w, bits)
        K = 1 << bits
        want_guide = np.searchsorted(s.cdf, np.arange(K + 1) / K, 'right')
        assert np.array_equal(s.guide(), want_guide), (I, kind, bits)
        for name, state in start_states():
            rs = np.random.RandomState()
            rs.set_state(state)
            eng.rng_set_state(state)
            for count in COUNTS:
                got = s.draw(count)
                want = rs.choice(I, size=count, p=s.p)
                assert np.array_equal(got, want), (I, kind, bits, name, count)
                assert same_state(eng.rng_get_state(), rs.get_state()), (I, kind, bits, name, count)
                assert (w[got] > 0).all(), 'an item of weight zero was drawn'


def check_interleaving(be):
    """uniform, weighted, uniform on ONE ctx == randint, choice, randint from one RandomState; the state after every step."""
    eng = be.engine
    I = 1000
    s = Sampler(be, weights('zipf_zeros', I), eng.cdf_guide_bits(I))
    for name, state in start_states():
        rs = np.random.RandomState()
        rs.set_state(state)
        eng.rng_set_state(state)
        for step, count in enumerate((100, 257, 50, 312, 1)):
            if step % 2 == 0:
                out = be.alloc(np.full(count, -1, dtype=np.int64))
                eng.sample_items(I, count, be.ptr(out), be.stream)
                got, want = be.get(out), rs.randint(0, I, count, dtype=np.int64)
            else:
                got, want = s.draw(count), rs.choice(I, size=count, p=s.p)
            assert np.array_equal(got, want), (name, step)
            assert same_state(eng.rng_get_state(), rs.get_state()), (name, step)


def check_one_item_consumes_two_words(be):
    """num_items == 1: choice() still calls random_sample -- unlike randint(0, 1), which consumes nothing."""
    eng = be.engine
    s = Sampler(be, np.ones(1), 0)
    rs = np.random.RandomState(7)
    eng.rng_set_state(rs.get_state())
    assert (s.draw(10) == 0).all()
    rs.random_sample(10)
    assert same_state(eng.rng_get_state(), rs.get_state())
    out = be.alloc(np.full(10, -1, dtype=np.int64))
    eng.sample_items(1, 10, be.ptr(out), be.stream)
    assert (be.get(out) == 0).all() and same_state(eng.rng_get_state(), rs.get_state())


def check_count_zero(be):
    eng = be.engine
    s = Sampler(be, weights('constant', 7), 3)
    for _, state in start_states():
        eng.rng_set_state(state)
        assert s.draw(0).shape == (0,)
        eng.sample_items_weighted(be.ptr(s.d_cdf), be.ptr(s.d_guide), 3, 7, 0, None, be.stream)  # nothing to write: no buffer needed
        assert same_state(eng.rng_get_state(), state)


def check_split_draws(be):
    """A count beyond the per-draw limit is a run of consecutive draws inside the call: same ids, same state (the limit lowered
    to 100 values through option "weighted_max_values"; 100, 101 and 1000 end on, just behind and well behind a boundary)."""
    eng = be.engine
    I = 1000
    s = Sampler(be, weights('zipf_zeros', I), eng.cdf_guide_bits(I))
    for name, state in start_states():
        rs = np.random.RandomState()
        rs.set_state(state)
        eng.rng_set_state(state)
        with eng.options(weighted_max_values=100):
            for count in (100, 101, 1000, 99):
                assert np.array_equal(s.draw(count), rs.choice(I, size=count, p=s.p)), (name, count)
                assert same_state(eng.rng_get_state(), rs.get_state()), (name, count)


def check_refusals(be):
    eng, P = be.engine, be.ptr
    s = Sampler(be, weights('constant', 7), 3)
    out = be.alloc(np.zeros(4, dtype=np.int64))

    def refused(match, fn):
        with pytest.raises(_native.SlkError, match=match) as e:
            fn()
        assert e.value.code == _native.SLK_EINVAL

    draw = lambda cdf=s.d_cdf, guide=s.d_guide, bits=3, I=7, count=4, o=out: (
        lambda: eng.sample_items_weighted(P(cdf), P(guide), bits, I, count, P(o), be.stream))
    refused('NULL', draw(cdf=None))
    refused('NULL', draw(guide=None))
    refused('NULL', draw(o=None))
    refused('num_items', draw(I=0))
    refused('num_items', draw(I=(1 << 32) + 1))
    refused('negative count', draw(count=-1))
    refused('guide_bits', draw(bits=-1))
    refused('guide_bits', draw(bits=29))
    guide = lambda cdf=s.d_cdf, g=s.d_guide, bits=3, I=7: (lambda: eng.cdf_guide(P(cdf), I, bits, P(g), be.stream))
    refused('NULL', guide(cdf=None))
    refused('NULL', guide(g=None))
    refused('num_items', guide(I=0))
    refused('num_items', guide(I=(1 << 32) + 1))
    refused('guide_bits', guide(bits=-1))
    refused('guide_bits', guide(bits=29))


def check_profiled_as_sample(be):
    eng = be.engine
    s = Sampler(be, weights('constant', 1000), 10)
    eng.rng_set_state(np.random.RandomState(3).get_state())
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        s.draw(700)
        prof = eng.profile_read()
    finally:
        eng.profile_enable(False)
    assert prof['sample'][0] == 1 and all(v[0] == 0 for k, v in prof.items() if k != 'sample'), prof


def check_state_sampled(be):
    """slk_rng_get_state_sampled behind a weighted draw is slk_rng_get_state (the draw records the event it waits for)."""
    eng = be.engine
    I = 1000
    s = Sampler(be, weights('zipf_zeros', I), 10)
    rs = np.random.RandomState(99)
    eng.rng_set_state(rs.get_state())
    assert same_state(eng.rng_get_state_sampled(), rs.get_state())  # nothing drawn yet: the state that was set
    s.draw(500)
    rs.choice(I, size=500, p=s.p)
    sampled = eng.rng_get_state_sampled()
    assert same_state(sampled, rs.get_state()) and same_state(sampled, eng.rng_get_state())
