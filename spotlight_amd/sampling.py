"""Negative sampling (mirrors spotlight/sampling.py:8-36).

`sample_items` is the host numpy form kept for API compatibility.  During fit() the draw
happens on the GPU (csrc/slk_rng.hip) from the very same MT19937 stream, bit-exactly;
`sample_items_device` exposes that path directly.

Uniform negatives are `RandomState.randint`; with item weights (`p`, an `ItemDistribution`) a draw is
`RandomState.choice(num_items, size=shape, p=p)` -- on the device too (slk_sample_items_weighted), bit for bit and with
the RandomState left where numpy leaves it.

Verified negatives (`SeenItems`, `verify_negatives`): of several candidates drawn up front per negative slot, the first one the
user has not interacted with -- slk_verify_negatives on the device, restated here in numpy for one minibatch.
"""
import numpy as np

NEGATIVE_SAMPLING_MODES = ('uniform', 'popularity')


class ItemDistribution(object):
    """Item weights of a non-uniform negative draw: THE place that validates them.

    `weights`: one finite, non-negative number per item with a positive sum (ValueError otherwise -- raised here, before
    anything is drawn from a RandomState).  `p = weights / weights.sum()` in float64 is what numpy's `choice` is given;
    `cdf = p.cumsum(); cdf /= cdf[-1]` is what it searches.  An item of weight zero is never drawn.

    The device side (the float64 cdf, its cutpoint table `guide` and `guide_bits`: include/spotlight_hip.h, slk_cdf_guide)
    is built by `bind`, once per fit(), and is not pickled: the next bind rebuilds it.
    """

    def __init__(self, weights, num_items):
        try:
            w = np.array(weights, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError('negative_sampling weights must be an array of numbers')
        if w.shape[0] != int(num_items):
            raise ValueError('negative_sampling weights must hold one weight per item ({}), got {}'.format(int(num_items), w.shape[0]))
        if not np.isfinite(w).all():
            raise ValueError('negative_sampling weights must be finite')
        if (w < 0).any():
            raise ValueError('negative_sampling weights must be non-negative')
        total = w.sum()
        if not (total > 0 and np.isfinite(total)):
            raise ValueError('negative_sampling weights must have a positive, finite sum')
        self.num_items = int(num_items)
        self.p = w / total
        self.cdf = self.p.cumsum()
        self.cdf /= self.cdf[-1]
        self.guide_bits = None
        self.d_cdf = self.d_guide = None

    @classmethod
    def from_counts(cls, item_ids, num_items, power=0.75, zero=()):
        """word2vec's unigram distribution: weight = count(item) ** power over `item_ids`; the items of `zero` (a sequence
        model's padding item) and every item that does not occur get weight 0."""
        counts = np.bincount(np.asarray(item_ids).reshape(-1), minlength=int(num_items)).astype(np.float64)
        for item in zero:
            counts[item] = 0.0
        return cls(counts ** float(power), num_items)

    def __getstate__(self):
        state = dict(self.__dict__)
        state['d_cdf'] = state['d_guide'] = None  # device tensors: rebuilt by the next bind()
        return state

    def bind(self, engine, device, stream=0, guide_bits=None):
        """The cdf and its guide on `device` (idempotent per device and guide_bits); returns self."""
        import torch
        bits = engine.cdf_guide_bits(self.num_items) if guide_bits is None else int(guide_bits)
        if self.d_cdf is not None and self.d_cdf.device == torch.device(device) and self.guide_bits == bits:
            return self
        d_cdf = torch.from_numpy(self.cdf).to(device)
        d_guide = torch.empty((1 << bits) + 1, dtype=torch.int32, device=device)  # (uint32 entries)
        engine.cdf_guide(d_cdf.data_ptr(), self.num_items, bits, d_guide.data_ptr(), stream)
        if d_cdf.device.type == 'cuda':
            torch.cuda.synchronize(d_cdf.device)  # once per fit(): the draws may run on another stream (the prep lane)
        self.d_cdf, self.d_guide, self.guide_bits = d_cdf, d_guide, bits
        return self

    def sample(self, engine, count, d_out, stream=0):
        """`count` ids to the device address d_out from the engine's RNG state: choice(num_items, size=count, p=self.p)."""
        if self.d_cdf is None:
            raise RuntimeError('ItemDistribution.bind() has not been called')
        engine.sample_items_weighted(self.d_cdf.data_ptr(), self.d_guide.data_ptr(), self.guide_bits, self.num_items, count, d_out,
                                     stream)


VERIFY_TRIES_MAX = 16  # include/spotlight_hip.h: slk_verify_negatives


def check_verify_tries(verify_tries):
    """The constructor-time check of a model's `verify_tries` argument: an int in [1, VERIFY_TRIES_MAX]."""
    if (isinstance(verify_tries, bool) or not isinstance(verify_tries, (int, np.integer))
            or not 1 <= verify_tries <= VERIFY_TRIES_MAX):
        raise ValueError('verify_tries must be an int in [1, {}], got {!r}'.format(VERIFY_TRIES_MAX, verify_tries))
    return int(verify_tries)


class SeenItems(object):
    """The users' histories that verified negatives are checked against (`verify_negatives=True`): the (user, item) pairs of
    the fit() call in progress as a CSR over users -- int64 offsets [num_users + 1], int64 items ascending inside a user's
    segment, duplicates kept (include/spotlight_hip.h: slk_verify_negatives).

    `from_interactions` validates; `bind` builds the CSR on the device, once per fit(); `csr()` is the same CSR on the host,
    built on first use (the numpy restatement `verify_negatives` reads it).  The device tensors are not pickled: the next
    bind rebuilds them."""

    def __init__(self, user_ids, item_ids, num_users, num_items):
        self.user_ids, self.item_ids = user_ids, item_ids
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.d_off = self.d_items = None
        self._csr = self._keys = None

    @classmethod
    def from_interactions(cls, user_ids, item_ids, num_users, num_items):
        """ValueError unless the two id arrays are one-dimensional integer arrays of one length with every id in range."""
        user_ids, item_ids = np.asarray(user_ids), np.asarray(item_ids)
        if user_ids.ndim != 1 or item_ids.ndim != 1 or len(user_ids) != len(item_ids):
            raise ValueError('verify_negatives: one user id and one item id per interaction are needed')
        for name, ids, bound in (('user', user_ids, num_users), ('item', item_ids, num_items)):
            if ids.dtype.kind not in 'iu':
                raise ValueError('verify_negatives: {} ids must be integers'.format(name))
            if ids.size and (ids.min() < 0 or ids.max() >= int(bound)):
                raise ValueError('verify_negatives: {} ids must be in [0, {})'.format(name, int(bound)))
        return cls(user_ids, item_ids, num_users, num_items)

    def __len__(self):
        return len(self.user_ids)

    def __getstate__(self):
        state = dict(self.__dict__)
        state['d_off'] = state['d_items'] = None  # device tensors: rebuilt by the next bind()
        state['_csr'] = state['_keys'] = None  # (and the host forms by their next use)
        return state

    def csr(self):
        """(offsets int64 [num_users + 1], items int64) on the host."""
        if self._csr is None:
            users = np.asarray(self.user_ids, dtype=np.int64)
            items = np.asarray(self.item_ids, dtype=np.int64)
            order = np.lexsort((items, users))
            off = np.zeros(self.num_users + 1, dtype=np.int64)
            np.cumsum(np.bincount(users, minlength=self.num_users), out=off[1:])
            self._csr = (off, np.ascontiguousarray(items[order]))
        return self._csr

    def packed_keys(self):
        """The pairs as ascending int64 keys user * num_items + item (host; what `verify_negatives` searches)."""
        if self._keys is None:
            self._keys = _packed_keys(*self.csr(), self.num_items)
        return self._keys

    def bind(self, engine, device, stream=0, ids=None):
        """The CSR on `device` (idempotent per device); returns self.  `ids`: the (users, items) int64 tensors if they are on
        the device already.  Set-up, not the epoch path: one sort of the packed key user * num_items + item (two stable sorts
        where the key does not fit 63 bits), stock tensor ops on the device."""
        import torch
        device = torch.device(device)
        if self.d_off is not None and self.d_off.device == device:
            return self
        if ids is None:
            ids = [torch.from_numpy(np.ascontiguousarray(a).astype(np.int64, copy=False)).to(device)
                   for a in (self.user_ids, self.item_ids)]
        users, items = ids
        if self.num_users * self.num_items < 1 << 63:
            key = torch.sort(users * self.num_items + items).values
            d_items = key % self.num_items
            bounds = torch.arange(self.num_users + 1, dtype=torch.int64, device=device) * self.num_items
            d_off = torch.searchsorted(key, bounds)
        else:
            by_item = torch.sort(items, stable=True)
            by_user = torch.sort(users[by_item.indices], stable=True)
            d_items = by_item.values[by_user.indices]
            d_off = torch.searchsorted(by_user.values, torch.arange(self.num_users + 1, dtype=torch.int64, device=device))
        if device.type == 'cuda':
            torch.cuda.synchronize(device)  # once per fit(): the kernel may run on another stream (the prep lane)
        self.d_off, self.d_items = d_off.contiguous(), d_items.contiguous()
        return self


def _packed_keys(off, items, span):
    """The (user, item) pairs of a CSR as ascending packed keys user * span + item."""
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    return rows * span + items[:len(rows)]


def verify_negatives(candidates, users, seen, n_neg, tries):
    """The rule of slk_verify_negatives (include/spotlight_hip.h) for ONE minibatch, in numpy: `candidates` are the
    tries * n_neg * bm ids of one draw for the bm `users` (viewed [tries][n_neg][bm]), `seen` a SeenItems or an
    (offsets, items) CSR.  Returns (negatives int64 [n_neg, bm], replaced, unresolved): per slot the first attempt's candidate
    that is not in the user's history -- attempt 0's, counted as unresolved, if every attempt is."""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    bm = users.shape[0]
    cand = np.asarray(candidates, dtype=np.int64).reshape(int(tries), int(n_neg), bm)
    if isinstance(seen, SeenItems):
        span, keys = seen.num_items, seen.packed_keys()
    else:
        off, items = np.asarray(seen[0], dtype=np.int64), np.asarray(seen[1], dtype=np.int64)
        span = int(max(items.max() if items.size else 0, cand.max() if cand.size else 0)) + 1
        keys = _packed_keys(off, items, span)
    query = users[None, None, :] * span + cand
    if len(keys):
        at = np.minimum(np.searchsorted(keys, query), len(keys) - 1)
        unseen = keys[at] != query
    else:
        unseen = np.ones(cand.shape, dtype=bool)
    resolved = unseen.any(axis=0)
    first = np.where(resolved, unseen.argmax(axis=0), 0)  # the smallest attempt with an unseen candidate
    out = np.take_along_axis(cand, first[None], axis=0)[0]
    return out, int((first > 0).sum()), int((~resolved).sum())


def check_negative_sampling(negative_sampling):
    """The constructor-time check of a model's `negative_sampling` argument (the weights themselves are checked by
    ItemDistribution at fit(), when num_items is known)."""
    if isinstance(negative_sampling, str) and negative_sampling not in NEGATIVE_SAMPLING_MODES:
        raise ValueError("negative_sampling must be 'uniform', 'popularity', None or an array of item weights, got {!r}"
                         .format(negative_sampling))


def is_uniform(negative_sampling):
    return negative_sampling is None or (isinstance(negative_sampling, str) and negative_sampling == 'uniform')


def item_distribution(negative_sampling, power, num_items, item_ids, zero=()):
    """None for uniform sampling, else the ItemDistribution of a model's `negative_sampling` argument over the item ids
    of the fit() call in progress."""
    check_negative_sampling(negative_sampling)
    if is_uniform(negative_sampling):
        return None
    if isinstance(negative_sampling, str):  # 'popularity'
        return ItemDistribution.from_counts(item_ids, num_items, power, zero)
    return ItemDistribution(negative_sampling, num_items)


def draw_items(engine, num_items, count, d_out, stream=0, dist=None):
    """`count` negatives to the device address d_out from the engine's RNG state: uniform (slk_sample_items), or from the
    bound ItemDistribution `dist` (slk_sample_items_weighted)."""
    if dist is None:
        engine.sample_items(num_items, count, d_out, stream=stream)
    else:
        dist.sample(engine, count, d_out, stream)


def _p_of(p, num_items):
    return p.p if isinstance(p, ItemDistribution) else ItemDistribution(p, num_items).p


def sample_items(num_items, shape, random_state=None, p=None):
    """Uniform item ids (`randint`), or with `p` (item weights or an ItemDistribution)
    `random_state.choice(num_items, size=shape, p=weights / weights.sum())`."""
    if p is not None:
        p = _p_of(p, num_items)  # (validated before anything is drawn)
    if random_state is None:
        random_state = np.random.RandomState()
    if p is not None:
        return random_state.choice(num_items, size=shape, p=p).astype(np.int64, copy=False)
    return random_state.randint(0, num_items, shape, dtype=np.int64)


def sample_items_device(num_items, shape, random_state, engine=None, device=None, p=None):
    """Same ids as `sample_items`, drawn by the gfx950 sampler; returns an int64 tensor on the
    HIP device and advances `random_state` exactly as numpy would have."""
    import torch

    from spotlight_amd import _native
    dist = None
    if p is not None:
        dist = p if isinstance(p, ItemDistribution) else ItemDistribution(p, num_items)
    engine = engine or _native.Engine(torch.cuda.current_device())
    count = int(np.prod(shape))
    out = torch.empty(count, dtype=torch.int64, device=device or 'cuda')
    stream = torch.cuda.current_stream().cuda_stream if out.device.type == 'cuda' else 0
    if dist is not None:
        dist.bind(engine, out.device, stream)
    engine.rng_set_state(random_state.get_state())
    draw_items(engine, num_items, count, out.data_ptr(), stream, dist)
    random_state.set_state(engine.rng_get_state())
    return out.view(shape)
