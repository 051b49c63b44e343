"""Shared checks of verified negatives (include/spotlight_hip.h: slk_verify_negatives; the models' `verify_negatives` keyword).

Kernel checks take a backend `be` -- tests/emu_backend.EmuBackend (tests/test_emu_verify_negatives.py) or
tests/hip_backend.HipBackend (tests/test_gpu_verify_negatives.py) -- and compare ids and counters with the numpy restatement
spotlight_amd.sampling.verify_negatives, which tests/test_host_verify_negatives.py in turn holds against a loop over Python
sets.  Model checks run through the emulator (tests/test_host_verify_negatives.py points the device hooks of
factorization/implicit.py at it) and on the gfx950 library.  Every comparison is exact: nothing here has a tolerance."""
import functools
import io

import numpy as np
import pytest
import torch

import negative_sampling_checks as nc
import weighted_sampler_checks as wc
from spotlight_amd import _native
from spotlight_amd import sampling
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.interactions import Interactions
from spotlight_amd.sampling import SeenItems, sample_items
from spotlight_amd.torch_utils import shuffle

BATCHES = (1, 63, 64, 65, 257, 1000)  # both sides of a wavefront (64) and of a workgroup (256); several workgroups
N_NEG = (1, 3, 5)
TRIES = (1, 2, 4, 16)
NUM_ITEMS = (1, 2, 7, 333, 100003)


# ---- histories ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def histories(num_items, seed=0):
    """A CSR (offsets, items) whose users cover: an empty history, one of length 1, one holding every item, one with
    duplicates, lengths 2^k - 1, 2^k, 2^k + 1 (k = 1 .. 6; drawn with replacement, so duplicates occur and a length may exceed
    num_items), the catalogue without its first and last item (candidates below a segment's first and above its last element)
    and the first / last item alone.  An empty history also closes the CSR (an empty LAST segment)."""
    rs = np.random.RandomState(seed)
    segs = [[], [rs.randint(0, num_items)], list(range(num_items)), sorted([num_items // 2] * 3 + [0, 0, num_items - 1]),
            list(range(1, num_items - 1)), [0], [num_items - 1]]
    for k in range(1, 7):
        for length in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            segs.append(sorted(rs.randint(0, num_items, length).tolist()))
    segs.append([])
    off = np.zeros(len(segs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in segs])
    items = np.array([x for s in segs for x in s], dtype=np.int64)
    return off, items


def dense_histories(seed=0):
    """The designated dense case: 7 items, every user has seen 5 to 7 of them."""
    rs = np.random.RandomState(seed)
    segs = [sorted(rs.permutation(7)[:5 + u % 3].tolist()) for u in range(12)]
    off = np.zeros(len(segs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in segs])
    return off, np.array([x for s in segs for x in s], dtype=np.int64)


def candidates_for(seed, users, n, bsz, nn, T, num_items, seen):
    """Uniform candidates in the kernel's layout, with planted values in attempt 0 of every minibatch's first row: the
    segment's first and last element (seen) and their outer neighbours first - 1 / last + 1 where the catalogue has them."""
    off, items = seen
    rs = np.random.RandomState(seed)
    cand = rs.randint(0, num_items, n * nn * T).astype(np.int64)
    for m0 in range(0, n, bsz):
        bm = min(bsz, n - m0)
        block = cand[m0 * nn * T:(m0 + bm) * nn * T].reshape(T, nn, bm)
        for c in range(bm):
            lo, hi = off[users[m0 + c]], off[users[m0 + c] + 1]
            if lo == hi:
                continue
            first, last = items[lo], items[hi - 1]
            block[0, 0, c] = (first, last, max(first - 1, 0), min(last + 1, num_items - 1))[c % 4]
    return cand


def restate(cand, users, seen, n, bsz, nn, T):
    """The numpy restatement over an epoch: per minibatch sampling.verify_negatives on its candidate block, the blocks at the
    contract's offsets.  Returns (negatives [n * nn], replaced, unresolved)."""
    out, replaced, unresolved = np.empty(n * nn, dtype=np.int64), 0, 0
    for m0 in range(0, n, bsz):
        bm = min(bsz, n - m0)
        picked, r, u = sampling.verify_negatives(cand[m0 * nn * T:(m0 + bm) * nn * T], users[m0:m0 + bm], seen, nn, T)
        assert picked.shape == (nn, bm)
        out[m0 * nn:(m0 + bm) * nn] = picked.reshape(-1)
        replaced, unresolved = replaced + r, unresolved + u
    return out, replaced, unresolved


def brute_force(cand, users, seen, n, bsz, nn, T):
    """The rule again, slot by slot over Python sets: (negatives, attempt used per slot; -1: unresolved)."""
    off, items = seen
    sets = [set(items[off[u]:off[u + 1]].tolist()) for u in range(len(off) - 1)]
    out, attempt = np.empty(n * nn, dtype=np.int64), np.empty(n * nn, dtype=np.int64)
    for m0 in range(0, n, bsz):
        bm = min(bsz, n - m0)
        for r in range(nn):
            for c in range(bm):
                tries = [cand[m0 * nn * T + (a * nn + r) * bm + c] for a in range(T)]
                ok = [a for a in range(T) if tries[a] not in sets[users[m0 + c]]]
                slot = m0 * nn + r * bm + c
                out[slot], attempt[slot] = (tries[ok[0]], ok[0]) if ok else (tries[0], -1)
    return out, attempt


class Device(object):
    """A CSR in the backend's memory, and one kernel call over host arrays."""

    def __init__(self, be, seen):
        self.be, self.num_users = be, len(seen[0]) - 1
        self.d_off = be.alloc(seen[0])
        self.d_items = be.alloc(seen[1] if len(seen[1]) else np.zeros(1, dtype=np.int64))

    def run(self, users, cand, n, bsz, nn, T, counts=True, fill=-7):
        be = self.be
        d_users, d_cand = be.alloc(users), be.alloc(cand)
        d_out = be.alloc(np.full(max(n * nn, 1), fill, dtype=np.int64))
        d_counts = be.alloc(np.zeros(2, dtype=np.int64)) if counts else None
        be.engine.verify_negatives(be.ptr(d_users), n, bsz, nn, T, be.ptr(d_cand), be.ptr(self.d_off), be.ptr(self.d_items),
                                   self.num_users, be.ptr(d_out), be.ptr(d_counts), be.stream)
        return be.get(d_out)[:n * nn], (tuple(int(x) for x in be.get(d_counts)) if counts else None)


def n_for(bm):
    return 2 * bm + max(1, bm // 3)  # two full minibatches and a short one (bm == 1: three of one)


# ---- 1. the kernel against the restatement --------------------------------------------------------------------------------------
def check_kernel_equals_restatement(be, bm):
    """Every (n_neg, tries, num_items) at minibatch size bm: ids and both counters."""
    n = n_for(bm)
    for num_items in NUM_ITEMS:
        seen = histories(num_items)
        dev = Device(be, seen)
        users = np.random.RandomState(bm).randint(0, dev.num_users, n).astype(np.int64)
        for nn in N_NEG:
            for T in TRIES:
                cand = candidates_for(nn * 100 + T, users, n, bm, nn, T, num_items, seen)
                want, replaced, unresolved = restate(cand, users, seen, n, bm, nn, T)
                got, counts = dev.run(users, cand, n, bm, nn, T)
                assert np.array_equal(got, want), (bm, num_items, nn, T)
                assert counts == (replaced, unresolved), (bm, num_items, nn, T, counts, replaced, unresolved)
                if T == 1:
                    assert np.array_equal(got, cand) and replaced == 0


def dense_case(seed=3):
    """65-wide minibatches over the dense histories, tries = 4, n_neg = 3.  Asserted on the restatement alone, before any
    kernel runs: some slots are replaced, some unresolved, and outputs come from attempt 0, a middle attempt and the last."""
    seen = dense_histories()
    n, bsz, nn, T = 150, 65, 3, 4
    rs = np.random.RandomState(seed)
    users = rs.randint(0, len(seen[0]) - 1, n).astype(np.int64)
    cand = rs.randint(0, 7, n * nn * T).astype(np.int64)
    want, replaced, unresolved = restate(cand, users, seen, n, bsz, nn, T)
    slow, attempt = brute_force(cand, users, seen, n, bsz, nn, T)
    assert np.array_equal(want, slow)
    assert replaced > 0 and unresolved > 0
    assert replaced == (attempt > 0).sum() and unresolved == (attempt < 0).sum()
    assert (attempt == 0).any() and ((attempt > 0) & (attempt < T - 1)).any() and (attempt == T - 1).any()
    return seen, users, cand, (n, bsz, nn, T), want, (replaced, unresolved)


def check_dense_case(be):
    seen, users, cand, shape, want, totals = dense_case()
    got, counts = Device(be, seen).run(users, cand, *shape)
    assert np.array_equal(got, want) and counts == totals
    # the counters are ADDED to: a second call on the same buffer doubles them; without a buffer the ids are the same
    dev = Device(be, seen)
    d_counts = be.alloc(np.array([5, 7], dtype=np.int64))
    d_users, d_cand, d_out = be.alloc(users), be.alloc(cand), be.alloc(np.zeros(want.size, dtype=np.int64))
    n, bsz, nn, T = shape
    be.engine.verify_negatives(be.ptr(d_users), n, bsz, nn, T, be.ptr(d_cand), be.ptr(dev.d_off), be.ptr(dev.d_items), dev.num_users,
                               be.ptr(d_out), be.ptr(d_counts), be.stream)
    assert tuple(be.get(d_counts)) == (5 + totals[0], 7 + totals[1])
    got, counts = dev.run(users, cand, *shape, counts=False)
    assert counts is None and np.array_equal(got, want)


def check_empty_call_and_batch_beyond_n(be):
    seen, users, cand, (n, bsz, nn, T), want, totals = dense_case()
    dev = Device(be, seen)
    got, counts = dev.run(users, cand, 0, bsz, nn, T)  # n == 0: nothing is written, nothing counted
    assert got.size == 0 and counts == (0, 0)
    d_out = be.alloc(np.full(4, -7, dtype=np.int64))
    be.engine.verify_negatives(None, 0, bsz, nn, T, None, None, None, 0, be.ptr(d_out), None, be.stream)  # (no buffer needed)
    assert (be.get(d_out) == -7).all()
    # a batch size beyond n is one short minibatch
    one, r1, u1 = restate(cand, users, seen, n, n, nn, T)
    got, counts = dev.run(users, cand, n, 1 << 62, nn, T)
    assert np.array_equal(got, one) and counts == (r1, u1)


def check_refusals(be):
    """Every refusal is SLK_EINVAL, and the ctx works afterwards."""
    seen, users, cand, (n, bsz, nn, T), want, totals = dense_case()
    dev = Device(be, seen)
    eng, P = be.engine, be.ptr
    d_users, d_cand, d_out = be.alloc(users), be.alloc(cand), be.alloc(np.zeros(n * nn, dtype=np.int64))

    def call(users=d_users, n=n, bsz=bsz, nn=nn, T=T, cand=d_cand, off=dev.d_off, items=dev.d_items, out=d_out, out_ptr=None):
        return lambda: eng.verify_negatives(P(users), n, bsz, nn, T, P(cand), P(off), P(items), dev.num_users,
                                            out_ptr if out_ptr is not None else P(out), None, be.stream)

    def refused(match, fn):
        with pytest.raises(_native.SlkError, match=match) as e:
            fn()
        assert e.value.code == _native.SLK_EINVAL

    for name in ('users', 'cand', 'off', 'items', 'out'):
        refused('NULL', call(**{name: None}))
    refused('tries', call(T=0))
    refused('tries', call(T=17))
    refused('n_neg', call(nn=0))
    refused('batch_size', call(bsz=0))
    refused('negative n', call(n=-1))
    refused('overlaps', call(out_ptr=P(d_cand)))  # in place
    refused('overlaps', call(out_ptr=P(d_cand) + 8 * (n * nn * T - 1)))  # the output's first element is the candidates' last
    refused('overlaps', call(cand=d_out))
    call()()
    assert np.array_equal(be.get(d_out), want)


def check_draw_then_verify_leaves_numpys_state(be, weighted):
    """The T-fold draw on the engine followed by the kernel: the ids of the restatement over numpy's own draws, per minibatch
    sample_items(num_items, (T * nn, bm)), and numpy's RandomState afterwards."""
    eng = be.engine
    num_items, n, bsz, nn, T = 333, 150, 64, 3, 4
    seen = histories(num_items)
    dev = Device(be, seen)
    users = np.random.RandomState(8).randint(0, dev.num_users, n).astype(np.int64)
    sampler = wc.Sampler(be, wc.weights('zipf_zeros', num_items), eng.cdf_guide_bits(num_items)) if weighted else None
    for name, state in wc.start_states():
        rs = np.random.RandomState()
        rs.set_state(state)
        eng.rng_set_state(state)
        d_cand = be.alloc(np.full(n * nn * T, -1, dtype=np.int64))
        if weighted:
            eng.sample_items_weighted(be.ptr(sampler.d_cdf), be.ptr(sampler.d_guide), sampler.bits, num_items, n * nn * T,
                                      be.ptr(d_cand), be.stream)
        else:
            eng.sample_items(num_items, n * nn * T, be.ptr(d_cand), be.stream)
        d_users, d_out = be.alloc(users), be.alloc(np.zeros(n * nn, dtype=np.int64))
        d_counts = be.alloc(np.zeros(2, dtype=np.int64))
        eng.verify_negatives(be.ptr(d_users), n, bsz, nn, T, be.ptr(d_cand), be.ptr(dev.d_off), be.ptr(dev.d_items), dev.num_users,
                             be.ptr(d_out), be.ptr(d_counts), be.stream)
        blocks = [sample_items(num_items, (T * nn, min(bsz, n - m0)), random_state=rs, p=sampler.p if weighted else None)
                  for m0 in range(0, n, bsz)]
        cand = np.concatenate([b.reshape(-1) for b in blocks])
        assert np.array_equal(be.get(d_cand), cand), name
        want, replaced, unresolved = restate(cand, users, seen, n, bsz, nn, T)
        assert np.array_equal(be.get(d_out), want) and tuple(be.get(d_counts)) == (replaced, unresolved), name
        assert wc.same_state(eng.rng_get_state(), rs.get_state()), name


def check_profiled_as_sample(be):
    eng = be.engine
    seen, users, cand, shape, want, totals = dense_case()
    dev = Device(be, seen)
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        dev.run(users, cand, *shape)
        prof = eng.profile_read()
    finally:
        eng.profile_enable(False)
    assert prof['sample'][0] == 1 and all(v[0] == 0 for k, v in prof.items() if k != 'sample'), prof


# ---- 2. the restatement itself (host only) -------------------------------------------------------------------------------------
def check_restatement_against_sets():
    dense_case()
    for num_items in (1, 2, 7, 333):
        seen = histories(num_items)
        n, bsz, nn, T = 45, 20, 3, 4
        users = np.random.RandomState(num_items).randint(0, len(seen[0]) - 1, n).astype(np.int64)
        cand = candidates_for(1, users, n, bsz, nn, T, num_items, seen)
        want, replaced, unresolved = restate(cand, users, seen, n, bsz, nn, T)
        slow, attempt = brute_force(cand, users, seen, n, bsz, nn, T)
        assert np.array_equal(want, slow) and replaced == (attempt > 0).sum() and unresolved == (attempt < 0).sum()


def check_seen_items_class():
    users = np.array([3, 0, 3, 3, 1, 0], dtype=np.int32)
    items = np.array([5, 2, 1, 5, 0, 2], dtype=np.int32)
    seen = SeenItems.from_interactions(users, items, 5, 6)
    off, its = seen.csr()
    assert off.dtype == np.int64 and its.dtype == np.int64
    assert off.tolist() == [0, 2, 3, 3, 6, 6] and its.tolist() == [2, 2, 0, 1, 5, 5]  # duplicates kept, users 2 and 4 empty
    # a SeenItems and its CSR are the same thing to the restatement
    cand = np.array([2, 0, 5, 1, 4, 4, 4, 0], dtype=np.int64)  # [tries 2][n_neg 1][bm 4]
    for form in (seen, (off, its)):
        out, replaced, unresolved = sampling.verify_negatives(cand, np.array([0, 1, 3, 2]), form, 1, 2)
        assert out.tolist() == [[4, 4, 4, 1]] and (replaced, unresolved) == (3, 0)
    bad = [((users, items[:-1]), 'one user id and one item id'), ((users.astype(np.float32), items), 'integers'),
           ((users, np.where(items == 5, 6, items)), r'item ids must be in \[0, 6\)'), ((users - 1, items), 'user ids must be in')]
    for args, match in bad:
        with pytest.raises(ValueError, match=match):
            SeenItems.from_interactions(*args, 5, 6)


def check_seen_items_bind(engine, device):
    """The device CSR is the host CSR, by either sort; bind is idempotent and the device side is not pickled."""
    import pickle
    rs = np.random.RandomState(5)
    users, items = rs.randint(0, 50, 700).astype(np.int32), rs.randint(0, 33, 700).astype(np.int32)
    for num_items in (33, 1 << 60):  # (a catalogue of 2^60 items: the packed key does not fit 63 bits, two stable sorts)
        seen = SeenItems.from_interactions(users, items, 50, num_items)
        assert seen.bind(engine, device) is seen
        assert seen.d_off.dtype == torch.int64 and seen.d_items.dtype == torch.int64 and seen.d_off.device.type == torch.device(device).type
        assert np.array_equal(seen.d_off.cpu().numpy(), seen.csr()[0]) and np.array_equal(seen.d_items.cpu().numpy(), seen.csr()[1])
        kept = seen.d_off
        assert seen.bind(engine, device).d_off is kept
        clone = pickle.loads(pickle.dumps(seen))
        assert clone.d_off is None and clone.d_items is None and np.array_equal(clone.csr()[1], seen.csr()[1])


# ---- 3. the models ------------------------------------------------------------------------------------------------------------------
U, I, N, B, EPOCHS, NN, T = nc.U, nc.I, nc.N, nc.B, nc.EPOCHS, nc.NN, 3
LOSSES = ('bpr', 'adaptive_hinge', 'warp')
VARIANTS = ('alone', 'use_weights', 'popularity')


def dataset(weights=False):
    inter = nc.dataset()
    if weights:
        inter.weights = np.random.RandomState(6).uniform(0.5, 2.0, N).astype(np.float32)
    return inter


def variant_kw(variant):
    return {'alone': {}, 'use_weights': {'use_weights': True}, 'popularity': {'negative_sampling': 'popularity'}}[variant]


def replay(inter, seed, loss, tries, p=None, weights=None):
    """The stream of a verifying fit() on the host: the constructor's draw, then per epoch the reference's shuffle and per
    minibatch ONE draw of tries * nn * bm candidates and the restatement.  Returns (RandomState, epochs of (users, items,
    weights, negatives), totals {'candidates', 'replaced', 'unresolved'}, unresolved slots per epoch)."""
    nn = NN if loss in host.COLUMN_LOSSES else 1
    seen = SeenItems.from_interactions(inter.user_ids, inter.item_ids, U, I)
    rs = np.random.RandomState(seed)
    rs.randint(-10**8, 10**8)
    epochs, totals = [], {'candidates': 0, 'replaced': 0, 'unresolved': 0}
    for _ in range(EPOCHS):
        arrays = shuffle(*((inter.user_ids, inter.item_ids) + ((weights,) if weights is not None else ())), random_state=rs)
        users = arrays[0].astype(np.int64)
        negs = []
        for lo in range(0, N, B):
            bm = len(users[lo:lo + B])
            cand = sample_items(I, (tries * nn, bm), random_state=rs, p=p)
            picked, replaced, unresolved = sampling.verify_negatives(cand, users[lo:lo + bm], seen, nn, tries)
            negs.append(picked.reshape(-1))
            totals['candidates'] += cand.size
            totals['replaced'] += replaced
            totals['unresolved'] += unresolved
        epochs.append((users, arrays[1].astype(np.int64), arrays[2] if weights is not None else None, np.concatenate(negs)))
    return rs, epochs, totals


def false_negatives(inter, users, negs, nn):
    """How many of an epoch's negatives (per minibatch [nn][bm]) are in their user's history."""
    sets = [set() for _ in range(U)]
    for u, i in zip(inter.user_ids, inter.item_ids):
        sets[u].add(int(i))
    count = 0
    for lo in range(0, N, B):
        bm = len(users[lo:lo + B])
        block = negs[lo * nn:(lo + bm) * nn].reshape(nn, bm)
        count += sum(int(block[r, c]) in sets[users[lo + c]] for r in range(nn) for c in range(bm))
    return count


def check_fit_equals_restated_hand_in(monkeypatch, loss, variant, seed=21):
    """A verifying fit() == the training entry handed the restatement's negatives: tables, RandomState, the counters, the
    negatives themselves -- none of which is in its user's history but the unresolved ones."""
    inter = dataset(weights=variant == 'use_weights')
    kw = dict(variant_kw(variant), verify_negatives=True, verify_tries=T)
    nn = NN if loss in host.COLUMN_LOSSES else 1
    rec = nc.Recorded(monkeypatch, host._ImplicitEpochs, lambda job, e: job.slots[e % len(job.slots)][2])
    model = nc.model_for(loss, seed, **kw)
    model.fit(inter)
    assert not model._autograd_route

    p = nc.popularity_p(inter.item_ids, I) if variant == 'popularity' else None
    weights = inter.weights if variant == 'use_weights' else None
    rs, epochs, totals = replay(inter, seed, loss, T, p, weights)
    assert totals['replaced'] > 0 and totals['unresolved'] > 0 and totals['candidates'] == EPOCHS * N * nn * T  # (not vacuous)
    assert model.negative_verification_ == totals
    assert len(rec.epochs) == EPOCHS
    wrong = 0
    for got, (users, _, _, negs) in zip(rec.epochs, epochs):
        assert np.array_equal(got, negs)
        wrong += false_negatives(inter, users, got, nn)
    assert wrong == totals['unresolved']

    twin = nc.model_for(loss, seed, **kw)
    twin._initialize(inter)
    binding = twin._bind()
    device = twin._net.tables()[0].device
    engine, stream = host._engine_for(device), host._stream_for(device)
    mb_loss = torch.empty((N + B - 1) // B, dtype=torch.float32, device=device)
    before = nc.tables_of(twin)
    with host.fit_scope(twin):
        for users, items, w, negs in epochs:
            d_u, d_i, d_n = [torch.from_numpy(a).to(device) for a in (users, items, negs)]
            ostruct = binding.as_struct()
            if w is not None:
                d_w = torch.from_numpy(np.ascontiguousarray(w)).to(device)
                engine.bilinear_train_weighted(twin._slk_tables(), ostruct, d_u.data_ptr(), d_i.data_ptr(), d_w.data_ptr(), N, B, loss,
                                               NN, mb_loss.data_ptr(), d_neg_in=d_n.data_ptr(), stream=stream)
            else:
                engine.bilinear_train(twin._slk_tables(), ostruct, d_u.data_ptr(), d_i.data_ptr(), N, B, loss, NN, mb_loss.data_ptr(),
                                      d_neg_in=d_n.data_ptr(), stream=stream)
            binding.store_steps(ostruct.step)
            engine.check()
    for t, (x, y) in enumerate(zip(nc.tables_of(model), nc.tables_of(twin))):
        assert nc.same_bits(x, y), (loss, variant, 'table', t)
    assert not nc.same_bits(nc.tables_of(twin)[1], before[1])
    assert nc.same_state(model._random_state, rs)


def check_one_try_is_the_unverified_fit(loss, seed=5):
    inter = dataset()
    base = nc.model_for(loss, seed)
    base.fit(inter)
    one = nc.model_for(loss, seed, verify_negatives=True, verify_tries=1)
    one.fit(inter)
    nc.assert_same_fit(base, one, 'verify_tries=1')
    nn = NN if loss in host.COLUMN_LOSSES else 1
    stats = one.negative_verification_
    assert stats['candidates'] == EPOCHS * N * nn and stats['replaced'] == 0 and stats['unresolved'] > 0
    assert base.negative_verification_ is None and base._seen_items is None
    # ... and verifying does change the fit from two tries on
    two = nc.model_for(loss, seed, verify_negatives=True, verify_tries=2)
    two.fit(inter)
    assert not nc.same_state(base._random_state, two._random_state)


def check_candidate_cap_changes_nothing(monkeypatch, loss='adaptive_hinge', seed=9):
    """Groups of one minibatch per draw (the cap below a minibatch's candidates), of two, and the whole epoch in one."""
    inter = dataset()
    fits = []
    for cap in (1, 2 * B * NN * T, 1 << 25):
        monkeypatch.setattr(host, '_VERIFY_MAX_CANDIDATES', cap)
        model = nc.model_for(loss, seed, verify_negatives=True, verify_tries=T)
        model.fit(inter)
        fits.append(model)
    for other in fits[1:]:
        nc.assert_same_fit(fits[0], other, 'cap')
        assert other.negative_verification_ == fits[0].negative_verification_


class TwoTower(torch.nn.Module):
    """A representation that is not BilinearNet: the fit takes the autograd route."""

    def __init__(self, num_users, num_items, dim=8):
        super(TwoTower, self).__init__()
        self.users, self.items = torch.nn.Embedding(num_users, dim), torch.nn.Embedding(num_items, dim)
        self.mix = torch.nn.Linear(dim, dim)

    def forward(self, user_ids, item_ids):
        return (torch.tanh(self.mix(self.users(user_ids))) * self.items(item_ids)).sum(1)


def check_autograd_route_uses_the_same_negatives(monkeypatch, loss, seed=19):
    inter = dataset()
    nn = NN if loss in host.COLUMN_LOSSES else 1
    rs, epochs, totals = replay(inter, seed, loss, T)
    used = []
    inner = sampling.verify_negatives

    def recording(*a, **kw):
        out = inner(*a, **kw)
        used.append(out[0].reshape(-1).copy())
        return out
    monkeypatch.setattr(sampling, 'verify_negatives', recording)
    torch.manual_seed(0)
    custom = ImplicitFactorizationModel(loss=loss, n_iter=EPOCHS, batch_size=B, num_negative_samples=NN, representation=TwoTower(U, I),
                                        random_state=np.random.RandomState(seed), verify_negatives=True, verify_tries=T)
    custom.fit(inter)
    assert custom._autograd_route
    assert np.array_equal(np.concatenate(used), np.concatenate([e[3] for e in epochs]))
    assert custom.negative_verification_ == totals and nc.same_state(custom._random_state, rs)
    del used[:]
    other = nc.model_for(loss, seed, optimizer_func=nc._rmsprop, verify_negatives=True, verify_tries=T)  # no fused update
    other.fit(inter)
    assert other._autograd_route
    assert np.array_equal(np.concatenate(used), np.concatenate([e[3] for e in epochs]))
    assert other.negative_verification_ == totals and nc.same_state(other._random_state, rs)
    assert totals['candidates'] == EPOCHS * N * nn * T


def check_constructor_refusals():
    for bad in (0, 17, -1, 2.0, '4', None, True):
        rs = np.random.RandomState(3)
        before = rs.get_state()
        for verify in (False, True):
            with pytest.raises(ValueError, match='verify_tries'):
                ImplicitFactorizationModel(verify_negatives=verify, verify_tries=bad, random_state=rs)
        assert wc.same_state(rs.get_state(), before)
    for good in (1, 16, np.int64(4)):
        assert ImplicitFactorizationModel(verify_tries=good, random_state=np.random.RandomState(3))._verify_tries == int(good)


def check_models_that_do_not_verify():
    """The sharded model and the sequence model refuse the keyword before anything is drawn; fold_in() stays unverified."""
    from spotlight_amd.factorization.sharded import ShardedImplicitFactorizationModel
    from spotlight_amd.sequence.implicit import ImplicitSequenceModel
    rs = np.random.RandomState(3)
    before = rs.get_state()
    with pytest.raises(NotImplementedError, match='verify_negatives'):
        ShardedImplicitFactorizationModel(verify_negatives=True, random_state=rs)
    with pytest.raises(TypeError, match='verify_negatives'):
        ImplicitSequenceModel(verify_negatives=True, random_state=rs)
    assert wc.same_state(rs.get_state(), before)
    ShardedImplicitFactorizationModel(verify_negatives=False, random_state=np.random.RandomState(1))


def check_fold_in_stays_unverified(loss='bpr', seed=17):
    inter = dataset()
    model = nc.model_for(loss, seed, verify_negatives=True, verify_tries=T)
    model.fit(inter)
    users = np.repeat(np.arange(3), (4, 0, 9))
    new = Interactions(users.astype(np.int32), np.random.RandomState(3).randint(0, I, users.size).astype(np.int32), num_users=3,
                       num_items=I)
    init = (np.full((3, 16), 0.05, np.float32), np.zeros(3, np.float32))
    copy = np.random.RandomState()
    copy.set_state(model._random_state.get_state())
    drawn = model.fold_in(new, n_iter=2, init=init)
    want = np.stack([sample_items(I, (1, users.size), random_state=copy) for _ in range(2)])
    assert nc.same_state(model._random_state, copy)
    given = model.fold_in(new, n_iter=2, init=init, negatives=want)
    assert nc.same_bits(drawn[0], given[0]) and nc.same_bits(drawn[1], given[1])


def check_pickle_drops_the_device_csr():
    inter = dataset()
    model = nc.model_for('bpr', 23, verify_negatives=True, verify_tries=T)
    model.fit(inter)
    assert model._seen_items.d_off is not None and model._seen_items.d_items is not None
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    clone = torch.load(buf, weights_only=False)
    assert clone._seen_items.d_off is None and clone._seen_items.d_items is None
    assert clone.negative_verification_ == model.negative_verification_
    assert np.array_equal(clone.predict(2), model.predict(2))
    model.fit(inter)
    clone.fit(inter)  # the device side is rebuilt
    assert clone._seen_items.d_off is not None
    nc.assert_same_fit(model, clone, 'after the pickle round trip')
    assert clone.negative_verification_ == model.negative_verification_
