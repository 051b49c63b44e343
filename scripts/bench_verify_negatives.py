"""Times verified negatives (slk_verify_negatives, DESIGN.md 4b "Verified negatives") on the device, at 10^6 users, 10^6 items
with Zipf(1.0) item ids and 2^25 interactions:

  (a) kernel   slk_verify_negatives over 2^20 columns, n_neg 1, tries 4, against the CSR of the 2^25 interactions, candidates
               drawn uniformly and by popularity; next to the uniform and the weighted sampler's time for the 4 * 2^20-value
               draw it follows, in the same run;
  (b) build    SeenItems.bind, the once-per-fit CSR build, from ids already on the device;
  (c) fit      ImplicitFactorizationModel.fit() (BPR, Adagrad, dim 64, batch 2^20): verify_negatives=True, verify_tries=4 next
               to the unverified fit forced onto the same two-lane schedule with negatives handed in, uniform negatives.
               Per mode a fit() of 6 epochs and one of 2: (t6 - t2) / 4 is the steady-state epoch;
  (d) shares   negative_verification_ of fits under 'uniform' and 'popularity' with verify_tries 1 (which only counts: its
               `unresolved` is the number of false negatives an unverified fit trains on) and 4.

Two warm-up calls, then repeats timed with events on the stream; prints every case and writes one JSON file.

    python scripts/bench_verify_negatives.py [--out profiles/bench_verify_negatives.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spotlight_amd import _native
from spotlight_amd.factorization import implicit as host
from spotlight_amd.interactions import Interactions
from spotlight_amd.sampling import ItemDistribution, SeenItems

OUT = os.path.join(ROOT, 'profiles', 'bench_verify_negatives.json')
if '--out' in sys.argv:
    OUT = sys.argv[sys.argv.index('--out') + 1]
dev = torch.device('cuda', 0)
eng = _native.Engine(0)
stream = torch.cuda.current_stream(dev).cuda_stream
U, I, n, D, B = 1000000, 1000000, 1 << 25, 64, 1 << 20
COLS, NN, T = 1 << 20, 1, 4


def timed(fn, warm=2, rep=9):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(min_ms=ts[0], median_ms=ts[len(ts) // 2], max_ms=ts[-1], repeats=rep)


def zipf_ids(count, n_ids, seed):
    """count ids over n_ids items, item of popularity rank r with probability ~ 1 / r, the ranks scattered over the id range."""
    r = np.random.RandomState(seed)
    cdf = np.cumsum(1.0 / np.arange(1, n_ids + 1))
    ranks = np.minimum(np.searchsorted(cdf / cdf[-1], r.random_sample(count)), n_ids - 1)
    return r.permutation(n_ids)[ranks]


rs = np.random.RandomState(7)
inter = Interactions(rs.randint(0, U, n).astype(np.int32), zipf_ids(n, I, 5).astype(np.int32), num_users=U, num_items=I)
out = {'shape': dict(users=U, items=I, interactions=n, item_ids='zipf(1.0)', columns=COLS, n_neg=NN, tries=T),
       'device': torch.cuda.get_device_name(0)}

# ---- (b) the CSR build ---------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
seen = SeenItems.from_interactions(inter.user_ids, inter.item_ids, U, I)
out['seen_items_validation_host_seconds'] = time.perf_counter() - t0
ids = host.IdUpload([inter.user_ids, inter.item_ids], dev).result()
torch.cuda.synchronize()


def build():
    seen.d_off = seen.d_items = None
    seen.bind(eng, dev, stream, ids=ids)


out['csr_build'] = timed(build, warm=1, rep=5)
print('csr_build', out['csr_build'], flush=True)

# ---- (a) the kernel next to the draw it follows ---------------------------------------------------------------------------------------
eng.rng_set_state(np.random.RandomState(1).get_state())
dist = ItemDistribution.from_counts(inter.item_ids, I).bind(eng, dev, stream)
d_users = ids[0][:COLS].contiguous()
d_cand = torch.empty(COLS * NN * T, dtype=torch.int64, device=dev)
d_neg = torch.empty(COLS * NN, dtype=torch.int64, device=dev)
d_counts = torch.zeros(2, dtype=torch.int64, device=dev)


def verify(counts):
    eng.verify_negatives(d_users.data_ptr(), COLS, B, NN, T, d_cand.data_ptr(), seen.d_off.data_ptr(), seen.d_items.data_ptr(), U,
                         d_neg.data_ptr(), d_counts.data_ptr() if counts else None, stream=stream)


out['draw_uniform'] = timed(lambda: eng.sample_items(I, d_cand.numel(), d_cand.data_ptr(), stream))
out['verify_uniform_candidates'] = timed(lambda: verify(True))
out['verify_uniform_candidates_uncounted'] = timed(lambda: verify(False))
out['draw_popularity'] = timed(lambda: dist.sample(eng, d_cand.numel(), d_cand.data_ptr(), stream))
d_counts.zero_()
verify(True)
out['popularity_candidates_one_call'] = dict(zip(('replaced', 'unresolved'), d_counts.cpu().tolist()), slots=COLS * NN)
out['verify_popularity_candidates'] = timed(lambda: verify(True))
for k in ('draw_uniform', 'verify_uniform_candidates', 'verify_uniform_candidates_uncounted', 'draw_popularity',
          'popularity_candidates_one_call', 'verify_popularity_candidates'):
    print(k, out[k], flush=True)
del d_cand, d_neg, d_users, ids
seen.d_off = seen.d_items = None

# ---- (c), (d) fit() ------------------------------------------------------------------------------------------------------------------
out['fit_shape'] = dict(users=U, items=I, interactions=n, dim=D, batch=B, loss='bpr', optimizer='adagrad', item_ids='zipf(1.0)')
model = host.ImplicitFactorizationModel(loss='bpr', embedding_dim=D, n_iter=3, batch_size=B, sparse=True,
                                        optimizer_func=lambda p: torch.optim.Adagrad(p, lr=1e-2),
                                        random_state=np.random.RandomState(1))
host._PIPELINE_MAX_DRAWS = 1 << 40  # every fit below: the two-lane schedule, negatives handed in
model.fit(inter)  # warm: table initialisation, scratch, the id buffers
torch.cuda.synchronize()


def fit_seconds(epochs):
    model._n_iter = epochs
    t0 = time.perf_counter()
    model.fit(inter)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for name, verifying, tries in (('unverified_two_lane', False, 4), ('verified_4_tries_two_lane', True, 4)):
    model._verify_negatives, model._verify_tries = verifying, tries
    fit_seconds(3)  # warm this mode's buffers
    t6, t2 = fit_seconds(6), fit_seconds(2)
    out['fit_' + name] = dict(seconds_6_epochs=t6, seconds_2_epochs=t2, steady_state_ms_per_epoch=(t6 - t2) / 4 * 1e3,
                              ms_per_epoch_of_6=t6 / 6 * 1e3)
    print('fit', name, out['fit_' + name], flush=True)

for sampling_mode in ('uniform', 'popularity'):
    for tries in (1, 4):
        model._negative_sampling, model._verify_negatives, model._verify_tries = sampling_mode, True, tries
        fit_seconds(2)
        stats = dict(model.negative_verification_)
        slots = stats['candidates'] // tries
        stats.update(slots=slots, replaced_share=stats['replaced'] / slots, unresolved_share=stats['unresolved'] / slots)
        out['shares_%s_tries_%d' % (sampling_mode, tries)] = stats
        print('shares', sampling_mode, tries, stats, flush=True)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print(json.dumps(out))
