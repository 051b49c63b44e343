"""Times the weighted sampler (slk_sample_items_weighted, DESIGN.md 4b "Weighted negatives") on the device:

  (a) draws      one weighted draw of 2^20 and of 2^25 values over 10^6 items, constant weights and Zipf(1.0)-count ** 0.75
                 weights, next to slk_sample_items (the uniform sampler) of the same count in the same run;
  (b) guide      the same draws under guide_bits 0 (a plain binary search of the whole cdf), 12, 16, 20 and the automatic value;
                 and what building the guide costs;
  (c) fit        ImplicitFactorizationModel.fit() at 2^25 interactions (10^6 users, 10^6 items with Zipf(1.0) item ids, BPR,
                 Adagrad, dim 64, batch 2^20): negative_sampling='popularity' next to 'uniform' on the three-stage pipeline and
                 'uniform' forced onto the two-lane schedule -- the cost of the schedule and the cost of the sampler apart.
                 Per mode a fit() of 6 epochs and one of 2: (t6 - t2) / 4 is the steady-state epoch.

Two warm-up calls, then repeats timed with events on the stream; prints min / median / max per case and writes one JSON file.

    python scripts/bench_weighted_sampler.py [--out profiles/bench_weighted_sampler.json] [--skip-fit]
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
from spotlight_amd.sampling import ItemDistribution

OUT = os.path.join(ROOT, 'profiles', 'bench_weighted_sampler.json')
if '--out' in sys.argv:
    OUT = sys.argv[sys.argv.index('--out') + 1]
dev = torch.device('cuda', 0)
eng = _native.Engine(0)
stream = torch.cuda.current_stream(dev).cuda_stream
I = 1000000
rs = np.random.RandomState(7)


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


def zipf_ids(n, n_ids, seed):
    """n ids over n_ids items, item of popularity rank r with probability ~ 1 / r, the ranks scattered over the id range."""
    r = np.random.RandomState(seed)
    cdf = np.cumsum(1.0 / np.arange(1, n_ids + 1))
    ranks = np.minimum(np.searchsorted(cdf / cdf[-1], r.random_sample(n)), n_ids - 1)
    return r.permutation(n_ids)[ranks]


out = {'shape': dict(items=I), 'device': torch.cuda.get_device_name(0)}
WEIGHTS = {'constant': np.ones(I), 'zipf_counts_pow_0.75': np.bincount(zipf_ids(1 << 25, I, 3), minlength=I).astype(np.float64) ** 0.75}
eng.rng_set_state(np.random.RandomState(1).get_state())
auto = eng.cdf_guide_bits(I)
out['auto_guide_bits'] = auto
for count in (1 << 20, 1 << 25):
    d_out = torch.empty(count, dtype=torch.int64, device=dev)
    key = 'draw_%d' % count
    out[key] = {'uniform_sample_items': timed(lambda: eng.sample_items(I, count, d_out.data_ptr(), stream))}
    print(key, 'uniform', out[key]['uniform_sample_items'], flush=True)
    for name, w in WEIGHTS.items():
        for bits in (0, 12, 16, 20, None):
            dist = ItemDistribution(w, I).bind(eng, dev, stream, guide_bits=bits)
            r = timed(lambda: dist.sample(eng, count, d_out.data_ptr(), stream))
            r['guide_bits'] = dist.guide_bits
            r['ratio_to_uniform'] = r['median_ms'] / out[key]['uniform_sample_items']['median_ms']
            out[key]['%s_guide_%s' % (name, 'auto' if bits is None else bits)] = r
            print(key, name, 'guide_bits', bits, r, flush=True)
    del d_out
dist = ItemDistribution(WEIGHTS['zipf_counts_pow_0.75'], I).bind(eng, dev, stream)
for bits in (12, 16, 20, 24):
    d_guide = torch.empty((1 << bits) + 1, dtype=torch.int32, device=dev)
    out['cdf_guide_bits_%d' % bits] = timed(lambda: eng.cdf_guide(dist.d_cdf.data_ptr(), I, bits, d_guide.data_ptr(), stream))
    print('cdf_guide', bits, out['cdf_guide_bits_%d' % bits], flush=True)

if '--skip-fit' not in sys.argv:
    from spotlight_amd.factorization import implicit as host
    from spotlight_amd.interactions import Interactions
    from spotlight_amd import sampling
    U, n, D, B = 1000000, 1 << 25, 64, 1 << 20
    inter = Interactions(rs.randint(0, U, n).astype(np.int32), zipf_ids(n, I, 5).astype(np.int32), num_users=U, num_items=I)
    out['fit_shape'] = dict(users=U, items=I, interactions=n, dim=D, batch=B, loss='bpr', optimizer='adagrad', item_ids='zipf(1.0)')
    t0 = time.perf_counter()
    sampling.item_distribution('popularity', 0.75, I, inter.item_ids)
    out['fit_item_distribution_host_seconds'] = time.perf_counter() - t0  # once per fit(): bincount, power, cumsum on the host
    model = host.ImplicitFactorizationModel(loss='bpr', embedding_dim=D, n_iter=3, batch_size=B, sparse=True,
                                            optimizer_func=lambda p: torch.optim.Adagrad(p, lr=1e-2),
                                            random_state=np.random.RandomState(1))
    model.fit(inter)  # warm: table initialisation, scratch, the id buffers of the three-stage loop
    torch.cuda.synchronize()
    default_max = host._PIPELINE_MAX_DRAWS

    def fit_seconds(epochs):
        model._n_iter = epochs
        t0 = time.perf_counter()
        model.fit(inter)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name, sampling_mode, max_draws in (('uniform_three_stage', 'uniform', default_max), ('uniform_two_lane', 'uniform', 1 << 40),
                                           ('popularity_two_lane', 'popularity', default_max)):
        model._negative_sampling = sampling_mode
        host._PIPELINE_MAX_DRAWS = max_draws
        try:
            fit_seconds(3)  # warm this schedule's buffers
            t6, t2 = fit_seconds(6), fit_seconds(2)
        finally:
            host._PIPELINE_MAX_DRAWS = default_max
        out['fit_' + name] = dict(seconds_6_epochs=t6, seconds_2_epochs=t2, steady_state_ms_per_epoch=(t6 - t2) / 4 * 1e3,
                                  ms_per_epoch_of_6=t6 / 6 * 1e3)
        print('fit', name, out['fit_' + name], flush=True)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print(json.dumps(out))
