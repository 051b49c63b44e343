"""Times a bpr / Adagrad epoch at dim 64 on interaction weights (use_weights=True, slk_bilinear_train_weighted; DESIGN.md 4b
"Interaction weights") next to the unweighted one in the same run:

  (a) c2     the engine calls at C2-shaped tables (10^7 users, 10^6 items, dim 64), minibatches of 2^20, 20 minibatches per
             call, "overlap_prep" 1 as fit() sets it: slk_bilinear_train inside the user-row ping-pong scope (what an
             unweighted fit() of this size runs), the same call outside the scope, and slk_bilinear_train_weighted (which
             takes no scope).  ms per step = call / 20.
  (b) ml100k ImplicitFactorizationModel.fit() on a MovieLens-100K-sized set (943 users, 1682 items, 100 000 interactions) at the
             reference's batch_size 256: use_weights=False (two-lane schedule, the persistent kernel) next to use_weights=True
             (two-lane schedule, per-minibatch launches).  Per mode a fit() of 6 epochs and one of 2: (t6 - t2) / 4 is the
             steady-state epoch.

Two warm-up calls, then repeats timed with events on the stream; prints min / median / max per case and writes one JSON file.

    python scripts/bench_weighted_fit.py [--out profiles/bench_weighted_fit.json] [--skip-c2] [--skip-fit]
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

OUT = os.path.join(ROOT, 'profiles', 'bench_weighted_fit.json')
if '--out' in sys.argv:
    OUT = sys.argv[sys.argv.index('--out') + 1]
dev = torch.device('cuda', 0)
D = 64
out = {'device': torch.cuda.get_device_name(0), 'dim': D, 'loss': 'bpr', 'optimizer': 'adagrad'}


def timed(fn, warm=2, rep=7):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(min_ms=ts[0], median_ms=ts[len(ts) // 2], max_ms=ts[-1], repeats=rep)


if '--skip-c2' not in sys.argv:
    U, I, B, STEPS = 10 ** 7, 10 ** 6, 1 << 20, 20
    n = B * STEPS
    eng = _native.Engine(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(1)
    tabs = [torch.randn(U, D, device=dev, generator=g) / D, torch.randn(I, D, device=dev, generator=g) / D,
            torch.zeros(U, device=dev), torch.zeros(I, device=dev)]
    state = [torch.zeros_like(t) for t in tabs]
    tables = _native.make_tables([t.data_ptr() for t in tabs], U, I, D)
    optim = _native.make_optim('adagrad', [t.data_ptr() for t in state], None, lr=1e-2)
    users = torch.randint(0, U, (n,), device=dev, generator=g)
    items = torch.randint(0, I, (n,), device=dev, generator=g)
    weights = torch.exp2(torch.rand(n, device=dev, generator=g) * 12 - 6)
    mb_loss = torch.empty(STEPS, dtype=torch.float32, device=dev)
    eng.rng_set_state(np.random.RandomState(1).get_state())
    plain = lambda: eng.bilinear_train(tables, optim, users.data_ptr(), items.data_ptr(), n, B, 'bpr', 1, mb_loss.data_ptr(), stream=stream)
    weighted = lambda: eng.bilinear_train_weighted(tables, optim, users.data_ptr(), items.data_ptr(), weights.data_ptr(), n, B, 'bpr', 1,
                                                   mb_loss.data_ptr(), stream=stream)
    out['c2_shape'] = dict(users=U, items=I, batch=B, steps_per_call=STEPS)
    with eng.options(overlap_prep=1):
        eng.bilinear_reserve(tables, optim, n, B, 'bpr', 1, stream=stream)
        with eng.user_pingpong(tables, optim, stream=stream):
            out['c2_unweighted_pingpong'] = timed(plain)
        out['c2_unweighted_one_table'] = timed(plain)
        out['c2_weighted'] = timed(weighted)
    for key in ('c2_unweighted_pingpong', 'c2_unweighted_one_table', 'c2_weighted'):
        out[key]['ms_per_step'] = out[key]['median_ms'] / STEPS
        print(key, out[key], flush=True)
    out['c2_ratio_weighted_to_pingpong'] = out['c2_weighted']['median_ms'] / out['c2_unweighted_pingpong']['median_ms']
    out['c2_ratio_weighted_to_one_table'] = out['c2_weighted']['median_ms'] / out['c2_unweighted_one_table']['median_ms']
    del tabs, state, users, items, weights
    eng.close()
    torch.cuda.empty_cache()

if '--skip-fit' not in sys.argv:
    from spotlight_amd.factorization import implicit as host
    from spotlight_amd.interactions import Interactions
    U, I, n, B = 943, 1682, 100000, 256
    rs = np.random.RandomState(7)
    inter = Interactions(rs.randint(0, U, n).astype(np.int32), rs.randint(0, I, n).astype(np.int32),
                         weights=(2.0 ** rs.uniform(-6, 6, n)).astype(np.float32), num_users=U, num_items=I)
    out['ml100k_shape'] = dict(users=U, items=I, interactions=n, batch=B)
    for name, use in (('ml100k_unweighted', False), ('ml100k_weighted', True)):
        model = host.ImplicitFactorizationModel(loss='bpr', embedding_dim=D, n_iter=3, batch_size=B, sparse=True, use_weights=use,
                                                optimizer_func=lambda p: torch.optim.Adagrad(p, lr=1e-2),
                                                random_state=np.random.RandomState(1))

        def fit_seconds(epochs):
            model._n_iter = epochs
            t0 = time.perf_counter()
            model.fit(inter)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        fit_seconds(3)  # warm: table initialisation, scratch, the epoch buffers
        reps = sorted((fit_seconds(6), fit_seconds(2)) for _ in range(5))
        t6, t2 = reps[len(reps) // 2]
        out[name] = dict(seconds_6_epochs=t6, seconds_2_epochs=t2, steady_state_ms_per_epoch=(t6 - t2) / 4 * 1e3,
                         ms_per_epoch_of_6=t6 / 6 * 1e3)
        print(name, out[name], flush=True)
    out['ml100k_ratio_weighted_to_unweighted'] = (out['ml100k_weighted']['steady_state_ms_per_epoch'] /
                                                  out['ml100k_unweighted']['steady_state_ms_per_epoch'])

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print(json.dumps(out))
