"""Times loss='warp' next to loss='adaptive_hinge' (same build, same data, n = 5 negatives, Adagrad, dim 64; DESIGN.md 4b "WARP"):

  (a) persistent  MovieLens-100K-sized tables (943 users, 1682 items), 100 000 interactions in minibatches of 256: one
                  slk_bilinear_train call is 391 minibatches inside persistent launches.  us per minibatch = call / 391.
  (b) staged      C2-shaped tables (10^7 users, 10^6 items), minibatches of 2^20, 10 per call, "overlap_prep" 1 as fit() sets it:
                  score pass, k_adaptive_select, the late live list, user pass, item pass.  ms per step = call / 10.
  (c) mrr         evaluation.mrr_score on a synthetic set after equal epochs of bpr, adaptive_hinge and warp (for the docs only).

SPOTLIGHT_HIP_LIB=PATH (spotlight_amd/_native.py) times another build of the library -- the parent commit's, for its
adaptive-hinge numbers -- through the same calls; --losses a,b restricts (a) and (b) to the losses that build knows.  Two warm-up calls, then repeats timed with events on the
stream; prints min / median / max per case and writes one JSON file.

    python scripts/bench_warp.py [--out profiles/bench_warp.json] [--losses adaptive_hinge,warp]
                                 [--skip-persistent] [--skip-staged] [--skip-mrr]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spotlight_amd import _native

arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
OUT = arg('--out', os.path.join(ROOT, 'profiles', 'bench_warp.json'))
LOSSES = arg('--losses', 'adaptive_hinge,warp').split(',')
LIB = os.environ.get('SPOTLIGHT_HIP_LIB')
# (loss ids by number: a build that predates warp still takes adaptive hinge's 3)
KIND = {'adaptive_hinge': 3, 'warp': 7}
dev = torch.device('cuda', 0)
D, NN = 64, 5
out = {'device': torch.cuda.get_device_name(0), 'dim': D, 'optimizer': 'adagrad', 'num_negative_samples': NN, 'library': LIB or 'this build'}


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


def engine_point(name, U, I, n, B, options, scale):
    eng = _native.Engine(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randint(0, U, (n,), device=dev, generator=g)
    items = torch.randint(0, I, (n,), device=dev, generator=g)
    steps = (n + B - 1) // B
    mb_loss = torch.empty(steps, dtype=torch.float32, device=dev)
    out[name + '_shape'] = dict(users=U, items=I, interactions=n, batch=B, steps_per_call=steps)
    for loss in LOSSES:
        g.manual_seed(2)  # the same start for every loss
        tabs = [torch.randn(U, D, device=dev, generator=g) * scale, torch.randn(I, D, device=dev, generator=g) * scale,
                torch.zeros(U, device=dev), torch.zeros(I, device=dev)]
        state = [torch.zeros_like(t) for t in tabs]
        tables = _native.make_tables([t.data_ptr() for t in tabs], U, I, D)
        optim = _native.make_optim('adagrad', [t.data_ptr() for t in state], None, lr=1e-2)
        eng.rng_set_state(np.random.RandomState(1).get_state())
        call = lambda: eng.bilinear_train(tables, optim, users.data_ptr(), items.data_ptr(), n, B, KIND[loss], NN, mb_loss.data_ptr(),
                                          stream=stream)
        with eng.options(**options):
            eng.bilinear_reserve(tables, optim, n, B, KIND[loss], NN, stream=stream)
            r = timed(call)
        r['per_step_ms'] = r['median_ms'] / steps
        r['last_mean_loss'] = float(mb_loss.mean())
        out['%s_%s' % (name, loss)] = r
        print(name, loss, r, flush=True)
        del tabs, state
    if len(LOSSES) == 2:
        out[name + '_ratio_warp_to_adaptive_hinge'] = out[name + '_warp']['median_ms'] / out[name + '_adaptive_hinge']['median_ms']
    eng.close()
    torch.cuda.empty_cache()


if '--skip-persistent' not in sys.argv:
    engine_point('persistent', 943, 1682, 100000, 256, {}, 0.3)
if '--skip-staged' not in sys.argv:
    engine_point('staged', 10 ** 7, 10 ** 6, 10 << 20, 1 << 20, dict(overlap_prep=1), 1.0 / D)

if '--skip-mrr' not in sys.argv and 'warp' in LOSSES:
    from spotlight_amd.cross_validation import random_train_test_split
    from spotlight_amd.datasets import synthetic
    from spotlight_amd.evaluation import mrr_score
    from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
    data = synthetic.generate_sequential(num_users=1000, num_items=1000, num_interactions=100000, concentration_parameter=0.05,
                                         order=2, random_state=np.random.RandomState(3))
    train, test = random_train_test_split(data, random_state=np.random.RandomState(4))
    out['mrr_shape'] = dict(users=1000, items=1000, interactions=100000, epochs=10, batch=256, test_fraction=0.2)
    for loss in ('bpr', 'adaptive_hinge', 'warp'):
        model = ImplicitFactorizationModel(loss=loss, embedding_dim=32, n_iter=10, batch_size=256, num_negative_samples=NN,
                                           optimizer_func=lambda p: torch.optim.Adagrad(p, lr=0.05), sparse=True,
                                           random_state=np.random.RandomState(5))
        model.fit(train)
        out['mrr_' + loss] = float(mrr_score(model, test, train=train).mean())
        print('mrr', loss, out['mrr_' + loss], flush=True)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print(json.dumps(out))
