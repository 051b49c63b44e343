"""Times loss='softmax' next to loss='adaptive_hinge' (same build, same data, n = 5 negatives, Adagrad, dim 64; DESIGN.md 4b
"Sampled softmax"), both on C2-shaped tables (10^7 users, 10^6 items):

  (a) small   minibatches of 256, 400 per call.  Adaptive hinge runs them inside persistent launches; softmax takes the launch
              path at every size (score pass, k_softmax_loss, user pass, item pass per minibatch).  us per minibatch = call / 400.
  (b) staged  minibatches of 2^20, 10 per call, "overlap_prep" 1 as fit() sets it.  Adaptive hinge: score pass,
              k_adaptive_select, the late live list of 2 occurrences per interaction, user pass, item pass.  Softmax: score pass,
              k_softmax_loss, user pass, item pass over all 1 + n occurrences, every one live.  ms per step = call / 10.

SPOTLIGHT_HIP_LIB=PATH (spotlight_amd/_native.py) times another build of the library -- the parent commit's, for its
adaptive-hinge numbers -- through the same calls; --losses a,b restricts the run to the losses that build knows.  Two warm-up
calls, then repeats timed with events on the stream; prints min / median / max per case and writes one JSON file.

    python scripts/bench_softmax.py [--out profiles/bench_softmax.json] [--losses adaptive_hinge,softmax]
                                    [--skip-small] [--skip-staged]
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
OUT = arg('--out', os.path.join(ROOT, 'profiles', 'bench_softmax.json'))
LOSSES = arg('--losses', 'adaptive_hinge,softmax').split(',')
LIB = os.environ.get('SPOTLIGHT_HIP_LIB')
# (loss ids by number: a build that predates softmax still takes adaptive hinge's 3)
KIND = {'adaptive_hinge': 3, 'softmax': 8}
dev = torch.device('cuda', 0)
D, NN = 64, 5
U, I = 10 ** 7, 10 ** 6
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


def engine_point(name, n, B, options):
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
        tabs = [torch.randn(U, D, device=dev, generator=g) / D, torch.randn(I, D, device=dev, generator=g) / D,
                torch.zeros(U, device=dev), torch.zeros(I, device=dev)]
        state = [torch.zeros_like(t) for t in tabs]
        tables = _native.make_tables([t.data_ptr() for t in tabs], U, I, D)
        optim = _native.make_optim('adagrad', [t.data_ptr() for t in state], None, lr=1e-2)
        eng.rng_set_state(np.random.RandomState(1).get_state())
        call = lambda: eng.bilinear_train(tables, optim, users.data_ptr(), items.data_ptr(), n, B, KIND[loss], NN, mb_loss.data_ptr(),
                                          stream=stream)
        with eng.options(**options):
            eng.bilinear_reserve(tables, optim, n, B, KIND[loss], NN, stream=stream)
            eng.profile_reset()
            eng.profile_enable(True)
            call()
            eng.profile_enable(False)
            prof = eng.profile_read()
            r = timed(call)
        r['per_step_ms'] = r['median_ms'] / steps
        r['last_mean_loss'] = float(mb_loss.mean())
        # one profiled call (not among the timed ones): launches and ms per kernel class
        r['profile_one_call'] = {k: [int(v[0]), float(v[1])] for k, v in prof.items() if v[0]}
        out['%s_%s' % (name, loss)] = r
        print(name, loss, r, flush=True)
        del tabs, state
    if len(LOSSES) == 2:
        out[name + '_ratio_softmax_to_adaptive_hinge'] = out[name + '_softmax']['median_ms'] / out[name + '_adaptive_hinge']['median_ms']
    eng.close()
    torch.cuda.empty_cache()


if '--skip-small' not in sys.argv:
    engine_point('small', 400 * 256, 256, {})
if '--skip-staged' not in sys.argv:
    engine_point('staged', 10 << 20, 1 << 20, dict(overlap_prep=1))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print(json.dumps(out))
