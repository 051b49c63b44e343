"""Times slk_bilinear_foldin on the device (BPR, Adagrad, dim 64, 10 steps, an item table of 4 * 10^6 rows = 1 GB) at the two
shapes of DESIGN.md 4b ("Fold-in"):

  one_user   H = 1, m = 64: the latency of serving one new user (on the default route, on either route alone, and with an empty
             history: the cost of the call's two launches when neither has work);
  zipf       H = 2^17 users with Zipf-distributed history lengths (median about 30, maximum 12 000), under "foldin_wg_min_len" =
             0 (the built-in default), 64, 256, 1024, 4096 and 2^40 (no workgroup route at all);

against the gather-byte model (1 + nn) * n * n_steps * 256 B over the read rate slk_probe_stream measures on this device, and
against the generic route (spotlight_amd/foldin.py: generic_steps, torch autograd with the ids and negatives already on the
device; at the zipf shape ONE step, its cost per step does not depend on the step).  Two warm-up calls, then repeats timed with
events on the stream; prints min / median / max per case and one JSON line.

    python scripts/bench_foldin.py [--skip-generic]
"""
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotlight_amd import _native, foldin
dev = torch.device('cuda', 0)
eng = _native.Engine(0)
stream = torch.cuda.current_stream(dev).cuda_stream
I, D, T, LR = 4000000, 64, 10, 0.05
g = torch.Generator(device='cpu').manual_seed(1)
V = (torch.randn(I, D, generator=g) * 0.125).to(dev)
BI = (torch.randn(I, generator=g) * 0.1).to(dev)
rs = np.random.RandomState(7)


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


class Shape(object):
    def __init__(self, lens):
        self.lens = np.asarray(lens, dtype=np.int64)
        self.H, self.n = len(lens), int(self.lens.sum())
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.items = rs.randint(0, I, self.n).astype(np.int64)
        self.emb = rs.normal(0, 1.0 / D, (self.H, D)).astype(np.float32)
        self.b = np.zeros(self.H, np.float32)
        self.d_off, self.d_items = torch.from_numpy(self.off).to(dev), torch.from_numpy(self.items).to(dev)
        self.d_neg = torch.randint(0, I, (T, 1, self.n), dtype=torch.int64, device=dev)
        self.u, self.ub = torch.from_numpy(self.emb).to(dev), torch.from_numpy(self.b).to(dev)
        self.s1u, self.s1b = torch.zeros_like(self.u), torch.zeros_like(self.ub)
        self.tables = _native.make_tables([self.u.data_ptr(), V.data_ptr(), self.ub.data_ptr(), BI.data_ptr()], self.H, I, D)
        self.model_bytes = 2 * self.n * T * 4 * D  # (1 + nn) * n * n_steps * 256 B

    def fused(self, steps=T):
        def run():
            optim = _native.make_optim('adagrad', [self.s1u.data_ptr(), None, self.s1b.data_ptr(), None], None, lr=LR)
            eng.bilinear_foldin(self.tables, optim, self.d_off.data_ptr(), self.d_items.data_ptr(), self.H, self.n, 'bpr', 1, steps,
                                self.d_neg.data_ptr(), None, stream)
        return run

    def generic(self, steps):
        model = types.SimpleNamespace(_loss='bpr', _optimizer_func=lambda p: torch.optim.Adagrad(p, lr=LR), _l2=0.0, _learning_rate=LR)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        foldin.generic_steps(model, V, BI, self.off, self.items, self.d_neg, self.emb, self.b, steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3


out = {'shape': dict(items=I, dim=D, steps=T, loss='bpr', optimizer='adagrad'), 'device': torch.cuda.get_device_name(0)}
# the device's read rate: 1 GB, read only (include/spotlight_hip.h: slk_probe_stream kind 4)
probe = torch.empty(1 << 28, dtype=torch.float32, device=dev)
read_ms = eng.probe_stream(4, probe.data_ptr(), probe.data_ptr(), probe.data_ptr(), probe.numel(), iters=10, stream=stream)
out['read_GBps'] = probe.numel() * 4 / read_ms / 1e6
del probe
print('read rate GB/s', out['read_GBps'], flush=True)

one = Shape([64])
out['one_user'] = timed(one.fused(), rep=21)
print('one_user', out['one_user'], flush=True)
for name, wg in (('one_user_wave_route', 1 << 40), ('one_user_workgroup_route', 1)):
    with eng.options(foldin_wg_min_len=wg):
        out[name] = timed(one.fused(), rep=21)
    print(name, out[name], flush=True)
# what the two launches of a call cost when neither has anything to do: one user without a history
out['one_user_empty_history'] = timed(Shape([0]).fused(), rep=21)
print('one_user_empty_history', out['one_user_empty_history'], flush=True)

z = rs.zipf(2.0, 1 << 17)
lens = np.clip(30 * np.minimum(z, 400) + rs.randint(-10, 11, z.size), 1, 12000)
zipf = Shape(lens)
out['zipf_lengths'] = dict(users=zipf.H, interactions=zipf.n, median=float(np.median(lens)), max=int(lens.max()), mean=float(lens.mean()))
print('zipf lengths', out['zipf_lengths'], flush=True)
floor_ms = zipf.model_bytes / (out['read_GBps'] * 1e6)
out['zipf_byte_model'] = dict(bytes=zipf.model_bytes, ms_at_read_rate=floor_ms)
for wg in (0, 64, 256, 1024, 4096, 1 << 40):
    with eng.options(foldin_wg_min_len=wg):
        r = timed(zipf.fused())
    r['fraction_of_byte_model'] = floor_ms / r['median_ms']
    out['zipf_wg_min_len_%d' % wg] = r
    print('zipf wg_min_len', wg, r, flush=True)

if '--skip-generic' not in sys.argv:
    one.generic(T)  # warm-up
    out['one_user_generic_ms'] = sorted(one.generic(T) for _ in range(5))[2]
    out['zipf_generic_one_step_ms'] = zipf.generic(1)
    out['one_user_ratio_generic_over_fused'] = out['one_user_generic_ms'] / out['one_user']['median_ms']
    out['zipf_ratio_generic_over_fused_per_step'] = out['zipf_generic_one_step_ms'] / (out['zipf_wg_min_len_0']['median_ms'] / T)
print(json.dumps(out))
