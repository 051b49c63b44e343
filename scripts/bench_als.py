"""Times the ALS engine (csrc/slk_als.hip) on the device at the shapes of DESIGN.md 4b ("ALS"), dim 64:

  gram       slk_als_gram over 10^6 x 64 and 10^7 x 64 tables against the byte floor 4 * n * dim over the read rate
             slk_probe_stream measures on this device;
  half-step  a user half-step and an item half-step (slk_als_solve + the Gram matrix of the fixed side) on a CSR of about
             2 * 10^7 distinct entries (163 840 users x 2^20 items; the JSON records the exact count) whose row lengths are
             Zipf-like on BOTH sides (users: the lengths of scripts/bench_foldin.py; items: drawn from a power-law
             popularity), under "als_wg_min_len" = 0 (the built-in default), 8, 16, 32, 64, 256, 1024, 4096 and 2^40 (no
             workgroup route at all);
  iteration  one full iteration as fit() runs it (both half-steps, three Gram matrices' worth of sweeps, the objective), and
             the set-up of a fit() (both CSRs built on the device).

Two warm-up calls, then repeats timed with events on the stream; prints min / median / max per case and writes one JSON
document to profiles/bench_als.json.

    python scripts/bench_als.py [--out FILE] [--small]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotlight_amd import _native
from spotlight_amd.factorization import als
dev = torch.device('cuda', 0)
eng = _native.Engine(0)
stream = torch.cuda.current_stream(dev).cuda_stream
SMALL = '--small' in sys.argv  # a rehearsal size
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'bench_als.json')
D, LAM, ALPHA = 64, 0.05, 40.0
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


out = {'shape': dict(dim=D, regularization=LAM, alpha=ALPHA), 'device': torch.cuda.get_device_name(0)}
# the device's read rate: 1 GB, read only (include/spotlight_hip.h: slk_probe_stream kind 4)
probe = torch.empty(1 << (22 if SMALL else 28), dtype=torch.float32, device=dev)
read_ms = eng.probe_stream(4, probe.data_ptr(), probe.data_ptr(), probe.data_ptr(), probe.numel(), iters=10, stream=stream)
out['read_GBps'] = probe.numel() * 4 / read_ms / 1e6
del probe
print('read rate GB/s', out['read_GBps'], flush=True)

# ---- gram ---------------------------------------------------------------------------------------------------------------------------
gram = torch.empty((D, D), dtype=torch.float32, device=dev)
for n in ((10 ** 4,) if SMALL else (10 ** 6, 10 ** 7)):
    table = torch.randn((n, D), dtype=torch.float32, device=dev) * 0.1
    r = timed(lambda: eng.als_gram(table.data_ptr(), n, D, gram.data_ptr(), stream))
    floor_ms = 4.0 * n * D / (out['read_GBps'] * 1e6)
    r.update(bytes=4 * n * D, ms_at_read_rate=floor_ms, fraction_of_read_rate=floor_ms / r['median_ms'],
             gflops=2.0 * n * D * D / r['median_ms'] / 1e6)
    out['gram_%d' % n] = r
    print('gram', n, r, flush=True)
    del table

# ---- the Zipf CSR -------------------------------------------------------------------------------------------------------------------
U, I = (1 << 12, 1 << 12) if SMALL else (163840, 1 << 20)
z = rs.zipf(2.0, U)
lens = np.clip(30 * np.minimum(z, 400) + rs.randint(-10, 11, z.size), 1, 12000)
users = np.repeat(np.arange(U, dtype=np.int64), lens)
# item popularity: p(rank) ~ 1 / (rank + 20)^0.9, drawn on the device through the inverse CDF
cdf = torch.cumsum(1.0 / (torch.arange(I, dtype=torch.float64, device=dev) + 20.0) ** 0.9, 0)
cdf = cdf / cdf[-1]
g = torch.Generator(device=dev).manual_seed(3)
items = torch.searchsorted(cdf, torch.rand(users.size, dtype=torch.float64, device=dev, generator=g)).clamp_(max=I - 1).cpu().numpy()
del cdf
torch.cuda.synchronize()
t0 = time.perf_counter()
by_user, by_item = als.build_csrs(users, items, None, U, I, ALPHA, dev)
torch.cuda.synchronize()
out['csr_setup_ms'] = (time.perf_counter() - t0) * 1e3
ul, il = np.diff(by_user.off.cpu().numpy()), np.diff(by_item.off.cpu().numpy())
out['csr'] = dict(users=U, items=I, pairs_drawn=int(users.size), entries=by_user.nnz,
                  user_lengths=dict(median=float(np.median(ul)), mean=float(ul.mean()), max=int(ul.max())),
                  item_lengths=dict(median=float(np.median(il)), mean=float(il.mean()), max=int(il.max()), empty=int((il == 0).sum())))
print('csr', out['csr'], 'setup ms', out['csr_setup_ms'], flush=True)

X = torch.randn((U, D), dtype=torch.float32, device=dev) * 0.1
Y = torch.randn((I, D), dtype=torch.float32, device=dev) * 0.1
gx, gy = torch.empty_like(gram), torch.empty_like(gram)
failed = torch.zeros(1, dtype=torch.int32, device=dev)
per_row = torch.empty(U, dtype=torch.float64, device=dev)


def solve(fixed, g, csr, dst):
    eng.als_solve(fixed.data_ptr(), g.data_ptr(), D, LAM, csr.off.data_ptr(), csr.cols.data_ptr(), csr.vals.data_ptr(), None, csr.n_rows,
                  dst.data_ptr(), failed.data_ptr(), stream)


def user_half():
    eng.als_gram(Y.data_ptr(), I, D, gy.data_ptr(), stream)
    solve(Y, gy, by_user, X)


def item_half():
    eng.als_gram(X.data_ptr(), U, D, gx.data_ptr(), stream)
    solve(X, gx, by_item, Y)


def iteration():
    user_half()
    item_half()
    eng.als_gram(Y.data_ptr(), I, D, gy.data_ptr(), stream)
    eng.als_loss(X.data_ptr(), Y.data_ptr(), gy.data_ptr(), D, LAM, by_user.off.data_ptr(), by_user.cols.data_ptr(),
                 by_user.vals.data_ptr(), U, per_row.data_ptr(), stream)


# what a half-step must do at the least: gather every entry's row once (256 B) and read the fixed table once for its Gram matrix
gather_ms = by_user.nnz * 4.0 * D / (out['read_GBps'] * 1e6)
out['half_step_gather_bytes'] = dict(bytes=by_user.nnz * 4 * D, ms_at_read_rate=gather_ms)
# ... and the arithmetic: nnz * D (D + 1) / 2 multiply-adds for the systems, rows * D^3 / 6 for the factorizations
fma = lambda csr: csr.nnz * D * (D + 1) / 2.0 + csr.n_rows * (D ** 3 / 6.0 + D * D)
for wg in (0, 8, 16, 32, 64, 256, 1024, 4096, 1 << 40):
    with eng.options(als_wg_min_len=wg):
        for name, fn, csr in (('user', user_half, by_user), ('item', item_half, by_item)):
            r = timed(fn, warm=1, rep=5)
            r['gflops'] = 2.0 * fma(csr) / r['median_ms'] / 1e6
            out['%s_half_step_wg_min_len_%d' % (name, wg)] = r
            print(name, 'half-step wg_min_len', wg, r, flush=True)
out['failed_rows'] = int(failed.item())
out['iteration'] = timed(iteration, warm=1, rep=5)
print('iteration', out['iteration'], flush=True)
out['objective'] = float(per_row.sum())
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
