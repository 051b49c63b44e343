"""Times the top-k sweep (slk_bilinear_topk) on the device at 4096 users x 10^6 items, dim 64 (k = 10, k = 128) and 64 users
(k = 10), against the two yardsticks of DESIGN.md 4b: the route that gives the same answer without it (slk_bilinear_scores
tiles of 256 MB + torch.topk) and the COUNT sweep over the same rows (slk_bilinear_rank: the same item bytes).  Two warm-up
calls, then repeats timed with events on the stream; prints min / median / max per case and one JSON line.

    python scripts/bench_topk.py
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotlight_amd import _native
dev = torch.device('cuda', 0)
eng = _native.Engine(0)
stream = torch.cuda.current_stream(dev).cuda_stream
U, I, D = 4096, 1000000, 64
g = torch.Generator(device='cpu').manual_seed(1)
p = [torch.randn(U, D, generator=g).to(dev), torch.randn(I, D, generator=g).to(dev) * 0.1, torch.randn(U, generator=g).to(dev), torch.randn(I, generator=g).to(dev) * 0.1]
tb = _native.make_tables([t.data_ptr() for t in p], U, I, D)
users = torch.arange(U, dtype=torch.int64, device=dev)
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
out = {}
def topk(n, k):
    items = torch.empty((n, k), dtype=torch.int64, device=dev); scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    return lambda: eng.bilinear_topk(tb, users.data_ptr(), n, k, None, None, items.data_ptr(), scores.data_ptr(), stream)
def parent(n, k):
    tile = max(1, (256 << 20) // (4 * I))
    buf = torch.empty((tile, I), dtype=torch.float32, device=dev)
    def run():
        for lo in range(0, n, tile):
            m = min(tile, n - lo)
            eng.bilinear_scores(tb, users[lo:].data_ptr(), m, buf.data_ptr(), stream)
            torch.topk(buf[:m], k, dim=1, largest=True, sorted=True)
    return run
def count(n):
    rg = torch.arange(n, dtype=torch.int64, device=dev); rt = torch.randint(0, I, (n,), device=dev); ranks = torch.empty(n, dtype=torch.float64, device=dev)
    return lambda: eng.bilinear_rank(tb, users.data_ptr(), n, rg.data_ptr(), rt.data_ptr(), n, None, None, ranks.data_ptr(), stream)
for name, fn in [('select_4096_k10', topk(4096, 10)), ('select_4096_k128', topk(4096, 128)), ('select_64_k10', topk(64, 10)),
                 ('count_4096', count(4096)), ('count_64', count(64)),
                 ('parent_scores_torch_topk_64_k10', parent(64, 10)), ('parent_scores_torch_topk_4096_k10', parent(4096, 10)),
                 ('parent_scores_torch_topk_4096_k128', parent(4096, 128))]:
    out[name] = timed(fn, rep=5 if name.startswith('parent') else 7)
    print(name, out[name], flush=True)
# agreement with the parent route where no tie crosses (random tables: none)
items = torch.empty((64, 10), dtype=torch.int64, device=dev); scores = torch.empty((64, 10), dtype=torch.float32, device=dev)
eng.bilinear_topk(tb, users.data_ptr(), 64, 10, None, None, items.data_ptr(), scores.data_ptr(), stream)
buf = torch.empty((64, I), dtype=torch.float32, device=dev)
eng.bilinear_scores(tb, users.data_ptr(), 64, buf.data_ptr(), stream)
v, ix = torch.topk(buf, 10, dim=1)
out['agrees_with_torch_topk'] = bool(torch.equal(ix, items) and torch.equal(v, scores))
out['shape'] = dict(users=U, items=I, dim=D)
out['device'] = torch.cuda.get_device_name(0)
print(json.dumps(out))
