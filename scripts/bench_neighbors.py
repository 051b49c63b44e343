"""Times the neighbour sweep (slk_neighbors_topk, cosine) on the device at 4096 and 64 queries x 10^6 rows, dim 64, k = 10 and
k = 128, against the two yardsticks of DESIGN.md 4b: slk_bilinear_topk on the same table, row count and k (the same bytes and
matrix instructions: the epilogue is the only difference) and the route that gives the answer without the fused entry
(slk_neighbors_scores tiles of 256 MB + torch.topk).  Also slk_rows_inv_norm on the 10^6 x 64 table, against the table's bytes
at 8 TB/s.  Two warm-up calls, then 7 repeats timed with events on the stream; prints min / median / max per case and one JSON
line.

    python scripts/bench_neighbors.py
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spotlight_amd import _native  # noqa: E402

dev = torch.device('cuda', 0)
eng = _native.Engine(0)
stream = torch.cuda.current_stream(dev).cuda_stream
Q, I, D = 4096, 1000000, 64
g = torch.Generator(device='cpu').manual_seed(1)
table = (torch.randn(I, D, generator=g) * 0.1).to(dev)
queries = table[:Q].clone()
tscale = torch.empty(I, dtype=torch.float32, device=dev)
qscale = torch.empty(Q, dtype=torch.float32, device=dev)
eng.rows_inv_norm(table.data_ptr(), I, D, tscale.data_ptr(), stream)
eng.rows_inv_norm(queries.data_ptr(), Q, D, qscale.data_ptr(), stream)
# the yardstick's model: the queries as its user table, the table as its item table, random biases
bu, bi = torch.randn(Q, generator=g).to(dev), (torch.randn(I, generator=g) * 0.1).to(dev)
tb = _native.make_tables([queries.data_ptr(), table.data_ptr(), bu.data_ptr(), bi.data_ptr()], Q, I, D)
users = torch.arange(Q, dtype=torch.int64, device=dev)


def timed(fn, warm=2, rep=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(min_ms=ts[0], median_ms=ts[len(ts) // 2], max_ms=ts[-1], repeats=rep)


def outputs(n, k):
    return torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev)


def neighbors(n, k):
    items, scores = outputs(n, k)
    return lambda: eng.neighbors_topk(table.data_ptr(), I, D, tscale.data_ptr(), queries.data_ptr(), qscale.data_ptr(), n, k, None,
                                      None, items.data_ptr(), scores.data_ptr(), stream)


def bilinear(n, k):
    items, scores = outputs(n, k)
    return lambda: eng.bilinear_topk(tb, users.data_ptr(), n, k, None, None, items.data_ptr(), scores.data_ptr(), stream)


def scores_torch_topk(n, k):
    tile = max(1, (256 << 20) // (4 * I))
    buf = torch.empty((tile, I), dtype=torch.float32, device=dev)

    def run():
        for lo in range(0, n, tile):
            m = min(tile, n - lo)
            eng.neighbors_scores(table.data_ptr(), I, D, tscale.data_ptr(), queries[lo:].data_ptr(), qscale[lo:].data_ptr(), m,
                                 buf.data_ptr(), stream)
            torch.topk(buf[:m], k, dim=1, largest=True, sorted=True)
    return run


out = {}
cases = []
for n in (4096, 64):
    for k in (10, 128):
        cases += [('neighbors_%d_k%d' % (n, k), neighbors(n, k)), ('bilinear_topk_%d_k%d' % (n, k), bilinear(n, k)),
                  ('scores_torch_topk_%d_k%d' % (n, k), scores_torch_topk(n, k))]
cases.append(('rows_inv_norm', lambda: eng.rows_inv_norm(table.data_ptr(), I, D, tscale.data_ptr(), stream)))
for name, fn in cases:
    out[name] = timed(fn)
    print(name, out[name], flush=True)
for n in (4096, 64):
    for k in (10, 128):
        nb = out['neighbors_%d_k%d' % (n, k)]['median_ms']
        out['ratio_%d_k%d' % (n, k)] = dict(vs_bilinear_topk=nb / out['bilinear_topk_%d_k%d' % (n, k)]['median_ms'],
                                            vs_scores_torch_topk=nb / out['scores_torch_topk_%d_k%d' % (n, k)]['median_ms'])
floor_ms = I * D * 4 / 8e12 * 1e3
out['rows_inv_norm']['table_bytes_at_8TBs_ms'] = floor_ms
out['rows_inv_norm']['fraction_of_8TBs'] = floor_ms / out['rows_inv_norm']['median_ms']
# agreement with the tile + torch.topk route where no tie crosses (random rows: none)
items, scores = outputs(64, 10)
eng.neighbors_topk(table.data_ptr(), I, D, tscale.data_ptr(), queries.data_ptr(), qscale.data_ptr(), 64, 10, None, None,
                   items.data_ptr(), scores.data_ptr(), stream)
buf = torch.empty((64, I), dtype=torch.float32, device=dev)
eng.neighbors_scores(table.data_ptr(), I, D, tscale.data_ptr(), queries.data_ptr(), qscale.data_ptr(), 64, buf.data_ptr(), stream)
v, ix = torch.topk(buf, 10, dim=1)
out['agrees_with_torch_topk'] = bool(torch.equal(ix, items) and torch.equal(v, scores))
out['shape'] = dict(queries=Q, rows=I, dim=D, metric='cosine')
out['device'] = torch.cuda.get_device_name(0)
print(json.dumps(out))
