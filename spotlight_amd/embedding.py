"""Embedding front-end for encoders whose body runs on stock PyTorch-ROCm.

`lookup(weight, ids, ...)` is what `ScaledEmbedding` / `ZeroEmbedding` / `BloomEmbedding` call in their
`forward`: the gather (or hashed-row sum) and its autograd backward are the gfx950 kernels of
csrc/slk_embed.hip -- one stable radix sort of the looked-up rows, one owner group per distinct row adding
its gradient rows in ascending lookup order -- instead of torch's index_select / embedding_backward
(and, for bloom layers, instead of the reference's cached hash table + gather + sum,
spotlight/layers.py:177-242).  The recurrent / convolutional body of LSTMNet, CNNNet and MixtureLSTMNet
(spotlight/sequence/representations.py:147-596) stays on MIOpen through torch.

The gradient comes back dense (zero where untouched) for ordinary layers and as a coalesced sparse COO
tensor for `sparse=True` layers, so torch.optim's Adam / Adagrad / SparseAdam consume it unchanged.
There is no CPU compute path: tables on the HIP device are used in place, host-resident ones are staged onto it per call.
"""
import torch


def _hooks():
    # resolved at call time: the GPU-less test harness substitutes these hooks (tests/emu)
    from spotlight_amd.factorization import implicit as _host
    return _host


class _Lookup(torch.autograd.Function):

    @staticmethod
    def forward(ctx, weight, ids, bloom, padding_idx, sparse, device):
        """`device`: where the kernels run.  A table that lives elsewhere (in host memory) is staged onto it here and the result
        handed back on the table's own device -- inside the Function, not through autograd's copy nodes: the node of
        `weight.to(device)` cannot carry a sparse gradient home (it converts to the table's options, layout included)."""
        host = _hooks()
        if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.dim() != 2:
            raise RuntimeError('embedding tables must be contiguous 2-D fp32 tensors')
        home = weight.device
        table = weight if home == device else weight.to(device)
        engine = host._engine_for(device)
        stream = host._stream_for(device)
        flat = ids.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
        rows, dim = table.shape
        out = torch.empty((flat.numel(), dim), dtype=torch.float32, device=device)
        engine.embedding_forward(table.data_ptr(), rows, dim, bloom, flat.data_ptr(), flat.numel(), out.data_ptr(),
                                 stream)
        ctx.save_for_backward(flat)
        ctx.lookup = (rows, dim, bloom, padding_idx, sparse, device, home)
        return out.view(tuple(ids.shape) + (dim,)).to(home)

    @staticmethod
    def backward(ctx, grad_out):
        (flat,) = ctx.saved_tensors
        rows, dim, bloom, padding_idx, sparse, device, home = ctx.lookup
        host = _hooks()
        engine = host._engine_for(device)
        stream = host._stream_for(device)
        g = grad_out.reshape(flat.numel(), dim).to(device=device, dtype=torch.float32).contiguous()
        n_rows = engine.embedding_backward_plan(rows, dim, bloom, padding_idx, flat.data_ptr(), flat.numel(),
                                                count_rows=sparse, stream=stream)
        if sparse:
            idx = torch.empty((1, n_rows), dtype=torch.int64, device=device)
            val = torch.empty((n_rows, dim), dtype=torch.float32, device=device)
            engine.embedding_backward_fill(g.data_ptr(), None, idx.data_ptr(), val.data_ptr(), stream=stream)
            grad = torch.sparse_coo_tensor(idx.to(home), val.to(home), (rows, dim), is_coalesced=True)
        else:
            grad = torch.empty((rows, dim), dtype=torch.float32, device=device)
            engine.embedding_backward_fill(g.data_ptr(), grad.data_ptr(), stream=stream)
            grad = grad.to(home)
        return grad, None, None, None, None, None


def lookup(weight, ids, bloom=None, padding_idx=None, sparse=False):
    """weight[ids] (or the bloom layer's hashed-row sum) with shape ids.shape + (dim,), differentiable
    w.r.t. `weight`.  `bloom`: the layer's slk_bloom descriptor (BloomEmbedding.descriptor()).

    A layer that still lives in host memory (the reference's layers are plain torch modules and its tests call them right
    after construction, tests/test_layers.py) is staged onto the HIP device for the call and the result is handed back on
    the table's own device: the gather / hashed-row sum still runs in the gfx950 kernel (there is no CPU compute path;
    without a HIP device this raises), and the gradient, dense or sparse, comes back on the host as well."""
    home = weight.device
    dev = _hooks()._model_device() if home.type == 'cpu' else home
    return _Lookup.apply(weight, ids, bloom, padding_idx, bool(sparse), dev)
