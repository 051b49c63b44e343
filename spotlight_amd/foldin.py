"""fold_in() / recommend_vectors(): rows for users who arrived after fit() -- the pieces behind the model methods.

A fold-in step of new user u is one reference minibatch (spotlight/factorization/implicit.py:229-243) made of u's interactions
alone, with the item tables frozen: score, loss over the user's m interactions (mean over m), gradient with respect to the
user's row and bias only, one optimizer step on them (include/spotlight_hip.h: slk_bilinear_foldin states the contract).

  fused route    plain item tables and an optimizer with a fused update (Adam, Adagrad, SparseAdam, plain SGD): ONE call into
                 csrc/slk_foldin.hip for all users and all steps.
  generic route  an item BloomEmbedding (materialised once, as similar_items() does), any other `optimizer_func`, a custom
                 representation that exposes `item_embeddings` / `item_biases`: two nn.Parameters trained by the model's own
                 optimizer_func on the HIP device; the loss is the SUM over users of the reference loss function on that user's
                 slice, and every term sees only its own row, so element-wise optimizers give the per-user semantics.  It is also
                 what the tests compare the fused route with.
"""
import numpy as np
import torch
import torch.optim as optim

from spotlight_amd import _native
from spotlight_amd import recommend as _rec
from spotlight_amd import sampling as _sampling
from spotlight_amd.factorization import implicit as _host
from spotlight_amd.layers import BloomEmbedding


def _item_side(model, what):
    """(item embeddings [I, dim] float32 device tensor, item biases [I], plain) of the model's representation; `plain`: both are
    the net's own storage (no BloomEmbedding), so the fused kernels may read them in place."""
    net = model._net
    if net is None:
        raise RuntimeError('{}() needs a fitted model'.format(what))
    if isinstance(getattr(net, 'user_embeddings', None), BloomEmbedding):
        raise TypeError('{}(): the user table is a BloomEmbedding -- a user has no row of their own there (their vector is a sum of '
                        'hashed rows shared with other users), so there is nothing to fold a new user into'.format(what))
    if getattr(net, 'item_embeddings', None) is None or getattr(net, 'item_biases', None) is None:
        raise TypeError('{}(): {} has no `item_embeddings` / `item_biases`: the frozen item side of a custom representation is read '
                        'from those two layers'.format(what, type(net).__name__))
    table = model._embedding_table('item_embeddings', model._num_items)
    bias = model._embedding_table('item_biases', model._num_items).reshape(-1)
    plain = (not isinstance(net.item_embeddings, BloomEmbedding) and not model._is_custom_net()
             and table.data_ptr() == net.item_embeddings.weight.data_ptr() and bias.data_ptr() == net.item_biases.weight.data_ptr())
    if not (table.is_contiguous() and bias.is_contiguous() and table.dtype == torch.float32 and bias.dtype == torch.float32):
        raise RuntimeError('the item tables must be contiguous fp32 tensors')
    return table, bias, plain


def _refuse_inside_open_scope(engine, stream, table, bias, num_items):
    """Raises what predict() raises inside an open fit() scope whose item biases are shadowed (the array is stale until the scope
    ends), BEFORE anything is drawn from the model's RandomState and on every route: an empty slk_shard_scores call over the
    item side runs the entry's table checks and nothing else."""
    tables = _native.make_tables([None, table.data_ptr(), None, bias.data_ptr()], 0, num_items, int(table.shape[1]))
    engine.shard_scores(tables, None, None, 0, None, stream)


def history_csr(model, interactions):
    """(off [H + 1], items [n]) of the new users' histories: a STABLE sort by user, so duplicates are kept and the order within a
    user is the order of appearance (tocsr() would sum duplicates).  The user ids label the new users 0 .. H - 1."""
    users = np.asarray(interactions.user_ids).reshape(-1)
    items = np.asarray(interactions.item_ids).reshape(-1)
    H = int(interactions.num_users)
    if users.size:
        if users.max() >= H:
            raise ValueError('Maximum user id greater than number of users in interactions.')
        _host._reject_negative_ids(users)
        model._check_item_id_max(items)
        _host._reject_negative_ids(items)
    order = np.argsort(users, kind='stable')
    counts = np.bincount(users.astype(np.int64), minlength=H) if users.size else np.zeros(H, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return off, np.ascontiguousarray(items[order], dtype=np.int64), H


def _fresh_optimizer(model, params):
    """The model's own optimizer kind and hyper-parameters over `params`, with fresh state and a fresh step counter."""
    if model._optimizer_func is None:
        return optim.Adam(params, weight_decay=model._l2, lr=model._learning_rate)
    return model._optimizer_func(params)


def _negatives(model, negatives, T, nn, n, device, engine, stream):
    """int64 device tensor [T, nn, n]: the caller's, or drawn on the device from the model's RandomState exactly as T successive
    sample_items(num_items, (nn, n)) calls would draw them (one contiguous draw: state set, draw, state read back, as fit()) -- with
    the item weights of the model's last fit() (`negative_sampling`) as T successive choice(num_items, (nn, n), p=p) calls would."""
    if negatives is not None:
        neg = np.ascontiguousarray(np.asarray(negatives), dtype=np.int64)
        if neg.shape == (T, n) and nn == 1:
            neg = neg.reshape(T, 1, n)
        if neg.shape != (T, nn, n):
            raise ValueError('negatives must have shape (n_iter, {}, {}), got {}'.format(nn, n, neg.shape))
        if neg.size:
            model._check_item_id_max(neg)
            _host._reject_negative_ids(neg)
        return torch.from_numpy(neg).to(device)
    out = torch.empty((T, nn, max(n, 1)) if n == 0 else (T, nn, n), dtype=torch.int64, device=device)
    if n:
        dist = getattr(model, '_item_distribution', None)  # the item weights of the last fit() (None: uniform)
        if dist is not None:
            dist.bind(engine, device, stream)
        engine.rng_set_state(model._random_state.get_state())
        _sampling.draw_items(engine, model._num_items, T * nn * n, out.data_ptr(), stream, dist)
        model._random_state.set_state(engine.rng_get_state())
    return out


def _initial_rows(model, init, H, dim):
    if init is None:
        # ScaledEmbedding's and ZeroEmbedding's distributions (spotlight/layers.py:23-56)
        return model._random_state.normal(0, 1.0 / dim, (H, dim)).astype(np.float32), np.zeros(H, np.float32)
    emb, bias = init
    emb = np.array(emb, dtype=np.float32, order='C').reshape(H, dim)
    bias = np.array(bias, dtype=np.float32, order='C').reshape(H)
    return emb, bias


def generic_steps(model, table, bias, off, items, neg, emb, b, T):
    """The generic route: T steps of the model's own optimizer_func on two nn.Parameters (the rows and biases of the users with a
    history; a user without one keeps theirs untouched, whatever the optimizer does to a zero gradient)."""
    from spotlight_amd import losses as _losses
    loss_func = {'pointwise': _losses.pointwise_loss, 'bpr': _losses.bpr_loss, 'hinge': _losses.hinge_loss,
                 'adaptive_hinge': _losses.adaptive_hinge_loss,
                 'warp': lambda pos, neg: _losses.warp_loss(pos, neg, model._num_items),
                 'softmax': _losses.softmax_loss}[model._loss]
    device = table.device
    lens = np.diff(off)
    live = np.nonzero(lens > 0)[0]
    if not live.size:
        return emb, b
    u = torch.nn.Parameter(torch.from_numpy(emb[live]).to(device))
    ub = torch.nn.Parameter(torch.from_numpy(b[live]).to(device))
    opt = _fresh_optimizer(model, [u, ub])
    row_of = torch.from_numpy(np.repeat(np.arange(live.size), lens[live])).to(device)
    d_items = torch.from_numpy(items).to(device)
    bounds = np.concatenate([[0], np.cumsum(lens[live])])
    adaptive = model._loss in _host.MULTI_NEGATIVE_LOSSES  # every candidate row of the column goes to the loss
    score =lambda ids: (u[row_of] * table[ids]).sum(1) + ub[row_of] + bias[ids]
    for t in range(T):
        opt.zero_grad()
        pos = score(d_items)
        negs = torch.stack([score(neg[t, r]) for r in range(neg.shape[1])])  # [nn, n]
        total = None
        for i in range(live.size):
            lo, hi = int(bounds[i]), int(bounds[i + 1])
            term = loss_func(pos[lo:hi], negs[:, lo:hi] if adaptive else negs[0, lo:hi])
            total = term if total is None else total + term
        total.backward()
        if isinstance(opt, optim.SparseAdam):  # every row is touched at every step: the dense gradient IS the sparse one
            for p in (u, ub):
                p.grad = p.grad.to_sparse()
        opt.step()
    emb, b = emb.copy(), b.copy()
    emb[live] = u.detach().cpu().numpy()
    b[live] = ub.detach().cpu().numpy()
    return emb, b


def fold_in(model, interactions, n_iter=None, init=None, negatives=None, generic=False):
    table, bias, plain = _item_side(model, 'fold_in')
    off, items, H = history_csr(model, interactions)
    n = int(off[-1])
    T = model._n_iter if n_iter is None else int(n_iter)
    if T < 1:
        raise ValueError('n_iter must be at least 1, got {!r}'.format(n_iter))
    dim = int(table.shape[1])
    nn = model._num_negative_samples if model._loss in _host.MULTI_NEGATIVE_LOSSES else 1
    if H < 1:
        return np.zeros((0, dim), np.float32), np.zeros(0, np.float32)
    device = table.device
    engine, stream = _host._engine_for(device), _host._stream_for(device)
    _refuse_inside_open_scope(engine, stream, table, bias, model._num_items)
    emb, b = _initial_rows(model, init, H, dim)
    neg = _negatives(model, negatives, T, nn, n, device, engine, stream)
    # (sampled softmax: every candidate of a position is live -- not the fused gather's pair / column rule; slk_bilinear_foldin
    # refuses it and the generic route, whose [nn, n] negatives are per position already, trains through losses.softmax_loss)
    if plain and not generic and model._loss != 'softmax':
        u, ub = torch.from_numpy(emb).to(device), torch.from_numpy(b).to(device)
        try:
            binding = _host._OptimizerBinding(_fresh_optimizer(model, [u, ub]), [u, ub], model._sparse)
        except NotImplementedError:
            binding = None  # an optimizer without a fused update: the generic route trains with it
        if binding is not None:
            slots = lambda s: [s[0].data_ptr(), None, s[1].data_ptr(), None] if s else None
            ostruct = _native.make_optim(binding.kind, slots(binding.s1), slots(binding.s2), step=0, **binding.hp)
            tables = _native.make_tables([u.data_ptr(), table.data_ptr(), ub.data_ptr(), bias.data_ptr()], H, model._num_items, dim)
            d_off = torch.from_numpy(off).to(device)
            d_items = torch.from_numpy(items if n else np.zeros(1, np.int64)).to(device)
            engine.bilinear_foldin(tables, ostruct, d_off.data_ptr(), d_items.data_ptr(), H, n, model._loss,
                                   model._num_negative_samples, T, neg.data_ptr(), None, stream)
            return u.cpu().numpy(), ub.cpu().numpy()
    return generic_steps(model, table, bias, off, items, neg, emb, b, T)


def recommend_vectors(model, embeddings, biases=None, k=10, exclude=None, generic=False):
    table, bias, plain = _item_side(model, 'recommend_vectors')
    k = _rec.check_k(k)
    I, dim = model._num_items, int(table.shape[1])
    emb = np.array(embeddings, dtype=np.float32, order='C')
    if emb.ndim == 1:
        emb = emb.reshape(1, -1)
    if emb.ndim != 2 or emb.shape[1] != dim:
        raise ValueError('embeddings must have shape (n, {}), got {}'.format(dim, emb.shape))
    n = emb.shape[0]
    b = np.zeros(n, np.float32) if biases is None else np.array(biases, dtype=np.float32, order='C').reshape(-1)
    if b.shape != (n,):
        raise ValueError('biases must hold one value per embedding row ({}), got {}'.format(n, b.shape))
    if not n:
        return _rec.empty_result(k)
    lists = _rec.exclusion_lists(exclude, np.arange(n), I)
    device = table.device
    engine, stream = _host._engine_for(device), _host._stream_for(device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    d_rep, d_rbias = dev(emb), dev(b)
    # the item side alone, as the row-sharded entries read it at world 1: local row == item id
    tables = _native.make_tables([None, table.data_ptr(), None, bias.data_ptr()], 0, I, dim)
    if k <= _rec.TOPK_K_MAX and plain and not generic:
        d_eo, d_ei = [dev(a) for a in _rec.csr_of(lists)] if lists is not None else (None, None)
        items = torch.empty((n, k), dtype=torch.int64, device=device)
        scores = torch.empty((n, k), dtype=torch.float32, device=device)
        engine.shard_topk(tables, d_rep.data_ptr(), d_rbias.data_ptr(), n, k, d_eo.data_ptr() if d_eo is not None else None,
                          d_ei.data_ptr() if d_ei is not None else None, items.data_ptr(), scores.data_ptr(), stream)
        return items.cpu().numpy(), scores.cpu().numpy()

    def score_rows(idx):
        lo, m = int(idx[0]), len(idx)
        out = torch.empty((m, I), dtype=torch.float32, device=device)
        engine.shard_scores(tables, d_rep[lo:lo + m].data_ptr(), d_rbias[lo:lo + m].data_ptr(), m, out.data_ptr(), stream)
        return out.cpu().numpy()
    return _rec.generic_topk(score_rows, np.arange(n), I, k, lists)
