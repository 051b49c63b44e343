"""ALSFactorizationModel -- implicit-feedback matrix factorization trained by alternating least squares (Hu, Koren and
Volinsky, "Collaborative Filtering for Implicit Feedback Datasets"; the headline algorithm of the `implicit` library).  The
reference has no such trainer.

With p_ui = 1 for the observed pairs and the confidence c_ui = 1 + alpha * r_ui, fit() minimises

    L = sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2 + regularization * (sum_u |x_u|^2 + sum_i |y_i|^2)

by exact half-steps: with the item table fixed every user row is the solution of its own dim x dim system, then the same for
the items (csrc/slk_als.hip: slk_als_gram, slk_als_solve; include/spotlight_hip.h states the contract).  No learning rate, no
negative sampler, no random numbers after the tables are initialised; deterministic.

The model is an ImplicitFactorizationModel whose tables ALS has filled: predict(), recommend(), recommend_vectors(),
similar_items(), similar_users(), the fast paths of evaluation.py, pickling and the id checks are the parent's.
"""
import numpy as np
import torch

from spotlight_amd import _epochs
from spotlight_amd.factorization import implicit as _host
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.factorization.representations import BilinearNet
from spotlight_amd.layers import BloomEmbedding, ScaledEmbedding, ZeroEmbedding

# keywords of the parent's constructor that have no meaning without a loss function, an optimizer and a negative sampler
_NO_MEANING = ('loss', 'batch_size', 'l2', 'learning_rate', 'optimizer_func', 'sparse', 'num_negative_samples', 'negative_sampling',
               'negative_sampling_power', 'verify_negatives', 'verify_tries')
_NORM_CHUNK_ROWS = 1 << 20  # rows per float64 temporary of the objective's |Y|^2


class _Csr(object):
    """Histories of one side on the device: off int64 [rows + 1], cols int64 [nnz] (ascending within a row, duplicates merged),
    vals float32 [nnz] = c - 1 = alpha * r.  Empty arrays keep one element so that their address is never NULL."""

    def __init__(self, off, cols, vals, n_rows):
        pad = lambda t, dtype: t.contiguous() if t.numel() else torch.zeros(1, dtype=dtype, device=off.device)
        self.off, self.cols, self.vals = off.contiguous(), pad(cols, torch.int64), pad(vals, torch.float32)
        self.n_rows, self.nnz = int(n_rows), int(cols.numel())


def merged_pairs(rows, cols, weights, n_cols):
    """The distinct (row, col) pairs of the int64 device tensors `rows` / `cols`, sorted by (row, col), and r per pair in
    float64: its number of occurrences, or with `weights` (float32, one per occurrence) their sum.  The sum is a segmented one
    without atomics and without a pass per duplicate: a float64 prefix sum over the weights in stably sorted order (order of
    appearance inside a pair), differenced at the pairs' boundaries -- the same bits on every run, whatever the multiplicities.
    A pair's sum carries an absolute error of at most a few 2^-53 of the prefix it is cut from (at most the sum of ALL weights):
    exact for weights that are small integers or share a power-of-two scale, and far below one float32 rounding of a sum that is
    not vanishingly small beside the total.  Set-up, not the sweep path: stock tensor ops."""
    key = rows * n_cols + cols
    if weights is None:
        ukey, counts = torch.unique_consecutive(torch.sort(key).values, return_counts=True)
        return ukey // n_cols, ukey % n_cols, counts.to(torch.float64)
    skey, order = torch.sort(key, stable=True)
    ukey, counts = torch.unique_consecutive(skey, return_counts=True)
    prefix = torch.cumsum(weights[order].to(torch.float64), 0)
    end = torch.cumsum(counts, 0) - 1  # the last occurrence of every pair
    total = prefix[end] if end.numel() else prefix
    r = total - torch.cat([total.new_zeros(1), total[:-1]]) if end.numel() else total
    return ukey // n_cols, ukey % n_cols, r


def build_csrs(user_ids, item_ids, weights, num_users, num_items, alpha, device):
    """(histories by user, histories by item) as _Csr on `device` from host id arrays (and float32 weights or None)."""
    if num_users * num_items >= 1 << 62:
        raise ValueError('num_users * num_items must be below 2^62')
    dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
    users, items = dev(user_ids, np.int64), dev(item_ids, np.int64)
    u, i, r = merged_pairs(users, items, dev(weights, np.float32) if weights is not None else None, num_items)
    vals = (r * float(alpha)).to(torch.float32)
    bounds = lambda sorted_rows, n: torch.searchsorted(sorted_rows, torch.arange(n + 1, dtype=torch.int64, device=device))
    by_user = _Csr(bounds(u, num_users), i, vals, num_users)
    order = torch.sort(i * num_users + u).indices  # (the pairs are distinct: any sort gives the same order)
    by_item = _Csr(bounds(i[order], num_items), u[order], vals[order], num_items)
    return by_user, by_item


class ALSFactorizationModel(ImplicitFactorizationModel):
    """Implicit-feedback matrix factorization trained by alternating least squares.

    Parameters
    ----------
    embedding_dim: int, at most 128 (and a multiple of 4 above 64)
    n_iter: int, iterations per fit(); one iteration is a user half-step followed by an item half-step
    regularization: float >= 0, the lambda of the objective
    alpha: float > 0, the confidence of one interaction: c_ui = 1 + alpha * r_ui
    use_weights: False (default): r_ui is the number of times the pair occurs in the fit() call.  True: the sum of the pair's
        `Interactions.weights`, which must be finite and > 0 (ValueError before anything runs)
    use_cuda: accepted for signature compatibility; the model always lives on the HIP device
    random_state: numpy RandomState; consumed by the constructor and by the initialisation of the tables exactly as the
        parent consumes it, never afterwards

    fit() appends the value of L after every iteration to `loss_history_`.  The biases are zero and stay zero.  A second fit()
    continues from the current tables.  Not supported: BloomEmbedding tables (ValueError), any other custom `representation`
    and the row-sharded model (NotImplementedError)."""

    def __init__(self, embedding_dim=32, n_iter=15, regularization=0.01, alpha=40.0, use_weights=False, use_cuda=False,
                 random_state=None, representation=None, **refused):
        for name in refused:
            if name in _NO_MEANING:
                raise TypeError('ALSFactorizationModel() has no {!r}: alternating least squares has no loss function to choose, no '
                                'optimizer, no minibatches and no negative sampler'.format(name))
            raise TypeError('ALSFactorizationModel() got an unexpected keyword argument {!r}'.format(name))
        if representation is not None:
            _check_representation(representation)
        _check_dim(embedding_dim, 'embedding_dim')
        if not (np.isfinite(regularization) and regularization >= 0):
            raise ValueError('regularization must be finite and >= 0, got {!r}'.format(regularization))
        if not (np.isfinite(alpha) and alpha > 0):
            raise ValueError('alpha must be finite and > 0, got {!r}'.format(alpha))
        if int(n_iter) < 0:
            raise ValueError('n_iter must be >= 0, got {!r}'.format(n_iter))
        super(ALSFactorizationModel, self).__init__(embedding_dim=int(embedding_dim), n_iter=int(n_iter), use_cuda=use_cuda,
                                                    representation=representation, random_state=random_state,
                                                    use_weights=use_weights)
        self._loss = 'als'
        self._regularization = float(regularization)
        self._alpha = float(alpha)
        self.loss_history_ = []

    def _initialize(self, interactions):
        super(ALSFactorizationModel, self)._initialize(interactions)
        _check_representation(self._net)
        self.loss_history_ = []

    def _bind(self):
        """No optimizer is bound: there is no optimizer state to allocate (the parent's _initialize would create Adam's two
        moment tensors per table here)."""
        return None

    # -- the trainer ------------------------------------------------------------------------------------------------------------
    def _device_side(self):
        tables = [t.detach() for t in self._net.tables()]
        for t in tables:
            if not (t.is_contiguous() and t.dtype == torch.float32):
                raise RuntimeError('model tables must be contiguous fp32 tensors on the HIP device')
        device = tables[0].device
        return tables, device, _host._engine_for(device), _host._stream_for(device)

    def _refuse_open_scope(self, engine, stream, tables):
        """What predict() raises inside an open fit() scope of a model on these tables (the item-bias shadow); the doubled user
        table of such a scope is refused by the engine's own entries."""
        from spotlight_amd import foldin as _foldin
        _foldin._refuse_inside_open_scope(engine, stream, tables[1], tables[3].reshape(-1), self._num_items)

    def _solve(self, engine, stream, fixed, gram, csr, rows, out):
        """One half-step into `out`; the counter of failed rows is read back once."""
        failed = torch.zeros(1, dtype=torch.int32, device=out.device)
        engine.als_solve(fixed.data_ptr(), gram.data_ptr(), fixed.shape[1], self._regularization, csr.off.data_ptr(), csr.cols.data_ptr(),
                         csr.vals.data_ptr(), rows.data_ptr() if rows is not None else None, csr.n_rows if rows is None else rows.numel(),
                         out.data_ptr(), failed.data_ptr(), stream)
        count = int(failed.item())
        if count:
            raise ValueError('{} of {} rows have a system that is not positive definite in float32 and were left as they were: '
                             'use a larger regularization (got {!r})'.format(count, csr.n_rows, self._regularization))

    def _gram(self, engine, stream, table):
        gram = torch.empty((table.shape[1], table.shape[1]), dtype=torch.float32, device=table.device)
        engine.als_gram(table.data_ptr(), table.shape[0], table.shape[1], gram.data_ptr(), stream)
        return gram

    def _objective(self, engine, stream, users, items, gram_items, by_user):
        per_row = torch.empty(by_user.n_rows, dtype=torch.float64, device=users.device)
        engine.als_loss(users.data_ptr(), items.data_ptr(), gram_items.data_ptr(), users.shape[1], self._regularization,
                        by_user.off.data_ptr(), by_user.cols.data_ptr(), by_user.vals.data_ptr(), by_user.n_rows, per_row.data_ptr(),
                        stream)
        norm = 0.0
        for lo in range(0, items.shape[0], _NORM_CHUNK_ROWS):
            norm += float(items[lo:lo + _NORM_CHUNK_ROWS].to(torch.float64).square().sum())
        return float(per_row.sum()) + self._regularization * norm

    def _prepare(self, interactions):
        """Everything fit() checks and builds before the first half-step: weights and ids validated, tables initialised, the
        open-scope refusal, both CSRs on the device."""
        weights = _host.interaction_weights(self._use_weights, interactions)
        user_ids, item_ids = interactions.user_ids, interactions.item_ids
        if not self._initialized:
            self._initialize(interactions)
        if len(user_ids):
            self._check_input(user_ids, item_ids)
        tables, device, engine, stream = self._device_side()
        self._refuse_open_scope(engine, stream, tables)
        if bool(tables[2].any()) or bool(tables[3].any()):
            raise ValueError('ALSFactorizationModel needs zero bias tables: the objective has no bias terms')
        by_user, by_item = build_csrs(user_ids, item_ids, weights, self._num_users, self._num_items, self._alpha, device)
        return tables, engine, stream, by_user, by_item

    def fit(self, interactions, verbose=False):
        """n_iter iterations of (user half-step, item half-step) on the interactions; appends L to loss_history_ after each.
        Opens no training scope and draws nothing from random_state once the tables are initialised."""
        tables, engine, stream, by_user, by_item = self._prepare(interactions)
        users, items = tables[0], tables[1]
        gram_items = self._gram(engine, stream, items)
        for it in range(self._n_iter):
            self._solve(engine, stream, items, gram_items, by_user, None, users)
            self._solve(engine, stream, users, self._gram(engine, stream, users), by_item, None, items)
            gram_items = self._gram(engine, stream, items)  # of the new item table: this iteration's L, the next user half-step
            value = self._objective(engine, stream, users, items, gram_items, by_user)
            self.loss_history_.append(value)
            _epochs.end_epoch(it, value, verbose)

    def fold_in(self, interactions, **refused):
        """Rows for users who arrived after fit(): (embeddings float32 [H, dim], biases float32 [H], all zero) -- ONE user
        half-step over the new users' histories against the frozen item table.  No steps, no negatives, no random numbers; the
        model is not modified.  `interactions`: as for the parent's fold_in() (user ids 0 .. H - 1, the model's item ids);
        duplicate pairs are merged, r as in fit() (`interactions.weights` under use_weights=True).  A user without interactions
        gets the zero row.  recommend_vectors() serves the users from these rows."""
        for name in refused:
            raise TypeError('ALSFactorizationModel.fold_in() has no {!r}: a fold-in is one exact half-step, without steps, initial '
                            'rows or negatives'.format(name))
        if self._net is None:
            raise RuntimeError('fold_in() needs a fitted model')
        weights = _host.interaction_weights(self._use_weights, interactions)
        users = np.asarray(interactions.user_ids).reshape(-1)
        item_ids = np.asarray(interactions.item_ids).reshape(-1)
        H = int(interactions.num_users)
        tables, device, engine, stream = self._device_side()
        dim = int(tables[1].shape[1])  # the item table's own dim: a `representation=` net's dim wins over the embedding_dim keyword
        if users.size:
            if users.max() >= H:
                raise ValueError('Maximum user id greater than number of users in interactions.')
            _host._reject_negative_ids(users)
            self._check_item_id_max(item_ids)
            _host._reject_negative_ids(item_ids)
        if H < 1:
            return np.zeros((0, dim), np.float32), np.zeros(0, np.float32)
        self._refuse_open_scope(engine, stream, tables)
        by_user, _ = build_csrs(users, item_ids, weights, H, self._num_items, self._alpha, device)
        rows = torch.empty((H, dim), dtype=torch.float32, device=device)
        self._solve(engine, stream, tables[1], self._gram(engine, stream, tables[1]), by_user, None, rows)
        return rows.cpu().numpy(), np.zeros(H, np.float32)

    def _fold_in_generic(self, interactions, **kw):
        raise NotImplementedError('ALSFactorizationModel.fold_in() is one exact half-step: there is no generic route')


def _check_dim(dim, what):
    """The dims the engine's ALS entries accept: at most 128, and a multiple of 4 above 64."""
    if not 1 <= int(dim) <= 128 or (dim > 64 and dim % 4):
        raise ValueError('{} must be at most 128, and a multiple of 4 above 64, got {!r}'.format(what, dim))


def _check_representation(net):
    """ValueError for BloomEmbedding tables and for a dim the engine does not solve, NotImplementedError for anything but a
    plain BilinearNet."""
    if not isinstance(net, BilinearNet):
        raise NotImplementedError('ALSFactorizationModel supports the plain BilinearNet only: {} (a custom representation, or the '
                                  'row-sharded model) has no ALS trainer'.format(type(net).__name__))
    for layer in (net.user_embeddings, net.item_embeddings):
        if isinstance(layer, BloomEmbedding):
            raise ValueError('ALSFactorizationModel does not support BloomEmbedding tables: a hashed row is shared by many ids, '
                             'so no id has a least-squares system of its own')
        if not isinstance(layer, ScaledEmbedding) and type(layer) is not torch.nn.Embedding:
            raise NotImplementedError('ALSFactorizationModel supports plain embedding layers only, got {}'.format(type(layer).__name__))
    for layer in (net.user_biases, net.item_biases):
        if not isinstance(layer, (ZeroEmbedding, torch.nn.Embedding)):
            raise NotImplementedError('ALSFactorizationModel supports plain bias layers only, got {}'.format(type(layer).__name__))
    dims = {int(layer.weight.shape[1]) for layer in (net.user_embeddings, net.item_embeddings)}
    if len(dims) != 1:
        raise ValueError('the representation\'s user and item tables must have one dim, got {}'.format(sorted(dims)))
    _check_dim(dims.pop(), 'the representation\'s embedding dim')
