"""ExplicitFactorizationModel -- drop-in for spotlight/factorization/explicit.py:21-284.

The explicit-feedback sibling of ImplicitFactorizationModel: the same BilinearNet and the same
fused gather / dot / backward / row-update kernels, with observed ratings instead of sampled
negatives and the regression / poisson / logistic losses of spotlight/losses.py:169-244
(include/spotlight_hip.h: slk_bilinear_train_explicit).  Same constructor, fit(), predict(),
error behaviour and random-state consumption as the reference (one draw in the constructor, one
numpy-exact shuffle of the three arrays per epoch, computed on the device).
"""
import contextlib

import numpy as np
import torch

from spotlight_amd import _epochs
from spotlight_amd.factorization._components import _predict_process_ids
from spotlight_amd.factorization import implicit as _host
from spotlight_amd.factorization.implicit import ImplicitFactorizationModel
from spotlight_amd.torch_utils import set_seed


class _ExplicitEpochs(object):
    """What the schedules of spotlight_amd/_epochs.py ask of the explicit-feedback model: the shuffle of the three arrays and
    slk_bilinear_train_explicit.  `lane_stream`: the raw stream of the two-lane schedule's prep lane (two sets of epoch
    buffers, the ratings converted on that stream); None under the serial schedule (one set, this thread's stream).
    `sources`: users, items, the ratings' int64 carriers and -- a fit on interaction weights (use_weights=True) -- the weights';
    a set of epoch buffers is one buffer per source, then the float32 values read back out of each carrier."""

    def __init__(self, model, binding, tables, sources, device, lane_stream=None):
        self.binding, self.tables, self.sources, self.n = binding, tables, sources, sources[0].numel()
        self.call = (self.n, model._batch_size, model._loss)
        self.mb_loss = torch.empty((self.n + model._batch_size - 1) // model._batch_size, dtype=torch.float32, device=device)
        self.floats = len(sources) - 2
        self.slots = [[torch.empty_like(d) for d in sources] +
                      [torch.empty(self.n, dtype=torch.float32, device=device) for _ in range(self.floats)]
                      for _ in range(1 if lane_stream is None else 2)]
        self.d_perm = torch.empty(self.n, dtype=torch.int64, device=device)
        self.side = (torch.cuda.ExternalStream(lane_stream, device=device)
                     if lane_stream is not None and device.type == 'cuda' else None)

    def prepare(self, engine, stream, random_state, epoch_num):
        slot = self.slots[epoch_num % len(self.slots)]
        _epochs.device_epoch_shuffle(engine, random_state, self.n, self.d_perm,
                                     [(src, dst, 1) for src, dst in zip(self.sources, slot)], stream)
        # (on the prep lane's stream where there is one: the state read-back that follows then covers the conversion too)
        with torch.cuda.stream(self.side) if self.side is not None else contextlib.nullcontext():
            for k in range(self.floats):  # the float32 bit patterns back out of their int64 carriers
                slot[2 + self.floats + k].view(torch.int32).copy_(slot[2 + k])

    def train(self, engine, stream, epoch_num):
        slot = self.slots[epoch_num % len(self.slots)]
        d_users, d_items, d_ratings = slot[0], slot[1], slot[2 + self.floats]
        ostruct = self.binding.as_struct()
        if self.floats == 2:
            n, batch_size, loss = self.call
            engine.bilinear_train_weighted(self.tables, ostruct, d_users.data_ptr(), d_items.data_ptr(), slot[5].data_ptr(), n,
                                           batch_size, loss, 0, self.mb_loss.data_ptr(), d_ratings=d_ratings.data_ptr(),
                                           stream=stream)
        else:
            engine.bilinear_train_explicit(self.tables, ostruct, d_users.data_ptr(), d_items.data_ptr(), d_ratings.data_ptr(),
                                           *self.call, self.mb_loss.data_ptr(), stream=stream)
        self.binding.store_steps(ostruct.step)


class ExplicitFactorizationModel(ImplicitFactorizationModel):
    """Explicit-feedback matrix factorization (ratings).  Parameters follow
    spotlight/factorization/explicit.py:68-79; `use_cuda` is accepted for signature compatibility
    (the model always lives on the HIP device), `representation` may be a BilinearNet.  `use_weights` (not in the reference):
    False ignores `Interactions.weights`, as the reference does; True fits the weighted regression / likelihood
    sum(w_i * l_i) / sum(w_i) per minibatch (ImplicitFactorizationModel's docstring: same checks, same schedule, same
    RandomState as the unweighted fit)."""

    def __init__(self, loss='regression', embedding_dim=32, n_iter=10, batch_size=256, l2=0.0,
                 learning_rate=1e-2, optimizer_func=None, use_cuda=False, representation=None, sparse=False,
                 random_state=None, use_weights=False):

        assert loss in ('regression', 'poisson', 'logistic')

        self._loss = loss
        self._embedding_dim = embedding_dim
        self._n_iter = n_iter
        self._learning_rate = learning_rate
        self._batch_size = batch_size
        self._l2 = l2
        self._use_cuda = use_cuda
        self._representation = representation
        self._sparse = sparse
        self._optimizer_func = optimizer_func
        self._random_state = random_state or np.random.RandomState()
        self._use_weights = bool(use_weights)

        self._num_users = None
        self._num_items = None
        self._net = None
        self._optimizer = None
        self._loss_func = None
        self._binding = None

        # consumes one draw of the stream, like the reference (explicit.py:103-104)
        set_seed(self._random_state.randint(-10**8, 10**8), cuda=self._use_cuda)

    def fit(self, interactions, verbose=False):
        """Fit the model on interactions that carry ratings; repeated calls resume
        (explicit.py:173-243)."""
        with _host.fit_scope(self):
            return self._fit(interactions, verbose)

    def _fit(self, interactions, verbose):
        user_ids, item_ids = interactions.user_ids, interactions.item_ids

        if not self._initialized:
            self._initialize(interactions)

        self._check_input(user_ids, item_ids)
        if interactions.ratings is None:
            # the reference fails inside shuffle() when it indexes None (explicit.py:201-204)
            raise TypeError("'NoneType' object is not subscriptable: explicit feedback needs interactions.ratings")
        iw = _host.interaction_weights(getattr(self, '_use_weights', False), interactions)  # (ValueError before anything is drawn)

        binding = self._bind()
        device = self._net.tables()[0].device
        engine = _host._engine_for(device)
        stream = _host._stream_for(device)
        n = len(user_ids)
        # ids and ratings go to the device once; the ratings ride through the shuffle as int64 bit
        # patterns (slk_gather_rows_i64 moves 8-byte elements)
        ratings = np.ascontiguousarray(interactions.ratings, dtype=np.float32)
        sources = [_host.ids_to_device(user_ids, device), _host.ids_to_device(item_ids, device), _host.float_carrier(ratings, device)]
        if iw is not None:  # the weights ride the shuffle beside the ratings
            sources.append(_host.float_carrier(iw, device))
        # The reference's README example fits MovieLens-100K with batch_size 256: training draws nothing from the RandomState,
        # so epochs of that scale shuffle epoch e + 1 on a second slk_ctx / HIP stream while epoch e trains (_epochs.run_two_lane).
        # Same permutations, same RandomState afterwards, bit-identical tables.
        # (a fit on interaction weights: the two-lane schedule at every size)
        if iw is not None or (self._n_iter > 1 and n <= _host._PIPELINE_MAX_DRAWS):
            lane = _host._prep_lane_for(device)
            job = _ExplicitEpochs(self, binding, self._slk_tables(), sources, device, lane_stream=lane[1])
            return _epochs.run_two_lane(engine, stream, lane, self._random_state, self._n_iter, verbose, job, device)
        job = _ExplicitEpochs(self, binding, self._slk_tables(), sources, device)
        return _epochs.run_serial(engine, stream, self._random_state, self._n_iter, verbose, job)

    def fold_in(self, interactions, n_iter=None, init=None, negatives=None):
        raise NotImplementedError('fold_in() of the explicit-feedback model is not built (INTEGRATION.md 2m): its step needs the new '
                                  "users' ratings and has no negatives")

    def recommend_vectors(self, embeddings, biases=None, k=10, exclude=None):
        raise NotImplementedError('recommend_vectors() of the explicit-feedback model is not built (INTEGRATION.md 2m): it goes with '
                                  'fold_in()')

    def predict(self, user_ids, item_ids=None):
        """Predicted ratings for one user against all/some items, or for explicit (user, item) pairs:
        exp() of the score under the poisson loss, sigmoid() under the logistic one (explicit.py:245-284)."""
        self._check_input(user_ids, item_ids, allow_items_none=True)
        self._net.train(False)

        users, items, n = _predict_process_ids(user_ids, item_ids, self._num_items)
        device = self._net.tables()[0].device
        engine = _host._engine_for(device)
        d_users = torch.from_numpy(users).to(device)
        d_items = torch.from_numpy(items).to(device) if items is not None else None
        out = torch.empty(n, dtype=torch.float32, device=device)
        engine.bilinear_predict(self._slk_tables(), d_users.data_ptr(), users.size,
                                d_items.data_ptr() if d_items is not None else None, n,
                                out.data_ptr(), _host._stream_for(device))
        if self._loss == 'poisson':
            out = torch.exp(out)
        elif self._loss == 'logistic':
            out = torch.sigmoid(out)
        return out.cpu().numpy().flatten()

    # evaluation.mrr_score's device fast path ranks raw scores; predicted ratings (exp / sigmoid of them)
    # take the generic predict() route, as in the reference (evaluation.py:9-56)
    _batch_scores = None
    _fused_ranks = None
