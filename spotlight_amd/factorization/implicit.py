"""ImplicitFactorizationModel -- drop-in for spotlight/factorization/implicit.py:22-311.

Same constructor, fit(), predict(), error messages and random-state behaviour as the
reference; everything inside the epoch loop (negative sampling, both forward passes, loss,
backward, optimizer update) is one C-ABI call into csrc/libspotlight_hip.so per epoch.
"""
import contextlib
import inspect

import numpy as np
import torch
import torch.optim as optim

from spotlight_amd import _epochs, _native
from spotlight_amd._epochs import IdUpload, device_epoch_shuffle, ids_to_device  # noqa: F401 -- reached through this module
from spotlight_amd.factorization._components import _predict_process_ids
from spotlight_amd.factorization.representations import BilinearNet
from spotlight_amd.helpers import _repr_model
from spotlight_amd.layers import BloomEmbedding, ScaledEmbedding, ZeroEmbedding
from spotlight_amd import sampling as _sampling
from spotlight_amd.torch_utils import set_seed

_ENGINES = {}
# fit(): epochs of at most this many negative draws prepare the next epoch while training.  Larger epochs do not gain:
# at 10^8 interactions the two lanes time-slice the chip (train 71 ms + prepare 38 ms alone, 100 ms together:
# profiles/r02_m_*_at_1e8_no_gain.json)
_PIPELINE_MAX_DRAWS = 1 << 22
_VERIFY_MAX_CANDIDATES = 1 << 25  # verify_negatives=True: candidates one draw covers at the most (a 256-MB scratch buffer)
_DEFERRED_CHECK_MIN = 1 << 22  # ids per fit() from which the id-range checks run on worker threads beside the upload
_PREFETCH = True  # large epochs: the next epoch's first chunk is prepared beside the last passes of this one (test switch)
# Item tables of at least this many rows train with their biases and the biases' Adagrad accumulator interleaved for the duration
# of fit() (include/spotlight_hip.h: slk_bias_shadow_begin): on such tables a minibatch's biases share no cache line and the two
# scalars cost the item pass a quarter of its memory requests (12.5 % of them are saved: C5 shard).
_BIAS_SHADOW_MIN_ITEMS = 1 << 24
# Minibatches of at least this many interactions (pair losses, plain tables, row-sparse optimizers) train on a DOUBLED user table
# for the duration of fit() (include/spotlight_hip.h: slk_user_pingpong_begin): the user pass writes a user's updated row to the
# copy that does not hold the current one and no pre-step-row record (a row per interaction: 13 % of the pass's traffic), the item
# pass gathers the pre-step row where it still stands.  Below, the passes are latency-bound and the record is cache-resident.
_USER_PINGPONG_MIN_BATCH = 1 << 17
# The column losses: num_negative_samples draws per positive, viewed as [n, B] (implicit.py:266-275), one selection per column --
# adaptive hinge the largest candidate, warp the first violating one (include/spotlight_hip.h: SLK_LOSS_WARP)
COLUMN_LOSSES = ('adaptive_hinge', 'warp')
# The multi-negative losses: num_negative_samples draws per positive, ONE draw of B * n per minibatch.  The column losses view it
# as [n, B]; sampled softmax keeps flat draw f with the user it was drawn for -- negative f % n of positive f // n
# (include/spotlight_hip.h: SLK_LOSS_SOFTMAX)
MULTI_NEGATIVE_LOSSES = COLUMN_LOSSES + ('softmax',)


def _engine_for(device):
    """One slk_ctx per (process, HIP device)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _ENGINES:
        _ENGINES[index] = _native.Engine(index)
    return _ENGINES[index]


# What a fit() asks of the shared ctx FOR ITS OWN DURATION (it used to be set once, process-wide, on the
# ctx every model, evaluation and to_sequence of the process share).  Epochs are runs of multi-chunk training calls: the next
# chunk's negatives + sorts go to the ctx's second stream beside the current chunk's passes (include/spotlight_hip.h, option
# "overlap_prep"; a bare ctx keeps them in line).
_FIT_OPTIONS = {'overlap_prep': 1}


def fit_scope(model):
    """`with fit_scope(model):` -- _FIT_OPTIONS on the model's engine for the block, the previous values afterwards."""
    net = getattr(model, '_net', None)
    device = net.tables()[0].device if (net is not None and hasattr(net, 'tables')) else _model_device()
    return _engine_for(device).options(**_FIT_OPTIONS)


def _stream_for(device):
    """Raw hipStream_t of torch's current stream on `device`."""
    return torch.cuda.current_stream(device).cuda_stream


_PREP = {}


def _prep_lane_for(device):
    """(engine, raw stream) on which the NEXT epoch's shuffle and negatives are prepared while the current epoch trains
    (fit() of small datasets, see ImplicitFactorizationModel.fit): a second slk_ctx with its own scratch and a side HIP
    stream.  Under the GPU-less test harness it is a second ctx of the same (synchronous, single-threaded) emulator library:
    two ctxs, as on the GPU -- what the prep lane does to its RNG state must not reach the training ctx."""
    engine = _engine_for(device)
    if _native._LIB is None or engine._lib is not _native._LIB:
        twin = getattr(engine, '_prep_twin', None)
        if twin is None:
            twin = engine._prep_twin = _native.Engine(0, lib=engine._lib)
        return twin, _stream_for(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _PREP:
        _PREP[index] = (_native.Engine(index), torch.cuda.Stream(device))
    prep_engine, side = _PREP[index]
    return prep_engine, side.cuda_stream


def _model_device():
    """The HIP device models live on.  (The GPU-less test harness substitutes these three
    hooks to drive the same host logic through its emulator build of the kernels.)"""
    if not torch.cuda.is_available():
        raise RuntimeError('spotlight_amd needs a HIP device (MI355X): torch.cuda.is_available() '
                           'is False and there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def interaction_weights(use_weights, interactions):
    """The float32 weights a fit() with use_weights=True trains on (None without it: interactions.weights is ignored, as the
    reference ignores it): one per interaction, finite and strictly positive -- an interaction of weight 0 is one to drop, and a
    minibatch whose weights sum to 0 has no loss.  ValueError otherwise; draws nothing."""
    if not use_weights:
        return None
    if interactions.weights is None:
        raise ValueError('use_weights=True needs interactions.weights')
    weights = np.asarray(interactions.weights)
    if weights.ndim != 1 or len(weights) != len(interactions.user_ids):
        raise ValueError('interactions.weights: one weight per interaction is needed')
    try:
        weights = np.ascontiguousarray(weights, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError('interactions.weights must be numbers')
    if not np.isfinite(weights).all():
        raise ValueError('interactions.weights must be finite (float32)')
    if weights.size and weights.min() <= 0:
        raise ValueError('interactions.weights must be strictly positive: drop an interaction instead of weighting it 0')
    return weights


def float_carrier(values, device):
    """float32 values as the int64 bit patterns slk_gather_rows_i64 moves through the epoch shuffle (8-byte elements)."""
    return torch.from_numpy(values).to(device).view(torch.int32).to(torch.int64)


def _state_tensor(state, key, like):
    if key not in state:
        state[key] = torch.zeros_like(like, memory_format=torch.preserve_format)
    return state[key]


def _reject_negative_ids(ids):
    """The reference's torch embedding raises IndexError on a negative id; the kernels address rows with
    unsigned 32-bit ids, so a negative one must never reach them."""
    id_min = ids if isinstance(ids, int) else np.asarray(ids).min()
    if id_min < 0:
        raise IndexError('index out of range in self')


# param-group keys that select an implementation of the same arithmetic (torch/optim/optimizer.py), never another rule
_ARITHMETIC_NEUTRAL_KEYS = ('foreach', 'fused', 'capturable', 'differentiable')


def _refuse_unread_options(optimizer, group, read):
    """A param-group key that the binding neither reads (`read`) nor knows to be arithmetic-neutral, set to something
    else than the optimizer class's own default, asks for a rule the fused update does not have: NotImplementedError, so
    that fit() takes the autograd route with the real torch optimizer instead of silently ignoring the option.
    LIMITATION: the defaults are those of type(optimizer).__init__'s signature.  A key that signature does not name has no
    default to differ from and is skipped: a scheduler's 'initial_lr' (rightly), but also an option that a subclass of
    Adagrad / SparseAdam takes through **kwargs and writes into its param groups -- such a subclass is bound as its base class."""
    defaults = inspect.signature(type(optimizer).__init__).parameters
    for key, value in group.items():
        if key == 'params' or key in read or key in _ARITHMETIC_NEUTRAL_KEYS or key not in defaults:
            continue
        default = defaults[key].default
        same = (value is default) or (not torch.is_tensor(value) and not torch.is_tensor(default) and value == default)
        if not same:
            raise NotImplementedError('{}({}={!r}) has no fused gfx950 update'.format(type(optimizer).__name__, key, value))


class _OptimizerBinding(object):
    """Maps a torch.optim object onto slk_optim.  The torch optimizer stays the owner of
    hyper-parameters and state tensors (so state_dict / pickle / resuming fit() behave as
    in the reference); the kernels update those tensors in place."""

    def __init__(self, optimizer, params, sparse):
        self.optimizer = optimizer
        self.params = params
        groups = optimizer.param_groups
        if len(groups) != 1:
            raise NotImplementedError('spotlight_amd supports a single optimizer param group')
        g = groups[0]
        if g.get('maximize', False):
            raise NotImplementedError('maximize=True is not supported')
        st = optimizer.state
        if isinstance(optimizer, optim.Adagrad):
            wd = g['weight_decay']
            if sparse and wd != 0:
                # torch/optim/adagrad.py:355-358
                raise RuntimeError('weight_decay option is not compatible with sparse gradients')
            # (initial_accumulator_value is already in state['sum'], torch/optim/adagrad.py:80-90)
            _refuse_unread_options(optimizer, g, ('lr', 'eps', 'weight_decay', 'lr_decay', 'initial_accumulator_value', 'maximize'))
            self.kind = 'adagrad_dense' if wd != 0 else 'adagrad'
            self.hp = dict(lr=g['lr'], eps=g['eps'], weight_decay=wd, lr_decay=g['lr_decay'])
            self.s1 = [st[p]['sum'] for p in params]
            self.s2 = None
        elif isinstance(optimizer, optim.SparseAdam):
            if not sparse:
                raise RuntimeError('SparseAdam does not support dense gradients, please consider '
                                   'Adam instead')
            _refuse_unread_options(optimizer, g, ('lr', 'eps', 'betas', 'maximize'))
            self.kind = 'sparse_adam'
            self.hp = dict(lr=g['lr'], eps=g['eps'], betas=g['betas'])
            for p in params:
                st[p].setdefault('step', 0)
            self.s1 = [_state_tensor(st[p], 'exp_avg', p) for p in params]
            self.s2 = [_state_tensor(st[p], 'exp_avg_sq', p) for p in params]
        elif type(optimizer) is optim.Adam:
            if sparse:
                raise RuntimeError('Adam does not support sparse gradients, please consider '
                                   'SparseAdam instead')
            if g.get('amsgrad', False):
                raise NotImplementedError('amsgrad=True is not supported')
            if g.get('decoupled_weight_decay', False) and g['weight_decay'] != 0:
                # AdamW's rule, p *= 1 - lr * wd (torch/optim/adam.py); the fused update adds wd * p to the gradient
                raise NotImplementedError('decoupled_weight_decay=True with a non-zero weight_decay is not supported')
            _refuse_unread_options(optimizer, g, ('lr', 'eps', 'betas', 'weight_decay', 'amsgrad', 'maximize', 'decoupled_weight_decay'))
            self.kind = 'adam_dense'
            self.hp = dict(lr=g['lr'], eps=g['eps'], betas=g['betas'], weight_decay=g['weight_decay'])
            for p in params:
                if 'step' not in st[p]:
                    st[p]['step'] = torch.tensor(0.0, dtype=torch.float32)
            self.s1 = [_state_tensor(st[p], 'exp_avg', p) for p in params]
            self.s2 = [_state_tensor(st[p], 'exp_avg_sq', p) for p in params]
        elif type(optimizer) is optim.SGD:
            # torch/optim/sgd.py, the plain form: param.add_(grad, alpha=-lr).  Stateless, and a zero gradient is a zero update, so
            # dense and sparse gradients give the same row-sparse step.  Momentum / weight decay / Nesterov would touch every row
            # every step and have no fused form.
            if g.get('momentum', 0) != 0 or g.get('weight_decay', 0) != 0 or g.get('nesterov', False):
                raise NotImplementedError('torch.optim.SGD has a fused gfx950 update only with momentum=0, weight_decay=0, '
                                          'nesterov=False')
            # (dampening scales the gradient's share of a momentum buffer: without momentum there is none)
            _refuse_unread_options(optimizer, g, ('lr', 'momentum', 'dampening', 'weight_decay', 'nesterov', 'maximize'))
            self.kind = 'sgd'
            self.hp = dict(lr=g['lr'])
            self.s1 = None
            self.s2 = None
        else:
            raise NotImplementedError(
                'optimizer {} has no fused gfx950 update; supported: Adam (default), Adagrad, SparseAdam, SGD '
                '(momentum=0)'.format(type(optimizer).__name__))
        for t in (self.s1 or []) + (self.s2 or []):
            if not t.is_contiguous():
                raise RuntimeError('optimizer state must be contiguous')

    def steps_taken(self):
        if self.kind == 'sgd':  # stateless (and touching optimizer.state[...] would create an entry)
            return 0
        step = self.optimizer.state[self.params[0]].get('step', 0)
        return int(step.item()) if torch.is_tensor(step) else int(step)

    def as_struct(self):
        return _native.make_optim(self.kind, [t.data_ptr() for t in self.s1] if self.s1 else None,
                                  [t.data_ptr() for t in self.s2] if self.s2 else None,
                                  step=self.steps_taken(), **self.hp)

    def store_steps(self, step):
        if self.kind == 'sgd':  # stateless: torch keeps no step count for it either
            return
        for p in self.params:
            s = self.optimizer.state[p]
            if torch.is_tensor(s.get('step')):
                s['step'].fill_(float(step))
            else:
                s['step'] = int(step)


class _ImplicitEpochs(object):
    """What the schedules of spotlight_amd/_epochs.py ask of the implicit model: the epoch buffers (`slots`: (users, items) of
    the three-stage schedule's ShuffledIds, or (users, items, negatives) of its own under the two-lane one) and the entry
    points slk_bilinear_reserve / _prefetch / _train over the model's tables, optimizer and hyper-parameters."""

    def __init__(self, model, binding, tables, n, device):
        self.binding, self.tables, self.n, self.device, self.num_items = binding, tables, n, device, model._num_items
        self.dist = getattr(model, '_item_distribution', None)  # None: uniform negatives
        self.call = (n, model._batch_size, model._loss, model._num_negative_samples)
        self.mb_loss = torch.empty((n + model._batch_size - 1) // model._batch_size, dtype=torch.float32, device=device)
        self.slots, self.scopes, self.sources, self.weighted, self.side = [], [], None, False, None
        self.seen = self.d_cand = self.d_counts = self.d_rep = None  # verified negatives (verify_with)
        self.tries, self.nn = 1, 1

    def verify_with(self, seen, tries, nn):
        """Two-lane schedule, verify_negatives=True: every epoch's negatives are the first unseen of `tries` candidates
        (slk_verify_negatives against the bound SeenItems `seen`).  The candidates of a group of minibatches are drawn into
        one scratch buffer of at most _VERIFY_MAX_CANDIDATES values (a minibatch's block at the least); the counters are
        summed on the device over the whole fit()."""
        self.seen, self.tries, self.nn = seen, int(tries), int(nn)
        bsz = self.call[1]
        # sampled softmax: flat slot f of a minibatch belongs to user f // nn, not to the column f % bm of the view(nn, bm) that
        # slk_verify_negatives checks against -- the same flat layout read as ONE negative row over the users repeated user-major
        self.own_user = self.call[2] == 'softmax' and self.nn > 1
        per_mb = bsz * self.nn * self.tries
        self.group = max(1, _VERIFY_MAX_CANDIDATES // per_mb) * bsz  # interactions per draw: whole minibatches
        self.d_cand = torch.empty(min(self.n, self.group) * self.nn * self.tries, dtype=torch.int64, device=self.device)
        self.d_counts = torch.zeros(2, dtype=torch.int64, device=self.device)

    def _draw_verified(self, engine, stream, d_users, d_neg):
        """The epoch's T-fold draw, group by group (consecutive draws are one draw: the ids do not depend on the grouping),
        each followed on the same stream by the selection into the slot's negatives."""
        seen = self.seen
        for lo in range(0, self.n, self.group):
            m = min(self.group, self.n - lo)
            _sampling.draw_items(engine, self.num_items, m * self.nn * self.tries, self.d_cand.data_ptr(), stream, self.dist)
            users, m_v, bsz_v, nn_v = d_users.data_ptr() + 8 * lo, m, self.call[1], self.nn
            if self.own_user:
                if self.d_rep is None:
                    self.d_rep = torch.empty(min(self.n, self.group) * self.nn, dtype=torch.int64, device=self.device)
                # the copy goes to the very stream the draw and the selection are enqueued on, whichever stream is current in
                # this thread (a handle of 0 is the device's null stream: torch's default stream)
                side = None
                if self.device.type == 'cuda':
                    side = torch.cuda.ExternalStream(stream, device=self.device) if stream else torch.cuda.default_stream(self.device)
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    self.d_rep[:m * self.nn].view(m, self.nn).copy_(d_users[lo:lo + m].unsqueeze(1).expand(m, self.nn))
                users, m_v, bsz_v, nn_v = self.d_rep.data_ptr(), m * self.nn, self.call[1] * self.nn, 1
            engine.verify_negatives(users, m_v, bsz_v, nn_v, self.tries, self.d_cand.data_ptr(),
                                    seen.d_off.data_ptr(), seen.d_items.data_ptr(), seen.num_users,
                                    d_neg.data_ptr() + 8 * lo * self.nn, self.d_counts.data_ptr(), stream=stream)

    def reserve(self, engine, stream):
        engine.bilinear_reserve(self.tables, self.binding.as_struct(), *self.call, stream=stream)

    def own_slots(self, sources, nn, lane_stream=None):
        """Two-lane schedule: two sets of epoch buffers, shuffled from the uploaded `sources` -- (users, items) or, for a fit on
        interaction weights, (users, items, the weights' int64 carriers); such a set then ends with the carriers' buffer and
        the float32 weights read back out of it on the prep lane's stream (`lane_stream`)."""
        self.sources, self.weighted = sources, len(sources) > 2
        extra = lambda: ((torch.empty_like(sources[2]), torch.empty(self.n, dtype=torch.float32, device=self.device))
                         if self.weighted else ())
        self.slots = [(torch.empty_like(sources[0]), torch.empty_like(sources[1]),
                       torch.empty(self.n * nn, dtype=torch.int64, device=self.device)) + extra() for _ in range(2)]
        if self.weighted and lane_stream is not None and self.device.type == 'cuda':
            self.side = torch.cuda.ExternalStream(lane_stream, device=self.device)
        # (the permutation AFTER the epoch buffers, all of one size class in the caching allocator: allocated first it cost a
        # MovieLens-100K fit() 0.9 %, profiles/fit_driver_parent_vs_head.json, sessions 1 and 2)
        self.d_perm = torch.empty(self.n, dtype=torch.int64, device=self.device)

    def prepare(self, engine, stream, random_state, epoch_num):
        slot = self.slots[epoch_num % 2]
        d_neg = slot[2]
        # (the weights travel with their interactions: a third array through the same permutation)
        _epochs.device_epoch_shuffle(engine, random_state, self.n, self.d_perm,
                                     [(src, dst, 1) for src, dst in zip(self.sources, slot[:2] + slot[3:4])], stream)
        if self.weighted:  # (on the prep lane's stream: the state read-back behind the negatives covers the conversion)
            with torch.cuda.stream(self.side) if self.side is not None else contextlib.nullcontext():
                slot[4].view(torch.int32).copy_(slot[3])
        if self.seen is not None:
            return self._draw_verified(engine, stream, slot[0], d_neg)
        # one randint (one choice) per minibatch == one contiguous draw over the epoch (sampling.py:34)
        _sampling.draw_items(engine, self.num_items, d_neg.numel(), d_neg.data_ptr(), stream, self.dist)

    def open_scopes(self, stack, engine, stream):
        shadow, pingpong = self.scopes
        stack.enter_context(shadow)  # (from here to the scope's end the item-bias tensors are stale: nothing inside reads them)
        stack.enter_context(pingpong)  # (... and the user-embedding tensor holds only some of the current rows)
        if pingpong.active:  # the scope's {dL/dscore, src} pairs are wider than the one-table layout's side array: grown now,
            self.reserve(engine, stream)  # not inside the first training call

    def prefetch(self, engine, stream, epoch_num, state):
        d_users, d_items = self.slots[epoch_num % len(self.slots)]
        engine.bilinear_prefetch(self.tables, self.binding.as_struct(), d_users.data_ptr(), d_items.data_ptr(), *self.call,
                                 state=state, stream=stream)

    def train(self, engine, stream, epoch_num):
        slot = self.slots[epoch_num % len(self.slots)]
        d_neg = slot[2].data_ptr() if len(slot) > 2 else None  # (handed in under the two-lane schedule, else drawn by the call)
        ostruct = self.binding.as_struct()
        if self.weighted:
            engine.bilinear_train_weighted(self.tables, ostruct, slot[0].data_ptr(), slot[1].data_ptr(), slot[4].data_ptr(),
                                           *self.call, self.mb_loss.data_ptr(), d_neg_in=d_neg, stream=stream)
        else:
            engine.bilinear_train(self.tables, ostruct, slot[0].data_ptr(), slot[1].data_ptr(), *self.call,
                                  self.mb_loss.data_ptr(), d_neg_in=d_neg, stream=stream)
        self.binding.store_steps(ostruct.step)


class ImplicitFactorizationModel(object):
    """Implicit-feedback matrix factorization trained by negative sampling.

    Parameters and semantics follow spotlight/factorization/implicit.py:76-88.  Two
    notes specific to this implementation:

    * `use_cuda` is accepted for signature compatibility; the model always lives on the HIP
      device (there is no CPU path).
    * `representation` may be a :class:`BilinearNet` (fused kernels) or any torch module with the reference's
      `forward(user_ids, item_ids)` contract; a custom module, or an `optimizer_func` whose optimizer has no fused update
      (anything but Adam / Adagrad / SparseAdam / plain SGD), trains through the AUTOGRAD ROUTE: the reference's own
      minibatch loop (implicit.py:208-252) in stock PyTorch-ROCm ops on the HIP device -- host numpy shuffle and
      negatives exactly as the reference draws them, the embedding gathers and their backward through this package's
      kernels when the module is built from this package's layers.  Slower than the fused path by the reference's own
      per-minibatch overheads, never on the CPU.
    * `loss='warp'` (not in the reference): the rank-weighted hinge of WSABIE / LightFM's `loss='warp'`.  Of a positive's
      `num_negative_samples` draws -- adaptive hinge's, in its `view(n, B)` layout, all drawn and scored up front -- the FIRST one
      that violates the margin (`neg - pos + 1 > 0`) is trained against, the hinge scaled by `log(max(1, (num_items - 1) // tries))`;
      a positive without a violator contributes nothing.  The RandomState is consumed exactly as by `loss='adaptive_hinge'` with
      the same `num_negative_samples`.  The rank estimate assumes uniform draws: under `negative_sampling='popularity'` it is a
      popularity-weighted rank (include/spotlight_hip.h: SLK_LOSS_WARP; `spotlight_amd.losses.warp_loss` on the autograd route).
    * `loss='softmax'` (not in the reference): sampled softmax (InfoNCE).  A positive and ITS OWN `num_negative_samples` draws go
      into one softmax, `logsumexp([pos; negs]) - pos`, and every candidate carries a gradient in proportion to how wrongly it is
      ranked -- no margin, no rank estimate.  The draws are adaptive hinge's (one draw of B * n per minibatch; the RandomState is
      consumed exactly as by `loss='adaptive_hinge'` with the same `num_negative_samples`), but each draw stays with the user it
      was drawn for instead of the reference's `view(n, B)` column.  Composes with `use_weights`, `negative_sampling` (no logQ
      correction: popular items are then over-penalised in proportion to their sampling rate) and `verify_negatives` (each draw is
      checked against its own user); fold_in() takes its generic route (include/spotlight_hip.h: SLK_LOSS_SOFTMAX;
      `spotlight_amd.losses.softmax_loss` on the autograd route).
    * `negative_sampling` (not in the reference): what the negatives are drawn from.  'uniform' or None: every item alike
      (`RandomState.randint`, the reference's sampler).  'popularity': in proportion to
      `count(item) ** negative_sampling_power` (word2vec's unigram distribution; default power 0.75), the counts taken over
      the interactions of the fit() call in progress -- an item that does not occur there has weight 0 and is NEVER drawn as
      a negative.  An array of `num_items` finite, non-negative weights with a positive sum: in proportion to them (checked
      at fit(); ValueError before anything is drawn).  A weighted draw is `RandomState.choice(num_items, size=..., p=p)` on
      the model's RandomState, made on the device bit for bit (csrc/slk_rng.hip); fit() then prepares every epoch's
      negatives beside the epoch before it at every size (the two-lane schedule), and fold_in() draws from the distribution
      of the last fit().
    * `use_weights` (not in the reference, which carries `Interactions.weights` and never reads them): False (default) ignores
      the weights, as the reference does.  True: fit() minimises, per minibatch, sum(w_i * l_i) / sum(w_i) over the
      per-interaction terms l_i of the loss (adaptive hinge: a column carries the weight of its positive) -- play counts, dwell
      times, recency decay.  `interactions.weights` must then be given, finite and > 0 (ValueError before anything is drawn).
      Shuffles, negatives and the RandomState are those of the unweighted fit; the weights ride the shuffle with their
      interactions.  Such a fit runs the two-lane schedule at every size and opens neither training scope (item-bias shadow,
      user-row ping-pong); dL/dscore is formed ahead of the user pass (include/spotlight_hip.h: slk_bilinear_train_weighted).
      fold_in() stays unweighted.
    * `verify_negatives` (not in the reference; LightFM and implicit's `verify_negative_samples`): False (default) uses every
      draw as it comes, as the reference does -- a "negative" may then be an item the user has interacted with.  True: per
      negative slot `verify_tries` (an int in [1, 16], default 4; ValueError at construction otherwise) candidates are drawn
      up front -- per minibatch ONE draw of verify_tries * nn * B values, so the RandomState ends where
      `sample_items(num_items, (verify_tries * nn, B))` per minibatch leaves it -- and the first one that is not in the
      user's history (the interactions of the fit() call in progress) is used; if all are seen, the first one, and the slot
      counts as unresolved (include/spotlight_hip.h: slk_verify_negatives; `spotlight_amd.sampling.verify_negatives` is the
      rule in numpy, which the autograd route applies).  verify_tries=1 trains exactly as verify_negatives=False does and
      only counts.  Such a fit runs the two-lane schedule at every size and composes with every loss, `use_weights` and
      `negative_sampling`.  Afterwards `negative_verification_` holds {'candidates': values drawn, 'replaced': slots that do
      not use their first candidate, 'unresolved'}, summed over the epochs, and `_seen_items` the histories' CSR (on the
      device until the next fit(); not pickled).  fold_in() stays unverified.
    """

    def __init__(self, loss='pointwise', embedding_dim=32, n_iter=10, batch_size=256, l2=0.0,
                 learning_rate=1e-2, optimizer_func=None, use_cuda=False, representation=None,
                 sparse=False, random_state=None, num_negative_samples=5, negative_sampling='uniform',
                 negative_sampling_power=0.75, use_weights=False, verify_negatives=False, verify_tries=4):

        assert loss in ('pointwise', 'bpr', 'hinge', 'adaptive_hinge', 'warp', 'softmax')
        _sampling.check_negative_sampling(negative_sampling)
        self._verify_tries = _sampling.check_verify_tries(verify_tries)
        self._verify_negatives = bool(verify_negatives)
        self._seen_items = None  # sampling.SeenItems of the last verifying fit()
        self.negative_verification_ = None  # {'candidates', 'replaced', 'unresolved'} of the last verifying fit()

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
        self._num_negative_samples = num_negative_samples
        self._negative_sampling = negative_sampling
        self._negative_sampling_power = negative_sampling_power
        self._item_distribution = None  # sampling.ItemDistribution of the last fit() (None: uniform)
        self._use_weights = bool(use_weights)

        self._num_users = None
        self._num_items = None
        self._net = None
        self._optimizer = None
        self._loss_func = None
        self._binding = None
        self._autograd_route = False

        # consumes one draw of the stream, like the reference (implicit.py:114-115)
        set_seed(self._random_state.randint(-10**8, 10**8), cuda=self._use_cuda)

    def __repr__(self):
        return _repr_model(self)

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_binding'] = None  # holds raw pointers; rebuilt on the next fit()
        return state

    @property
    def _initialized(self):
        return self._net is not None

    def _initialize(self, interactions):
        self._num_users, self._num_items = interactions.num_users, interactions.num_items
        self._autograd_route = False
        if self._representation is not None:
            net = self._representation
        else:
            net = BilinearNet(self._num_users, self._num_items, self._embedding_dim,
                              sparse=self._sparse)
        if not isinstance(net, BilinearNet):
            self._autograd_route = True  # an arbitrary module: the reference's loop through autograd (see the class docstring)
            self._fused_ranks = None
            self._batch_scores = None    # (evaluation's whole-table fast path needs BilinearNet's tables; predict() serves it)
        else:
            for layer in (net.user_embeddings, net.item_embeddings):
                if not isinstance(layer, (ScaledEmbedding, BloomEmbedding)) and type(layer) is not torch.nn.Embedding:
                    self._autograd_route = True
            if not isinstance(net.user_biases, (ZeroEmbedding, torch.nn.Embedding)):
                self._autograd_route = True
        self._net = net.to(_model_device())

        if self._optimizer_func is None:
            self._optimizer = optim.Adam(self._net.parameters(), weight_decay=self._l2,
                                         lr=self._learning_rate)
        else:
            self._optimizer = self._optimizer_func(self._net.parameters())
        self._loss_func = self._loss  # the loss is fused into the kernel; kept for introspection
        self._binding = None
        if not self._autograd_route:
            try:
                self._bind()
            except NotImplementedError:
                # an optimizer without a fused update (RMSprop, SGD with momentum, ...): the reference accepts any
                # optimizer_func (implicit.py:150), so does this model -- through the autograd route
                self._autograd_route = True

    def _bind(self):
        if self._binding is None:
            tables = self._net.tables()
            for t in tables:
                if not (t.device.type == _model_device().type and t.is_contiguous()
                        and t.dtype == torch.float32):
                    raise RuntimeError('model tables must be contiguous fp32 tensors on the HIP device')
            self._binding = _OptimizerBinding(self._optimizer, tables, self._sparse)
        return self._binding

    def _check_user_id_max(self, user_ids):
        user_id_max = user_ids if isinstance(user_ids, int) else user_ids.max()
        if user_id_max >= self._num_users:
            raise ValueError('Maximum user id greater than number of users in model.')

    def _check_item_id_max(self, item_ids):
        item_id_max = item_ids if isinstance(item_ids, int) else item_ids.max()
        if item_id_max >= self._num_items:
            raise ValueError('Maximum item id greater than number of items in model.')

    def _id_checks(self, user_ids, item_ids):
        """The checks of _check_input as separate functions, in the order they raise (one reduction over a host array each)."""
        return [lambda: self._check_user_id_max(user_ids), lambda: _reject_negative_ids(user_ids),
                lambda: self._check_item_id_max(item_ids), lambda: _reject_negative_ids(item_ids)]

    def _check_input(self, user_ids, item_ids, allow_items_none=False):
        checks = self._id_checks(user_ids, item_ids)
        for f in (checks[:2] if allow_items_none and item_ids is None else checks):
            f()

    def _slk_tables(self):
        return self._net.slk_tables()

    def fit(self, interactions, verbose=False):
        """Fit the model; repeated calls resume from the current parameters and optimizer
        state (implicit.py:184-252)."""
        with fit_scope(self):
            return self._fit(interactions, verbose)

    def _fit(self, interactions, verbose):
        user_ids, item_ids = interactions.user_ids, interactions.item_ids

        if not self._initialized:
            self._initialize(interactions)

        n = len(user_ids)
        nn = self._num_negative_samples if self._loss in MULTI_NEGATIVE_LOSSES else 1
        autograd = getattr(self, '_autograd_route', False)
        # non-uniform negatives are handed in at every size (the two-lane schedule): the three-stage pipeline's
        # slk_bilinear_prefetch draws uniform ones ahead of time
        weighted = not _sampling.is_uniform(getattr(self, '_negative_sampling', None))
        # interaction weights (use_weights=True; a model pickled before the keyword existed has none): validated with the item
        # weights, before anything is drawn.  They ride the two-lane schedule's shuffle at every size, too.
        iw = interaction_weights(getattr(self, '_use_weights', False), interactions)
        # verified negatives (verify_negatives=True; absent from a model pickled before the keyword existed): the selection runs
        # between the draw and the training call, so these negatives are handed in at every size as well
        verifying = getattr(self, '_verify_negatives', False)
        small = weighted or iw is not None or verifying or (self._n_iter > 1 and n * nn <= _PIPELINE_MAX_DRAWS)
        # the id-range checks (implicit.py:169-182): four reductions over the host arrays, 12 ms at 2^25 ids.  On the large-epoch
        # path they run on worker threads beside the id upload and the first epoch's shuffle; their verdict is collected before
        # the first training call is enqueued (nothing the caller can observe has changed by then: the RandomState is restored,
        # the tables are untouched).
        check = _epochs._Deferred(self._id_checks(user_ids, item_ids),
                                  threaded=not (autograd or small) and n >= _DEFERRED_CHECK_MIN)
        if not check.threaded:
            check.result()
        # the item weights of this fit(): validated (ValueError) before anything is drawn from the RandomState
        self._item_distribution = _sampling.item_distribution(getattr(self, '_negative_sampling', None),
                                                              getattr(self, '_negative_sampling_power', 0.75), self._num_items,
                                                              item_ids)
        # ... and the histories of this fit() that a verifying one checks its negatives against
        self._seen_items = (_sampling.SeenItems.from_interactions(user_ids, item_ids, self._num_users, self._num_items)
                            if verifying else None)
        self.negative_verification_ = None
        if autograd:
            return self._fit_autograd(user_ids, item_ids, verbose, iw)
        binding = self._bind()
        device = self._net.tables()[0].device
        engine = _engine_for(device)
        stream = _stream_for(device)
        tables = self._slk_tables()
        if self._item_distribution is not None:
            self._item_distribution.bind(engine, device, stream)
        # bpr / hinge leave the user biases' gradient at exactly zero (+g - g), so a model the reference initialised (ZeroEmbedding)
        # keeps them identically zero; checked HERE, on the device, once per fit(): the user pass then does not fetch a cache line
        # per interaction for a table of zeros (include/spotlight_hip.h: SLK_TABLES_USER_BIAS_ZERO).  Same values either way.
        if (self._loss in ('bpr', 'hinge') and binding.kind in ('adagrad', 'sgd') and not tables.user_bloom and not tables.item_bloom
                and not bool(self._net.tables()[2].any())):
            tables.flags |= _native.TABLES_USER_BIAS_ZERO
        job = _ImplicitEpochs(self, binding, tables, n, device)
        job.reserve(engine, stream)
        lane = _prep_lane_for(device)
        # ids go to the device once (on a worker thread: the first epoch's permutation is drawn meanwhile); every epoch's
        # permutation x[shuffle_indices] of them (torch_utils.py:35-52) is computed there, bit-exact with numpy's Fisher-Yates
        if small:
            sources = IdUpload([user_ids, item_ids], device).result()
            job.own_slots(sources + ([float_carrier(iw, device)] if iw is not None else []), nn, lane_stream=lane[1])
            if not verifying:
                return _epochs.run_two_lane(engine, stream, lane, self._random_state, self._n_iter, verbose, job, device)
            job.verify_with(self._seen_items.bind(engine, device, stream, ids=sources[:2]), self._verify_tries, nn)
            _epochs.run_two_lane(engine, stream, lane, self._random_state, self._n_iter, verbose, job, device)
            # the counters, summed on the device over the epochs and read back once (no epoch: the schedule still prepared one)
            epochs = max(self._n_iter, 0)
            self._store_verification(epochs * n * nn, *(job.d_counts.cpu().tolist() if epochs else (0, 0)))
            return
        threaded = _PREFETCH and lane[0] is not engine and engine._lib is _native._LIB  # (the test harness's emulator is single-threaded)
        ids = _epochs.ShuffledIds(lane[0], lane[1], user_ids, item_ids, min(self._n_iter, 3 if _PREFETCH else 2), device)
        job.slots = ids.bufs
        job.scopes = [
            engine.bias_shadow(tables, binding.as_struct(), stream=stream,
                               enabled=(binding.kind == 'adagrad' and self._num_items >= _BIAS_SHADOW_MIN_ITEMS and
                                        self._batch_size >= 4096 and not tables.item_bloom)),
            engine.user_pingpong(tables, binding.as_struct(), stream=stream,
                                 enabled=(self._loss in ('pointwise', 'bpr', 'hinge') and binding.kind in ('adagrad', 'sparse_adam', 'sgd')
                                          and min(self._batch_size, n) >= _USER_PINGPONG_MIN_BATCH
                                          and not tables.user_bloom and not tables.item_bloom))]
        return _epochs.run_three_stage(engine, stream, self._random_state, self._n_iter, verbose, job, ids, check,
                                       prefetch=_PREFETCH, threaded=threaded)

    def _store_verification(self, slots, replaced, unresolved):
        """negative_verification_ of a verifying fit(): `slots` negatives were used, each the first unseen of verify_tries
        candidates; `replaced` of them are not the first candidate, `unresolved` had every candidate seen (and use the first)."""
        self.negative_verification_ = {'candidates': int(slots) * self._verify_tries, 'replaced': int(replaced),
                                       'unresolved': int(unresolved)}

    def _fit_autograd(self, user_ids, item_ids, verbose, weights=None):
        """The reference's epoch / minibatch loop (implicit.py:208-252, 254-275) for models without a fused path: host numpy
        shuffle and negatives from `random_state` (the reference's exact consumption of the stream), forward / loss /
        backward / optimizer.step() as stock torch ops on the HIP device.  `weights` (use_weights=True): shuffled with the ids,
        the minibatch loss is losses.py's weighted form."""
        from spotlight_amd import losses as _losses
        from spotlight_amd.sampling import sample_items
        from spotlight_amd.torch_utils import minibatch, shuffle
        loss_func = {'pointwise': _losses.pointwise_loss, 'bpr': _losses.bpr_loss, 'hinge': _losses.hinge_loss,
                     'adaptive_hinge': _losses.adaptive_hinge_loss,
                     'warp': lambda pos, neg, **kw: _losses.warp_loss(pos, neg, self._num_items, **kw),
                     'softmax': _losses.softmax_loss}[self._loss]
        device = next(self._net.parameters()).device
        self._net.train(True)

        seen = getattr(self, '_seen_items', None)  # verify_negatives=True: the numpy restatement of slk_verify_negatives
        counts = [0, 0, 0]  # slots, replaced, unresolved

        def negatives_for(batch_user, n_draws):
            if seen is None:
                return torch.from_numpy(sample_items(self._num_items, n_draws, random_state=self._random_state,
                                                     p=self._item_distribution)).to(device)
            # ONE draw of verify_tries * n_draws candidates, viewed [tries][n_draws / B][B]
            cand = sample_items(self._num_items, self._verify_tries * n_draws, random_state=self._random_state,
                                p=self._item_distribution)
            users, per_user = batch_user.cpu().numpy(), n_draws // len(batch_user)
            if self._loss == 'softmax':  # slot f belongs to user f // n: one "negative row" over the users repeated user-major
                users, per_user = np.repeat(users, per_user), 1
            picked, replaced, unresolved = _sampling.verify_negatives(cand, users, seen, per_user, self._verify_tries)
            for k, v in enumerate((n_draws, replaced, unresolved)):
                counts[k] += v
            return torch.from_numpy(np.ascontiguousarray(picked.reshape(-1))).to(device)

        for epoch_num in range(self._n_iter):
            arrays = shuffle(*((user_ids, item_ids) + ((weights,) if weights is not None else ())), random_state=self._random_state)
            tensors = [torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)).to(device) for x in arrays[:2]]
            if weights is not None:
                tensors.append(torch.from_numpy(np.ascontiguousarray(arrays[2])).to(device))
            epoch_loss, n_mb = 0.0, 0
            for batch in minibatch(*tensors, batch_size=self._batch_size):
                batch_user, batch_item = batch[:2]
                positive_prediction = self._net(batch_user, batch_item)
                if self._loss in COLUMN_LOSSES:
                    # implicit.py:266-275: users repeated user-major, ONE draw of B * n, scores viewed as [n, B]
                    n = self._num_negative_samples
                    batch_size = batch_user.size(0)
                    negative_items = negatives_for(batch_user, batch_size * n).view(batch_size * n)
                    batch_user_rep = batch_user.view(batch_size, 1).expand(batch_size, n).reshape(-1)
                    negative_prediction = self._net(batch_user_rep, negative_items).view(n, batch_size)
                elif self._loss == 'softmax':
                    # the same draw of B * n and the same user-major repeat, but each positive meets ITS OWN draws: [B, n] -> [n, B]
                    n = self._num_negative_samples
                    batch_size = batch_user.size(0)
                    negative_items = negatives_for(batch_user, batch_size * n).view(batch_size * n)
                    batch_user_rep = batch_user.view(batch_size, 1).expand(batch_size, n).reshape(-1)
                    negative_prediction = self._net(batch_user_rep, negative_items).view(batch_size, n).t()
                else:
                    negative_prediction = self._net(batch_user, negatives_for(batch_user, len(batch_user)))
                self._optimizer.zero_grad()
                loss = loss_func(positive_prediction, negative_prediction, weights=batch[2] if weights is not None else None)
                epoch_loss += loss.item()
                loss.backward()
                self._optimizer.step()
                n_mb += 1
            epoch_loss /= n_mb
            _epochs.end_epoch(epoch_num, epoch_loss, verbose)
        if seen is not None:
            self._store_verification(*counts)

    def predict(self, user_ids, item_ids=None):
        """Scores for one user against all/some items, or for explicit (user, item) pairs;
        returns a flat np.float32 array (implicit.py:277-311)."""
        self._check_input(user_ids, item_ids, allow_items_none=True)
        self._net.train(False)

        if getattr(self, '_autograd_route', False) and not isinstance(self._net, BilinearNet):
            # a custom module scores with its own forward, as in the reference
            users, items, n = _predict_process_ids(user_ids, item_ids, self._num_items)
            device = next(self._net.parameters()).device
            d_users = torch.from_numpy(np.broadcast_to(users, (n,)).astype(np.int64)).to(device)
            d_items = torch.from_numpy(items if items is not None else np.arange(self._num_items, dtype=np.int64)).to(device)
            with torch.no_grad():
                return self._net(d_users, d_items).cpu().numpy().flatten()

        users, items, n = _predict_process_ids(user_ids, item_ids, self._num_items)
        device = self._net.tables()[0].device
        engine = _engine_for(device)
        d_users = torch.from_numpy(users).to(device)
        d_items = torch.from_numpy(items).to(device) if items is not None else None
        out = torch.empty(n, dtype=torch.float32, device=device)
        engine.bilinear_predict(self._slk_tables(), d_users.data_ptr(), users.size,
                                d_items.data_ptr() if d_items is not None else None, n,
                                out.data_ptr(), _stream_for(device))
        return out.cpu().numpy().flatten()

    def _fused_ranks(self, user_ids, row_group, row_target, exc_off, exc_items):
        """Average ranks of the rows' target items (evaluation.mrr_score's fast path): one counting sweep of the item table
        per 64 rows on the matrix cores, no score matrix (csrc/slk_eval.hip, slk_bilinear_rank)."""
        users = np.ascontiguousarray(np.asarray(user_ids).reshape(-1), dtype=np.int64)
        self._check_input(users, None, allow_items_none=True)
        self._net.train(False)
        device = self._net.tables()[0].device
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int64))).to(device)
        d_users, d_rg, d_rt = dev(users), dev(row_group), dev(row_target)
        d_eo, d_ei = (dev(exc_off), dev(exc_items)) if exc_off is not None else (None, None)
        ranks = torch.empty(len(row_group), dtype=torch.float64, device=device)
        _engine_for(device).bilinear_rank(self._slk_tables(), d_users.data_ptr(), users.size, d_rg.data_ptr(), d_rt.data_ptr(),
                                          len(row_group), d_eo.data_ptr() if d_eo is not None else None,
                                          d_ei.data_ptr() if d_ei is not None else None, ranks.data_ptr(), _stream_for(device))
        return ranks.cpu().numpy()

    def _is_custom_net(self):
        return getattr(self, '_autograd_route', False) and not isinstance(self._net, BilinearNet)

    def _recommend_prepare(self, user_ids, k, exclude):
        from spotlight_amd import recommend as _rec
        k = _rec.check_k(k)
        users = np.ascontiguousarray(np.asarray(user_ids).reshape(-1), dtype=np.int64)
        if users.size:
            self._check_input(users, None, allow_items_none=True)
        self._net.train(False)
        return _rec, users, k, _rec.exclusion_lists(exclude, users, self._num_items)

    def _recommend_generic(self, users, k, lists):
        """Score rows a tile at a time, sorted on the host (spotlight_amd/recommend.py: generic_topk)."""
        from spotlight_amd import recommend as _rec
        if self._is_custom_net():  # a custom module scores with its own forward: one predict() per user
            rows = lambda us: np.stack([self.predict(int(u)) for u in us])
        else:
            rows = lambda us: self._batch_scores(us).cpu().numpy()
        return _rec.generic_topk(rows, users, self._num_items, k, lists)

    def recommend(self, user_ids, k=10, exclude=None):
        """The k best items of every user: (items int64 [n, k], scores float32 [n, k]), best first.

        Order: score descending (-0.0 == +0.0), ties to the smaller item id, a NaN score after every number -- a total order,
        so the result is the same on every route, grid and world size.  `exclude`: None, an Interactions / scipy sparse matrix
        (row u = the items to hide from user u: the `train` of mrr_score) or one index array per user; an excluded item never
        appears.  A user with fewer than k eligible items gets item -1 / score -inf in the tail.  Every score is the bits
        predict() returns for that (user, item), except that a zero may lose its sign (and a NaN its payload).

        k <= TOPK_K_MAX (128) selects inside the scoring sweep (csrc/slk_eval.hip, slk_bilinear_topk: one pass over the item
        table per 64 users, no score matrix, no library kernel); a larger k, or a custom representation module, sorts score
        rows a tile at a time."""
        _rec, users, k, lists = self._recommend_prepare(user_ids, k, exclude)
        if not users.size:
            return _rec.empty_result(k)
        if k > _rec.TOPK_K_MAX or self._is_custom_net():
            return self._recommend_generic(users, k, lists)
        device = self._net.tables()[0].device
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        d_users = dev(users)
        d_eo, d_ei = [dev(a) for a in _rec.csr_of(lists)] if lists is not None else (None, None)
        items = torch.empty((users.size, k), dtype=torch.int64, device=device)
        scores = torch.empty((users.size, k), dtype=torch.float32, device=device)
        _engine_for(device).bilinear_topk(self._slk_tables(), d_users.data_ptr(), users.size, k,
                                          d_eo.data_ptr() if d_eo is not None else None,
                                          d_ei.data_ptr() if d_ei is not None else None, items.data_ptr(), scores.data_ptr(),
                                          _stream_for(device))
        return items.cpu().numpy(), scores.cpu().numpy()

    def fold_in(self, interactions, n_iter=None, init=None, negatives=None):
        """Rows for users who arrived after fit(): (embeddings float32 [H, dim], biases float32 [H]) learned from the new users'
        own histories with the item parameters FROZEN.  The model is not modified (its RandomState is consumed, see below);
        recommend_vectors() serves the users from these rows.

        `interactions`: the new users' (user, item) pairs; the user ids label the new users 0 .. H - 1 (H =
        interactions.num_users), the item ids are the model's.  Duplicates are kept, the order within a user is the order of
        appearance.  One step of user u is one reference minibatch made of u's interactions alone (mean over them), one
        optimizer step on u's row and bias -- so a user's result does not depend on who else is in the call.  A user without
        interactions keeps their initial row.
        `n_iter`: steps (default: the model's).  `init`: None draws the rows from the model's RandomState as fit() initialises
        them (normal(0, 1 / dim); zero biases) -- before the negatives --, or an (embeddings, biases) pair.  `negatives`: None
        draws them on the device from the model's RandomState, consuming the stream exactly as n_iter successive
        sample_items(num_items, (nn, n)) calls would (nn = num_negative_samples under adaptive hinge, else 1); an array
        [n_iter, nn, n] (columns in history order: sorted by user, stable) is used as given and leaves the RandomState alone.
        A fresh optimizer of the model's own kind and hyper-parameters (optimizer_func) is created for the new rows.

        Plain tables with Adam / Adagrad / SparseAdam / plain SGD: one fused call (csrc/slk_foldin.hip).  An item
        BloomEmbedding (materialised once), any other optimizer_func, or a custom representation with `item_embeddings` /
        `item_biases`: the same steps through autograd (spotlight_amd/foldin.py).  A user BloomEmbedding has no per-user row:
        TypeError.  Refused inside an open fit() scope whose item biases are shadowed, as predict() is.
        Interaction weights do not enter: a model built with use_weights=True folds in unweighted (`interactions.weights` is not read)."""
        from spotlight_amd import foldin as _foldin
        return _foldin.fold_in(self, interactions, n_iter, init, negatives)

    def _fold_in_generic(self, interactions, n_iter=None, init=None, negatives=None):
        """fold_in() through the generic route whatever the model (what the tests compare the fused route with)."""
        from spotlight_amd import foldin as _foldin
        return _foldin.fold_in(self, interactions, n_iter, init, negatives, generic=True)

    def recommend_vectors(self, embeddings, biases=None, k=10, exclude=None):
        """recommend() for user VECTORS (fold_in()'s rows, or any [n, dim] array; `biases` default 0): the k best items of every
        row, in recommend()'s order, padding, exclusion forms (None, a sparse matrix / Interactions whose row r lists row r's
        items, one index array per row) and outputs.  The score of (row, item) is predict()'s: (dot + bias) + item bias, so the
        model's own trained rows give recommend()'s arrays bit for bit.  k <= TOPK_K_MAX on a plain item table selects inside
        the scoring sweep (slk_shard_topk over the item side alone); a larger k, or an item BloomEmbedding (materialised once),
        sorts score rows a tile at a time."""
        from spotlight_amd import foldin as _foldin
        return _foldin.recommend_vectors(self, embeddings, biases, k, exclude)

    def _embedding_table(self, attr, num_rows):
        """The dense float32 [num_rows, dim] device tensor behind the net's `attr` layer: a plain layer's weight in place; a
        BloomEmbedding's representation of id j (the sum of its hashed rows) materialised once with the module's own forward on
        arange(num_rows)."""
        layer = getattr(self._net, attr, None)
        if layer is None:
            raise TypeError('{} has no `{}`: similar_items() / similar_users() read the embedding table of the '
                            'representation module'.format(type(self._net).__name__, attr))
        weight = getattr(layer, 'weight', None)
        if isinstance(layer, BloomEmbedding) or weight is None or weight.dim() != 2 or weight.shape[0] != num_rows:
            device = next(layer.parameters()).device
            with torch.no_grad():
                return layer(torch.arange(num_rows, dtype=torch.int64, device=device)).reshape(num_rows, -1).float().contiguous()
        return weight.detach()

    def _similar(self, attr, num_rows, ids, k, metric, exclude_self, exclude, always=None, generic=False):
        """similar_items() / similar_users(): argument checks, exclusion lists, then spotlight_amd/recommend.py: similar_rows."""
        from spotlight_amd import recommend as _rec
        k, metric = _rec.check_k(k), _rec.check_metric(metric)
        table = self._embedding_table(attr, num_rows)
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
        if not ids.size:
            return _rec.empty_result(k)
        if attr == 'user_embeddings':
            self._check_input(ids, None, allow_items_none=True)
        else:
            self._check_item_id_max(ids)
            _reject_negative_ids(ids)
        self._net.train(False)
        lists = _rec.neighbor_lists(ids, num_rows, exclude_self, exclude, always)
        device = table.device
        return _rec.similar_rows(_engine_for(device), _stream_for(device), table, ids, k, metric, lists, generic=generic)

    def similar_items(self, item_ids, k=10, metric='cosine', exclude_self=True, exclude=None):
        """The k nearest items of every query item in the embedding space: (items int64 [n, k], scores float32 [n, k]), best
        first, in recommend()'s order and padding (score descending, -0.0 == +0.0, ties to the smaller id, NaN last; item -1 /
        score -inf where fewer than k rows are eligible).

        metric 'cosine': <q, v> / (|q| |v|), formed as (dot * 1/|q|) * 1/|v| with the dot product the fma chain of predict()
        and 1/|x| = 1 / sqrt(fma chain of x with itself); an all-zero row scores 0 against everything.  metric 'dot': the bare
        chain.  No biases enter.  `exclude_self` hides the query id from its own row; `exclude`: one index array per query,
        merged with it.  A BloomEmbedding table is materialised once per call ([num_items, dim]: the sums of the hashed rows).

        k <= TOPK_K_MAX (128) selects inside the scoring sweep (csrc/slk_eval.hip, slk_neighbors_topk: one pass over the table
        per 64 queries, no [n, num_items] score matrix); a larger k sorts score rows (slk_neighbors_scores) a tile at a time."""
        return self._similar('item_embeddings', self._num_items, item_ids, k, metric, exclude_self, exclude)

    def similar_users(self, user_ids, k=10, metric='cosine', exclude_self=True, exclude=None):
        """similar_items() over the user table.  Refused inside an open fit() scope whose user table is doubled (as predict()
        is: the tensor holds only some of the current rows until the scope ends)."""
        return self._similar('user_embeddings', self._num_users, user_ids, k, metric, exclude_self, exclude)

    def _batch_scores(self, user_ids):
        """[len(user_ids), num_items] device tensor: row r == predict(user_ids[r]) (bit-identical), a
        tile of users per pass over the item table (csrc/slk_eval.hip); used by evaluation.mrr_score."""
        users = np.ascontiguousarray(np.asarray(user_ids).reshape(-1), dtype=np.int64)
        self._check_input(users, None, allow_items_none=True)
        self._net.train(False)
        device = self._net.tables()[0].device
        d_users = torch.from_numpy(users).to(device)
        out = torch.empty((users.size, self._num_items), dtype=torch.float32, device=device)
        _engine_for(device).bilinear_scores(self._slk_tables(), d_users.data_ptr(), users.size, out.data_ptr(),
                                            _stream_for(device))
        return out
