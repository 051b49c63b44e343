"""The epoch loops behind every fused fit(): what is not specific to one model.

Three schedules consume the model's ONE numpy MT19937 stream in the reference's order -- shuffle(e), negatives(e),
shuffle(e + 1), ... (implicit.py:212-221, torch_utils.py:46-47, sampling.py:34) -- and differ only in what runs beside the
passes of an epoch:

  run_serial       nothing: set the state, shuffle, train, read the state back (large explicit / sequence epochs)
  run_two_lane     epoch e + 1's shuffle (and negatives) on a second slk_ctx / HIP stream (small epochs of every model)
  run_three_stage  the negatives of epoch e + 1 on the ctx's second stream and the shuffle of epoch e + 2 on the second
                   ctx (large epochs of the implicit model)

A schedule is handed the engines, streams and switches by the model (which resolves the hooks of factorization/implicit.py at
fit() time) and a per-model object that knows the model's buffers and its training entry point.  serial / two-lane ask it for
`mb_loss`, `prepare(engine, stream, random_state, epoch_num)` (shuffle -- and negatives where the model hands them in -- of one
epoch, drawn from the engine's RNG state) and `train(engine, stream, epoch_num)` (enqueue the epoch's training call);
three-stage asks for `mb_loss`, `train`, `open_scopes(stack, engine, stream)` and `prefetch(engine, stream, epoch_num, state)`.
On every way out a schedule leaves the RandomState where the reference would hold it: behind the negatives (explicit feedback:
the shuffle) of the last epoch whose training call was enqueued.  The module keeps no state of its own.
"""
import contextlib
import functools

import numpy as np
import torch

from spotlight_amd import _native


def ids_to_device(ids, device):
    """int64 device tensor of a host id array: uploaded in the array's own dtype (int32 in the reference's
    datasets: half the PCIe bytes) and widened on the device, instead of widening on the host first."""
    ids = np.ascontiguousarray(ids)
    if ids.dtype not in (np.int32, np.int64):
        ids = ids.astype(np.int64)
    return torch.from_numpy(ids).to(device).to(torch.int64)


def device_epoch_shuffle(engine, random_state, n, d_perm, arrays, stream):
    """d_dst = d_src[numpy-exact shuffle of arange(n)] for every (d_src, d_dst, row_len) of `arrays`,
    drawn from the engine's RNG state (slk_shuffle_perm: the reference's `shuffle`, torch_utils.py:35-52).
    If the device shuffle reports a failure (it cannot, short of a 12-sigma rejection tail) the
    permutation is drawn by numpy on the host from `random_state`, as the reference does, and the
    engine's RNG state is re-synchronised -- the results are identical either way.
    `arrays` may be a callable returning the list: it is called AFTER the permutation has been drawn (the permutation
    needs only n, so an upload of the ids can still be in flight while it is computed: IdUpload)."""
    try:
        engine.shuffle_perm(n, d_perm.data_ptr(), stream=stream)
    except _native.SlkError:
        order = np.arange(n)
        random_state.shuffle(order)
        d_perm.copy_(torch.from_numpy(order))
        engine.rng_set_state(random_state.get_state())
    if callable(arrays):
        arrays = arrays()
    for entry in arrays:
        if len(entry) == 4:  # ('pairs', d_pairs, d_users_dst, d_items_dst): both id arrays from their packed form in one pass
            _, d_pairs, d_users_dst, d_items_dst = entry
            engine.gather_id_pairs(d_pairs.data_ptr(), d_perm.data_ptr(), n, d_users_dst.data_ptr(), d_items_dst.data_ptr(),
                                   stream=stream)
            continue
        d_src, d_dst, row_len = entry
        engine.gather_rows_i64(d_src.data_ptr(), d_perm.data_ptr(), n, row_len, d_dst.data_ptr(), stream=stream)


class IdUpload(object):
    """The host -> HBM copy of fit()'s id arrays on a worker thread (ids_to_device; the copies release the GIL), so that the
    first epoch's permutation -- which needs only len(ids) -- is drawn on the GPU meanwhile.  result() joins and returns the
    int64 device tensors; the copies run on the worker's (default) stream, and a pageable copy has completed when the call
    returns, so after the join the data is in place for any stream."""

    def __init__(self, arrays, device):
        import threading
        self._out = [None] * len(arrays)
        self._err = []

        def work():
            try:
                if device.type == 'cuda':
                    torch.cuda.set_device(device)
                for k, a in enumerate(arrays):
                    self._out[k] = ids_to_device(a, device)
                if device.type == 'cuda':
                    torch.cuda.current_stream(device).synchronize()  # the widening kernels on this thread's stream
            except BaseException as e:  # re-raised by result()
                self._err.append(e)
        self._thread = threading.Thread(target=work, name='spotlight-id-upload')
        self._thread.start()

    def result(self):
        self._thread.join()
        if self._err:
            raise self._err[0]
        return self._out


class _Background(object):
    """fn() on a worker thread (or at once); join() returns its value or re-raises what it raised.  (Module level on purpose: a
    class created inside fit() would form a reference cycle through its closure and keep the epoch's id buffers -- GBs at
    bench scale -- out of the caching allocator until the cyclic collector runs; the next fit() then paid 20-50 ms of
    hipMalloc, profiles/r04_t_fit_first_epoch_probe.txt.)"""

    def __init__(self, fn, threaded):
        self._fn, self._out, self._err, self._thread = fn, None, None, None
        if threaded:
            import threading
            self._thread = threading.Thread(target=self._run, name='spotlight-epoch-shuffle')
            self._thread.start()
        else:
            self._run()

    def _run(self):
        try:
            self._out = self._fn()
        except BaseException as e:  # noqa: BLE001 -- re-raised by join()
            self._err = e
        self._fn = None

    def join(self):
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._err is not None:
            raise self._err
        return self._out


class _Deferred(object):
    """Every function of `fns` now, or each on a worker thread of its own; result() joins and re-raises the first error in
    the order of `fns` (the order the serial checks would have raised in)."""

    def __init__(self, fns, threaded):
        self.threaded = bool(threaded)
        self._errs, self._threads = [None] * len(fns), []

        def work(k):
            try:
                fns[k]()
            except BaseException as e:  # noqa: BLE001 -- re-raised by result()
                self._errs[k] = e
        for k in range(len(fns)):
            if self.threaded:
                import threading
                self._threads.append(threading.Thread(target=work, args=(k,), name='spotlight-id-check'))
                self._threads[-1].start()
            else:
                work(k)
                if self._errs[k] is not None:
                    break

    def join(self):
        for t in self._threads:
            t.join()
        self._threads = []

    def result(self):
        self.join()
        for k, e in enumerate(self._errs):
            if e is not None:
                self._errs = [None] * len(self._errs)
                raise e


def mean_loss(mb_loss):
    """Mean of per-minibatch loss.item() (implicit.py:240,245): one D2H per epoch; also waits for the epoch's kernels."""
    return float(mb_loss.double().mean().item())


def end_epoch(epoch_num, epoch_loss, verbose):
    """The reference's last lines of an epoch (implicit.py:245-252): it stops at a degenerate loss having consumed the
    stream up to this epoch's negatives only."""
    if verbose:
        print('Epoch {}: loss {}'.format(epoch_num, epoch_loss))
    if np.isnan(epoch_loss) or epoch_loss == 0.0:
        raise ValueError('Degenerate epoch loss: {}'.format(epoch_loss))


def run_serial(engine, stream, random_state, n_iter, verbose, job):
    """Nothing beside the passes: every epoch sets the engine's RNG state, shuffles, trains (the training call draws its own
    negatives) and reads the state back, which synchronises the stream."""
    consumed = random_state.get_state()
    try:
        for epoch_num in range(n_iter):
            engine.rng_set_state(random_state.get_state())
            job.prepare(engine, stream, random_state, epoch_num)
            job.train(engine, stream, epoch_num)
            consumed = engine.rng_get_state()  # synchronises the stream
            random_state.set_state(consumed)
            end_epoch(epoch_num, mean_loss(job.mb_loss), verbose)
    finally:  # (device_epoch_shuffle's host fall-back draws from random_state itself: an epoch that failed behind it is undone)
        random_state.set_state(consumed)


def _prepare_on_lane(prep, prep_stream, random_state, job, epoch_num):
    """One epoch's shuffle, then its negatives: one MT19937 stream, consumed on the prep lane exactly as numpy would consume
    it; random_state runs AHEAD of training from here on."""
    prep.rng_set_state(random_state.get_state())
    job.prepare(prep, prep_stream, random_state, epoch_num)
    random_state.set_state(prep.rng_get_state())  # synchronises the prep stream


def run_two_lane(engine, stream, lane, random_state, n_iter, verbose, job, device):
    """The epoch loop for datasets of the reference's own scale (MovieLens-100K: 80 000 interactions per epoch): there an
    epoch trains in about a millisecond and the numpy-exact device shuffle -- a chain of small launches and read-backs --
    costs as much again.  Nothing in training touches the RandomState stream, so epoch e + 1's shuffle and negatives are drawn
    on a second slk_ctx / HIP stream (`lane`) while epoch e trains from its own (already drawn) negatives.  Same ids, same
    negatives, same RandomState afterwards, bit-identical tables; only the wall time changes."""
    prep, prep_stream = lane
    if device.type == 'cuda':
        torch.cuda.current_stream(device).synchronize()  # the uploads are complete
    consumed = random_state.get_state()  # what the reference would hold: restored on every way out
    try:
        _prepare_on_lane(prep, prep_stream, random_state, job, 0)
        for epoch_num in range(n_iter):
            job.train(engine, stream, epoch_num)
            consumed = random_state.get_state()
            if epoch_num + 1 < n_iter:
                _prepare_on_lane(prep, prep_stream, random_state, job, epoch_num + 1)  # overlaps this epoch's training kernels
            epoch_loss = mean_loss(job.mb_loss)
            engine.check()  # errors the training kernels can only report through the ctx (e.g. an abandoned launch)
            end_epoch(epoch_num, epoch_loss, verbose)
    finally:
        random_state.set_state(consumed)


class ShuffledIds(object):
    """The id side of the three-stage schedule: the upload of the two id arrays (on a worker thread), their packed form, the
    permutation and `n_slots` pairs of epoch buffers, all on the prep lane (a second slk_ctx and its stream)."""

    def __init__(self, prep, prep_stream, user_ids, item_ids, n_slots, device):
        self.prep, self.prep_stream, self.device, self.n = prep, prep_stream, device, len(user_ids)
        self.bufs = [(torch.empty(self.n, dtype=torch.int64, device=device), torch.empty(self.n, dtype=torch.int64, device=device))
                     for _ in range(max(n_slots, 1))]
        self.d_perm = torch.empty(self.n, dtype=torch.int64, device=device)
        self.d_pairs = self._unpacked = None
        # (the upload starts AFTER the epoch buffers exist: its worker allocates from the same caching allocator, and racing it
        # for the blocks the previous fit() left there sent this thread to hipMalloc, 15 ms per pair of buffers)
        self.upload = IdUpload([user_ids, item_ids], device)

    def _sources(self, slot):
        # the uploaded ids, packed once per fit() into (user, item) pairs of 32 bits: a shuffled interaction is then
        # ONE random 8-byte read for both arrays (slk_gather_id_pairs)
        if self.d_pairs is None:
            self._unpacked = self.upload.result()  # (kept until the prep lane has been waited for, in shuffle_into)
            self.upload._out = None
            self.d_pairs = torch.empty(2 * self.n, dtype=torch.int32, device=self.device)
            # INVARIANT: with the id checks on worker threads (`check.threaded`) these ids are NOT validated
            # yet -- they are truncated to uint32, permuted and gathered as DATA only.  Nothing may index a table with
            # them, and no training call or prefetch may be enqueued, before `check.result()` has returned
            # (tests/test_host_model.py::test_id_checks_on_worker_threads_raise_like_the_serial_ones).
            self.prep.pack_id_pairs(self._unpacked[0].data_ptr(), self._unpacked[1].data_ptr(), self.n, self.d_pairs.data_ptr(),
                                    stream=self.prep_stream)
        return [('pairs', self.d_pairs, self.bufs[slot][0], self.bufs[slot][1])]

    def shuffle_into(self, slot, state):
        """bufs[slot] = ids[numpy-exact shuffle] drawn from `state` on the prep lane; returns the state behind the shuffle
        (reading it waits for the prep lane's stream: the gathers are complete)."""
        fallback = np.random.RandomState()  # (device_epoch_shuffle's host fall-back draws from it: private to this call)
        fallback.set_state(state)
        if self.device.type == 'cuda':
            torch.cuda.set_device(self.device)
        self.prep.rng_set_state(state)
        device_epoch_shuffle(self.prep, fallback, self.n, self.d_perm, functools.partial(self._sources, slot), self.prep_stream)
        after = self.prep.rng_get_state()
        self._unpacked = None  # the 64-bit copies of the ids: packed by now
        return after

    def start_shuffle(self, slot, state, threaded):
        """shuffle_into on a worker thread (or at once, under the single-threaded test harness): join() returns its state."""
        return _Background(functools.partial(self.shuffle_into, slot, state), threaded)

    def release(self):
        """The epoch's device buffers go back to the caching allocator NOW: the next fit() reuses them instead of allocating."""
        del self.bufs[:]
        self.d_perm = self.d_pairs = self._unpacked = None
        self.upload._out = None


class _ThreeStage(object):
    """The moving parts of run_three_stage: `consumed` is the state the reference would hold at this point (the RandomState
    itself is not touched before the way out), `pending` the shuffle running on the worker thread."""

    def __init__(self, engine, stream, job, ids, n_iter, prefetch, threaded, consumed):
        self.engine, self.stream, self.job, self.ids, self.n_iter = engine, stream, job, ids, n_iter
        self.prefetch, self.threaded, self.consumed = prefetch, threaded, consumed
        self.after_negs, self.drawn_ahead, self.pending = None, False, None

    def prepare_ahead(self, epoch_num, state):
        """Epoch `epoch_num`, shuffled up to `state`: its negatives and first chunk's sorts onto the ctx's second stream, and
        the shuffle of the epoch behind it onto the worker from the position behind those negatives."""
        engine, n_slots = self.engine, len(self.ids.bufs)
        if not self.prefetch:
            engine.rng_set_state(state)
            return
        self.job.prefetch(engine, self.stream, epoch_num, state)
        self.after_negs = engine.rng_get_state_sampled()  # behind the negatives -- or `state` itself if nothing was drawn ahead
        self.drawn_ahead = engine.get_stat('prefetch_pending') == 2
        if self.drawn_ahead and epoch_num + 1 < self.n_iter:
            self.pending = self.ids.start_shuffle((epoch_num + 1) % n_slots, self.after_negs, self.threaded)

    def epoch(self, epoch_num, verbose):
        engine = self.engine
        self.job.train(engine, self.stream, epoch_num)
        # the state the reference holds at the end of this epoch: behind its negatives
        self.consumed = self.after_negs if self.drawn_ahead else engine.rng_get_state_sampled()
        if epoch_num + 1 < self.n_iter:
            # shuffle(e + 1): prepared an epoch ago on the worker -- or now, beside the last passes of this epoch
            pending, self.pending = self.pending, None
            state = (pending.join() if pending is not None
                     else self.ids.shuffle_into((epoch_num + 1) % len(self.ids.bufs), self.consumed))
            self.prepare_ahead(epoch_num + 1, state)
        epoch_loss = mean_loss(self.job.mb_loss)
        engine.check()  # errors the training kernels can only report through the ctx
        end_epoch(epoch_num, epoch_loss, verbose)

    def close(self, random_state, check):
        """After the scopes: whatever their write-back raised, the threads are joined and the RandomState is the reference's."""
        if self.pending is not None:
            try:
                self.pending.join()
            except BaseException:  # noqa: BLE001 -- the exception already on its way out wins
                pass
        try:
            self.ids.upload.result()  # (joins the upload thread on the exceptional paths too)
            check.join()
        finally:
            random_state.set_state(self.consumed)
            # a chunk prepared ahead for an epoch that will not run (an exception left the loop): its draws are dropped and the
            # ctx's stream is put back where the reference's would be, so that the next training call on this engine -- any
            # model's -- finds no stale prefetch (slk_bilinear_train would refuse it once)
            if self.prefetch and self.engine.get_stat('prefetch_pending'):
                self.engine.rng_set_state(self.consumed)
            self.ids.release()


def run_three_stage(engine, stream, random_state, n_iter, verbose, job, ids, check, prefetch, threaded):
    """Large epochs: a three-stage pipeline over epochs, every stage consuming the one stream in the reference's order:
      train lane   the passes of epoch e (slk_bilinear_train; it draws nothing: its negatives exist already)
      prep stream  the negatives of the WHOLE epoch e + 1 and the sorts of its first chunk (slk_bilinear_prefetch), drawn
                   beside the last passes of epoch e as soon as epoch e's training call has been enqueued
      prep lane    the shuffle + id gathers of epoch e + 2 on the second slk_ctx / HIP stream (`ids`), from the stream position
                   behind epoch e + 1's negatives -- known an epoch ahead (slk_rng_get_state_sampled); on a worker thread
                   (`threaded`), because the numpy-exact shuffle reads counts back and would hold the host up
    so that in the steady state nothing but the passes is on the critical path.  Same ids, negatives and RandomState as
    the serial loop, bit-identical tables (tests/test_host_model.py, tests/test_gpu_model.py).  Before: 28.9 ms per epoch
    at 2^25 interactions, of which 3.3 ms shuffle and 2.1 ms first-chunk prep ran with no pass beside them
    (profiles/r04_m_fit_epoch_breakdown.txt).  `check`: the id-range checks (_Deferred), collected before anything is enqueued
    that indexes a table.  `prefetch=False` (test switch): the state is set and every first chunk prepared in line."""
    run = _ThreeStage(engine, stream, job, ids, n_iter, prefetch, threaded, random_state.get_state())
    try:
        if n_iter <= 0:  # nothing to train: no shuffle is drawn, the RandomState stays where it is (as in the reference)
            check.result()
            return
        state = ids.shuffle_into(0, run.consumed)  # the first epoch's shuffle: the one nothing hides
        check.result()  # raises what _check_input raised
        with contextlib.ExitStack() as stack:  # (the scopes close in reverse, each even if the other's write-back raises)
            job.open_scopes(stack, engine, stream)
            run.prepare_ahead(0, state)
            for epoch_num in range(n_iter):
                run.epoch(epoch_num, verbose)
    finally:
        run.close(random_state, check)
