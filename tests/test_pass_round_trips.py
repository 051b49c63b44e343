"""The item pass's issue-then-consume gather (k_item_pass step (2b), every MODE, NPRE 1 and 4), its ballot head compaction, and
the pipelined user pass that feeds it inside a ping-pong scope (k_user_pass<..., PP>) against code they do not share a line
with: the C oracle, the persistent route (slk_epoch.hip) and plain training outside the scope.  The shapes are the small ones at
which the passes take their other paths: runs that cross a tile end by less than a row group's G lanes, by exactly G and by
more (I = 40 items under B = 512: runs of ~25 occurrences, tiles of 64 / 256 positions), the usual runs of 1-3 (I = 2000), a
short last minibatch behind a full one in the same chunk, a run that ends exactly at a tile end, dims that are no multiple
of 4; users that recur 10-30 times, users that all occur once, users hot enough for the long-run form.

The same tests run on the fiber emulator here and on the gfx950 library (`-m gpu`)."""
import os

import numpy as np
import pytest

import engine_checks as ec

# two full minibatches and a short last one (300 positions: its last tile holds fewer than T) in ONE chunk
B, N = 512, 2 * 512 + 300
LAUNCH = dict(epoch_kernel=0)  # the two passes, not the persistent kernel that takes minibatches of this size by default
NPRE = {4: 2048, 1: 0}         # item_lat_max_tiles: launches of this few tiles take the every-head-early form by default


@pytest.fixture(scope='module', params=['emu', pytest.param('gpu', marks=pytest.mark.gpu)])
def be(request):
    if request.param == 'emu':
        from emu_backend import EmuBackend
        b = EmuBackend()
    else:
        from hip_backend import HipBackend
        b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('npre', [4, 1])
@pytest.mark.parametrize('I', [40, 2000])
@pytest.mark.parametrize('D', [64, 16, 6])
@pytest.mark.parametrize('loss,opt', [('bpr', 'adagrad'), ('hinge', 'sparse_adam'), ('hinge', 'adagrad'), ('bpr', 'sparse_adam')])
def test_spilling_runs_equal_the_persistent_route(be, loss, opt, D, I, npre):
    # one-table SNAP (no ping-pong scope): every table and state tensor bit for bit
    n0 = be.engine.get_stat('item_long_launches')
    with be.engine.options(item_lat_max_tiles=NPRE[npre]):
        ec.check_epoch_kernel_is_bit_identical(be, loss, opt, D, U=300, I=I, N=N, B=B, epochs=1)
    assert be.engine.get_stat('item_long_launches') == n0  # (no run covers a tile: the LONG = false form, whose owner walks the spill)


@pytest.mark.parametrize('D,I', [(64, 40), (16, 40), (6, 40), (64, 2000), (6, 2000)])
@pytest.mark.parametrize('loss,opt', [('bpr', 'adagrad'), ('hinge', 'sparse_adam')])
def test_spilling_runs_match_oracle(be, loss, opt, D, I):
    with be.engine.options(**LAUNCH):
        ec.check_train_matches_oracle(be, loss, opt, D, U=300, I=I, N=N, B=B, nn=1, epochs=1)


def _seed_with_a_run_ending_at_a_tile_end(T, U=50, I=40, B=512):
    """check_single_step_gradients draws users, items, negatives from RandomState(seed) in that order; the minibatch's item-sorted
    occurrence list is the positives and the negatives together.  The first seed for which some run ends exactly where a tile of
    T positions ends (the next key differs by construction) and some other run crosses a tile end."""
    for seed in range(100, 400):
        rs = np.random.RandomState(seed)
        rs.randint(0, U, B)
        items = rs.randint(0, I, B)
        negs = rs.randint(0, I, B)
        ends = np.cumsum(np.bincount(np.concatenate([items, negs]), minlength=I))[:-1]
        ends = ends[np.r_[True, ends[1:] != ends[:-1]]]
        n_tiles = 2 * B // T
        if (ends % T == 0).any() and np.setdiff1d(np.arange(1, n_tiles) * T, ends).size:
            return seed
    raise AssertionError('no such seed')


@pytest.mark.parametrize('loss', ['bpr', 'hinge'])
@pytest.mark.parametrize('D', [64, 16])
def test_run_that_ends_exactly_at_a_tile_end(be, loss, D):
    T = 4 * 256 // (D // 4)
    seed = _seed_with_a_run_ending_at_a_tile_end(T)
    with be.engine.options(**LAUNCH):
        ec.check_single_step_gradients(be, loss, D, U=50, I=40, B=512, nn=1, seed=seed)


@pytest.mark.parametrize('npre', [4, 1])
@pytest.mark.parametrize('D,I', [(64, 40), (16, 40), (6, 40), (64, 2000), (16, 2000)])
@pytest.mark.parametrize('loss,opt', [('bpr', 'adagrad'), ('hinge', 'sparse_adam')])
def test_pingpong_forms_equal_plain_training(be, loss, opt, D, I, npre):
    # the bandwidth-bound (pipelined) user pass and SNAPPP item pass forced at this size; the plain side is the persistent kernel
    opts = dict(user_lat_max_batch=0, item_lat_max_tiles=NPRE[npre])
    ec.check_user_pingpong_is_bit_neutral(be, loss, opt, D, U=300, I=I, N=N, B=B, options=opts)


@pytest.mark.parametrize('D,I', [(64, 700), (16, 700), (6, 2000), (64, 40)])
@pytest.mark.parametrize('loss', ['bpr', 'hinge'])
def test_pingpong_single_occurrence_holes_among_the_gathers(be, loss, D, I):
    # SNAPPPS: positions whose item occurs once are skipped by the item pass -- holes among a group's four gathers (I = 700:
    # singles and runs mix; I = 40: no single at all)
    opts = dict(user_lat_max_batch=0, item_single_min_items=1)
    n0 = be.engine.get_stat('single_minibatches')
    ec.check_user_pingpong_is_bit_neutral(be, loss, 'adagrad', D, U=300, I=I, N=N, B=B, seed=61, options=opts)
    assert be.engine.get_stat('single_minibatches') > n0  # (the path did run)


@pytest.mark.parametrize('npre', [4, 1])
@pytest.mark.parametrize('D', [64, 6])
@pytest.mark.parametrize('opt', ['adagrad', 'sparse_adam'])
def test_adaptive_hinge_dead_occurrences(be, opt, D, npre):
    # n = 5: four of an interaction's six occurrences are dead (dL/dscore == 0), their rows are not fetched
    with be.engine.options(item_lat_max_tiles=NPRE[npre]):
        ec.check_epoch_kernel_is_bit_identical(be, 'adaptive_hinge', opt, D, U=300, I=40, N=N, B=B, epochs=1, nn=5)
        ec.check_epoch_kernel_is_bit_identical(be, 'adaptive_hinge', opt, D, U=300, I=2000, N=N, B=B, epochs=1, nn=5)
    # (the oracle under Adagrad only: Adam's normalised step turns the summation-order noise of a 75-term row sum into an error of
    # the step's own size in single elements -- the fixed 2e-5 of the check is a statement about the order, not the kernel; under
    # SparseAdam the bit-for-bit comparison above is the whole statement)
    if opt == 'adagrad':
        with be.engine.options(**LAUNCH):
            ec.check_train_matches_oracle(be, 'adaptive_hinge', opt, D, U=300, I=40, N=B + 100, B=B, nn=5, epochs=1)


@pytest.mark.parametrize('npre', [4, 1])
def test_poolnet_item_pass(be, npre):
    # SLK_ITEM_SEQ: the own item's record half is taken as it is, a sampled item's is scaled.  (PoolNet's launches count a tile
    # four times against item_lat_max_tiles -- slk_launch_item_pass, lat_div -- and a minibatch here is at most 32 x 9 x 2
    # occurrences = 3 to 10 tiles: 2048 still selects the every-head-early form, 0 the default one.  There is no counter for the
    # route; both settings must give what the oracle gives.)
    with be.engine.options(item_lat_max_tiles=NPRE[npre]):
        ec.check_seq_train_matches_oracle(be, 'bpr', 'adagrad', 16, I=31, N=70, L=9, B=32, nn=1, epochs=1)
        ec.check_seq_train_matches_oracle(be, 'hinge', 'sparse_adam', 6, I=300, N=70, L=9, B=32, nn=1, epochs=1)


@pytest.mark.parametrize('npre', [4, 1])
def test_user_bloom_rows_item_pass(be, npre):
    # SLK_ITEM_ROW: the hashed user rows' gradients are summed by the item pass from [vec | bias grad] records
    with be.engine.options(item_lat_max_tiles=NPRE[npre], **LAUNCH):
        ec.check_bloom_train_matches_oracle(be, 'bpr', 'adagrad', 16, user_bloom=2, item_bloom=0, U=300, I=40, N=B + 100, B=B, nn=1,
                                            epochs=1)
        ec.check_bloom_train_matches_oracle(be, 'hinge', 'adagrad', 6, user_bloom=2, item_bloom=4, U=300, I=200, N=B + 100, B=B, nn=1,
                                            epochs=1)


@pytest.mark.parametrize('kind,D,n', [('adagrad', 64, 5), ('sparse_adam', 24, 3), ('adagrad', 6, 5)])
def test_sampled_softmax_item_pass(be, kind, D, n):
    # SLK_ITEM_SNAPALL: every one of the 1 + n occurrences is live, the rows are fetched without looking at dL/dscore.  40 items
    # under minibatches of 64 x (1 + n) occurrences: runs of ~10 that cross the ends of the 64- / 128- / 256-position tiles.
    # Reference: softmax_checks' float64 restatement, closed loop, with its own bounds
    import softmax_checks as sm
    sm.check_closed_loop(be, kind, D, n, 40)


def test_sharded_exchange_item_pass(be):
    """SLK_ITEM_BLK (slk_shard.hip): the row-sharded path at world 1 -- its item pass sums [row | scalar] exchange slots -- against
    the fused path on the same tables, ids and RNG state, every element within bench_parity's 1e-5 of the table's norm (the two
    paths associate a row's sum differently).  40 items under minibatches of 512: spilling runs, two minibatches."""
    import torch
    import torch.distributed as dist
    import bench_parity as bp
    dev = torch.device('cuda', 0) if type(be).__name__ == 'HipBackend' else torch.device('cpu')
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29467')
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        for D, I in ((64, 40), (16, 40), (64, 2000)):
            bp.sharded_world1_vs_fused(be.engine, dev, be.stream, 3000, I, D, B, n_mb=2, seed=7, block_rows=1024)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('U', [30, 10 ** 5, 5])
@pytest.mark.parametrize('loss,opt', [('bpr', 'adagrad'), ('hinge', 'sparse_adam'), ('pointwise', 'adagrad')])
def test_pipelined_user_pass_equals_plain_training(be, loss, opt, U):
    # U = 30: runs of 10-30 positions per user, below a covered SLK_USER_TILE; U = 10^5: every user once (the first
    # run-end test ends the run); U = 5: runs of ~100 positions, which wholly cover aligned tiles -- the long-run form and its stitch
    n0 = be.engine.get_stat('user_long_launches')
    for D in (64, 6):
        ec.check_user_pingpong_is_bit_neutral(be, loss, opt, D, U=U, I=2000, N=N, B=B, seed=71, options=dict(user_lat_max_batch=0))
    assert (be.engine.get_stat('user_long_launches') > n0) == (U == 5)


@pytest.mark.parametrize('U', [30, 10 ** 5])
def test_pipelined_user_pass_with_user_biases_zero_and_hinted(be, U):
    """Inside a ping-pong scope, user biases identically zero: with SLK_TABLES_USER_BIAS_ZERO the pipelined pass skips them; every
    table, state tensor and loss equals the unhinted run's bit for bit (the same kernel on both sides: the same loss sums)."""
    from spotlight_amd import _native
    eng = be.engine
    D, I = 16, 2000
    rs = np.random.RandomState(83)
    users, items = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
    params = [rs.normal(0, 0.1, (U, D)), rs.normal(0, 0.1, (I, D)), np.zeros(U), rs.normal(0, 0.1, I)]
    state = np.random.RandomState(84).get_state()
    n_mb = (N + B - 1) // B
    results = []
    with eng.options(user_lat_max_batch=0):
        for hinted in (False, True):
            dev = be.model(params, opt='adagrad', lr=0.05)
            if hinted:
                dev.tables.flags = _native.TABLES_USER_BIAS_ZERO
            eng.rng_set_state(state)
            d_users, d_items = be.alloc(users), be.alloc(items)
            mb_loss = be.alloc(np.zeros(2 * n_mb, dtype=np.float32))
            with eng.user_pingpong(dev.tables, dev.optim, stream=be.stream):
                for rep in range(2):
                    eng.bilinear_train(dev.tables, dev.optim, be.ptr(d_users), be.ptr(d_items), N, B, 'bpr', 1,
                                       be.ptr(mb_loss) + 4 * rep * n_mb, stream=be.stream)
            results.append([be.get(mb_loss)] + [be.get(x) for x in dev.p + dev.s1 + dev.s2])
    for k, (a, b) in enumerate(zip(*results)):
        assert np.array_equal(a, b), 'tensor %d differs with the user-bias hint' % k
    assert not results[1][3].any() and not np.array_equal(results[1][1], params[0].astype(np.float32))


@pytest.mark.parametrize('U', [30, 10 ** 5])
def test_regression_loss_user_biases_live(be, U):
    # explicit feedback: the user pass in its dL/dscore-forming mode, the item pass one-table SNAP with one occurrence per interaction
    for opt in ('adagrad', 'sparse_adam'):
        ec.check_epoch_kernel_is_bit_identical(be, 'regression', opt, 16, U=U, I=40, N=N, B=B, epochs=1)
    with be.engine.options(**LAUNCH):
        ec.check_explicit_train_matches_oracle(be, 'regression', 'adagrad', 16, U=min(U, 300), I=40, N=N, B=B, epochs=1)
