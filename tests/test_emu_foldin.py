"""slk_bilinear_foldin on the emulator build of the engine sources.  The same checks run on the gfx950 library in
tests/test_gpu_foldin.py, there over more of the grid; here every loss, every optimizer kind, every dim, item count and user count
occurs at least once, and every (loss, kind) pair goes through the closed loop."""
import pytest

import foldin_checks as fc
from emu_backend import EmuBackend


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


def rotated(i):
    """(D, I, H) for case i: walks the dims fastest, so 20 cases see every dim five times and every I / H several times."""
    return fc.DS[i % 4], fc.ITEMS[(i // 2) % 2], fc.USERS[(i // 3) % 3]


PAIRS = [(loss, opt) for loss in fc.LOSSES for opt in fc.KINDS]


@pytest.mark.parametrize('D,n,opt', fc.WIDE)
def test_adaptive_hinge_over_many_candidates_against_the_oracle(be, D, n, opt):
    fc.check_wide_adaptive(be, D, n, opt)


@pytest.mark.parametrize('i', range(len(PAIRS)))
def test_closed_loop_against_the_oracle(be, i):
    loss, opt = PAIRS[i]
    D, I, H = rotated(i)
    fc.check_closed_loop(be, loss, opt, D, I, H)


@pytest.mark.parametrize('loss,opt', [('bpr', 'adagrad'), ('adaptive_hinge', 'adam_dense')])
def test_item_side_is_frozen(be, loss, opt):
    fc.check_frozen(be, loss, opt)


@pytest.mark.parametrize('loss,opt,D,I', [('bpr', 'adagrad', 64, 333), ('pointwise', 'sparse_adam', 6, 7),
                                          ('adaptive_hinge', 'adagrad_dense', 72, 333), ('hinge', 'sgd', 24, 7)])
def test_batch_composition_invariance(be, loss, opt, D, I):
    fc.check_batch_composition(be, loss, opt, D, I)


@pytest.mark.parametrize('loss,opt,D,I', [('bpr', 'adam_dense', 64, 333), ('pointwise', 'adagrad_dense', 24, 7),
                                          ('adaptive_hinge', 'sparse_adam', 6, 333), ('hinge', 'adagrad', 72, 7)])
def test_step_composition(be, loss, opt, D, I):
    fc.check_step_composition(be, loss, opt, D, I)


def test_step_composition_across_chained_launches(be):
    """17 steps: more than one launch holds (SLK_FOLDIN_MAX_STEPS = 16)."""
    fc.check_step_composition(be, 'bpr', 'adam_dense', 24, 333, H=3, T=17, lengths=[3, 0, 9])


def test_empty_histories(be):
    fc.check_empty(be)


def test_refusals(be):
    fc.check_refusals(be)


def test_profiled_as_user_pass(be):
    fc.check_profiled_as_user_pass(be)
