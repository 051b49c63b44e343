"""slk_verify_negatives on the emulator build of the engine sources, against the numpy restatement
(spotlight_amd.sampling.verify_negatives).  The same checks run on the gfx950 library in tests/test_gpu_verify_negatives.py."""
import pytest

import verify_negatives_checks as vc
from emu_backend import EmuBackend


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('bm', vc.BATCHES)
def test_ids_and_counters_equal_the_restatement(be, bm):
    vc.check_kernel_equals_restatement(be, bm)


def test_dense_case_every_attempt_and_both_counters(be):
    vc.check_dense_case(be)


def test_empty_call_and_batch_size_beyond_n(be):
    vc.check_empty_call_and_batch_beyond_n(be)


def test_refusals_leave_the_ctx_usable(be):
    vc.check_refusals(be)


@pytest.mark.parametrize('weighted', [False, True], ids=['uniform', 'weighted'])
def test_draw_then_verify_leaves_numpys_state(be, weighted):
    vc.check_draw_then_verify_leaves_numpys_state(be, weighted)


def test_profiled_as_sample(be):
    vc.check_profiled_as_sample(be)
