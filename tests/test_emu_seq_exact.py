"""The PoolNet sequence pass (spotlight_amd/csrc/slk_seq.hip and the SEQ item pass of slk_kernels.h, unmodified) run by the fiber
emulator against the float64 restatement of tests/seq_exact_checks.py, per timestep, under both forms of the pass.  The same
checks run on the gfx950 library in tests/test_gpu_seq_exact.py."""
import os

import pytest

import seq_exact_checks as sx
from emu_backend import EmuBackend

EMU_CUS = int(os.environ.get('SLK_EMU_CUS') or 2)  # tests/emu/emu_runtime.cpp: the compute units the emulated device reports


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('loss,n_neg', sx.SCAN_LOSSES)
@pytest.mark.parametrize('D,L', sx.SCAN_SHAPES)
def test_scan_shapes(be, D, L, loss, n_neg):
    sx.check_isolating(be, D, L, loss, n_neg, B=3)


@pytest.mark.parametrize('loss,n_neg', [(l, 5) for l in sx.LOSSES] + [('adaptive_hinge', 1), ('adaptive_hinge', 4)])
def test_losses_one_term_per_row(be, loss, n_neg):
    sx.check_isolating(be, 64, 17, loss, n_neg)


@pytest.mark.parametrize('n_neg', sx.WIDE_NS)
def test_adaptive_hinge_over_many_candidates(be, n_neg):
    sx.check_wide_adaptive(be, n_neg)


@pytest.mark.parametrize('loss', sx.LOSSES)
def test_losses_long_runs(be, loss):
    sx.check_shared(be, loss, 5, L=17)


@pytest.mark.parametrize('loss', ['bpr', 'pointwise'])
def test_long_runs_of_4096_timesteps(be, loss):
    sx.check_shared(be, loss)


@pytest.mark.parametrize('loss,n_neg', sx.SCAN_LOSSES)
@pytest.mark.parametrize('n_hash', [0, 2])
@pytest.mark.parametrize('D,L', sx.PAD_SHAPES)
def test_padding_and_zeros(be, D, L, n_hash, loss, n_neg):
    sx.check_padding(be, D, L, loss, n_neg, n_hash)


def test_adaptive_tie_goes_to_the_candidate_drawn_first(be):
    sx.check_tie(be)


@pytest.mark.parametrize('loss,n_neg', sx.SCAN_LOSSES)
def test_grid_stride(be, loss, n_neg):
    sx.check_grid_stride(be, EMU_CUS, loss, n_neg)


def test_minibatch_with_no_real_entry(be):
    sx.check_no_real_entry(be)


@pytest.mark.parametrize('n_hash', [0, 2])
@pytest.mark.parametrize('D,L', sx.PAD_SHAPES)
def test_prediction_on_padding_and_zeros(be, D, L, n_hash):
    sx.check_prediction(be, D, L, n_hash)
