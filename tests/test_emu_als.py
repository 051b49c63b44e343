"""slk_als_gram / slk_als_solve / slk_als_loss on the emulator build of the engine sources.  The same checks run on the gfx950
library in tests/test_gpu_als.py, there over the full grid; here every dim, every table size and every history length occurs
at least once (every Problem holds all the lengths)."""
import pytest

import als_checks as ac
from emu_backend import EmuBackend


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


# (dim, rows of the fixed table): the dims walk the table sizes
SHAPES = [(6, 2000), (24, 333), (64, 7), (72, 333), (128, 7)]


@pytest.mark.parametrize('D,n', SHAPES + [(24, 7), (64, 333)])
def test_gram(be, D, n):
    ac.check_gram(be, D, n)


def test_gram_of_no_rows(be):
    ac.check_gram_empty(be)


@pytest.mark.parametrize('D,I', SHAPES)
def test_half_step_against_float64(be, D, I):
    ac.check_half_step(be, D, I)


@pytest.mark.parametrize('D,I', [(24, 333), (72, 7)])
def test_composition_invariance(be, D, I):
    ac.check_composition(be, D, I)


def test_failed_rows_are_counted_and_left_untouched(be):
    ac.check_failure(be)


def test_objective(be):
    ac.check_loss(be)


def test_refusals(be):
    ac.check_refusals(be)


def test_profile_classes(be):
    ac.check_profile_classes(be)
