"""The multi-negative losses at wide n, exact scores, pair by pair (tests/wide_negatives_checks.py) on the real gfx950 library:
the whole grid, n up to the cap of 1024, B in {1, 37, 300}.  tests/test_emu_wide_negatives.py runs the same checks on the
emulator build."""
import pytest

import wide_negatives_checks as wn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from hip_backend import HipBackend
    b = HipBackend()
    yield b
    b.close()


@pytest.mark.parametrize('n,B,D,regime', wn.SOFTMAX_CASES)
def test_softmax_gradients_pair_by_pair(be, n, B, D, regime):
    wn.check_softmax(be, n, B, D, regime)


@pytest.mark.parametrize('route', wn.ROUTES)
@pytest.mark.parametrize('n,B,D', wn.COLUMN_CASES)
@pytest.mark.parametrize('loss', wn.COLUMN_LOSSES)
def test_column_selection_pair_by_pair(be, loss, n, B, D, route):
    wn.check_column(be, loss, n, B, D, route)
