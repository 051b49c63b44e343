"""The multi-negative losses at wide n, exact scores, pair by pair (tests/wide_negatives_checks.py) on the emulator build.  The
same checks run on the gfx950 library in tests/test_gpu_wide_negatives.py."""
import pytest

import wide_negatives_checks as wn


@pytest.fixture(scope='module')
def be():
    from emu_backend import EmuBackend
    b = EmuBackend()
    yield b
    b.close()


SOFTMAX_CASES = wn.SOFTMAX_CASES
COLUMN_CASES = wn.COLUMN_CASES


def test_the_softmax_grid_takes_every_lane_group_width():
    wn.check_grid_covers_the_kernel()


@pytest.mark.parametrize('n,B,D,regime', SOFTMAX_CASES)
def test_softmax_gradients_pair_by_pair(be, n, B, D, regime):
    wn.check_softmax(be, n, B, D, regime)


@pytest.mark.parametrize('route', wn.ROUTES)
@pytest.mark.parametrize('n,B,D', COLUMN_CASES)
@pytest.mark.parametrize('loss', wn.COLUMN_LOSSES)
def test_column_selection_pair_by_pair(be, loss, n, B, D, route):
    wn.check_column(be, loss, n, B, D, route)
