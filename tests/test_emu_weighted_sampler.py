"""slk_cdf_guide / slk_sample_items_weighted on the emulator build of the engine sources, against RandomState.choice.  The same
checks run on the gfx950 library in tests/test_gpu_weighted_sampler.py."""
import pytest

import weighted_sampler_checks as wc
from emu_backend import EmuBackend


@pytest.fixture(scope='module')
def be():
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('kind', wc.WEIGHTS)
@pytest.mark.parametrize('num_items', wc.NUM_ITEMS)
def test_ids_state_and_guide_equal_numpy_choice(be, num_items, kind):
    wc.check_bit_exact(be, num_items, kind)


def test_automatic_guide_bits(be):
    wc.check_auto_guide_bits(be)


def test_uniform_and_weighted_draws_interleave_on_one_ctx(be):
    wc.check_interleaving(be)


def test_one_item_still_consumes_two_words_per_value(be):
    wc.check_one_item_consumes_two_words(be)


def test_count_zero_leaves_the_state_untouched(be):
    wc.check_count_zero(be)


def test_a_large_count_splits_into_consecutive_draws(be):
    wc.check_split_draws(be)


def test_refusals(be):
    wc.check_refusals(be)


def test_profiled_as_sample(be):
    wc.check_profiled_as_sample(be)


def test_state_sampled_behind_a_weighted_draw(be):
    wc.check_state_sampled(be)
