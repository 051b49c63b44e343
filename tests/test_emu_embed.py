"""The embedding front-end (slk_embedding_forward / _backward_plan / _backward_fill, csrc/slk_embed.hip) entry by entry on the
emulator build, against exact integer sums: tests/embed_checks.py.  The same checks run on the gfx950 library in
tests/test_gpu_embed.py, which adds the cases that need the device's grid cap; the torch-side callers are
tests/test_host_encoders.py.  Every case of the list runs here, the table of 2^20 rows included."""
import pytest

import embed_checks as ec


@pytest.fixture(scope='module')
def be():
    from emu_backend import EmuBackend
    b = EmuBackend()
    yield b
    b.close()


@pytest.mark.parametrize('D', ec.DIMS)
@pytest.mark.parametrize('n', ec.ONE_ROW_NS)
def test_one_row_owns_every_lookup(be, n, D):
    ec.check_one_row(be, n, D)


@pytest.mark.parametrize('D', ec.DIMS)
@pytest.mark.parametrize('n', ec.ALL_PADDING_NS)
def test_every_lookup_is_padding(be, n, D):
    ec.check_all_padding(be, n, D)


@pytest.mark.parametrize('D', ec.DIMS)
@pytest.mark.parametrize('rows,padding_idx', ec.UNIFORM_TABLES)
@pytest.mark.parametrize('c', ec.UNIFORM_COUNTS)
def test_every_row_has_exactly_c_lookups(be, c, rows, padding_idx, D):
    ec.check_uniform(be, c, rows, padding_idx, D)


@pytest.mark.parametrize('D', ec.SHIPPED_DIMS)
@pytest.mark.parametrize('name', sorted(ec.NAMED))
def test_run_layouts_across_chunk_edges_and_levels(be, name, D):
    ec.check_named(be, name, D)


@pytest.mark.parametrize('D', ec.KEY_WIDTH_DIMS)
@pytest.mark.parametrize('rows,padding_idx', ec.KEY_WIDTH_TABLES)
def test_row_counts_around_key_width_edges(be, rows, padding_idx, D):
    ec.check_key_width(be, rows, padding_idx, D)


@pytest.mark.parametrize('D', ec.DIMS)
def test_one_row_table(be, D):
    ec.check_one_row_table(be, D)


@pytest.mark.parametrize('rows', ec.BLOOM_ROWS)
@pytest.mark.parametrize('D', ec.BLOOM_DIMS)
@pytest.mark.parametrize('n_hash', ec.BLOOM_HASHES)
def test_bloom_layer(be, n_hash, D, rows):
    ec.check_bloom(be, n_hash, D, rows)


@pytest.mark.parametrize('D', ec.REUSE_DIMS)
def test_a_small_call_after_a_large_one_reuses_the_scratch_buffers(be, D):
    ec.check_buffer_reuse(be, D)


def test_plan_and_fill_state_machine(be):
    ec.check_state_machine(be)


def test_float_gradients_within_the_summation_bound_of_each_element(be):
    ec.check_float(be)
