"""The optimizer step (csrc/slk_optim.h) against torch.optim in float64, off the default hyper-parameters, on the emulator build:
tests/optim_checks.py.  The same checks run on the gfx950 library in tests/test_gpu_optim.py."""
import pytest

import engine_checks as ec
import optim_checks as oc


@pytest.fixture(scope='module')
def be():
    from emu_backend import EmuBackend
    b = EmuBackend()
    yield b
    b.close()


# ---- the bound itself (no engine) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', oc.WHICH)
@pytest.mark.parametrize('kind', oc.KINDS)
def test_bound_holds_for_an_fp32_restatement_at_slack_one(kind, which):
    oc.check_bound_holds_for_fp32_restatement(kind, which)


@pytest.mark.parametrize('kind', [k for k in oc.KINDS if k != 'sgd'])
def test_bound_sees_a_default_in_place_of_a_set_hyper_parameter(kind):
    oc.check_bound_is_tight_enough(kind)


# ---- A: one step per route, every kind, both hyper-parameter sets, every step0 ---------------------------------------------------------
@pytest.mark.parametrize('name,D', oc.ROUTES)
def test_readout_is_the_gradient_the_fused_kinds_apply(be, name, D):
    oc.check_readout_is_the_gradient(be, oc.route(name, D))


@pytest.mark.parametrize('name,D,kind', oc.ROUTE_KINDS)
def test_one_step_matches_torch_float64(be, name, D, kind):
    for which in oc.WHICH:
        for step0 in oc.STEP0S:
            oc.check_rule_against_torch(be, oc.route(name, D), kind, which, step0)


# ---- B: several steps, and the routes against each other off the defaults --------------------------------------------------------------
@pytest.mark.parametrize('which,step0', [('off', 999), ('default', 0)])
@pytest.mark.parametrize('kind', oc.KINDS)
def test_closed_loop_matches_torch_and_one_call_equals_four(be, kind, which, step0):
    oc.check_closed_loop_against_torch(be, kind, which, step0=step0)


@pytest.mark.parametrize('kind', oc.KINDS)
def test_epoch_kernel_is_bit_identical_off_the_defaults(be, kind):
    oc.check_routes_agree_off_the_defaults(be, 'epoch', kind)


@pytest.mark.parametrize('kind', oc.KINDS)
def test_chunking_is_bit_neutral_off_the_defaults(be, kind):
    oc.check_routes_agree_off_the_defaults(be, 'chunking', kind)


@pytest.mark.parametrize('kind', oc.SPARSE_KINDS)
def test_user_pingpong_is_bit_neutral_off_the_defaults(be, kind):
    oc.check_routes_agree_off_the_defaults(be, 'pingpong', kind)


@pytest.mark.parametrize('kind', oc.KINDS)
def test_foldin_steps_compose_off_the_defaults(be, kind):
    oc.check_foldin_steps_compose_off_the_defaults(be, kind)
