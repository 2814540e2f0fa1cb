"""CPU (host functional simulator): the SimCLR path -- the csrc/sf_simclr.h kernels per element against fp64, the
ContrastiveModel with CONTRASTIVE.TYPE "simclr" against the recorded reference, the SimCLR_SlowR50_8x8 recipe.  Checks in
tests/simclr_checks.py; the same ones run on the MI355X in tests/test_simclr_gpu.py."""
import pytest

from tests import simclr_checks as checks


def test_reference_stays_inside_the_bounds():
    checks.check_reference_inside_bounds()


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("n,C", checks.NTX_SHAPES)
def test_simclr_ntxent(sim, n, C, pitched):
    checks.check_ntx(sim, n, C, pitched)


def test_simclr_ntxent_returns_the_normalised_rows(sim):
    checks.check_q_out(sim)


def test_second_call_keeps_the_first_loss(sim):
    checks.check_second_call_keeps_the_first(sim)


def test_simclr_ntxent_zero_row_is_nan_everywhere(sim):
    checks.check_zero_row(sim)


def test_simclr_ntxent_rejections(sim):
    checks.check_ntx_rejections(sim)


def test_state_dict_contract(sim):
    checks.check_state_dict(sim)


def test_model_surface(sim):
    checks.check_model_surface(sim)


@pytest.mark.slow       # a minute on the simulator (five pairs of clips through a ResNet-18); runs on the MI355X in test_simclr_gpu.py
def test_tiny_model_three_iterations(sim):
    checks.check_model(sim)


def test_recipe_preset_builds_with_lars_and_binds(sim):
    checks.check_recipe()


def test_excluded_combinations_raise():
    checks.check_rejections()
