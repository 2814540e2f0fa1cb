"""CPU (host functional simulator): the BYOL path -- the csrc/sf_byol.h kernels per element against fp64, the predictor heads,
the ContrastiveModel with CONTRASTIVE.TYPE "byol" against the recorded reference, the BYOL_SlowR50_8x8 recipe.  Checks in
tests/byol_checks.py; the same ones run on the MI355X in tests/test_byol_gpu.py."""
import pytest

from tests import byol_checks as checks


def test_reference_stays_inside_the_bounds():
    checks.check_reference_inside_bounds()


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("n,V,C", checks.SIM_SHAPES)
def test_byol_sim(sim, n, V, C, pitched):
    checks.check_sim(sim, n, V, C, pitched)


def test_byol_sim_takes_a_list_of_keys(sim):
    checks.check_sim_list_of_keys(sim)


def test_byol_sim_zero_row_is_nan(sim):
    checks.check_sim_zero_row(sim)


def test_byol_sim_rejections(sim):
    checks.check_sim_rejections(sim)


def test_predictor_heads(sim):
    checks.check_heads(sim)


def test_state_dict_contract(sim):
    checks.check_state_dict(sim)


def test_model_surface(sim):
    checks.check_model_surface(sim)


@pytest.mark.slow       # a minute on the simulator (clips through two ResNet-18s, three times); runs on the MI355X in test_byol_gpu.py
def test_tiny_model_three_iterations(sim):
    checks.check_model(sim)


def test_bound_flat_history_matches_per_tensor(sim):
    checks.check_bound_flat_matches_per_tensor(sim)


def test_recipe_preset_builds_with_lars_and_binds(sim):
    checks.check_recipe()


def test_excluded_combinations_raise():
    checks.check_rejections()
