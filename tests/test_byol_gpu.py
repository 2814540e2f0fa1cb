"""MI355X: the BYOL path (csrc/sf_byol.h, slowfast_amd/contrastive.py, slowfast_amd/heads.py).  Checks in tests/byol_checks.py."""
import pytest

from tests import byol_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("n,V,C", checks.SIM_SHAPES)
def test_byol_sim(gpu, n, V, C, pitched):
    checks.check_sim(gpu, n, V, C, pitched)


def test_byol_sim_takes_a_list_of_keys(gpu):
    checks.check_sim_list_of_keys(gpu)


def test_byol_sim_zero_row_is_nan(gpu):
    checks.check_sim_zero_row(gpu)


def test_byol_sim_rejections(gpu):
    checks.check_sim_rejections(gpu)


def test_host_tensors_are_rejected(gpu):
    checks.check_rejects_host_tensors()


def test_capture_replays_match_eager(gpu):
    checks.check_capture(gpu)


def test_predictor_heads(gpu):
    checks.check_heads(gpu)


def test_state_dict_contract(gpu):
    checks.check_state_dict(gpu)


def test_model_surface(gpu):
    checks.check_model_surface(gpu)


def test_tiny_model_three_iterations(gpu):
    checks.check_model(gpu)


def test_bound_flat_history_matches_per_tensor(gpu):
    checks.check_bound_flat_matches_per_tensor(gpu)
