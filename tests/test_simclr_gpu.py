"""MI355X: the SimCLR path (csrc/sf_simclr.h, slowfast_amd/contrastive.py).  Checks in tests/simclr_checks.py."""
import pytest

from tests import simclr_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("n,C", checks.NTX_SHAPES)
def test_simclr_ntxent(gpu, n, C, pitched):
    checks.check_ntx(gpu, n, C, pitched)


def test_simclr_ntxent_returns_the_normalised_rows(gpu):
    checks.check_q_out(gpu)


def test_second_call_keeps_the_first_loss(gpu):
    checks.check_second_call_keeps_the_first(gpu)


def test_simclr_ntxent_zero_row_is_nan_everywhere(gpu):
    checks.check_zero_row(gpu)


def test_simclr_ntxent_rejections(gpu):
    checks.check_ntx_rejections(gpu)


def test_host_tensors_are_rejected(gpu):
    checks.check_rejects_host_tensors()


def test_capture_replays_match_eager(gpu):
    checks.check_capture(gpu)


def test_state_dict_contract(gpu):
    checks.check_state_dict(gpu)


def test_model_surface(gpu):
    checks.check_model_surface(gpu)


def test_tiny_model_three_iterations(gpu):
    checks.check_model(gpu)
