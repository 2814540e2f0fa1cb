"""CPU: the MAE path through the host functional simulator (csrc/sf_pixel.h, the keep / restore kernels of csrc/sf_tokens.h,
slowfast_amd/masked.py, masking.py and the (preds, labels) form of TrainStep).  Checks in tests/mae_checks.py; the same ones
run on the GPU in tests/test_mae_gpu.py."""
import pytest

from tests import mae_checks as checks


def test_masks_are_the_references():
    checks.check_masks()


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("name", sorted(checks.TOKEN_CASES))
def test_token_kernels(sim, name, cls, pitched):
    checks.check_token_kernels(sim, name, cls, pitched)


@pytest.mark.parametrize("cls", [0, 1])
def test_tables_that_keep_nothing_stay_in_bounds(sim, cls):
    checks.check_bad_tables(sim, cls)


@pytest.mark.parametrize("kind", checks.PIXEL_INPUTS)
@pytest.mark.parametrize("name", sorted(checks.PIXEL_CASES))
def test_pixel_targets(sim, name, kind):
    checks.check_pixels(sim, name, kind)


@pytest.mark.parametrize("name", sorted(checks.MODEL_CASES))
def test_oracle_reproduces_the_reference(name):
    checks.check_oracle(name)


@pytest.mark.parametrize("name", sorted(checks.MODEL_CASES))
def test_model_parity(sim, name):
    checks.check_model(sim, name)


def test_train_step_dense(sim):
    """One eager iteration of the (preds, labels) step form."""
    checks.check_captured_step(sim, use_graph=False, iterations=1)


@pytest.mark.slow
def test_train_step_dense_four_iterations(sim):
    """Host-simulator twin of test_captured_step (SF_RUN_SLOW=1)."""
    checks.check_captured_step(sim, use_graph=False, iterations=4)


def test_rejections(sim):
    checks.check_rejections(sim)
