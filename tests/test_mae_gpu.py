"""MI355X: pixel targets (csrc/sf_pixel.h), the keep / restore kernels (csrc/sf_tokens.h), MaskMViT's MAE path against the
recorded reference and the captured MAE step.  Checks in tests/mae_checks.py; reads tests/golden/mae_contract.json only."""
import pytest

from tests import mae_checks as checks

pytestmark = pytest.mark.gpu


def test_masks_are_the_references():
    checks.check_masks()


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("name", sorted(checks.TOKEN_CASES))
def test_token_kernels(gpu, name, cls, pitched):
    checks.check_token_kernels(gpu, name, cls, pitched)


@pytest.mark.parametrize("cls", [0, 1])
def test_tables_that_keep_nothing_stay_in_bounds(gpu, cls):
    checks.check_bad_tables(gpu, cls)


@pytest.mark.parametrize("kind", checks.PIXEL_INPUTS)
@pytest.mark.parametrize("name", sorted(checks.PIXEL_CASES))
def test_pixel_targets(gpu, name, kind):
    checks.check_pixels(gpu, name, kind)


@pytest.mark.parametrize("name", sorted(checks.MODEL_CASES))
def test_model_parity(gpu, name):
    checks.check_model(gpu, name)


def test_captured_step(gpu):
    checks.check_captured_step(gpu, use_graph=True)


def test_rejections(gpu):
    checks.check_rejections(gpu)
    checks.check_host_tensor_rejected()
