"""MI355X: HOG targets (csrc/sf_hog.h), mask tokens (csrc/sf_tokens.h), MaskMViT parity against the recorded reference and the
captured MaskFeat step.  Checks in tests/maskfeat_checks.py; reads tests/golden/maskfeat_contract.json only."""
import pytest

from tests import maskfeat_checks as checks

pytestmark = pytest.mark.gpu
HOG_NAMES = [c["name"] for c in checks.HOG_CASES]


@pytest.mark.parametrize("name", HOG_NAMES)
def test_hog_fp64_parity(gpu, name):
    checks.check_hog_case(gpu, name)


@pytest.mark.parametrize("name", HOG_NAMES)
def test_hog_recorded_reference(gpu, name):
    checks.check_hog_recorded(gpu, name)


@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("use_pos", [False, True])
def test_mask_tokens(gpu, use_pos, cls):
    checks.check_mask_tokens(gpu, use_pos, cls)


def test_multi_mse_dense_equals_gathered(gpu):
    checks.check_loss(gpu)


@pytest.mark.parametrize("name", sorted(checks.MODEL_CASES))
def test_model_parity(gpu, name):
    checks.check_model(gpu, name)


def test_captured_step(gpu):
    checks.check_captured_step(gpu, use_graph=True)


def test_rejections(gpu):
    checks.check_rejections(gpu)
    checks.check_host_tensor_rejected()
