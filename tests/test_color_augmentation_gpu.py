"""MI355X: colour-augmentation kernels (csrc/sf_color.h), the composition with spatial sampling and the rejections.  Checks in
tests/color_augmentation_checks.py."""
import pytest

from tests import color_augmentation_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(gpu, index):
    checks.check_golden_case(gpu, index)


@pytest.mark.parametrize("which", [0, 1])
def test_frame_means(gpu, which):
    checks.check_frame_means(gpu, which)


@pytest.mark.parametrize("reverse", [True, False])
@pytest.mark.parametrize("order", checks.ORDERS)
@pytest.mark.parametrize("which", [0, 1])
def test_fp64_parity(gpu, which, order, reverse):
    checks.check_parity(gpu, which, order, reverse)


def test_composition_with_spatial_sampling(gpu):
    checks.check_composition(gpu)


def test_pca_only_is_one_launch(gpu):
    checks.check_pca_only_is_one_launch(gpu)


def test_rejects(gpu):
    checks.check_rejects(gpu)
    checks.check_host_tensor_rejected()
