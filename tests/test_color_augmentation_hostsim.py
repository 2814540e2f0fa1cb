"""CPU: colour augmentation of the AVA clip (csrc/sf_color.h through the host functional simulator), its draw against the
reference's, the boxes, the composition with spatial sampling, the rejections and the config glue.  Checks in
tests/color_augmentation_checks.py; the kernel ones run on the GPU in tests/test_color_augmentation_gpu.py."""
import pytest

from tests import color_augmentation_checks as checks


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(sim, index):
    checks.check_golden_case(sim, index)


@pytest.mark.parametrize("which", [0, 1])
def test_frame_means(sim, which):
    checks.check_frame_means(sim, which)


@pytest.mark.parametrize("reverse", [True, False])
@pytest.mark.parametrize("order", checks.ORDERS)
@pytest.mark.parametrize("which", [0, 1])
def test_fp64_parity(sim, which, order, reverse):
    checks.check_parity(sim, which, order, reverse)


def test_composition_with_spatial_sampling(sim):
    checks.check_composition(sim)


def test_pca_only_is_one_launch(sim):
    checks.check_pca_only_is_one_launch(sim)


def test_rejects(sim):
    checks.check_rejects(sim)


def test_config_and_constructors():
    checks.check_config()


def test_boxes():
    checks.check_boxes()
