"""MI355X: RandAugment kernels (csrc/sf_randaug.h) against the reference's recorded bytes and the numpy restatement, padded
buffers, determinism, launch counts, the composition with spatial sampling and the rejections.  Checks in
tests/rand_augment_checks.py."""
import pytest

from tests import rand_augment_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(gpu, index):
    checks.check_golden_case(gpu, index)


@pytest.mark.parametrize("cls,interpolation", checks.CLASS_FILTERS)
def test_padded_buffers(gpu, cls, interpolation):
    checks.check_padded(gpu, cls, interpolation)


@pytest.mark.parametrize("cls,interpolation", checks.CLASS_FILTERS)
@pytest.mark.parametrize("which", [0, 1])
def test_restatement_parity(gpu, which, cls, interpolation):
    checks.check_parity(gpu, which, cls, interpolation)


def test_determinism(gpu):
    checks.check_determinism(gpu)


def test_launch_counts(gpu):
    checks.check_launch_counts(gpu)


def test_composition_with_spatial_sampling(gpu):
    checks.check_composition(gpu)


def test_rejects(gpu):
    checks.check_rejects(gpu)
    checks.check_host_tensor_rejected()
