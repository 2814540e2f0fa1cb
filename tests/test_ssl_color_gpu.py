"""MI355X: the SSL colour-augmentation kernels (csrc/sf_sslcolor.h) against PIL's recorded bytes and the numpy restatement,
the HSV round trip on 2^16 colours x five shifts, padded buffers, in-place calls, determinism, launch counts, the composition
with RandAugment and the packing, and the rejections.  Checks in tests/ssl_color_checks.py."""
import pytest

from tests import ssl_color_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(gpu, index):
    checks.check_golden_case(gpu, index)


@pytest.mark.parametrize("name", checks.TABLE_NAMES)
def test_restatement_parity(gpu, name):
    checks.check_parity(gpu, name)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_restatement_parity_many_chunks(gpu, which):
    checks.check_parity_big(gpu, which)


@pytest.mark.parametrize("which", [0, 1])
def test_in_place_many_chunks(gpu, which):
    checks.check_in_place_big(gpu, which)


def test_hue_subset(gpu):
    checks.check_hue_subset(gpu)


def test_padding_out_and_in_place(gpu):
    checks.check_out_and_in_place(gpu)


def test_determinism(gpu):
    checks.check_determinism(gpu)


def test_launch_counts(gpu):
    checks.check_launch_counts(gpu)


def test_composition_with_rand_augment_and_packing(gpu):
    checks.check_composition(gpu)


def test_rejects(gpu):
    checks.check_rejects(gpu)
    checks.check_host_tensor_rejected()
