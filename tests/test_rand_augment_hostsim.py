"""CPU: RandAugment of the decoded uint8 frames (csrc/sf_randaug.h through the host functional simulator), its draw against the
reference's, the numpy restatement against the reference's bytes, padded buffers, launch counts, the composition with spatial
sampling, the rejections and the config glue.  Checks in tests/rand_augment_checks.py; the kernel ones run on the GPU in
tests/test_rand_augment_gpu.py."""
import pytest

from tests import rand_augment_checks as checks

TRANSFORM_CASES = [i for i, c in enumerate(checks.CASES) if c["kind"] == "transform"]


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(sim, index):
    checks.check_golden_case(sim, index)


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_restatement_reproduces_the_fixture(index):
    checks.check_restatement_golden(index)


@pytest.mark.parametrize("index", TRANSFORM_CASES)
def test_draw(index):
    checks.check_draw(index)


def test_fixture_covers_every_op_and_variant():
    checks.check_fixture_covers()


def test_restatement_against_pil():
    checks.check_restatement_against_pil()


@pytest.mark.parametrize("cls,interpolation", checks.CLASS_FILTERS)
def test_padded_buffers(sim, cls, interpolation):
    checks.check_padded(sim, cls, interpolation)


@pytest.mark.parametrize("cls,interpolation", checks.CLASS_FILTERS)
@pytest.mark.parametrize("which", [0, 1])
def test_restatement_parity(sim, which, cls, interpolation):
    checks.check_parity(sim, which, cls, interpolation)


def test_determinism(sim):
    checks.check_determinism(sim)


def test_launch_counts(sim):
    checks.check_launch_counts(sim)


def test_composition_with_spatial_sampling(sim):
    checks.check_composition(sim)


def test_rejects(sim):
    checks.check_rejects(sim)


def test_config_and_constructors():
    checks.check_config()
