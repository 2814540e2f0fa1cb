"""CPU: the SSL colour augmentation of the decoded uint8 frames (csrc/sf_sslcolor.h through the host functional simulator), its
draw, the numpy restatement against PIL's recorded bytes and against PIL itself (both HSV conversions over all 2^24 triples, the
blur over a sweep of sigma), padded buffers, launch counts, the composition with RandAugment and the packing, the rejections and
the config glue.  Checks in tests/ssl_color_checks.py; the kernel ones run on the GPU in tests/test_ssl_color_gpu.py."""
import pytest

from tests import ssl_color_checks as checks


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(sim, index):
    checks.check_golden_case(sim, index)


def test_fixture_is_there_and_covers_both_branches():
    assert checks.NUM_GOLDEN_CASES >= 4
    checks.check_fixture_covers()


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_restatement_reproduces_the_fixture(index):
    checks.check_restatement_golden(index)


@pytest.mark.parametrize("which", range(len(checks.DRAW_CASES)))
def test_draw_order(which):
    checks.check_draw(which)


@pytest.mark.parametrize("name", checks.TABLE_NAMES)
def test_restatement_parity(sim, name):
    checks.check_parity(sim, name)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_restatement_parity_many_chunks(sim, which):
    checks.check_parity_big(sim, which)


@pytest.mark.parametrize("which", [0, 1])
def test_in_place_many_chunks(sim, which):
    checks.check_in_place_big(sim, which)


@pytest.mark.parametrize("direction", ["rgb_to_hsv", "hsv_to_rgb"])
def test_hsv_restatement_against_pil_exhaustive(direction):
    checks.check_hsv_exhaustive(direction)


def test_blur_restatement_against_pil():
    checks.check_blur_against_pil()


def test_hue_subset(sim):
    checks.check_hue_subset(sim)


def test_padding_out_and_in_place(sim):
    checks.check_out_and_in_place(sim)


def test_determinism(sim):
    checks.check_determinism(sim)


def test_launch_counts(sim):
    checks.check_launch_counts(sim)


def test_composition_with_rand_augment_and_packing(sim):
    checks.check_composition(sim)


def test_rejects(sim):
    checks.check_rejects(sim)


def test_byte_round_trip():
    checks.check_byte_round_trip()


def test_config_and_constructors():
    checks.check_config()
