"""CPU: random erasing (csrc/sf_erase.h through the host functional simulator), its draw against the reference's, the packed
path and the step glue.  Checks in tests/random_erasing_checks.py; the same ones run on the GPU in
tests/test_random_erasing_gpu.py."""
import pytest

from tests import random_erasing_checks as checks


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(sim, index):
    checks.check_golden_case(sim, index)


def test_pixel_noise_matches_restatement(sim):
    checks.check_pixel_noise(sim)


@pytest.mark.parametrize("mode", ["rand", "pixel"])
def test_overlap_later_row_wins(sim, mode):
    checks.check_overlap(sim, mode)


def test_noise_quality(sim):
    checks.check_noise_quality(sim)


def test_out_and_empty_plan(sim):
    checks.check_out_and_empty(sim)


@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
@pytest.mark.parametrize("N", [2, 3])
def test_pack_erase(sim, N, mode):
    checks.check_pack(sim, N, mode)


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_erase_slowfast(sim, reverse):
    checks.check_pack(sim, 2, "pixel", arch="slowfast", reverse=reverse)


def test_rejects(sim):
    checks.check_rejects(sim)


def test_config_and_construct_random_erasing():
    checks.check_config()


def test_train_step_with_erasing_and_mixup_eager(sim):
    """mvit_tiny, MIXUP.ENABLE and AUG.RE_PROB 1.0, eager: finite losses, and every iteration erased something."""
    losses, params, tables = checks.run_erase_mix_step(sim, use_graph=False, steps=2)
    assert all(l == l and abs(l) != float("inf") for l in losses)
    assert len(tables) == 2 and all(len(t.rows) > 0 for t in tables)
