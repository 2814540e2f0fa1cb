"""CPU: spatial sampling (csrc/sf_sample.h through the host functional simulator), its draw against the reference's, the packed
path, the rejections and the step glue.  Checks in tests/spatial_sampling_checks.py; the same ones run on the GPU in
tests/test_spatial_sampling_gpu.py."""
import pytest

from tests import spatial_sampling_checks as checks


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(sim, index):
    checks.check_golden_case(sim, index)


def test_window_clamp(sim):
    checks.check_window_clamp(sim)


@pytest.mark.parametrize("mode", [None, "const", "rand", "pixel"])
@pytest.mark.parametrize("N", [2, 3])
def test_pack_sample(sim, N, mode):
    checks.check_pack(sim, N, mode)


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_sample_slowfast(sim, reverse):
    checks.check_pack(sim, 2, "pixel", arch="slowfast", reverse=reverse)


def test_pack_without_crop_is_unchanged(sim):
    checks.check_pack_without_crop(sim)


def test_pack_entry_points_agree(sim):
    checks.check_pack_entry_points_agree(sim)


def test_rejects(sim):
    checks.check_rejects(sim)


def test_config_and_construct_spatial_sampling():
    checks.check_config()


def test_train_step_with_sampling_erasing_and_mixup_eager(sim):
    """mvit_tiny, frames sampled, erased and mixed by pack_pathways_u8, eager: finite losses."""
    losses, params, tables = checks.run_sample_step(sim, use_graph=False, steps=2)
    assert all(l == l and abs(l) != float("inf") for l in losses)
    assert len(tables) == 2 and all(len(t.rows) == 2 for t in tables)
