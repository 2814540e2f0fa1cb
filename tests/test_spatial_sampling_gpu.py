"""MI355X: spatial-sampling kernels (csrc/sf_sample.h), the packed path, the rejections and the step glue.  Checks in
tests/spatial_sampling_checks.py."""
import pytest
import torch

from tests import spatial_sampling_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(gpu, index):
    checks.check_golden_case(gpu, index)


def test_window_clamp(gpu):
    checks.check_window_clamp(gpu)


@pytest.mark.parametrize("mode", [None, "const", "rand", "pixel"])
@pytest.mark.parametrize("N", [2, 3])
def test_pack_sample(gpu, N, mode):
    checks.check_pack(gpu, N, mode)


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_sample_slowfast(gpu, reverse):
    checks.check_pack(gpu, 2, "pixel", arch="slowfast", reverse=reverse)


def test_pack_without_crop_is_unchanged(gpu):
    checks.check_pack_without_crop(gpu)


def test_pack_entry_points_agree(gpu):
    checks.check_pack_entry_points_agree(gpu)


def test_rejects(gpu):
    checks.check_rejects(gpu)
    checks.check_host_tensor_rejected()


def test_train_step_with_sampling_erasing_and_mixup_graph_replay_matches_eager(gpu):
    """Four iterations of TrainStep on mvit_tiny, generators seeded, frames sampled, erased and mixed by one pack_pathways_u8
    call per iteration: eager (fresh buffers) == captured graph (straight into static_inputs() from the third iteration on),
    bit for bit in losses and final parameters."""
    le, pe, te = checks.run_sample_step(gpu, use_graph=False, steps=4)
    lg, pg, tg = checks.run_sample_step(gpu, use_graph=True, steps=4)
    assert len(te) == 4 and all((a.rows == b.rows).all() for a, b in zip(te, tg))
    assert le == lg, (le, lg)
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
