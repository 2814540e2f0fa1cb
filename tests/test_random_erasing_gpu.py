"""MI355X: random-erasing kernels (csrc/sf_erase.h), the packed path and the step glue.  Checks in
tests/random_erasing_checks.py."""
import pytest
import torch

from tests import random_erasing_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(gpu, index):
    checks.check_golden_case(gpu, index)


def test_pixel_noise_matches_restatement(gpu):
    checks.check_pixel_noise(gpu)


@pytest.mark.parametrize("mode", ["rand", "pixel"])
def test_overlap_later_row_wins(gpu, mode):
    checks.check_overlap(gpu, mode)


def test_noise_quality(gpu):
    checks.check_noise_quality(gpu)


def test_out_and_empty_plan(gpu):
    checks.check_out_and_empty(gpu)


@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
@pytest.mark.parametrize("N", [2, 3])
def test_pack_erase(gpu, N, mode):
    checks.check_pack(gpu, N, mode)


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_erase_slowfast(gpu, reverse):
    checks.check_pack(gpu, 2, "pixel", arch="slowfast", reverse=reverse)


def test_rejects(gpu):
    checks.check_rejects(gpu)
    state = checks.random.getstate()
    with pytest.raises(checks.sa.lib.SfError):              # a host tensor never falls back to torch
        checks.sa.RandomErasing(probability=1.0, mode="pixel")(torch.randn((2, 3, 2, 6, 10)))
    assert checks.random.getstate() == state
    with pytest.raises(checks.sa.lib.SfError):
        checks.re_.erase_clip(torch.randn((2, 3, 2, 6, 10)), checks.re_.make_table([(0, 0, 2, 0, 0, 2, 2)], "const", (2, 3, 6, 10)))


def test_train_step_with_erasing_and_mixup_graph_replay_matches_eager(gpu):
    """Four iterations of TrainStep on mvit_tiny with MIXUP.ENABLE and AUG.RE_PROB 1.0, generators seeded: eager with the batch
    erased and mixed in place == captured graph with the batch erased, then mixed straight into static_inputs() from the third
    iteration on, bit for bit (losses and final parameters)."""
    le, pe, te = checks.run_erase_mix_step(gpu, use_graph=False, steps=4)
    lg, pg, tg = checks.run_erase_mix_step(gpu, use_graph=True, steps=4)
    assert len(te) == 4 and all(len(t.rows) > 0 for t in te)
    assert all((a.rows == b.rows).all() and (a.keys == b.keys).all() for a, b in zip(te, tg))
    assert le == lg, (le, lg)
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
