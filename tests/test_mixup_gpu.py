"""MI355X: MixUp / CutMix kernels (csrc/sf_mixup.h), the packed path and the step glue.  Checks in tests/mixup_checks.py."""
import pytest
import torch

from tests import mixup_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(gpu, index):
    checks.check_golden_case(gpu, index)


@pytest.mark.parametrize("shape", checks.SHAPES)
@pytest.mark.parametrize("B", checks.BATCHES)
def test_mix_clip_shapes(gpu, B, shape):
    checks.check_mix_clip_shapes(gpu, B, shape)


def test_mix_clip_rejects(gpu):
    checks.check_mix_clip_rejects(gpu)
    with pytest.raises(checks.sa.lib.SfError):              # a host tensor never falls back to torch
        checks.mixup.mix_clip(torch.randn((2, 3, 2, 6, 10)), checks.MixParams(0.3, False, None))


@pytest.mark.parametrize("B", [2, 3])
def test_pack_mix(gpu, B):
    checks.check_pack_mix(gpu, B)


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_mix_slowfast_fast_pathway_unmixed(gpu, reverse):
    checks.check_pack_mix(gpu, 2, arch="slowfast", reverse=reverse)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B,K", [(2, 7), (3, 400), (5, 1000)])
def test_mix_targets(gpu, B, K, smoothing):
    checks.check_mix_targets(gpu, B, K, smoothing)


def test_train_step_with_mixup_graph_replay_matches_eager(gpu):
    """Four iterations of TrainStep(track_stats=True) on mvit_tiny with MIXUP.ENABLE True, numpy seeded: eager with the batch
    mixed in place == captured graph with the batch mixed straight into static_inputs() from the third iteration on, bit for
    bit (losses and final parameters); both runs check pop_stats() against tools/train_net.py:174-190."""
    le, pe, de = checks.run_mix_step(gpu, use_graph=False, steps=4)
    lg, pg, dg = checks.run_mix_step(gpu, use_graph=True, steps=4)
    assert de == dg and {p.use_cutmix for p in de} == {False, True}, de
    assert le == lg, (le, lg)
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
