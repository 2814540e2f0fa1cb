"""CPU: MixUp / CutMix (csrc/sf_mixup.h through the host functional simulator), the loss table and the soft-label statistics
of TrainStep.  Checks in tests/mixup_checks.py; the same ones run on the GPU in tests/test_mixup_gpu.py."""
import pytest

from tests import mixup_checks as checks


@pytest.mark.parametrize("index", range(checks.NUM_GOLDEN_CASES))
def test_golden_contract(sim, index):
    checks.check_golden_case(sim, index)


@pytest.mark.parametrize("shape", checks.SHAPES)
@pytest.mark.parametrize("B", checks.BATCHES)
def test_mix_clip_shapes(sim, B, shape):
    checks.check_mix_clip_shapes(sim, B, shape)


def test_mix_clip_rejects(sim):
    checks.check_mix_clip_rejects(sim)


@pytest.mark.parametrize("B", [2, 3])
def test_pack_mix(sim, B):
    checks.check_pack_mix(sim, B)


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_mix_slowfast_fast_pathway_unmixed(sim, reverse):
    checks.check_pack_mix(sim, 2, arch="slowfast", reverse=reverse)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B,K", [(2, 7), (3, 400), (5, 1000)])
def test_mix_targets(sim, B, K, smoothing):
    checks.check_mix_targets(sim, B, K, smoothing)


def test_losses():
    checks.check_losses()


def test_config_and_construct_mixup():
    checks.check_config()


def test_train_step_with_mixup_eager(sim):
    """mvit_tiny, MIXUP.ENABLE True, eager: soft cross entropy on the mixed batch, top-1 / top-5 error from the two largest soft
    labels (tools/train_net.py:174-190)."""
    losses, params, draws = checks.run_mix_step(sim, use_graph=False, steps=2)
    assert all(l == l for l in losses) and len(draws) == 2 and all(p.lam != 1.0 for p in draws)
