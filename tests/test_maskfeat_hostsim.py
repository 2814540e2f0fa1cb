"""CPU: the MaskFeat path through the host functional simulator (csrc/sf_hog.h, the mask-token kernels of csrc/sf_tokens.h,
slowfast_amd/masked.py, masking.py, the multi_mse loss and the (preds, labels) form of TrainStep).  Checks in
tests/maskfeat_checks.py; the same ones run on the GPU in tests/test_maskfeat_gpu.py."""
import pytest

from tests import maskfeat_checks as checks

HOG_NAMES = [c["name"] for c in checks.HOG_CASES]


def test_masks_are_the_references():
    checks.check_masks()


@pytest.mark.parametrize("name", HOG_NAMES)
def test_hog_fp64_parity(sim, name):
    checks.check_hog_case(sim, name)


@pytest.mark.parametrize("name", HOG_NAMES)
def test_hog_recorded_reference(sim, name):
    checks.check_hog_recorded(sim, name)


@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("use_pos", [False, True])
def test_mask_tokens(sim, use_pos, cls):
    checks.check_mask_tokens(sim, use_pos, cls)


def test_multi_mse_dense_equals_gathered(sim):
    checks.check_loss(sim)


@pytest.mark.parametrize("name", sorted(checks.MODEL_CASES))
def test_oracle_reproduces_the_reference(name):
    checks.check_oracle(name)


@pytest.mark.parametrize("name", sorted(checks.MODEL_CASES))
def test_model_parity(sim, name):
    checks.check_model(sim, name)


def test_train_step_dense(sim):
    """One eager iteration of the (preds, labels) step form (the simulator needs ~25 s per iteration of the two models)."""
    checks.check_captured_step(sim, use_graph=False, iterations=1)


@pytest.mark.slow
def test_train_step_dense_four_iterations(sim):
    """Host-simulator twin of test_captured_step (minutes on the CPU: SF_RUN_SLOW=1)."""
    checks.check_captured_step(sim, use_graph=False, iterations=4)


def test_rejections(sim):
    checks.check_rejections(sim)
