"""GPU: the table-driven FlatOptimizer update and LARS on the device (csrc/sf_optim.h: sf_flat_sgd_tab / sf_flat_adamw_tab /
sf_flat_lars_trust) with the bounds of tests/test_optim_layer_decay_hostsim.py, and TrainStep graph replay == eager, bit for bit,
while set_lr changes every group's learning rate before every step."""
import pytest

from tests import optim_layer_decay_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", ["adamw", "sgd"])
def test_many_groups_match_torch_gpu(gpu, method):
    checks.check_many_groups(gpu, method)


def test_lars_matches_reference_trajectory_gpu(gpu):
    checks.check_lars_trajectory(gpu)


@pytest.mark.parametrize("method", ["sgd", "adamw"])
def test_overflow_leaves_everything_untouched_gpu(gpu, method):
    checks.check_lars_overflow(gpu, method)


def test_layer_decay_graph_replay_matches_eager(gpu):
    """mvit_tiny at SOLVER.LAYER_DECAY 0.75 (12 groups: the table path): the learning-rate schedule survives graph replay."""
    facts = checks.check_graph_replay_equals_eager("mvit_tiny", gpu, ["SOLVER.LAYER_DECAY", 0.75], expect_lars=False)
    assert facts["groups"] == 12 and len(set(facts["lrs"].tolist())) > 1


def test_lars_graph_replay_matches_eager(gpu):
    checks.check_graph_replay_equals_eager("slow_tiny", gpu, ["SOLVER.LARS_ON", True], expect_lars=True)
