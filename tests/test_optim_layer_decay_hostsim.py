"""CPU (host simulator): SOLVER.LAYER_DECAY < 1 and SOLVER.LARS_ON on FlatOptimizer's table-driven update path
(csrc/sf_optim.h: sf_flat_sgd_tab / sf_flat_adamw_tab / sf_flat_lars_trust) against torch.optim and against what the reference's
own optimizer.py recorded into tests/golden/optimizer_contract.json (tools/make_optimizer_golden.py)."""
import pytest
import torch

from slowfast_amd import optim
from slowfast_amd.data_parallel import GradReducer
from slowfast_amd.optim import FlatOptimizer
from tests import optim_layer_decay_checks as checks

LAYER_DECAY_OPTS = ["SOLVER.LAYER_DECAY", 0.75]


@pytest.mark.parametrize("method", ["adamw", "sgd"])
def test_many_groups_match_torch(sim, method):
    checks.check_many_groups(sim, method)


@pytest.mark.parametrize("case", ["vit_tiny", "mvit_tiny", "mvit_nocls_sepqkv_tiny"])
def test_layer_decay_group_contract(sim, case):
    """construct_optimizer(LAYER_DECAY 0.75) == the reference's get_param_groups: names, order, weight decay, layer decay."""
    opt = checks.check_group_contract(case, sim, LAYER_DECAY_OPTS, ("weight_decay", "layer_decay"))
    assert len({g["layer_decay"] for g in opt.param_groups}) > 1


def test_set_lr_applies_layer_decay(sim):
    opt = checks.check_group_contract("mvit_tiny", sim, LAYER_DECAY_OPTS, ("weight_decay", "layer_decay"))
    for x in (0.3, 0.0125):
        optim.set_lr(opt, x)
        assert all(g["lr"] == x * g["layer_decay"] for g in opt.param_groups)
    assert opt.table_path and opt.sync_hyper() is True and opt.sync_hyper() is False      # uploaded once per change
    assert torch.equal(opt.hyper[:, 0], torch.tensor([g["lr"] for g in opt.param_groups], dtype=torch.float32))
    # the keys travel through the checkpoint surface
    sd = opt.state_dict()
    assert [g["layer_decay"] for g in sd["param_groups"]] == [g["layer_decay"] for g in opt.param_groups]
    assert all("apply_LARS" in g for g in sd["param_groups"])
    for g in opt.param_groups:
        g["layer_decay"] = -1.0
    opt.load_state_dict(sd)
    assert [g["layer_decay"] for g in sd["param_groups"]] == [g["layer_decay"] for g in opt.param_groups]


def test_lars_matches_reference_trajectory(sim):
    checks.check_lars_trajectory(sim)


def test_lars_on_group_contract(sim):
    opt = checks.check_group_contract("slow_tiny", sim, ["SOLVER.LARS_ON", True], ("weight_decay", "layer_decay", "apply_LARS"))
    assert opt.lars and opt.table_path and opt.trust_coefficient == 0.001
    assert opt.hyper[:, 2].tolist() == [float(g["apply_LARS"]) for g in opt.param_groups]


@pytest.mark.parametrize("method", ["sgd", "adamw"])
def test_overflow_leaves_everything_untouched(sim, method):
    checks.check_lars_overflow(sim, method)


def test_adam_still_raises(sim):
    with pytest.raises(NotImplementedError):
        checks.constructed("mvit_tiny", sim, ["SOLVER.OPTIMIZING_METHOD", "adam"])


def test_small_group_counts_keep_the_argument_path(sim, monkeypatch):
    """8 groups or fewer without LARS: sf_flat_sgd / sf_flat_adamw run as before, no table exists."""
    from slowfast_amd import lib
    native = lib.get_lib()
    called = []
    real = native.call
    monkeypatch.setattr(native, "call", lambda name, *a, **k: (called.append(name), real(name, *a, **k))[1])
    for method, entry in (("sgd", "sf_flat_sgd"), ("adamw", "sf_flat_adamw")):
        net = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(50 + i)) for i in range(8)])
        red = GradReducer(net)
        opt = FlatOptimizer([{"params": [p], "lr": 0.1, "weight_decay": 1e-3} for p in net], red, method=method, momentum=0.9)
        assert not opt.table_path and opt.hyper is None
        del called[:]
        for p in net:
            p.grad.normal_()
        red.finish(loss_scale=None)
        opt.step()
        assert called == ["sf_flat_blocks", "sf_flat_sumsq", "sf_step_control", entry], called
        red.close()
        # the ninth group moves it to the table
        net = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(50 + i)) for i in range(9)])
        red = GradReducer(net)
        opt = FlatOptimizer([{"params": [p], "lr": 0.1} for p in net], red, method=method, momentum=0.9)
        del called[:]
        red.finish(loss_scale=None)
        opt.step()
        assert called[-1] == entry + "_tab" and entry not in called
        red.close()
