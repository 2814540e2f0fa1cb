"""Records tests/golden/optimizer_contract.json from the UNMODIFIED reference (slowfast/models/optimizer.py), imported through
oracle.refshim like tests/test_reference_integration.py does.  Build container only (needs the reference tree).

    python tools/make_optimizer_golden.py

(a) "groups": what the reference's construct_optimizer makes of the reference's own models --
      vit_tiny / mvit_tiny / mvit_nocls_sepqkv_tiny (cfgs of tests/golden/<case>.json) at SOLVER.LAYER_DECAY 0.75:
      per group, in order, the parameter names, weight_decay and layer_decay;
      slow_tiny with SOLVER.LARS_ON True: the same plus apply_LARS.
(b) "lars": five steps of the reference's LARS(torch.optim.SGD(...), trust_coefficient=0.001, clip=False) on a small seeded
    module with seeded gradients: the parameter values after every step (float32, little endian, base64, in named_parameters
    order), and "f64_dev": the largest |difference| between that trajectory and a float64 run of the same steps -- the
    yardstick for a consumer whose norms are not accumulated in float32.
Recorded results only: no reference program text goes into the fixture or this tool.
"""
import base64
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "optimizer_contract.json")
LAYER_DECAY_CASES = ("vit_tiny", "mvit_tiny", "mvit_nocls_sepqkv_tiny")
LARS_CASE = "slow_tiny"
LAYER_DECAY = 0.75

# (b): hyper-parameters of the recorded LARS run (the test rebuilds module and gradients from them)
LARS_RUN = {"steps": 5, "param_seed": 7, "grad_seed": 100, "lr": 0.1, "momentum": 0.9, "dampening": 0.0, "nesterov": False,
            "weight_decay": 1e-2, "bn_weight_decay": 5e-3, "trust_coefficient": 0.001, "eps": 1e-8}


class LarsNet(torch.nn.Module):
    """conv: 4-D, 1080 elements (one full 1024-element block and a ragged tail); fc: 2-D + bias; bn: a BatchNorm pair for the
    group LARS leaves alone; dead: a 2-D weight that starts at zero (no trust ratio on its first step)."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv = torch.nn.Conv3d(10, 12, (1, 3, 3), bias=False)
        self.fc = torch.nn.Linear(12, 8)
        self.bn = torch.nn.BatchNorm3d(12)
        self.dead = torch.nn.Linear(8, 6, bias=False)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.1)
            self.fc.weight.copy_(torch.randn(self.fc.weight.shape, generator=g) * 0.3)
            self.fc.bias.copy_(torch.randn(self.fc.bias.shape, generator=g))
            self.bn.weight.copy_(1.0 + 0.1 * torch.randn(self.bn.weight.shape, generator=g))
            self.bn.bias.copy_(0.1 * torch.randn(self.bn.bias.shape, generator=g))
            self.dead.weight.zero_()


def lars_groups(net, run):
    """BatchNorm apart (apply_LARS False, its own decay); everything else -- the bias included -- in ONE decayed LARS group."""
    bn = list(net.bn.parameters())
    rest = [p for p in net.parameters() if all(p is not q for q in bn)]
    return [{"params": bn, "weight_decay": run["bn_weight_decay"], "layer_decay": 1.0, "apply_LARS": False},
            {"params": rest, "weight_decay": run["weight_decay"], "layer_decay": 1.0, "apply_LARS": True}]


def lars_grads(net, run, step):
    g = torch.Generator().manual_seed(run["grad_seed"] + step)
    return [torch.randn(p.shape, generator=g) for p in net.parameters()]


def _lars_trajectory(run, dtype):
    from slowfast.models.optimizer import LARS
    net = LarsNet(run["param_seed"]).to(dtype)
    opt = LARS(torch.optim.SGD(lars_groups(net, run), lr=run["lr"], momentum=run["momentum"], dampening=run["dampening"],
                               nesterov=run["nesterov"]), trust_coefficient=run["trust_coefficient"], clip=False, eps=run["eps"])
    traj, sums = [], []
    for it in range(run["steps"]):
        grads = lars_grads(net, run, it)
        sums.append(float(sum(g.double().sum() for g in grads)))
        for p, g in zip(net.parameters(), grads):
            p.grad = g.to(dtype).clone()                    # LARS.step() rescales p.grad in place
        opt.step()
        traj.append(torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone())
    return net, traj, sums


def record_lars():
    net, t32, sums = _lars_trajectory(LARS_RUN, torch.float32)
    _, t64, _ = _lars_trajectory(LARS_RUN, torch.float64)
    dev = max(float((a.double() - b).abs().max()) for a, b in zip(t32, t64))
    return dict(LARS_RUN, names=[k for k, _ in net.named_parameters()], shapes=[list(p.shape) for p in net.parameters()],
                grad_sums=sums, f64_dev=dev,
                params_after_step=[base64.b64encode(t.numpy().astype("<f4").tobytes()).decode("ascii") for t in t32])


def record_groups(case, extra, keys):
    with open(os.path.join(ROOT, "tests", "golden", case + ".json")) as f:
        gold = json.load(f)
    cfg = refshim.reference_cfg(gold["reference_yaml"], list(gold["opts"]) + list(extra))
    torch.manual_seed(0)
    model = refshim.reference_model(cfg)
    from slowfast.models.optimizer import construct_optimizer
    opt = construct_optimizer(model, cfg)
    name_of = {id(p): k for k, p in model.named_parameters()}
    return {"opts": list(extra), "method": cfg.SOLVER.OPTIMIZING_METHOD, "base_lr": cfg.SOLVER.BASE_LR,
            "groups": [dict({k: g[k] for k in keys}, params=[name_of[id(p)] for p in g["params"]]) for g in opt.param_groups]}


def main():
    assert refshim.available(), "the reference tree is not present"
    refshim.install()
    rec = {"torch_version": torch.__version__, "groups": {}}
    for case in LAYER_DECAY_CASES:
        rec["groups"][case] = record_groups(case, ["SOLVER.LAYER_DECAY", LAYER_DECAY], ("weight_decay", "layer_decay"))
    rec["groups"][LARS_CASE] = record_groups(LARS_CASE, ["SOLVER.LARS_ON", True], ("weight_decay", "layer_decay", "apply_LARS"))
    rec["lars"] = record_lars()
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes;", {k: len(v["groups"]) for k, v in rec["groups"].items()},
          "f64_dev %.3e" % rec["lars"]["f64_dev"])


if __name__ == "__main__":
    main()
