"""Checks shared by tests/test_optim_layer_decay_hostsim.py (CPU, host simulator) and tests/test_optim_layer_decay_gpu.py:
FlatOptimizer's table-driven update (any number of groups, hyper-parameters in device memory) and LARS against torch.optim and
against the trajectory the reference's own LARS recorded into tests/golden/optimizer_contract.json
(tools/make_optimizer_golden.py; slowfast/models/optimizer.py:146-237, :251-259, :262-359)."""
import base64
import importlib.util
import json
import os

import numpy as np
import torch

from slowfast_amd import optim
from slowfast_amd.data_parallel import GradReducer
from slowfast_amd.optim import CTL_SKIPPED, CTL_STEPS, FlatOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-6, 2e-7          # tests/test_optim_hostsim.py: FlatOptimizer against torch.optim


def contract():
    with open(os.path.join(ROOT, "tests", "golden", "optimizer_contract.json")) as f:
        return json.load(f)


def golden_tool():
    """tools/make_optimizer_golden.py as a module: the recorded LARS run's module, groups and gradients are defined there once."""
    spec = importlib.util.spec_from_file_location("make_optimizer_golden", os.path.join(ROOT, "tools", "make_optimizer_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- many groups -------------------------------------------------------------------------------------------------------
NGROUPS = 40


class ManyNet(torch.nn.Module):
    """40 parameters, one group each: odd sizes (segments that start off a 16-byte boundary: scalar path), multiples of four
    (vector path), several 1024-element blocks with ragged tails."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        sizes = [(37, 19), (2100,), (5, 4, 3), (16,), (1024,), (3, 7), (4, 4, 4, 4), (1,), (2052,), (33, 32)]
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(sizes[i % len(sizes)], generator=g))
                                          for i in range(NGROUPS)])


def many_groups(net, lr):
    return [{"params": [p], "weight_decay": (0.0, 1e-2, 5e-3)[i % 3], "lr": lr, "layer_decay": 0.97 ** (NGROUPS - i)}
            for i, p in enumerate(net.ps)]


def set_grads(net, ref, red, seed, scale, world, poison=None):
    g = torch.Generator().manual_seed(seed)
    red.zero_grad()
    for p, q in zip(net.parameters(), ref.parameters()):
        gr = torch.randn(p.shape, generator=g)
        q.grad = gr.clone()
        p.grad.copy_((gr * scale * world).to(p.device))  # what backward + a SUM all-reduce over `world` ranks would leave
    if poison is not None:
        poison.grad.view(-1)[1] = float("inf")


def check_many_groups(device, method):
    """40 groups with distinct layer_decay, set_lr every iteration, loss scale 128, gradients summed over 4 ranks, norm
    clipping: FlatOptimizer == torch.optim on the same groups."""
    net, ref = ManyNet(), ManyNet()
    net.to(device)
    red = GradReducer(net)
    red.world = 4
    kw = dict(loss_scale=128.0, clip_grad_l2norm=1.0)
    if method == "adamw":
        opt = FlatOptimizer(many_groups(net, 3e-3), red, method="adamw", **kw)
        topt = torch.optim.AdamW(many_groups(ref, 3e-3), betas=(0.9, 0.999), eps=1e-8)
        base = 3e-3
    else:
        opt = FlatOptimizer(many_groups(net, 0.05), red, method="sgd", momentum=0.9, nesterov=True, **kw)
        topt = torch.optim.SGD(many_groups(ref, 0.05), momentum=0.9, nesterov=True)
        base = 0.05
    assert opt.table_path and opt.hyper.shape == (NGROUPS, 4)
    worst = 0.0
    try:
        for it in range(4):
            lr = base * (0.5 ** it)
            optim.set_lr(opt, lr)
            optim.set_lr(topt, lr)
            assert len({g["lr"] for g in opt.param_groups}) == NGROUPS
            set_grads(net, ref, red, 10 + it, 128.0, 4.0)
            red.finish(loss_scale=None)
            opt.step()
            total = torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 1.0)
            assert float(total) > 1.0, "the test must actually clip"
            topt.step()
            for i, (p, q) in enumerate(zip(net.parameters(), ref.parameters())):
                d = (p.data.cpu() - q.data).abs()
                worst = max(worst, float((d / (ATOL + RTOL * q.data.abs())).max()))
        print("many groups %s: worst |diff| / (atol + rtol |ref|) = %.3f" % (method, worst))
        for i, (p, q) in enumerate(zip(net.parameters(), ref.parameters())):
            assert torch.allclose(p.data.cpu(), q.data, rtol=RTOL, atol=ATOL), (method, i)
        assert worst <= 1.0
        assert float(opt.ctl[CTL_STEPS]) == 4 and float(opt.ctl[CTL_SKIPPED]) == 0
    finally:
        red.world = 1
        red.close()


# ---- LARS against the recorded reference trajectory ---------------------------------------------------------------------
def _lars_setup(device):
    tool = golden_tool()
    rec = contract()["lars"]
    run = {k: rec[k] for k in tool.LARS_RUN}
    net = tool.LarsNet(run["param_seed"]).to(device)
    assert [k for k, _ in net.named_parameters()] == rec["names"]
    red = GradReducer(net)
    return tool, rec, run, net, red


def lars_flat_optimizer(tool, run, net, red, **kw):
    groups = [dict(g, lr=run["lr"]) for g in tool.lars_groups(net, run)]
    return FlatOptimizer(groups, red, method="sgd", momentum=run["momentum"], dampening=run["dampening"],
                         nesterov=run["nesterov"], lars=True, trust_coefficient=run["trust_coefficient"], lars_eps=run["eps"], **kw)


def check_lars_trajectory(device):
    """SGD + momentum under LARS, five steps: the parameters after every step equal what the reference's LARS(torch.optim.SGD)
    recorded.  Then the parts of LARS.step() that are easy to get wrong, each against an independent torch.optim.SGD run:
    the 1-D bias of the decayed LARS group and the weight that starts at zero step WITHOUT weight decay (and the zero weight's
    first step is unscaled), the BatchNorm group keeps its own decay."""
    tool, rec, run, net, red = _lars_setup(device)
    opt = lars_flat_optimizer(tool, run, net, red, loss_scale=16.0)
    assert opt.table_path
    names = rec["names"]
    # independent plain-SGD twins: bias with wd 0, bias WITH the group's wd (must differ), BatchNorm pair with its wd
    twin = tool.LarsNet(run["param_seed"])
    sgd = dict(lr=run["lr"], momentum=run["momentum"], dampening=run["dampening"], nesterov=run["nesterov"])
    bias_nodecay = torch.optim.SGD([twin.fc.bias], weight_decay=0.0, **sgd)
    bn_decay = torch.optim.SGD(list(twin.bn.parameters()), weight_decay=run["bn_weight_decay"], **sgd)
    twin2 = tool.LarsNet(run["param_seed"])
    bias_decay = torch.optim.SGD([twin2.fc.bias], weight_decay=run["weight_decay"], **sgd)
    worst = 0.0
    try:
        for it in range(run["steps"]):
            grads = tool.lars_grads(net, run, it)
            assert abs(float(sum(g.double().sum() for g in grads)) - rec["grad_sums"][it]) < 1e-9, "gradients differ from the recorded run"
            red.zero_grad()
            for p, g in zip(net.parameters(), grads):
                p.grad.copy_((g * 16.0).to(device))
            for m in (twin, twin2):
                for p, g in zip(m.parameters(), grads):
                    p.grad = g.clone()
            red.finish(loss_scale=None)
            opt.step()
            bias_nodecay.step(); bn_decay.step(); bias_decay.step()
            want = torch.from_numpy(np.frombuffer(base64.b64decode(rec["params_after_step"][it]), dtype="<f4").copy())
            have = torch.cat([p.detach().reshape(-1).cpu() for p in net.parameters()])
            assert have.shape == want.shape
            worst = max(worst, float(((have - want).abs() / (ATOL + RTOL * want.abs())).max()))
            print("lars step %d: max |diff| %.3e, worst |diff| / (atol + rtol |ref|) %.3f"
                  % (it, float((have - want).abs().max()), worst))
            assert torch.allclose(have, want, rtol=RTOL, atol=ATOL), it
            mine = dict(zip(names, [p.detach().cpu() for p in net.parameters()]))
            assert torch.allclose(mine["fc.bias"], twin.fc.bias.data, rtol=RTOL, atol=ATOL)          # no decay, no scaling
            assert float((mine["fc.bias"] - twin2.fc.bias.data).abs().max()) > 1e-4                # ... and decay would show
            assert torch.allclose(mine["bn.weight"], twin.bn.weight.data, rtol=RTOL, atol=ATOL)      # BatchNorm: its own decay
            assert torch.allclose(mine["bn.bias"], twin.bn.bias.data, rtol=RTOL, atol=ATOL)
            if it == 0:
                # zero weight norm: neither decay nor trust ratio -- exactly the plain first SGD step -lr * g
                g_dead = grads[names.index("dead.weight")]
                assert torch.allclose(mine["dead.weight"], -run["lr"] * g_dead, rtol=RTOL, atol=ATOL)
                assert float(opt.trust_ratio(net.dead.weight)) == 0.0
                assert float(opt.trust_ratio(net.conv.weight)) > 0.0 and float(opt.trust_ratio(net.fc.bias)) == 0.0
            else:
                assert float(opt.trust_ratio(net.dead.weight)) > 0.0     # it left zero: adapted like any other weight
    finally:
        red.close()


def check_lars_overflow(device, method="sgd"):
    """A non-finite gradient: parameters, moments and the trust buffer keep their content, CTL_SKIPPED counts."""
    tool, rec, run, net, red = _lars_setup(device)
    if method == "sgd":
        opt = lars_flat_optimizer(tool, run, net, red, loss_scale=16.0, dynamic_loss_scale=True)
    else:
        groups = [dict(g, lr=1e-3) for g in tool.lars_groups(net, run)]
        opt = FlatOptimizer(groups, red, method="adamw", lars=True, loss_scale=16.0, dynamic_loss_scale=True)
    ref = tool.LarsNet(run["param_seed"])
    try:
        set_grads(net, ref, red, 1, 16.0, 1.0)
        red.finish(loss_scale=None)
        opt.step()
        assert float(opt.ctl[CTL_STEPS]) == 1 and float(opt.trust.abs().sum()) > 0
        keep = [t.detach().clone() for t in (opt.flat_param, opt.m1, opt.trust) + ((opt.m2,) if opt.m2 is not None else ())]
        set_grads(net, ref, red, 2, 16.0, 1.0, poison=net.conv.weight)
        red.finish(loss_scale=None)
        opt.step()
        now = (opt.flat_param, opt.m1, opt.trust) + ((opt.m2,) if opt.m2 is not None else ())
        for a, b in zip(keep, now):
            assert torch.equal(a, b)
        assert float(opt.ctl[CTL_SKIPPED]) == 1 and float(opt.ctl[CTL_STEPS]) == 1 and float(opt.found_inf) == 1.0
        assert float(opt.loss_scale) == 8.0
    finally:
        red.close()


# ---- construct_optimizer against the recorded groups --------------------------------------------------------------------
def constructed(case, device, extra, **kw):
    from tests import model_checks as mc
    gold = mc.load_golden(case)
    cfg = mc.cfg_for(gold, extra=extra)
    model, sd, inputs, labels, *_ = mc.oracle_run(gold, cfg)
    model.load_state_dict(sd)
    model = model.to(device).train()
    red = GradReducer(model, **({"bucket_mb": 0.05} if kw.pop("small_buckets", False) else {}))
    opt = optim.construct_optimizer(model, cfg, red, **kw)
    return model, cfg, red, opt, inputs, labels


def check_group_contract(case, device, extra, keys):
    rec = contract()["groups"][case]
    assert rec["opts"] == list(extra)
    model, cfg, red, opt, *_ = constructed(case, device, extra)
    try:
        name_of = {id(p): k for k, p in model.named_parameters()}
        mine = [dict({k: g[k] for k in keys}, params=[name_of[id(p)] for p in g["params"]]) for g in opt.param_groups]
        assert len(mine) == len(rec["groups"])
        for a, b in zip(mine, rec["groups"]):
            assert a == b, (a, b)
        assert all(g["lr"] == cfg.SOLVER.BASE_LR == rec["base_lr"] for g in opt.param_groups)
        return opt
    finally:
        red.close()


# ---- TrainStep: graph replay == eager with a learning rate that changes every iteration ---------------------------------
def run_train_step(case, device, extra, use_graph, steps=6, poison_step=3):
    """TrainStep + construct_optimizer(extra) on a golden-case model; set_lr with a new value before every step, one step
    with non-finite inputs (skipped, loss scale halved).  Returns (parameters, ctl, losses, optimizer facts)."""
    import torch.nn.functional as F
    from slowfast_amd.step import TrainStep
    model, cfg, red, opt, inputs, labels = constructed(case, device, extra, small_buckets=True, loss_scale=64.0,
                                                       dynamic_loss_scale=True)
    red.attach_torch_param_hooks(model.head.parameters())
    step = TrainStep(model, red, opt, F.cross_entropy, use_graph=use_graph, warmup=1)
    xs, ys = [x.to(device) for x in inputs], labels.to(device)
    losses = []
    try:
        for i in range(steps):
            optim.set_lr(opt, 0.01 * (0.8 ** i))
            batch = [x * float("inf") for x in xs] if i == poison_step else xs
            losses.append(float(step(batch, ys)))
        facts = dict(table=opt.table_path, lars=opt.lars, groups=len(opt.param_groups), graph=step._graph is not None,
                     lrs=opt.hyper[:, 0].detach().cpu().clone())
        return ([p.detach().float().cpu().clone() for p in model.parameters()], opt.ctl.detach().cpu().clone(), losses, facts)
    finally:
        red.close()


def check_graph_replay_equals_eager(case, device, extra, expect_lars):
    pe, ce, le, fe = run_train_step(case, device, extra, use_graph=False)
    pg, cg, lg, fg = run_train_step(case, device, extra, use_graph=True)
    assert fe["table"] and fg["table"] and fg["graph"] and not fe["graph"] and fe["lars"] == fg["lars"] == expect_lars
    assert torch.equal(fe["lrs"], fg["lrs"]) and float(fe["lrs"].max()) <= 0.01 * 0.8 ** 5 * (1 + 1e-6)     # the LAST set_lr arrived
    assert torch.equal(ce, cg), (ce, cg)
    assert float(ce[CTL_SKIPPED]) == 1 and float(ce[CTL_STEPS]) == 5
    assert len(le) == len(lg) and [a for a in le if a == a] == [a for a in lg if a == a], (le, lg)
    assert sum(1 for a in le if a == a) >= 5
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
    return fe
