"""Record tests/golden/simclr_contract.json from the UNMODIFIED reference (build container only).

Results only; every input is a seed tests/simclr_checks.py draws again.  Recorded:
  ntx      per loss case of the grid of simclr_checks (n x C x T x input scale x kind): the reference's own fp32 run -- its
           ContrastiveModel.forward, unbound on a holder whose backbone is the identity and whose l2_norm is the reference's
           Normalize, so that the lines of the simclr branch (contrastive.py:692-754) themselves run on the case's (a, b),
           autograd for da and db -- as a loss, a seeded sample of da and db, and its deviation from the fp64 restatement in
           units of the tests' bounds (loss, da, db).  Asserted <= 1: the condition the bounds have to meet.
  model    a tiny reference ContrastiveModel (slow_tiny + the SimCLR keys of simclr_checks.MODEL_OPTS) driven for two iterations
           of the reference's contrastive_forward with CONTRASTIVE.SEQUENTIAL and one of the non-sequential form, 3 crops of
           batch 4: state-dict keys (in the reference's order) and shapes, per iteration the loss, the gradient norm,
           perform_backward, the shape of the dummy logits and num_batches_tracked of every BatchNorm layer.

The reference is loaded through oracle/refshim.install().  ``slowfast.utils.distributed`` (the process-group helpers, not used
with one device) is pre-seeded with a stand-in, and ``.cuda()`` is the identity in this process: the reference runs on the CPU.

    python tools/make_simclr_golden.py
"""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tests import simclr_checks as sc  # noqa: E402
from tools.make_moco_golden import load_reference  # noqa: E402


def record_ntx(rc):
    out, worst = {}, [0.0, 0.0, 0.0]
    for n, C in sc.NTX_SHAPES:
        for T, scale, kind in sc.ntx_cases(n, C):
            r = sc.ntx_reference(n, C, T, scale, kind)
            a, b = r["a"].clone().requires_grad_(True), r["b"].clone().requires_grad_(True)
            cfg = types.SimpleNamespace(NUM_GPUS=1, CONTRASTIVE=types.SimpleNamespace(SIMCLR_DIST_ON=True))
            holder = types.SimpleNamespace(type="simclr", training=True, T=T, k=3, cfg=cfg, momentum_annealing=False,
                                           backbone=lambda clip: clip[0], l2_norm=rc.Normalize(), knn_mem_update=lambda q, i: None)
            logits, loss = rc.ContrastiveModel.forward(holder, [[a], [b]], index=torch.arange(n))
            assert tuple(logits.shape) == (n, 4)
            loss.backward()
            again = sc.reference_sequence(r["a"], r["b"], T)
            assert torch.equal(again, loss.detach()), "simclr_checks.reference_sequence drifted"
            ratios = sc.ntx_ratios(r, loss, a.grad, b.grad)
            assert max(ratios) <= 1.0, (n, C, T, scale, kind, ratios)
            worst = [max(w, x) for w, x in zip(worst, ratios)]
            idx = sc.sample_index(n * C, 1, sc.GRAD_SAMPLE)
            out.setdefault(sc.shape_key(n, C), []).append(sc.pack_record(float(loss.detach()), sc.f32_list(a.grad.flatten()[idx]),
                                                                         sc.f32_list(b.grad.flatten()[idx]), ratios))
        print("ntx n=%d C=%d: reference vs fp64 so far: loss %.3f da %.3f db %.3f of the bounds" % ((n, C) + tuple(worst)))
    return out, worst


def record_model(rc):
    cfg = refshim.reference_cfg(sc.mc.MODEL_YAML, sc.MODEL_OPTS)
    model = refshim.reference_model(cfg)
    state = [[k, list(v.shape)] for k, v in model.state_dict().items()]        # in the reference's order
    model.load_state_dict(sc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.train()
    scaler = types.SimpleNamespace(scale=lambda loss: loss)

    def perturb(m):
        with torch.no_grad():
            for p in m.backbone.parameters():
                p.data.mul_(sc.PERTURB)

    runs = sc.drive(model, cfg, torch.device("cpu"),
                    lambda m, c, inputs, index, time, e: rc.contrastive_forward(m, c, inputs, index, time, e, scaler), perturb)
    its = []
    for it, r in enumerate(runs):
        assert bool((r["preds"][:, 0] == 9999.0).all()) and bool((r["preds"][:, 1:] == 0).all())
        its.append(dict(loss=r["loss"], grad_norm=r["grad_norm"], perform_backward=r["perform_backward"],
                        preds_shape=list(r["preds"].shape), grads=r["grads"], batches_tracked=r["batches_tracked"]))
        print("model iteration %d: loss %.6f grad_norm %.6f tracked %s" % (it, r["loss"], r["grad_norm"], r["batches_tracked"]))
    return dict(state=state, iterations=its)


def main():
    rc = load_reference()
    fx = dict(torch_version=torch.__version__, reference_yaml=sc.mc.MODEL_YAML)
    fx["model"] = record_model(rc)
    fx["ntx"], worst = record_ntx(rc)
    fx["ntx_worst_reference_ratio"] = worst
    with open(sc.GOLDEN, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
    print("wrote", sc.GOLDEN, os.path.getsize(sc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
