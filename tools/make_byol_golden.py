"""Record tests/golden/byol_contract.json from the UNMODIFIED reference (build container only).

Results only; every input is a seed tests/byol_checks.py draws again.  Recorded:
  sim      per loss case of the grid of byol_checks (n x V x C x T x input scale x kind): the reference's own fp32 run -- its
           Normalize class on the predictor output, ContrastiveModel.sim_loss (unbound on a holder that carries T) per key and
           the `+=` / `/= len(keys)` lines of the byol branch (contrastive.py:512, :532-535), autograd for df -- as a loss, a
           seeded sample of df, and its deviation from the fp64 restatement in units of the tests' bounds (loss, df).
           Asserted <= 1: the condition the bounds have to meet.
  model    a tiny reference ContrastiveModel (slow_tiny + the BYOL keys of byol_checks.MODEL_OPTS) driven for two iterations of
           the reference's contrastive_forward with CONTRASTIVE.SEQUENTIAL and one of the symmetric form, 2 crops of batch 4:
           state-dict keys (in the reference's order) and shapes, per iteration the loss, the gradient norm, perform_backward,
           the shape of the dummy logits, iter, ptr, the queue's digest and the annealed momentum; afterwards the digest of every
           backbone_hist parameter and num_batches_tracked of the heads' BatchNorm1d layers.

The reference is loaded through oracle/refshim.install().  ``slowfast.utils.distributed`` (the process-group helpers, not used
with one device) is pre-seeded with a stand-in, and ``.cuda()`` is the identity in this process: the reference runs on the CPU.

    python tools/make_byol_golden.py
"""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tests import byol_checks as bc  # noqa: E402
from tools.make_moco_golden import load_reference  # noqa: E402


def record_sim(rc):
    norm = rc.Normalize()
    out, worst = {}, [0.0, 0.0]
    for n, V, C in bc.SIM_SHAPES:
        for T, scale, kind in bc.sim_cases(n, V, C):
            r = bc.sim_reference(n, V, C, T, scale, kind)
            holder = types.SimpleNamespace(T=T)
            p = r["p"].clone().requires_grad_(True)
            keys = [k for k in r["keys"]]
            predictor = norm(p)
            loss_reg = rc.ContrastiveModel.sim_loss(holder, predictor, keys[0])
            for i in range(1, len(keys)):
                loss_reg += rc.ContrastiveModel.sim_loss(holder, predictor, keys[i])
            loss_reg /= len(keys)
            loss_reg.backward()
            again = bc.reference_sequence(r["p"], r["keys"], T)
            assert torch.equal(again, loss_reg.detach()), "byol_checks.reference_sequence drifted"
            ratios = bc.sim_ratios(r, loss_reg, p.grad)
            assert max(ratios) <= 1.0, (n, V, C, T, scale, kind, ratios)
            worst = [max(w, x) for w, x in zip(worst, ratios)]
            idx = bc.sample_index(n * C, 1, bc.DF_SAMPLE)
            out[bc.sim_key(n, V, C, T, scale, kind)] = dict(loss=float(loss_reg), df_sample=bc.f32_list(p.grad.flatten()[idx]),
                                                           reference_ratio=[float("%.4g" % x) for x in ratios])
        print("sim n=%d V=%d C=%d: reference vs fp64 so far: loss %.3f df %.3f of the bounds" % (n, V, C, worst[0], worst[1]))
    return out, worst


def record_model(rc):
    cfg = refshim.reference_cfg(bc.mc.MODEL_YAML, bc.MODEL_OPTS)
    model = refshim.reference_model(cfg)
    state = bc.state_list(model.state_dict())
    order = list(model.state_dict())
    sd0 = bc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, cfg.CONTRASTIVE.QUEUE_LEN,
                          cfg.CONTRASTIVE.DIM)
    model.load_state_dict(sd0)
    model.train()
    scaler = types.SimpleNamespace(scale=lambda loss: loss)

    def perturb(m):
        with torch.no_grad():
            for p in m.backbone.parameters():
                p.data.mul_(bc.PERTURB)

    runs = bc.drive(model, cfg, torch.device("cpu"),
                    lambda m, c, inputs, index, time, e: rc.contrastive_forward(m, c, inputs, index, time, e, scaler), perturb)
    its = []
    for it, r in enumerate(runs):
        assert bool((r["preds"][:, 0] == 9999.0).all()) and bool((r["preds"][:, 1:] == 0).all())
        its.append(dict(loss=r["loss"], grad_norm=r["grad_norm"], perform_backward=r["perform_backward"],
                        preds_shape=list(r["preds"].shape), iter=r["iter"], ptr=r["ptr"], queue_sha256=r["queue_sha256"],
                        mmt=r["mmt"], grads=r["grads"]))
        print("model iteration %d: loss %.6f grad_norm %.6f momentum %.6f" % (it, r["loss"], r["grad_norm"], r["mmt"]))
    sd = model.state_dict()
    params = dict(model.named_parameters())
    return dict(state=state, state_order=order, iterations=its,
                batches_tracked={k: int(v) for k, v in sd.items() if k.endswith("num_batches_tracked") and ".head." in k},
                hist_sha256={k: bc.digest(v) for k, v in sd.items() if k.startswith("backbone_hist.") and k in params})


def main():
    rc = load_reference()
    fx = dict(torch_version=torch.__version__, reference_yaml=bc.mc.MODEL_YAML)
    fx["model"] = record_model(rc)
    fx["sim"], worst = record_sim(rc)
    fx["sim_worst_reference_ratio"] = worst
    with open(bc.GOLDEN, "w") as f:
        json.dump(fx, f)
    print("wrote", bc.GOLDEN, os.path.getsize(bc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
