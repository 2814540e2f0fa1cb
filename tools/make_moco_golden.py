"""Record tests/golden/moco_contract.json from the UNMODIFIED reference (build container only).

Results only; every input is a seed tests/moco_checks.py draws again.  Recorded:
  nce      per loss case of moco_checks.nce_recorded_cases(): the reference's own fp32 run -- its Normalize and ContrastiveLoss
           classes around the einsum / cat / div lines of ContrastiveModel.forward (contrastive.py:452-477), autograd for df --
           as a loss, a seeded sample of the logits, and its deviation from the fp64 restatement in units of the tests'
           per-element bounds (logits, loss, df).  Asserted <= 1: the condition the bounds have to meet.
  l2norm   Normalize on the l2norm cases: the same ratio.
  ema      ContrastiveModel._update_history, unbound on a holder with two one-tensor modules: SHA-256 of the history.
  enqueue  ContrastiveModel._dequeue_and_enqueue, unbound on a holder: SHA-256 of the queue and the pointer.
  anneal   ContrastiveModel.momentum_anneal_cosine, unbound on a holder.
  model    a tiny reference ContrastiveModel (slow_tiny + the MoCo keys of moco_checks.MODEL_OPTS) driven for two iterations of
           the reference's contrastive_forward with 3 crops of batch 4, the shuffle on: state-dict keys and shapes, per iteration
           the loss, a seeded sample of the logits and the gradient norm; afterwards ptr, iter, which queue rows were written, the
           digest of the others and of every backbone_hist parameter.

The reference is loaded through oracle/refshim.install().  ``slowfast.utils.distributed`` (the process-group helpers, not used
with one device) is pre-seeded with a stand-in, and ``.cuda()`` is the identity in this process: the reference runs on the CPU.

    python tools/make_moco_golden.py
"""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tests import moco_checks as mc  # noqa: E402


def load_reference():
    refshim.install()
    if "slowfast.utils.distributed" not in sys.modules:
        du = types.ModuleType("slowfast.utils.distributed")
        du.get_world_size = lambda: 1
        du.get_rank = du.get_local_rank = lambda: 0
        du.get_local_size = lambda: 1
        sys.modules["slowfast.utils.distributed"] = du
        sys.modules["slowfast.utils"].distributed = du
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    import slowfast.models.contrastive as rc
    return rc


def record_nce(rc):
    from slowfast.models.losses import ContrastiveLoss
    norm, loss_fn = rc.Normalize(), ContrastiveLoss(reduction="mean")
    out = {}
    for n, V, K, C, kind in mc.nce_recorded_cases():
        r = mc.nce_reference(n, V, K, C, kind)
        f = r["f"].clone().requires_grad_(True)
        q = norm(f)
        queue_neg = torch.einsum("nc,kc->nk", [q, r["queue"].clone().detach()])
        for k, key in enumerate(r["keys"]):
            out_pos = torch.einsum("nc,nc->n", [q, key]).unsqueeze(-1)
            lgt_k = torch.cat([out_pos, queue_neg], dim=1)
            logits = lgt_k if k == 0 else torch.cat([logits, lgt_k], dim=0)
        logits = torch.div(logits, r["T"])
        loss = loss_fn(logits)
        loss.backward()
        l2, ls2 = mc.reference_sequence(r["f"], r["keys"], r["queue"], r["T"])
        assert torch.equal(l2, logits.detach()) and torch.equal(ls2, loss.detach()), "moco_checks.reference_sequence drifted"
        ratios = mc.nce_ratios(r, logits, loss, f.grad)
        print("nce %-36s reference vs fp64: logits %.3f loss %.3f df %.3f of the bounds" % ((mc.nce_key(n, V, K, C, kind),) + ratios))
        assert max(ratios) <= 1.0, ratios
        idx = mc.sample_index(logits.numel(), 1, 64)
        out[mc.nce_key(n, V, K, C, kind)] = dict(loss=float(loss), logits_sample=mc.f32_list(logits.flatten()[idx]),
                                                 reference_ratio=list(ratios))
    return out


def record_l2norm(rc):
    out = {}
    for n, C in mc.L2_CASES:
        for scale in mc.L2_SCALES:
            x = mc.l2_input(n, C, scale)
            ref, bound = mc.l2_reference(x)
            ratio = float(((rc.Normalize()(x).double() - ref).abs() / bound).max())
            print("l2norm n=%d C=%d scale=%g reference vs fp64: %.3f of the bound" % (n, C, scale, ratio))
            assert ratio <= 1.0
            out["n%d_C%d_s%g" % (n, C, scale)] = ratio
    return out


def record_ema(rc):
    out = {}
    for n in mc.EMA_SIZES:
        for m in mc.EMA_M:
            p, h = mc.ema_inputs(n)
            holder = types.SimpleNamespace(iter=torch.ones([1], dtype=torch.long), mmt=m,
                                           backbone=torch.nn.ParameterDict({"w": torch.nn.Parameter(p.clone())}),
                                           backbone_hist=torch.nn.ParameterDict({"w": torch.nn.Parameter(h.clone())}))
            rc.ContrastiveModel._update_history(holder)
            out["n%d_m%r" % (n, m)] = mc.digest(holder.backbone_hist["w"].data)
    return out


def record_enqueue(rc):
    out = {}
    for views, multi, start in ((3, True, 0), (1, True, 0), (3, False, 0), (3, False, 8), (1, True, 4)):
        queue, keys = mc.enqueue_inputs(views=views)
        cfg = types.SimpleNamespace(CONTRASTIVE=types.SimpleNamespace(MOCO_MULTI_VIEW_QUEUE=multi))
        holder = types.SimpleNamespace(cfg=cfg, ptr=torch.tensor([start]), queue_x=queue.clone(), k=queue.shape[0])
        rc.ContrastiveModel._dequeue_and_enqueue(holder, keys)
        out["views%d_multi%d_start%d" % (views, int(multi), start)] = dict(queue_sha256=mc.digest(holder.queue_x),
                                                                            ptr=int(holder.ptr))
    return out


def record_anneal(rc):
    cfg = types.SimpleNamespace(CONTRASTIVE=types.SimpleNamespace(MOMENTUM=0.994), SOLVER=types.SimpleNamespace(MAX_EPOCH=200))
    holder = types.SimpleNamespace(cfg=cfg, mmt=0.994)
    vals = []
    for e in (0.0, 0.5, 17.25, 100.0, 199.9, 200.0):
        rc.ContrastiveModel.momentum_anneal_cosine(holder, e)
        vals.append([e, holder.mmt])
    return dict(max_epoch=200, values=vals)


def record_model(rc):
    cfg = refshim.reference_cfg(mc.MODEL_YAML, mc.MODEL_OPTS)
    model = refshim.reference_model(cfg)
    state = mc.state_list(model.state_dict())
    sd0 = mc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, cfg.CONTRASTIVE.QUEUE_LEN,
                          cfg.CONTRASTIVE.DIM)
    model.load_state_dict(sd0)
    model.train()
    scaler = types.SimpleNamespace(scale=lambda loss: loss)
    runs = mc.drive(model, cfg, torch.device("cpu"),
                    lambda m, c, inputs, index, time, e: rc.contrastive_forward(m, c, inputs, index, time, e, scaler))
    its = []
    for it, r in enumerate(runs):
        idx = mc.sample_index(r["logits"].numel(), 100 + it, mc.LOGITS_SAMPLE)
        its.append(dict(loss=r["loss"], grad_norm=r["grad_norm"], logits_shape=list(r["logits"].shape),
                        logits_absmax=float(r["logits"].abs().max()), logits_sample=mc.f32_list(r["logits"].flatten()[idx])))
        print("model iteration %d: loss %.6f grad_norm %.6f" % (it, r["loss"], r["grad_norm"]))
    sd = model.state_dict()
    K = sd["queue_x"].shape[0]
    changed = [r for r in range(K) if not torch.equal(sd["queue_x"][r], sd0["queue_x"][r])]
    keep = [r for r in range(K) if r not in changed]
    params = dict(model.named_parameters())
    return dict(state=state, iterations=its, ptr=int(sd["ptr"]), iter=int(sd["iter"]), queue_rows_written=changed,
                queue_unwritten_sha256=mc.digest(sd["queue_x"][keep]),
                hist_sha256={k: mc.digest(v) for k, v in sd.items() if k.startswith("backbone_hist.") and k in params})


def main():
    rc = load_reference()
    fx = dict(torch_version=torch.__version__, reference_yaml=mc.MODEL_YAML)
    fx["model"] = record_model(rc)
    fx["nce"] = record_nce(rc)
    fx["l2norm"] = record_l2norm(rc)
    fx["ema"] = record_ema(rc)
    fx["enqueue"] = record_enqueue(rc)
    fx["anneal"] = record_anneal(rc)
    with open(mc.GOLDEN, "w") as f:
        json.dump(fx, f)
    print("wrote", mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
