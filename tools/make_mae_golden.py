"""Record tests/golden/mae_contract.json from the UNMODIFIED reference (build container only).

What is recorded (results only; every input is a seed the tests draw again, tests/mae_checks.py):
  masks   ``MaskMViT._mae_random_masking`` (slowfast/models/masked.py:283-317) under ``torch.manual_seed(s)`` for a few
          (N, L, ratio): SHA-256 of the int32 ids_restore table and len_keep.  The tool asserts that the noise has no equal
          values, so the table does not depend on how a sort orders ties;
  pixels  ``MaskMViT._get_pixel_label_3d`` (masked.py:212-230, with ``_patchify``) with an all-ones output mask on the pixel
          cases: a seeded sample of the output and the reference's largest deviation from the fp64 restatement in units of the
          tests' per-element bound (asserted <= 1 on the well-conditioned inputs, printed for the others);
  model   the tiny MAE MaskMViTs of tests/mae_checks.py in fp32: state-dict keys and shapes, the digest of the ids_restore table the
          forward drew, loss, gradient norm, a seeded sample of the gathered predictions, (norm, seeded random projection) of every
          parameter gradient -- the numbers that pin mae_checks.oracle_run, through which the tests compare every element; and the
          reference's own run under torch.autocast("cpu", float16 / bfloat16) as the yardstick.

The reference is loaded through oracle/refshim.install(); ``slowfast.utils.misc`` (psutil, torchvision, matplotlib, fvcore
counters -- not used on this path) is pre-seeded with an empty stand-in.

    python tools/make_mae_golden.py
"""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tests import mae_checks as mc  # noqa: E402
from tests import model_checks  # noqa: E402


def load_reference_model_code():
    refshim.install()
    if "slowfast.utils.misc" not in sys.modules:
        misc = types.ModuleType("slowfast.utils.misc")
        sys.modules["slowfast.utils.misc"] = misc
        sys.modules["slowfast.utils"].misc = misc
    import slowfast.models.masked  # noqa: F401  (registers MaskMViT)


def reference_model(name):
    cfg = refshim.reference_cfg(mc.MODEL_YAML, mc.model_opts(name))
    model = refshim.reference_model(cfg)
    model.load_state_dict(mc.seeded_state(model))
    return cfg, model.train()


def record_masks(model):
    out = {}
    for N, L, ratio, seeds in mc.MASK_CASES:
        for seed in seeds:
            torch.manual_seed(seed)
            noise = torch.rand(N, L)
            assert all(noise[b].unique().numel() == L for b in range(N)), "equal noise values: choose another seed"
            torch.manual_seed(seed)
            holder = types.SimpleNamespace(cfg=model.cfg)
            x_masked, mask, ids_restore, _ = type(model)._mae_random_masking(holder, torch.zeros(N, L, 1), ratio)
            table = ids_restore.to(torch.int32)
            assert torch.equal(mask, (ids_restore >= x_masked.shape[1]).float())
            out[mc.mask_key(N, L, ratio, seed)] = dict(len_keep=int(x_masked.shape[1]), sha256=mc.table_digest(table))
    return out


def record_pixels(model):
    out = {}
    for name, c in mc.PIXEL_CASES.items():
        for kind in mc.PIXEL_INPUTS:
            x, ref, bound, const = mc.pixel_reference(name, kind)
            model.cfg.MVIT.PATCH_STRIDE = [c["ts"], c["p"], c["p"]]
            model.patch_stride = [c["ts"], c["p"], c["p"]]
            model.pretrain_depth, model.feat_stride = [0], [[c["ts"], c["p"], c["p"]]]
            ones = torch.ones(tuple(ref.shape[:2]), dtype=torch.bool)
            with torch.no_grad():
                label = model._get_pixel_label_3d(x, [ones], time_stride_loss=c["u"] == 1, norm=True)[0][0]
            got = label.view(ref.shape)
            dev = float(((got.double() - ref).abs() / bound.clamp(min=1e-300))[~const].max())
            worst_const = float(got[const].abs().max()) if bool(const.any()) else 0.0
            print("pixels %-8s %-9s reference vs fp64: %.3f of the bound; on constant rows |out| <= %.3e" % (name, kind, dev, worst_const))
            if kind in mc.PIXEL_RECORDED:
                assert dev <= 1.0
            idx = mc.sample_index(got.numel(), c["seed"], mc.PIXEL_SAMPLE)
            out["%s/%s" % (name, kind)] = dict(shape=list(got.shape), reference_deviation=dev, reference_on_constant_rows=worst_const)
            if kind != "constant":
                out["%s/%s" % (name, kind)]["out"] = mc.f32_bytes(got.flatten()[idx])
    return out


def _run(model, clip, autocast=None):
    from slowfast.models.losses import get_loss_func
    model.zero_grad(set_to_none=True)
    loss_fn = get_loss_func("multi_mse")(reduction="mean")
    torch.manual_seed(mc.MASK_SEED)             # the forward draws torch.rand(N, L): the table of mae_checks.model_inputs
    if autocast is None:
        preds, labels = model([clip])
        loss, _ = loss_fn(preds, labels)
    else:
        with torch.autocast("cpu", dtype=autocast):
            preds, labels = model([clip])
            loss, _ = loss_fn([p.float() for p in preds], [(l[0].float(),) + tuple(l[1:]) for l in labels])
    loss.backward()
    grads = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
    return [p.detach().float() for p in preds], float(loss.detach()), grads


def record_model(name):
    cfg, model = reference_model(name)
    clip, ids = mc.model_inputs(cfg)
    preds, loss, grads = _run(model, clip)
    # the table the forward drew, recovered from the reference's own masking under the same seed
    torch.manual_seed(mc.MASK_SEED)
    L = ids.shape[1]
    _, _, ids_ref, _ = model._mae_random_masking(torch.zeros(mc.BATCH, L, 1), cfg.AUG.MASK_RATIO)
    assert torch.equal(ids_ref.to(torch.int32), ids), "mae_checks.model_inputs does not draw the reference's table"
    gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
    rec = dict(state=mc.state_list(model.state_dict()), ids_sha256=mc.table_digest(ids), loss=loss, grad_norm=gn,
               preds=[dict(shape=list(p.shape), data=mc.f32_bytes(p.flatten()[mc.sample_index(p.numel(), mc.PROBE_SEED + i, mc.SAMPLE)]))
                      for i, p in enumerate(preds)],
               grads={k: mc.grad_probe(k, g) for k, g in grads.items()}, yardstick={})
    for dtype, key in ((torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
        a_preds, a_loss, a_grads = _run(model, clip, autocast=dtype)
        worst, _ = model_checks._param_worst(a_grads, grads, gn)
        agn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in a_grads.values())))
        rec["yardstick"][key] = dict(
            preds=max(float((a - p).abs().max() / p.abs().max()) for a, p in zip(a_preds, preds)),
            loss=abs(a_loss - loss) / max(1.0, abs(loss)), grad_norm=abs(agn - gn) / gn,
            grad_global=model_checks._global_rel(a_grads, grads), param_grad_worst=worst)
        print(name, key, {k: "%.2e" % v for k, v in rec["yardstick"][key].items()})
    print(name, "loss %.6f grad_norm %.6f, %d parameters" % (loss, gn, len(grads)))
    return rec


def main():
    torch.manual_seed(0)
    load_reference_model_code()
    fx = dict(torch_version=torch.__version__, reference_yaml=mc.MODEL_YAML)
    fx["model"] = {name: record_model(name) for name in mc.MODEL_CASES}
    model = reference_model("ratio75")[1]
    fx["masks"] = record_masks(model)
    fx["pixels"] = record_pixels(model)
    with open(mc.GOLDEN, "w") as f:
        json.dump(fx, f)
    print("wrote", mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
