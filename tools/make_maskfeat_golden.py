"""Record tests/golden/maskfeat_contract.json from the UNMODIFIED reference (build container only).

What is recorded (results only; every input is a seed the tests draw again, tests/maskfeat_checks.py):
  masks   ``Kinetics._gen_mask`` (slowfast/datasets/kinetics.py:470-504) under ``random.seed(s)`` for the cube, tube and frame
          modes (SHA-256 of the table), plus one ``random.random()`` drawn afterwards;
  hog     ``HOGLayerC`` + ``MaskMViT._get_hog_label_3d`` (models/operators.py:62-112, models/masked.py:254-281) with an all-ones
          output mask on the HOG cases (a seeded sample of the larger outputs), the number of ambiguous elements of the fp64 restatement and the reference's largest
          deviation from that restatement on unambiguous cells (asserted <= 1e-6);
  model   the tiny MaskMViT of tests/maskfeat_checks.py in fp32: state-dict digest, loss, gradient norm, a seeded sample of the
          gathered predictions, (norm, seeded random projection) of every parameter gradient -- the numbers that pin
          maskfeat_checks.oracle_run, through which the tests compare every element; and the reference's own run under torch.autocast("cpu", float16 / bfloat16) as the yardstick
          (``hogs[0].forward`` wrapped to run in fp32 outside autocast: HOGLayerC.scatter_add_ fails on half inputs).

The reference is loaded through oracle/refshim.install(); ``slowfast.utils.misc`` (psutil, torchvision, matplotlib, fvcore
counters -- not used on this path) is pre-seeded with an empty stand-in, the dataset modules are loaded by file path with
stand-ins for the image libraries they import.

    python tools/make_maskfeat_golden.py
"""
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tests import maskfeat_checks as mc  # noqa: E402
from tests import model_checks  # noqa: E402

REFERENCE_ROOT = refshim.REFERENCE_ROOT


class _Anything(types.ModuleType):
    """A stand-in module: every attribute exists."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def _standin(name, **attrs):
    m = _Anything(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def load_reference_model_code():
    refshim.install()
    if "slowfast.utils.misc" not in sys.modules:
        misc = types.ModuleType("slowfast.utils.misc")
        sys.modules["slowfast.utils.misc"] = misc
        sys.modules["slowfast.utils"].misc = misc
    import slowfast.models.masked  # noqa: F401  (registers MaskMViT)


def load_reference_kinetics():
    """The reference's Kinetics class (for _gen_mask) loaded by file path."""
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "PIL", "PIL.Image",
                 "PIL.ImageFilter", "scipy", "scipy.ndimage", "cv2", "pandas", "slowfast.utils.env"):
        if name not in sys.modules:
            _standin(name)

    class _Registry:
        def register(self):
            return lambda cls: cls

    pkg = types.ModuleType("reference_datasets")
    pkg.__path__ = []
    sys.modules["reference_datasets"] = pkg
    for stem in ("rand_augment", "random_erasing", "decoder", "utils", "video_container"):
        _standin("reference_datasets." + stem)
    _standin("reference_datasets.build", DATASET_REGISTRY=_Registry())
    mods = {}
    for stem in ("transform", "kinetics"):
        path = os.path.join(REFERENCE_ROOT, "slowfast", "datasets", stem + ".py")
        spec = importlib.util.spec_from_file_location("reference_datasets." + stem, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        setattr(pkg, stem, mod)
        spec.loader.exec_module(mod)
        mods[stem] = mod
    return mods["kinetics"].Kinetics


def record_masks(Kinetics):
    out = {}
    for case in mc.MASK_CASES:
        holder = types.SimpleNamespace(cfg=mc.mask_cfg(case))
        for seed in case["seeds"]:
            random.seed(seed)
            table = np.stack([Kinetics._gen_mask(holder) for _ in range(case["draws"])]).astype(np.uint8)
            after = random.random()
            out["%s/%d" % (case["name"], seed)] = dict(shape=list(table.shape), masked=int(table.sum()),
                                                      sha256=mc.table_digest(torch.from_numpy(table)), random_after=after)
    return out


def reference_model(name):
    cfg = refshim.reference_cfg(mc.MODEL_YAML, mc.model_opts(name))
    model = refshim.reference_model(cfg)
    model.load_state_dict(mc.seeded_state(model))
    return cfg, model.train()


def record_hog(model):
    out = {}
    for case in mc.HOG_CASES:
        x, ref = mc.hog_reference(case)
        fs = case["fs"]
        Tu = (case["T"] + case["ts"] - 1) // case["ts"]
        model.cfg.MVIT.PATCH_STRIDE = [case["ts"], 4, 4]
        model.pretrain_depth, model.feat_size = [0], [[Tu, fs, fs]]
        ones = torch.ones((case["B"], Tu * fs * fs), dtype=torch.bool)
        with torch.no_grad():
            label = model._get_hog_label_3d(x, [ones])[0][0]
        got = label.view(case["B"], Tu * fs * fs, -1)
        assert tuple(got.shape) == tuple(ref["out"].shape), (got.shape, ref["out"].shape)
        amb = ref["ambiguous"]
        dev = float(((got.double() - ref["out"]).abs() * (~amb)).max())
        frac = float(amb.float().mean())
        print("hog %-10s reference vs fp64 restatement %.3e on unambiguous cells; ambiguous %.4f" % (case["name"], dev, frac))
        assert dev <= 1e-6 and frac <= mc.HOG_MAX_AMBIGUOUS
        idx = mc.sample_index(got.numel(), case["seed"], mc.SAMPLE)
        out[case["name"]] = dict(shape=list(got.shape), out=mc.f32_bytes(got.flatten()[idx]), ambiguous_elements=int(amb.sum()),
                                 reference_deviation=dev)
    return out


def _run(model, clip, mask, autocast=None):
    from slowfast.models.losses import get_loss_func
    model.zero_grad(set_to_none=True)
    loss_fn = get_loss_func("multi_mse")(reduction="mean")
    if autocast is None:
        preds, labels = model([clip, torch.Tensor(), mask])
        loss, _ = loss_fn(preds, labels)
    else:
        hog = model.hogs[0]
        inner = hog.forward

        def fp32_hog(x):            # wraps the call; the reference is not edited
            with torch.autocast("cpu", enabled=False):
                return inner(x.float())
        hog.forward = fp32_hog
        try:
            with torch.autocast("cpu", dtype=autocast):
                preds, labels = model([clip, torch.Tensor(), mask])
                loss, _ = loss_fn([p.float() for p in preds], [(l[0].float(),) + tuple(l[1:]) for l in labels])
        finally:
            hog.forward = inner
    loss.backward()
    grads = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
    return [p.detach().float() for p in preds], float(loss.detach()), grads


def record_model(name):
    cfg, model = reference_model(name)
    clip, mask = mc.model_inputs(cfg)
    preds, loss, grads = _run(model, clip, mask)
    gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
    rec = dict(state_digest=mc.state_digest(model.state_dict()), loss=loss, grad_norm=gn,
               preds=[dict(shape=list(p.shape), data=mc.f32_bytes(p.flatten()[mc.sample_index(p.numel(), mc.PROBE_SEED + i, mc.SAMPLE)]))
                      for i, p in enumerate(preds)],
               grads={k: mc.grad_probe(k, g) for k, g in grads.items()}, yardstick={})
    for dtype, key in ((torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
        a_preds, a_loss, a_grads = _run(model, clip, mask, autocast=dtype)
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
    fx["masks"] = record_masks(load_reference_kinetics())
    fx["model"] = {name: record_model(name) for name in mc.MODEL_CASES}
    fx["hog"] = record_hog(reference_model("depth3")[1])
    with open(mc.GOLDEN, "w") as f:
        json.dump(fx, f)
    print("wrote", mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
