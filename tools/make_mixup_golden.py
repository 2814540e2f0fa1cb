"""Records tests/golden/mixup_contract.json from the UNMODIFIED reference's slowfast/datasets/mixup.py.  Build container only
(needs the reference tree).

    python tools/make_mixup_golden.py

The module is loaded BY FILE PATH: the package around it imports decoders that are not installed, the file itself needs numpy
and torch only.  Per case (constructor arguments, np.random seed, batch size): the inputs are drawn from a seeded
torch.Generator (the test draws them again), the reference's MixUp is called on them, and the fixture keeps what it returned
-- lam as the exact double, whether cutmix was used, the box, the mixed clip and the soft labels.  lam / use_cutmix / box are
read by running the reference's own draw functions a second time from the same seed.  Recorded results only: no reference
program text goes into the fixture or this tool.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("SLOWFAST_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "mixup_contract.json")

CLIP = (3, 2, 6, 10)        # (C, T, H, W) of every case
NUM_CLASSES = 7

# (constructor arguments besides num_classes, np.random seed, batch size)
CASES = [
    (dict(mixup_alpha=0.8, cutmix_alpha=0.0), 0, 2),                                    # mixup only
    (dict(mixup_alpha=0.8, cutmix_alpha=0.0, label_smoothing=0.0), 1, 3),               # ... odd batch, no smoothing
    (dict(mixup_alpha=0.0, cutmix_alpha=1.0), 2, 2),                                    # cutmix only
    (dict(mixup_alpha=0.0, cutmix_alpha=1.0), 3, 3),                                    # ... odd batch
    (dict(mixup_alpha=0.0, cutmix_alpha=1.0, correct_lam=False), 4, 4),                 # lam not corrected for the clipped box
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5), 5, 2),                   # both, switching
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5), 6, 4),
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5), 7, 3),
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5), 11, 2),
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.0), 8, 2),                      # never mixed: no draw at all
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.5), 9, 2),                      # mixed or not by the first draw
    (dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.5), 10, 2),
]


def load_reference():
    path = os.path.join(REFERENCE_ROOT, "slowfast", "datasets", "mixup.py")
    spec = importlib.util.spec_from_file_location("reference_mixup", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_inputs(data_seed, batch):
    """The inputs of a case (tests/mixup_checks.py draws the same)."""
    g = torch.Generator().manual_seed(data_seed)
    x = torch.randn((batch,) + CLIP, generator=g)
    y = torch.randint(0, NUM_CLASSES, (batch,), generator=g)
    return x, y


def f32_list(t):
    """float32 tensor -> flat list of Python floats whose JSON text is the shortest decimal that reads back to the same float32."""
    out = []
    for v in t.detach().contiguous().view(-1).numpy():
        f = float(str(v))
        if np.float32(f) != v:
            f = float(v)
        assert np.float32(f) == v
        out.append(f)
    return out


def main():
    ref = load_reference()
    cases = []
    for i, (args, seed, batch) in enumerate(CASES):
        x, y = case_inputs(1000 + i, batch)
        fn = ref.MixUp(num_classes=NUM_CLASSES, **args)
        np.random.seed(seed)
        mixed, target = fn(x.clone(), y)
        # the draw behind it, from the same seed
        np.random.seed(seed)
        lam, use_cutmix, box = 1.0, False, None
        if fn.mix_prob > 0.0:
            lam, use_cutmix = fn._get_mixup_params()
            if lam == 1.0:
                use_cutmix = False
            elif use_cutmix:
                (yl, yh, xl, xh), lam = ref.get_cutmix_bbox(x.shape, lam, correct_lam=fn.correct_lam)
                box = [int(yl), int(yh), int(xl), int(xh)]
        np.random.seed(seed)
        assert fn.mix_prob == 0.0 or float(fn._mix_batch(x.clone())) == float(lam)
        cases.append({"args": args, "np_seed": seed, "data_seed": 1000 + i, "batch": batch, "lam": repr(float(lam)),
                      "use_cutmix": bool(use_cutmix), "box": box, "clip": f32_list(mixed), "target": f32_list(target)})
        print(i, args, "B", batch, "lam", repr(float(lam)), "cutmix", bool(use_cutmix), box)
    doc = {"clip_shape": list(CLIP), "num_classes": NUM_CLASSES, "torch_version": torch.__version__,
           "numpy_version": np.__version__, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
