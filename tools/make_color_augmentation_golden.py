"""Records tests/golden/color_augmentation_contract.json from the UNMODIFIED reference's slowfast/datasets/transform.py
(``color_jitter``, ``lighting_jitter``, ``color_normalization``) and slowfast/datasets/ava_dataset.py
(``Ava._images_and_boxes_preprocessing``).  Build container only (needs the reference tree).

    python tools/make_color_augmentation_golden.py

The reference is loaded BY FILE PATH with stand-in modules exactly as tools/make_spatial_sampling_golden.py loads it;
``ava_dataset.py`` loads the same way (its registry decorator gets a stand-in that returns the class), and
``Ava._images_and_boxes_preprocessing`` is called unbound on a ``types.SimpleNamespace`` that carries the attributes it reads.

Two kinds of cases, all with S = 12 and T = 3.  Every sample's uint8 frames are drawn from a seeded ``torch.Generator`` with a
different brightness range per frame and per channel (the test draws them again), so that a mean over the clip differs from a
mean over a frame and the grey value depends on which channel gets which weight.

* colour cases: the (T, 3, S, S) image ``frames / 255.0`` goes through the reference's ``color_jitter``, ``lighting_jitter``,
  ``color_normalization`` and -- ``reverse`` -- the channel reordering, in the order ava_dataset.py:306-333 calls them, sample
  after sample under one seed of ``np.random``.
* whole-pipeline cases: uint8 (T, h, w, 3) frames and (K, 4) boxes go through ``Ava._images_and_boxes_preprocessing`` (train,
  train with a flip, val, val with AVA.TEST_FORCE_FLIP); one of the boxes crosses the crop border.

Per case the fixture keeps
* ``order`` / ``alpha`` / ``rgb``: per sample the drawn op order (0 brightness, 1 contrast, 2 saturation), the blend factors and
  the PCA term, captured by wrapping ``np.random.permutation`` / ``uniform`` / ``normal`` and ``np.sum`` while the reference runs;
* ``np_after``: one ``np.random.uniform()`` drawn right afterwards: how far the generator got;
* ``out``: the reference's output, float32 little-endian bytes in base64, layout (N, 3, T, S, S); ``boxes``: its boxes;
* ``effect_diff``: the smallest mean absolute difference between that output and three deliberately wrong variants of it (the
  contrast mean taken over the whole clip instead of per frame; ``rgb[c]`` instead of ``rgb[2 - c]``; the R and B grey weights
  swapped), over the variants the case can tell apart (null when it can tell none).  The variants are computed by this tool's own
  float64 restatement from the recorded draws; the restatement without a variant must agree with the reference to 1e-5.

Seeds are found by search so that every drawn ``|1 - alpha| >= 0.1`` and ``|rgb[0] - rgb[2]| >= 0.02``: otherwise the wrong
variants are too close to the right answer to tell apart.  Recorded results only: no reference program text goes into the
fixture or this tool.
"""
import base64
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_spatial_sampling_golden import REFERENCE_ROOT, ROOT, _standin, load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "color_augmentation_contract.json")

S, T = 12, 3
MEAN, STD = [0.45, 0.40, 0.35], [0.225, 0.25, 0.2]
EIGVAL = [0.225, 0.224, 0.229]
EIGVEC = [[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]]
LAND, PORT = (18, 26), (26, 18)
BOXES = [[0.10, 0.20, 0.60, 0.90], [0.40, 0.05, 0.98, 0.70], [0.0, 0.0, 1.0, 1.0], [0.30, 0.35, 0.55, 0.60]]
ALL = dict(brightness=0.4, contrast=0.4, saturation=0.4, alphastd=0.1)
OFF = dict(brightness=0.0, contrast=0.0, saturation=0.0, alphastd=0.0)

# (name, ColorAugmentation arguments without eigval / eigvec / mean / std, number of samples)
COLOR_CASES = [
    ("brightness alone", dict(OFF, brightness=0.4), 1),
    ("contrast alone", dict(OFF, contrast=0.4), 1),
    ("saturation alone", dict(OFF, saturation=0.4), 1),
    ("all three ops and lighting", dict(ALL), 1),
    ("PCA lighting only", dict(OFF, alphastd=0.1), 1),
    ("all three ops, alphastd 0", dict(ALL, alphastd=0.0), 1),
    ("nothing on: normalise and reorder", dict(OFF), 1),
    ("all three ops and lighting, reverse off", dict(ALL, reverse=False), 1),
    ("N 3: a draw per sample", dict(ALL), 3),
]
# (name, split, flip wanted or None, AVA.TEST_FORCE_FLIP, frame size)
PIPELINE_CASES = [
    ("pipeline: train", "train", 0, False, LAND),
    ("pipeline: train, flipped, portrait", "train", 1, False, PORT),
    ("pipeline: val", "val", None, False, LAND),
    ("pipeline: val, forced flip", "val", None, True, LAND),
]
JITTER = (14, 20)


def load_ava(tr, ut):
    """The reference's ava_dataset module, loaded by file path beside the transform / utils modules of load_reference()."""
    import importlib.util

    class _Registry:
        def register(self):
            return lambda cls: cls

    _standin("reference_datasets.ava_helper")
    _standin("reference_datasets.cv2_transform")
    _standin("reference_datasets.build", DATASET_REGISTRY=_Registry())
    path = os.path.join(REFERENCE_ROOT, "slowfast", "datasets", "ava_dataset.py")
    spec = importlib.util.spec_from_file_location("reference_datasets.ava_dataset", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def case_frames(data_seed, sizes):
    """uint8 (T, h, w, 3) frames per sample; every frame and every channel is drawn from its own brightness range
    (tests/color_augmentation_checks.py draws the same)."""
    g = torch.Generator().manual_seed(data_seed)
    out = []
    for h, w in sizes:
        out.append(torch.stack([torch.stack([torch.randint(20 + 45 * t + 30 * c, 100 + 45 * t + 30 * c, (h, w), generator=g,
                                                           dtype=torch.int64) for c in range(3)], dim=-1)
                                for t in range(T)]).to(torch.uint8))
    return out


class Recorder:
    """Wraps the numpy calls the reference's colour functions make and files what they return, per sample."""

    def __init__(self):
        self.samples = []

    def begin(self):
        self.samples.append({"order": [], "alpha": [], "rgb": None, "pending": None})

    def __enter__(self):
        self.saved = (np.random.permutation, np.random.uniform, np.random.normal, np.sum)
        perm, uni, nor, npsum = self.saved

        def permutation(x):
            out = perm(x)
            self.samples[-1]["pending"] = [int(v) for v in out]
            return out

        def uniform(*a, **kw):
            out = uni(*a, **kw)
            if self.samples and self.samples[-1]["pending"] is not None and len(a) == 2 and a[0] == -a[1] and a[1] != 0:
                self.samples[-1]["alpha"].append(1.0 + out)
            return out

        def normal(*a, **kw):
            out = nor(*a, **kw)
            self.samples[-1]["lit"] = True
            return out

        def summed(x, *a, **kw):
            out = npsum(x, *a, **kw)
            if self.samples and self.samples[-1].pop("lit", False):
                self.samples[-1]["rgb"] = [float(v) for v in out]
            return out

        np.random.permutation, np.random.uniform, np.random.normal, np.sum = permutation, uniform, normal, summed
        return self

    def __exit__(self, *exc):
        np.random.permutation, np.random.uniform, np.random.normal, np.sum = self.saved

    def finish(self, ratios):
        """Per sample: the op codes in application order, the alphas, the PCA term."""
        out = []
        for s in self.samples:
            listed = [code for code, var in enumerate(ratios) if var != 0]
            order = [listed[i] for i in (s["pending"] or [])]
            assert len(order) == len(s["alpha"]), (order, s["alpha"])
            out.append({"order": order, "alpha": s["alpha"], "rgb": s["rgb"]})
        return out


def restate(x, draws, mean, std, reverse, variant=0):
    """This tool's float64 restatement on one sample's (3, T, S, S) image, from the recorded draws.  variant 1: the contrast
    mean over the whole clip; 2: rgb[c] instead of rgb[2 - c]; 3: the R and B grey weights swapped."""
    v = x.double().clone()
    wb, wg, wr = (0.299, 0.587, 0.114) if variant == 3 else (0.114, 0.587, 0.299)
    for op, a in zip(draws["order"], draws["alpha"]):
        gray = wb * v[0] + wg * v[1] + wr * v[2]
        if op == 0:
            v = v * a
        elif op == 1:
            m = gray.mean() if variant == 1 else gray.mean(dim=(1, 2), keepdim=True)
            v = v * a + m * (1.0 - a)
        else:
            v = v * a + gray * (1.0 - a)
    if draws["rgb"] is not None:
        for c in range(3):
            v[c] = v[c] + draws["rgb"][c if variant == 2 else 2 - c]
    for c in range(3):
        v[c] = (v[c] - mean[c]) / std[c]
    return v.flip(0) if reverse else v


def effect_of(inputs, outs, draws, reverse):
    """(smallest mean |reference - wrong variant| over the variants the case can tell apart or None, largest
    |reference - restatement|)."""
    ref = torch.stack(outs).double()
    same = torch.stack([restate(x, d, MEAN, STD, reverse) for x, d in zip(inputs, draws)])
    effects = []
    for variant, applies in ((1, any(1 in d["order"] for d in draws)), (2, any(d["rgb"] is not None for d in draws)),
                             (3, any(1 in d["order"] or 2 in d["order"] for d in draws))):
        if applies:
            wrong = torch.stack([restate(x, d, MEAN, STD, reverse, variant) for x, d in zip(inputs, draws)])
            effects.append(float((ref - wrong).abs().mean()))
    return (min(effects) if effects else None), float((ref - same).abs().max())


def separated(draws):
    return all(abs(1.0 - a) >= 0.1 for d in draws for a in d["alpha"]) and \
        all(abs(d["rgb"][0] - d["rgb"][2]) >= 0.02 for d in draws if d["rgb"] is not None)


def run_color(tr, args, N, seed, data_seed):
    ratios = (args["brightness"], args["contrast"], args["saturation"])
    frames = case_frames(data_seed, [(S, S)] * N)
    rec = Recorder()
    np.random.seed(seed)
    inputs, outs = [], []
    with rec:
        for f in frames:
            rec.begin()
            x = f.permute(0, 3, 1, 2).float() / 255.0                       # (T, 3, S, S), the reference's layout
            y = x
            if any(r != 0 for r in ratios):
                y = tr.color_jitter(y, img_brightness=ratios[0], img_contrast=ratios[1], img_saturation=ratios[2])
            y = tr.lighting_jitter(y, alphastd=args["alphastd"], eigval=np.array(EIGVAL).astype(np.float32),
                                   eigvec=np.array(EIGVEC).astype(np.float32))
            y = tr.color_normalization(y, np.array(MEAN, dtype=np.float32), np.array(STD, dtype=np.float32))
            if args.get("reverse", True):
                y = y[:, [2, 1, 0], ...]
            inputs.append(x.permute(1, 0, 2, 3).contiguous())
            outs.append(y.permute(1, 0, 2, 3).contiguous())
    np_after = float(np.random.uniform())
    return inputs, outs, rec.finish(ratios), np_after


def run_pipeline(tr, ava, split, force_flip, size, seed, data_seed):
    frames = case_frames(data_seed, [size])[0]
    this = types.SimpleNamespace(
        _split=split, _crop_size=S, _jitter_min_scale=JITTER[0], _jitter_max_scale=JITTER[1], _use_color_augmentation=True,
        _pca_jitter_only=False, _pca_eigval=EIGVAL, _pca_eigvec=EIGVEC, _data_mean=MEAN, _data_std=STD, _use_bgr=False,
        _test_force_flip=force_flip, random_horizontal_flip=True)
    seen = {}
    hflip = tr.horizontal_flip

    def rec_hflip(prob, images, boxes=None):
        out, b = hflip(prob, images, boxes=boxes)
        seen["flip"] = int(out is not images)
        return out, b

    rec = Recorder()
    np.random.seed(seed)
    tr.horizontal_flip = rec_hflip
    try:
        with rec:
            rec.begin()
            imgs, boxes = ava.Ava._images_and_boxes_preprocessing(this, frames.permute(0, 3, 1, 2), np.array(BOXES, dtype=np.float64))
    finally:
        tr.horizontal_flip = hflip
    np_after = float(np.random.uniform())
    assert tuple(imgs.shape) == (T, 3, S, S), tuple(imgs.shape)
    ratios = (0.4, 0.4, 0.4) if split == "train" else (0.0, 0.0, 0.0)
    return imgs.permute(1, 0, 2, 3).contiguous(), boxes, rec.finish(ratios), np_after, seen.get("flip", 0)


def b64(t):
    return base64.b64encode(t.numpy().astype("<f4").tobytes()).decode("ascii")


def main():
    tr, ut = load_reference()
    ava = load_ava(tr, ut)
    cases, tried, qualified = [], 0, 0
    for i, (name, args, N) in enumerate(COLOR_CASES):
        data_seed = 5000 + i
        for seed in range(4000):
            inputs, outs, draws, np_after = run_color(tr, args, N, seed, data_seed)
            tried += 1
            if separated(draws):
                qualified += 1
                break
        else:
            raise SystemExit("no seed in 0..3999 separates the variants of %r" % name)
        reverse = args.get("reverse", True)
        effect, restated = effect_of(inputs, outs, draws, reverse)
        assert restated < 1e-5, (name, restated)
        cases.append({"name": name, "kind": "color", "args": args, "N": N, "seed": seed, "data_seed": data_seed, "draws": draws,
                      "np_after": repr(np_after), "effect_diff": effect, "restated": restated, "out": b64(torch.stack(outs))})
        print(i, name, "seed", seed, "effect", effect, "restated %.2e" % restated, [d["order"] for d in draws])
    for j, (name, split, want_flip, force, size) in enumerate(PIPELINE_CASES):
        data_seed = 6000 + j
        for seed in range(4000):
            out, boxes, draws, np_after, flip = run_pipeline(tr, ava, split, force, size, seed, data_seed)
            if separated(draws) and (want_flip is None or flip == want_flip):
                break
        else:
            raise SystemExit("no seed in 0..3999 gives %r" % name)
        cases.append({"name": name, "kind": "pipeline", "split": split, "force_flip": force, "size": list(size),
                      "jitter": list(JITTER), "seed": seed, "data_seed": data_seed, "draws": draws, "flip": flip,
                      "np_after": repr(np_after), "boxes_in": BOXES, "boxes": [[float(v) for v in b] for b in boxes],
                      "effect_diff": None, "out": b64(out[None])})
        print(len(COLOR_CASES) + j, name, "seed", seed, "flip", flip, [d["order"] for d in draws], boxes.tolist())
    doc = {"torch_version": torch.__version__, "crop_size": S, "T": T, "mean": MEAN, "std": STD, "eigval": EIGVAL,
           "eigvec": EIGVEC, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes; %d of %d colour seeds tried qualified" % (qualified, tried))


if __name__ == "__main__":
    sys.exit(main())
