"""Records tests/golden/spatial_sampling_contract.json from the UNMODIFIED reference's slowfast/datasets/utils.py
(``tensor_normalize``, ``spatial_sampling``) and slowfast/datasets/transform.py.  Build container only (needs the reference
tree).

    python tools/make_spatial_sampling_golden.py

Both files are loaded BY FILE PATH into a stand-in package: ``transform.py`` imports torchvision, PIL and scipy at module
level and ``utils.py`` cv2 and the project's path manager, none of which the functions recorded here use, so empty stand-in
modules are put into ``sys.modules`` for them and for the sibling imports first (as oracle/refshim.py does for the models).

Per case (constructor arguments, the seed of ``random`` and ``np.random``, T, the frame size of every sample and -- in test
mode -- its spatial index): every sample's uint8 frames (T, h, w, 3) are drawn from a seeded ``torch.Generator`` (the test
draws them again), normalised by the reference's ``tensor_normalize``, permuted to (C, T, H, W) and passed through the
reference's ``spatial_sampling``, sample after sample.  The fixture keeps

* ``rows``: what the reference's draw implies, per sample, in the order of ``spatial_sampling.CropRow``.  It is read off the
  reference's own behaviour: the sizes it hands to ``F.interpolate``, the window ``_get_param_spatial_crop`` returns, the
  storage offset of the view its crop returns and whether ``horizontal_flip`` returned another tensor;
* ``py_after`` / ``np_after``: one ``random.random()`` and one ``np.random.uniform()`` drawn right after the calls: how far each
  generator got;
* ``out``: the reference's output, float32 little-endian bytes in base64, layout (N, C, T, S, S);
* ``shift_diff``: the mean absolute difference between that output and itself shifted by one pixel in x.

Some cases are found by a search over seeds (offsets at 0 and at the maximum, flip on / off, a window that touches no border,
a draw that retries, a draw that resizes); what the search looks at is the recorded row and the number of attempts the
reference made.  Recorded results only: no reference program text goes into the fixture or this tool.
"""
import base64
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("SLOWFAST_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "spatial_sampling_contract.json")

S = 12
MEAN, STD = [0.45, 0.40, 0.35], [0.225, 0.25, 0.2]
LAND, PORT = (18, 26), (26, 18)
JIT = dict(min_scale=14, max_scale=20, crop_size=S)

# (name, constructor arguments, T, [(height, width)] per sample, [spatial index] per sample or None, seed or a search name)
CASES = [
    ("jitter, landscape, upscale to 21", dict(min_scale=21, max_scale=21, crop_size=S), 2, [LAND], None, 0),
    ("jitter, portrait, downscale to 13", dict(min_scale=13, max_scale=13, crop_size=S), 2, [PORT], None, 1),
    ("jitter, short side already 18: no resize", dict(min_scale=18, max_scale=18, crop_size=S), 2, [LAND], None, 2),
    ("jitter, resized frame exactly S x S: no randint", dict(min_scale=S, max_scale=S, crop_size=S), 2, [(20, 20)], None, 3),
    ("jitter, offsets 0", JIT, 2, [LAND], None, "offsets_zero"),
    ("jitter, offsets at the maximum", JIT, 2, [LAND], None, "offsets_max"),
    ("jitter, flipped", JIT, 3, [LAND], None, "flip_on"),
    ("jitter, not flipped", JIT, 3, [LAND], None, "flip_off"),
    ("jitter, no flip draw", dict(JIT, random_horizontal_flip=False), 2, [LAND], None, 4),
    ("jitter, inverse uniform sampling", dict(JIT, inverse_uniform_sampling=True), 2, [PORT], None, "resized"),
    ("resized crop, window touches no border", dict(JIT, aspect_ratio=[0.75, 1.3333], scale=[0.3, 0.8]), 2, [LAND], None,
     "inside"),
    ("resized crop, retries", dict(JIT, aspect_ratio=[0.5, 2.0], scale=[0.7, 1.0]), 2, [LAND], None, "retry"),
    ("resized crop, central fallback", dict(JIT, aspect_ratio=[0.4, 0.5], scale=[0.9, 1.0]), 2, [LAND], None, 6),
    ("test, landscape, indices 0 1 2", dict(min_scale=14, max_scale=14, crop_size=S), 2, [LAND] * 3, [0, 1, 2], 7),
    ("test, portrait, indices 0 1 2", dict(min_scale=14, max_scale=14, crop_size=S), 2, [PORT] * 3, [0, 1, 2], 8),
    ("test, one spatial crop: index 1 at TRAIN_JITTER_SCALES[0]", dict(min_scale=16, max_scale=16, crop_size=S), 2, [LAND],
     [1], 9),
    ("N 3, three valid sizes in one padded buffer", JIT, 2, [LAND, PORT, (22, 24)], None, 10),
]


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


def load_reference():
    """(transform module, utils module) of the reference, loaded by file path."""
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "PIL", "PIL.Image",
                 "PIL.ImageFilter", "scipy", "scipy.ndimage", "cv2", "slowfast", "slowfast.utils", "slowfast.utils.env"):
        if name not in sys.modules:
            _standin(name)
    pkg = types.ModuleType("reference_datasets")
    pkg.__path__ = []
    sys.modules["reference_datasets"] = pkg
    _standin("reference_datasets.rand_augment")
    _standin("reference_datasets.random_erasing")
    mods = []
    for stem in ("transform", "utils"):
        path = os.path.join(REFERENCE_ROOT, "slowfast", "datasets", stem + ".py")
        spec = importlib.util.spec_from_file_location("reference_datasets." + stem, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        setattr(pkg, stem, mod)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def case_frames(data_seed, T, sizes):
    """The uint8 (T, h, w, 3) frames of every sample of a case (tests/spatial_sampling_checks.py draws the same)."""
    g = torch.Generator().manual_seed(data_seed)
    return [torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.int64).to(torch.uint8) for h, w in sizes]


def run_reference(tr, ut, args, T, sizes, idxs, seed, data_seed):
    """The reference on the case's samples, in order.  Returns (rows, outputs (N, C, T, S, S), random.random() after,
    np.random.uniform() after, attempts of _get_param_spatial_crop per sample)."""
    seen = {}
    interpolate, get_param = torch.nn.functional.interpolate, tr._get_param_spatial_crop
    random_crop, uniform_crop, hflip, uniform = tr.random_crop, tr.uniform_crop, tr.horizontal_flip, random.uniform

    def rec_interpolate(x, size=None, **kw):
        seen["res"] = tuple(int(v) for v in size)
        return interpolate(x, size=size, **kw)

    def rec_get_param(*a, **kw):
        seen["win"] = tuple(int(v) for v in get_param(*a, **kw))
        return seen["win"]

    def rec_crop(fn):
        def wrapped(images, *a, **kw):
            out, boxes = fn(images, *a, **kw)
            off = out.storage_offset() - images.storage_offset() if out.data_ptr() != images.data_ptr() else 0
            seen["off"] = (off // images.stride(2), off % images.stride(2) // images.stride(3))
            return out, boxes
        return wrapped

    def rec_hflip(prob, images, boxes=None):
        out, boxes = hflip(prob, images, boxes)
        seen["flip"] = int(out is not images)
        return out, boxes

    def counting_uniform(a, b):
        seen["uniforms"] = seen.get("uniforms", 0) + 1
        return uniform(a, b)

    random.seed(seed)
    np.random.seed(seed)
    rows, outs, attempts = [], [], []
    torch.nn.functional.interpolate, tr._get_param_spatial_crop = rec_interpolate, rec_get_param
    tr.random_crop, tr.uniform_crop, tr.horizontal_flip = rec_crop(random_crop), rec_crop(uniform_crop), rec_hflip
    random.uniform = counting_uniform
    try:
        for n, frames in enumerate(case_frames(data_seed, T, sizes)):
            seen.clear()
            h, w = sizes[n]
            x = ut.tensor_normalize(frames, MEAN, STD).permute(3, 0, 1, 2)
            y = ut.spatial_sampling(x, spatial_idx=-1 if idxs is None else idxs[n], **args)
            assert tuple(y.shape) == (3, T, S, S), tuple(y.shape)
            win = seen.get("win", (0, 0, h, w))
            res = seen.get("res", (h, w))
            rows.append([h, w, win[0], win[1], win[2], win[3], res[0], res[1]] + list(seen.get("off", (0, 0)))
                        + [seen.get("flip", 0)])
            outs.append(y.contiguous())
            attempts.append(seen.get("uniforms", 0) // 2)
    finally:
        torch.nn.functional.interpolate, tr._get_param_spatial_crop = interpolate, get_param
        tr.random_crop, tr.uniform_crop, tr.horizontal_flip = random_crop, uniform_crop, hflip
        random.uniform = uniform
    return rows, torch.stack(outs, 0), random.random(), float(np.random.uniform()), attempts


def search(tr, ut, kind, args, T, sizes, idxs, data_seed):
    for seed in range(4000):
        rows, _, _, _, attempts = run_reference(tr, ut, args, T, sizes, idxs, seed, data_seed)
        r = rows[0]
        if kind == "offsets_zero" and r[6] > S and r[7] > S and r[8] == 0 and r[9] == 0:
            return seed
        if kind == "resized" and r[6] != r[0]:
            return seed
        if kind == "offsets_max" and r[6] != r[0] and r[6] > S + 1 and r[7] > S + 1 and r[8] == r[6] - S - 1 and r[9] == r[7] - S - 1:
            return seed
        if kind == "flip_on" and r[10] == 1:
            return seed
        if kind == "flip_off" and r[10] == 0:
            return seed
        if kind == "inside" and r[2] > 0 and r[3] > 0 and r[2] + r[4] < r[0] and r[3] + r[5] < r[1]:
            return seed
        if kind == "retry" and 1 < attempts[0] < 10:
            return seed
    raise SystemExit("no seed in 0..3999 gives a %r case" % kind)


def main():
    tr, ut = load_reference()
    cases = []
    for i, (name, args, T, sizes, idxs, seed) in enumerate(CASES):
        data_seed = 3000 + i
        if isinstance(seed, str):
            seed = search(tr, ut, seed, args, T, sizes, idxs, data_seed)
        rows, out, py_after, np_after, attempts = run_reference(tr, ut, args, T, sizes, idxs, seed, data_seed)
        shift = float((out[..., 1:] - out[..., :-1]).abs().mean())
        cases.append({"name": name, "args": args, "seed": seed, "data_seed": data_seed, "T": T, "sizes": [list(s) for s in sizes],
                      "spatial_idx": idxs, "rows": rows, "py_after": repr(py_after), "np_after": repr(np_after),
                      "shift_diff": shift, "out": base64.b64encode(out.numpy().astype("<f4").tobytes()).decode("ascii")})
        print(i, name, "seed", seed, "rows", rows, "attempts", attempts, "shift %.3f" % shift)
    doc = {"torch_version": torch.__version__, "crop_size": S, "mean": MEAN, "std": STD, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
