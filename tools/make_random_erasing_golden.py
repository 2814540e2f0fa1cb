"""Records tests/golden/random_erasing_contract.json from the UNMODIFIED reference's slowfast/datasets/random_erasing.py.  Build
container only (needs the reference tree).

    python tools/make_random_erasing_golden.py

The module is loaded BY FILE PATH (the ``slowfast.datasets`` package around it imports decoders that are not installed; the
file itself needs torch only).  Per case (constructor arguments, ``random.seed`` / ``torch.manual_seed`` values, N, the
(T, C, H, W) geometry): N clips are drawn from a seeded torch.Generator (the test draws them again), the reference's
RandomErasing(device="cpu") is called on them in order, and the fixture keeps

* ``const`` / ``rand`` modes: the reference's output, float32 little-endian bytes in base64, layout (N, T, C, H, W);
* ``pixel`` mode: the set of elements the reference changed, as per-frame boxes [n, t, top, left, h, w] (all channels);
* ``random.random()`` and ``torch.rand(1)`` drawn right after the call: how far each generator was consumed.

Some cases are found by a search over seeds (a draw that retries, one that gives up, one that erases nothing, overlapping
boxes); what the search looks at is the reference's own behaviour: its output, the number of ``random.uniform`` calls it made
and the patch sizes it asked ``_get_pixels`` for.  Recorded results only: no reference program text goes into the fixture or
this tool.
"""
import base64
import importlib.util
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("SLOWFAST_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "random_erasing_contract.json")

G0 = (4, 3, 12, 10)         # (T, C, H, W)
ALWAYS = dict(probability=1.0)

# (name, constructor arguments, geometry, N, seed or the name of a search over seeds 0..199)
CASES = [
    ("const", dict(ALWAYS, mode="const"), G0, 1, 0),
    ("rand", dict(ALWAYS, mode="rand"), G0, 1, 1),
    ("pixel", dict(ALWAYS, mode="pixel"), G0, 1, 2),
    ("const, clean first half", dict(ALWAYS, mode="const", max_count=2, num_splits=2), G0, 1, 3),
    ("rand, clean first half", dict(ALWAYS, mode="rand", max_count=2, num_splits=2), G0, 1, 4),
    ("pixel, clean first half", dict(ALWAYS, mode="pixel", max_count=2, num_splits=2), G0, 1, 5),
    ("retries (h >= H rejected)", dict(ALWAYS, mode="const"), (4, 3, 6, 20), 1, "retry"),
    ("retries, pixel", dict(ALWAYS, mode="pixel"), (4, 3, 6, 20), 1, "retry"),
    ("p 0.25: erased", dict(probability=0.25, mode="pixel", max_count=3, num_splits=3), (2, 3, 14, 18), 1, "erased"),
    ("p 0.25: not erased", dict(probability=0.25, mode="pixel", max_count=3, num_splits=3), (2, 3, 14, 18), 1, "clean"),
    ("p 0.25: erased, const", dict(probability=0.25, mode="const", max_count=3, num_splits=3), (2, 3, 14, 18), 1, "erased"),
    # a 4 x 4 frame and boxes of 70-100 % of it: h < 4 and w < 4 only for a sliver of the (area, aspect) draws
    ("attempts exhausted", dict(ALWAYS, mode="const", min_area=0.7, max_area=1.0), (4, 3, 4, 4), 1, "exhausted"),
    ("attempts nearly exhausted", dict(ALWAYS, mode="rand", min_area=0.7, max_area=1.0), (4, 3, 4, 4), 1, "retry"),
    ("per frame, rand", dict(ALWAYS, mode="rand", cube=False), G0, 1, 6),
    ("per frame, pixel, two boxes", dict(ALWAYS, mode="pixel", cube=False, min_count=2), G0, 1, 7),
    ("per frame, p 0.5, const", dict(probability=0.5, mode="const", cube=False), G0, 1, 8),
    ("three overlapping boxes, rand", dict(ALWAYS, mode="rand", min_count=3, max_area=0.9), G0, 1, "overlap"),
    ("N 3, rand", dict(probability=0.6, mode="rand", max_count=2), (2, 3, 14, 18), 3, 9),
    ("N 3, pixel", dict(probability=0.6, mode="pixel", max_count=2), G0, 3, 10),
    ("N 3, per frame, const", dict(probability=0.6, mode="const", cube=False, max_count=2), G0, 3, 11),
]


def load_reference():
    path = os.path.join(REFERENCE_ROOT, "slowfast", "datasets", "random_erasing.py")
    spec = importlib.util.spec_from_file_location("reference_random_erasing", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_input(data_seed, N, geom):
    """The N input clips of a case, (N, T, C, H, W) (tests/random_erasing_checks.py draws the same)."""
    return torch.randn((N,) + tuple(geom), generator=torch.Generator().manual_seed(data_seed))


def run_reference(ref, args, geom, N, seed, data_seed):
    """The reference on the case's clips, in order.  Returns (input, output, random.random() after, torch.rand(1) after,
    number of random.uniform calls, patch sizes asked of _get_pixels)."""
    x = case_input(data_seed, N, geom)
    y = x.clone()
    fn = ref.RandomErasing(device="cpu", **args)
    calls, patches = [0], []
    uniform, get_pixels = random.uniform, ref._get_pixels

    def counting_uniform(a, b):
        calls[0] += 1
        return uniform(a, b)

    def recording_get_pixels(per_pixel, rand_color, patch_size, **kw):
        patches.append(tuple(int(v) for v in patch_size))
        return get_pixels(per_pixel, rand_color, patch_size, **kw)

    random.seed(seed)
    torch.manual_seed(seed)
    random.uniform, ref._get_pixels = counting_uniform, recording_get_pixels
    try:
        for n in range(N):
            fn(y[n])
    finally:
        random.uniform, ref._get_pixels = uniform, get_pixels
    return x, y, random.random(), float(torch.rand(1)), calls[0], patches


def changed_boxes(x, y):
    """Elements whose bits changed, as per-frame boxes [n, t, top, left, h, w]: runs of changed columns per line, merged over
    consecutive lines with the same run.  Asserts that a changed pixel changed in every channel."""
    diff = (x.view(torch.int32) != y.view(torch.int32))
    assert torch.equal(diff.any(2), diff.all(2)), "a pixel changed in some channels only"
    mask = diff.any(2).numpy()                  # (N, T, H, W)
    boxes = []
    for n in range(mask.shape[0]):
        for t in range(mask.shape[1]):
            open_runs = {}                      # (left, w) -> index into boxes of the box that ended on the previous line
            for yy in range(mask.shape[2]):
                line, runs, xx = mask[n, t, yy], [], 0
                while xx < len(line):
                    if line[xx]:
                        x0 = xx
                        while xx < len(line) and line[xx]:
                            xx += 1
                        runs.append((x0, xx - x0))
                    else:
                        xx += 1
                nxt = {}
                for run in runs:
                    if run in open_runs:
                        boxes[open_runs[run]][4] += 1
                        nxt[run] = open_runs[run]
                    else:
                        boxes.append([n, t, yy, run[0], 1, run[1]])
                        nxt[run] = len(boxes) - 1
                open_runs = nxt
    return boxes


def search(ref, kind, args, geom, N, data_seed):
    for seed in range(200):
        x, y, _, _, uniforms, patches = run_reference(ref, args, geom, N, seed, data_seed)
        changed = not torch.equal(x.view(torch.int32), y.view(torch.int32))
        T = geom[0]
        if kind == "retry" and changed and uniforms > 2:
            return seed
        if kind == "erased" and changed:
            return seed
        if kind == "clean" and not changed and uniforms == 0:
            return seed
        if kind == "exhausted" and not changed and uniforms == 200:
            return seed
        if kind == "overlap" and changed:
            per_frame = sum(h * w for _, h, w in patches) // T          # cube: every box is assigned once per frame
            boxes = changed_boxes(x, y)
            if sum(b[4] * b[5] for b in boxes if b[1] == 0) < per_frame:
                return seed
    raise SystemExit("no seed in 0..199 gives a %r case" % kind)


def main():
    ref = load_reference()
    cases = []
    for i, (name, args, geom, N, seed) in enumerate(CASES):
        data_seed = 2000 + i
        if isinstance(seed, str):
            seed = search(ref, seed, args, geom, N, data_seed)
        x, y, py_after, torch_after, uniforms, patches = run_reference(ref, args, geom, N, seed, data_seed)
        case = {"name": name, "args": args, "seed": seed, "data_seed": data_seed, "N": N, "shape": list(geom),
                "py_after": repr(py_after), "torch_after": repr(torch_after), "boxes": changed_boxes(x, y)}
        if args["mode"] != "pixel":
            case["out"] = base64.b64encode(y.contiguous().numpy().astype("<f4").tobytes()).decode("ascii")
        cases.append(case)
        print(i, name, "seed", seed, "uniform calls", uniforms, "assignments", len(patches), "boxes", len(case["boxes"]))
    doc = {"torch_version": torch.__version__, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
