"""Microbenchmark of RandAugment on the device (csrc/sf_randaug.h) at the MViTv2-S loader's shape: uint8 (8, 16, 256, 340, 3)
decoded frames, four layers (``rand-m7-n4-mstd0.5-inc1``).  HIP-event timed with COLD operands: every call works on the next of
several source / destination pairs whose sum exceeds the 256 MiB Infinity Cache (the rotation of
tools/spatial_sampling_bench.py); the ping-pong scratch is one buffer and stays where the previous call left it.
  all_table      four lookup-table layers per sample, three of them with a histogram (Equalize, Contrast, AutoContrast)
  all_bicubic    four affine layers per sample (Rotate, ShearX, ShearY, TranslateXRel), bicubic
  recipe         the recipe's own draw under seed 0: ``RandAugment("rand-m7-n4-mstd0.5-inc1").sample_batch(8)``
Every entry is ``rand_augment_clip`` as a loader calls it: the table checked, packed and uploaded per call.  Bytes are the
algorithm's (computed from the shapes), not counters: a layer reads and writes the frames once, a histogram pass reads them
once more.  Needs the GPU; there is no CPU fallback of the product path.

``--cpu`` times the numpy restatement of the same rules (tests/rand_augment_checks.py:restate_clip, no PIL) on ONE clip of the
same shape instead: what a host loop of that arithmetic costs, not what PIL costs.
`python tools/rand_augment_bench.py [--cpu] [--batch B] [--iters N] [--rounds R] [--out profiles/rand_augment_bench.json]`"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from slowfast_amd import rand_augment as ra

RECIPE = "rand-m7-n4-mstd0.5-inc1"


def tables(B):
    tab = [[(ra.EQUALIZE, False, 0.0), (ra.CONTRAST, False, 1.4 - 0.1 * (n % 3)), (ra.SOLARIZE_ADD, False, 40 + n),
            (ra.AUTO_CONTRAST, False, 0.0)] for n in range(B)]
    cub = [[(ra.ROTATE, False, 17.0 - 3 * n), (ra.SHEAR_X, False, 0.2), (ra.SHEAR_Y, False, -0.2), (ra.TRANSLATE_X_REL, False, 0.2)]
           for n in range(B)]
    np.random.seed(0)
    random.seed(0)
    return {"all_table": ra.make_table(tab), "all_bicubic": ra.make_table(cub), "recipe": ra.RandAugment(RECIPE).sample_batch(B)}


def layer_bytes(table, frame_bytes):
    hist = sum(bool(np.any(~table.skip[:, l] & np.isin(table.ops[:, l], ra.HIST_OPS))) for l in range(table.ops.shape[1]))
    return (2.0 * table.ops.shape[1] + hist) * frame_bytes


def entry(samples, nbytes):
    med = statistics.median(samples)
    return {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2),
            "bytes": int(nbytes), "TBps": round(nbytes / med / 1e6, 3)}


def describe(table, n=None):
    """The ops of sample n (all samples: joined with " | ") as one string."""
    rows = [", ".join(("skip " if s else "") + ra.OP_NAMES[o] for o, s in zip(table.ops[k], table.skip[k])) for k in range(len(table.ops))]
    return " | ".join(rows) if n is None else rows[n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, H, W = a.batch, a.frames, a.height, a.width
    tabs = tables(B)
    if a.cpu:
        from tests.rand_augment_checks import restate_clip
        g = np.random.RandomState(0)
        clip = g.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
        entries = {}
        for k, tab in tabs.items():
            t0 = time.perf_counter()
            restate_clip(clip, list(zip(tab.ops[0], tab.skip[0], tab.args[0])), tab.filter)
            entries[k] = {"seconds_per_clip": round(time.perf_counter() - t0, 3), "ops": describe(tab, 0)}
        res = {"mode": "cpu: numpy restatement, one clip", "clip": [T, H, W, 3], "entries": entries}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("rand_augment_bench needs the GPU (--cpu times the host-side restatement)")
        dev = torch.device("cuda:0")
        frame_bytes = 3.0 * B * T * H * W
        nset = max(2, int(600e6 // (2 * frame_bytes)) + 1)
        src = [torch.randint(0, 256, (B, T, H, W, 3), device=dev, dtype=torch.uint8) for _ in range(nset)]
        dst = [torch.empty_like(s) for s in src]

        def timed(fns, iters):
            for f in fns:
                f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fns[i % len(fns)]()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / iters
        runs = {k: [lambda s=s, d=d, tab=tab: ra.rand_augment_clip(s, tab, out=d) for s, d in zip(src, dst)] for k, tab in tabs.items()}
        samples = {k: [] for k in runs}
        for _ in range(a.rounds):                              # alternate the variants inside every round
            for k, fns in runs.items():
                samples[k].append(timed(fns, a.iters))
        res = {"mode": "gpu", "frames": [B, T, H, W, 3], "recipe": RECIPE, "buffer_sets": nset, "iters": a.iters, "rounds": a.rounds,
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
               "note": "bytes = the frames read and written once per layer, read once more by every histogram pass; the time "
                       "includes packing and uploading the table",
               "recipe_ops": describe(tabs["recipe"]),
               "entries": {k: entry(samples[k], layer_bytes(tabs[k], frame_bytes)) for k in runs}}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
