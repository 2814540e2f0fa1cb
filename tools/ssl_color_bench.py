"""Microbenchmark of the SSL colour augmentation on the device (csrc/sf_sslcolor.h) at the contrastive recipes' loader shape: uint8
(32, 8, 256, 340, 3) after decode, rotating through enough buffer sets (> 600 MB) that every call finds its frames in HBM, not in
a cache.

  recipe          the MoCo-v2 draw under seed 0: ``SslColorJitter([0.6] * 3, 0.15, 0.2, True).sample_batch(32)``
  brightness      every clip draws brightness only: the streaming pass alone
  jitter          every clip draws all four ops, contrast third: the histogram pass and the streaming pass
  grey            every clip is converted to grey: the streaming pass alone
  blur            every clip is blurred (sigma 1.0) and nothing else: the streaming pass copies, then the row and the column pass

Every entry is ``ssl_color_clip`` as a loader calls it (``out`` given): the table checked, packed and uploaded per call.  ``passes``
times the recipe's passes one by one with a pair of events around each library call.  Bytes are what a pass must move: the
histogram pass reads the clips that drew contrast, the streaming pass reads and writes every clip, a blur pass reads and writes
the clips that drew the blur.  ``pil`` is the PIL restatement of the same draw (tools/make_ssl_color_golden.py:pil_clip) for the
same batch on one CPU core, the reference's loader-side cost.

`python tools/ssl_color_bench.py [--no-pil] [--batch B] [--iters N] [--rounds R] [--out profiles/ssl_color_bench.json]`"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from slowfast_amd import lib as sflib
from slowfast_amd import ssl_color as sc

RECIPE = dict(bri_con_sat=[0.6, 0.6, 0.6], hue=0.15, p_convert_gray=0.2, moco_v2_aug=True)
PASSES = ("sf_sslcolor_hist_u8", "sf_sslcolor_stream_u8", "sf_sslcolor_blur_rows_u8", "sf_sslcolor_blur_cols_u8")


def tables(B):
    def row(order=(0, 1, 2, 3), b=None, c=None, s=None, hue=None, gray=False, sigma=None, jitter=True):
        return sc.SslRow(jitter, order, b, c, s, hue, gray, sigma)
    torch.manual_seed(0)
    random.seed(0)
    return {"recipe": sc.SslColorJitter(**RECIPE).sample_batch(B),
            "brightness": sc.SslTable(tuple(row(b=0.7 + 0.02 * n) for n in range(B)), False),
            "jitter": sc.SslTable(tuple(row((0, 2, 1, 3), 0.7 + 0.02 * n, 1.3, 0.8, 0.1) for n in range(B)), False),
            "grey": sc.SslTable(tuple(row(jitter=False, gray=True) for n in range(B)), False),
            "blur": sc.SslTable(tuple(row(jitter=False, sigma=1.0) for n in range(B)), False)}


def pass_bytes(table, clip_bytes):
    """Bytes each pass must move for the table: {pass: bytes} (a pass that is not launched is left out)."""
    rows = sc.pack_words(table, [(1, 1)] * len(table.rows)).reshape(-1, sc.ROW_WORDS)
    hist = sum(sc._needs_hist(r) for r in rows)
    blur = int(np.sum((rows[:, 0] & sc.FLAG_BLUR) != 0))
    out = {}
    if hist:
        out[PASSES[0]] = 1.0 * hist * clip_bytes
    if np.any(rows[:, 0] & (sc.FLAG_JITTER | sc.FLAG_GREY | sc.FLAG_BLUR)):
        out[PASSES[1]] = 2.0 * len(rows) * clip_bytes
    if blur:
        out[PASSES[2]] = out[PASSES[3]] = 2.0 * blur * clip_bytes
    return out


def entry(samples, nbytes):
    med = statistics.median(samples)
    return {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2),
            "bytes": int(nbytes), "TBps": round(nbytes / med / 1e6, 3)}


def describe(table):
    return " | ".join("%s%s%s" % ("jitter " + "".join("bcsh"[o] for o in r.order) if r.jitter else "-", " grey" if r.gray else "",
                                  " blur %.2f" % r.sigma if r.sigma is not None else "") for r in table.rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-pil", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, H, W = a.batch, a.frames, a.height, a.width
    if not torch.cuda.is_available():
        raise SystemExit("ssl_color_bench needs the GPU")
    tabs = tables(B)
    dev = torch.device("cuda:0")
    clip_bytes = 3.0 * T * H * W
    nset = max(2, int(600e6 // (2 * B * clip_bytes)) + 1)
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
    runs = {k: [lambda s=s, d=d, tab=tab: sc.ssl_color_clip(s, tab, out=d) for s, d in zip(src, dst)] for k, tab in tabs.items()}
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):                               # alternate the variants inside every round
        for k, fns in runs.items():
            samples[k].append(timed(fns, a.iters))
    # the recipe's passes one by one: a pair of events around every library call
    events = []

    def observer(name, thunk, work):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = thunk()
        e1.record()
        events.append((name, e0, e1))
        return rc
    sflib.set_call_observer(observer)
    try:
        for i in range(a.rounds * a.iters):
            runs["recipe"][i % nset]()
    finally:
        sflib.set_call_observer(None)
    torch.cuda.synchronize()
    per_pass = {}
    for name, e0, e1 in events:
        per_pass.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    recipe_bytes = pass_bytes(tabs["recipe"], clip_bytes)
    res = {"mode": "gpu", "frames": [B, T, H, W, 3], "recipe": RECIPE, "buffer_sets": nset, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "note": "bytes = what the launched passes must move (see the module docstring); an entry's time includes checking, "
                   "packing and uploading the table; 'passes' are the recipe's library calls between two events each",
           "recipe_rows": describe(tabs["recipe"]),
           "entries": {k: entry(samples[k], sum(pass_bytes(tabs[k], clip_bytes).values())) for k in runs},
           "passes": {name: entry(per_pass[name], recipe_bytes[name]) for name in PASSES if name in per_pass}}
    if not a.no_pil:
        from make_ssl_color_golden import pil_clip
        torch.set_num_threads(1)
        clips = src[0].cpu().numpy()
        t0 = time.perf_counter()
        for n in range(B):
            pil_clip(clips[n], tabs["recipe"].rows[n], tabs["recipe"].gray_first)
        res["pil"] = {"seconds_per_batch": round(time.perf_counter() - t0, 3), "what": "PIL on one CPU core, the recipe's draw, %d clips" % B}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
