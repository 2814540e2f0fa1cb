"""Microbenchmark of the grouped (1,3,3) convolutions (csrc/sf_gconv.h) at the conv-b shapes of ResNeXt-50 32x4d and 32x8d as a Slow
backbone (8 frames, 224 crop, batch 8): forward (with statistics), data gradient, weight gradient and the weight packing, HIP-event
timed with COLD operands (the calls rotate through enough buffer sets to exceed the 256 MiB Infinity Cache, as tools/dw_bench.py
does), against two yardsticks measured in the same run on the same tensors:
  torch   torch's own grouped conv3d forward / convolution_backward (channels-last, the storage type): what a user gets without
          the feature;
  dense   the engine's dense sf_conv_* on the same channel count: the same activation bytes at G times the real MACs, i.e. what
          the bundle scheme could reach if the block-diagonal zeros cost nothing and nothing else did.
Bytes/s are stated against the ``work=`` accounting of ops.gconv_* (activation bytes that must cross HBM once).
`python tools/gconv_bench.py [--iters N] [--out profiles/resnext_bench.json] [--only 32x4d|32x8d] [--no-torch]`"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from slowfast_amd import lib, ops

# (stage, channels per group multiplier, spatial size of the stage input, stride): b of the first block of res3..res5 strides
STAGES = [("res2", 1, 56, 1), ("res3.0", 2, 56, 2), ("res3", 2, 28, 1), ("res4.0", 4, 28, 2), ("res4", 4, 14, 1), ("res5.0", 8, 14, 2),
          ("res5", 8, 7, 1)]
MODELS = {"32x4d": (32, 4), "32x8d": (32, 8)}


def timed(fns, iters):
    for f in fns:
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fns[i % len(fns)]()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def layer(name, G, Cg, hw, stride, batch, frames, iters, dev, with_torch):
    f16 = lib.act_dtype()
    C = G * Cg
    shape = (batch, C, frames, hw, hw)
    geom = ops.GroupedConvGeom(shape, G, (1, 3, 3), (1, stride, stride), (0, 1, 1), 1)
    dense = ops.ConvGeom(shape, C, (1, 3, 3), (1, stride, stride), (0, 1, 1), 1)
    g = torch.Generator().manual_seed(0)
    by_in, by_out = 2.0 * C * batch * frames * hw * hw, 2.0 * C * geom.out_rows
    nset = max(2, int(400e6 // (by_in + by_out)) + 1)
    x0 = torch.randn(shape, generator=g).to(f16).to(dev).contiguous(memory_format=torch.channels_last_3d)
    dy0 = torch.randn(geom.out_shape, generator=g).to(f16).to(dev).contiguous(memory_format=torch.channels_last_3d)
    xs, dys = [x0.clone(memory_format=torch.preserve_format) for _ in range(nset)], [dy0.clone(memory_format=torch.preserve_format) for _ in range(nset)]
    w = (torch.randn((C, Cg, 1, 3, 3), generator=g) / (9 * Cg) ** 0.5).to(dev)
    wdense = (torch.randn((C, C, 1, 3, 3), generator=g) / (9 * C) ** 0.5).to(dev)
    dw, dwd = torch.empty_like(w), torch.empty_like(wdense)
    wf, wd = ops.gconv_prep_weights(w, geom)
    df, dd = ops.prep_weights(wdense, dense)
    ys, dxs = [ops.cl_empty(geom.out_shape, dev) for _ in range(nset)], [ops.cl_empty(shape, dev) for _ in range(nset)]
    res = {"C": C, "Cg": Cg, "groups": G, "input": list(shape), "stride": stride, "buffer_sets": nset, "us": {}, "work": {}}
    res["work"] = {"fwd": geom.work(reads_x=1, writes_y=1), "dgrad": geom.work(reads_y=1, writes_x=1), "wgrad": geom.work(reads_x=1, reads_y=1),
                   "prep": dict(bytes=4.0 * w.numel() + 4.0 * wf.numel(), flops=0.0)}
    us = res["us"]
    us["gconv"] = {
        "fwd": timed([(lambda x=x, y=y: ops.gconv_fwd(x, wf, geom, stats=True, out=y)) for x, y in zip(xs, ys)], iters),
        "dgrad": timed([(lambda dy=dy, dx=dx: ops.gconv_dgrad(dy, wd, geom, out=dx)) for dy, dx in zip(dys, dxs)], iters),
        "wgrad": timed([(lambda x=x, dy=dy: ops.gconv_wgrad(x, dy, geom, dw)) for x, dy in zip(xs, dys)], iters),
        "prep": timed([lambda: ops.gconv_prep_weights(w, geom)], iters)}
    us["dense"] = {
        "fwd": timed([(lambda x=x, y=y: ops.conv_fwd(x, df, dense, stats=True, out=y)) for x, y in zip(xs, ys)], iters),
        "dgrad": timed([(lambda dy=dy, dx=dx: ops.conv_dgrad(dy, dd, dense, out=dx)) for dy, dx in zip(dys, dxs)], iters),
        "wgrad": timed([(lambda x=x, dy=dy: ops.conv_wgrad(x, dy, dense, dwd)) for x, dy in zip(xs, dys)], iters),
        "prep": timed([lambda: ops.prep_weights(wdense, dense)], iters)}
    if with_torch:
        w16 = w.to(f16).contiguous(memory_format=torch.channels_last_3d)
        st, pd, dl = [1, stride, stride], [0, 1, 1], [1, 1, 1]
        try:
            bwd = torch.ops.aten.convolution_backward
            us["torch"] = {
                "fwd": timed([(lambda x=x: torch.nn.functional.conv3d(x, w16, None, st, pd, dl, G)) for x in xs], iters),
                "dgrad": timed([(lambda x=x, dy=dy: bwd(dy, x, w16, None, st, pd, dl, False, [0, 0, 0], G, [True, False, False]))
                                for x, dy in zip(xs, dys)], iters),
                "wgrad": timed([(lambda x=x, dy=dy: bwd(dy, x, w16, None, st, pd, dl, False, [0, 0, 0], G, [False, True, False]))
                                for x, dy in zip(xs, dys)], iters),
                "prep": timed([lambda: w.to(f16)], iters)}
        except Exception as e:                  # a yardstick that does not run is recorded as such, the rest of the table stands
            us["torch"] = {"error": repr(e)[:300]}
    gb = {k: res["work"][k]["bytes"] / us["gconv"][k] * 1e-3 for k in ("fwd", "dgrad", "wgrad")}
    res["gconv_GBps"] = gb
    t = us.get("torch", {})
    print("%-14s C=%4d Cg=%2d %3dx%-3d s%d | " % (name, C, Cg, hw, hw, stride) + " | ".join(
        "%s gconv %7.1f us (%4.0f GB/s) dense %7.1f torch %s" % (k, us["gconv"][k], gb[k], us["dense"][k],
                                                              ("%7.1f" % t[k]) if k in t else "   n/a") for k in ("fwd", "dgrad", "wgrad"))
          + " | prep %5.1f us" % us["gconv"]["prep"], flush=True)
    return res


def save(out, path):
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "act": lib.ACT_MODE, "batch": a.batch, "frames": a.frames, "crop": 224,
           "iters": a.iters, "torch_version": torch.__version__, "layers": {}}
    for model, (G, w0) in MODELS.items():
        if a.only and a.only != model:
            continue
        for stage, mult, hw, stride in STAGES:
            name = "%s %s b" % (model, stage)
            out["layers"][name] = layer(name, G, w0 * mult, hw, stride, a.batch, a.frames, a.iters, dev, not a.no_torch)
            save(out, a.out)
    slower = sorted({"%s %s" % (n, k) for n, r in out["layers"].items() for k in ("fwd", "dgrad", "wgrad")
                     if k in r["us"].get("torch", {}) and r["us"]["gconv"][k] > r["us"]["torch"][k]})
    out["slower_than_torch"] = slower
    print("entry points slower than torch's grouped convolution:", slower or "none")
    save(out, a.out)


if __name__ == "__main__":
    main()
