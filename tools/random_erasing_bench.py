"""Microbenchmark of the random-erasing entry points (csrc/sf_erase.h; the pack_u8 rows are specialisations of
sf_pack_clip_kernel, csrc/sf_pack.h) at an (8, 3, 16, 224, 224) batch, `pixel` mode, one
112 x 112 box (a quarter of the frame, unaligned corner) over all frames of every sample.  HIP-event timed with COLD operands:
every call works on the next of several batches whose sum exceeds the 256 MiB Infinity Cache (the rotation of
tools/mixup_bench.py):
  erase_inplace_kernel   sf_erase_clip_f32 in place, table already on the device   (writes 4 bytes per erased element)
  erase_inplace          random_erasing.erase_clip: the same with the table packed and uploaded per call
  erase_copy             erase_clip(out=): every element read once and written once
  torch_erase            the yardstick: x[n, :, t, top:top+h, left:left+w] = normal_() per frame on the same device
  pack_u8                sf_pack_clip_u8      uint8 frames -> 16-bit W-pair clip
  pack_u8_erase          sf_pack_clip_u8_aug  the same with the erase table
Bytes are the algorithm's (computed from the shapes), not counters.  Needs the GPU; there is no CPU fallback.
`python tools/random_erasing_bench.py [--batch B] [--iters N] [--rounds R] [--out profiles/random_erasing_bench.json]`"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import slowfast_amd as sa
from slowfast_amd import ops
from slowfast_amd import random_erasing as re_
from slowfast_amd.lib import get_lib


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


def entry(samples, nbytes):
    med = statistics.median(samples)
    return {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2),
            "bytes": int(nbytes), "TBps": round(nbytes / med / 1e6, 3)}


def torch_erase(x, table):
    C = x.shape[1]
    for n, t0, t1, top, left, h, w in table.rows.tolist():
        for t in range(t0, t1):
            x[n, :, t, top:top + h, left:left + w] = torch.empty((C, h, w), dtype=x.dtype, device=x.device).normal_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("random_erasing_bench needs the GPU")
    dev = torch.device("cuda:0")
    B, T, S = a.batch, a.frames, a.crop
    shape = (B, 3, T, S, S)
    n = B * 3 * T * S * S
    nset = max(2, int(600e6 // (4.0 * n)) + 1)
    clips = [torch.randn(shape, device=dev) for _ in range(nset)]
    outs = [torch.empty(shape, device=dev) for _ in range(2)]
    cfg = sa.get_preset("MVITv2_S_16x4", ["NUM_GPUS", 1, "DATA.NUM_FRAMES", T, "DATA.TRAIN_CROP_SIZE", S])
    nset_u8 = max(2, int(600e6 // (11.0 * B * T * S * S)) + 1)     # 3 bytes in + 8 bytes out per pixel
    frames = [torch.randint(0, 256, (B, T, S, S, 3), device=dev, dtype=torch.uint8) for _ in range(nset_u8)]
    packed = [sa.pack_pathways_u8(f, cfg) for f in frames]
    h = w = S // 2
    top, left = S // 6, S // 4 - 5
    table = re_.make_table([(i, 0, T, top, left, h, w) for i in range(B)], "pixel", (T, 3, S, S),
                           keys=[0x9E3779B97F4A7C15 * (i + 1) % 2 ** 64 for i in range(B)])
    erased = B * 3 * T * h * w
    host, devtab, R = re_.upload_table(table, B, dev)
    stream = ops._stream(clips[0])

    def kernel_only(c):
        get_lib().call("sf_erase_clip_f32", c.data_ptr(), c.data_ptr(), B, 3, T, S, S, re_.MODES["pixel"], host.ctypes.data,
                       devtab.data_ptr(), R, int(host.size), stream)

    pix = B * T * S * S
    runs = {
        "erase_inplace_kernel": ([lambda c=c: kernel_only(c) for c in clips], 4.0 * erased),
        "erase_inplace": ([lambda c=c: re_.erase_clip(c, table) for c in clips], 4.0 * erased),
        "erase_copy": ([lambda c=c, i=i: re_.erase_clip(c, table, out=outs[i % 2]) for i, c in enumerate(clips)], 8.0 * n),
        "torch_erase": ([lambda c=c: torch_erase(c, table) for c in clips], 4.0 * erased),
        "pack_u8": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o) for f, o in zip(frames, packed)], 3.0 * pix + 8.0 * pix),
        "pack_u8_erase": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o, erase=table) for f, o in zip(frames, packed)],
                          3.0 * pix + 8.0 * pix),
    }
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):                                  # alternate the variants inside every round
        for k, (fns, _) in runs.items():
            samples[k].append(timed(fns, a.iters))
    res = {"clip": list(shape), "clip_bytes": 4 * n, "box": [top, left, h, w], "erased_elements": erased, "buffer_sets": nset,
           "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "note": "bytes = what the algorithm must move; torch_erase carries the same bytes as erase_inplace, so its TBps is "
                   "the useful rate, not the traffic of its B*T normal_() + slice-assign launches",
           "entries": {k: entry(samples[k], runs[k][1]) for k in runs}}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
