"""Microbenchmark of the spatial-sampling entry points (csrc/sf_sample.h; the pack_u8 rows are specialisations of
sf_pack_clip_kernel, csrc/sf_pack.h): uint8 (8, 16, 256, 340, 3) decoded frames -> 224 x 224,
short-side jitter to 288 (288 x 382 resized), crop at an unaligned offset, every other sample flipped.  HIP-event timed with COLD
operands: every call works on the next of several buffer sets whose sum exceeds the 256 MiB Infinity Cache (the rotation of
tools/random_erasing_bench.py):
  sample_clip_kernel   sf_sample_clip_u8, table already on the device     uint8 frames -> dense fp32 (N, 3, T, S, S)
  sample_clip          spatial_sampling.sample_clip: the same with the table packed and uploaded per call
  pack_u8_sample       pack_pathways_u8(crop=): uint8 frames -> 16-bit W-pair clip, sampled while packing
                       (sf_pack_clip_u8_sample: sf_pack_clip_kernel<PackSampled, true, true>)
  pack_u8_sample_aug   the same with an erase table (pixel mode) and mixup
  pack_u8              sf_pack_clip_u8 on frames that are already 224 x 224 (what the sampling is added to)
  torch_sample         the yardstick: the normalised fp32 clip is already on the device; per sample F.interpolate (bilinear,
                       align_corners=False) + slice + flip into the output -- the reference's arithmetic, and it does not
                       include the normalisation the kernels above do
Bytes are the algorithm's (computed from the shapes: the source rows the crop touches are not subtracted), not counters.  Needs
the GPU; there is no CPU fallback.
`python tools/spatial_sampling_bench.py [--batch B] [--iters N] [--rounds R] [--out profiles/spatial_sampling_bench.json]`"""
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
from slowfast_amd import spatial_sampling as ss
from slowfast_amd.lib import get_lib
from slowfast_amd.mixup import MixParams


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


def torch_sample(clip, rows, S, out):
    for n, (_, _, wy, wx, wh, ww, rh, rw, oy, ox, flip) in enumerate(rows):
        x = torch.nn.functional.interpolate(clip[n, :, :, wy:wy + wh, wx:wx + ww], size=(rh, rw), mode="bilinear",
                                            align_corners=False)[:, :, oy:oy + S, ox:ox + S]
        out[n] = x.flip(-1) if flip else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_sampling_bench needs the GPU")
    dev = torch.device("cuda:0")
    B, T, H, W, S = a.batch, a.frames, a.height, a.width, a.crop
    size = S + S // 7 * 2                                           # 288 for 224
    rh, rw = ss.SpatialSampling._jitter_size(H, W, size)
    table = ss.make_table([(H, W, 0, 0, H, W, rh, rw, (rh - S) // 3 + n, (rw - S) // 2 + 3 * n + 1, n % 2) for n in range(B)], S)
    cfg = sa.get_preset("MVITv2_S_16x4", ["NUM_GPUS", 1, "DATA.NUM_FRAMES", T, "DATA.TRAIN_CROP_SIZE", S])
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD
    src_b, f32_b, pk_b = 3.0 * B * T * H * W, 12.0 * B * T * S * S, 8.0 * B * T * S * S
    nset = max(2, int(600e6 // (src_b + f32_b)) + 1)
    frames = [torch.randint(0, 256, (B, T, H, W, 3), device=dev, dtype=torch.uint8) for _ in range(nset)]
    outs = [torch.empty((B, 3, T, S, S), device=dev) for _ in range(nset)]
    packed = [sa.pack_pathways_u8(f, cfg, crop=table) for f in frames]
    nset_t = max(2, int(600e6 // (4.0 * src_b + f32_b)) + 1)
    clips = [torch.randn((B, 3, T, H, W), device=dev) for _ in range(nset_t)]
    nset_c = max(2, int(600e6 // (11.0 * B * T * S * S)) + 1)
    cropped = [torch.randint(0, 256, (B, T, S, S, 3), device=dev, dtype=torch.uint8) for _ in range(nset_c)]
    cropped_out = [sa.pack_pathways_u8(f, cfg) for f in cropped]
    erase = re_.make_table([(i, 0, T, S // 6, S // 4 - 5, S // 2, S // 2) for i in range(B)], "pixel", (T, 3, S, S),
                           keys=[0x9E3779B97F4A7C15 * (i + 1) % 2 ** 64 for i in range(B)])
    mix = MixParams(0.3, False, None)
    host, devtab = ss.upload_table(table, B, dev)
    stream = ops._stream(frames[0])
    m, s = [float(v) for v in mean], [float(v) for v in std]

    def kernel_only(f, o):
        get_lib().call("sf_sample_clip_u8", f.data_ptr(), B, T, H, W, host.ctypes.data, devtab.data_ptr(), S, m[0], m[1], m[2],
                       s[0], s[1], s[2], o.data_ptr(), stream)

    rows = table.rows.tolist()
    pix = B * T * S * S
    runs = {
        "sample_clip_kernel": ([lambda f=f, o=o: kernel_only(f, o) for f, o in zip(frames, outs)], src_b + f32_b),
        "sample_clip": ([lambda f=f, o=o: ss.sample_clip(f, table, mean, std, out=o) for f, o in zip(frames, outs)], src_b + f32_b),
        "pack_u8_sample": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o, crop=table) for f, o in zip(frames, packed)],
                           src_b + pk_b),
        "pack_u8_sample_aug": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o, crop=table, erase=erase, mix=mix)
                                for f, o in zip(frames, packed)], src_b + pk_b),
        "pack_u8": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o) for f, o in zip(cropped, cropped_out)], 11.0 * pix),
        "torch_sample": ([lambda c=c, i=i: torch_sample(c, rows, S, outs[i % len(outs)]) for i, c in enumerate(clips)],
                         4.0 * src_b + f32_b),
    }
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):                                  # alternate the variants inside every round
        for k, (fns, _) in runs.items():
            samples[k].append(timed(fns, a.iters))
    res = {"frames": [B, T, H, W, 3], "resized": [rh, rw], "crop": S, "buffer_sets": nset, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "note": "bytes = the whole source buffer + the output (the rows outside the crop are not subtracted); torch_sample "
                   "reads an already normalised fp32 clip (4 x the source bytes) and launches per sample",
           "entries": {k: entry(samples[k], runs[k][1]) for k in runs}}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
