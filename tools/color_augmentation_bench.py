"""Microbenchmark of the colour-augmentation entry points (csrc/sf_color.h) on the dense fp32 (8, 3, 32, 224, 224) clip of the AVA
configuration, in place.  HIP-event timed with COLD operands: every call works on the next of several buffer sets whose sum
exceeds the 256 MiB Infinity Cache (the rotation of tools/spatial_sampling_bench.py):
  color_kernel_pca     sf_color_clip_f32, PCA lighting + normalisation + channel reversal, table already on the device
  color_kernel_all     sf_color_frame_means_f32 + sf_color_clip_f32, brightness / contrast / saturation in three different orders
  color_clip_pca       color_augmentation.color_clip: the first with the table checked, packed and uploaded per call
  color_clip_all       the same for the second
  sample_then_color    spatial_sampling.sample_clip (uint8 (8, 32, 256, 340, 3) -> 224, mean 0, std 1) + color_clip with all ops:
                       decoded frames -> model input, the extra round trip through the fp32 clip included
  sample_clip          the sampling alone (what the colour stage is added to)
  torch_color_pca      the yardsticks: the same arithmetic as torch operations on the device, sample by sample
  torch_color_all
Bytes are the algorithm's (computed from the shapes), not counters: the streaming pass reads and writes the clip once, the
reduction reads it once more.  Needs the GPU; there is no CPU fallback.
`python tools/color_augmentation_bench.py [--batch B] [--iters N] [--rounds R] [--out profiles/color_augmentation_bench.json]`"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from slowfast_amd import color_augmentation as ca
from slowfast_amd import ops
from slowfast_amd import spatial_sampling as ss
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


def torch_color(clip, rows, mean, std, reverse):
    """The arithmetic of csrc/sf_color.h as torch operations, in place, sample by sample."""
    for n, (order, alpha, add) in enumerate(rows):
        v = clip[n]
        for op, a in zip(order, alpha):
            if op == 0:
                v = v * a
                continue
            gray = 0.299 * v[2] + 0.587 * v[1] + 0.114 * v[0]
            other = gray.mean(dim=(1, 2), keepdim=True) if op == 1 else gray
            v = v * a + other * (1.0 - a)
        v = (v + add.view(3, 1, 1, 1) - mean.view(3, 1, 1, 1)) / std.view(3, 1, 1, 1)
        clip[n] = v.flip(0) if reverse else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("color_augmentation_bench needs the GPU")
    dev = torch.device("cuda:0")
    B, T, H, W, S = a.batch, a.frames, a.height, a.width, a.crop
    # factors close to 1 and mean 0 / std 1: the clips are jittered again and again in place and must stay finite
    orders = [(0, 1, 2), (2, 0, 1), (1, 2, 0)]
    rows_all = [(orders[n % 3], (1.01, 0.97, 1.02), (0.003, -0.002, 0.001)) for n in range(B)]
    rows_pca = [((), (), (0.003, -0.002, 0.001)) for n in range(B)]
    mean, std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    tab_all, tab_pca = ca.make_table(rows_all), ca.make_table(rows_pca)
    clip_b = 12.0 * B * T * S * S
    src_b = 3.0 * B * T * H * W
    nset = max(2, int(600e6 // clip_b) + 1)
    clips = [torch.rand((B, 3, T, S, S), device=dev) for _ in range(nset)]
    size = S + S // 7 * 2                                           # 288 for 224
    rh, rw = ss.SpatialSampling._jitter_size(H, W, size)
    crop = ss.make_table([(H, W, 0, 0, H, W, rh, rw, (rh - S) // 3 + n, (rw - S) // 2 + 3 * n + 1, n % 2) for n in range(B)], S)
    nset_f = max(2, int(600e6 // (src_b + clip_b)) + 1)
    frames = [torch.randint(0, 256, (B, T, H, W, 3), device=dev, dtype=torch.uint8) for _ in range(nset_f)]
    lib = get_lib()
    stream = ops._stream(clips[0])
    host_all, dev_all = ca.upload_table(tab_all, B, dev)
    host_pca, dev_pca = ca.upload_table(tab_pca, B, dev)
    partials = torch.empty((B * T, lib.call("sf_color_chunks", S * S)), device=dev)
    means = torch.empty((B * T,), device=dev)

    def kernel_pca(c):
        lib.call("sf_color_clip_f32", c.data_ptr(), B, T, S * S, host_pca.ctypes.data, dev_pca.data_ptr(), None, 0.0, 0.0, 0.0, 1.0,
                 1.0, 1.0, 1, stream)

    def kernel_all(c):
        lib.call("sf_color_frame_means_f32", c.data_ptr(), B, T, S * S, host_all.ctypes.data, dev_all.data_ptr(),
                 partials.data_ptr(), means.data_ptr(), stream)
        lib.call("sf_color_clip_f32", c.data_ptr(), B, T, S * S, host_all.ctypes.data, dev_all.data_ptr(), means.data_ptr(), 0.0, 0.0,
                 0.0, 1.0, 1.0, 1.0, 1, stream)

    def sample_then_color(f, o):
        ca.color_clip(ss.sample_clip(f, crop, mean, std, out=o), tab_all, mean, std, True)

    t_mean, t_std = torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    t_all = [(o, al, torch.tensor(ad, device=dev)) for o, al, ad in rows_all]
    t_pca = [(o, al, torch.tensor(ad, device=dev)) for o, al, ad in rows_pca]
    outs = clips[:nset_f] if nset_f <= nset else clips
    runs = {
        "color_kernel_pca": ([lambda c=c: kernel_pca(c) for c in clips], 2 * clip_b),
        "color_kernel_all": ([lambda c=c: kernel_all(c) for c in clips], 3 * clip_b),
        "color_clip_pca": ([lambda c=c: ca.color_clip(c, tab_pca, mean, std, True) for c in clips], 2 * clip_b),
        "color_clip_all": ([lambda c=c: ca.color_clip(c, tab_all, mean, std, True) for c in clips], 3 * clip_b),
        "sample_then_color": ([lambda f=f, i=i: sample_then_color(f, outs[i % len(outs)]) for i, f in enumerate(frames)],
                              src_b + 4 * clip_b),
        "sample_clip": ([lambda f=f, i=i: ss.sample_clip(f, crop, mean, std, out=outs[i % len(outs)]) for i, f in enumerate(frames)],
                        src_b + clip_b),
        "torch_color_pca": ([lambda c=c: torch_color(c, t_pca, t_mean, t_std, True) for c in clips], 2 * clip_b),
        "torch_color_all": ([lambda c=c: torch_color(c, t_all, t_mean, t_std, True) for c in clips], 3 * clip_b),
    }
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):                                  # alternate the variants inside every round
        for k, (fns, _) in runs.items():
            samples[k].append(timed(fns, a.iters))
    finite = all(bool(torch.isfinite(c).all()) for c in clips)
    res = {"clip": [B, 3, T, S, S], "frames": [B, T, H, W, 3], "buffer_sets": nset, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clips_finite_after": finite,
           "note": "bytes = the clip read and written once by the streaming pass, read once more by the reduction (all ops), plus "
                   "the uint8 source and the fp32 clip written by sample_clip where it runs; the torch yardsticks launch per "
                   "sample and per operation and move more bytes than that",
           "entries": {k: entry(samples[k], runs[k][1]) for k in runs}}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
