"""Microbenchmark of the MixUp / CutMix entry points (csrc/sf_mixup.h; the pack_u8 rows are specialisations of
sf_pack_clip_kernel, csrc/sf_pack.h) at the MViTv2-S bs32 clip (32, 3, 16, 224, 224),
HIP-event timed with COLD operands: every call works on the next of several clips whose sum exceeds the 256 MiB Infinity Cache
(the rotation of tools/optim_bench.py):
  mixup_inplace     sf_mix_clip_f32 mode 0, in place                     (reads + writes the clip once: 2 x 308 MB)
  cutmix_inplace    sf_mix_clip_f32 mode 1, in place, half-area box      (reads + writes the two halves of the box)
  torch_mixup       the reference's x.flip(0).mul_(1 - lam); x.mul_(lam).add_(..) on the same device (the yardstick)
  torch_cutmix      the reference's x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
  pack_u8           sf_pack_clip_u8      uint8 frames -> 16-bit W-pair clip
  pack_u8_mixup     sf_pack_clip_u8_mix  the same with mixup (reads two frames per output pixel)
  pack_u8_cutmix    sf_pack_clip_u8_mix  the same with the half-area cutmix box
Bytes are the algorithm's (computed from the shapes), not counters.  Needs the GPU; there is no CPU fallback.
`python tools/mixup_bench.py [--batch B] [--iters N] [--rounds R] [--out profiles/mixup_bench.json]`"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import slowfast_amd as sa
from slowfast_amd import mixup
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


def torch_mixup(x, lam):
    x_flipped = x.flip(0).mul_(1.0 - lam)
    x.mul_(lam).add_(x_flipped)


def torch_cutmix(x, box):
    yl, yh, xl, xh = box
    x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixup_bench needs the GPU")
    dev = torch.device("cuda:0")
    B, T, S = a.batch, a.frames, a.crop
    shape = (B, 3, T, S, S)
    n = B * 3 * T * S * S
    nset = max(2, int(600e6 // (4.0 * n)) + 1)
    clips = [torch.randn(shape, device=dev) for _ in range(nset)]
    cfg = sa.get_preset("MVITv2_S_16x4", ["NUM_GPUS", 1, "DATA.NUM_FRAMES", T, "DATA.TRAIN_CROP_SIZE", S])
    nset_u8 = max(2, int(600e6 // (11.0 * B * T * S * S)) + 1)     # 3 bytes in + 8 bytes out per pixel
    frames = [torch.randint(0, 256, (B, T, S, S, 3), device=dev, dtype=torch.uint8) for _ in range(nset_u8)]
    packed = [sa.pack_pathways_u8(f, cfg) for f in frames]
    lam = 0.37
    box = (0, S, 0, S // 2)                                   # half the area; xh on a 16-byte boundary
    box_elems = (B // 2) * 2 * 3 * T * (box[1] - box[0]) * (box[3] - box[2])
    p_mix, p_cut = MixParams(lam, False, None), MixParams(0.5, True, box)
    pix = B * T * S * S
    runs = {
        "mixup_inplace": ([lambda c=c: mixup.mix_clip(c, p_mix) for c in clips], 8.0 * n),
        "cutmix_inplace": ([lambda c=c: mixup.mix_clip(c, p_cut) for c in clips], 8.0 * box_elems),
        "torch_mixup": ([lambda c=c: torch_mixup(c, lam) for c in clips], 8.0 * n),
        "torch_cutmix": ([lambda c=c: torch_cutmix(c, box) for c in clips], 8.0 * box_elems),
        "pack_u8": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o) for f, o in zip(frames, packed)], 3.0 * pix + 8.0 * pix),
        "pack_u8_mixup": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o, mix=p_mix) for f, o in zip(frames, packed)],
                          6.0 * pix + 8.0 * pix),
        "pack_u8_cutmix": ([lambda f=f, o=o: sa.pack_pathways_u8(f, cfg, out=o, mix=p_cut) for f, o in zip(frames, packed)],
                           3.0 * pix + 8.0 * pix),
    }
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):                                  # alternate the variants inside every round
        for k, (fns, _) in runs.items():
            samples[k].append(timed(fns, a.iters))
    res = {"clip": list(shape), "clip_bytes": 4 * n, "buffer_sets": nset, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "note": "bytes = what the algorithm must move (torch_* rows carry the SAME bytes as the fused rows, so their TBps is "
                   "the useful rate, not the traffic the op sequence causes)",
           "entries": {k: entry(samples[k], runs[k][1]) for k in runs}}
    e = res["entries"]
    res["speedup_mixup_vs_torch"] = round(e["torch_mixup"]["median_us"] / e["mixup_inplace"]["median_us"], 2)
    res["speedup_cutmix_vs_torch"] = round(e["torch_cutmix"]["median_us"] / e["cutmix_inplace"]["median_us"], 2)
    res["pack_mixup_over_pack"] = round(e["pack_u8_mixup"]["median_us"] / e["pack_u8"]["median_us"], 2)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
