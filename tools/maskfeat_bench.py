"""Timing of the MaskFeat path on the GPU, HIP-event timed with COLD operands (every call works on the next of several buffer
sets whose sum exceeds the 256 MiB Infinity Cache):
  hog_kernel    sf_hog_targets_f32 on a dense fp32 (32, 3, 16, 224, 224) clip, ts 2, fs 14 (csrc/sf_hog.h): reads the 8 used frames
                of every sample once (4.8 MB) and writes 0.68 MB of targets per sample;
  hog_torch     the same targets from torch operations on the same device -- this tool's own restatement of the arithmetic
                (pad, shifted differences, atan2, scatter_add_ into a (B*T', 3, 9, H, W) tensor, cell sums, normalise, permute);
  step          one captured TrainStep of the MVITv2_S_16x4_MaskFeat_PT preset (model.dense = True, FlatOptimizer) at --batch,
                with a new mask table per iteration.
Bytes are the algorithm's (computed from the shapes), not counters.  Needs the GPU; there is no CPU fallback.
`python tools/maskfeat_bench.py [--batch B] [--iters N] [--rounds R] [--no-step] [--out profiles/maskfeat_bench.json]`"""
import argparse
import json
import math
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import slowfast_amd as sa
from slowfast_amd import masked, masking


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


def torch_hog(x, ts, fs):
    """The arithmetic of csrc/sf_hog.h as fp32 torch operations."""
    xs = x[:, :, ::ts]
    B, C, Tu, H, W = xs.shape
    xp = F.pad(xs.reshape(B * C * Tu, 1, H, W), (1, 1, 1, 1), mode="reflect")[:, 0]
    win = lambda r, c: xp[:, r:r + H, c:c + W]                                  # noqa: E731
    gx = (win(0, 0) - win(0, 2)) + 2.0 * (win(1, 0) - win(1, 2)) + (win(2, 0) - win(2, 2))
    gy = (win(0, 0) - win(2, 0)) + 2.0 * (win(0, 1) - win(2, 1)) + (win(0, 2) - win(2, 2))
    norm = torch.sqrt(gx * gx + gy * gy)
    bins = torch.floor(torch.atan2(gx, gy) / math.pi * 9.0).long() % 9
    bins = torch.where(gx == 0, torch.zeros_like(bins), bins)
    hist = torch.zeros((B * C * Tu, 9, H, W), dtype=torch.float32, device=x.device)
    hist.scatter_add_(1, bins[:, None], norm[:, None])
    Hc, Wc = H // 8, W // 8
    hist = hist.reshape(-1, 9, Hc, 8, Wc, 8).sum((3, 5))
    hist = hist / hist.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-12)
    u = Hc // fs
    return hist.reshape(B, C, Tu, 9, fs, u, fs, u).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, Tu * fs * fs, C * 9 * u * u)


def entry(samples, nbytes=None):
    med = statistics.median(samples)
    e = {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2)}
    if nbytes is not None:
        e.update({"bytes": int(nbytes), "TBps": round(nbytes / med / 1e6, 3)})
    return e


def bench_hog(a, dev):
    B, T, S, ts, fs = a.hog_batch, 16, 224, 2, 14
    Tu, u = T // ts, S // 8 // fs
    nbytes = 4.0 * B * (3 * Tu * S * S + Tu * fs * fs * 27 * u * u)
    clips = [torch.randn((B, 3, T, S, S), device=dev) for _ in range(2)]        # 2 x 308 MB at B = 32
    outs = [torch.empty((B, Tu * fs * fs, 27 * u * u), device=dev) for _ in range(2)]
    small = clips[0][:2].contiguous()
    dev_err = float((masked.hog_targets(small, ts, fs) - torch_hog(small, ts, fs)).abs().max())
    runs = {"hog_kernel": [lambda c=c, o=o: masked.hog_targets(c, ts, fs, out=o) for c, o in zip(clips, outs)],
            "hog_torch": [lambda c=c: torch_hog(c, ts, fs) for c in clips]}
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fns in runs.items():
            samples[k].append(timed(fns, a.iters))
    res = {k: entry(v, nbytes) for k, v in samples.items()}
    res["clip"] = [B, 3, T, S, S]
    res["bytes_per_sample"] = {"read": 4 * 3 * Tu * S * S, "written": 4 * Tu * fs * fs * 27 * u * u}
    # a sanity figure, not a parity check (tests/maskfeat_checks.py is): fp32 atan2 / floor puts pixels on a bin boundary into
    # the neighbouring bin, so single cells differ by a whole pixel's magnitude
    res["max_abs_diff_kernel_vs_torch_ops_2_samples"] = dev_err
    return res


def bench_step(a, dev):
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    from slowfast_amd.step import TrainStep
    cfg = sa.get_preset("MVITv2_S_16x4_MaskFeat_PT", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", a.batch])
    torch.manual_seed(cfg.RNG_SEED)
    model = sa.build_model(cfg, gpu_id=0).train()
    model.dense = True
    reducer = GradReducer(model)
    reducer.attach_torch_param_hooks(list(model.pred_head.projections.parameters()) + [model.mask_token])
    opt = construct_optimizer(model, cfg, reducer, loss_scale=a.loss_scale, dynamic_loss_scale=True)
    loss_fn = sa.get_loss_func(cfg.MODEL.LOSS_FUNC)(reduction="mean")
    step = TrainStep(model, reducer, opt, loss_fn, loss_scale=a.loss_scale, warmup=1, clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM)
    random.seed(cfg.RNG_SEED)
    gen = masking.construct_mask_generator(cfg)
    g = torch.Generator(device=dev).manual_seed(cfg.RNG_SEED)
    clip = torch.randn((a.batch, 3, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_CROP_SIZE), generator=g, device=dev)
    empty, placeholder = torch.Tensor().to(dev), torch.zeros(1, device=dev)
    tables = [gen.sample_batch(a.batch).to(dev) for _ in range(8)]
    losses = []

    def one(i):
        losses.append(step([clip, empty, tables[i % len(tables)]], placeholder))
    for i in range(4):
        one(i)
    torch.cuda.synchronize()
    samples = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.step_iters):
            one(i)
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1e3 / a.step_iters)
    vals = [float(l) for l in losses]
    res = entry(samples)
    res.update({"batch": a.batch, "clips_per_s": round(a.batch / statistics.median(samples) * 1e6, 2), "graph": step._graph is not None,
                "first_loss": vals[0], "last_loss": vals[-1], "losses_finite": all(math.isfinite(v) for v in vals)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hog-batch", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loss-scale", type=float, default=1024.0)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskfeat_bench needs the GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "act_dtype": sa.lib.ACT_MODE,
           "iters": a.iters, "rounds": a.rounds, "hog": bench_hog(a, dev)}
    if not a.no_step:
        res["step"] = bench_step(a, dev)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
