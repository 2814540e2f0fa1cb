"""Timing of the MAE path on the GPU, HIP-event timed with COLD operands (every call works on the next of several buffer sets
whose sum exceeds the 256 MiB Infinity Cache):
  pixel_kernel    sf_pixel_targets_f32 on a dense fp32 (32, 3, 16, 224, 224) clip, ts 2, u 1, p 16, normalised (csrc/sf_pixel.h):
                  reads the 8 used frames of every sample once and writes (1568, 768) fp32 targets per sample;
  pixel_torch     the reference's formulation on the same device: slice, reshape / einsum / reshape, mean, var, subtract, divide;
  keep_* / restore_*   the four token kernels at (32, 1569, 768) -> K 156 and (32, 157, 512) -> 1569 rows against the reference's
                  chain of argsort / gather / repeat / cat / += (forward) and its autograd backward, in the activation type;
  step            one captured TrainStep of the k400_VIT_B_16x4_MAE_PT preset (model.dense = True, FlatOptimizer AdamW) at
                  --batch, with a new ids_restore table per iteration.
Bytes are the algorithm's (computed from the shapes), not counters.  Needs the GPU; there is no CPU fallback.
`python tools/mae_bench.py [--batch B] [--iters N] [--rounds R] [--no-step] [--out profiles/mae_bench.json]`"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import slowfast_amd as sa
from slowfast_amd import masked, masking, tokens


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


def entry(samples, nbytes=None):
    med = statistics.median(samples)
    e = {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2)}
    if nbytes is not None:
        e.update({"bytes": int(nbytes), "TBps": round(nbytes / med / 1e6, 3)})
    return e


def run_all(runs, a, nbytes):
    samples = {k: [] for k in runs}
    for _ in range(a.rounds):           # the variants alternate inside a round
        for k, fns in runs.items():
            samples[k].append(timed(fns, a.iters))
    return {k: entry(v, nbytes.get(k)) for k, v in samples.items()}


def torch_pixels(x, ts, p):
    """_get_pixel_label_3d with TIME_STRIDE_LOSS and NORM_PRED_PIXEL for all rows, as fp32 torch operations."""
    x = x[:, :, ::ts]
    N, _, T, H, W = x.shape
    h = w = H // p
    x = torch.einsum("nctuhpwq->nthwupqc", x.reshape(N, 3, T, 1, h, p, w, p)).reshape(N, T * h * w, p * p * 3)
    mean = x.mean(dim=-1, keepdim=True)
    var = x.var(dim=-1, keepdim=True)
    return (x - mean) / (var + 1.0e-6) ** 0.5


def bench_pixels(a, dev):
    B, T, S, ts, p = a.pixel_batch, 16, 224, 2, 16
    rows, n = (T // ts) * (S // p) ** 2, p * p * 3
    nbytes = 4.0 * B * (3 * (T // ts) * S * S + rows * n)
    clips = [torch.randn((B, 3, T, S, S), device=dev) for _ in range(2)]        # 2 x 308 MB at B = 32
    outs = [torch.empty((B, rows, n), device=dev) for _ in range(2)]
    small = clips[0][:2].contiguous()
    err = float((masked.pixel_targets(small, ts, 1, p, True) - torch_pixels(small, ts, p)).abs().max())
    runs = {"pixel_kernel": [lambda c=c, o=o: masked.pixel_targets(c, ts, 1, p, True, out=o) for c, o in zip(clips, outs)],
            "pixel_torch": [lambda c=c: torch_pixels(c, ts, p) for c in clips]}
    res = run_all(runs, a, {k: nbytes for k in runs})
    res["clip"] = [B, 3, T, S, S]
    res["bytes_per_sample"] = {"read": 4 * 3 * (T // ts) * S * S, "written": 4 * rows * n}
    res["max_abs_diff_kernel_vs_torch_ops_2_samples"] = err         # a sanity figure; tests/mae_checks.py is the parity check
    return res


def ref_keep(x, ids, K):
    """gather of the kept rows behind the cls row (the reference gathers x and pos_embed separately; one gather here)."""
    ids_keep = torch.argsort(ids.long(), dim=1)[:, :K]
    kept = torch.gather(x[:, 1:], 1, ids_keep.unsqueeze(-1).repeat(1, 1, x.shape[-1]))
    return torch.cat([x[:, :1], kept], 1)


def ref_restore(e, ids, tok, dpos):
    B, L = ids.shape
    x_ = torch.cat([e[:, 1:], tok.to(e.dtype).repeat(B, L + 1 - e.shape[1], 1)], dim=1)
    x_ = torch.gather(x_, 1, ids.long().unsqueeze(-1).repeat(1, 1, e.shape[-1]))
    return torch.cat([e[:, :1], x_], dim=1) + dpos.to(e.dtype)


def bench_tokens(a, dev):
    act = sa.lib.act_dtype()
    B, L, K, C, Cd = a.batch, 1568, 156, 768, 512
    gen = masking.MaeMaskGenerator(L, 0.9)
    sets = 6                                                  # 6 x 77 MB of (B, 1569, 768) rows at B = 32
    ids = [gen.sample_batch(B).to(dev) for _ in range(sets)]
    xs = [torch.randn((B, 1 + L, C), device=dev).to(act) for _ in range(sets)]
    dys = [torch.randn((B, 1 + K, C), device=dev).to(act) for _ in range(sets)]
    es = [torch.randn((B, 1 + K, Cd), device=dev).to(act) for _ in range(sets)]
    dyr = [torch.randn((B, 1 + L, Cd), device=dev).to(act) for _ in range(sets)]
    tok = torch.randn((1, 1, Cd), device=dev)
    dpos = torch.randn((1, 1 + L, Cd), device=dev)
    tok1, dpos2 = tok.view(-1).contiguous(), dpos.view(1 + L, Cd).contiguous()

    def ref_keep_bwd(x, i, g):
        x = x.detach().requires_grad_(True)
        ref_keep(x, i, K).backward(g)
        return x.grad

    def ref_restore_bwd(e, i, g):
        e, t, p = e.detach().requires_grad_(True), tok.detach().requires_grad_(True), dpos.detach().requires_grad_(True)
        ref_restore(e, i, t, p).backward(g)
        return e.grad, t.grad, p.grad
    z = zip
    runs = {
        "keep_fwd_kernel": [lambda x=x, i=i: tokens.token_keep_fwd(x, i, K, 1) for x, i in z(xs, ids)],
        "keep_fwd_torch": [lambda x=x, i=i: ref_keep(x, i, K) for x, i in z(xs, ids)],
        "keep_bwd_kernel": [lambda g=g, i=i: tokens.token_keep_bwd(g, i, L, 1) for g, i in z(dys, ids)],
        "keep_fwd_bwd_torch": [lambda x=x, i=i, g=g: ref_keep_bwd(x, i, g) for x, i, g in z(xs, ids, dys)],
        "restore_fwd_kernel": [lambda e=e, i=i: tokens.token_restore_fwd(e, i, tok1, dpos2, 1) for e, i in z(es, ids)],
        "restore_fwd_torch": [lambda e=e, i=i: ref_restore(e, i, tok, dpos) for e, i in z(es, ids)],
        "restore_bwd_kernel": [lambda g=g, i=i: tokens.token_restore_bwd(g, i, K, 1) for g, i in z(dyr, ids)],
        "restore_fwd_bwd_torch": [lambda e=e, i=i, g=g: ref_restore_bwd(e, i, g) for e, i, g in z(es, ids, dyr)],
    }
    nbytes = {"keep_fwd_kernel": 4.0 * B * (1 + K) * C + 4.0 * B * L, "keep_bwd_kernel": 2.0 * B * (2 + K + L) * C + 4.0 * B * L,
              "restore_fwd_kernel": 2.0 * B * (2 + K + L) * Cd + 4.0 * (1 + L) * Cd + 4.0 * B * L,
              "restore_bwd_kernel": 2.0 * B * (2 + K + L) * Cd + 4.0 * (1 + L) * Cd + 4.0 * B * L}
    res = run_all(runs, a, nbytes)
    res["shapes"] = {"keep": [B, 1 + L, C], "restore": [B, 1 + L, Cd], "K": K}
    res["keep_fwd_equal"] = bool(torch.equal(tokens.token_keep_fwd(xs[0], ids[0], K, 1), ref_keep(xs[0], ids[0], K)))
    return res


def bench_step(a, dev):
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    from slowfast_amd.step import TrainStep
    cfg = sa.get_preset("k400_VIT_B_16x4_MAE_PT", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", a.batch])
    torch.manual_seed(cfg.RNG_SEED)
    model = sa.build_model(cfg, gpu_id=0).train()
    model.dense = True
    reducer = GradReducer(model)
    torch_params = list(model.pred_head.projections.parameters()) + [model.mask_token]
    torch_params += [p for n, p in model.named_parameters() if n.startswith(("pos_embed", "dec_pos_embed", "decoder_pos_embed"))]
    reducer.attach_torch_param_hooks(torch_params)
    opt = construct_optimizer(model, cfg, reducer, loss_scale=a.loss_scale, dynamic_loss_scale=True)
    loss_fn = sa.get_loss_func(cfg.MODEL.LOSS_FUNC)(reduction="mean")
    step = TrainStep(model, reducer, opt, loss_fn, loss_scale=a.loss_scale, warmup=1, clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM)
    gen = masking.construct_mae_mask_generator(cfg)
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
    ap.add_argument("--pixel-batch", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loss-scale", type=float, default=1024.0)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mae_bench needs the GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "act_dtype": sa.lib.ACT_MODE,
           "iters": a.iters, "rounds": a.rounds, "pixels": bench_pixels(a, dev), "tokens": bench_tokens(a, dev)}
    if not a.no_step:
        res["step"] = bench_step(a, dev)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
