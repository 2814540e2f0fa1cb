"""Microbenchmark of the MoCo step glue (csrc/sf_moco.h) against the reference's torch-op sequence on the same device in the same
process, HIP-event timed with COLD operands (every call works on the next of several operand sets whose sum exceeds the 256 MiB
Infinity Cache; the method of tools/optim_bench.py):
  nce   the fused loss forward + gradient (contrastive.moco_nce + backward: two launches and one n x C multiply) against
        Normalize / einsum / cat / div / CrossEntropyLoss + autograd (tests/moco_checks.reference_sequence, the lines of
        slowfast/models/contrastive.py:452-477) at (n, V, K, C) = (8, 3, 65536, 128) and (64, 3, 65536, 128);
  ema   sf_ema_update over Slow-R50's parameter count against `hist = p * (1.0 - m) + hist * m`.
Bytes moved are the algorithmic minimum of the fused path (queue once, logits once, features; parameters and history once each
way), so the achieved bandwidth of the torch sequence is in the same unit.
`python tools/moco_bench.py [--iters N] [--rounds R] [--out profiles/moco_bench.json]`"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import slowfast_amd as sa
from slowfast_amd import contrastive as ct
from tests.moco_checks import reference_sequence

NCE_SHAPES = ((8, 3, 65536, 128), (64, 3, 65536, 128))
T = 0.1


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


def spread(samples):
    med = statistics.median(samples)
    return {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2),
            "spread_pct": round(100.0 * (max(samples) - min(samples)) / med, 2)}


def bench_nce(n, V, K, C, iters, rounds, dev):
    by = 4.0 * (K * C + V * n * (K + 1) + (V + 2) * n * C)
    nset = max(3, int(600e6 // by) + 1)
    g = torch.Generator(device=dev).manual_seed(1)
    sets = []
    for _ in range(nset):
        f = (torch.randn((n, C), generator=g, device=dev) * 3.0).requires_grad_(True)
        keys = ct.l2norm_rows(torch.randn((V * n, C), generator=g, device=dev)).view(V, n, C)
        queue = ct.l2norm_rows(torch.randn((K, C), generator=g, device=dev))
        sets.append((f, keys, queue))

    def fused(s):
        def run():
            s[0].grad = None
            _, loss = ct.moco_nce(s[0], s[1], s[2], T)
            loss.backward()
        return run

    def torch_ops(s):
        def run():
            s[0].grad = None
            _, loss = reference_sequence(s[0], s[1], s[2], T)
            loss.backward()
        return run

    # same numbers first
    fused(sets[0])()
    a = sets[0][0].grad.clone()
    torch_ops(sets[0])()
    rel = float((a - sets[0][0].grad).abs().max() / sets[0][0].grad.abs().max())
    # the two launches on their own (no autograd, no allocation): what the kernels take of the fused figure
    from slowfast_amd.lib import get_lib
    native, ws = get_lib(), ct._workspace(dev, n, V, K, C)
    outs = [(torch.empty((V * n, 1 + K), device=dev), torch.empty((n, C), device=dev), torch.empty(1, device=dev)) for _ in sets]

    def launch(name, s, o):
        args = (n, V, K, C, s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 1.0 / T, o[0].data_ptr(), o[1].data_ptr(),
                o[2].data_ptr(), ws.data_ptr(), ws.numel() * 4, None)
        return lambda: native.call(name, *args)

    variants = {"fused": [fused(s) for s in sets], "torch_sequence": [torch_ops(s) for s in sets],
                "slab_kernel": [launch("sf_moco_nce_slabs", s, o) for s, o in zip(sets, outs)],
                "finalize_kernel": [launch("sf_moco_nce_finalize", s, o) for s, o in zip(sets, outs)]}
    samples = {k: [] for k in variants}
    for _ in range(rounds):                                   # interleaved rounds: drift hits both alike
        for k, fns in variants.items():
            samples[k].append(timed(fns, iters))
    res = {"n": n, "V": V, "K": K, "C": C, "bytes": by, "operand_sets": nset, "iters": iters, "rounds": rounds,
           "df_max_rel_difference": rel}
    for k, v in samples.items():
        res[k] = spread(v)
        res[k]["GBps"] = round(by / res[k]["median_us"] * 1e-3, 1)
    res["torch_over_fused"] = round(res["torch_sequence"]["median_us"] / res["fused"]["median_us"], 3)
    print("nce", json.dumps(res), flush=True)
    return res


def bench_ema(iters, rounds, dev):
    cfg = sa.get_preset("MoCo_SlowR50_8x8")
    count = sum(p.numel() for p in sa.video_models.ResNet(cfg).parameters())
    by = 12.0 * count
    nset = max(3, int(600e6 // (8.0 * count)) + 1)
    g = torch.Generator(device=dev).manual_seed(2)
    sets = [[torch.randn(count, generator=g, device=dev), torch.randn(count, generator=g, device=dev)] for _ in range(nset)]
    m = 0.994
    mm = ct.momentum_words(m).to(dev)

    def fused(s):
        return lambda: ct.ema_update(s[0], s[1], mm)

    def torch_ops(s):
        def run():
            s[1] = s[0] * (1.0 - m) + s[1] * m
        return run

    variants = {"fused": [fused(s) for s in sets], "torch_three_ops": [torch_ops(s) for s in sets]}
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fns in variants.items():
            samples[k].append(timed(fns, iters))
    res = {"parameters": count, "bytes": by, "operand_sets": nset, "iters": iters, "rounds": rounds}
    for k, v in samples.items():
        res[k] = spread(v)
        res[k]["GBps"] = round(by / res[k]["median_us"] * 1e-3, 1)
    res["torch_over_fused"] = round(res["torch_three_ops"]["median_us"] / res["fused"]["median_us"], 3)
    print("ema", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    res["nce"] = [bench_nce(n, V, K, C, a.iters, a.rounds, dev) for n, V, K, C in NCE_SHAPES]
    res["ema"] = bench_ema(a.iters, a.rounds, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
