"""Microbenchmark of the optimizer update on the parameter sets of MViTv2-S (36 layer-decay groups, AdamW) and SlowFast-R50
(SGD-Nesterov), HIP-event timed with COLD operands (every call works on the next of several buffer sets whose sum exceeds the
256 MiB Infinity Cache):
  (i)   the table-driven update (sf_flat_adamw_tab / sf_flat_sgd_tab: hyper-parameters from device memory, 16-byte accesses)
        against sf_flat_adamw / sf_flat_sgd on the same buffers -- of this build and, when slowfast_amd/libsfamd_prev.so exists
        (tools/build_prev_lib.sh), of the parent commit's build in the same process on the same box;
  (ii)  the LARS norm pass + finalize (sf_flat_lars_trust: reads parameters AND gradients) against sf_flat_sumsq (reads the
        gradients) in achieved bytes/s;
  (iii) (--step) the whole TrainStep of SlowFast-R50 with SOLVER.LARS_ON False / True.
`python tools/optim_bench.py [--iters N] [--rounds R] [--step] [--batch B] [--out profiles/optim_layer_decay_bench.json]`"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import slowfast_amd as sa
from slowfast_amd import lib as sflib
from slowfast_amd.optim import _BLOCK, _SEG_DTYPE, construct_optimizer

PREV = os.path.join(ROOT, "slowfast_amd", "libsfamd_prev.so")


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


def param_groups_of(preset, opts):
    """(sizes, dims, group index) per parameter in FlatOptimizer's order (reverse registration), the hyper table rows."""
    from slowfast_amd.data_parallel import GradReducer
    cfg = sa.get_preset(preset, ["NUM_GPUS", 1] + list(opts))
    torch.manual_seed(0)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)            # CPU: only shapes and names are needed
    red = GradReducer(model)
    groups = _groups_only(model, cfg)
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    params = [(p.numel(), p.dim(), group_of[id(p)]) for p in red.params]
    red.close()
    hyper = [[1e-3 * g.get("layer_decay", 1.0), g["weight_decay"], float(bool(g.get("apply_LARS", False))), 0.0] for g in groups]
    return cfg, params, hyper


def _groups_only(model, cfg):
    from slowfast_amd import optim
    if float(cfg.SOLVER.get("LAYER_DECAY", 1.0)) != 1.0:
        return optim._layer_decay_groups(model, cfg)
    return optim._flat_groups(model, cfg, cfg.SOLVER.BASE_LR, bool(cfg.SOLVER.get("LARS_ON", False)))


class BufferSet:
    def __init__(self, n, dev, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.p = torch.randn(n, generator=g, device=dev)
        self.g = torch.randn(n, generator=g, device=dev) * 1e-3
        self.m1 = torch.zeros(n, device=dev)
        self.m2 = torch.zeros(n, device=dev)


def bench_set(name, preset, opts, method, iters, rounds, dev, prev):
    cfg, params, hyper = param_groups_of(preset, opts)
    n = sum(s for s, _, _ in params)
    segs, segs8, blk_seg, blk_off, seg_row = [], [], [], [], []
    off = 0
    for si, (size, dim, gi) in enumerate(params):
        segs.append((off, off + size, gi, 1 if dim != 1 else 0))
        segs8.append((off, off + size, gi % 8, 0))          # the argument path carries 8 groups: same bytes, folded groups
        seg_row.append(len(blk_seg))
        for b in range(0, size, _BLOCK):
            blk_seg.append(si)
            blk_off.append(b)
        off += size
    seg_row.append(len(blk_seg))
    to_dev = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    t_segs = torch.from_numpy(np.array(segs, dtype=_SEG_DTYPE).view(np.uint8).copy()).to(dev)
    t_segs8 = torch.from_numpy(np.array(segs8, dtype=_SEG_DTYPE).view(np.uint8).copy()).to(dev)
    t_bs, t_bo, t_row = to_dev(blk_seg, torch.int32), to_dev(blk_off, torch.int32), to_dev(seg_row, torch.int32)
    nblocks, nseg, ng = len(blk_seg), len(segs), len(hyper)
    t_hyper = to_dev(hyper, torch.float32)
    hyper_lars = [[h[0], h[1], 1.0, 0.0] for h in hyper]
    t_hyper_lars = to_dev(hyper_lars, torch.float32)
    ctl = torch.zeros(8, device=dev)
    ctl[0], ctl[4], ctl[5] = 1.0, 1.0, 3.0
    nbuf = 7 if method == "adamw" else 5
    nset = max(3, int(600e6 // (4.0 * n * 2)) + 1)              # the two-array norm pass must run cold as well
    sets = [BufferSet(n, dev, 10 + i) for i in range(nset)]
    trust = torch.zeros(nseg, device=dev)
    lpart = torch.empty((nblocks, 2), dtype=torch.float64, device=dev)
    native = sflib.get_lib()
    rows = native.call("sf_flat_blocks", n)
    part = torch.empty((rows, 2), device=dev)
    lr8 = (ctypes.c_float * 8)(*[1e-3] * 8)
    wd8 = (ctypes.c_float * 8)(*[hyper[i % ng][1] for i in range(8)])
    s = None

    def old(cdll, b):
        if method == "adamw":
            return lambda: cdll.sf_flat_adamw(b.p.data_ptr(), b.g.data_ptr(), b.m1.data_ptr(), b.m2.data_ptr(), t_segs8.data_ptr(),
                                              t_bs.data_ptr(), t_bo.data_ptr(), nblocks, ctl.data_ptr(), lr8, wd8, 8, 0.0, 0.9,
                                              0.999, 1e-8, s)
        return lambda: cdll.sf_flat_sgd(b.p.data_ptr(), b.g.data_ptr(), b.m1.data_ptr(), t_segs8.data_ptr(), t_bs.data_ptr(),
                                        t_bo.data_ptr(), nblocks, ctl.data_ptr(), lr8, wd8, 8, 0.0, 0.9, 0.0, 1, s)

    def tab(b, hyp, tr):
        if method == "adamw":
            return lambda: native.call("sf_flat_adamw_tab", b.p.data_ptr(), b.g.data_ptr(), b.m1.data_ptr(), b.m2.data_ptr(),
                                       t_segs.data_ptr(), t_bs.data_ptr(), t_bo.data_ptr(), nblocks, ctl.data_ptr(),
                                       hyp.data_ptr(), tr, 0.0, 0.9, 0.999, 1e-8, s)
        return lambda: native.call("sf_flat_sgd_tab", b.p.data_ptr(), b.g.data_ptr(), b.m1.data_ptr(), t_segs.data_ptr(),
                                   t_bs.data_ptr(), t_bo.data_ptr(), nblocks, ctl.data_ptr(), hyp.data_ptr(), tr, 0.0, 0.9, 0.0,
                                   1, s)

    def lars(b):
        return lambda: native.call("sf_flat_lars_trust", b.p.data_ptr(), b.g.data_ptr(), t_segs.data_ptr(), t_bs.data_ptr(),
                                   t_bo.data_ptr(), nblocks, t_row.data_ptr(), nseg, ctl.data_ptr(), t_hyper_lars.data_ptr(),
                                   lpart.data_ptr(), trust.data_ptr(), 0.0, 0.001, 1e-8, s)

    def sumsq(b):
        return lambda: native.call("sf_flat_sumsq", b.g.data_ptr(), n, part.data_ptr(), s)

    variants = {"args_this_build": [old(native.cdll, b) for b in sets], "table": [tab(b, t_hyper, None) for b in sets],
                "table_lars": [tab(b, t_hyper_lars, trust.data_ptr()) for b in sets],
                "lars_trust": [lars(b) for b in sets], "sumsq": [sumsq(b) for b in sets]}
    if prev is not None:
        variants["args_parent_build"] = [old(prev, b) for b in sets]
    samples = {k: [] for k in variants}
    for _ in range(rounds):                                   # interleaved rounds: drift hits every variant alike
        for k, fns in variants.items():
            samples[k].append(timed(fns, iters))
    res = {"preset": preset, "method": method, "parameters": n, "segments": nseg, "blocks": nblocks, "groups": ng,
           "buffer_sets": nset, "iters": iters, "rounds": rounds}
    by_upd = 4.0 * n * nbuf
    for k, v in samples.items():
        res[k] = spread(v)
    for k in ("args_this_build", "args_parent_build", "table", "table_lars"):
        if k in res:
            res[k]["GBps"] = round(by_upd / res[k]["median_us"] * 1e-3, 1)
    res["lars_trust"]["GBps"] = round(8.0 * n / res["lars_trust"]["median_us"] * 1e-3, 1)
    res["sumsq"]["GBps"] = round(4.0 * n / res["sumsq"]["median_us"] * 1e-3, 1)
    base = "args_parent_build" if prev is not None else "args_this_build"
    res["table_over_parent"] = round(res["table"]["median_us"] / res[base]["median_us"], 4)
    res["table_over_parent_baseline"] = base
    res["lars_over_sumsq_rate"] = round(res["lars_trust"]["GBps"] / res["sumsq"]["GBps"], 3)
    print(name, json.dumps(res), flush=True)
    return res


def bench_step(batch, steps, dev):
    """End-to-end TrainStep (HIP graph) of SlowFast-R50, SOLVER.LARS_ON off / on."""
    import torch.nn.functional as F
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.step import TrainStep
    out = {"preset": "SLOWFAST_8x8_R50", "batch": batch, "steps": steps}
    for label, lars in (("lars_off", False), ("lars_on", True)):
        cfg = sa.get_preset("SLOWFAST_8x8_R50", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", batch, "SOLVER.LARS_ON", lars])
        torch.manual_seed(cfg.RNG_SEED)
        model = sa.build_model(cfg, gpu_id=0).train()
        red = GradReducer(model)
        red.attach_torch_param_hooks(model.head.parameters())
        opt = construct_optimizer(model, cfg, red, loss_scale=1024.0, dynamic_loss_scale=True)
        g = torch.Generator(device=dev).manual_seed(1)
        T, S = cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE
        fast = torch.randn((batch, 3, T, S, S), generator=g, device=dev)
        idx = torch.linspace(0, T - 1, T // cfg.SLOWFAST.ALPHA).long().to(dev)
        inputs = [torch.index_select(fast, 2, idx).contiguous(), fast]
        labels = torch.randint(0, cfg.MODEL.NUM_CLASSES, (batch,), generator=g, device=dev)
        ts = TrainStep(model, red, opt, F.cross_entropy, use_graph=True, warmup=1)
        for _ in range(3):
            ts(inputs, labels)
        inputs, labels = ts.static_inputs()
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ts(inputs, labels)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / steps * 1e3)
        out[label] = {"step_ms": [round(t, 3) for t in times], "median_ms": round(statistics.median(times), 3),
                      "table_path": opt.table_path, "skipped": float(opt.ctl[6])}
        print("step", label, out[label], flush=True)
        red.close()
        del ts, opt, red, model, fast, inputs, labels
        torch.cuda.empty_cache()
    out["lars_on_over_off"] = round(out["lars_on"]["median_ms"] / out["lars_off"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prev = None
    if os.path.exists(PREV):
        prev = ctypes.CDLL(PREV)
        for name in ("sf_flat_sgd", "sf_flat_adamw"):
            fn = getattr(prev, name)
            fn.restype, fn.argtypes = sflib._SIGNATURES[name]
    res = {"device": torch.cuda.get_device_name(0), "parent_build": prev is not None}
    res["mvitv2_s_layer_decay"] = bench_set("MViTv2-S", "MVITv2_S_16x4", ["SOLVER.LAYER_DECAY", 0.75], "adamw", a.iters, a.rounds,
                                            dev, prev)
    res["slowfast_r50"] = bench_set("SlowFast-R50", "SLOWFAST_8x8_R50", [], "sgd", a.iters, a.rounds, dev, prev)
    if a.step:
        res["train_step"] = bench_step(a.batch, a.steps, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
