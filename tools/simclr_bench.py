"""Microbenchmark of the SimCLR NT-Xent loss (csrc/sf_simclr.h) against the reference's torch-op sequence on the same device in
the same process, HIP-event timed with COLD operands (every call works on the next of several operand sets whose sum exceeds the
256 MiB Infinity Cache; the method of tools/moco_bench.py):
  ntx   the loss forward + both gradients (contrastive.simclr_ntxent + backward: three launches and two n x C multiplies) against
        Normalize twice / cat / mm / exp / the mask / masked_select / sum / the positives / div / log / mean + autograd
        (tests/simclr_checks.reference_sequence, the lines of slowfast/models/contrastive.py:698-745) at (n, C) = (64, 128),
        (256, 128) and (512, 128): one pair of crops at the recipe's batch per device, and larger batches.
The operands of one call are 64 KB .. 0.5 MB, so being cold costs each call a few first-touch misses; the workspace (the M x M
matrix E among it) is shared between the sets and stays warm.  `timed` runs every set once before it times the first `iters` of
them.  No ratio is expected in advance; the file is where the number goes.  Device kernels per call are counted on both sides with
torch.profiler (the fused side also by the native calls it makes); the torch sequence synchronises the host inside masked_select.
`--bench-lines NAME=FILE ...` adds recorded `bench.py` result lines under `default_bench_ab` (the outputs of this tree's and the
parent tree's `python bench.py --gpus 1 --steps 20 --warmup 5`, alternating on one box).
`python tools/simclr_bench.py [--iters N] [--rounds R] [--out profiles/simclr_bench.json]`"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from slowfast_amd import contrastive as ct
from tests.moco_checks import count_calls
from tests.simclr_checks import LAUNCHES, reference_sequence
from tools.moco_bench import spread, timed

NTX_SHAPES = ((64, 128), (256, 128), (512, 128))
T = 0.1


def device_kernels(fn):
    """Device kernels launched by one call of ``fn`` (None when the profiler gives no device events on this build)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(names) or None
    except Exception as e:      # the count is a side figure: a profiler that cannot start must not cost the timings
        print("device_kernels: %s: %s" % (type(e).__name__, e))
        return None


def bench_ntx(n, C, iters, rounds, dev):
    by = 4.0 * (4 * n * C)                                      # a, b read, da, db written
    nset = int(600e6 // (8.0 * n * C)) + 1
    g = torch.Generator(device=dev).manual_seed(1)
    sets = [((torch.randn((n, C), generator=g, device=dev) * 3.0).requires_grad_(True),
             (torch.randn((n, C), generator=g, device=dev) * 3.0).requires_grad_(True)) for _ in range(nset)]

    def fused(s):
        def run():
            s[0].grad = s[1].grad = None
            ct.simclr_ntxent(s[0], s[1], T).backward()
        return run

    def torch_ops(s):
        def run():
            s[0].grad = s[1].grad = None
            reference_sequence(s[0], s[1], T).backward()
        return run

    # same numbers first
    fused(sets[0])()
    ga, gb = sets[0][0].grad.clone(), sets[0][1].grad.clone()
    torch_ops(sets[0])()
    rel = max(float((ga - sets[0][0].grad).abs().max() / sets[0][0].grad.abs().max()),
              float((gb - sets[0][1].grad).abs().max() / sets[0][1].grad.abs().max()))
    with count_calls() as calls:
        fused(sets[0])()
    launches = {"fused_native_calls": [c for c in calls if c != "sf_simclr_workspace"],
                "fused_device_kernels": device_kernels(fused(sets[0])),
                "torch_sequence_device_kernels": device_kernels(torch_ops(sets[0]))}
    # the three launches on their own (no autograd, no allocation): what the kernels take of the fused figure
    from slowfast_amd.lib import get_lib
    native, ws = get_lib(), ct._simclr_workspace(dev, n, C)
    outs = [(torch.empty((n, C), device=dev), torch.empty((n, C), device=dev), torch.empty(1, device=dev)) for _ in sets]

    def launch(name, s, o):
        args = (n, C, s[0].data_ptr(), C, s[1].data_ptr(), C, 1.0 / T, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None,
                ws.data_ptr(), ws.numel() * 4, None)
        return lambda: native.call(name, *args)

    variants = {"fused": [fused(s) for s in sets], "torch_sequence": [torch_ops(s) for s in sets]}
    for name in LAUNCHES:
        variants[name[len("sf_simclr_"):] + "_kernel"] = [launch(name, s, o) for s, o in zip(sets, outs)]
    samples = {k: [] for k in variants}
    for _ in range(rounds):                                   # interleaved rounds: drift hits both alike
        for k, fns in variants.items():
            samples[k].append(timed(fns, iters))
    res = {"n": n, "C": C, "T": T, "bytes": by, "flops": 4.0 * (2 * n) ** 2 * C, "operand_sets": nset, "iters": iters,
           "rounds": rounds, "grad_max_rel_difference": rel, "launches": launches}
    for k, v in samples.items():
        res[k] = spread(v)
    res["torch_over_fused"] = round(res["torch_sequence"]["median_us"] / res["fused"]["median_us"], 3)
    print("ntx", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-lines", nargs="*", default=[], metavar="NAME=FILE",
                    help="files holding the output of `bench.py` (its JSON result line is the last line that starts with `{`)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    res["ntx"] = [bench_ntx(n, C, a.iters, a.rounds, dev) for n, C in NTX_SHAPES]
    if a.bench_lines:
        ab = {"cmd": "python bench.py --gpus 1 --steps 20 --warmup 5 (SLOWFAST_8x8_R50, batch 32), parent tree and this tree "
                     "alternating on one box; value = clips/s"}
        for item in a.bench_lines:
            name, path = item.split("=", 1)
            with open(path) as f:
                line = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
            ab[name] = {k: line[k] for k in ("value", "ms_per_step", "final_loss") if k in line}
        res["default_bench_ab"] = ab
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
