"""Microbenchmark of the BYOL similarity loss (csrc/sf_byol.h) against the reference's torch-op sequence on the same device in
the same process, HIP-event timed with COLD operands (every call works on the next of several operand sets whose sum exceeds the
256 MiB Infinity Cache; the method of tools/moco_bench.py):
  sim   the loss forward + gradient (contrastive.byol_sim + backward: two launches and one n x C multiply) against Normalize /
        einsum / div / mean / neg per key, the sum over keys and the division + autograd (tests/byol_checks.reference_sequence,
        the lines of slowfast/models/contrastive.py:237-243, :512, :532-535) at (n, V, C) = (64, 1, 256) and (64, 3, 256): the
        symmetric and the sequential form of the recipe's batch.
At this size both sides are bound by launches and the host, not by bytes: the operands of one call are 0.2 .. 0.3 MB, so being
cold costs each call a few first-touch misses and no more.  `timed` runs every set once before it times the first `iters` of
them, so each timed call finds its operands 600 MB of traffic old.  No ratio is expected in advance; the file is where the number goes.
`--bench-lines NAME=FILE ...` adds recorded `bench.py` result lines under `default_bench_ab` (the outputs of this tree's and the
parent tree's `python bench.py --gpus 1 --steps 20 --warmup 5`, alternating on one box: the head code is shared with every model).
`python tools/byol_bench.py [--iters N] [--rounds R] [--out profiles/byol_bench.json]`"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from slowfast_amd import contrastive as ct
from tests.byol_checks import reference_sequence
from tools.moco_bench import spread, timed

SIM_SHAPES = ((64, 1, 256), (64, 3, 256))
T = 0.5


def bench_sim(n, V, C, iters, rounds, dev):
    by = 4.0 * ((V + 2) * n * C)
    nset = int(600e6 // by) + 1                                # thousands of small sets: 600 MB in all
    g = torch.Generator(device=dev).manual_seed(1)
    sets = []
    for _ in range(nset):
        p = (torch.randn((n, C), generator=g, device=dev) * 3.0).requires_grad_(True)
        keys = ct.l2norm_rows(torch.randn((V * n, C), generator=g, device=dev)).view(V, n, C)
        sets.append((p, keys))

    def fused(s):
        def run():
            s[0].grad = None
            ct.byol_sim(s[0], s[1], T).backward()
        return run

    def torch_ops(s):
        def run():
            s[0].grad = None
            reference_sequence(s[0], s[1], T).backward()
        return run

    # same numbers first
    fused(sets[0])()
    a = sets[0][0].grad.clone()
    torch_ops(sets[0])()
    rel = float((a - sets[0][0].grad).abs().max() / sets[0][0].grad.abs().max())
    # the two launches on their own (no autograd, no allocation): what the kernels take of the fused figure
    from slowfast_amd.lib import get_lib
    native, ws = get_lib(), ct._byol_workspace(dev, n, V, C)
    outs = [(torch.empty((n, C), device=dev), torch.empty(1, device=dev)) for _ in sets]

    def launch(name, s, o):
        args = (n, V, C, s[0].data_ptr(), C, s[1].data_ptr(), 1.0 / T, o[0].data_ptr(), o[1].data_ptr(), ws.data_ptr(),
                ws.numel() * 4, None)
        return lambda: native.call(name, *args)

    variants = {"fused": [fused(s) for s in sets], "torch_sequence": [torch_ops(s) for s in sets],
                "rows_kernel": [launch("sf_byol_sim_rows", s, o) for s, o in zip(sets, outs)],
                "finalize_kernel": [launch("sf_byol_sim_finalize", s, o) for s, o in zip(sets, outs)]}
    samples = {k: [] for k in variants}
    for _ in range(rounds):                                   # interleaved rounds: drift hits both alike
        for k, fns in variants.items():
            samples[k].append(timed(fns, iters))
    res = {"n": n, "V": V, "C": C, "bytes": by, "operand_sets": nset, "iters": iters, "rounds": rounds,
           "df_max_rel_difference": rel}
    for k, v in samples.items():
        res[k] = spread(v)
    res["torch_over_fused"] = round(res["torch_sequence"]["median_us"] / res["fused"]["median_us"], 3)
    print("sim", json.dumps(res), flush=True)
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
    res["sim"] = [bench_sim(n, V, C, a.iters, a.rounds, dev) for n, V, C in SIM_SHAPES]
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
