"""Checks of the BYOL path (csrc/sf_byol.h, slowfast_amd/contrastive.py, the predictor heads of slowfast_amd/heads.py), shared by
tests/test_byol_hostsim.py and the -m gpu file tests/test_byol_gpu.py.

Reference.  An fp64 restatement of the reference's arithmetic (slowfast/models/contrastive.py: Normalize on the predictor
output, sim_loss, the loop over the keys of the byol branch), pinned to tests/golden/byol_contract.json, which
tools/make_byol_golden.py records from the unmodified reference; df comes from fp64 autograd.  Every comparison is per element.

Bounds, read off the operation counts (u = 2^-24; nothing is fitted to an observed error; any summation order is covered).
They are absolute in the magnitudes of the TERMS, not relative to the result: a result that is pure cancellation (the gradient
of the `parallel` kind) is held to the rounding of what was cancelled.
  eq     relative error of an element of q = p / |p|: a C-term sum of squares ((C + 1) u, halved by the root), the root, the
         division: (C / 2 + 4) u.
  E_s    a similarity (q . k) / T: a C-term fp32 dot in any order, (C + 1) u sum|q_c k_c|; q's own error, eq sum|q_c k_c|;
         1 / T rounded to fp32 and the product (or the division), 2 u, one to spare:  (1.5 C + 8) u sum_c|q_c k_c| / T.
  E_loss sum_v [-mean_i s_v,i] / V: the similarities' own errors, mean(E_s); an n-term and a V-term sum in any order, the two
         divisions and the negation: (n + V + 4) u mean|s| / T.
  E_S    an element of S = sum_v k_v: a V-term sum, (V + 1) u sum_v|k_v,c|.
  E_d    d = q . S: the C-term dot ((C + 1) u), q's error (eq), one to spare: (1.5 C + 6) u sum_c|q_c S_c|; S's own error,
         sum_c|q_c| E_S,c.
  E_df   df = -(1 / (V n T)) (S - q d) / |p|.  The numerator: E_S; d's error times |q|; q's error in the product, eq |q d|; the
         product and the difference, 3 u (|S| + |q d|).  The division by |p| (its relative error is below eq), the factor
         1 / (V n T) however it is formed (1 / T rounded, a product or a division by V n, the scaling): (eq + 6 u) (|S| + |q d|).
         All over V n T |p|.  A grad_out g scales df and its bound by |g| and adds one rounding.
The condition on these bounds is that the reference's OWN fp32 CPU run stays inside them on every recorded input (ratio <= 1):
asserted by the golden tool, recorded in the fixture, and checked again here on the CPU (check_reference_inside_bounds).
"""
import itertools
import json
import math
import os

import torch

import slowfast_amd as sa
from slowfast_amd import contrastive as ct
from slowfast_amd import engine
from slowfast_amd.lib import SfError
from tests import moco_checks as mc
from tests.moco_checks import U, count_calls, digest, f32_list, sample_index, state_list  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "byol_contract.json")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with open(GOLDEN) as f:
            _fx = json.load(f)
    return _fx


# ------------------------------------------------------------------------------------------------ the loss kernel
SIM_N = (1, 5, 67)          # 67: 17 workgroups of four rows, and more row terms than one wave of the finalize workgroup holds
SIM_V = (1, 2, 3)
SIM_C = (64, 100, 256)      # 100: tail lanes (36 lanes own two columns, 28 own one)
SIM_T = (0.5, 0.07)
SIM_SCALES = (1.0, 1e-3, 1e3)
SIM_KINDS = ("randn", "parallel", "antiparallel", "near", "onehot")
SIM_GRADS = (1.0, 1024.0)
SIM_SHAPES = tuple(itertools.product(SIM_N, SIM_V, SIM_C))
DF_SAMPLE = 4
PITCH_PAD = 24


def sim_cases(n, V, C):
    """Every (T, scale, kind) of one shape."""
    return itertools.product(SIM_T, SIM_SCALES, SIM_KINDS)


def sim_key(n, V, C, T, scale, kind):
    return "n%d_V%d_C%d_T%g_s%g_%s" % (n, V, C, T, scale, kind)


def sim_inputs(n, V, C, scale, kind, seed=71):
    """(p (n, C), keys (V, n, C)), float32 on the CPU.  `parallel`: p = 2.5 key_0, the similarity with view 0 is 1 and its
    gradient is pure cancellation; `antiparallel`: p = -2.5 key_0; `near`: key_0 plus a 1e-3 perturbation; `onehot`: a one-hot
    p.  The input scale multiplies p afterwards."""
    g = torch.Generator().manual_seed(seed + 7 * n + 13 * V + C)
    keys = mc._unit(torch.randn((V, n, C), generator=g))
    p = torch.randn((n, C), generator=g) * 3.0
    if kind == "parallel":
        p = keys[0] * 2.5
    elif kind == "antiparallel":
        p = keys[0] * -2.5
    elif kind == "near":
        p = keys[0] + 1e-3 * torch.randn((n, C), generator=g)
    elif kind == "onehot":
        p = torch.zeros((n, C))
        p[torch.arange(n), torch.randint(0, C, (n,), generator=g)] = 1.0
    else:
        assert kind == "randn", kind
    return (p * scale).contiguous(), keys.contiguous()


def reference_sequence(p, keys, T):
    """The reference's torch-op sequence (contrastive.py:512 with Normalize :881-884, sim_loss :237-243, the loop :532-535) in
    the dtype of its arguments.  ``p`` may require grad."""
    q = p.div(p.pow(2).sum(1, keepdim=True).pow(0.5))

    def sim_loss(q, k):
        similarity = torch.einsum("nc,nc->n", [q, k])
        similarity /= T
        return -similarity.mean()

    loss = sim_loss(q, keys[0])
    for i in range(1, len(keys)):
        loss += sim_loss(q, keys[i])
    loss /= len(keys)
    return loss


_sim_cache = {}


def sim_reference(n, V, C, T, scale, kind):
    """fp64: loss, df (autograd, grad_out 1) and the bounds of the module docstring.  Computed once per case and shared by the
    checks of its shape."""
    key = (n, V, C, T, scale, kind)
    if key in _sim_cache:
        return _sim_cache[key]
    if _sim_cache and next(iter(_sim_cache))[:3] != (n, V, C):
        _sim_cache.clear()                  # one shape's cases at a time: the tests walk the grid shape by shape
    p, keys = sim_inputs(n, V, C, scale, kind)
    pd = p.double().requires_grad_(True)
    kd = keys.double()
    loss = reference_sequence(pd, kd, T)
    loss.backward()
    loss, df = loss.detach(), pd.grad.detach()
    with torch.no_grad():
        x = pd.detach()
        nrm = x.pow(2).sum(1, keepdim=True).sqrt()
        q = x / nrm
        qa = q.abs()
        eq = (C / 2 + 4) * U
        s = (q.unsqueeze(0) * kd).sum(-1)                                         # (V, n)
        E_s = (1.5 * C + 8) * U * (qa.unsqueeze(0) * kd.abs()).sum(-1) / T
        E_loss = float(E_s.mean() + (n + V + 4) * U * s.abs().mean() / T)
        S = kd.sum(0)                                                             # (n, C)
        E_S = (V + 1) * U * kd.abs().sum(0)
        d = (q * S).sum(1, keepdim=True)
        E_d = (1.5 * C + 6) * U * (qa * S.abs()).sum(1, keepdim=True) + (qa * E_S).sum(1, keepdim=True)
        mag = S.abs() + (q * d).abs()
        E_df = (E_S + qa * E_d + eq * (q * d).abs() + 3 * U * mag + (eq + 6 * U) * mag) / (V * n * T * nrm)
    out = dict(p=p, keys=keys, T=T, loss=loss, df=df, E_loss=E_loss, E_df=E_df)
    _sim_cache[key] = out
    return out


def sim_ratios(r, loss, df, grad_out=1.0):
    """Deviations from the fp64 reference in units of the bounds: (loss, df); df is the gradient for ``grad_out``."""
    g = abs(grad_out)
    a = abs(float(loss.detach()) - float(r["loss"])) / r["E_loss"]
    b = float(((df.detach().cpu().double() - r["df"] * grad_out).abs() / (r["E_df"] * g + U * (r["df"] * g).abs() + 1e-300)).max())
    return a, b


def reference_fp32_ratios(n, V, C, T, scale, kind):
    """The reference's own fp32 CPU run (its torch-op sequence and autograd) in units of the bounds."""
    r = sim_reference(n, V, C, T, scale, kind)
    p = r["p"].clone().requires_grad_(True)
    loss = reference_sequence(p, r["keys"], T)
    loss.backward()
    return sim_ratios(r, loss, p.grad)


def check_reference_inside_bounds():
    """CPU: the condition on the bounds over the whole grid, and the fp64 restatement against the recorded reference results."""
    fx = fixture()["sim"]
    worst = [0.0, 0.0]
    count = 0
    for n, V, C in SIM_SHAPES:
        for T, scale, kind in sim_cases(n, V, C):
            ratios = reference_fp32_ratios(n, V, C, T, scale, kind)
            rec = fx[sim_key(n, V, C, T, scale, kind)]
            assert max(ratios) <= 1.0, (n, V, C, T, scale, kind, ratios)
            assert max(rec["reference_ratio"]) <= 1.0
            r = sim_reference(n, V, C, T, scale, kind)
            assert abs(float(r["loss"]) - rec["loss"]) <= r["E_loss"] + 1e-7 * abs(rec["loss"]), (rec["loss"], float(r["loss"]))
            idx = sample_index(n * C, 1, DF_SAMPLE)
            got = r["df"].flatten()[idx]
            want = torch.tensor(rec["df_sample"], dtype=torch.float64)
            assert bool(((got - want).abs() <= r["E_df"].flatten()[idx] + 1e-7 * want.abs()).all()), (n, V, C, T, scale, kind)
            worst = [max(w, x) for w, x in zip(worst, ratios)]
            count += 1
    assert count == len(SIM_SHAPES) * len(SIM_T) * len(SIM_SCALES) * len(SIM_KINDS) == len(fx), "a case was skipped"
    print("reference fp32 vs fp64 over %d cases: loss %.3f df %.3f of the bounds" % (count, worst[0], worst[1]))
    return worst


def _device_p(p, device, pitched):
    if not pitched:
        return p.clone().to(device).requires_grad_(True)
    n, C = p.shape
    base = torch.full((n, C + PITCH_PAD), float("nan"))
    base[:, :C] = p
    base = base.to(device).requires_grad_(True)         # a leaf; the query is a pitched view of it
    return base


def run_sim(device, r, pitched=False):
    """(loss, the leaf, the (n, C) tensor handed to byol_sim)."""
    leaf = _device_p(r["p"], device, pitched)
    C = r["p"].shape[1]
    x = leaf[:, :C] if pitched else leaf
    if pitched:
        assert x.stride(0) == C + PITCH_PAD
    loss = ct.byol_sim(x, r["keys"].to(device), r["T"])
    return loss, leaf, x


def check_sim(device, n, V, C, pitched, report=None):
    """Every (T, scale, kind, grad_out) of one shape: two launches, per-element parity, equal bits on a second call."""
    worst = [0.0, 0.0]
    count = 0
    for T, scale, kind in sim_cases(n, V, C):
        r = sim_reference(n, V, C, T, scale, kind)
        with count_calls() as calls:
            loss, leaf, x = run_sim(device, r, pitched)
        launches = [c for c in calls if c != "sf_byol_sim_workspace"]
        assert launches == ["sf_byol_sim_rows", "sf_byol_sim_finalize"] and len(launches) <= 2, calls
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss2, leaf2, _ = run_sim(device, r, pitched)
        assert torch.equal(loss.detach(), loss2.detach()), "two runs differ"
        for g in SIM_GRADS:
            (dl,) = torch.autograd.grad(loss, leaf, grad_outputs=torch.tensor(g).to(device), retain_graph=True)
            df = dl[:, :C]
            if pitched:
                assert bool((dl[:, C:] == 0).all()), "the pad columns have no gradient"
            ratios = sim_ratios(r, loss, df, g)
            if max(ratios) > 1.0 or report is not None:
                print("byol_sim %s pitched=%s g=%g: loss %.3f df %.3f of the bounds" % ((sim_key(n, V, C, T, scale, kind), pitched, g) + ratios))
            assert max(ratios) <= 1.0, (n, V, C, T, scale, kind, g, ratios)
            (dl2,) = torch.autograd.grad(loss2, leaf2, grad_outputs=torch.tensor(g).to(device), retain_graph=True)
            assert torch.equal(dl[:, :C], dl2[:, :C]), "two runs differ"
            worst = [max(w, x) for w, x in zip(worst, ratios)]
            count += 1
    assert count == len(SIM_T) * len(SIM_SCALES) * len(SIM_KINDS) * len(SIM_GRADS), "a case was skipped"
    print("byol_sim n=%d V=%d C=%d pitched=%s, %d cases: loss %.3f df %.3f of the bounds" % (n, V, C, pitched, count, worst[0], worst[1]))
    if report is not None:
        report["n%d_V%d_C%d_pitched%d" % (n, V, C, int(pitched))] = worst
    return worst


def check_sim_list_of_keys(device):
    """A list of V key matrices gives the bits of the stacked tensor; one key matrix is taken without a copy."""
    r = sim_reference(5, 3, 100, 0.5, 1.0, "randn")
    p, keys = r["p"].to(device), r["keys"].to(device)
    a = ct.byol_sim(p, keys, 0.5)
    b = ct.byol_sim(p, [keys[v] for v in range(3)], 0.5)
    assert torch.equal(a, b)
    batched = keys.reshape(15, 100)
    c = ct.byol_sim(p, [batched[5:10]], 0.5)
    assert torch.equal(c, ct.byol_sim(p, keys[1:2], 0.5))


def check_sim_zero_row(device):
    """No epsilon: a zero row is NaN in its own df row and in the loss, as the reference's Normalize gives; the other rows' df
    is finite."""
    r = sim_reference(5, 2, 100, 0.5, 1.0, "randn")
    p = r["p"].clone()
    p[3] = 0.0
    ref = p.clone().requires_grad_(True)
    ref_loss = reference_sequence(ref, r["keys"], 0.5)
    ref_loss.backward()
    assert bool(ref_loss.isnan()) and bool(ref.grad[3].isnan().all())
    x = p.to(device).requires_grad_(True)
    loss = ct.byol_sim(x, r["keys"].to(device), 0.5)
    (df,) = torch.autograd.grad(loss, x)
    df = df.cpu()
    assert bool(loss.isnan()) and bool(df[3].isnan().all())
    keep = [0, 1, 2, 4]
    assert bool(df[keep].isfinite().all())
    # the other rows are what they are without the zero row (the loss's 1 / n is the same)
    err = (df[keep].double() - sim_reference(5, 2, 100, 0.5, 1.0, "randn")["df"][keep]).abs()
    assert bool((err <= sim_reference(5, 2, 100, 0.5, 1.0, "randn")["E_df"][keep]).all())


def check_sim_rejections(device):
    """Each raises SfError before anything is allocated or written."""
    def make(n, V, C, dtype=torch.float32):
        return torch.ones((n, C), dtype=dtype).to(device), torch.ones((V, n, C), dtype=dtype).to(device)

    cases = {"V = 0": lambda: ct.byol_sim(*make(2, 0, 64), 0.5),
             "V = 0 (list)": lambda: ct.byol_sim(make(2, 1, 64)[0], [], 0.5),
             "V = 17": lambda: ct.byol_sim(*make(2, 17, 64), 0.5),
             "C = 0": lambda: ct.byol_sim(*make(2, 1, 0), 0.5),
             "C = 4097": lambda: ct.byol_sim(*make(2, 1, 4097), 0.5),
             "n = 0": lambda: ct.byol_sim(*make(0, 1, 64), 0.5),
             "keys of another n": lambda: ct.byol_sim(make(2, 1, 64)[0], make(3, 1, 64)[1], 0.5),
             "keys of another C": lambda: ct.byol_sim(make(2, 1, 64)[0], make(2, 1, 100)[1], 0.5),
             "2-D keys": lambda: ct.byol_sim(make(2, 1, 64)[0], make(2, 1, 64)[0], 0.5),
             "fp64 p": lambda: ct.byol_sim(make(2, 1, 64, torch.float64)[0], make(2, 1, 64)[1], 0.5),
             "fp16 keys": lambda: ct.byol_sim(make(2, 1, 64)[0], make(2, 1, 64, torch.float16)[1], 0.5),
             "transposed p": lambda: ct.byol_sim(make(64, 1, 2)[0].t(), make(2, 1, 64)[1], 0.5),
             "strided keys": lambda: ct.byol_sim(make(2, 1, 64)[0], make(2, 1, 128)[1][:, :, ::2], 0.5)}
    before = set(ct._byol_workspaces)
    for what, fn in cases.items():
        with count_calls() as calls:
            try:
                fn()
            except SfError:
                pass
            else:
                raise AssertionError("%s accepted" % what)
        assert [c for c in calls if c != "sf_byol_sim_workspace"] == [], (what, calls)     # no launch: nothing was written
    assert set(ct._byol_workspaces) == before, "a rejected shape left a workspace behind"
    # the limits themselves are taken
    for n, V, C in ((1, 16, 3), (2, 1, 4096), (3, 2, 1)):
        p, keys = make(n, V, C)
        loss = ct.byol_sim(p, mc._unit(keys), 0.5)
        want = reference_sequence(p.cpu().double(), mc._unit(keys).cpu().double(), 0.5)
        assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (n, V, C, float(loss), float(want))


def check_rejects_host_tensors():
    """With the gfx950 library loaded, host tensors are refused (no torch fallback)."""
    try:
        ct.byol_sim(torch.randn(2, 64), torch.randn(1, 2, 64), 0.5)
    except SfError as e:
        assert "need CUDA/HIP tensors" in str(e)
    else:
        raise AssertionError("a host tensor was accepted by the gfx950 library")
    try:
        ct.byol_sim(torch.randn(2, 64).cuda(), torch.randn(1, 2, 64), 0.5)
    except SfError as e:
        assert "do not match" in str(e)
    else:
        raise AssertionError("host keys were accepted beside a device query")


# ------------------------------------------------------------------------------------------------ capture (GPU)
def check_capture(device, n=8, V=2, C=100, size=4097, iters=3):
    """EMA -> loss -> gradient of the loss on one stream, captured once and replayed with a new momentum each time, against
    the same three iterations run eagerly: hist, loss and df bit for bit."""
    p0, keys = sim_inputs(n, V, C, 1.0, "randn")
    w0, h0 = mc.ema_inputs(size)
    ms = (0.5, 0.996, 0.999)
    T = 0.5

    def state():
        return dict(p=p0.to(device).requires_grad_(True), keys=keys.to(device), w=w0.to(device), h=h0.to(device),
                    mm=ct.momentum_words(ms[0]).to(device))

    def step(s):
        ct.ema_update(s["w"], s["h"], s["mm"])
        loss = ct.byol_sim(s["p"], s["keys"], T)
        (df,) = torch.autograd.grad(loss, s["p"])
        return loss, df

    eager, e_out = state(), []
    for it in range(iters):
        eager["mm"].copy_(ct.momentum_words(ms[it]).to(device))
        loss, df = step(eager)
        e_out.append((loss.detach().clone(), df.clone(), eager["h"].clone()))
    cap = state()
    ct._byol_workspace(device, n, V, C)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):          # warm-up off the default stream, then restore the state it touched
        step(cap)
    torch.cuda.current_stream(device).wait_stream(side)
    cap["h"].copy_(h0.to(device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_loss, c_df = step(cap)
    cap["h"].copy_(h0.to(device))
    for it in range(iters):
        cap["mm"].copy_(ct.momentum_words(ms[it]).to(device))
        graph.replay()
        assert torch.equal(c_loss, e_out[it][0]) and torch.equal(c_df, e_out[it][1]) and torch.equal(cap["h"], e_out[it][2]), it
    torch.cuda.synchronize(device)
    assert torch.equal(cap["h"], eager["h"])


# ------------------------------------------------------------------------------------------------ heads
BYOL_OPTS = ["CONTRASTIVE.TYPE", "byol", "CONTRASTIVE.NUM_MLP_LAYERS", 2, "CONTRASTIVE.BN_MLP", True,
             "CONTRASTIVE.BN_SYNC_MLP", True, "CONTRASTIVE.PREDICTOR_DEPTHS", "[2]", "CONTRASTIVE.T", 0.5,
             "CONTRASTIVE.MOMENTUM", 0.996, "CONTRASTIVE.MOMENTUM_ANNEALING", True, "CONTRASTIVE.SEQUENTIAL", True,
             "DATA.TRAIN_CROP_NUM_TEMPORAL", 2, "SOLVER.MAX_EPOCH", 200]
MODEL_OPTS = mc.MODEL_OPTS + BYOL_OPTS     # later keys win: the MoCo keys of moco_checks.MODEL_OPTS are overridden
CROPS, BATCH = 2, 4
EPOCHS = (0.0, 37.5, 150.25)               # epoch_exact of the three iterations: the cosine annealing moves the momentum
SEQUENTIAL = (True, True, False)


def model_cfg(extra=()):
    return sa.get_preset("SLOW_8x8_R50", MODEL_OPTS + list(extra))


def check_heads(device):
    from slowfast_amd.heads import MLPHead, ResNetBasicHead
    cfg = model_cfg()
    torch.manual_seed(5)
    head = ResNetBasicHead([32], 64, [None], cfg=cfg).to(device).train()
    kinds = ["Linear", "BatchNorm1d", "ReLU", "Linear"]
    assert isinstance(head.projection, MLPHead) and [type(m).__name__ for m in head.projection.projection] == kinds
    assert isinstance(head.predictors, torch.nn.ModuleList) and len(head.predictors) == 1
    assert isinstance(head.predictors[0], MLPHead) and [type(m).__name__ for m in head.predictors[0].projection] == kinds
    names = ["%s.projection.%s" % (top, s) for top in ("predictors.0", "projection")
             for s in ("0.weight", "1.bias", "1.weight", "3.bias", "3.weight")]
    assert sorted(k for k, _ in head.named_parameters()) == names, sorted(k for k, _ in head.named_parameters())
    shapes = {k: tuple(v.shape) for k, v in head.named_parameters()}
    assert shapes["projection.projection.0.weight"] == (32, 32) and shapes["projection.projection.3.weight"] == (64, 32)
    assert shapes["predictors.0.projection.0.weight"] == (32, 64) and shapes["predictors.0.projection.3.weight"] == (64, 32)
    x = torch.randn(4, 32, 2, 3, 3, generator=torch.Generator().manual_seed(6)).to(device)
    out = head([x])
    assert isinstance(out, list) and len(out) == 2 and all(tuple(o.shape) == (4, 64) for o in out)
    pooled = x.float().mean((2, 3, 4))
    assert torch.equal(out[1], head.predictors[0](out[0]))
    assert torch.allclose(out[0], head.projection(pooled), rtol=1e-5, atol=1e-6)
    out[1].sum().backward()
    assert all(p.grad is not None for p in head.parameters())
    # without predictors: a tensor, and no parameter under `predictors`
    cfg1 = model_cfg(["CONTRASTIVE.PREDICTOR_DEPTHS", "[]", "CONTRASTIVE.TYPE", "moco", "CONTRASTIVE.BN_SYNC_MLP", False])
    h1 = ResNetBasicHead([32], 64, [None], cfg=cfg1).to(device).train()
    assert torch.is_tensor(h1([x])) and len(h1.predictors) == 0 and not any("predictors" in k for k in h1.state_dict())
    # BatchNorm statistics shared between devices are not built
    for kw in (dict(bn_sync_num=2), dict(global_sync=True), dict(bn_sync_num=2, global_sync=True)):
        try:
            MLPHead(8, 8, 8, 2, bn_on=True, **kw)
        except NotImplementedError as e:
            assert "BN_SYNC_MLP" in str(e)
        else:
            raise AssertionError("MLPHead(%r) accepted" % (kw,))
    assert isinstance(MLPHead(8, 8, 8, 2, bn_on=True, bn_sync_num=1).projection[1], torch.nn.BatchNorm1d)


# ------------------------------------------------------------------------------------------------ the model
PARAM_SEED, DATA_SEED = 81, 82
PERTURB = mc.PERTURB


def seeded_state(shapes, K, dim):
    from oracle import video_ref
    sd = video_ref.randomize_state({k: s for k, s in shapes.items() if k not in ("ptr", "iter", "queue_x")}, PARAM_SEED)
    g = torch.Generator().manual_seed(PARAM_SEED + 1)
    stdv = 1.0 / math.sqrt(dim / 3)
    sd["queue_x"] = torch.rand((K, dim), generator=g).mul_(2 * stdv).add_(-stdv)
    sd["ptr"] = torch.tensor([0])
    sd["iter"] = torch.zeros([1], dtype=torch.long)
    for k in list(sd):                      # the key encoder starts from other weights than the query encoder: the iteration-0
        if k.startswith("backbone_hist.") and sd[k].is_floating_point() and "running" not in k:   # copy must show
            sd[k] = sd[k] * 0.5
    return sd


def model_inputs(cfg, it):
    g = torch.Generator().manual_seed(DATA_SEED + it)
    shape = (BATCH, 3, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_CROP_SIZE)
    return [[torch.randn(shape, generator=g)] for _ in range(CROPS)]


def drive(model, cfg, device, forward_fn, perturb):
    """Two iterations of contrastive_forward with CONTRASTIVE.SEQUENTIAL, then one of the symmetric form, as the golden tool
    drives the reference: per iteration the loss, the gradient norm over the backbone, the preds, perform_backward and the
    buffers.  ``perturb(model)`` scales the query encoder between iterations (an exact fp32 operation)."""
    out = []
    index = torch.arange(BATCH).to(device)
    time = torch.zeros((BATCH, CROPS, 2)).to(device)
    for it, (epoch, seq) in enumerate(zip(EPOCHS, SEQUENTIAL)):
        cfg.CONTRASTIVE.SEQUENTIAL = seq
        model.zero_grad(set_to_none=True)
        inputs = [[x.to(device) for x in clip] for clip in model_inputs(cfg, it)]
        _, preds, loss, perform_backward = forward_fn(model, cfg, inputs, index, time, epoch)
        if perform_backward:
            loss.backward()
        grads = [p.grad.detach().float().cpu() for p in model.parameters() if p.grad is not None]
        gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads)))
        sd = model.state_dict()
        out.append(dict(loss=float(loss.detach()), grad_norm=gn, perform_backward=bool(perform_backward), preds=preds.detach().float().cpu(),
                        iter=int(sd["iter"]), ptr=int(sd["ptr"]), queue_sha256=digest(sd["queue_x"]), mmt=float(model.mmt),
                        grads=len(grads)))
        perturb(model)
    cfg.CONTRASTIVE.SEQUENTIAL = True
    return out


def perturb_backbone(model):
    with torch.no_grad():
        for p in model.backbone.parameters():
            p.data.mul_(PERTURB)
    engine.PARAM_EPOCH += 1


def build_model(device, extra=()):
    cfg = model_cfg(extra)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    model.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, cfg.CONTRASTIVE.QUEUE_LEN,
                                       cfg.CONTRASTIVE.DIM))
    return cfg, model.to(device).train()


def check_state_dict(device):
    rec = fixture()["model"]
    cfg, model = build_model(device)
    assert state_list(model.state_dict()) == rec["state"]
    assert list(model.state_dict()) == rec["state_order"], "state_dict() lists its entries in the reference's order"
    keys = set(model.state_dict())
    for top in ("backbone", "backbone_hist"):
        for s in ("0.weight", "1.weight", "1.bias", "1.running_mean", "1.running_var", "1.num_batches_tracked", "3.weight", "3.bias"):
            assert "%s.head.predictors.0.projection.%s" % (top, s) in keys
    assert {"ptr", "queue_x", "iter"} <= keys and not model._batch_shuffle_on
    assert not any(p.requires_grad for p in model.backbone_hist.parameters())


def check_model(device, report=None):
    rec = fixture()["model"]
    cfg, model = build_model(device)
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with count_calls() as calls:
        runs = drive(model, cfg, device, ct.contrastive_forward, perturb_backbone)
    # per iteration: one byol_sim per query (two launches each), and never an enqueue
    assert calls.count("sf_byol_sim_rows") == calls.count("sf_byol_sim_finalize") == 2 * len(runs), calls.count("sf_byol_sim_rows")
    assert "sf_queue_enqueue" not in calls and "sf_moco_nce_slabs" not in calls
    b = mc.model_bounds()
    res = []
    K = cfg.CONTRASTIVE.QUEUE_LEN
    for it, (got, want) in enumerate(zip(runs, rec["iterations"])):
        r = dict(loss=abs(got["loss"] - want["loss"]) / max(1.0, abs(want["loss"])),
                 grad_norm=abs(got["grad_norm"] - want["grad_norm"]) / want["grad_norm"])
        print("byol tiny model, iteration %d (sequential %s): loss %.6f (reference %.6f) grad_norm %.6f (%.6f): %s (bounds %s)" % (
            it, SEQUENTIAL[it], got["loss"], want["loss"], got["grad_norm"], want["grad_norm"], r, {k: b[k] for k in r}))
        res.append(r)
        for k, v in r.items():
            assert v <= b[k], (it, k, v, b[k])
        assert got["perform_backward"] == want["perform_backward"] == (not SEQUENTIAL[it])
        assert got["iter"] == want["iter"] == it + 1 and got["ptr"] == want["ptr"] == 0
        assert got["queue_sha256"] == want["queue_sha256"] == digest(sd0["queue_x"]), "byol never writes the queue"
        assert got["mmt"] == want["mmt"] and got["grads"] == want["grads"]
        rows = BATCH * (CROPS if SEQUENTIAL[it] else 1)
        assert list(got["preds"].shape) == want["preds_shape"] == [rows, 1 + K]
        assert bool((got["preds"][:, 0] == 9999.0).all()) and bool((got["preds"][:, 1:] == 0).all())
    assert len(runs) == len(rec["iterations"]) == 3
    if report is not None:
        report["model"] = res
    assert model._iter_host == 3
    # exact: the key encoder's parameters (an EMA of exact inputs under the annealed momentum)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    hist = {k: v for k, v in sd.items() if k.startswith("backbone_hist.") and k in dict(model.named_parameters())}
    assert len(hist) == len(rec["hist_sha256"])
    for k, v in hist.items():
        assert digest(v) == rec["hist_sha256"][k], k
    # the heads' BatchNorm1d layers count their own batches (torch's forward), once per pass
    tracked = {k: int(v) for k, v in sd.items() if k.endswith("num_batches_tracked") and ".head." in k}
    assert tracked == rec["batches_tracked"] and len(tracked) == 4, tracked


def check_model_surface(device):
    """What needs the query encoder alone: the cached dummy logits, compute_predictor_keys, the projection for index None, a
    forward with given keys (no momentum update), the kNN memory under KNN_ON, eval."""
    a = ct.dummy_logits(4, 48, device)
    assert a is ct.dummy_logits(4, 48, device) and a is not ct.dummy_logits(8, 48, device)
    assert tuple(a.shape) == (4, 49) and not a.requires_grad
    assert bool((a[:, 0] == 9999.0).all()) and bool((a[:, 1:] == 0).all())
    cfg, model = build_model(device, ["CONTRASTIVE.KNN_ON", True, "CONTRASTIVE.LENGTH", 256])
    clip = [x.to(device) for x in model_inputs(cfg, 0)[0]]
    try:
        model.compute_key_feat([clip], compute_predictor_keys=True)
    except NotImplementedError as e:
        assert "compute_predictor_keys" in str(e)
    else:
        raise AssertionError("compute_predictor_keys=True accepted")
    with torch.no_grad():
        proj = model(clip)                  # index None: the projection
    assert torch.is_tensor(proj) and tuple(proj.shape) == (BATCH, cfg.CONTRASTIVE.DIM)
    assert int(model.iter) == 0
    # KNN_ON: the memory bank takes the normalised projection at `index`; eval returns eval_knn of it
    index = torch.tensor([3, 200, 17, 255]).to(device)
    keys = [k.to(device) for k in sim_inputs(BATCH, 1, cfg.CONTRASTIVE.DIM, 1.0, "randn")[1]]
    mem0 = model.knn_mem.memory.detach().clone()
    with count_calls() as calls:
        logits, loss = model([clip], index, None, None, keys=keys)
    assert "sf_ema_update" not in calls and calls.count("sf_byol_sim_rows") == 1 and int(model.iter) == 0      # keys were given
    assert logits is ct.dummy_logits(BATCH, cfg.CONTRASTIVE.QUEUE_LEN, device) and loss.requires_grad
    q = mc._unit(proj.float())              # the same batch in training mode: the same projection
    rows = model.knn_mem.memory[index, 0]
    assert float((rows - q).abs().max()) < 1e-5, float((rows - q).abs().max())
    untouched = torch.ones(256, dtype=torch.bool)
    untouched[index.cpu()] = False
    assert torch.equal(model.knn_mem.memory[untouched.to(device)], mem0[untouched.to(device)])
    model.eval()
    yd, yi = model(clip, index)
    assert tuple(yd.shape) == tuple(yi.shape) == (BATCH, 200) and bool((yd[:, :-1] >= yd[:, 1:]).all())


def check_bound_flat_matches_per_tensor(device):
    """bind_flat(): the key encoder's parameters (the predictor's among them) after the iteration-0 copy and two updates, the
    second under an annealed momentum, by ONE launch each over the flat buffers, have the bits of the per-tensor path."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    outs = []
    for bound in (False, True):
        cfg, model = build_model(device)
        if bound:
            reducer = GradReducer(model)
            opt = construct_optimizer(model, cfg, reducer)
            model.bind_flat(opt)
        names = [n for n, _ in model.backbone_hist.named_parameters()]
        assert any("head.predictors.0" in n for n in names)
        model.mmt = 0.996
        with count_calls() as calls:
            model._update_history()
        assert calls.count("sf_ema_update") == (1 if bound else len(names)), calls
        model._iter_host = 1
        perturb_backbone(model)
        model.momentum_anneal_cosine(37.5)
        model._update_history()
        outs.append({n: h.detach().cpu().clone() for n, h in model.backbone_hist.named_parameters()})
        if bound:
            engine.remove_grad_ready_listener(reducer._listener)
    for n in outs[0]:
        assert torch.equal(outs[0][n], outs[1][n]), n


# ------------------------------------------------------------------------------------------------ recipe plumbing, rejections
def check_recipe():
    """The BYOL_SlowR50_8x8 preset: build_model, construct_optimizer (LARS), bind_flat, the parameter surgery.  Construction
    only: no forward at recipe size."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import FlatOptimizer, construct_optimizer
    cfg = sa.get_preset("BYOL_SlowR50_8x8", ["NUM_GPUS", 0])
    c = cfg.CONTRASTIVE
    assert (c.TYPE, c.T, c.DIM, c.NUM_MLP_LAYERS, c.MLP_DIM, list(c.PREDICTOR_DEPTHS)) == ("byol", 0.5, 256, 2, 4096, [2])
    assert c.BN_MLP and c.BN_SYNC_MLP and c.SEQUENTIAL and c.MOMENTUM == 0.996 and c.MOMENTUM_ANNEALING
    assert cfg.MODEL.NUM_CLASSES == 256 and cfg.MODEL.ARCH == "slow" and cfg.TASK == "ssl"
    assert cfg.DATA.TRAIN_CROP_NUM_TEMPORAL == 2 and cfg.DATA.SSL_COLOR_JITTER and cfg.DATA.SSL_MOCOV2_AUG
    assert cfg.BN.NORM_TYPE == "sync_batchnorm" and cfg.BN.NUM_SYNC_DEVICES == 1
    s = cfg.SOLVER
    assert s.LARS_ON and s.LR_POLICY == "cosine" and s.WARMUP_EPOCHS == 35.0 and s.WEIGHT_DECAY == 1e-6 and s.BASE_LR == 0.6
    assert sa.get_preset("BYOL_SlowR50_8x8").NUM_GPUS == 1
    model = sa.build_model(cfg)
    assert type(model).__name__ == "ContrastiveModel" and model.type == "byol" and not model._batch_shuffle_on
    head = model.backbone.head
    assert [type(m).__name__ for m in head.predictors[0].projection] == ["Linear", "BatchNorm1d", "ReLU", "Linear"]
    assert tuple(head.predictors[0].projection[0].weight.shape) == (4096, 256)
    assert tuple(head.projection.projection[0].weight.shape) == (4096, 2048)
    reducer = GradReducer(model)
    try:
        opt = construct_optimizer(model, cfg, reducer)
        assert isinstance(opt, FlatOptimizer) and opt.lars
        model.bind_flat(opt)
        flat, hist_flat = model._flat
        assert flat.numel() == hist_flat.numel() == sum(p.numel() for p in model.backbone.parameters())
        lo, hi = hist_flat.data_ptr(), hist_flat.data_ptr() + 4 * hist_flat.numel()
        for n, h in model.backbone_hist.named_parameters():         # every history parameter is a view of the flat buffer
            assert lo <= h.data_ptr() < hi and h.data.is_contiguous(), n
    finally:
        engine.remove_grad_ready_listener(reducer._listener)
    assert ct.contrastive_parameter_surgery(model, cfg, 0.0, 0) == (model, True)
    assert ct.contrastive_parameter_surgery(model, cfg, 1.5, 7)[1] is True


REJECTED = ((["CONTRASTIVE.PREDICTOR_DEPTHS", "[]"], "CONTRASTIVE.TYPE"),
            (["CONTRASTIVE.PREDICTOR_DEPTHS", "[2, 2]"], "PREDICTOR_DEPTHS"),
            (["BN.NUM_SYNC_DEVICES", 2], "BN_SYNC_MLP"), (["BN.GLOBAL_SYNC", True], "BN_SYNC_MLP"),
            (["NUM_GPUS", 2], "NUM_GPUS"), (["NUM_SHARDS", 2], "NUM_GPUS"), (["MODEL.ARCH", "x3d"], "MODEL.ARCH"))


def check_rejections():
    for extra, key in REJECTED:
        try:
            sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(extra))
        except NotImplementedError as e:
            assert key in str(e), (extra, str(e))
            if not list(model_cfg(extra).CONTRASTIVE.PREDICTOR_DEPTHS):
                assert "predictor is missing" in str(e)
        else:
            raise AssertionError("%r accepted" % (extra,))
    for typ in ("mem", "self", "swav", "simclr"):
        try:
            sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(["CONTRASTIVE.TYPE", typ]))
        except NotImplementedError as e:
            assert "CONTRASTIVE.TYPE" in str(e)
        else:
            raise AssertionError("%r accepted" % (typ,))
