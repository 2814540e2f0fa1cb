"""Checks of the MaskFeat path (slowfast_amd/masked.py, masking.py, csrc/sf_hog.h, the mask-token kernels of csrc/sf_tokens.h),
shared by the GPU tests (tests/test_maskfeat_gpu.py) and their host-simulator twins (tests/test_maskfeat_hostsim.py).

References.  The HOG kernel is compared per cell with the fp64 restatement of its arithmetic below (``hog_restate``) and with the
bytes the unmodified reference produced (tests/golden/maskfeat_contract.json, recorded by tools/make_maskfeat_golden.py); the
mask-token kernels with fp64 autograd; the model with the reference's own fp32 run: elementwise through ``oracle_run``, a torch
restatement on the blocks of oracle/mvit_ref.py that is itself pinned to the reference's recorded loss, gradient norm, sampled
predictions and (norm, projection) of every parameter gradient -- the full tensors would be 4 MB of fixture.  Inputs are drawn from the
seeds the fixture names.
"""
import base64
import json
import math
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

import slowfast_amd as sa
from slowfast_amd import lib as sflib
from slowfast_amd import masked, masking, tokens
from slowfast_amd.lib import SfError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskfeat_contract.json")
_fixture = None
PROBE_SEED, SAMPLE = 51, 512


def fixture():
    global _fixture
    if _fixture is None:
        with open(GOLDEN) as f:
            _fixture = json.load(f)
    return _fixture


def table_digest(table):
    """SHA-256 of a mask table's bytes (equal digests are equal bytes; the tables themselves would be 50 KB of fixture)."""
    import hashlib
    return hashlib.sha256(table.contiguous().numpy().tobytes()).hexdigest()


def sample_index(numel, seed, count):
    """Seeded element sample of a recorded tensor: all of a small one, ``count`` drawn positions of a large one."""
    if numel <= count:
        return torch.arange(numel)
    return torch.randperm(numel, generator=torch.Generator().manual_seed(seed))[:count]


def grad_probe(k, g, seed=PROBE_SEED):
    """(norm, projection on a seeded random direction) of one parameter gradient: two numbers that pin the whole tensor."""
    d = torch.randn(g.numel(), generator=torch.Generator().manual_seed(seed + sum(k.encode())), dtype=torch.float64)
    return [float(g.double().norm()), float(g.double().flatten() @ d)]


def f32_bytes(t):
    return base64.b64encode(t.detach().cpu().float().contiguous().numpy().tobytes()).decode()


def f32_from(s, shape=None):
    a = np.frombuffer(base64.b64decode(s), dtype=np.float32).copy()
    t = torch.from_numpy(a)
    return t.view(shape) if shape is not None else t


# ---------------------------------------------------------------------------------------------------------------------------
# 1. masks
MASK_CASES = (
    dict(name="cube", window=[8, 7, 7], ratio=0.4, tube=False, frames=False, seeds=(0, 1, 7), draws=3),
    dict(name="cube_small", window=[4, 4, 4], ratio=0.4, tube=False, frames=False, seeds=(3,), draws=4),
    dict(name="tube", window=[14, 14], ratio=0.4, tube=True, frames=False, seeds=(0, 5), draws=3),
    dict(name="frames", window=[8, 7, 7], ratio=0.4, tube=False, frames=True, seeds=(0, 9), draws=3),
)


def mask_cfg(case):
    cfg = sa.get_cfg()
    cfg.AUG.GEN_MASK_LOADER = True
    cfg.AUG.MASK_WINDOW_SIZE = list(case["window"])
    cfg.AUG.MASK_RATIO = case["ratio"]
    cfg.AUG.MASK_TUBE, cfg.AUG.MASK_FRAMES = case["tube"], case["frames"]
    return cfg


def check_masks():
    fx = fixture()["masks"]
    for case in MASK_CASES:
        for seed in case["seeds"]:
            rec = fx["%s/%d" % (case["name"], seed)]
            random.seed(seed)
            gen = masking.construct_mask_generator(mask_cfg(case))
            table = gen.sample_batch(case["draws"])
            after = random.random()
            assert table.dtype == torch.uint8 and list(table.shape) == rec["shape"], (case["name"], table.shape)
            assert int(table.sum()) == rec["masked"] and table_digest(table) == rec["sha256"], (case["name"], seed)
            assert after == rec["random_after"], (case["name"], seed)
    assert masking.construct_mask_generator(sa.get_cfg()) is None


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. HOG targets
HOG_CASES = (
    dict(name="u2", B=2, T=4, ts=2, S=32, fs=2, seed=11),
    dict(name="u1", B=1, T=2, ts=1, S=16, fs=2, seed=12),
    dict(name="u3_oddT", B=1, T=3, ts=2, S=48, fs=2, seed=13),
    dict(name="real_width", B=1, T=2, ts=2, S=224, fs=14, seed=14),
    dict(name="flat", B=1, T=1, ts=1, S=32, fs=2, seed=15, flat=(7, 25, 0.37)),
    # u 8: a token row is split into chunks of 4 + 1 tokens (halo columns between workgroups, a partial last chunk) and the
    # staged output takes the large-LDS variant of the kernel
    dict(name="chunked", B=1, T=1, ts=1, S=320, fs=5, seed=16),
)
HOG_TOL = 2.0 ** -17            # 64 non-negative terms of a few ulp each, on values in [0, 1]
HOG_MAX_AMBIGUOUS = 0.02


def hog_input(case):
    g = torch.Generator().manual_seed(case["seed"])
    x = torch.randn((case["B"], 3, case["T"], case["S"], case["S"]), generator=g, dtype=torch.float32)
    if "flat" in case:
        lo, hi, v = case["flat"]
        x[..., lo:hi, lo:hi] = v
    return x


def _to_tokens(h, fs):
    """(B, 3, Tu, K, Hc, Wc) per-cell values -> (B, Tu*fs*fs, 3*K*u*u) in the per-token order."""
    B, C, Tu, K, Hc, Wc = h.shape
    u = Hc // fs
    return h.reshape(B, C, Tu, K, fs, u, fs, u).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, Tu * fs * fs, C * K * u * u)


def hog_restate(x, ts, fs):
    """fp64 restatement of csrc/sf_hog.h on a float32 (B, 3, T, H, W) clip -> dict(out (B, N, 27uu) fp64, ambiguous (B, N, 27uu)
    bool per-cell mask in the same layout, bin (pixel bins), gx, gy)."""
    xs = x[:, :, ::ts].double()
    B, C, Tu, H, W = xs.shape
    xp = F.pad(xs.reshape(B * C * Tu, 1, H, W), (1, 1, 1, 1), mode="reflect")[:, 0]
    win = lambda r, c: xp[:, r:r + H, c:c + W]                                  # noqa: E731
    gx = (win(0, 0) - win(0, 2)) + 2.0 * (win(1, 0) - win(1, 2)) + (win(2, 0) - win(2, 2))
    gy = (win(0, 0) - win(2, 0)) + 2.0 * (win(0, 1) - win(2, 1)) + (win(0, 2) - win(2, 2))
    norm = torch.sqrt(gx * gx + gy * gy)
    phase = torch.atan2(gx, gy) / math.pi * 9.0
    bins = torch.floor(phase).long() % 9
    bins = torch.where(gx == 0, torch.zeros_like(bins), bins)
    ax = win(0, 0).abs() + win(0, 2).abs() + 2.0 * (win(1, 0).abs() + win(1, 2).abs()) + win(2, 0).abs() + win(2, 2).abs()
    ay = win(0, 0).abs() + win(2, 0).abs() + 2.0 * (win(0, 1).abs() + win(2, 1).abs()) + win(0, 2).abs() + win(2, 2).abs()
    E = 8.0 * 2.0 ** -24 * torch.maximum(ax, ay)
    delta = (9.0 / math.pi) * math.sqrt(2.0) * E / norm.clamp(min=1e-300) + 2e-5
    amb = (gx != 0) & (norm > 0) & ((phase - torch.round(phase)).abs() < delta)
    hist = torch.zeros((B * C * Tu, 9, H, W), dtype=torch.float64)
    hist.scatter_add_(1, bins[:, None], norm[:, None])
    Hc, Wc = H // 8, W // 8
    hist = hist.reshape(-1, 9, Hc, 8, Wc, 8).sum((3, 5))
    hist = hist / hist.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-12)
    amb_c = amb.reshape(-1, 1, Hc, 8, Wc, 8).any(5).any(3).expand(-1, 9, -1, -1)
    shape6 = (B, C, Tu, 9, Hc, Wc)
    return dict(out=_to_tokens(hist.reshape(shape6), fs), ambiguous=_to_tokens(amb_c.reshape(shape6), fs),
                bins=bins.reshape(B, C, Tu, H, W), gx=gx.reshape(B, C, Tu, H, W), norm=norm.reshape(B, C, Tu, H, W))


_restate_cache = {}


def hog_reference(case):
    """(input, restatement) of a case, computed once and shared."""
    if case["name"] not in _restate_cache:
        x = hog_input(case)
        _restate_cache[case["name"]] = (x, hog_restate(x, case["ts"], case["fs"]))
    return _restate_cache[case["name"]]


def run_hog(device, x, ts, fs):
    """The launch into a sentinel-guarded buffer -> (out on the host, guard intact)."""
    B, _, T, S, _ = x.shape
    Tu, u = (T + ts - 1) // ts, S // 8 // fs
    n = B * Tu * fs * fs * 27 * u * u
    guard = 1024
    buf = torch.full((n + 2 * guard,), -12345.0, dtype=torch.float32, device=device)
    out = buf[guard:guard + n].view(B, Tu * fs * fs, 27 * u * u)
    res = masked.hog_targets(x.to(device), ts, fs, out=out)
    assert res.data_ptr() == out.data_ptr()
    host = buf.cpu()
    assert bool((host[:guard] == -12345.0).all()) and bool((host[guard + n:] == -12345.0).all()), "wrote outside the output"
    return host[guard:guard + n].view(out.shape).clone()


def check_hog_case(device, name):
    """Per-cell fp64 parity, determinism, the sentinel and (flat case) the exact zeros."""
    case = {c["name"]: c for c in HOG_CASES}[name]
    x, ref = hog_reference(case)
    out = run_hog(device, x, case["ts"], case["fs"])
    again = run_hog(device, x, case["ts"], case["fs"])
    assert torch.equal(out, again), "two launches on the same input differ"
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    B, N, Fd = out.shape
    u = case["S"] // 8 // case["fs"]
    cells = out.view(B, N, 3, 9, u, u)
    assert float(cells.double().pow(2).sum(3).sqrt().max()) <= 1.0 + 1e-5
    amb = ref["ambiguous"]
    frac = float(amb.float().mean())
    err = float(((out.double() - ref["out"]).abs() * (~amb)).max())
    print("hog %s: ambiguous cells %.4f (cap %.2f), max |kernel - fp64| on the others %.3e (bound %.3e)"
          % (name, frac, HOG_MAX_AMBIGUOUS, err, HOG_TOL))
    assert frac <= HOG_MAX_AMBIGUOUS, frac
    assert err <= HOG_TOL, err
    if "flat" in case:
        lo, hi, _ = case["flat"]
        # cells wholly inside the constant region, one pixel away from its edge: exact zeros
        c0, c1 = (lo + 1 + 7) // 8, (hi - 1) // 8
        assert c1 > c0
        grid = out.view(B, 1, case["fs"], case["fs"], 3, 9, u, u).permute(0, 1, 4, 5, 2, 6, 3, 7).reshape(
            B, 3, 9, case["S"] // 8, case["S"] // 8)
        assert bool((grid[:, :, :, c0:c1, c0:c1] == 0).all()), "flat cells are not exact zeros"
        # differences first: every pixel whose gx is exactly 0 (frame border columns, the flat region and its rows) lands in
        # bin 0 -- a cell whose pixels ALL have gx == 0 has nothing outside bin 0
        gx0 = (ref["gx"] == 0)
        assert bool(gx0[..., :, 0].all()) and bool(gx0[..., :, -1].all()) and bool(gx0[..., lo + 1:hi - 1, lo + 1:hi - 1].all())
        allzero = gx0.reshape(B, 3, 1, case["S"] // 8, 8, case["S"] // 8, 8).all(6).all(4)[:, :, 0]        # (B, 3, Hc, Wc)
        other = grid[:, :, 1:].abs().sum(2)
        assert bool((other[allzero] == 0).all())
    return frac, err


def check_hog_recorded(device, name):
    """Against the bytes of the unmodified reference (row and feature order pinned by the reference itself).  The fixture keeps
    a seeded sample of SAMPLE elements of the larger outputs, drawn over all rows and features; the recording tool compared
    EVERY element of the reference's output with the fp64 restatement (reference_deviation), as check_hog_case does for the
    kernel."""
    case = {c["name"]: c for c in HOG_CASES}[name]
    rec = fixture()["hog"][name]
    x, ref = hog_reference(case)
    out = run_hog(device, x, case["ts"], case["fs"])
    assert list(out.shape) == rec["shape"]
    idx = sample_index(out.numel(), case["seed"], SAMPLE)          # the recorded elements (all of them for a small case)
    want = f32_from(rec["out"])
    amb = ref["ambiguous"]
    assert int(amb.sum()) == rec["ambiguous_elements"], "the ambiguity rule moved since the fixture was recorded"
    err = float(((out.flatten()[idx].double() - want.double()).abs() * (~amb.flatten()[idx])).max())
    bound = HOG_TOL + rec["reference_deviation"]
    print("hog %s vs recorded reference (%d of %d elements): %.3e (bound %.3e, reference's own deviation %.3e)"
          % (name, idx.numel(), out.numel(), err, bound, rec["reference_deviation"]))
    assert rec["reference_deviation"] <= 1e-6
    assert err <= bound, err


# ---------------------------------------------------------------------------------------------------------------------------
# 4. mask tokens
def _mask_table_cases(device):
    """Window [2, 2, 2] tables for tokens 2x4x4: B 2 with one all-masked and one unmasked sample, and B 4 with two partly
    masked samples behind them."""
    g = torch.Generator().manual_seed(21)
    m = torch.zeros((4, 2, 2, 2), dtype=torch.uint8)
    m[0] = 1
    m[2] = (torch.rand((2, 2, 2), generator=g) < 0.5).to(torch.uint8)
    m[3] = (torch.rand((2, 2, 2), generator=g) < 0.5).to(torch.uint8)
    return [m[:2].contiguous().to(device), m.to(device)]


def _token_mask(m, thw):
    T, H, W = thw
    ih = (torch.arange(H, device=m.device) * m.shape[2]) // H
    iw = (torch.arange(W, device=m.device) * m.shape[3]) // W
    full = m[:, :, ih][:, :, :, iw]
    ref = F.interpolate(m.float(), size=(H, W))                 # the reference's nearest-neighbour map
    assert torch.equal(full.float(), ref)
    return full.flatten(1).bool()


def check_mask_tokens(device, use_pos, cls):
    for m in _mask_table_cases(device):
        _check_mask_tokens(device, use_pos, cls, m)


def _check_mask_tokens(device, use_pos, cls, m):
    act = sflib.act_dtype()
    thw, C = (2, 4, 4), 32
    N = thw[0] * thw[1] * thw[2]
    B = m.shape[0]
    g = torch.Generator().manual_seed(22 + 2 * int(use_pos) + cls)
    x0 = torch.randn((B, cls + N, C), generator=g).to(act).to(device)
    tok = (torch.randn((1, 1, C), generator=g) * 0.5).to(device).requires_grad_(True)
    pos = (torch.randn((1, cls + N, C), generator=g) * 0.5).to(device).requires_grad_(True) if use_pos else None
    dy = torch.randn((B, cls + N, C), generator=g).to(act).to(device)
    rows = _token_mask(m, thw)                                   # (B, N) bool

    class _Leaf(torch.autograd.Function):                       # x as a differentiable non-leaf the op may overwrite
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g_):
            return g_

    xin = x0.clone().requires_grad_(True)
    y = tokens.MaskTokenFn.apply(_Leaf.apply(xin), m, thw, cls, tok, pos)
    # forward: bit for bit act(mask_token + pos_row) on masked rows, untouched elsewhere (cls row included)
    want = x0.clone()
    sub = tok.detach().float().view(1, 1, C).expand(B, N, C)
    if use_pos:
        sub = sub + pos.detach().float()[:, cls:]
    want[:, cls:][rows] = sub.to(act)[rows]
    assert torch.equal(y.detach(), want)
    y.backward(dy)
    # backward against fp64 autograd of x * (1 - m) + tok * m + pos
    x64 = x0.double().requires_grad_(True)
    t64 = tok.detach().double().requires_grad_(True)
    p64 = pos.detach().double().requires_grad_(True) if use_pos else None
    mf = rows.double().unsqueeze(-1)
    body = x64[:, cls:] * (1 - mf) + t64 * mf
    y64 = torch.cat([x64[:, :cls], body], 1)
    if use_pos:
        y64 = y64 + p64 * torch.cat([torch.zeros((B, cls, 1), device=device, dtype=torch.float64), mf], 1)
    y64.backward(dy.double())
    dx = xin.grad
    assert bool((dx[:, cls:][rows] == 0).all()), "gradient leaks into masked rows"
    keep = torch.cat([torch.ones((B, cls), dtype=torch.bool, device=device), ~rows], 1)
    assert torch.equal(dx[keep], dy[keep]), "gradient of unmasked rows is not the incoming value"
    ulp = 2.0 ** -23
    big_tok = float((dy.double().abs() * torch.cat([torch.zeros((B, cls, 1), device=device, dtype=torch.float64), mf], 1)).amax())
    e_tok = float((tok.grad.double() - t64.grad).abs().max())
    print("mask tokens B=%d pos=%s cls=%d: d_mask_token err %.3e (bound %.3e)" % (B, use_pos, cls, e_tok, 64 * ulp * big_tok))
    assert e_tok <= 64 * ulp * big_tok
    if use_pos:
        e_pos = float((pos.grad.double() - p64.grad).abs().max())
        print("  d_pos err %.3e (bound %.3e)" % (e_pos, 64 * ulp * big_tok))
        assert e_pos <= 64 * ulp * big_tok
        assert bool((pos.grad[:, :cls] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. loss
def check_loss(device):
    g = torch.Generator().manual_seed(31)
    loss_fn = sa.get_loss_func("multi_mse")(reduction="mean")
    assert sa.get_loss_func("mse") is torch.nn.MSELoss
    B, N, C = 3, 40, 27
    x = torch.randn((B, N, C), generator=g).to(device).requires_grad_(True)
    y = torch.randn((B, N, C), generator=g).to(device)
    m = (torch.rand((B, N), generator=g) < 0.4).to(device)
    total, parts = loss_fn([x], [(y, 1.0, "mse", m.float())])
    total.backward()
    xg = x.detach().clone().requires_grad_(True)
    total_g, parts_g = loss_fn([xg[m]], [(y[m], 1.0, "mse")])
    total_g.backward()
    assert len(parts) == 1 and len(parts_g) == 1
    assert abs(float(total.detach()) - float(total_g.detach())) <= 1e-6 * abs(float(total_g.detach()))
    assert float((x.grad - xg.grad).norm()) <= 1e-6 * float(xg.grad.norm())
    x2 = x.detach().clone().requires_grad_(True)
    z, _ = loss_fn([x2], [(y, 1.0, "mse", torch.zeros((B, N), device=device))])
    z.backward()
    assert float(z.detach()) == 0.0 and bool((x2.grad == 0).all()) and bool(torch.isfinite(x2.grad).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. / 7. the model
MODEL_YAML = "configs/masked_ssl/k400_MVITv2_S_16x4_MaskFeat_PT.yaml"
MODEL_OPTS = ["NUM_GPUS", 0, "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
              "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
              "MVIT.POOL_Q_STRIDE", "[[0, 1, 1, 1], [1, 1, 2, 2], [2, 1, 1, 1], [3, 1, 2, 2]]",
              "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]", "AUG.MASK_WINDOW_SIZE", "[4, 4, 4]"]
MODEL_CASES = {"depth3": ["MASK.PRETRAIN_DEPTH", "[3]"], "depth13": ["MASK.PRETRAIN_DEPTH", "[1, 3]"]}
PARAM_SEED, DATA_SEED, BATCH = 41, 42, 2


def model_opts(name):
    return MODEL_OPTS + MODEL_CASES[name]


def model_inputs(cfg, seed=DATA_SEED, batch=BATCH):
    g = torch.Generator().manual_seed(seed)
    clip = torch.randn((batch, 3, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_CROP_SIZE), generator=g)
    mask = (torch.rand((batch,) + tuple(cfg.AUG.MASK_WINDOW_SIZE), generator=g) < 0.4).to(torch.uint8)
    return clip, mask


def state_digest(sd):
    import hashlib
    return hashlib.sha256(json.dumps(sorted([k, list(v.shape)] for k, v in sd.items())).encode()).hexdigest()


def seeded_state(model):
    """Seeded generic parameters for every key but the fixed Sobel buffers of the HOG layer."""
    from oracle import mvit_ref
    own = model.state_dict()
    sd = mvit_ref.randomize_state({k: tuple(v.shape) for k, v in own.items() if not k.startswith("hogs.")}, PARAM_SEED)
    sd.update({k: v for k, v in own.items() if k.startswith("hogs.")})
    return sd


def build_model(name, device):
    cfg = sa.get_preset("MVITv2_S_16x4_MaskFeat_PT", model_opts(name))
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    model.load_state_dict(seeded_state(model))
    return cfg, model.to(device).train()


def _run_model(model, clip, mask, device, dense):
    model.zero_grad(set_to_none=True)
    model.dense = dense
    loss_fn = sa.get_loss_func("multi_mse")(reduction="mean")
    preds, labels = model([clip.to(device), torch.Tensor(), mask.to(device)])
    loss, _ = loss_fn([p.float() for p in preds], labels)
    loss.backward()
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    return preds, labels, loss.detach(), grads


def hog_reference_ops(clip, ts, fs):
    """The reference's own fp32 op sequence for the targets (reflect pad, two grouped 3x3 correlations, atan2, scatter_add_,
    cell sums, normalise, per-token order): what the oracle below regresses on, as the reference does."""
    xs = clip[:, :, ::ts].transpose(1, 2)
    B, Tu = xs.shape[:2]
    xp = F.pad(xs.flatten(0, 1), (1, 1, 1, 1), mode="reflect")
    wx = torch.tensor([[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]]).view(1, 1, 3, 3).repeat(3, 1, 1, 1)
    gx, gy = F.conv2d(xp, wx, groups=3), F.conv2d(xp, wx.transpose(2, 3), groups=3)
    norm = torch.stack([gx, gy], dim=-1).norm(dim=-1)
    phase = torch.atan2(gx, gy) / math.pi * 9
    n, c, h, w = norm.shape
    hist = torch.zeros((n, c, 9, h, w))
    hist.scatter_add_(2, phase.view(n, c, 1, h, w).floor().long() % 9, norm.view(n, c, 1, h, w))
    hist = F.normalize(hist.unfold(3, 8, 8).unfold(4, 8, 8).sum(dim=[-1, -2]), p=2, dim=2)
    return _to_tokens(hist.view(B, Tu, 3, 9, h // 8, w // 8).transpose(1, 2), fs)


def oracle_run(cfg, sd, clip, mask):
    """fp32 torch restatement of MaskMViT._maskfeat_forward + MSSeparateHead + multi_mse on the blocks of oracle/mvit_ref.py
    -> (gathered predictions, loss, parameter gradients).  check_oracle pins it to the numbers of the unmodified reference."""
    from oracle import mvit_ref
    m = cfg.MVIT
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items() if not k.startswith("hogs.")}
    x = F.conv3d(clip, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], tuple(m.PATCH_STRIDE), tuple(m.PATCH_PADDING))
    B, _, T, H, W = x.shape
    x = x.flatten(2).transpose(1, 2)
    fm = F.interpolate(mask.float(), size=(H, W)).flatten(1).unsqueeze(-1)
    x = x * (1 - fm) + sd["mask_token"] * fm
    has_cls = bool(m.CLS_EMBED_ON)
    if has_cls:
        x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    assert not m.USE_ABS_POS
    depths = list(cfg.MASK.PRETRAIN_DEPTH)
    feat_size, _ = masked.calc_mvit_feature_geometry(cfg)
    thw, outs = [T, H, W], []
    for i, (heads, sq, skv) in enumerate(mvit_ref.mvit_plan(cfg)[:depths[-1] + 1]):
        x, thw = mvit_ref.block(x, sd, "blocks.%d" % i, thw, heads, sq, skv, has_cls=has_cls,
                                residual_pooling=m.RESIDUAL_POOLING, dim_mul_in_att=m.DIM_MUL_IN_ATT, pool_first=m.POOL_FIRST)
        if i in depths:
            outs.append(x)
    preds, loss = [], 0.0
    for i, (d, x) in enumerate(zip(depths, outs)):
        fs = feat_size[d][-1]
        rows = F.interpolate(mask.float(), size=fs).flatten(1).bool()
        x = mvit_ref._ln(x, sd, "pred_head.transforms.%d.0" % i)
        x = (x[:, 1:] if has_cls else x)[rows]
        p = F.linear(x, sd["pred_head.projections.%d.weight" % i], sd["pred_head.projections.%d.bias" % i])
        loss = loss + F.mse_loss(p, hog_reference_ops(clip, m.PATCH_STRIDE[0], fs)[rows])
        preds.append(p)
    loss.backward()
    return [p.detach() for p in preds], float(loss.detach()), {k: v.grad for k, v in sd.items()}


_oracle_cache = {}


def oracle_case(name):
    """(cfg, clip, mask, oracle predictions, loss, gradients) of a model case, computed once and shared."""
    if name not in _oracle_cache:
        cfg, model = build_model(name, torch.device("cpu"))
        clip, mask = model_inputs(cfg)
        _oracle_cache[name] = (clip, mask) + oracle_run(cfg, model.state_dict(), clip, mask)
    return _oracle_cache[name]


def check_oracle(name):
    """The oracle reproduces what the unmodified reference produced: loss, gradient norm, a seeded sample of the predictions and
    (norm, random projection) of EVERY parameter gradient, within fp32 summation noise."""
    rec = fixture()["model"][name]
    _, _, preds, loss, grads = oracle_case(name)
    assert abs(loss - rec["loss"]) <= 1e-5 * max(1.0, abs(rec["loss"]))
    gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
    assert abs(gn - rec["grad_norm"]) <= 1e-4 * rec["grad_norm"]
    assert set(grads) == set(rec["grads"])
    for k, (norm, proj) in rec["grads"].items():
        n, p_ = grad_probe(k, grads[k])
        floor = 1e-3 * rec["grad_norm"] / len(grads) ** 0.5
        assert abs(n - norm) <= 2e-4 * max(norm, floor), (k, n, norm)
        assert abs(p_ - proj) <= 2e-4 * max(norm, floor) * 4, (k, p_, proj)     # |projection error| ~ |error| on a unit direction
    for i, p in enumerate(preds):
        r = rec["preds"][i]
        assert list(p.shape) == r["shape"]
        want = f32_from(r["data"])
        got = p.flatten()[sample_index(p.numel(), PROBE_SEED + i, SAMPLE)]
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), (i, float((got - want).abs().max()))


def model_bounds(rec):
    """The rule of tests/model_checks.py::check_engine: max(its tolerance, 1.5 x the fixture's autocast yardstick of the
    process's activation dtype)."""
    from tests import model_checks as mc
    yard = rec["yardstick"]["float16" if sflib.ACT_MODE == "fp16" else "bfloat16"]
    tol = dict(preds=4e-3, loss=1e-3, grad_norm=1e-3, param_grad_worst=2e-2, grad_global=1e-2)
    b = {k: max(t * mc.EPS_SCALE, mc.YARD * yard[k]) for k, t in tol.items()}
    b["grad_norm"] = max(b["grad_norm"], 0.5 * b["grad_global"] ** 2)
    return b, yard


def check_model(device, name, report=None):
    """Both call forms against the reference's fp32 run: elementwise through the oracle (pinned to the fixture by check_oracle,
    which runs first), loss and gradient norm also against the recorded numbers themselves."""
    from tests import model_checks as mc
    rec = fixture()["model"][name]
    check_oracle(name)
    cfg, model = build_model(name, device)
    assert state_digest(model.state_dict()) == rec["state_digest"], "state_dict keys / shapes differ from the reference's"
    clip, mask, o_preds, _, o_grads = oracle_case(name)
    bounds, yard = model_bounds(rec)
    ogn = rec["grad_norm"]
    res = {}
    runs = {}
    for form, dense in (("gathered", False), ("dense", True)):
        preds, labels, loss, grads = _run_model(model, clip, mask, device, dense)
        runs[form] = (loss, grads)
        assert set(grads) == set(o_grads)
        r = {}
        worst = 0.0
        for i, p in enumerate(preds):
            want = o_preds[i]
            got = p.detach().float().cpu()
            if dense:
                rows = labels[i][3].bool().cpu()
                assert tuple(got.shape[:2]) == tuple(rows.shape)
                got = got[rows]
            assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
            worst = max(worst, float((got - want).abs().max() / want.abs().max()))
        r["preds"] = worst
        r["loss"] = abs(float(loss) - rec["loss"]) / max(1.0, abs(rec["loss"]))
        gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
        r["grad_norm"] = abs(gn - ogn) / ogn
        r["grad_global"] = mc._global_rel(grads, o_grads)
        r["param_grad_worst"], r["param_grad_worst_name"] = mc._param_worst(grads, o_grads, ogn)
        res[form] = r
        for k in ("preds", "loss", "grad_norm", "grad_global", "param_grad_worst"):
            print("maskfeat %s %s %-17s value %.3e  bound %.3e  yardstick %.3e" % (name, form, k, r[k], bounds[k], yard[k]))
    (l0, g0), (l1, g1) = runs["gathered"], runs["dense"]
    res["forms"] = dict(loss=abs(float(l0) - float(l1)) / max(1.0, abs(float(l0))), grad_global=mc._global_rel(g1, g0))
    print("maskfeat %s gathered vs dense: loss %.3e  grad_global %.3e" % (name, res["forms"]["loss"], res["forms"]["grad_global"]))
    if report is not None:
        report[name] = dict(result=res, bounds=bounds, yardstick=yard)
    for form in ("gathered", "dense"):
        for k in ("preds", "loss", "grad_norm", "grad_global", "param_grad_worst"):
            assert res[form][k] <= bounds[k], (form, k, res[form])
    assert res["forms"]["loss"] <= bounds["loss"] and res["forms"]["grad_global"] <= bounds["grad_global"], res["forms"]
    return res


def check_captured_step(device, use_graph, iterations=4):
    """TrainStep with model.dense = True over ``iterations`` iterations with a new mask table each: the loss of iteration k equals an eager
    step's from the same state, and the library reports the HOG entry point exactly once per iteration."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.step import TrainStep
    rec = fixture()["model"]["depth3"]
    bounds, _ = model_bounds(rec)
    cfg, model = build_model("depth3", device)
    model.dense = True
    _, twin = build_model("depth3", device)
    twin.dense = True
    loss_fn = sa.get_loss_func("multi_mse")(reduction="mean")

    def make(m):
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        return TrainStep(m, GradReducer(m), opt, loss_fn, use_graph=use_graph, warmup=1), opt
    step, _ = make(model)
    eager, _ = make(twin)
    eager.use_graph = False
    random.seed(5)
    gen = masking.construct_mask_generator(cfg_with_masks(cfg))
    placeholder = torch.zeros(1, device=device)
    counts = []
    for it in range(iterations):
        clip, _ = model_inputs(cfg, seed=100 + it)
        masks = gen.sample_batch(BATCH)
        calls = []
        sflib.set_call_observer(lambda name, thunk, work, calls=calls: (calls.append(name), thunk())[1])
        try:
            la = step([clip.to(device), torch.Tensor().to(device), masks.to(device)], placeholder)
        finally:
            sflib.set_call_observer(None)
        lb = eager([clip.to(device), torch.Tensor().to(device), masks.to(device)], placeholder)
        replayed = use_graph and it >= 2
        if not replayed:                # a replay issues no library calls from Python: the capture recorded them
            counts.append(calls.count("sf_hog_targets_f32"))
        err = abs(float(la) - float(lb)) / max(1.0, abs(float(lb)))
        print("maskfeat step it %d: loss %.6f eager %.6f rel %.3e (bound %.3e)" % (it, float(la), float(lb), err, bounds["loss"]))
        assert math.isfinite(float(la)) and err <= bounds["loss"], (it, float(la), float(lb))
        assert step.logits.dim() == 3
    assert counts and all(c == 1 for c in counts), counts


def cfg_with_masks(cfg):
    c = cfg.clone()
    c.AUG.GEN_MASK_LOADER = True
    c.AUG.MASK_RATIO = 0.4
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 8. rejections
def check_rejections(device):
    import pytest
    x = torch.randn(1, 3, 2, 32, 32).to(device)
    packed = x.clone()
    packed._sf_wpairs = True
    with pytest.raises(NotImplementedError, match="W-pair"):
        masked.hog_targets(packed, 1, 2)
    with pytest.raises(SfError, match="H != W"):
        masked.hog_targets(torch.randn(1, 3, 2, 32, 16).to(device), 1, 2)
    with pytest.raises(SfError, match=r"8 \* fs"):
        masked.hog_targets(x, 1, 3)
    with pytest.raises(SfError, match="u <= 17"):
        masked.hog_targets(torch.randn(1, 3, 1, 144, 144).to(device), 1, 1)
    act = sflib.act_dtype()
    tok = torch.zeros((1, 2 * 4 * 4, 32), dtype=act, device=device)
    mt = torch.zeros((1, 1, 32), device=device)
    with pytest.raises(SfError, match="does not divide"):
        tokens.MaskTokenFn.apply(tok.clone(), torch.zeros((1, 2, 3, 3), dtype=torch.uint8, device=device), (2, 4, 4), 0, mt, None)
    with pytest.raises(SfError, match="Tw != T'"):
        tokens.MaskTokenFn.apply(tok.clone(), torch.zeros((1, 4, 2, 2), dtype=torch.uint8, device=device), (2, 4, 4), 0, mt, None)
    for opts, key in ((["MASK.MAE_ON", True], "MAE_ON"), (["MASK.PRED_HOG", False], "PRED_HOG"),
                      (["MASK.HEAD_TYPE", "separate_xformer"], "separate_xformer"), (["MASK.MAE_RND_MASK", True], "MAE_RND_MASK"),
                      (["MVIT.PATCH_2D", True], "PATCH_2D")):
        cfg = sa.get_preset("MVITv2_S_16x4_MaskFeat_PT", model_opts("depth3") + opts)
        with pytest.raises(NotImplementedError, match=key):
            sa.MODEL_REGISTRY.get("MaskMViT")(cfg)


def check_host_tensor_rejected():
    """With the gfx950 library a host tensor raises: there is no torch fallback."""
    import pytest
    assert sflib.get_lib().backend == "gfx950"
    with pytest.raises(SfError, match="CUDA/HIP tensors"):
        masked.hog_targets(torch.randn(1, 3, 2, 32, 32), 1, 2)
