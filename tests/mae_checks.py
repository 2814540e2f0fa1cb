"""Checks of the MAE path (slowfast_amd/masked.py, masking.py, csrc/sf_pixel.h, the keep / restore kernels of csrc/sf_tokens.h),
shared by the GPU tests (tests/test_mae_gpu.py) and their host-simulator twins (tests/test_mae_hostsim.py).

References.  The keep / restore kernels are pure copies (bit-equal to a torch restatement) plus two sums (fp64).  The pixel
targets are compared per element with an fp64 restatement and with the bytes the unmodified reference produced
(tests/golden/mae_contract.json, recorded by tools/make_mae_golden.py).  The model is compared with the reference's own fp32
run: elementwise through ``oracle_run``, a torch restatement of ``MaskMViT._mae_forward`` on the blocks of oracle/mvit_ref.py
that is itself pinned to the reference's recorded loss, gradient norm, sampled predictions and (norm, projection) of every
parameter gradient.  Inputs are drawn from the seeds the fixture names.
"""
import json
import math
import os

import torch
import torch.nn.functional as F

import slowfast_amd as sa
from slowfast_amd import lib as sflib
from slowfast_amd import masked, masking, tokens
from slowfast_amd.lib import SfError
from tests.maskfeat_checks import PROBE_SEED, SAMPLE, f32_bytes, f32_from, grad_probe, sample_index, table_digest  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mae_contract.json")
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with open(GOLDEN) as f:
            _fixture = json.load(f)
    return _fixture


# ---------------------------------------------------------------------------------------------------------------------------
# 1. masks: (N, L, ratio, seeds)
MASK_CASES = ((2, 64, 0.9, (0, 3)), (2, 64, 0.75, (1,)), (3, 256, 0.75, (5,)), (2, 1568, 0.9, (0,)))


def mask_key(N, L, ratio, seed):
    return "%d/%d/%g/%d" % (N, L, ratio, seed)


def check_masks():
    fx = fixture()["masks"]
    for N, L, ratio, seeds in MASK_CASES:
        for seed in seeds:
            rec = fx[mask_key(N, L, ratio, seed)]
            torch.manual_seed(seed)
            gen = masking.MaeMaskGenerator(L, ratio)
            table = gen.sample_batch(N)
            assert table.dtype == torch.int32 and tuple(table.shape) == (N, L)
            assert gen.len_keep == rec["len_keep"], (gen.len_keep, rec["len_keep"])
            assert torch.equal(table.long().sort(1).values, torch.arange(L).expand(N, L)), "a row is not a permutation"
            assert table_digest(table) == rec["sha256"], (N, L, ratio, seed)
            assert bool(((table < gen.len_keep).sum(1) == gen.len_keep).all())
            assert torch.equal(gen.mask(table), (table >= gen.len_keep).float())
    assert masking.MaeMaskGenerator(64, 0.9).len_keep == 6          # int(64 * (1 - 0.9)) as the reference computes it
    assert masking.construct_mae_mask_generator(sa.get_cfg()) is None
    cfg = sa.get_preset("k400_VIT_B_16x4_MAE_PT")
    gen = masking.construct_mae_mask_generator(cfg)
    assert (gen.num_tokens, gen.len_keep) == (1568, 156)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. keep / restore kernels
TOKEN_CASES = {"b2_444": dict(B=2, L=64, K=16, C=128), "b3_355": dict(B=3, L=75, K=7, C=96), "b1_k2": dict(B=1, L=64, K=2, C=64)}
SENTINEL = -1024.0          # exact in fp16 and bf16


def _perm_table(B, L, g):
    return torch.argsort(torch.argsort(torch.rand((B, L), generator=g), dim=1), dim=1).to(torch.int32)


def _rows(shape, g, device, pitched=False):
    """A random token tensor in the activation type; ``pitched``: a channel slice of a wider one (row pitch C + 16)."""
    act = sflib.act_dtype()
    B, N, C = shape
    if not pitched:
        return torch.randn(shape, generator=g).to(act).to(device)
    wide = torch.randn((B, N, C + 16), generator=g).to(act).to(device)
    return wide[..., :C]


def _gather_rows(x, idx):
    return torch.gather(x, 1, idx.long().unsqueeze(-1).expand(-1, -1, x.shape[-1]))


def check_token_kernels(device, name, cls, pitched):
    """Keep forward / backward and restore's de bit-equal to a torch restatement, restore forward bit-equal to one rounding of
    the fp32 sum, d_mask_token / d_dpos against fp64, two launches bit-identical."""
    act = sflib.act_dtype()
    c = TOKEN_CASES[name]
    B, L, K, C = c["B"], c["L"], c["K"], c["C"]
    g = torch.Generator().manual_seed(61 + 7 * cls + sum(name.encode()))
    ids = _perm_table(B, L, g).to(device)
    ids_keep = torch.argsort(ids.long(), dim=1)[:, :K]
    x = _rows((B, cls + L, C), g, device, pitched)
    # keep forward
    y = tokens.token_keep_fwd(x, ids, K, cls)
    want = torch.cat([x[:, :cls], _gather_rows(x[:, cls:], ids_keep)], 1)
    assert y.dtype == act and torch.equal(y, want), "keep forward"
    assert torch.equal(tokens.token_keep_fwd(x, ids, K, cls), y)
    # keep backward: every row written (the result buffer is torch.empty)
    dy = _rows((B, cls + K, C), g, device, pitched)
    dx = tokens.token_keep_bwd(dy, ids, L, cls)
    padded = torch.cat([dy[:, cls:], torch.zeros((B, L - K, C), dtype=act, device=device)], 1)
    want = torch.cat([dy[:, :cls], _gather_rows(padded, ids)], 1)
    assert torch.equal(dx, want), "keep backward"
    assert torch.equal(tokens.token_keep_bwd(dy, ids, L, cls), dx)
    # restore forward
    e = _rows((B, cls + K, C), g, device, pitched)
    tok = (torch.randn(C, generator=g) * 0.5).to(device)
    dpos = (torch.randn((cls + L, C), generator=g) * 0.5).to(device)
    yr = tokens.token_restore_fwd(e, ids, tok, dpos, cls)
    padded = torch.cat([e[:, cls:].float(), tok.view(1, 1, C).expand(B, L - K, C)], 1)
    want = (torch.cat([e[:, :cls].float(), _gather_rows(padded, ids)], 1) + dpos).to(act)
    assert torch.equal(yr, want), "restore forward"
    assert torch.equal(tokens.token_restore_fwd(e, ids, tok, dpos, cls), yr)
    # restore backward
    dyr = _rows((B, cls + L, C), g, device, pitched)
    de, dtok, ddpos = tokens.token_restore_bwd(dyr, ids, K, cls)
    want = torch.cat([dyr[:, :cls], _gather_rows(dyr[:, cls:], ids_keep)], 1)
    assert torch.equal(de, want), "restore backward: de"
    de2, dtok2, ddpos2 = tokens.token_restore_bwd(dyr, ids, K, cls)
    assert torch.equal(de2, de) and torch.equal(dtok2, dtok) and torch.equal(ddpos2, ddpos), "two launches differ"
    removed = (ids >= K)
    mf = torch.cat([torch.zeros((B, cls), dtype=torch.bool, device=device), removed], 1).double().unsqueeze(-1)
    tok64 = (dyr.double() * mf).sum((0, 1))
    pos64 = dyr.double().sum(0)
    ulp = 2.0 ** -23                            # the rule of maskfeat_checks._check_mask_tokens for the same kind of sums
    big = float((dyr.double().abs() * mf).amax())
    e_tok = float((dtok.double() - tok64).abs().max())
    e_pos = float((ddpos.double() - pos64).abs().max())
    big_pos = float(dyr.double().abs().amax())
    print("mae tokens %s cls=%d pitched=%s: d_mask_token err %.3e (bound %.3e), d_dpos err %.3e (bound %.3e)"
          % (name, cls, pitched, e_tok, 64 * ulp * big, e_pos, 64 * ulp * big_pos))
    assert e_tok <= 64 * ulp * big and e_pos <= 64 * ulp * big_pos
    # the autograd functions deliver the same tensors
    xin = x.detach().clone().contiguous().requires_grad_(True)
    tokens.TokenKeepFn.apply(xin, ids, K, cls).backward(dy)
    assert torch.equal(xin.grad, dx)
    ein = e.detach().clone().contiguous().requires_grad_(True)
    tp = tok.view(1, 1, C).clone().requires_grad_(True)
    pp = dpos.view(1, cls + L, C).clone().requires_grad_(True)
    out = tokens.TokenRestoreFn.apply(ein, ids, cls, tp, pp)
    assert torch.equal(out, yr)
    out.backward(dyr)
    assert torch.equal(ein.grad, de) and torch.equal(tp.grad.flatten(), dtok) and torch.equal(pp.grad[0], ddpos)


def _guarded(shape, dtype, device, guard_rows=8):
    """A sentinel-filled buffer with ``guard_rows`` rows in front of and behind the [B, N, C] view the kernel gets."""
    B, N, C = shape
    buf = torch.full(((B * N + 2 * guard_rows) * C,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[guard_rows * C:(guard_rows + B * N) * C].view(B, N, C)


def _guards_intact(buf, shape, guard_rows=8):
    B, N, C = shape
    host = buf.cpu()
    return bool((host[:guard_rows * C] == SENTINEL).all()) and bool((host[(guard_rows + B * N) * C:] == SENTINEL).all())


def check_bad_tables(device, cls):
    """A table full of 0x7fffffff and one full of -1: every entry is "not kept" (unsigned r >= K), nothing leaves the
    buffers (guard rows around every output), and what such a table defines is computed: only the cls row is kept."""
    act = sflib.act_dtype()
    B, L, K, C = 2, 40, 5, 64
    g = torch.Generator().manual_seed(71 + cls)
    lib = sflib.get_lib()
    for value in (0x7fffffff, -1):
        ids = torch.full((B, L), value, dtype=torch.int32, device=device)
        x = _rows((B, cls + L, C), g, device)
        short = _rows((B, cls + K, C), g, device)
        tok = torch.randn(C, generator=g).to(device)
        dpos = torch.randn((cls + L, C), generator=g).to(device)
        st = tokens._stream(x)
        # keep forward
        buf, y = _guarded((B, cls + K, C), act, device)
        lib.call("sf_token_keep_fwd", x.data_ptr(), C, y.data_ptr(), C, B, cls, L, K, C, ids.data_ptr(), st)
        assert _guards_intact(buf, (B, cls + K, C)), "keep forward wrote outside its output"
        assert torch.equal(y[:, :cls], x[:, :cls]) and bool((y[:, cls:] == SENTINEL).all())
        # keep backward
        buf, dx = _guarded((B, cls + L, C), act, device)
        lib.call("sf_token_keep_bwd", short.data_ptr(), C, dx.data_ptr(), C, B, cls, L, K, C, ids.data_ptr(), st)
        assert _guards_intact(buf, (B, cls + L, C)), "keep backward wrote outside its output"
        assert torch.equal(dx[:, :cls], short[:, :cls]) and bool((dx[:, cls:] == 0).all())
        # restore forward
        buf, yr = _guarded((B, cls + L, C), act, device)
        lib.call("sf_token_restore_fwd", short.data_ptr(), C, yr.data_ptr(), C, B, cls, L, K, C, ids.data_ptr(),
                 tok.data_ptr(), dpos.data_ptr(), st)
        assert _guards_intact(buf, (B, cls + L, C)), "restore forward wrote outside its output"
        want = torch.cat([short[:, :cls].float(), tok.view(1, 1, C).expand(B, L, C)], 1) + dpos
        assert torch.equal(yr, want.to(act))
        # restore backward
        buf, de = _guarded((B, cls + K, C), act, device)
        nrows = lib.call("sf_token_restore_bwd_blocks", cls + L, C)
        pbuf = torch.full(((nrows + 2) * 2 * C,), SENTINEL, dtype=torch.float32, device=device)
        dbuf = torch.full(((cls + L + 2) * C,), SENTINEL, dtype=torch.float32, device=device)
        lib.call("sf_token_restore_bwd", x.data_ptr(), C, de.data_ptr(), C, B, cls, L, K, C, ids.data_ptr(),
                 dbuf[C:].data_ptr(), pbuf[2 * C:].data_ptr(), st)
        assert _guards_intact(buf, (B, cls + K, C)), "restore backward wrote outside de"
        ph, dh = pbuf.cpu(), dbuf.cpu()
        assert bool((ph[:2 * C] == SENTINEL).all()) and bool((ph[-2 * C:] == SENTINEL).all()), "outside the partial table"
        assert bool((dh[:C] == SENTINEL).all()) and bool((dh[-C:] == SENTINEL).all()), "outside d_dpos"
        assert torch.equal(de[:, :cls], x[:, :cls]) and bool((de[:, cls:] == SENTINEL).all())
        assert not bool((ph[2 * C:-2 * C] == SENTINEL).any()) and not bool((dh[C:-C] == SENTINEL).any())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. pixel targets
PIXEL_CASES = {
    "p16_u1": dict(B=2, T=4, S=32, ts=2, u=1, p=16, seed=81),
    "p16_u2": dict(B=2, T=4, S=32, ts=2, u=2, p=16, seed=82),
    "p8": dict(B=1, T=2, S=64, ts=2, u=1, p=8, seed=83),
    "p16_t8": dict(B=2, T=8, S=64, ts=2, u=1, p=16, seed=84),
}
PIXEL_INPUTS = ("randn", "quantised", "lowvar", "constant")
PIXEL_RECORDED = ("randn", "quantised")         # the inputs on which the reference's own fp32 result is compared
PIXEL_SAMPLE = 256                              # recorded elements per (case, input), drawn over all rows and features
WAVE, FOLD_STEPS = 64, 6


def pixel_chain(n):
    """k of the bound: the kernel's longest addition chain on a row of n values.  Lane l of a 64-lane wavefront adds the
    elements l, l + 64, ... serially -- ceil(n / 64) terms -- and the 64 partial sums are folded by an xor butterfly over
    32, 16, 8, 4, 2, 1: six more additions on every path.  (Both sums of a row, mean and variance, have this shape.)"""
    return (n + WAVE - 1) // WAVE + FOLD_STEPS


assert pixel_chain(1536) == 30 and pixel_chain(1536) <= 64


def pixel_input(name, kind):
    c = PIXEL_CASES[name]
    g = torch.Generator().manual_seed(c["seed"] * 10 + PIXEL_INPUTS.index(kind))
    shape = (c["B"], 3, c["T"], c["S"], c["S"])
    if kind == "randn":
        return torch.randn(shape, generator=g)
    if kind == "quantised":                     # an 8-bit frame after mean / std normalisation
        return torch.round(255.0 * torch.rand(shape, generator=g)) / 255.0 / 0.225 - 2.0
    if kind == "lowvar":                        # a level far above the spread: an unshifted sum loses the spread
        return 1.7 + 1e-4 * torch.randn(shape, generator=g)
    x = torch.randn(shape, generator=g)         # constant patches (letterbox bars) and one constant token frame (padding)
    p, ts = c["p"], c["ts"]
    x[:, :, :, :p, :] = 1.7                     # the top row of patches of every frame
    x[0, :, :, -p:, -p:] = -0.25                # one more patch, in every frame of sample 0
    if c["T"] > ts:
        x[:, :, :ts] = 0.37                     # every frame of the first token frame (the clips with more than one)
    return x


def patchify(x, ts, u, p):
    """_patchify of the used frames: (B, 3, T, H, W) -> (B, t*h*w, u*p*p*3)."""
    if u == 1:
        x = x[:, :, ::ts]
    N, _, T, H, W = x.shape
    h = w = H // p
    t = T // u
    x = x.reshape(N, 3, t, u, h, p, w, p)
    return torch.einsum("nctuhpwq->nthwupqc", x).reshape(N, t * h * w, u * p * p * 3)


_pixel_cache = {}


def pixel_reference(name, kind):
    """(input, fp64 restatement, per-element bound, rows that are constant), computed once and shared."""
    key = (name, kind)
    if key not in _pixel_cache:
        c = PIXEL_CASES[name]
        x = pixel_input(name, kind)
        rows = patchify(x.double(), c["ts"], c["u"], c["p"])
        n = rows.shape[-1]
        mean = rows.mean(-1, keepdim=True)
        var = rows.var(-1, keepdim=True)
        s = (var + 1.0e-6).sqrt()
        out = (rows - mean) / s
        A = (rows - rows[..., :1]).abs().amax(-1, keepdim=True)
        k = pixel_chain(n)
        assert k <= 64
        bound = (k + 8) * 2.0 ** -24 * (A / s + out.abs())
        const = (rows.amax(-1) == rows.amin(-1))
        _pixel_cache[key] = (x, out, bound, const)
    return _pixel_cache[key]


def run_pixels(device, x, c, norm=True):
    """The launch into a sentinel-guarded buffer -> the result on the host."""
    B, _, T, S, _ = x.shape
    shape = (B, (T // c["ts"]) * (S // c["p"]) ** 2, c["u"] * c["p"] ** 2 * 3)
    n = shape[0] * shape[1] * shape[2]
    guard = 1024
    buf = torch.full((n + 2 * guard,), -12345.0, dtype=torch.float32, device=device)
    out = buf[guard:guard + n].view(shape)
    res = masked.pixel_targets(x.to(device), c["ts"], c["u"], c["p"], norm, out=out)
    assert res.data_ptr() == out.data_ptr()
    host = buf.cpu()
    assert bool((host[:guard] == -12345.0).all()) and bool((host[guard + n:] == -12345.0).all()), "wrote outside the output"
    return host[guard:guard + n].view(shape).clone()


def check_pixels(device, name, kind):
    c = PIXEL_CASES[name]
    x, ref, bound, const = pixel_reference(name, kind)
    out = run_pixels(device, x, c)
    assert torch.equal(run_pixels(device, x, c), out), "two launches on the same input differ"
    assert bool(torch.isfinite(out).all())
    ratio = float(((out.double() - ref).abs() / bound.clamp(min=1e-300))[~const].max())
    print("pixel %s %s: n %d, k %d, worst |kernel - fp64| / bound = %.3f" % (name, kind, ref.shape[-1], pixel_chain(ref.shape[-1]),
                                                                          ratio))
    assert bool(((out.double() - ref).abs() <= bound).all()), ratio
    if kind == "constant":
        assert int(const.sum()) >= 3, "the input has no constant patches"
        assert bool((out[const] == 0).all()), "a constant patch does not give exact zeros"
    else:
        assert not bool(const.any())
    if kind == "constant":                      # the reference's 1e-4 on constant rows is in the fixture as a number only
        return
    rec = fixture()["pixels"]["%s/%s" % (name, kind)]
    assert list(out.shape) == rec["shape"]
    idx = sample_index(out.numel(), c["seed"], PIXEL_SAMPLE)
    want = f32_from(rec["out"]).double()
    dev_ref = float(((want - ref.flatten()[idx]).abs() / bound.flatten()[idx].clamp(min=1e-300)).max())
    if kind in PIXEL_RECORDED:
        # both sides round: the kernel within the bound, the reference (k = n serial-ish sums of UNshifted values) measured at
        # 0.02 of it on these inputs -- twice the bound covers the pair
        err = (out.flatten()[idx].double() - want).abs()
        assert bool((err <= 2.0 * bound.flatten()[idx]).all()), float((err / bound.flatten()[idx]).max())
        assert dev_ref <= 1.0, dev_ref
    print("pixel %s %s: the recorded reference is at %.3f of the bound from fp64" % (name, kind, dev_ref))
    if kind == "randn":
        raw = run_pixels(device, x, c, norm=False)
        assert torch.equal(raw, patchify(x, c["ts"], c["u"], c["p"])), "norm = 0 is not _patchify"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the model
MODEL_YAML = "configs/masked_ssl/k400_VIT_B_16x4_MAE_PT.yaml"
MODEL_OPTS = ["NUM_GPUS", 0, "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.EMBED_DIM", 128,
              "MVIT.NUM_HEADS", 2, "MVIT.DEPTH", 3, "MASK.PRETRAIN_DEPTH", "[2]", "MASK.DECODER_DEPTH", 2,
              "MASK.DECODER_EMBED_DIM", 128, "AUG.MASK_RATIO", 0.75]
MODEL_CASES = {"ratio75": [], "ratio90": ["AUG.MASK_RATIO", 0.9], "nocls": ["MVIT.CLS_EMBED_ON", False],
               "dec_sep_pos": ["MASK.DECODER_SEP_POS_EMBED", True], "all_frames": ["MASK.TIME_STRIDE_LOSS", False]}
PARAM_SEED, DATA_SEED, MASK_SEED, BATCH = 43, 44, 45, 2


def model_opts(name):
    return MODEL_OPTS + MODEL_CASES[name]


def model_inputs(cfg, seed=DATA_SEED, mask_seed=MASK_SEED, batch=BATCH):
    """(clip, ids_restore): the table is what the reference draws inside its forward under torch.manual_seed(mask_seed)."""
    g = torch.Generator().manual_seed(seed)
    clip = torch.randn((batch, 3, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_CROP_SIZE), generator=g)
    state = torch.get_rng_state()
    torch.manual_seed(mask_seed)
    ids = masking.construct_mae_mask_generator(cfg).sample_batch(batch)
    torch.set_rng_state(state)
    return clip, ids


def state_list(sd):
    return sorted([k, list(v.shape)] for k, v in sd.items())


def seeded_state(model):
    from oracle import mvit_ref
    return mvit_ref.randomize_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, PARAM_SEED)


def build_model(name, device):
    cfg = sa.get_preset("k400_VIT_B_16x4_MAE_PT", model_opts(name))
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    model.load_state_dict(seeded_state(model))
    return cfg, model.to(device).train()


def _run_model(model, clip, ids, device, dense):
    model.zero_grad(set_to_none=True)
    model.dense = dense
    loss_fn = sa.get_loss_func("multi_mse")(reduction="mean")
    preds, labels = model([clip.to(device), torch.Tensor(), ids.to(device)])
    loss, _ = loss_fn([p.float() for p in preds], labels)
    loss.backward()
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    return preds, labels, loss.detach(), grads


def oracle_run(cfg, sd, clip, ids):
    """fp32 torch restatement of MaskMViT._mae_forward (masked.py:283-476) + MSSeparateHead("separate_xformer") + multi_mse
    on the blocks of oracle/mvit_ref.py, with the reference's own chain of gather / cat / repeat ->
    (gathered predictions, loss, parameter gradients).  check_oracle pins it to the numbers of the unmodified reference."""
    from oracle import mvit_ref
    m, k = cfg.MVIT, cfg.MASK
    sd = {n: v.detach().clone().requires_grad_(True) for n, v in sd.items()}
    x = F.conv3d(clip, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], tuple(m.PATCH_STRIDE), tuple(m.PATCH_PADDING))
    B, C, T, H, W = x.shape
    L = T * H * W
    x = x.flatten(2).transpose(1, 2)
    ids = ids.long()
    K = int(L * (1 - cfg.AUG.MASK_RATIO))
    ids_keep = torch.argsort(ids, dim=1)[:, :K]
    x = torch.gather(x, 1, ids_keep.unsqueeze(-1).repeat(1, 1, C))
    mask = torch.gather(torch.cat([torch.zeros(B, K), torch.ones(B, L - K)], 1), 1, ids).bool()
    has_cls = bool(m.CLS_EMBED_ON)
    s = int(has_cls)
    if has_cls:
        x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    assert m.USE_ABS_POS and m.SEP_POS_EMBED
    pos = sd["pos_embed_spatial"].repeat(1, T, 1) + torch.repeat_interleave(sd["pos_embed_temporal"], H * W, dim=1)
    pos = torch.gather(pos.expand(B, -1, -1), 1, ids_keep.unsqueeze(-1).repeat(1, 1, C))
    if has_cls:
        pos = torch.cat([sd["pos_embed_class"].expand(B, -1, -1), pos], 1)
    x = x + pos
    thw = [T, H, W]
    depth = list(k.PRETRAIN_DEPTH)[-1] + 1
    for i, (heads, sq, skv) in enumerate(mvit_ref.mvit_plan(cfg)[:depth]):
        x, thw = mvit_ref.block(x, sd, "blocks.%d" % i, thw, heads, sq, skv, has_cls=has_cls,
                                residual_pooling=m.RESIDUAL_POOLING, dim_mul_in_att=m.DIM_MUL_IN_ATT, pool_first=m.POOL_FIRST)
    x = mvit_ref._ln(x, sd, "norm")
    x = F.linear(x, sd["decoder_embed.weight"], sd["decoder_embed.bias"])
    Cd = x.shape[-1]
    x_ = torch.cat([x[:, s:], sd["mask_token"].repeat(B, L + s - x.shape[1], 1)], dim=1)
    x_ = torch.gather(x_, 1, ids.unsqueeze(-1).repeat(1, 1, Cd))
    x = torch.cat([x[:, :s], x_], dim=1)
    if k.DECODER_SEP_POS_EMBED:
        dpos = sd["dec_pos_embed_spatial"].repeat(1, T, 1) + torch.repeat_interleave(sd["dec_pos_embed_temporal"], H * W, dim=1)
        if has_cls:
            dpos = torch.cat([sd["dec_pos_embed_class"], dpos], 1)
        x = x + dpos
    else:
        x = x + sd["decoder_pos_embed"]
    for i in range(k.DECODER_DEPTH):
        x, _ = mvit_ref.block(x, sd, "pred_head.transforms.0.%d" % i, [T, H, W], Cd // 64, [1, 1, 1], [1, 1, 1], has_cls=has_cls,
                              residual_pooling=False, dim_mul_in_att=False, pool_first=m.POOL_FIRST)
    x = mvit_ref._ln(x, sd, "pred_head.transforms.0.%d" % k.DECODER_DEPTH)
    x = (x[:, 1:] if has_cls else x)[mask]
    pred = F.linear(x, sd["pred_head.projections.0.weight"], sd["pred_head.projections.0.bias"])
    ts = m.PATCH_STRIDE[0]
    label = patchify(clip, ts, 1 if k.TIME_STRIDE_LOSS else ts, m.PATCH_STRIDE[-1])[mask]
    if k.NORM_PRED_PIXEL:
        label = (label - label.mean(dim=-1, keepdim=True)) / (label.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5
    loss = F.mse_loss(pred, label)
    loss.backward()
    return [pred.detach()], float(loss.detach()), {n: v.grad for n, v in sd.items()}


_oracle_cache = {}


def oracle_case(name):
    """(clip, ids, oracle predictions, loss, gradients) of a model case, computed once and shared."""
    if name not in _oracle_cache:
        cfg, model = build_model(name, torch.device("cpu"))
        clip, ids = model_inputs(cfg)
        _oracle_cache[name] = (clip, ids) + oracle_run(cfg, model.state_dict(), clip, ids)
    return _oracle_cache[name]


def check_oracle(name):
    """The oracle reproduces what the unmodified reference produced: loss, gradient norm, a seeded sample of the predictions and
    (norm, random projection) of EVERY parameter gradient, within fp32 summation noise."""
    rec = fixture()["model"][name]
    _, ids, preds, loss, grads = oracle_case(name)
    assert table_digest(ids) == rec["ids_sha256"], "the ids_restore table is not the one the reference drew"
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
    from tests import maskfeat_checks
    return maskfeat_checks.model_bounds(rec)


def check_model(device, name, report=None):
    """The gathered and the dense call form against the reference's fp32 run: elementwise through the oracle (pinned to the
    fixture by check_oracle, which runs first), loss and gradient norm also against the recorded numbers themselves; then the
    form without a table (the model draws its own)."""
    from tests import model_checks as mc
    rec = fixture()["model"][name]
    check_oracle(name)
    cfg, model = build_model(name, device)
    assert state_list(model.state_dict()) == rec["state"], "state_dict keys / shapes differ from the reference's"
    assert not any(k.startswith("hogs.") for k in model.state_dict())
    clip, ids, o_preds, _, o_grads = oracle_case(name)
    bounds, yard = model_bounds(rec)
    ogn = rec["grad_norm"]
    res, runs = {}, {}
    for form, dense in (("gathered", False), ("dense", True)):
        preds, labels, loss, grads = _run_model(model, clip, ids, device, dense)
        runs[form] = (loss, grads)
        assert set(grads) == set(o_grads)
        assert len(preds) == 1 and len(labels) == 1
        got = preds[0].detach().float().cpu()
        if dense:
            rows = labels[0][3].bool().cpu()
            assert tuple(got.shape[:2]) == tuple(rows.shape) and torch.equal(rows, ids >= model_K(cfg))
            got = got[rows]
        want = o_preds[0]
        assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
        r = {"preds": float((got - want).abs().max() / want.abs().max())}
        r["loss"] = abs(float(loss) - rec["loss"]) / max(1.0, abs(rec["loss"]))
        gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
        r["grad_norm"] = abs(gn - ogn) / ogn
        r["grad_global"] = mc._global_rel(grads, o_grads)
        r["param_grad_worst"], r["param_grad_worst_name"] = mc._param_worst(grads, o_grads, ogn)
        res[form] = r
        for k in ("preds", "loss", "grad_norm", "grad_global", "param_grad_worst"):
            print("mae %s %s %-17s value %.3e  bound %.3e  yardstick %.3e" % (name, form, k, r[k], bounds[k], yard[k]))
    (l0, g0), (l1, g1) = runs["gathered"], runs["dense"]
    res["forms"] = dict(loss=abs(float(l0) - float(l1)) / max(1.0, abs(float(l0))), grad_global=mc._global_rel(g1, g0))
    print("mae %s gathered vs dense: loss %.3e  grad_global %.3e" % (name, res["forms"]["loss"], res["forms"]["grad_global"]))
    if report is not None:
        report[name] = dict(result=res, bounds=bounds, yardstick=yard)
    for form in ("gathered", "dense"):
        for k in ("preds", "loss", "grad_norm", "grad_global", "param_grad_worst"):
            assert res[form][k] <= bounds[k], (form, k, res[form])
    assert res["forms"]["loss"] <= bounds["loss"] and res["forms"]["grad_global"] <= bounds["grad_global"], res["forms"]
    # no table: the model draws torch.rand on the clip's device and argsorts it (eager only)
    model.dense = False
    with torch.no_grad():
        for inputs in ([clip.to(device)], [clip.to(device), torch.Tensor(), torch.Tensor()]):
            preds, labels = model(inputs)
            rows = BATCH * (ids.shape[1] - model_K(cfg))
            assert tuple(preds[0].shape) == (rows, o_preds[0].shape[1]) and tuple(labels[0][0].shape) == tuple(preds[0].shape)
            assert len(labels[0]) == 2 and labels[0][1] == 1.0 and bool(torch.isfinite(preds[0]).all())
    return res


def model_K(cfg):
    return masking.construct_mae_mask_generator(cfg).len_keep


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the captured step
def check_captured_step(device, use_graph, iterations=4):
    """TrainStep with model.dense = True over ``iterations`` iterations with a new ids_restore table each: the loss of iteration k
    equals an eager step's from the same state, and the library reports the three MAE forward entry points exactly once per
    (non-replayed) iteration."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.step import TrainStep
    rec = fixture()["model"]["ratio75"]
    bounds, _ = model_bounds(rec)
    cfg, model = build_model("ratio75", device)
    model.dense = True
    _, twin = build_model("ratio75", device)
    twin.dense = True
    loss_fn = sa.get_loss_func("multi_mse")(reduction="mean")

    def make(m):
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        return TrainStep(m, GradReducer(m), opt, loss_fn, use_graph=use_graph, warmup=1), opt
    step, _ = make(model)
    eager, _ = make(twin)
    eager.use_graph = False
    gen = masking.construct_mae_mask_generator(cfg)
    placeholder = torch.zeros(1, device=device)
    watched = ("sf_pixel_targets_f32", "sf_token_keep_fwd", "sf_token_restore_fwd")
    counts = []
    for it in range(iterations):
        clip, _ = model_inputs(cfg, seed=100 + it)
        torch.manual_seed(200 + it)
        ids = gen.sample_batch(BATCH)
        calls = []
        sflib.set_call_observer(lambda name, thunk, work, calls=calls: (calls.append(name), thunk())[1])
        try:
            la = step([clip.to(device), torch.Tensor().to(device), ids.to(device)], placeholder)
        finally:
            sflib.set_call_observer(None)
        lb = eager([clip.to(device), torch.Tensor().to(device), ids.to(device)], placeholder)
        replayed = use_graph and it >= 2
        if not replayed:                # a replay issues no library calls from Python: the capture recorded them
            counts.append(tuple(calls.count(w) for w in watched))
        err = abs(float(la) - float(lb)) / max(1.0, abs(float(lb)))
        print("mae step it %d: loss %.6f eager %.6f rel %.3e (bound %.3e)" % (it, float(la), float(lb), err, bounds["loss"]))
        assert math.isfinite(float(la)) and err <= bounds["loss"], (it, float(la), float(lb))
        assert step.logits.dim() == 3
    assert counts and all(c == (1, 1, 1) for c in counts), counts


# ---------------------------------------------------------------------------------------------------------------------------
# 6. rejections
REJECTED_KEYS = ((["MASK.PER_FRAME_MASKING", True], "PER_FRAME_MASKING"), (["AUG.MASK_TUBE", True], "MASK_TUBE"),
                 (["MASK.MAE_RND_MASK", False], "MAE_RND_MASK"), (["MVIT.USE_FIXED_SINCOS_POS", True], "USE_FIXED_SINCOS_POS"),
                 (["VIS_MASK.ENABLE", True], "VIS_MASK"), (["MVIT.PATCH_2D", True], "PATCH_2D"),
                 (["MASK.PRED_HOG", True], "PRED_HOG"), (["MASK.HEAD_TYPE", "separate"], "HEAD_TYPE"),
                 (["MASK.PRETRAIN_DEPTH", "[1, 2]"], "PRETRAIN_DEPTH"), (["MASK.DEC_KV_KERNEL", "[1, 3, 3]"], "DEC_KV_KERNEL"),
                 (["MVIT.POOL_Q_STRIDE", "[[1, 1, 2, 2]]"], "POOL_Q_STRIDE"), (["MVIT.REL_POS_SPATIAL", True], "REL_POS"),
                 (["MVIT.USE_ABS_POS", False], "USE_ABS_POS"))


def check_rejections(device):
    import pytest
    for opts, key in REJECTED_KEYS:
        cfg = sa.get_preset("k400_VIT_B_16x4_MAE_PT", model_opts("ratio75") + opts)
        with pytest.raises(NotImplementedError, match=key):
            sa.MODEL_REGISTRY.get("MaskMViT")(cfg)
    x = torch.randn(1, 3, 2, 32, 32).to(device)
    packed = x.clone()
    packed._sf_wpairs = True
    with pytest.raises(NotImplementedError, match="W-pair"):
        masked.pixel_targets(packed, 2, 1, 16, True)
    with pytest.raises(SfError, match="H != W"):
        masked.pixel_targets(torch.randn(1, 3, 2, 32, 16).to(device), 2, 1, 16, True)
    with pytest.raises(SfError, match="H % p"):
        masked.pixel_targets(x, 2, 1, 12, True)
    with pytest.raises(SfError, match="T % ts"):
        masked.pixel_targets(torch.randn(1, 3, 3, 32, 32).to(device), 2, 1, 16, True)
    with pytest.raises(SfError, match="u must be 1"):
        masked.pixel_targets(torch.randn(1, 3, 4, 32, 32).to(device), 4, 2, 16, True)
    with pytest.raises(SfError, match="beyond the staged row"):
        masked.pixel_targets(torch.randn(1, 3, 2, 64, 64).to(device), 2, 1, 64, True)
    assert masked.pixel_targets(torch.randn(1, 3, 2, 32, 32).to(device), 2, 2, 16, True).shape == (1, 4, 1536)
    # the launchers
    lib = sflib.get_lib()
    st = tokens._stream(x)
    for args, msg in (((1, 3, 2, 32, 16, 2, 1, 16), "H != W"), ((1, 3, 2, 32, 32, 2, 1, 12), "H % p"),
                      ((1, 3, 3, 32, 32, 2, 1, 16), "T % ts"), ((1, 3, 4, 32, 32, 4, 2, 16), "u must be 1"),
                      ((1, 3, 2, 64, 64, 2, 1, 64), "beyond the staged row")):
        B, _, T, H, W, ts, u, p = args
        clip = torch.zeros((B, 3, T, H, W), device=device)
        with pytest.raises(SfError, match=msg):
            lib.call("sf_pixel_targets_f32", clip.data_ptr(), B, T, H, W, ts, u, p, 1, clip.data_ptr(), st)
    act = sflib.act_dtype()
    tok = torch.zeros((1, 1 + 32, 64), dtype=act, device=device)
    ids = torch.zeros((1, 32), dtype=torch.int32, device=device)
    with pytest.raises(SfError, match="0 < K <= L"):
        tokens.token_keep_fwd(tok, ids, 33, 1)
    with pytest.raises(SfError, match="0 < K <= L"):
        tokens.token_keep_fwd(tok, ids, 0, 1)
    with pytest.raises(SfError, match="ids_restore must be a dense int32"):
        tokens.token_keep_fwd(tok, ids.long(), 4, 1)
    with pytest.raises(SfError, match="ids_restore must be a dense int32"):
        tokens.token_keep_fwd(tok, ids[:, :31].contiguous(), 4, 1)
    with pytest.raises(SfError):
        tokens.token_keep_fwd(torch.zeros((1, 33, 60), dtype=act, device=device), ids, 4, 1)       # C % 8
    with pytest.raises(SfError, match="bad shape"):
        lib.call("sf_token_restore_bwd_blocks", 33, 60)
    with pytest.raises(SfError, match="bad shape"):
        lib.call("sf_token_keep_fwd", tok.data_ptr(), 64, tok.data_ptr(), 64, 1, 2, 32, 4, 64, ids.data_ptr(), st)   # cls 2


def check_host_tensor_rejected():
    """With the gfx950 library a host tensor raises: there is no torch fallback."""
    import pytest
    assert sflib.get_lib().backend == "gfx950"
    with pytest.raises(SfError, match="CUDA/HIP tensors"):
        masked.pixel_targets(torch.randn(1, 3, 2, 32, 32), 2, 1, 16, True)
    with pytest.raises(SfError, match="CUDA/HIP tensors"):
        tokens.token_keep_fwd(torch.zeros((1, 33, 64), dtype=sflib.act_dtype()), torch.zeros((1, 32), dtype=torch.int32), 4, 1)
