"""MixUp / CutMix checks shared by the CPU (host simulator) and GPU (-m gpu) test files (csrc/sf_mixup.h, slowfast_amd/mixup.py,
losses.py, the soft-label statistics of step.TrainStep).

Every comparison of mixed data is BIT-EXACT (torch.equal): each output element is a copy, or two correctly rounded fp32
products and one correctly rounded fp32 sum of them (lam and 1 - lam rounded to fp32 from the host's doubles), which is what
the reference's ``x.mul_(lam).add_(x.flip(0).mul_(1 - lam))`` computes -- there is no accumulation order and no tolerance to
state.  ``ref_mix`` restates that contract in torch on the CPU; tests/golden/mixup_contract.json holds what the reference itself
returned (tools/make_mixup_golden.py).
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import slowfast_amd as sa
from slowfast_amd import lib as _sflib
from slowfast_amd import mixup
from slowfast_amd.mixup import MixParams

ACT = _sflib.act_dtype()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixup_contract.json")
with open(GOLDEN) as _f:
    CONTRACT = json.load(_f)
NUM_GOLDEN_CASES = len(CONTRACT["cases"])

SHAPES = [(3, 2, 6, 10), (3, 1, 5, 7), (1, 3, 4, 16)]       # W % 4 tail / odd W, odd sample size / fully vectorisable
BATCHES = [2, 3, 5]
MIX_LAM = 0.3


def boxes_for(H, W):
    """(yl, yh, xl, xh): empty, full frame, one pixel, odd xl with even xh, and one box on each pair of borders."""
    return [(2, 2, 1, 3), (1, 3, 2, 2), (0, H, 0, W), (1, 2, 2, 3), (1, 3, 1, 4), (0, 2, 0, 3), (H - 2, H, W - 3, W)]


def ref_mix(x, lam, use_cutmix, box):
    """slowfast/datasets/mixup.py:_mix_batch on a CPU fp32 clip, out of place: three separately rounded fp32 operations."""
    x = x.clone()
    if use_cutmix:
        yl, yh, xl, xh = box
        x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
        return x
    lam32 = torch.tensor(float(lam), dtype=torch.float32)
    oml32 = torch.tensor(1.0 - float(lam), dtype=torch.float32)
    return x * lam32 + x.flip(0) * oml32


def ref_targets(target, num_classes, lam, smoothing):
    """mixup_target restated (datasets/mixup.py:22-64)."""
    off_value = smoothing / num_classes
    on_value = 1.0 - smoothing + off_value

    def one_hot(t):
        return torch.full((t.shape[0], num_classes), off_value).scatter_(1, t.long().view(-1, 1), on_value)
    return one_hot(target) * lam + one_hot(target.flip(0)) * (1.0 - lam)


def case_inputs(case):
    g = torch.Generator().manual_seed(case["data_seed"])
    x = torch.randn((case["batch"],) + tuple(CONTRACT["clip_shape"]), generator=g)
    y = torch.randint(0, CONTRACT["num_classes"], (case["batch"],), generator=g)
    return x, y


# ---- 1. the reference's own results -----------------------------------------------------------------------------------
def check_golden_case(device, index):
    case = CONTRACT["cases"][index]
    x, y = case_inputs(case)
    fn = sa.MixUp(num_classes=CONTRACT["num_classes"], **case["args"])
    np.random.seed(case["np_seed"])
    p = fn.sample_params(tuple(x.shape))
    assert repr(float(p.lam)) == case["lam"], (p, case["lam"])
    assert p.use_cutmix == case["use_cutmix"]
    assert (None if p.box is None else list(p.box)) == case["box"]
    want_x = torch.tensor(case["clip"], dtype=torch.float32).view(x.shape)
    want_t = torch.tensor(case["target"], dtype=torch.float32).view(case["batch"], CONTRACT["num_classes"])
    xd, yd = x.clone().to(device), y.to(device)
    np.random.seed(case["np_seed"])
    got_x, got_t = fn(xd, yd)
    assert got_x.data_ptr() == xd.data_ptr(), "the clip is mixed in place"
    assert torch.equal(got_x.cpu(), want_x), "mixed clip differs from the reference's"
    assert got_t.dtype == torch.float32 and torch.equal(got_t.cpu(), want_t), "soft labels differ from the reference's"
    # the same draw from a private generator leaves the global one alone
    state = np.random.get_state()[1].copy()
    fn2 = sa.MixUp(num_classes=CONTRACT["num_classes"], rng=np.random.RandomState(case["np_seed"]), **case["args"])
    assert fn2.sample_params(tuple(x.shape)) == p
    assert np.array_equal(np.random.get_state()[1], state)


# ---- 2. shapes where the kernel can go wrong --------------------------------------------------------------------------
def check_mix_clip_shapes(device, B, shape):
    C, T, H, W = shape
    g = torch.Generator().manual_seed(B * 100 + W)
    x = torch.randn((B,) + tuple(shape), generator=g)
    modes = [MixParams(MIX_LAM, False, None)] + [MixParams(MIX_LAM, True, b) for b in boxes_for(H, W)]
    for p in modes:
        want = ref_mix(x, p.lam, p.use_cutmix, p.box)
        # in place
        xd = x.clone().to(device)
        got = mixup.mix_clip(xd, p)
        assert got.data_ptr() == xd.data_ptr()
        assert torch.equal(got.cpu(), want), ("in place", B, shape, p)
        if p.use_cutmix:                                    # pixels outside the box keep their bits
            yl, yh, xl, xh = p.box
            outside = torch.ones(x.shape, dtype=torch.bool)
            outside[..., yl:yh, xl:xh] = False
            assert torch.equal(got.cpu().view(torch.int32)[outside], x.view(torch.int32)[outside])
            if B % 2:
                assert torch.equal(got.cpu()[B // 2], x[B // 2]), "cutmix leaves the middle sample alone"
        # out=
        xd = x.clone().to(device)
        out = torch.full_like(xd, float("nan"))
        got = mixup.mix_clip(xd, p, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got.cpu(), want), ("out=", B, shape, p)
        assert torch.equal(xd.cpu(), x), "src must be unchanged with out="
    if B % 2:           # the middle sample of an odd batch under mixup is mixed with itself: not the identity
        mid = x[B // 2]
        lam32, oml32 = torch.tensor(MIX_LAM, dtype=torch.float32), torch.tensor(1.0 - MIX_LAM, dtype=torch.float32)
        got = mixup.mix_clip(x.clone().to(device), modes[0]).cpu()[B // 2]
        assert torch.equal(got, mid * lam32 + mid * oml32)
        assert not torch.equal(got, mid), "fl(x*lam) + fl(x*oml) must differ from x somewhere"


def check_mix_clip_rejects(device):
    """No torch fallback: anything but a dense fp32 NCTHW clip, and overlapping buffers, are errors."""
    import pytest
    p = MixParams(MIX_LAM, False, None)
    x = torch.randn((2, 3, 2, 6, 10)).to(device)       # (mixed in place below: its values do not matter)
    for bad in (x.to(ACT), x.double(), x[:, :, :, :, ::2], x[0], x.permute(0, 1, 2, 4, 3)):
        with pytest.raises(sa.lib.SfError):
            mixup.mix_clip(bad, p)
    with pytest.raises(sa.lib.SfError):
        mixup.mix_clip(x, p, out=torch.empty((2, 3, 2, 6, 12), device=device))
    big = torch.zeros(2 * x.numel(), device=device)
    src = big[:x.numel()].view(x.shape)
    with pytest.raises(sa.lib.SfError, match="overlap"):
        mixup.mix_clip(src, p, out=big[4:4 + x.numel()].view(x.shape))
    with pytest.raises(sa.lib.SfError, match="box"):
        mixup.mix_clip(x, MixParams(MIX_LAM, True, (0, 7, 0, 3)))
    fn = sa.MixUp(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=7)
    with pytest.raises(AssertionError):
        fn(x[:1].contiguous(), torch.zeros(1, dtype=torch.int64, device=device))
    with pytest.raises(NotImplementedError):
        sa.MixUp(mix_prob=-1.0, num_classes=7)(x, torch.zeros(2, dtype=torch.int64, device=device))


# ---- 3. packed path ---------------------------------------------------------------------------------------------------
def _unpack(x):
    """(N, 8, T, H, W/2) W-pair view -> ((N, 3, T, H, W) values, 4th channel)."""
    N, C8, T, H, W2 = x.shape
    assert C8 == 8 and getattr(x, "_sf_wpairs", False)
    buf = x.permute(0, 2, 3, 4, 1).reshape(N, T, H, W2 * 2, 4).cpu()
    return buf[..., :3].permute(0, 4, 1, 2, 3).contiguous(), buf[..., 3]


def check_pack_mix(device, B, arch="c2d", reverse=False):
    from oracle import data_ref
    cfg = sa.get_preset("SLOWFAST_8x8_R50" if arch == "slowfast" else "C2D_8x8_R50",
                        ["DATA.MEAN", [0.45, 0.40, 0.35], "DATA.STD", [0.225, 0.25, 0.2],
                         "DATA.REVERSE_INPUT_CHANNEL", reverse])
    g = torch.Generator().manual_seed(B)
    frames = torch.randint(0, 256, (B, 8, 6, 10, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    ref = data_ref.pack_pathways(frames, cfg)
    plain = sa.pack_pathways_u8(frames.to(device), cfg)
    same = sa.pack_pathways_u8(frames.to(device), cfg, mix=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, same)), "mix=None is the unmixed call"
    same = sa.pack_pathways_u8(frames.to(device), cfg, mix=MixParams(1.0, False, None))
    assert all(torch.equal(a, b) for a, b in zip(plain, same)), "lam == 1.0 mixes nothing"
    for p in (MixParams(MIX_LAM, False, None), MixParams(0.6, True, (1, 4, 2, 6)), MixParams(0.5, True, (0, 6, 3, 8))):
        got = sa.pack_pathways_u8(frames.to(device), cfg, mix=p)
        assert len(got) == len(ref)
        vals, pad = _unpack(got[0])
        want = ref_mix(ref[0], p.lam, p.use_cutmix, p.box).to(ACT)
        assert torch.equal(vals, want), (B, arch, p)
        assert float(pad.abs().max()) == 0.0
        assert not torch.equal(vals, ref[0].to(ACT)), "the case must actually mix"
        for a, b in zip(got[1:], plain[1:]):                # the reference mixes inputs[0] only
            assert torch.equal(a, b), "pathway 1 must stay unmixed"
        again = sa.pack_pathways_u8(frames.to(device), cfg, out=plain, mix=p)      # into the buffers of a previous call
        assert [a.data_ptr() for a in again] == [a.data_ptr() for a in plain]
        assert all(torch.equal(a, b) for a, b in zip(again, got))
        plain = sa.pack_pathways_u8(frames.to(device), cfg)


# ---- 4. targets -------------------------------------------------------------------------------------------------------
def check_mix_targets(device, B, K, smoothing, lam=0.37):
    g = torch.Generator().manual_seed(B * K)
    y = torch.randint(0, K, (B,), generator=g)
    fn = sa.MixUp(label_smoothing=smoothing, num_classes=K)
    for lam_ in (lam, 1.0):
        want = ref_targets(y, K, lam_, smoothing)
        got = fn.mix_targets(y.to(device), lam_)
        assert got.shape == (B, K) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), want), (B, K, smoothing, lam_)
        buf = torch.full((B, K), float("nan"), device=device)
        ret = fn.mix_targets(y.to(device), lam_, out=buf)
        assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf.cpu(), want)


# ---- 5. loss ----------------------------------------------------------------------------------------------------------
def check_losses():
    import pytest
    g = torch.Generator().manual_seed(3)
    logits = torch.randn((5, 11), generator=g) * 3
    target = ref_targets(torch.randint(0, 11, (5,), generator=g), 11, 0.37, 0.1)
    per_sample = torch.sum(-target * F.log_softmax(logits, dim=-1), dim=-1)         # oracle/refshim.py:73-82
    assert torch.equal(sa.get_loss_func("soft_cross_entropy")(reduction="mean")(logits, target), per_sample.mean())
    assert torch.equal(sa.get_loss_func("soft_cross_entropy")(reduction="none")(logits, target), per_sample)
    assert sa.get_loss_func("soft_cross_entropy")().normalize_targets is False
    assert sa.get_loss_func("cross_entropy") is torch.nn.CrossEntropyLoss
    assert sa.get_loss_func("bce") is torch.nn.BCELoss and sa.get_loss_func("bce_logit") is torch.nn.BCEWithLogitsLoss
    with pytest.raises(NotImplementedError, match="Loss focal is not supported"):
        sa.get_loss_func("focal")


def check_config():
    cfg = sa.get_cfg()
    assert dict(cfg.MIXUP) == {"ENABLE": False, "ALPHA": 0.8, "CUTMIX_ALPHA": 1.0, "PROB": 1.0, "SWITCH_PROB": 0.5,
                               "LABEL_SMOOTH_VALUE": 0.1}
    assert sa.construct_mixup(cfg) is None
    cfg.MIXUP.ENABLE = True
    cfg.MODEL.NUM_CLASSES = 13
    fn = sa.construct_mixup(cfg)
    assert (fn.mixup_alpha, fn.cutmix_alpha, fn.mix_prob, fn.switch_prob, fn.label_smoothing, fn.num_classes,
            fn.correct_lam) == (0.8, 1.0, 1.0, 0.5, 0.1, 13, True)


# ---- 6. step glue -----------------------------------------------------------------------------------------------------
def ref_errors(logits, labels):
    """top-1 / top-5 error of a mixed batch as tools/train_net.py:174-190 + metrics.topks_correct compute them."""
    _vals, inds = torch.topk(labels, 2, dim=1, largest=True, sorted=True)
    rows = torch.arange(labels.shape[0], device=labels.device)
    preds = logits.detach().clone()
    preds[rows, inds[:, 0]] += preds[rows, inds[:, 1]]
    preds[rows, inds[:, 1]] = 0.0
    top = preds.topk(min(5, preds.shape[1]), dim=1).indices
    hit = top.eq(inds[:, 0].view(-1, 1))
    return (float(100.0 * (1.0 - hit[:, :1].any(1).float().mean())), float(100.0 * (1.0 - hit.any(1).float().mean())))


STEP_SEED = 7


def run_mix_step(device, use_graph, steps=4):
    """``steps`` iterations of TrainStep(track_stats=True) on mvit_tiny with MIXUP.ENABLE True: mixed in place while the step
    runs eagerly, into the captured step's static buffers once they exist.  Returns (losses, parameters, draws) after checking
    every queued statistic against ref_errors on that iteration's logits and soft labels."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    from slowfast_amd.step import TrainStep
    from tests import model_checks as mc
    gold = mc.load_golden("mvit_tiny")
    cfg = mc.cfg_for(gold, extra=["MIXUP.ENABLE", True])
    model, sd, inputs, labels, *_ = mc.oracle_run(gold, cfg)
    model.load_state_dict(sd)
    model = model.to(device).train()
    red = GradReducer(model, bucket_mb=0.05)
    red.attach_torch_param_hooks(model.head.parameters())
    opt = construct_optimizer(model, cfg, red, loss_scale=64.0, dynamic_loss_scale=False)
    for g in opt.param_groups:
        g["lr"] = 0.01
    loss_fn = sa.get_loss_func("soft_cross_entropy")(reduction="mean")
    step = TrainStep(model, red, opt, loss_fn, use_graph=use_graph, warmup=1, track_stats=True)
    mix = sa.construct_mixup(cfg)
    assert mix is not None and len(inputs) == 1
    np.random.seed(STEP_SEED)
    draws, losses, expect, via_static = [], [], [], 0
    sample = mix.sample_params
    mix.sample_params = lambda shape: draws.append(sample(shape)) or draws[-1]
    K = cfg.MODEL.NUM_CLASSES
    for it in range(steps):
        clip = (inputs[0] * (1.0 + 0.125 * it)).to(device)
        y = ((labels + it) % K).to(device)
        y[1] = (y[0] + 3) % K                              # two classes per mixed sample: no tie among the soft labels
        static = step.static_inputs()
        if static is None:
            x, t = mix(clip, y)
            assert x.data_ptr() == clip.data_ptr()
            loss = step([x], t)
        else:
            x, t = mix(clip, y, out=static[0][0], target_out=static[1])
            assert x.data_ptr() == static[0][0].data_ptr() and t.data_ptr() == static[1].data_ptr()
            loss = step(*static)
            via_static += 1
        logits = step.logits.float()
        assert torch.equal(loss, loss_fn(logits, t)), "the step's loss is the soft cross entropy of its logits"
        losses.append(float(loss))
        expect.append(ref_errors(logits, t.clone()))
    for it in range(steps):
        stats = step.pop_stats()
        assert stats[0] == losses[it] and (stats[2], stats[3]) == expect[it], (it, stats, losses[it], expect[it])
    assert step.pop_stats() is None
    assert via_static == (max(0, steps - 2) if use_graph else 0)
    params = [p.detach().float().cpu().clone() for p in model.parameters()]
    red.close()
    return losses, params, draws
