"""Random-erasing checks shared by the CPU (host simulator) and GPU (-m gpu) test files (csrc/sf_erase.h,
slowfast_amd/random_erasing.py, data.pack_pathways_u8(erase=)).

``const`` / ``rand`` results are compared BIT FOR BIT: every erased element is a copy of 0 or of a colour the host drew.
``pixel`` noise is compared with ``ref_noise``: the contract of csrc/sf_erase.h / DESIGN.md §4 restated in numpy -- the same
Philox4x32-10 integer stream (exact), then Box-Muller in float64 rounded to fp32.  Only the evaluation of log / sin / cos (and
the fp32 rounding of u and of 2 pi u in the kernel) may differ, which NOISE_BOUND covers (profiles/random_erasing_noise.md: the
largest deviation measured on the host simulator and on an MI355X, times 8, capped at 1e-3 -- a wrong counter, key or lane
gives differences of order 1).  tests/golden/random_erasing_contract.json holds what the reference itself did
(tools/make_random_erasing_golden.py).
"""
import base64
import json
import os
import random

import numpy as np
import torch

import slowfast_amd as sa
from slowfast_amd import lib as _sflib
from slowfast_amd import mixup
from slowfast_amd import random_erasing as re_
from slowfast_amd.mixup import MixParams

ACT = _sflib.act_dtype()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_erasing_contract.json")
with open(GOLDEN) as _f:
    CONTRACT = json.load(_f)
NUM_GOLDEN_CASES = len(CONTRACT["cases"])

# 8 x the larger of the measured deviations of check_pixel_noise (profiles/random_erasing_noise.md), never above 1e-3.  The
# MI355X figure is None until that file holds one: no GPU run of this check exists yet, and the bound then rests on the host
# simulator's figure alone.
NOISE_MEASURED = {"hostsim": 1.073e-06, "mi355x": None}
NOISE_BOUND = min(8.0 * max(v for v in NOISE_MEASURED.values() if v is not None), 1e-3)


# ---- the pixel-mode contract restated ---------------------------------------------------------------------------------
def philox4x32_10(g, key):
    """Philox4x32-10 on counters (g_lo, g_hi, 0, 0) under the 64-bit ``key``: uint64 array g -> uint32 array (..., 4)."""
    m32 = np.uint64(0xFFFFFFFF)
    g = np.asarray(g, dtype=np.uint64)
    c = [g & m32, g >> np.uint64(32), np.zeros_like(g), np.zeros_like(g)]
    k0, k1 = np.uint64(int(key) & 0xFFFFFFFF), np.uint64(int(key) >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, -1).astype(np.uint32)


def ref_noise(idx, key):
    """The standard normal of element ``idx`` (= ((c*T + t)*H + y)*W + x) under ``key``: float64 transform, rounded to fp32."""
    idx = np.asarray(idx, dtype=np.uint64)
    r = philox4x32_10(idx >> np.uint64(2), key).astype(np.float64)
    u = r * 2.0 ** -32 + 2.0 ** -33
    e = (idx & np.uint64(3)).astype(np.int64)
    pair = (e >> 1) * 2
    ua = np.take_along_axis(u, pair[..., None], -1)[..., 0]
    ub = np.take_along_axis(u, (pair + 1)[..., None], -1)[..., 0]
    rad = np.sqrt(-2.0 * np.log(ua))
    return np.where(e & 1, rad * np.cos(2.0 * np.pi * ub), rad * np.sin(2.0 * np.pi * ub)).astype(np.float32)


def check_philox_vector():
    """Random123's known answer for philox4x32_10 with counter 0 and key 0."""
    assert [hex(v) for v in philox4x32_10(np.array([0], np.uint64), 0)[0]] == \
        ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]


def ref_erase(x, table):
    """The table's rows applied one after the other (later rows win) to a CPU fp32 (N, C, T, H, W) batch, out of place."""
    x = x.clone()
    N, C, T, H, W = x.shape
    line = 0
    for r, (n, t0, t1, top, left, h, w) in enumerate(table.rows.tolist()):
        frames = max(t1 - t0, 0)
        if table.mode == "rand":
            col = torch.from_numpy(table.colours[line:line + frames].copy())             # (frames, C)
            line += frames
            x[n, :, t0:t1, top:top + h, left:left + w] = col.t()[:, :, None, None]
        elif table.mode == "pixel":
            c, t, y, xx = np.meshgrid(np.arange(C), np.arange(t0, t1), np.arange(top, top + h), np.arange(left, left + w),
                                      indexing="ij")
            idx = ((c * T + t) * H + y) * W + xx
            x[n, :, t0:t1, top:top + h, left:left + w] = torch.from_numpy(ref_noise(idx, int(table.keys[r])))
        else:
            x[n, :, t0:t1, top:top + h, left:left + w] = 0.0
    return x


def box_mask(table, shape):
    """bool (N, C, T, H, W): elements some row contains."""
    m = torch.zeros(shape, dtype=torch.bool)
    for n, t0, t1, top, left, h, w in table.rows.tolist():
        m[n, :, t0:t1, top:top + h, left:left + w] = True
    return m


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_erased(got, x, table, what=""):
    """got == ref_erase(x, table): bit for bit in const / rand modes and outside the boxes, within NOISE_BOUND inside pixel
    boxes.  Returns the largest deviation inside the boxes."""
    want = ref_erase(x, table)
    m = box_mask(table, x.shape)
    assert torch.equal(bits(got)[~m], bits(x)[~m]), what + ": an element outside every box changed"
    if table.mode != "pixel":
        assert torch.equal(bits(got), bits(want)), what + ": erased batch differs from sequential application of the rows"
        return 0.0
    dev = float((got[m].double() - want[m].double()).abs().max()) if m.any() else 0.0
    print("%s: max |pixel noise - float64 restatement| = %.3e (bound %.3e)" % (what, dev, NOISE_BOUND))
    assert dev <= NOISE_BOUND, (what, dev, NOISE_BOUND)
    return dev


# ---- 1. the reference's own results -----------------------------------------------------------------------------------
def case_input(case):
    return torch.randn((case["N"],) + tuple(case["shape"]), generator=torch.Generator().manual_seed(case["data_seed"]))


def check_golden_case(device, index):
    case = CONTRACT["cases"][index]
    T, C, H, W = case["shape"]
    x_ref = case_input(case)                                            # (N, T, C, H, W), the reference's layout
    x = x_ref.permute(0, 2, 1, 3, 4).contiguous()
    fn = sa.RandomErasing(noise_seed=5, **case["args"])
    random.seed(case["seed"])
    torch.manual_seed(case["seed"])
    xd = x.clone().to(device)
    got = fn(xd)
    py_after, torch_after = random.random(), float(torch.rand(1))
    assert got.data_ptr() == xd.data_ptr(), "the batch is erased in place"
    assert repr(py_after) == case["py_after"], "random was not consumed as the reference consumes it"
    got = got.cpu().permute(0, 2, 1, 3, 4).contiguous()                 # back to (N, T, C, H, W)
    changed = torch.zeros(x_ref.shape, dtype=torch.bool)
    for n, t, top, left, h, w in case["boxes"]:
        changed[n, t, :, top:top + h, left:left + w] = True
    if case["args"]["mode"] == "pixel":
        assert torch.equal(bits(got) != bits(x_ref), changed), "changed elements differ from the reference's"
    else:
        assert repr(torch_after) == case["torch_after"], "torch's generator was not consumed as the reference consumes it"
        want = torch.from_numpy(np.frombuffer(base64.b64decode(case["out"]), dtype="<f4").copy()).view(x_ref.shape)
        assert torch.equal(bits(got), bits(want)), "erased batch differs from the reference's"
        if case["args"]["mode"] == "rand":
            assert torch.equal(bits(got) != bits(x_ref), changed)
    # the plans of the same draw: rows cover exactly the changed elements, clip by clip
    random.seed(case["seed"])
    torch.manual_seed(case["seed"])
    fn2 = sa.RandomErasing(noise_seed=5, **case["args"])
    cover = torch.zeros(x_ref.shape, dtype=torch.bool)
    for n in range(case["N"]):
        plan = fn2.sample_params((T, C, H, W))
        assert isinstance(plan, sa.ErasePlan) and plan.mode == case["args"]["mode"]
        for t0, t1, top, left, h, w in plan.rows:
            cover[n, t0:t1, :, top:top + h, left:left + w] = True
    assert torch.equal(cover, changed) and repr(random.random()) == case["py_after"]


# ---- 2. pixel noise against the restatement ---------------------------------------------------------------------------
def noise_tables():
    """Explicit pixel tables: boxes starting at left = 0..3 with widths 1..5 on (2,3,4,12,10), and on (1,3,2,9,7), whose odd W
    makes the 4-element groups straddle lines and start unaligned."""
    out = []
    for shape, N in (((4, 3, 12, 10), 2), ((2, 3, 9, 7), 1)):
        T, C, H, W = shape
        k = 0
        for left in range(4):
            rows, keys = [], []
            for w in range(1, 6):
                if left + w > W:
                    continue
                n = (w + left) % N
                rows.append((n, w % 2, T - (w // 3) % 2, (2 * w + left) % (H - 3), left, 1 + (w + left) % 3, w))
                keys.append(0x9E3779B97F4A7C15 * (k + 1) % 2 ** 64 + left)
                k += 1
            order = sorted(range(len(rows)), key=lambda i: rows[i][0])
            out.append((N, re_.make_table([rows[i] for i in order], "pixel", shape, keys=[keys[i] for i in order])))
    return out


def check_pixel_noise(device):
    check_philox_vector()
    worst = 0.0
    for N, table in noise_tables():
        T, C, H, W = table.shape
        x = torch.randn((N, C, T, H, W), generator=torch.Generator().manual_seed(W))
        got = re_.erase_clip(x.clone().to(device), table)
        worst = max(worst, assert_erased(got.cpu(), x, table, "noise %s" % (table.shape,)))
        again = re_.erase_clip(x.clone().to(device), table)
        assert torch.equal(bits(again.cpu()), bits(got.cpu())), "two launches with the same table differ"
        out = re_.erase_clip(x.clone().to(device), table, out=torch.full(x.shape, float("nan")).to(device))
        assert torch.equal(bits(out.cpu()), bits(got.cpu())), "out= differs from in place"
    print("pixel noise: largest deviation %.3e" % worst)
    return worst


# ---- 3. overlap order -------------------------------------------------------------------------------------------------
def overlap_tables(mode, shape=(3, 3, 9, 11), N=2, tables=20):
    """``tables`` distinct tables of two and three rows per sample that overlap on purpose (every row contains the centre)."""
    T, C, H, W = shape
    rng = random.Random(17 if mode == "rand" else 23)
    out = []
    for i in range(tables):
        rows, keys, colours = [], [], []
        for n in range(N):
            for _ in range(2 + (i + n) % 2):
                top, left = rng.randint(0, H // 2), rng.randint(0, W // 2)
                h, w = rng.randint(H // 2 - top + 1, H - top), rng.randint(W // 2 - left + 1, W - left)
                t0 = rng.randint(0, 1)
                rows.append((n, t0, T, top, left, h, w))
                keys.append(rng.getrandbits(64))
                colours.append(np.array([[rng.gauss(0, 1) for _ in range(C)] for _ in range(T - t0)], dtype=np.float32))
        out.append(re_.make_table(rows, mode, shape, keys=keys, colours=colours if mode == "rand" else None))
    return out


def check_overlap(device, mode):
    for i, table in enumerate(overlap_tables(mode)):
        T, C, H, W = table.shape
        x = torch.randn((2, C, T, H, W), generator=torch.Generator().manual_seed(i))
        got = re_.erase_clip(x.clone().to(device), table).cpu()
        assert_erased(got, x, table, "overlap %s %d" % (mode, i))
        # one launch per row, in order: what "later rows win" means, computed by the same device code
        seq, line = x.clone().to(device), 0
        for r in range(len(table.rows)):
            frames = int(table.rows[r, 2] - table.rows[r, 1])
            one = re_.make_table(table.rows[r:r + 1], mode, table.shape, keys=table.keys[r:r + 1],
                                 colours=table.colours[line:line + frames] if mode == "rand" else None)
            line += frames
            re_.erase_clip(seq, one)
        assert torch.equal(bits(seq.cpu()), bits(got)), (mode, i, "one launch differs from one launch per row")
        out = re_.erase_clip(x.clone().to(device), table, out=torch.empty(x.shape).to(device))
        assert torch.equal(bits(out.cpu()), bits(got)), (mode, i, "out= differs from in place")


# ---- 4. noise quality -------------------------------------------------------------------------------------------------
QUALITY_KEYS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)


def quality_stats(z):
    """z: float64 (2, 3, 8, 40, 40) noise of the two samples.  (worst |mean|, worst |var - 1|, worst |correlation| between
    adjacent frames, adjacent channels and the two samples)."""
    mean = max(abs(float(z[n].mean())) for n in range(2))
    var = max(abs(float(z[n].var()) - 1.0) for n in range(2))

    def corr(a, b):
        return abs(float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]))
    cs = [corr(z[n, c, t], z[n, c, t + 1]) for n in range(2) for c in range(3) for t in range(7)]
    cs += [corr(z[n, c, t], z[n, c + 1, t]) for n in range(2) for c in range(2) for t in range(8)]
    cs += [corr(z[0, c, t], z[1, c, t]) for c in range(3) for t in range(8)]
    return mean, var, max(cs)


def check_noise_quality(device):
    shape = (8, 3, 64, 64)
    table = re_.make_table([(0, 0, 8, 12, 12, 40, 40), (1, 0, 8, 12, 12, 40, 40)], "pixel", shape, keys=QUALITY_KEYS)
    x = torch.zeros((2, 3, 8, 64, 64))
    # the keys are chosen so that the restatement alone passes
    mean, var, cor = quality_stats(ref_erase(x, table)[:, :, :, 12:52, 12:52].double().numpy())
    assert mean < 0.0204 and var < 0.0289 and cor < 0.1, ("restatement", mean, var, cor)
    got = re_.erase_clip(x.clone().to(device), table).cpu()
    assert_erased(got, x, table, "quality")
    mean, var, cor = quality_stats(got[:, :, :, 12:52, 12:52].double().numpy())
    print("noise quality: |mean| %.4f  |var - 1| %.4f  max |corr| %.4f" % (mean, var, cor))
    assert mean < 0.0204, mean            # 4 / sqrt(38400)
    assert var < 0.0289, var              # 4 * sqrt(2 / 38400)
    assert cor < 0.1, cor                 # 4 / sqrt(1600)


# ---- 5. out= and empty plans ------------------------------------------------------------------------------------------
def check_out_and_empty(device):
    shape = (4, 3, 12, 10)
    T, C, H, W = shape
    x = torch.randn((3, C, T, H, W), generator=torch.Generator().manual_seed(1))
    for mode in ("const", "rand", "pixel"):
        fn = sa.RandomErasing(probability=1.0, mode=mode, max_count=2, noise_seed=3)
        random.seed(4)
        torch.manual_seed(4)
        table = fn.sample_batch(3, shape)
        assert len(table.rows) >= 3 and table.rows.dtype == np.int32 and table.rows.shape[1] == 7
        assert table.keys.dtype == np.uint64 and table.colours.dtype == np.float32
        src = x.clone().to(device)
        inplace = re_.erase_clip(src.clone(), table)
        out = torch.full(x.shape, float("nan")).to(device)
        ret = re_.erase_clip(src, table, out=out)
        assert ret.data_ptr() == out.data_ptr()
        assert torch.equal(bits(out.cpu()), bits(inplace.cpu())), mode
        assert torch.equal(bits(src.cpu()), bits(x)), "src must be unchanged with out="
        assert_erased(inplace.cpu(), x, table, "out= " + mode)
    # empty plans
    never = sa.RandomErasing(probability=0.0, mode="pixel")
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        xd = x.clone().to(device)
        random.seed(0)
        random.random()                                     # (probability 0.0 erases only on a draw of exactly 0.0)
        assert never(xd).data_ptr() == xd.data_ptr() and calls == [], "an empty plan launches nothing in place"
        assert torch.equal(bits(xd.cpu()), bits(x))
        out = torch.full(x.shape, float("nan")).to(device)
        assert never(xd, out=out).data_ptr() == out.data_ptr()
        assert torch.equal(bits(out.cpu()), bits(x)), "an empty plan with out= is a copy"
    finally:
        _sflib.set_call_observer(None)
    assert never.sample_params(shape).rows == []


# ---- 6. packed path ---------------------------------------------------------------------------------------------------
def _unpack(x):
    """(N, 8, T, H, W/2) W-pair view -> ((N, 3, T, H, W) values, 4th channel)."""
    N, C8, T, H, W2 = x.shape
    assert C8 == 8 and getattr(x, "_sf_wpairs", False)
    buf = x.permute(0, 2, 3, 4, 1).reshape(N, T, H, W2 * 2, 4).cpu()
    return buf[..., :3].permute(0, 4, 1, 2, 3).contiguous(), buf[..., 3]


def _ordered(t):
    """16-bit floats -> integers whose difference counts representable values between two numbers."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7FFF))


def _pathways(clip, cfg):
    """pack_pathway_output on a normalised (N, 3, T, H, W) batch (oracle/data_ref.py: reversal, then the Slow index_select)."""
    if cfg.DATA.REVERSE_INPUT_CHANNEL:
        clip = clip[:, [2, 1, 0]]
    idx = sa.data.pathway_frame_indices(cfg, clip.shape[2])
    return [clip if i is None else torch.index_select(clip, 2, i) for i in idx]


PACK_MIXES = (None, MixParams(0.3, False, None), MixParams(0.6, True, (3, 9, 4, 15)))


def check_pack(device, N, mode, arch="c2d", reverse=False):
    cfg = sa.get_preset("SLOWFAST_8x8_R50" if arch == "slowfast" else "C2D_8x8_R50",
                        ["DATA.MEAN", [0.45, 0.40, 0.35], "DATA.STD", [0.225, 0.25, 0.2],
                         "DATA.REVERSE_INPUT_CHANNEL", reverse])
    T, H, W = 8, 12, 20
    frames = torch.randint(0, 256, (N, T, H, W, 3), generator=torch.Generator().manual_seed(N), dtype=torch.int64).to(torch.uint8)
    norm = torch.stack([((f.float() / 255.0 - torch.tensor(cfg.DATA.MEAN)) / torch.tensor(cfg.DATA.STD)).permute(3, 0, 1, 2)
                        for f in frames], 0).contiguous()               # (N, 3, T, H, W), channels in DATA.MEAN order
    fn = sa.RandomErasing(probability=1.0, mode=mode, max_count=2, noise_seed=11)
    random.seed(N)
    torch.manual_seed(N)
    table = fn.sample_batch(N, (T, 3, H, W))
    assert len(table.rows) >= N
    fd = frames.to(device)
    plain = sa.pack_pathways_u8(fd, cfg)
    same = sa.pack_pathways_u8(fd, cfg, erase=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, same)), "erase=None is the call without erasing"
    erased = re_.erase_clip(norm.clone().to(device), table)
    assert_erased(erased.cpu(), norm, table, "pack reference " + mode)
    inbox = box_mask(table, norm.shape)
    prev = None
    for mix in PACK_MIXES:
        got = sa.pack_pathways_u8(fd, cfg, mix=mix, erase=table)
        unerased = sa.pack_pathways_u8(fd, cfg, mix=mix)
        mixed = erased.clone() if mix is None else mixup.mix_clip(erased.clone(), mix)
        want = _pathways(mixed.cpu(), cfg)
        want[1:] = _pathways(erased.cpu(), cfg)[1:]                     # the reference mixes inputs[0] only
        touched = inbox | inbox.flip(0) if mix is not None else inbox
        masks = _pathways(touched, cfg)
        masks[1:] = _pathways(inbox, cfg)[1:]
        assert len(got) == len(want)
        for p, (g, w_, m, u) in enumerate(zip(got, want, masks, unerased)):
            vals, pad = _unpack(g)
            w16 = w_.to(ACT)
            assert float(pad.abs().max()) == 0.0
            assert torch.equal(vals[~m], _unpack(u)[0][~m]), (p, mix, "outside the boxes the call without erase decides")
            if mode == "pixel":
                off = (_ordered(vals) - _ordered(w16)).abs()
                assert int(off.max()) <= 1, (p, mix, "more than one storage ulp from erase_clip + mix_clip", int(off.max()))
                assert torch.equal(vals[~m], w16[~m])
            else:
                assert torch.equal(vals, w16), (N, mode, arch, reverse, p, mix)
            assert not torch.equal(vals, _unpack(u)[0]), "the case must actually erase"
        if arch == "slowfast":
            fast, slow = _unpack(got[1])[0], _unpack(got[0])[0]
            if mix is None:
                idx = sa.data.pathway_frame_indices(cfg, T)[0]
                assert torch.equal(slow, torch.index_select(fast, 2, idx)), "Slow must be the index_select of Fast"
            assert torch.equal(got[1], sa.pack_pathways_u8(fd, cfg, erase=table)[1]), "Fast is erased but never mixed"
        if prev is not None:                                            # into the buffers of a previous call
            again = sa.pack_pathways_u8(fd, cfg, out=prev, mix=mix, erase=table)
            assert [a.data_ptr() for a in again] == [a.data_ptr() for a in prev]
            assert all(torch.equal(a, b) for a, b in zip(again, got))
        prev = sa.pack_pathways_u8(fd, cfg)


# ---- 7. rejects -------------------------------------------------------------------------------------------------------
def check_rejects(device):
    import pytest
    shape = (2, 3, 6, 10)
    fn = sa.RandomErasing(probability=1.0, mode="pixel")
    x = torch.randn((2, 3, 2, 6, 10)).to(device)
    random.seed(3)
    state = random.getstate()
    for bad in (x[:, :, :, :, ::2], x.to(ACT), x[0], x.permute(0, 1, 2, 4, 3), x[0, :, 0]):
        with pytest.raises(sa.lib.SfError):
            fn(bad)
        assert random.getstate() == state, "a rejected call must not consume random numbers"
    with pytest.raises(sa.lib.SfError, match="single images"):
        fn(x[0, :, 0].contiguous())
    with pytest.raises(sa.lib.SfError):
        fn(x, out=torch.empty((2, 3, 2, 6, 12)).to(device))
    assert random.getstate() == state
    before = x.clone()
    for row in ((0, 0, 2, 4, 0, 3, 4), (0, 0, 2, 0, 8, 2, 3), (0, 0, 3, 0, 0, 2, 2), (0, -1, 2, 0, 0, 2, 2), (2, 0, 2, 0, 0, 2, 2)):
        with pytest.raises(sa.lib.SfError):                 # top + h > H, left + w > W, t_end > T, t_start < 0, sample >= N
            re_.erase_clip(x, re_.make_table([row], "const", shape))
    with pytest.raises(sa.lib.SfError, match="ascending"):
        re_.erase_clip(x, re_.make_table([(1, 0, 2, 0, 0, 2, 2), (0, 0, 2, 0, 0, 2, 2)], "const", shape))
    with pytest.raises(sa.lib.SfError):
        re_.erase_clip(x, re_.make_table([(0, 0, 2, 0, 0, 2, 2)], "const", (2, 3, 6, 12)))
    big = torch.zeros(2 * x.numel()).to(device)
    with pytest.raises(sa.lib.SfError, match="overlap"):
        re_.erase_clip(big[:x.numel()].view(x.shape), re_.make_table([(0, 0, 2, 0, 0, 2, 2)], "const", shape),
                       out=big[4:4 + x.numel()].view(x.shape))
    assert torch.equal(x, before) and random.getstate() == state
    frames = torch.zeros((2, 2, 6, 10, 3), dtype=torch.uint8).to(device)
    with pytest.raises(sa.lib.SfError):
        sa.pack_pathways_u8(frames, sa.get_preset("C2D_8x8_R50"), erase=re_.make_table([(0, 0, 2, 4, 0, 3, 4)], "const", shape))


# ---- 8. config --------------------------------------------------------------------------------------------------------
def check_config():
    cfg = sa.get_cfg()
    assert dict(cfg.AUG) == {"ENABLE": False, "RE_PROB": 0.25, "RE_MODE": "pixel", "RE_COUNT": 1, "RE_SPLIT": False}
    assert sa.construct_random_erasing(cfg) is None
    cfg.AUG.ENABLE = True
    cfg.AUG.RE_PROB = 0.0
    assert sa.construct_random_erasing(cfg) is None
    cfg.AUG.RE_PROB = 0.25
    cfg.AUG.RE_COUNT = 2
    cfg.RNG_SEED = 9
    fn = sa.construct_random_erasing(cfg)
    assert isinstance(fn, sa.RandomErasing)
    assert (fn.probability, fn.min_area, fn.max_area, fn.min_count, fn.max_count, fn.num_splits, fn.cube, fn.per_pixel,
            fn.rand_color, fn.noise_seed) == (0.25, 0.02, 1 / 3, 1, 2, 2, True, True, False, 9)
    assert fn.log_aspect_ratio == (np.log(0.3), np.log(1 / 0.3)) or np.allclose(fn.log_aspect_ratio, (np.log(0.3), -np.log(0.3)))
    plan = sa.RandomErasing(probability=1.0, mode="pixel", num_splits=2, noise_seed=9).sample_params((8, 3, 16, 16))
    assert plan.rows and all(r[0] == 4 and r[1] == 8 for r in plan.rows), "num_splits 2 leaves the first T // 2 frames clean"
    # pixel keys come from the private generator, in row order, and leave the global one alone
    random.seed(1)
    a = sa.RandomErasing(probability=1.0, mode="pixel", noise_seed=9).sample_params((8, 3, 16, 16))
    state = random.getstate()
    random.seed(1)
    b = sa.RandomErasing(probability=1.0, mode="pixel", noise_seed=10).sample_params((8, 3, 16, 16))
    assert random.getstate() == state and a.rows == b.rows and a.keys != b.keys
    assert a.keys == [random.Random(9).getrandbits(64)]


# ---- 9. step glue -----------------------------------------------------------------------------------------------------
def run_erase_mix_step(device, use_graph, steps=4):
    """``steps`` iterations of TrainStep on mvit_tiny with MIXUP.ENABLE and AUG.RE_PROB 1.0: the batch is erased in place, then
    mixed in place (eager) or straight into the captured step's static buffers.  Returns (losses, parameters, tables)."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    from slowfast_amd.step import TrainStep
    from tests import mixup_checks
    from tests import model_checks as mc
    gold = mc.load_golden("mvit_tiny")
    cfg = mc.cfg_for(gold, extra=["MIXUP.ENABLE", True, "AUG.ENABLE", True, "AUG.RE_PROB", 1.0])
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
    mix, erase = sa.construct_mixup(cfg), sa.construct_random_erasing(cfg)
    assert mix is not None and erase is not None and erase.per_pixel and len(inputs) == 1
    np.random.seed(mixup_checks.STEP_SEED)
    random.seed(mixup_checks.STEP_SEED)
    tables, losses, via_static = [], [], 0
    sample = erase.sample_batch
    erase.sample_batch = lambda N, shape: tables.append(sample(N, shape)) or tables[-1]
    K = cfg.MODEL.NUM_CLASSES
    for it in range(steps):
        clip = (inputs[0] * (1.0 + 0.125 * it)).to(device)
        y = ((labels + it) % K).to(device)
        y[1] = (y[0] + 3) % K
        static = step.static_inputs()
        assert erase(clip).data_ptr() == clip.data_ptr()
        if static is None:
            x, t = mix(clip, y)
            loss = step([x], t)
        else:
            x, t = mix(clip, y, out=static[0][0], target_out=static[1])
            loss = step(*static)
            via_static += 1
        losses.append(float(loss))
    assert via_static == (max(0, steps - 2) if use_graph else 0)
    params = [p.detach().float().cpu().clone() for p in model.parameters()]
    red.close()
    return losses, params, tables
