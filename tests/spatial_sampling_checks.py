"""Spatial-sampling checks shared by the CPU (host simulator) and GPU (-m gpu) test files (csrc/sf_sample.h,
slowfast_amd/spatial_sampling.py, data.pack_pathways_u8(crop=)).

tests/golden/spatial_sampling_contract.json holds what the reference itself did (tools/make_spatial_sampling_golden.py): per
case the rows its draw implies, how far ``random`` and ``np.random`` got, and its fp32 output for uint8 frames this file draws
again.  Rows and generator positions are compared exactly.  Values are compared within VALUE_BOUND: the kernel evaluates the
coordinate rule and the blend in one fixed order without contraction, torch's CPU kernels in theirs, so the two differ by
rounding -- the bound is 8 x the larger of the deviations measured on the host simulator and on an MI355X
(profiles/spatial_sampling_parity.md), the margin random_erasing_checks.py uses, and must stay below 1 % of the smallest
one-pixel-shift difference of the fixture: a wrong tap, a half-pixel error or a mirrored axis gives a difference of that
order and cannot pass.  Where a row resizes nothing the output is compared BIT FOR BIT with the normalised source pixels.

The packed path is compared as random_erasing_checks.check_pack compares its own: the yardstick is the fp32 kernel's output,
erased by erase_clip, mixed by mix_clip and rounded once to the storage type.
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
from slowfast_amd import spatial_sampling as ss
from slowfast_amd.mixup import MixParams
from tests.random_erasing_checks import _ordered, _pathways, _unpack, bits

ACT = _sflib.act_dtype()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_sampling_contract.json")
with open(GOLDEN) as _f:
    CONTRACT = json.load(_f)
CASES = CONTRACT["cases"]
NUM_GOLDEN_CASES = len(CASES)
S, MEAN, STD = CONTRACT["crop_size"], CONTRACT["mean"], CONTRACT["std"]

# largest |kernel - reference| over all golden cases (profiles/spatial_sampling_parity.md)
VALUE_MEASURED = {"hostsim": 4.173e-06, "mi355x": 4.173e-06}
VALUE_BOUND = 8.0 * max(VALUE_MEASURED.values())
SMALLEST_SHIFT = min(c["shift_diff"] for c in CASES)
assert VALUE_BOUND < 0.01 * SMALLEST_SHIFT, (VALUE_BOUND, SMALLEST_SHIFT)


# ---- the fixture's inputs ---------------------------------------------------------------------------------------------
def case_frames(case):
    """The uint8 (T, h, w, 3) frames of every sample, drawn as tools/make_spatial_sampling_golden.py draws them."""
    g = torch.Generator().manual_seed(case["data_seed"])
    return [torch.randint(0, 256, (case["T"], h, w, 3), generator=g, dtype=torch.int64).to(torch.uint8) for h, w in case["sizes"]]


def padded(frames, fill=255):
    """Samples of different sizes in one (N, T, Hs, Ws, 3) buffer, the padding filled with ``fill``: a read outside the valid
    size shows."""
    Hs, Ws = max(f.shape[1] for f in frames), max(f.shape[2] for f in frames)
    buf = torch.full((len(frames), frames[0].shape[0], Hs, Ws, 3), fill, dtype=torch.uint8)
    for n, f in enumerate(frames):
        buf[n, :, :f.shape[1], :f.shape[2]] = f
    return buf


def normalise(frames, mean=None, std=None):
    """tensor_normalize + permute of one sample: uint8 (T, H, W, 3) -> fp32 (3, T, H, W), the arithmetic of sf_pack_clip_u8."""
    x = frames.float() / 255.0
    x = x - torch.tensor(MEAN if mean is None else mean)
    x = x / torch.tensor(STD if std is None else std)
    return x.permute(3, 0, 1, 2).contiguous()


def case_want(case):
    N = len(case["sizes"])
    return torch.from_numpy(np.frombuffer(base64.b64decode(case["out"]), dtype="<f4").copy()).view(N, 3, case["T"], S, S)


def draw_case(case):
    """The case's draw under its seeds: (CropTable, random.random() after, np.random.uniform() after)."""
    fn = sa.SpatialSampling(**case["args"])
    random.seed(case["seed"])
    np.random.seed(case["seed"])
    table = fn.sample_batch(case["sizes"], spatial_idx=case["spatial_idx"])
    return table, random.random(), float(np.random.uniform())


# ---- 1. the reference's own results -----------------------------------------------------------------------------------
def golden_deviation(device, index):
    """Rows and generator positions exactly; returns the largest |kernel - reference| of the case."""
    case = CASES[index]
    table, py_after, np_after = draw_case(case)
    assert isinstance(table, sa.CropTable) and table.rows.dtype == np.int32 and table.crop_size == S
    assert table.rows.tolist() == case["rows"], ("rows differ from the reference's draw", table.rows.tolist(), case["rows"])
    assert repr(py_after) == case["py_after"], "random was not consumed as the reference consumes it"
    assert repr(np_after) == case["np_after"], "np.random was not consumed as the reference consumes it"
    # the same draw clip by clip
    fn = sa.SpatialSampling(**case["args"])
    random.seed(case["seed"])
    np.random.seed(case["seed"])
    idxs = case["spatial_idx"] or [None] * len(case["sizes"])
    rows = [fn.sample_params(h, w, i) for (h, w), i in zip(case["sizes"], idxs)]
    assert all(isinstance(r, sa.CropRow) for r in rows) and [list(r) for r in rows] == case["rows"]
    assert repr(random.random()) == case["py_after"] and repr(float(np.random.uniform())) == case["np_after"]

    frames = case_frames(case)
    buf = padded(frames).to(device)
    got = sa.sample_clip(buf, table, MEAN, STD)
    assert tuple(got.shape) == (len(frames), 3, case["T"], S, S) and got.dtype == torch.float32
    into = torch.full(got.shape, float("nan")).to(device)
    assert sa.sample_clip(buf, table, MEAN, STD, out=into).data_ptr() == into.data_ptr()
    assert torch.equal(bits(into.cpu()), bits(got.cpu())), "out= differs"
    got, want = got.cpu(), case_want(case)
    dev = float((got.double() - want.double()).abs().max())
    for n, r in enumerate(table.rows.tolist()):             # nothing resized: the normalised source pixels, bit for bit
        r = sa.CropRow(*r)
        if (r.win_h, r.win_w) == (r.res_h, r.res_w):
            src = normalise(frames[n])[:, :, r.win_y + r.off_y:r.win_y + r.off_y + S, r.win_x + r.off_x:r.win_x + r.off_x + S]
            src = src.flip(-1) if r.flip else src
            assert torch.equal(bits(got[n]), bits(src)), (index, n, "an unresized crop must copy the normalised pixels")
            cfg = sa.get_preset("C2D_8x8_R50", ["DATA.MEAN", MEAN, "DATA.STD", STD])
            u8 = frames[n][:, r.off_y:r.off_y + S, r.off_x:r.off_x + S]
            u8 = (u8.flip(2) if r.flip else u8).contiguous()[None].to(device)
            assert torch.equal(_unpack(sa.pack_pathways_u8(u8, cfg)[0])[0][0], got[n].to(ACT)), "sf_pack_clip_u8 differs"
    return dev


def check_golden_case(device, index):
    dev = golden_deviation(device, index)
    print("case %d (%s): max |kernel - reference| = %.3e (bound %.3e, 1 %% of the smallest shift %.3e)" % (
        index, CASES[index]["name"], dev, VALUE_BOUND, 0.01 * SMALLEST_SHIFT))
    assert dev <= VALUE_BOUND, (index, dev, VALUE_BOUND)


def check_window_clamp(device):
    """A window strictly inside the frame, surrounded by 255: the resized window never reads its surroundings (a clamp to the
    frame instead of the window would): bit for bit what the same kernel gives for the window alone in its own buffer."""
    T, H, W = 2, 18, 26
    g = torch.Generator().manual_seed(5)
    win = torch.randint(0, 128, (T, 7, 9, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    frames = torch.full((1, T, H, W, 3), 255, dtype=torch.uint8)
    frames[0, :, 4:11, 6:15] = win
    for flip in (0, 1):
        table = ss.make_table([(H, W, 4, 6, 7, 9, S, S, 0, 0, flip)], S)
        alone = ss.make_table([(7, 9, 0, 0, 7, 9, S, S, 0, 0, flip)], S)
        got = sa.sample_clip(frames.to(device), table, MEAN, STD).cpu()
        want = sa.sample_clip(win[None].contiguous().to(device), alone, MEAN, STD).cpu()
        assert torch.equal(bits(got), bits(want)), "a tap was taken from outside the window"
        assert float(got.max()) <= float(normalise(win).max()) + 1e-6, "a surrounding 255 leaked into the window"


# ---- 2. packed path ---------------------------------------------------------------------------------------------------
PACK_MIXES = (None, MixParams(0.3, False, None), MixParams(0.6, True, (3, 9, 4, 11)))
PACK_SIZES = [(18, 26), (26, 18), (22, 24)]


def pack_inputs(N, T, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = PACK_SIZES[:N]
    frames = [torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.int64).to(torch.uint8) for h, w in sizes]
    fn = sa.SpatialSampling(min_scale=14, max_scale=20, crop_size=S)
    random.seed(seed)
    np.random.seed(seed)
    crop = fn.sample_batch(sizes)
    assert crop.rows[0].tolist() != crop.rows[-1].tolist(), "the partner's row must differ"
    return padded(frames), crop


def check_pack(device, N, mode, arch="c2d", reverse=False):
    """``mode``: None (crop alone) or the erase mode."""
    cfg = sa.get_preset("SLOWFAST_8x8_R50" if arch == "slowfast" else "C2D_8x8_R50",
                        ["DATA.MEAN", MEAN, "DATA.STD", STD, "DATA.REVERSE_INPUT_CHANNEL", reverse])
    T = 8 if arch == "slowfast" else 3
    buf, crop = pack_inputs(N, T, 40 + N)
    fd = buf.to(device)
    clip = sa.sample_clip(fd, crop, MEAN, STD)                            # the yardstick, fp32 (N, 3, T, S, S)
    table = None
    if mode is not None:
        fn = sa.RandomErasing(probability=1.0, mode=mode, max_count=2, noise_seed=11)
        random.seed(N)
        torch.manual_seed(N)
        table = fn.sample_batch(N, (T, 3, S, S))
        assert len(table.rows) >= N
    erased = clip.clone() if table is None else re_.erase_clip(clip.clone(), table)
    prev = None
    for mix in PACK_MIXES if (mode is not None or arch == "c2d") else PACK_MIXES[:1]:
        got = sa.pack_pathways_u8(fd, cfg, crop=crop, erase=table, mix=mix)
        mixed = erased.clone() if mix is None else mixup.mix_clip(erased.clone(), mix)
        want = _pathways(mixed.cpu(), cfg)
        want[1:] = _pathways(erased.cpu(), cfg)[1:]                     # the reference mixes inputs[0] only
        assert len(got) == len(want)
        for p, (g, w_) in enumerate(zip(got, want)):
            vals, pad = _unpack(g)
            w16 = w_.to(ACT)
            assert float(pad.abs().max()) == 0.0
            if mode == "pixel":                                         # erase_noise1 against erase_noise4: one storage ulp
                off = (_ordered(vals) - _ordered(w16)).abs()
                assert int(off.max()) <= 1, (p, mix, "more than one storage ulp from sample_clip + erase_clip + mix_clip")
            else:
                assert torch.equal(vals, w16), (N, mode, arch, reverse, p, mix)
        if arch == "slowfast":
            fast, slow = _unpack(got[1])[0], _unpack(got[0])[0]
            if mix is None:
                idx = sa.data.pathway_frame_indices(cfg, T)[0]
                assert torch.equal(slow, torch.index_select(fast, 2, idx)), "Slow must be the index_select of Fast"
            assert torch.equal(got[1], sa.pack_pathways_u8(fd, cfg, crop=crop, erase=table)[1]), "Fast is never mixed"
        if prev is not None:                                            # into the buffers of a previous call
            again = sa.pack_pathways_u8(fd, cfg, out=prev, crop=crop, erase=table, mix=mix)
            assert [a.data_ptr() for a in again] == [a.data_ptr() for a in prev]
            assert all(torch.equal(a, b) for a, b in zip(again, got))
        prev = sa.pack_pathways_u8(fd, cfg, crop=crop)
    if table is not None:
        plain = sa.pack_pathways_u8(fd, cfg, crop=crop)
        assert not torch.equal(plain[0], sa.pack_pathways_u8(fd, cfg, crop=crop, erase=table)[0]), "the case must erase"


def check_pack_without_crop(device):
    """crop=None reaches the three older kernels with the arguments of a direct call: bit-identical buffers."""
    cfg = sa.get_preset("C2D_8x8_R50", ["DATA.MEAN", MEAN, "DATA.STD", STD])
    N, T, H, W = 2, 3, 12, 20
    frames = torch.randint(0, 256, (N, T, H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.int64)
    fd = frames.to(torch.uint8).to(device)
    random.seed(2)
    table = sa.RandomErasing(probability=1.0, mode="const").sample_batch(N, (T, 3, H, W))
    host, dev, R = re_.upload_table(table, N, fd.device)
    stream = sa.ops._stream(fd)
    lib = _sflib.get_lib()
    head = (fd.data_ptr(), N, T, H, W, None, T, MEAN[0], MEAN[1], MEAN[2], STD[0], STD[1], STD[2], 0)
    lam, oml = mixup._f32_pair(0.3)

    def direct(name, *tail):
        out = torch.zeros((N, T, H, W // 2, 8), dtype=ACT, device=fd.device)
        lib.call(name, *head, out.data_ptr(), *tail, stream)
        return out.permute(0, 4, 1, 2, 3)

    mix = MixParams(0.3, False, None)
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        a = sa.pack_pathways_u8(fd, cfg, crop=None)[0]
        b = sa.pack_pathways_u8(fd, cfg, crop=None, mix=mix)[0]
        c = sa.pack_pathways_u8(fd, cfg, crop=None, mix=mix, erase=table)[0]
    finally:
        _sflib.set_call_observer(None)
    assert calls == ["sf_pack_clip_u8", "sf_pack_clip_u8_mix", "sf_pack_clip_u8_aug"], calls
    assert torch.equal(a, direct("sf_pack_clip_u8"))
    assert torch.equal(b, direct("sf_pack_clip_u8_mix", 0, lam, oml, 0, 0, 0, 0))
    assert torch.equal(c, direct("sf_pack_clip_u8_aug", 0, host.ctypes.data, dev.data_ptr(), R, int(host.size), 0, lam, oml,
                                 0, 0, 0, 0))


def words16(x):
    """The 16-bit storage words of a packed tensor."""
    return x.contiguous().view(torch.int16).cpu()


def check_pack_entry_points_agree(device):
    """The four packed entry points are one computation with stages switched off, so where their stages coincide their outputs
    are equal bit for bit on the storage words: (1) an identity crop row (nothing resized, nothing cut, no flip) makes
    sf_pack_clip_u8_sample the crop=None call, under every erase mode and mixing; (2) sf_pack_clip_u8_aug without an erase
    table and without mixing is sf_pack_clip_u8; (3) without an erase table and with mixing it is sf_pack_clip_u8_mix.
    N = 3 is odd (the middle sample is its own partner), 3 * 3 * 144 pixels are five workgroups and a tail of 16, and the
    cutmix box has odd column edges."""
    N, H = 3, 12
    identity = ss.make_table([sa.CropRow(H, H, 0, 0, H, H, H, H, 0, 0, 0)] * N, H)
    mixes = (None, MixParams(0.3, False, None), MixParams(0.3, True, (3, 9, 5, 11)))
    for preset, T in (("C2D_8x8_R50", 3), ("SLOWFAST_8x8_R50", 8)):
        frames = torch.randint(0, 256, (N, T, H, H, 3), generator=torch.Generator().manual_seed(17 + T), dtype=torch.int64)
        fd = frames.to(torch.uint8).to(device)
        for reverse in (False, True):
            cfg = sa.get_preset(preset, ["DATA.MEAN", MEAN, "DATA.STD", STD, "DATA.REVERSE_INPUT_CHANNEL", reverse])
            for mode in (None, "const", "rand", "pixel"):
                table = None
                if mode is not None:
                    random.seed(N)
                    torch.manual_seed(N)
                    table = sa.RandomErasing(probability=1.0, mode=mode, max_count=2, noise_seed=11).sample_batch(N, (T, 3, H, H))
                    assert len(table.rows) >= N
                for mix in mixes:
                    got = sa.pack_pathways_u8(fd, cfg, crop=identity, erase=table, mix=mix)
                    want = sa.pack_pathways_u8(fd, cfg, erase=table, mix=mix)
                    assert len(got) == len(want) == (2 if preset.startswith("SLOWFAST") else 1)
                    for p, (g, w_) in enumerate(zip(got, want)):
                        assert g.shape == w_.shape and torch.equal(words16(g), words16(w_)), (preset, reverse, mode, mix, p)

    T = 3
    fd = torch.randint(0, 256, (N, T, H, H, 3), generator=torch.Generator().manual_seed(5), dtype=torch.int64).to(torch.uint8).to(device)
    stream = sa.ops._stream(fd)
    lib = _sflib.get_lib()
    head = (fd.data_ptr(), N, T, H, H, None, T, MEAN[0], MEAN[1], MEAN[2], STD[0], STD[1], STD[2], 0)
    lam, oml = mixup._f32_pair(0.3)
    no_table = (0, None, None, 0, 0)

    def direct(name, *tail):
        out = torch.zeros((N, T, H, H // 2, 8), dtype=ACT, device=fd.device)
        lib.call(name, *head, out.data_ptr(), *tail, stream)
        return words16(out)

    assert torch.equal(direct("sf_pack_clip_u8_aug", *no_table, -1, 1.0, 0.0, 0, 0, 0, 0), direct("sf_pack_clip_u8"))
    for mix_tail in ((0, lam, oml, 0, 0, 0, 0), (1, lam, oml, 3, 9, 5, 11)):
        assert torch.equal(direct("sf_pack_clip_u8_aug", *no_table, *mix_tail), direct("sf_pack_clip_u8_mix", *mix_tail)), mix_tail


def generator_state():
    """Python's and numpy's global generator states, comparable with ==."""
    s = np.random.get_state()
    return random.getstate(), s[1].tobytes(), tuple(s[2:])


# ---- 3. rejects -------------------------------------------------------------------------------------------------------
GOOD_ROW = (18, 26, 0, 0, 18, 26, 15, 21, 1, 2, 0)
# one row per REQUIRE of check_crop_table (csrc/sf_api.hip)
BAD_ROWS = {
    "valid size outside the buffer": (19, 26, 0, 0, 18, 26, 15, 21, 1, 2, 0),
    "valid size not positive": (18, 0, 0, 0, 18, 26, 15, 21, 1, 2, 0),
    "window outside the valid size (rows)": (18, 26, 2, 0, 17, 26, 15, 21, 1, 2, 0),
    "window outside the valid size (columns)": (18, 24, 0, 0, 18, 26, 15, 21, 1, 2, 0),
    "window at a negative offset": (18, 26, 0, -1, 18, 26, 15, 21, 1, 2, 0),
    "empty window": (18, 26, 0, 0, 0, 26, 15, 21, 1, 2, 0),
    "resized size not positive": (18, 26, 0, 0, 18, 26, 15, 0, 1, 2, 0),
    "resized size too large": (18, 26, 0, 0, 18, 26, 15, 70000, 1, 2, 0),
    "crop outside the resized size (rows)": (18, 26, 0, 0, 18, 26, 15, 21, 4, 2, 0),
    "crop outside the resized size (columns)": (18, 26, 0, 0, 18, 26, 15, 21, 1, 10, 0),
    "crop at a negative offset": (18, 26, 0, 0, 18, 26, 15, 21, -1, 2, 0),
    "resized smaller than the crop": (18, 26, 0, 0, 18, 26, 11, 21, 0, 2, 0),
    "flip neither 0 nor 1": (18, 26, 0, 0, 18, 26, 15, 21, 1, 2, 2),
}


def check_rejects(device):
    import pytest
    T, H, W = 2, 18, 26
    frames = torch.randint(0, 256, (2, T, H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.int64)
    fd = frames.to(torch.uint8).to(device)
    cfg = sa.get_preset("C2D_8x8_R50")
    fn = sa.SpatialSampling(min_scale=14, max_scale=20, crop_size=S)
    random.seed(3)
    np.random.seed(3)
    snapshot = generator_state
    state = snapshot()
    good = ss.make_table([GOOD_ROW, GOOD_ROW], S)
    out = torch.full((2, 3, T, S, S), 7.0).to(device)
    packed = sa.pack_pathways_u8(fd, cfg, crop=good)
    before = [p.clone() for p in packed]
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        # the frames: dtype, rank, channel count, contiguity -- before any draw
        for bad in (fd.float(), fd[0], fd[..., :2], fd[:, :, :, ::2], fd.permute(0, 1, 3, 2, 4)):
            with pytest.raises(sa.lib.SfError):
                fn(bad, MEAN, STD)
            with pytest.raises(sa.lib.SfError):
                sa.sample_clip(bad, good, MEAN, STD)
            with pytest.raises(sa.lib.SfError):
                sa.pack_pathways_u8(bad, cfg, crop=good)
            assert snapshot() == state, "a rejected call must not consume random numbers"
        assert calls == [], "rejected frames never reach the library"
        # out=
        for bad_out in (out[:, :, :, :, ::2], out.double(), torch.empty((2, 3, T, S, S + 2)).to(device)):
            with pytest.raises(sa.lib.SfError):
                sa.sample_clip(fd, good, MEAN, STD, out=bad_out)
        with pytest.raises(sa.lib.SfError):
            sa.pack_pathways_u8(fd, cfg, crop=good, out=[torch.empty((2, 8, T, S, S)).to(device)])
        # a table drawn for another N
        with pytest.raises(sa.lib.SfError, match="drawn for 1 samples"):
            sa.sample_clip(fd, ss.make_table([GOOD_ROW], S), MEAN, STD, out=out)
        with pytest.raises(sa.lib.SfError, match="drawn for 3 samples"):
            sa.pack_pathways_u8(fd, cfg, crop=ss.make_table([GOOD_ROW] * 3, S), out=packed)
        assert calls == []
        # every REQUIRE on a row, on the host copy of the table: the message names the row, nothing is launched
        for what, row in BAD_ROWS.items():
            bad = ss.make_table([GOOD_ROW, row], S)
            with pytest.raises(sa.lib.SfError, match="crop row 1"):
                sa.sample_clip(fd, bad, MEAN, STD, out=out)
            with pytest.raises(sa.lib.SfError, match="crop row 1"):
                sa.pack_pathways_u8(fd, cfg, crop=bad, out=packed)
        # the sizes the index arithmetic assumes
        with pytest.raises(sa.lib.SfError, match="even"):
            sa.pack_pathways_u8(fd, cfg, crop=ss.make_table([(18, 26, 0, 0, 18, 26, 15, 21, 1, 2, 0)] * 2, S - 1))
        with pytest.raises(sa.lib.SfError, match="zero std"):
            sa.sample_clip(fd, good, MEAN, [0.2, 0.0, 0.2], out=out)
        # an erase table that was not drawn for the cropped clip (T, 3, S, S); one whose row leaves it
        for shape in ((T, 3, H, W), (T + 1, 3, S, S)):
            with pytest.raises(sa.lib.SfError, match="erase table was drawn"):
                sa.pack_pathways_u8(fd, cfg, crop=good, erase=re_.make_table([(0, 0, T, 0, 0, 2, 2)], "const", shape), out=packed)
        with pytest.raises(sa.lib.SfError, match="lies outside"):
            sa.pack_pathways_u8(fd, cfg, crop=good, erase=re_.make_table([(0, 0, T, S - 1, 0, 2, 2)], "const", (T, 3, S, S)),
                                out=packed)
        # a cutmix box outside the S x S plane
        with pytest.raises(sa.lib.SfError, match="outside"):
            sa.pack_pathways_u8(fd, cfg, crop=good, mix=MixParams(0.5, True, (0, S + 1, 0, 4)), out=packed)
    finally:
        _sflib.set_call_observer(None)
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0, "a rejected call wrote its output"
    assert all(torch.equal(a, b) for a, b in zip(packed, before)), "a rejected call wrote its output"
    assert snapshot() == state
    # the draw itself: a frame that would be resized below the crop is rejected before any draw
    small = sa.SpatialSampling(min_scale=S - 2, max_scale=20, crop_size=S)
    for call in (lambda: small.sample_params(18, 26), lambda: small.sample_batch([(18, 26)] * 2),
                 lambda: sa.SpatialSampling(spatial_idx=1, min_scale=S - 1, max_scale=S - 1, crop_size=S).sample_params(18, 26),
                 lambda: fn.sample_params(18, 26, spatial_idx=1),      # test path with min_scale != max_scale
                 lambda: fn.sample_params(18, 26, spatial_idx=3), lambda: fn.sample_params(0, 26),
                 lambda: fn.sample_batch([(18, 26)] * 2, spatial_idx=[1])):
        with pytest.raises(sa.lib.SfError):
            call()
        assert snapshot() == state
    with pytest.raises(NotImplementedError):
        sa.SpatialSampling(min_scale=14, max_scale=20, crop_size=S, motion_shift=True)
    with pytest.raises(sa.lib.SfError):
        sa.SpatialSampling(min_scale=14, max_scale=20, crop_size=S, scale=[0.3, 1.0])
    assert snapshot() == state


def check_host_tensor_rejected():
    """With the gfx950 library a host tensor raises (there is no torch fallback) and consumes no random number."""
    import pytest
    frames = torch.zeros((2, 2, 18, 26, 3), dtype=torch.uint8)
    fn = sa.SpatialSampling(min_scale=14, max_scale=20, crop_size=S)
    random.seed(3)
    np.random.seed(3)
    state = generator_state()
    good = ss.make_table([GOOD_ROW, GOOD_ROW], S)
    for call in (lambda: fn(frames, MEAN, STD), lambda: sa.sample_clip(frames, good, MEAN, STD),
                 lambda: sa.pack_pathways_u8(frames, sa.get_preset("C2D_8x8_R50"), crop=good)):
        with pytest.raises(sa.lib.SfError):
            call()
    assert generator_state() == state


# ---- 4. config --------------------------------------------------------------------------------------------------------
def check_config():
    import pytest
    cfg = sa.get_cfg()
    assert (cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE,
            cfg.DATA.TRAIN_JITTER_MOTION_SHIFT, cfg.DATA.INV_UNIFORM_SAMPLE, cfg.DATA.RANDOM_FLIP,
            cfg.TEST.NUM_SPATIAL_CROPS) == ([256, 320], [], [], False, False, True, 3)

    def fields(f):
        return (f.spatial_idx, f.min_scale, f.max_scale, f.crop_size, f.random_horizontal_flip, f.inverse_uniform_sampling,
                f.aspect_ratio, f.scale)
    assert fields(sa.construct_spatial_sampling(cfg, "train")) == (-1, 256, 320, 224, True, False, None, None)
    assert fields(sa.construct_spatial_sampling(cfg, "val")) == (-1, 256, 320, 224, True, False, None, None)
    assert fields(sa.construct_spatial_sampling(cfg, "test")) == (1, 256, 256, 256, True, False, None, None)
    cfg.TEST.NUM_SPATIAL_CROPS = 1
    cfg.DATA.TEST_CROP_SIZE = 224
    assert fields(sa.construct_spatial_sampling(cfg, "test")) == (1, 256, 256, 224, True, False, None, None)
    cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE = [0.08, 1.0]
    cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE = [0.75, 1.3333]
    cfg.DATA.RANDOM_FLIP = False
    cfg.DATA.INV_UNIFORM_SAMPLE = True
    assert fields(sa.construct_spatial_sampling(cfg, "train")) == (-1, 256, 320, 224, False, True, (0.75, 1.3333), (0.08, 1.0))
    assert fields(sa.construct_spatial_sampling(cfg, "val")) == (-1, 256, 320, 224, False, True, None, None)
    assert fields(sa.construct_spatial_sampling(cfg, "test")) == (1, 256, 256, 224, False, True, None, None)
    cfg.DATA.TRAIN_JITTER_MOTION_SHIFT = True
    assert sa.construct_spatial_sampling(cfg, "val").motion_shift is False
    with pytest.raises(NotImplementedError):
        sa.construct_spatial_sampling(cfg, "train")
    cfg.DATA.TRAIN_JITTER_MOTION_SHIFT = False
    with pytest.raises(NotImplementedError):
        sa.construct_spatial_sampling(cfg, "predict")
    cfg.merge_from_list(["MULTIGRID.DEFAULT_S", 224])
    with pytest.raises(sa.lib.SfError, match="multigrid"):
        sa.construct_spatial_sampling(cfg, "train")


# ---- 5. step glue -----------------------------------------------------------------------------------------------------
STEP_SEED = 7


def run_sample_step(device, use_graph, steps=4):
    """``steps`` iterations of TrainStep on mvit_tiny (its patch embedding is a StemConvUnit, so it takes the packed clip) with
    MIXUP.ENABLE and AUG.RE_PROB 1.0: decoded frames of two sizes are sampled, erased and mixed by ONE pack_pathways_u8 call,
    into fresh buffers while the step runs eagerly and straight into the captured step's static inputs afterwards.  Returns
    (losses, parameters, crop tables)."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    from slowfast_amd.step import TrainStep
    from tests import model_checks as mc
    gold = mc.load_golden("mvit_tiny")
    cfg = mc.cfg_for(gold, extra=["MIXUP.ENABLE", True, "AUG.ENABLE", True, "AUG.RE_PROB", 1.0])
    model, sd, inputs, labels, *_ = mc.oracle_run(gold, cfg)
    N, _, T, Sc, _ = inputs[0].shape
    assert Sc == cfg.DATA.TRAIN_CROP_SIZE and Sc % 2 == 0 and N == 2
    cfg.DATA.TRAIN_JITTER_SCALES = [Sc + 2, Sc + 8]
    model.load_state_dict(sd)
    model = model.to(device).train()
    red = GradReducer(model, bucket_mb=0.05)
    red.attach_torch_param_hooks(model.head.parameters())
    opt = construct_optimizer(model, cfg, red, loss_scale=64.0, dynamic_loss_scale=False)
    for g in opt.param_groups:
        g["lr"] = 0.01
    loss_fn = sa.get_loss_func("soft_cross_entropy")(reduction="mean")
    step = TrainStep(model, red, opt, loss_fn, use_graph=use_graph, warmup=1, track_stats=True)
    sampler, mix, erase = sa.construct_spatial_sampling(cfg, "train"), sa.construct_mixup(cfg), sa.construct_random_erasing(cfg)
    assert mix is not None and erase is not None and len(inputs) == 1
    np.random.seed(STEP_SEED)
    random.seed(STEP_SEED)
    g = torch.Generator().manual_seed(STEP_SEED)
    sizes = [(Sc + 6, Sc + 14), (Sc + 12, Sc + 4)]
    tables, losses, via_static = [], [], 0
    K = cfg.MODEL.NUM_CLASSES
    for it in range(steps):
        frames = padded([torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.int64).to(torch.uint8) for h, w in sizes])
        y = ((labels + it) % K).to(device)
        y[1] = (y[0] + 3) % K
        crop = sampler.sample_batch(sizes)
        etab = erase.sample_batch(N, (T, 3, Sc, Sc))
        mp = mix.sample_params((N, 3, T, Sc, Sc))
        tables.append(crop)
        static = step.static_inputs()
        if static is None:
            xs = sa.pack_pathways_u8(frames.to(device), cfg, crop=crop, erase=etab, mix=mp)
            loss = step(xs, mix.mix_targets(y, mp.lam))
        else:
            xs = sa.pack_pathways_u8(frames.to(device), cfg, crop=crop, erase=etab, mix=mp, out=static[0])
            assert xs[0].data_ptr() == static[0][0].data_ptr()
            mix.mix_targets(y, mp.lam, out=static[1])
            loss = step(*static)
            via_static += 1
        losses.append(float(loss))
    assert via_static == (max(0, steps - 2) if use_graph else 0)
    params = [p.detach().float().cpu().clone() for p in model.parameters()]
    red.close()
    return losses, params, tables
