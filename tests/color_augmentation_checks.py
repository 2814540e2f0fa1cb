"""Colour-augmentation checks shared by the CPU (host simulator) and GPU (-m gpu) test files (csrc/sf_color.h,
slowfast_amd/color_augmentation.py, spatial_sampling.transform_boxes / collate_boxes / construct_ava_sampling).

tests/golden/color_augmentation_contract.json holds what the reference itself did (tools/make_color_augmentation_golden.py):
per case the drawn op order, blend factors and PCA term, how far ``np.random`` got, its fp32 output for uint8 frames this file
draws again and -- for the whole-pipeline cases -- its boxes.  The draw (as the 32-bit words of the table) and the generator
position are compared exactly, the boxes bit for bit.  Values are compared within VALUE_BOUND: the kernels evaluate every
blend in one fixed order without contraction and take the frame mean in their own summation order, torch's CPU kernels in
theirs, so the two differ by rounding -- the bound is 8 x the larger of the deviations measured on the host simulator and on an
MI355X (profiles/color_augmentation_parity.md), the margin spatial_sampling_checks.py uses, and must stay below 1 % of the
smallest effect of a deliberately wrong variant recorded in the fixture (the contrast mean over the whole clip, the PCA term
indexed without the reversal, the R and B grey weights swapped): such a mistake cannot pass.  With nothing switched on the
output is compared BIT FOR BIT with ``(x - mean) / std`` of the input.

The frame means are compared at kernel level with the fp64 mean of the same fp32 values; the bound there follows from the
summation depth the library states (sf_color_sum_depth) and is asserted to be too tight for a dropped pixel.
"""
import base64
import itertools
import json
import os
import random

import numpy as np
import torch

import slowfast_amd as sa
from slowfast_amd import color_augmentation as ca
from slowfast_amd import lib as _sflib
from slowfast_amd import spatial_sampling as ss
from tests.random_erasing_checks import bits
from tests.spatial_sampling_checks import generator_state, padded

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_augmentation_contract.json")
with open(GOLDEN) as _f:
    CONTRACT = json.load(_f)
CASES = CONTRACT["cases"]
NUM_GOLDEN_CASES = len(CASES)
COLOR_CASES = [i for i, c in enumerate(CASES) if c["kind"] == "color"]
PIPELINE_CASES = [i for i, c in enumerate(CASES) if c["kind"] == "pipeline"]
S, T, MEAN, STD = CONTRACT["crop_size"], CONTRACT["T"], CONTRACT["mean"], CONTRACT["std"]
EIGVAL, EIGVEC = CONTRACT["eigval"], CONTRACT["eigvec"]

# largest |kernel - reference| over all golden cases (profiles/color_augmentation_parity.md)
VALUE_MEASURED = {"hostsim": 1.193e-06, "mi355x": 1.193e-06}
VALUE_BOUND = 8.0 * max(VALUE_MEASURED.values())
SMALLEST_EFFECT = min(c["effect_diff"] for c in CASES if c["effect_diff"] is not None)
assert VALUE_BOUND < 0.01 * SMALLEST_EFFECT, (VALUE_BOUND, SMALLEST_EFFECT)

ORDERS = list(itertools.permutations((0, 1, 2)))
W_B, W_G, W_R = (float(np.float32(v)) for v in (0.114, 0.587, 0.299))     # the kernel's fp32 grey weights, as doubles


# ---- the fixture's inputs ---------------------------------------------------------------------------------------------
def case_frames(data_seed, sizes):
    """The uint8 (T, h, w, 3) frames of every sample, drawn as tools/make_color_augmentation_golden.py draws them."""
    g = torch.Generator().manual_seed(data_seed)
    out = []
    for h, w in sizes:
        out.append(torch.stack([torch.stack([torch.randint(20 + 45 * t + 30 * c, 100 + 45 * t + 30 * c, (h, w), generator=g,
                                                           dtype=torch.int64) for c in range(3)], dim=-1)
                                for t in range(T)]).to(torch.uint8))
    return out


def unit_clip(frames):
    """uint8 (T, h, w, 3) frames of N samples of one size -> the [0, 1] fp32 (N, 3, T, h, w) clip (``byte / 255.0``)."""
    return torch.stack([(f.float() / 255.0).permute(3, 0, 1, 2) for f in frames]).contiguous()


def case_want(case):
    N = case.get("N", 1)
    return torch.from_numpy(np.frombuffer(base64.b64decode(case["out"]), dtype="<f4").copy()).view(N, 3, T, S, S)


def fixture_rows(case):
    """The rows the reference's draw implies: (order, alpha, the addition to input channel c = rgb[2 - c])."""
    return [(d["order"], d["alpha"], [0.0] * 3 if d["rgb"] is None else [d["rgb"][2 - c] for c in range(3)]) for d in case["draws"]]


def normalise_only(x, mean, std, reverse):
    """(x - mean) / std per input channel in torch's fp32, then the reordering."""
    y = (x - torch.tensor(mean).view(1, 3, 1, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1, 1)
    return y.flip(1) if reverse else y


# ---- fp64 restatement -------------------------------------------------------------------------------------------------
def restate(x, rows, mean, std, reverse):
    """csrc/sf_color.h in float64 on the fp32 (N, 3, T, H, W) clip, with the table's fp32 factors: (output, the frame means
    contrast used, (N, T), NaN where a row has no contrast)."""
    words = ca.make_table(rows).words
    f = words.view(np.float32)
    out = torch.empty(x.shape, dtype=torch.float64)
    means = torch.full((x.shape[0], x.shape[2]), float("nan"), dtype=torch.float64)
    for n in range(x.shape[0]):
        v = x[n].double().clone()
        for s in range(3):
            op, a, oma = int(words[n, s]), float(f[n, 4 + 2 * s]), float(f[n, 5 + 2 * s])
            gray = (W_R * v[2] + W_G * v[1]) + W_B * v[0]
            if op == 0:
                v = v * a
            elif op == 1:
                means[n] = gray.mean(dim=(1, 2))
                v = v * a + means[n].view(1, -1, 1, 1) * oma
            elif op == 2:
                v = v * a + gray.unsqueeze(0) * oma
        for c in range(3):
            v[c] = (v[c] + float(f[n, 10 + c]) - float(np.float32(mean[c]))) / float(np.float32(std[c]))
        out[n] = v.flip(0) if reverse else v
    return out, means


# ---- 1. the reference's own results -----------------------------------------------------------------------------------
def _augmentation(args):
    args = dict(args)
    return sa.ColorAugmentation(eigval=EIGVAL, eigvec=EIGVEC, mean=MEAN, std=STD, **args)


def color_case_deviation(device, index):
    """Draw and generator position exactly; returns the largest |kernel - reference| of the case."""
    case = CASES[index]
    N = case["N"]
    fn = _augmentation(case["args"])
    np.random.seed(case["seed"])
    table = fn.sample_batch(N)
    np_after = float(np.random.uniform())
    assert isinstance(table, sa.ColorTable) and table.words.dtype == np.int32 and table.words.shape == (N, ca.ROW_WORDS)
    want_words = ca.make_table(fixture_rows(case)).words
    assert table.words.tolist() == want_words.tolist(), ("the draw differs from the reference's", table.words, want_words)
    assert repr(np_after) == case["np_after"], "np.random was not consumed as the reference consumes it"
    np.random.seed(case["seed"])                            # the same draw clip by clip
    rows = [fn.sample_params() for _ in range(N)]
    assert all(isinstance(r, sa.ColorRow) for r in rows) and ca.make_table(rows).words.tolist() == want_words.tolist()
    assert repr(float(np.random.uniform())) == case["np_after"]

    x = unit_clip(case_frames(case["data_seed"], [(S, S)] * N))
    clip = x.clone().to(device)
    got = sa.color_clip(clip, table, MEAN, STD, fn.reverse)
    assert got.data_ptr() == clip.data_ptr(), "color_clip works in place"
    got = got.cpu()
    np.random.seed(case["seed"])                            # the object draws for itself when no table is given
    own = fn(x.clone().to(device)).cpu()
    assert torch.equal(bits(own), bits(got)) and repr(float(np.random.uniform())) == case["np_after"]
    given = fn(x.clone().to(device), table).cpu()
    assert torch.equal(bits(given), bits(got))
    if not any(d["order"] or d["rgb"] is not None for d in case["draws"]):
        assert torch.equal(bits(got), bits(normalise_only(x, MEAN, STD, fn.reverse))), "nothing on: (x - mean) / std bit for bit"
    return float((got.double() - case_want(case).double()).abs().max())


def _pipeline_cfg(case):
    cfg = sa.get_cfg()
    cfg.merge_from_list([
        "DATA.TRAIN_JITTER_SCALES", case["jitter"], "DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S, "DATA.MEAN", MEAN,
        "DATA.STD", STD, "DATA.TRAIN_PCA_EIGVAL", EIGVAL, "DATA.TRAIN_PCA_EIGVEC", EIGVEC, "AVA.TRAIN_USE_COLOR_AUGMENTATION", True,
        "AVA.TRAIN_PCA_JITTER_ONLY", False, "AVA.TEST_FORCE_FLIP", case["force_flip"]])
    return cfg


def pipeline_draw(case):
    """The case's draw through the constructed objects, in the reference's per-clip order (crop, then colour):
    (crop table, colour table, colour object, np.random.uniform() after)."""
    cfg = _pipeline_cfg(case)
    sampler, color = sa.construct_ava_sampling(cfg, case["split"]), sa.construct_color_augmentation(cfg, case["split"])
    np.random.seed(case["seed"])
    h, w = case["size"]
    crop = ss.make_table([sampler.sample_params(h, w)], sampler.crop_size)
    ctab = color.sample_batch(1)
    return crop, ctab, color, float(np.random.uniform())


def pipeline_case_deviation(device, index):
    case = CASES[index]
    crop, ctab, color, np_after = pipeline_draw(case)
    assert repr(np_after) == case["np_after"], "np.random was not consumed as the reference consumes it"
    assert int(crop.rows[0][10]) == case["flip"]
    assert ctab.words.tolist() == ca.make_table(fixture_rows(case)).words.tolist(), "the colour draw differs from the reference's"
    frames = case_frames(case["data_seed"], [tuple(case["size"])])
    clip = sa.sample_clip(padded(frames).to(device), crop, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    got = color(clip, ctab).cpu()
    boxes_in = np.array(case["boxes_in"], dtype=np.float64)
    keep = boxes_in.copy()
    boxes = sa.transform_boxes(crop.rows[0], boxes_in, S)
    assert boxes.dtype == np.float64 and boxes.tobytes() == np.array(case["boxes"], dtype=np.float64).tobytes(), (
        "boxes differ from the reference's", boxes.tolist(), case["boxes"])
    assert boxes_in.tobytes() == keep.tobytes(), "transform_boxes must not modify its input"
    assert any(b[0] == 0.0 or b[2] == S - 1.0 for b in case["boxes"][:2]), "a box of the case must cross the crop border"
    return float((got.double() - case_want(case).double()).abs().max())


def golden_deviation(device, index):
    return (color_case_deviation if CASES[index]["kind"] == "color" else pipeline_case_deviation)(device, index)


def check_golden_case(device, index):
    dev = golden_deviation(device, index)
    print("case %d (%s): max |kernel - reference| = %.3e (bound %.3e, 1 %% of the smallest wrong-variant effect %.3e)" % (
        index, CASES[index]["name"], dev, VALUE_BOUND, 0.01 * SMALLEST_EFFECT))
    assert dev <= VALUE_BOUND, (index, dev, VALUE_BOUND)


# ---- 2. frame means at kernel level -----------------------------------------------------------------------------------
def chunk_pixels():
    """The library's chunk size, read off sf_color_chunks."""
    lib = _sflib.get_lib()
    lo, hi = 1, 1 << 18
    while lo < hi:                                          # the largest HW that is still one chunk
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if lib.call("sf_color_chunks", mid) == 1 else (lo, mid - 1)
    return lo


def kernel_sizes():
    """S = 13 (unaligned planes, one chunk) and the smallest even S whose frame spans more than one chunk with a remainder."""
    chunk = chunk_pixels()
    even = next(s for s in range(2, 2048, 2) if s * s > chunk and (s * s) % chunk != 0)
    return 13, even


def means_input(S_, chunk, N=2, T_=3, seed=0):
    """Small non-negative values; the first pixel of every chunk and the last three pixels of every frame are 1.0."""
    g = torch.Generator().manual_seed(seed + S_)
    x = torch.rand((N, 3, T_, S_ * S_), generator=g) * 1e-3
    x[..., 0::chunk] = 1.0
    x[..., -3:] = 1.0
    return x.view(N, 3, T_, S_, S_).contiguous()


def check_frame_means(device, which):
    S_ = kernel_sizes()[which]
    chunk = chunk_pixels()
    lib = _sflib.get_lib()
    depth = lib.call("sf_color_sum_depth")
    bound = (depth + 6) * 2.0 ** -24
    assert bound < 0.1 / (S_ * S_), "the bound must be too tight for a dropped pixel"
    assert lib.call("sf_color_chunks", S_ * S_) == (1 if which == 0 else 2) and (which == 0 or (S_ * S_) % 4 == 0)
    N, T_ = 2, 3
    x = means_input(S_, chunk, N, T_)
    rows = [((1, 0, 2), (1.3, 0.8, 1.2), (0.0, 0.0, 0.0)), ((2, 0), (0.7, 1.25), (0.01, 0.0, -0.01))]
    table = ca.make_table(rows)
    xd = x.to(device)
    means = torch.full((N * T_,), -7.0).to(device)
    out = ca.frame_means(xd, table, means)
    assert out.data_ptr() == means.data_ptr()
    got = means.cpu()
    again = torch.full((N * T_,), -7.0).to(device)
    ca.frame_means(xd, table, again)
    assert torch.equal(bits(again.cpu()), bits(got)), "two calls must give the same bits"
    assert torch.equal(xd.cpu(), x), "the reduction must not write the clip"
    assert got[T_:].tolist() == [-7.0] * T_, "means of a sample without contrast must be left untouched"
    v = x.double()
    want = ((W_R * v[0, 2] + W_G * v[0, 1]) + W_B * v[0, 0]).mean(dim=(1, 2))
    rel = ((got[:T_].double() - want) / want).abs().max()
    print("S %d: frame means, largest relative deviation %.3e (bound %.3e, a dropped pixel %.3e)" % (
        S_, float(rel), bound, 1.0 / float(want.max() * S_ * S_)))
    assert float(rel) <= bound, (S_, float(rel), bound)
    # behind another op the mean is taken over the values as they stand there
    rows2 = [((0, 2, 1), (1.3, 0.8, 1.2), (0.0, 0.0, 0.0)), rows[1]]
    got2 = ca.frame_means(xd, ca.make_table(rows2), torch.full((N * T_,), -7.0).to(device)).cpu()
    _, want2 = restate(x, rows2, (0, 0, 0), (1, 1, 1), False)
    # brightness rounds every value once, the saturation blend eight more times (gray 5, two products, one sum); all terms
    # are positive, so the relative error of a term grows by less than 12 roundings
    assert float(((got2[:T_].double() - want2[0]) / want2[0]).abs().max()) <= bound + 12 * 2.0 ** -24, "mean behind two ops"
    assert got2[T_:].tolist() == [-7.0] * T_
    assert ca.frame_means(xd, ca.make_table([rows[1], rows[1]])) is None, "no contrast: nothing to reduce"


# ---- 3. per-element fp64 parity ---------------------------------------------------------------------------------------
def check_parity(device, which, order, reverse):
    S_ = kernel_sizes()[which]
    N, T_ = 3, 2
    g = torch.Generator().manual_seed(17 * S_ + sum(o * 3 ** i for i, o in enumerate(order)))
    x = torch.rand((N, 3, T_, S_, S_), generator=g)
    x[:, :, 1] *= 0.5                                       # frames of different means
    o = list(order)
    rows = [(o, (1.31, 0.72, 1.18), (0.031, -0.012, 0.044)),
            (o[::-1], (0.64, 1.27, 0.85), (-0.05, 0.02, 0.0)),
            ((o[0], -1, o[2]), (1.12, 1.0, 0.69), (0.0, 0.0, 0.0))]
    want, _ = restate(x, rows, MEAN, STD, reverse)
    got = sa.color_clip(x.clone().to(device), ca.make_table(rows), MEAN, STD, reverse).cpu()
    dev = float((got.double() - want).abs().max())
    print("S %d order %s reverse %s: max |kernel - fp64| = %.3e (bound %.3e)" % (S_, order, reverse, dev, VALUE_BOUND))
    assert dev <= VALUE_BOUND, (S_, order, reverse, dev, VALUE_BOUND)


# ---- 4. composition ---------------------------------------------------------------------------------------------------
def check_composition(device):
    """The whole-pipeline cases as ONE padded batch of two frame sizes: sample_clip(mean 0, std 1) -> color_clip."""
    cases = [CASES[i] for i in PIPELINE_CASES]
    assert len({tuple(c["size"]) for c in cases}) >= 2
    draws = [pipeline_draw(c) for c in cases]
    crop = ss.make_table([d[0].rows[0] for d in draws], S)
    ctab = sa.ColorTable(np.concatenate([d[1].words for d in draws]))
    frames = padded([case_frames(c["data_seed"], [tuple(c["size"])])[0] for c in cases]).to(device)
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append((name, work)) or thunk())
    try:
        clip = sa.sample_clip(frames, crop, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        got = sa.color_clip(clip, ctab, MEAN, STD, reverse=True).cpu()
    finally:
        _sflib.set_call_observer(None)
    assert [c[0] for c in calls] == ["sf_sample_clip_u8", "sf_color_chunks", "sf_color_frame_means_f32", "sf_color_clip_f32"], calls
    assert all(w and w.get("bytes", 0) > 0 for n, w in calls if n in ("sf_color_frame_means_f32", "sf_color_clip_f32"))
    for n, c in enumerate(cases):
        dev = float((got[n].double() - case_want(c)[0].double()).abs().max())
        assert dev <= VALUE_BOUND, (c["name"], dev)
    boxes = sa.collate_boxes([sa.transform_boxes(crop.rows[n], c["boxes_in"], S) for n, c in enumerate(cases)])
    assert tuple(boxes.shape) == (sum(len(c["boxes"]) for c in cases), 5) and boxes.dtype == torch.float32
    assert boxes[:, 0].tolist() == [float(n) for n, c in enumerate(cases) for _ in c["boxes"]]


def check_pca_only_is_one_launch(device):
    """A table without contrast issues no reduction launch and reads no mean."""
    x = unit_clip(case_frames(11, [(S, S)] * 2))
    rows = [((), (), (0.03, -0.01, 0.02)), ((2, 0), (1.2, 0.8), (0.0, 0.01, -0.02))]
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        got = sa.color_clip(x.clone().to(device), ca.make_table(rows), MEAN, STD).cpu()
    finally:
        _sflib.set_call_observer(None)
    assert calls == ["sf_color_clip_f32"], calls
    want, _ = restate(x, rows, MEAN, STD, True)
    assert float((got.double() - want).abs().max()) <= VALUE_BOUND


# ---- 5. rejections ----------------------------------------------------------------------------------------------------
GOOD_ROW = ((0, 1, 2), (1.2, 0.8, 1.1), (0.01, -0.02, 0.03))


def _bad_words(edit):
    t = ca.make_table([GOOD_ROW, GOOD_ROW])
    edit(t.words, t.words.view(np.float32))
    return t


BAD_TABLES = {
    "op out of range": _bad_words(lambda w, f: w.__setitem__((1, 0), 3)),
    "op below -1": _bad_words(lambda w, f: w.__setitem__((1, 2), -2)),
    "op twice": _bad_words(lambda w, f: w.__setitem__((1, 2), 0)),
    "alpha not finite": _bad_words(lambda w, f: f.__setitem__((1, 6), float("inf"))),
    "one minus alpha not finite": _bad_words(lambda w, f: f.__setitem__((1, 5), float("nan"))),
    "addition not finite": _bad_words(lambda w, f: f.__setitem__((1, 12), float("-inf"))),
}


def check_rejects(device):
    import pytest
    x = unit_clip(case_frames(3, [(S, S)] * 2))
    xd = x.to(device)
    fn = _augmentation(dict(brightness=0.4, contrast=0.4, saturation=0.4, alphastd=0.1))
    good = ca.make_table([GOOD_ROW, GOOD_ROW])
    np.random.seed(5)
    random.seed(5)
    state = generator_state()
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        # the clip: dtype, rank, channel count, contiguity -- before any draw
        for bad in (xd.double(), xd.half(), xd[0], xd[:, :2], torch.cat([xd, xd[:, :1]], 1), xd[..., ::2], xd.transpose(3, 4)):
            with pytest.raises(sa.lib.SfError):
                fn(bad)
            with pytest.raises(sa.lib.SfError):
                fn(bad, good)
            with pytest.raises(sa.lib.SfError):
                sa.color_clip(bad, good, MEAN, STD)
            assert generator_state() == state, "a rejected call must not consume random numbers"
        # a table drawn for another N
        for n in (1, 3):
            other = ca.make_table([GOOD_ROW] * n)
            with pytest.raises(sa.lib.SfError, match="drawn for %d samples" % n):
                fn(xd, other)
            with pytest.raises(sa.lib.SfError, match="drawn for %d samples" % n):
                sa.color_clip(xd, other, MEAN, STD)
            with pytest.raises(sa.lib.SfError, match="drawn for %d samples" % n):
                ca.frame_means(xd, other)
        # the rows of the host copy
        for what, bad in BAD_TABLES.items():
            with pytest.raises(sa.lib.SfError, match="colour row 1"):
                sa.color_clip(xd, bad, MEAN, STD)
            with pytest.raises(sa.lib.SfError, match="colour row 1"):
                fn(xd, bad)
        with pytest.raises(sa.lib.SfError):
            sa.color_clip(xd, sa.ColorTable(good.words[:, :12]), MEAN, STD)
        with pytest.raises(sa.lib.SfError):
            sa.color_clip(xd, good, MEAN[:2], STD)
        assert calls == [], "a rejected call never reaches the library"
        # the library's own checks (the Python side's are bypassed)
        stream = sa.ops._stream(xd)
        lib = _sflib.get_lib()
        host, dev = ca.upload_table(good, 2, xd.device)
        with pytest.raises(sa.lib.SfError, match="zero std"):
            sa.color_clip(xd, good, MEAN, [0.2, 0.0, 0.2])
        part, means = torch.zeros(64).to(device), torch.zeros(2 * T).to(device)
        for what, bad in BAD_TABLES.items():
            words = np.ascontiguousarray(bad.words.reshape(-1))
            with pytest.raises(sa.lib.SfError, match="colour row 1"):
                lib.call("sf_color_clip_f32", xd.data_ptr(), 2, T, S * S, words.ctypes.data, dev.data_ptr(), means.data_ptr(),
                         0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1, stream)
            with pytest.raises(sa.lib.SfError, match="colour row 1"):
                lib.call("sf_color_frame_means_f32", xd.data_ptr(), 2, T, S * S, words.ctypes.data, dev.data_ptr(),
                         part.data_ptr(), means.data_ptr(), stream)
        with pytest.raises(sa.lib.SfError, match="needs the frame means"):
            lib.call("sf_color_clip_f32", xd.data_ptr(), 2, T, S * S, host.ctypes.data, dev.data_ptr(), None, 0.0, 0.0, 0.0, 1.0,
                     1.0, 1.0, 1, stream)
        with pytest.raises(sa.lib.SfError, match="pixels"):
            lib.call("sf_color_chunks", (1 << 18) + 1)
    finally:
        _sflib.set_call_observer(None)
    assert torch.equal(bits(xd.cpu()), bits(x)), "a rejected call wrote the clip"
    assert generator_state() == state


def check_host_tensor_rejected():
    """With the gfx950 library a host tensor raises (there is no torch fallback) and consumes no random number."""
    import pytest
    x = unit_clip(case_frames(3, [(S, S)] * 2))
    fn = _augmentation(dict(brightness=0.4, contrast=0.4, saturation=0.4, alphastd=0.1))
    good = ca.make_table([GOOD_ROW, GOOD_ROW])
    np.random.seed(5)
    state = generator_state()
    for call in (lambda: fn(x), lambda: fn(x, good), lambda: sa.color_clip(x, good, MEAN, STD), lambda: ca.frame_means(x, good)):
        with pytest.raises(sa.lib.SfError):
            call()
    assert generator_state() == state


# ---- 6. host only -----------------------------------------------------------------------------------------------------
def check_config():
    import pytest
    cfg = sa.get_cfg()
    assert (cfg.AVA.BGR, cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION, cfg.AVA.TRAIN_PCA_JITTER_ONLY, cfg.AVA.TEST_FORCE_FLIP) == (
        False, False, True, False)
    assert cfg.DATA.TRAIN_PCA_EIGVAL == [0.225, 0.224, 0.229]
    assert cfg.DATA.TRAIN_PCA_EIGVEC == [[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]]

    def fields(f):
        return (f.brightness, f.contrast, f.saturation, f.alphastd, f.mean, f.std, f.reverse)
    plain = (0.0, 0.0, 0.0, 0.0, [0.45] * 3, [0.225] * 3, True)
    for split in ("train", "val", "test"):                  # colour off: normalise and reorder only, nothing is drawn
        fn = sa.construct_color_augmentation(cfg, split)
        assert fields(fn) == plain
        np.random.seed(1)
        state = generator_state()
        row = fn.sample_params()
        assert row == sa.ColorRow((-1, -1, -1), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)) and generator_state() == state
    cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION = True             # PCA only (the default of TRAIN_PCA_JITTER_ONLY)
    cfg.DATA.MEAN, cfg.DATA.STD = MEAN, STD
    fn = sa.construct_color_augmentation(cfg, "train")
    assert fields(fn) == (0.0, 0.0, 0.0, 0.1, MEAN, STD, True)
    assert fn.eigval.dtype == np.float32 and fn.eigvec.dtype == np.float32 and fn.eigvec.shape == (3, 3)
    np.random.seed(1)
    row = fn.sample_params()
    assert row.order == (-1, -1, -1) and any(v != 0.0 for v in row.add)
    assert fields(sa.construct_color_augmentation(cfg, "val")) == (0.0, 0.0, 0.0, 0.0, MEAN, STD, True)
    cfg.AVA.TRAIN_PCA_JITTER_ONLY = False
    cfg.AVA.BGR = True
    assert fields(sa.construct_color_augmentation(cfg, "train")) == (0.4, 0.4, 0.4, 0.1, MEAN, STD, False)
    assert fields(sa.construct_color_augmentation(cfg, "val")) == (0.0, 0.0, 0.0, 0.0, MEAN, STD, False)

    def crop_fields(f):
        return (f.spatial_idx, f.min_scale, f.max_scale, f.crop_size, f.random_horizontal_flip, f.force_flip, f.scale)
    cfg = sa.get_cfg()
    assert crop_fields(sa.construct_ava_sampling(cfg, "train")) == (-1, 256, 320, 224, True, False, None)
    assert crop_fields(sa.construct_ava_sampling(cfg, "val")) == (1, 256, 256, 256, False, False, None)
    cfg.AVA.TEST_FORCE_FLIP = True
    forced = sa.construct_ava_sampling(cfg, "val")
    assert crop_fields(forced) == (1, 256, 256, 256, False, True, None)
    np.random.seed(2)
    np.random.uniform(256, 256)                             # the draw of the test path
    np.random.uniform()                                     # horizontal_flip(1, ...) compares one more with 1
    after = generator_state()
    np.random.seed(2)
    assert forced.sample_params(300, 400).flip == 1 and generator_state() == after
    assert crop_fields(sa.construct_ava_sampling(cfg, "train"))[5] is False
    for split in ("test", "predict"):
        with pytest.raises(NotImplementedError):
            sa.construct_ava_sampling(cfg, split)
    assert sa.SpatialSampling().force_flip is False


def check_boxes():
    import pytest
    b = np.array([[0.10, 0.20, 0.60, 0.90], [0.0, 0.0, 1.0, 1.0], [-0.1, 0.5, 1.2, 0.6]], dtype=np.float64)
    # nothing resized: scale to the frame, clip to it, move by the offset, clip to the crop
    row = sa.CropRow(18, 26, 0, 0, 18, 26, 18, 26, 3, 7, 0)
    px = b * np.array([26.0, 18.0, 26.0, 18.0])
    px[:, [0, 2]] = px[:, [0, 2]].clip(0.0, 25.0)
    px[:, [1, 3]] = px[:, [1, 3]].clip(0.0, 17.0)
    want = (px - np.array([7.0, 3.0, 7.0, 3.0])).clip(0.0, 11.0)
    got = sa.transform_boxes(row, b, 12)
    assert got.tobytes() == want.tobytes(), (got, want)
    # flipped: x1, x2 = S - x2 - 1, S - x1 - 1 before the last clip
    moved = px - np.array([7.0, 3.0, 7.0, 3.0])
    flipped = moved.copy()
    flipped[:, 0], flipped[:, 2] = 12 - moved[:, 2] - 1, 12 - moved[:, 0] - 1
    assert sa.transform_boxes(row._replace(flip=1), b, 12).tobytes() == flipped.clip(0.0, 11.0).tobytes()
    # the forced-flip val row: landscape, short side to 12 -> 12 x 17, centre crop at x = ceil(5 / 2)
    val = sa.SpatialSampling(spatial_idx=1, min_scale=12, max_scale=12, crop_size=12, random_horizontal_flip=False,
                             force_flip=True).sample_params(18, 26)
    assert tuple(val) == (18, 26, 0, 0, 18, 26, 12, 17, 0, 3, 1)
    scaled = px * float(17) / 26
    moved = scaled - np.array([3.0, 0.0, 3.0, 0.0])
    flipped = moved.copy()
    flipped[:, 0], flipped[:, 2] = 12 - moved[:, 2] - 1, 12 - moved[:, 0] - 1
    assert sa.transform_boxes(val, b, 12).tobytes() == flipped.clip(0.0, 11.0).tobytes()
    # portrait rows scale by the height
    port = sa.CropRow(26, 18, 0, 0, 26, 18, 20, 14, 4, 1, 0)
    pp = b * np.array([18.0, 26.0, 18.0, 26.0])
    pp[:, [0, 2]] = pp[:, [0, 2]].clip(0.0, 17.0)
    pp[:, [1, 3]] = pp[:, [1, 3]].clip(0.0, 25.0)
    assert sa.transform_boxes(port, b, 12).tobytes() == ((pp * float(20) / 26) - np.array([1.0, 4.0, 1.0, 4.0])).clip(0.0, 11.0).tobytes()
    assert sa.transform_boxes(row, b.astype(np.float32), 12).dtype == np.float32
    assert sa.transform_boxes(row, np.zeros((0, 4)), 12).shape == (0, 4)
    for bad in (np.zeros((2, 5)), np.zeros(4), np.zeros((2, 4), dtype=np.int64)):
        with pytest.raises(sa.lib.SfError):
            sa.transform_boxes(row, bad, 12)
    with pytest.raises(sa.lib.SfError):                     # a resized-crop row resizes a window: the boxes have no rule for it
        sa.transform_boxes(sa.CropRow(18, 26, 2, 3, 10, 12, 12, 12, 0, 0, 0), b, 12)
    # collate: batch index in front, a sample without boxes contributes no row
    out = sa.collate_boxes([got, np.zeros((0, 4)), want[:1]])
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 5)
    assert out[:, 0].tolist() == [0.0, 0.0, 0.0, 2.0]
    assert torch.equal(out[:, 1:], torch.tensor(np.concatenate([got, want[:1]])).float())
    assert tuple(sa.collate_boxes([np.zeros((0, 4))]).shape) == (0, 5) and tuple(sa.collate_boxes([]).shape) == (0, 5)
