"""RandAugment checks shared by the CPU (host simulator) and GPU (-m gpu) test files (csrc/sf_randaug.h,
slowfast_amd/rand_augment.py).

tests/golden/rand_augment_contract.json holds what the reference itself did (tools/make_rand_augment_golden.py): per op case
the argument its level function returned and the SHA-256 of PIL's output bytes for a landscape and a portrait clip (the bytes
of 96 clips would be half a megabyte of fixture; equal digests are equal bytes); per whole-transform case the chosen ops, the
skip decisions, the arguments, how far ``np.random`` and ``random`` got, and the output bytes themselves.  Everything is
compared EXACTLY: the draw value for value, the generator positions by one more draw from each, the output byte for byte --
zero differing bytes, no tolerance (every op is integer or short fixed-order floating-point arithmetic on uint8).  Where a
digest differs, the count that is reported is taken against the restatement below, which must itself reproduce every digest.

``restate_clip`` is the numpy restatement of the rules in csrc/sf_randaug.h.  It is itself checked against the fixture on the
CPU and -- where Pillow is installed -- against PIL directly; the kernels are compared with it at shapes the fixture does not
reach.  Its ``variant`` argument switches on one deliberately wrong rule (the golden tool records how many bytes each changes:
``effect_diff``; a case whose count is not zero cannot be passed by a kernel that makes that mistake).

Neither PIL nor anything of the reference is imported here.
"""
import base64
import hashlib
import json
import os
import random

import numpy as np
import torch

import slowfast_amd as sa
from slowfast_amd import lib as _sflib
from slowfast_amd import rand_augment as ra
from slowfast_amd import spatial_sampling as ss
from tests.spatial_sampling_checks import generator_state, padded

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rand_augment_contract.json")
if os.path.exists(GOLDEN):                                  # the golden tool imports this module before the fixture exists
    with open(GOLDEN) as _f:
        CONTRACT = json.load(_f)
else:
    CONTRACT = {"cases": [], "T": 3}
CASES = CONTRACT["cases"]
NUM_GOLDEN_CASES = len(CASES)
T = CONTRACT["T"]
VARIANTS = ("cubic_half", "round", "clip_hist", "sharp_border")


# ---- the fixture's inputs ---------------------------------------------------------------------------------------------
def case_frames(data_seed, sizes, constant_channel=None):
    """The uint8 (T, h, w, 3) frames of every sample, drawn as tools/make_rand_augment_golden.py draws them: another range per
    frame and channel, so a statistic of the clip differs from one of a frame."""
    g = np.random.RandomState(data_seed)
    out = []
    for h, w in sizes:
        f = np.stack([np.stack([g.randint(20 + 45 * t + 30 * c, 100 + 45 * t + 30 * c, (h, w)) for c in range(3)], axis=-1)
                      for t in range(T)]).astype(np.uint8)
        if constant_channel is not None:
            f[..., constant_channel] = 77
        out.append(torch.from_numpy(f))
    return out


def case_want(case):
    """The reference's output per sample: uint8 (T, h, w, 3) tensors."""
    raw = np.frombuffer(base64.b64decode(case["out"]), dtype=np.uint8)
    out, at = [], 0
    for h, w in case["sizes"]:
        out.append(torch.from_numpy(raw[at:at + T * h * w * 3].reshape(T, h, w, 3).copy()))
        at += T * h * w * 3
    assert at == len(raw)
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a)).tobytes()).hexdigest()


def differing_from_reference(case, n, got, restated):
    """Bytes by which ``got`` (sample n's valid region) differs from the reference's output; ``restated``: a function that
    returns the restatement's bytes for the sample, used for the count where the fixture keeps the digest only."""
    if "out" in case:
        return differing(got, case_want(case)[n])
    if digest(got) == case["sha256"][n]:
        return 0
    return max(1, differing(got, restated()))


def case_table(case):
    return ra.make_table([[(r[0], r[1], r[2]) for r in rows] for rows in case["rows"]], case["interpolation"])


# ---- numpy restatement of csrc/sf_randaug.h ---------------------------------------------------------------------------
def luma(img):
    v = img.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def blend(d, v, f):
    """PIL's blend of the degenerate value d and the pixel v (integer arrays) with factor f: fp32, product then sum."""
    ff = np.float32(f)
    prod = (ff * (v - d).astype(np.float32)).astype(np.float32)
    t = (d.astype(np.float32) + prod).astype(np.float32)
    if 0 <= ff <= 1:
        return t.astype(np.int64)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.minimum(t, 255).astype(np.int64)))


def histograms(img):
    """(4, 256) counts of R, G, B, L over an (..., 3) uint8 array."""
    chans = [img[..., 0], img[..., 1], img[..., 2], luma(img)]
    return np.stack([np.bincount(np.asarray(c).reshape(-1).astype(np.int64), minlength=256) for c in chans])


def lookup_table(op, arg, f, hist):
    """The (3, 256) table of a table op; hist: (4, 256)."""
    i = np.arange(256, dtype=np.int64)
    lut = np.stack([i, i, i])
    if op == ra.INVERT:
        lut[:] = 255 - i
    elif op == ra.POSTERIZE:
        bits = int(arg)
        lut[:] = i if bits >= 8 else i & ~((1 << (8 - bits)) - 1)
    elif op == ra.SOLARIZE:
        lut[:] = np.where(i < int(arg), i, 255 - i)
    elif op == ra.SOLARIZE_ADD:
        lut[:] = np.where(i < 128, np.minimum(255, i + int(arg)), i)
    elif op == ra.BRIGHTNESS:
        lut[:] = blend(np.zeros(256, np.int64), i, f)
    elif op == ra.CONTRAST:
        total = int((i * hist[3]).sum())
        m = int(total / int(hist[3].sum()) + 0.5)
        lut[:] = blend(np.full(256, m, np.int64), i, f)
    elif op == ra.AUTO_CONTRAST:
        for c in range(3):
            nz = np.nonzero(hist[c])[0]
            lo, hi = int(nz[0]), int(nz[-1])
            if hi > lo:
                scale = 255.0 / (hi - lo)
                off = -lo * scale
                lut[c] = np.clip((i.astype(np.float64) * scale + off).astype(np.int64), 0, 255)
    elif op == ra.EQUALIZE:
        for c in range(3):
            nz = hist[c][hist[c] != 0]
            if len(nz) <= 1:
                continue
            step = (int(hist[c].sum()) - int(nz[-1])) // 255
            if step == 0:
                continue
            below = np.concatenate([[0], np.cumsum(hist[c])[:-1]])
            lut[c] = np.minimum((step // 2 + below) // step, 255)
    else:
        raise AssertionError(op)
    return lut


def sharpness(img, f, border=1):
    v = img.astype(np.int64)
    h, w = v.shape[:2]
    s = v.copy()
    if h > 2 * border and w > 2 * border and h >= 3 and w >= 3:
        acc = 4 * v[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                acc = acc + v[dy:h - 2 + dy, dx:w - 2 + dx]
        inner = (2 * acc + 13) // 26
        b = border - 1
        s[border:h - border, border:w - border] = inner[b:inner.shape[0] - b, b:inner.shape[1] - b]
    return blend(s, v, f)


def _cubic(v1, v2, v3, v4, d, half):
    if half:                                                # the WRONG kernel (a = -0.5, what PIL's resize uses)
        p1, p2 = v2, 0.5 * (-v1 + v3)
        p3 = v1 - 2.5 * v2 + 2.0 * v3 - 0.5 * v4
        p4 = 0.5 * (-v1 + 3.0 * v2 - 3.0 * v3 + v4)
    else:
        p1, p2 = v2, -v1 + v3
        p3 = 2 * (v1 - v2) + v3 - v4
        p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, m, filt, variant=None):
    h, w = img.shape[:2]
    v = img.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64) + 0.5, np.arange(w, dtype=np.float64) + 0.5, indexing="ij")
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    inside = ~((xin < 0) | (yin < 0) | (xin >= w) | (yin >= h))
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)

    def tap(ox, oy):
        return v[np.clip(iy + oy, 0, h - 1), np.clip(ix + ox, 0, w - 1)]
    if filt == 0:
        r0 = tap(0, 0) + (tap(1, 0) - tap(0, 0)) * dx
        r1 = tap(0, 1) + (tap(1, 1) - tap(0, 1)) * dx
        val = r0 + (r1 - r0) * dy
        res = np.round(val).astype(np.int64) if variant == "round" else val.astype(np.int64)
    else:
        half = variant == "cubic_half"
        rows = [_cubic(tap(-1, k), tap(0, k), tap(1, k), tap(2, k), dx, half) for k in (-1, 0, 1, 2)]
        val = _cubic(rows[0], rows[1], rows[2], rows[3], dy, half)
        body = np.round(val) if variant == "round" else val
        res = np.where(val <= 0, 0, np.where(val >= 255, 255, np.clip(body, 0, 255).astype(np.int64)))
    return np.where(inside[..., None], res, 128)


def restate_clip(frames, rows, filt, variant=None):
    """``rows`` ((op, skip, arg) per layer) on the uint8 (T, h, w, 3) numpy frames of ONE clip: the uint8 result."""
    cur = np.asarray(frames).copy()
    h, w = cur.shape[1:3]
    for op, skip, arg in rows:
        op = int(op)
        if skip:
            continue
        f = float(np.float32(arg))
        nxt = np.empty_like(cur)
        for t in range(cur.shape[0]):
            img = cur[t]
            if op in ra.LUT_OPS:
                hist = histograms(cur if variant == "clip_hist" else img) if op in ra.HIST_OPS else None
                lut = lookup_table(op, arg, f, hist)
                out = np.stack([lut[c][img[..., c]] for c in range(3)], axis=-1)
            elif op == ra.COLOR:
                out = blend(np.repeat(luma(img)[..., None], 3, axis=-1), img.astype(np.int64), f)
            elif op == ra.SHARPNESS:
                out = sharpness(img, f, border=2 if variant == "sharp_border" else 1)
            else:
                m = ra.affine_matrix(op, arg, w, h)
                out = img if m is None else affine(img, m, filt, variant)
            nxt[t] = out.astype(np.uint8)
        cur = nxt
    return cur


def restate_batch(frames, table, variant=None):
    """One restated uint8 (T, h, w, 3) tensor per sample (``frames``: a list of such tensors)."""
    return [torch.from_numpy(restate_clip(f.numpy(), list(zip(table.ops[n], table.skip[n], table.args[n])), table.filter, variant))
            for n, f in enumerate(frames)]


def differing(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


# ---- 1. the reference's own results -----------------------------------------------------------------------------------
def check_restatement_golden(index):
    """CPU only: the numpy restatement reproduces the reference's bytes."""
    case = CASES[index]
    frames = case_frames(case["data_seed"], case["sizes"], case.get("constant_channel"))
    got = restate_batch(frames, case_table(case))
    for n, g in enumerate(got):
        if "out" in case:
            assert differing(g, case_want(case)[n]) == 0, (case["name"], n)
        else:
            assert digest(g) == case["sha256"][n], (case["name"], n)


def check_draw(index):
    """A whole-transform case: the draw equals the reference's and leaves both generators where it left them."""
    case = CASES[index]
    N = len(case["sizes"])
    fn = sa.RandAugment(case["config"], case["interpolation"])
    for how in ("batch", "clips"):
        np.random.seed(case["seed"])
        random.seed(case["seed"])
        if how == "batch":
            table = fn.sample_batch(N)
        else:
            rows = [fn.sample_params() for _ in range(N)]
            assert all(isinstance(r, sa.AugRow) for clip in rows for r in clip)
            table = ra.make_table(rows, case["interpolation"])
        np_after, py_after = float(np.random.uniform()), random.random()
        assert isinstance(table, sa.AugTable) and table.ops.shape == (N, fn.num_layers)
        got = [[[int(o), bool(s), float(a)] for o, s, a in zip(table.ops[n], table.skip[n], table.args[n])] for n in range(N)]
        assert got == [[[r[0], bool(r[1]), float(r[2])] for r in rows] for rows in case["rows"]], (
            "the draw differs from the reference's", got, case["rows"])
        assert repr(np_after) == case["np_after"], "np.random was not consumed as the reference consumes it"
        assert repr(py_after) == case["py_after"], "random was not consumed as the reference consumes it"
    return table


def golden_differing(device, index):
    """Bytes by which the device output differs from the reference's, summed over the case's samples."""
    case = CASES[index]
    table = check_draw(index) if case["kind"] == "transform" else case_table(case)
    frames = case_frames(case["data_seed"], case["sizes"], case.get("constant_channel"))
    buf = padded(frames, fill=201)
    keep = buf.clone()
    dev = buf.to(device)
    got = sa.rand_augment_clip(dev, table, case["sizes"]).cpu()
    assert torch.equal(dev.cpu(), keep), "frames must be left untouched"
    assert got.dtype == torch.uint8 and got.shape == buf.shape
    bad = 0
    for n, (h, w) in enumerate(case["sizes"]):
        bad += differing_from_reference(case, n, got[n, :, :h, :w], lambda: restate_batch(frames, table)[n])
        mask = torch.ones(buf.shape[2:4], dtype=torch.bool)
        mask[:h, :w] = False
        assert torch.equal(got[n][:, mask], keep[n][:, mask]), "the padding must come out as it went in"
    if case["kind"] == "transform":                         # the object draws for itself when no table is given
        np.random.seed(case["seed"])
        random.seed(case["seed"])
        own = sa.RandAugment(case["config"], case["interpolation"])(dev, sizes=case["sizes"]).cpu()
        assert torch.equal(own, got) and repr(float(np.random.uniform())) == case["np_after"]
    return bad


def check_golden_case(device, index):
    bad = golden_differing(device, index)
    case = CASES[index]
    print("case %d (%s): %d of %d bytes differ from the reference's" % (
        index, case["name"], bad, sum(T * h * w * 3 for h, w in case["sizes"])))
    assert bad == 0, (index, case["name"], bad)


def check_fixture_covers():
    """The fixture itself: every op applied, an op skipped, and every wrong variant visible somewhere."""
    applied = {int(r[0]) for c in CASES if c["kind"] == "transform" for rows in c["rows"] for r in rows if not r[1]}
    assert applied == set(range(ra.NUM_OPS)), applied
    assert any(r[1] for c in CASES if c["kind"] == "transform" for rows in c["rows"] for r in rows)
    assert {int(c["rows"][0][0][0]) for c in CASES if c["kind"] == "op"} == set(range(ra.NUM_OPS))
    for v in VARIANTS + ("input",):
        assert any(c["effect_diff"].get(v, 0) > 0 for c in CASES), v


# ---- 2. padded buffers ------------------------------------------------------------------------------------------------
CLASS_ROWS = {                                              # one table per op class: three samples, two layers
    "table": [[(ra.EQUALIZE, False, 0.0), (ra.SOLARIZE_ADD, False, 40)], [(ra.CONTRAST, False, 1.6), (ra.POSTERIZE, False, 3)],
              [(ra.AUTO_CONTRAST, False, 0.0), (ra.BRIGHTNESS, False, 0.55)]],
    "color": [[(ra.COLOR, False, 1.7), (ra.COLOR, False, 0.3)], [(ra.COLOR, False, 0.45), (ra.INVERT, False, 0.0)],
              [(ra.SOLARIZE, False, 140), (ra.COLOR, False, 1.25)]],
    "sharpness": [[(ra.SHARPNESS, False, 1.8), (ra.SHARPNESS, True, 0.0)], [(ra.SHARPNESS, False, 0.2), (ra.COLOR, False, 1.4)],
                  [(ra.EQUALIZE, True, 0.0), (ra.SHARPNESS, False, 1.3)]],
    "affine": [[(ra.ROTATE, False, -21.5), (ra.SHEAR_X, False, 0.23)], [(ra.TRANSLATE_X_REL, False, -0.31), (ra.SHEAR_Y, False, -0.17)],
               [(ra.TRANSLATE_Y_REL, False, 0.4), (ra.ROTATE, False, 13.25)]],
    "mixed": [[(ra.ROTATE, False, 29.0), (ra.CONTRAST, False, 0.4)], [(ra.INVERT, True, 0.0), (ra.EQUALIZE, False, 0.0)],
              [(ra.SHARPNESS, False, 1.9), (ra.TRANSLATE_X_REL, False, 0.2)]],
}
# the filter is read by the affine ops only: the other classes run with one
CLASS_FILTERS = [(cls, f) for cls in sorted(CLASS_ROWS) for f in (("bicubic", "bilinear") if cls in ("affine", "mixed") else ("bicubic",))]


def check_padded(device, cls, interpolation="bicubic"):
    """Samples of 18 x 26, 26 x 18 and 26 x 26 in one 26 x 26 buffer whose padding holds a pattern: the valid regions equal the
    per-sample results, the padding comes out as it went in, the input is unchanged."""
    sizes = [(18, 26), (26, 18), (26, 26)]
    frames = case_frames(41, sizes)
    table = ra.make_table(CLASS_ROWS[cls], interpolation)
    buf = padded(frames, fill=0)
    g = torch.Generator().manual_seed(5)
    pattern = torch.randint(0, 256, buf.shape, generator=g, dtype=torch.int64).to(torch.uint8)
    for n, (h, w) in enumerate(sizes):
        pattern[n, :, :h, :w] = frames[n]
    dev = pattern.to(device)
    got = sa.rand_augment_clip(dev, table, sizes).cpu()
    assert torch.equal(dev.cpu(), pattern), "frames must be unchanged"
    want = restate_batch(frames, table)
    for n, (h, w) in enumerate(sizes):
        assert differing(got[n, :, :h, :w], want[n]) == 0, (cls, n, differing(got[n, :, :h, :w], want[n]))
        alone = sa.rand_augment_clip(frames[n][None].contiguous().to(device), ra.make_table([CLASS_ROWS[cls][n]], interpolation)).cpu()
        assert torch.equal(alone[0], got[n, :, :h, :w]), "a sample in a padded buffer must equal the sample alone"
        mask = torch.ones(buf.shape[2:4], dtype=torch.bool)
        mask[:h, :w] = False
        assert torch.equal(got[n][:, mask], pattern[n][:, mask]), "the padding must come out as it went in"


# ---- 3. restatement parity at shapes the fixture does not reach -------------------------------------------------------
def parity_shapes():
    """(Hs, Ws): more than one chunk per frame with odd Ws -- once with a slab that is no multiple of 16 pixels (thread-per-pixel
    accesses) and once with one that is (16-byte accesses)."""
    chunk = _sflib.get_lib().call("sf_randaug_chunk")
    assert chunk == 4096, "choose the shapes again for another chunk size"
    return [(71, 67), (80, 67)]


def check_parity(device, which, cls, interpolation):
    Hs, Ws = parity_shapes()[which]
    chunk = _sflib.get_lib().call("sf_randaug_chunk")
    assert Hs * Ws > chunk and Ws % 2 == 1 and ((Hs * Ws) % 16 == 0) == (which == 1)
    g = np.random.RandomState(100 * which + len(cls))
    N, T_ = 2, 2
    sizes = [(Hs, Ws), (Hs - 9, Ws - 4)]                    # the second sample: its valid region ends inside the second chunk
    assert (Hs - 9) * Ws > chunk
    frames = [torch.from_numpy(np.stack([g.randint(10 + 60 * t, 150 + 50 * t, (h, w, 3)) for t in range(T_)]).astype(np.uint8))
              for h, w in sizes]
    table = ra.make_table(CLASS_ROWS[cls][:N], interpolation)
    buf = padded(frames, fill=201)
    got = sa.rand_augment_clip(buf.to(device), table, sizes).cpu()
    want = restate_batch(frames, table)
    bad = [differing(got[n, :, :h, :w], want[n]) for n, (h, w) in enumerate(sizes)]
    print("%d x %d, %s, %s: differing bytes per sample %s" % (Hs, Ws, cls, interpolation, bad))
    assert bad == [0, 0], (Hs, Ws, cls, interpolation, bad)
    assert torch.equal(got[1, :, sizes[1][0]:], buf[1, :, sizes[1][0]:]) and torch.equal(got[1, :, :, sizes[1][1]:], buf[1, :, :, sizes[1][1]:])


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
def check_determinism(device):
    Hs, Ws = parity_shapes()[1]
    g = np.random.RandomState(3)
    frames = torch.from_numpy(g.randint(0, 256, (2, 2, Hs, Ws, 3)).astype(np.uint8)).to(device)
    table = ra.make_table(CLASS_ROWS["table"][:2])
    a = sa.rand_augment_clip(frames, table).cpu()
    out = torch.empty_like(frames)
    b = sa.rand_augment_clip(frames, table, out=out)
    assert b.data_ptr() == out.data_ptr()
    assert torch.equal(a, b.cpu()), "two calls must give the same bytes"


# ---- 5. launch counts -------------------------------------------------------------------------------------------------
def _logged(device, rows, interpolation="bicubic"):
    frames = padded(case_frames(7, [(18, 26)] * len(rows))).to(device)
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        got = sa.rand_augment_clip(frames, ra.make_table(rows, interpolation)).cpu()
    finally:
        _sflib.set_call_observer(None)
    want = restate_batch(list(frames.cpu()), ra.make_table(rows, interpolation))
    assert all(differing(got[n], want[n]) == 0 for n in range(len(rows)))
    return calls, got, frames.cpu()


def check_launch_counts(device):
    """At most one histogram pass and one streaming pass per layer; a layer without a histogram op launches no histogram pass."""
    # no histogram op at all
    calls, _, _ = _logged(device, [[(ra.INVERT, False, 0.0), (ra.ROTATE, False, 10.0)], [(ra.COLOR, False, 1.3), (ra.SHARPNESS, False, 0.5)]])
    assert calls == ["sf_randaug_layer_u8"] * 2, calls
    # the only histogram ops are skipped; layer 0 is skipped as a whole: it copies
    calls, got, src = _logged(device, [[(ra.EQUALIZE, True, 0.0), (ra.CONTRAST, True, 0.0)], [(ra.AUTO_CONTRAST, True, 0.0), (ra.INVERT, True, 0.0)]])
    assert calls == ["sf_randaug_layer_u8"] * 2, calls
    assert torch.equal(got, src), "a table of skipped rows copies"
    # one histogram op in layer 1 of one sample: one histogram pass
    calls, _, _ = _logged(device, [[(ra.INVERT, False, 0.0), (ra.EQUALIZE, False, 0.0)], [(ra.COLOR, False, 1.3), (ra.SHARPNESS, True, 0.0)]])
    assert calls == ["sf_randaug_layer_u8", "sf_randaug_hist_u8", "sf_randaug_layer_u8"], calls
    # Rotate by 0 degrees is PIL's copy
    calls, got, src = _logged(device, [[(ra.ROTATE, False, 0.0)]])
    assert calls == ["sf_randaug_layer_u8"] and torch.equal(got, src)


# ---- 6. composition ---------------------------------------------------------------------------------------------------
def check_composition(device):
    """sample_clip takes the result as it is."""
    sizes = [(18, 26), (26, 18)]
    frames = case_frames(23, sizes)
    table = ra.make_table(CLASS_ROWS["mixed"][:2])
    crop = ss.make_table([(18, 26, 0, 0, 18, 26, 15, 21, 1, 2, 0), (26, 18, 0, 0, 26, 18, 20, 14, 4, 1, 1)], 12)
    mean, std = (0.45, 0.40, 0.35), (0.225, 0.25, 0.2)
    got = sa.sample_clip(sa.rand_augment_clip(padded(frames).to(device), table, sizes), crop, mean, std).cpu()
    want = sa.sample_clip(padded(restate_batch(frames, table)).to(device), crop, mean, std).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- 7. rejections ----------------------------------------------------------------------------------------------------
GOOD = [[(ra.COLOR, False, 1.3), (ra.POSTERIZE, False, 3)]] * 2


def check_rejects(device):
    import pytest
    frames = padded(case_frames(3, [(18, 26)] * 2))
    fd = frames.to(device)
    good = ra.make_table(GOOD)
    fn = sa.RandAugment("rand-m7-n2-mstd0.5-inc1")
    np.random.seed(5)
    random.seed(5)
    state = generator_state()
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        for bad in (fd.float(), fd.to(torch.int8), fd[0], fd[..., :2], fd[:, :, :, ::2], fd.transpose(2, 3)):
            for call in (lambda: fn(bad), lambda: fn(bad, good), lambda: sa.rand_augment_clip(bad, good)):
                with pytest.raises(sa.lib.SfError):
                    call()
            assert generator_state() == state, "a rejected call must not consume random numbers"
        for n in (1, 3):                                    # a table drawn for another N
            with pytest.raises(sa.lib.SfError, match="drawn for %d samples" % n):
                sa.rand_augment_clip(fd, ra.make_table(GOOD[:1] * n))
        for sizes in ([(19, 26), (18, 26)], [(18, 26), (18, 27)], [(0, 26), (18, 26)], [(18, 26)]):
            with pytest.raises(sa.lib.SfError):
                sa.rand_augment_clip(fd, good, sizes)
            with pytest.raises(sa.lib.SfError):
                fn(fd, None, sizes)
            assert generator_state() == state
        for rows, what in (([[(15, False, 0.0)]] * 2, "unknown op code 15"), ([[(-1, False, 0.0)]] * 2, "unknown op code -1"),
                           ([[(ra.POSTERIZE, False, 9)]] * 2, "Posterize keeps 0 .. 8 bits"),
                           ([[(ra.POSTERIZE, False, -1)]] * 2, "Posterize keeps 0 .. 8 bits"),
                           ([[(ra.SOLARIZE, False, 257)]] * 2, "threshold"), ([[(ra.COLOR, False, float("nan"))]] * 2, "finite"),
                           ([[(ra.ROTATE, False, 90.0)]] * 2, "transpose shortcut")):
            with pytest.raises(sa.lib.SfError, match=what):
                sa.rand_augment_clip(fd, ra.make_table(rows))
        with pytest.raises(sa.lib.SfError):
            sa.rand_augment_clip(fd, (good.ops, good.skip, good.args, good.filter))
        with pytest.raises(sa.lib.SfError):
            sa.rand_augment_clip(fd, good, out=fd)
        with pytest.raises(sa.lib.SfError):
            sa.rand_augment_clip(fd, good, out=torch.empty_like(fd)[:, :, :, :20])
        assert calls == [], "a rejected call never reaches the library"
        # the library's own checks (the Python side's are bypassed)
        lib = _sflib.get_lib()
        stream = sa.ops._stream(fd)
        host = ra.pack_words(good, [(18, 26)] * 2).reshape(2, 2, ra.ROW_WORDS)
        dev = torch.from_numpy(host.reshape(-1).copy()).to(device)
        out, hist, lut = torch.empty_like(fd), torch.zeros(2 * T * 1024, dtype=torch.int32).to(device), torch.zeros(2 * T * 768, dtype=torch.uint8).to(device)

        def layer(words, h=hist, l=lut, dst=out):
            words = np.ascontiguousarray(words.reshape(-1))
            lib.call("sf_randaug_layer_u8", fd.data_ptr(), dst.data_ptr(), 2, T, 18, 26, words.ctypes.data, dev.data_ptr(),
                     None if h is None else h.data_ptr(), None if l is None else l.data_ptr(), stream)

        def edited(layer_index, word, value):
            w = host[layer_index].copy()
            w[1, word] = value
            return w
        for words, what in ((edited(0, 1, 15), "unknown op code"), (edited(0, 0, 5), "unknown class"), (edited(0, 0, 1), "not of class"),
                            (edited(1, 2, 9), "Posterize keeps"), (edited(0, 5, 19), "not inside"), (edited(0, 6, 0), "not inside"),
                            (edited(0, 3, 0x7f800000), "finite")):
            with pytest.raises(sa.lib.SfError, match=what):
                layer(words)
            with pytest.raises(sa.lib.SfError, match=what):
                lib.call("sf_randaug_hist_u8", fd.data_ptr(), 2, T, 18, 26, np.ascontiguousarray(words.reshape(-1)).ctypes.data,
                         dev.data_ptr(), hist.data_ptr(), stream)
        eq = ra.pack_words(ra.make_table([[(ra.EQUALIZE, False, 0.0)]] * 2), [(18, 26)] * 2)
        with pytest.raises(sa.lib.SfError, match="needs the histograms"):
            layer(eq, h=None)
        with pytest.raises(sa.lib.SfError, match="needs the table scratch"):
            layer(eq, l=None)
        with pytest.raises(sa.lib.SfError, match="another buffer"):
            layer(host[0], dst=fd)
        rot = ra.pack_words(ra.make_table([[(ra.ROTATE, False, 12.0)]] * 2), [(18, 26)] * 2).reshape(2, ra.ROW_WORDS)
        rot[1, 13] = 0x7ff00000
        with pytest.raises(sa.lib.SfError, match="matrix entry 2 is not finite"):
            layer(rot)
        rot[1, 13], rot[1, 4] = 0, 2
        with pytest.raises(sa.lib.SfError, match="filter"):
            layer(rot)
    finally:
        _sflib.set_call_observer(None)
    assert torch.equal(fd.cpu(), frames), "a rejected call wrote the frames"
    assert generator_state() == state


def check_host_tensor_rejected():
    """With the gfx950 library a host tensor raises (there is no torch fallback) and consumes no random number."""
    import pytest
    frames = padded(case_frames(3, [(18, 26)] * 2))
    fn = sa.RandAugment()
    good = ra.make_table(GOOD)
    np.random.seed(5)
    random.seed(5)
    state = generator_state()
    for call in (lambda: fn(frames), lambda: fn(frames, good), lambda: sa.rand_augment_clip(frames, good)):
        with pytest.raises(sa.lib.SfError):
            call()
    assert generator_state() == state


# ---- 8. host only -----------------------------------------------------------------------------------------------------
def check_config():
    import pytest
    cfg = sa.get_cfg()
    assert cfg.AUG.ENABLE is False and (ra.AA_TYPE_DEFAULT, ra.INTERPOLATION_DEFAULT) == ("rand-m9-mstd0.5-inc1", "bicubic")
    for mode in ("train", "val", "test"):
        assert sa.construct_rand_augment(cfg, mode) is None     # AUG.ENABLE is off
    cfg.AUG.ENABLE = True
    assert sa.construct_rand_augment(cfg, "val") is None and sa.construct_rand_augment(cfg, "test") is None
    fn = sa.construct_rand_augment(cfg, "train")

    def fields(f):
        return (f.magnitude, f.num_layers, f.magnitude_std, f.increasing, f.choice_weights is not None, f.filter)
    assert isinstance(fn, sa.RandAugment) and fields(fn) == (9, 2, 0.5, True, False, 1)     # the reference's defaults
    cfg.merge_from_dict({"AUG": {"AA_TYPE": "rand-m5-n3-mstd0.25", "INTERPOLATION": "bilinear"}})       # a merged recipe
    assert fields(sa.construct_rand_augment(cfg, "train")) == (5, 3, 0.25, False, False, 0)
    cfg.AUG.AA_TYPE = ""
    assert sa.construct_rand_augment(cfg, "train") is None
    cfg.AUG.AA_TYPE, cfg.AUG.INTERPOLATION = "rand-m7-n4-mstd0.5-inc1", "bilinear"
    assert fields(sa.construct_rand_augment(cfg, "train")) == (7, 4, 0.5, True, False, 0)
    cfg.AUG.AA_TYPE = "augmix-m5-w4-d2"
    with pytest.raises(NotImplementedError):
        sa.construct_rand_augment(cfg, "train")
    cfg.AUG.AA_TYPE, cfg.AUG.INTERPOLATION = "rand-m9-mstd0.5-inc1", "random"
    with pytest.raises(NotImplementedError, match="per frame"):
        sa.construct_rand_augment(cfg, "train")
    for name in ("lanczos", "hamming", "nearest"):
        with pytest.raises(sa.lib.SfError):
            sa.RandAugment(interpolation=name)
    # every section of the config string
    assert fields(sa.RandAugment("rand")) == (10.0, 2, 0.0, False, False, 1)
    assert fields(sa.RandAugment("rand-m3")) == (3, 2, 0.0, False, False, 1)
    assert fields(sa.RandAugment("rand-n5-mstd1")) == (10.0, 5, 1.0, False, False, 1)
    assert fields(sa.RandAugment("rand-mstd0.25-mstd2")) == (10.0, 2, 0.25, False, False, 1)    # setdefault: the first one holds
    assert sa.RandAugment("rand-inc1").increasing and sa.RandAugment("rand-inc0").increasing      # bool("0") is True
    assert not sa.RandAugment("rand-inc").increasing            # no digit: the section is not read
    assert fields(sa.RandAugment("rand-m9-n2-w0")) == (9, 2, 0.0, False, True, 1)
    with pytest.raises(sa.lib.SfError):
        sa.RandAugment("rand-w1")
    p = sa.RandAugment("rand-w0").choice_weights
    w = np.array(ra.CHOICE_WEIGHTS_0, dtype=np.float64)
    assert p.tolist() == (w / np.sum(w)).tolist() and abs(p.sum() - 1.0) < 1e-12 and p[ra.POSTERIZE] == 0 and p[ra.INVERT] == 0
    assert p[ra.ROTATE] == 0.3 / np.sum(w)
    # the level functions, at the ends of the range (mstd 0: nothing random but the sign)
    for config, op, want in (("rand-m10", ra.POSTERIZE, 4.0), ("rand-m10-inc1", ra.POSTERIZE, 0.0), ("rand-m0-inc1", ra.POSTERIZE, 4.0),
                             ("rand-m10", ra.SOLARIZE, 256.0), ("rand-m10-inc1", ra.SOLARIZE, 0.0), ("rand-m5", ra.SOLARIZE_ADD, 55.0),
                             ("rand-m5", ra.BRIGHTNESS, 1.0), ("rand-m0", ra.COLOR, 0.1), ("rand-m0-inc1", ra.SHARPNESS, 1.0)):
        assert sa.RandAugment(config)._level_arg(op, sa.RandAugment(config).magnitude) == want, (config, op)
    random.seed(0)
    signs = {sa.RandAugment("rand-m10")._level_arg(ra.ROTATE, 10.0) for _ in range(40)}
    assert signs == {30.0, -30.0}
    # a table without samples, a transform without layers
    assert sa.RandAugment("rand-n3").sample_batch(0).ops.shape == (0, 3)
    assert ra.make_table([]).ops.shape == (0, 0)
    with pytest.raises(sa.lib.SfError):
        ra.make_table([[(0, False, 0.0)], []])
    # the affine matrices are PIL's
    assert ra.affine_matrix(ra.SHEAR_X, 0.25, 26, 18) == (1.0, 0.25, 0.0, 0.0, 1.0, 0.0)
    assert ra.affine_matrix(ra.TRANSLATE_Y_REL, -0.2, 26, 18) == (1.0, 0.0, 0.0, 0.0, 1.0, -0.2 * 18)
    assert ra.affine_matrix(ra.ROTATE, 360.0, 26, 18) is None and ra.affine_matrix(ra.ROTATE, 0.0, 26, 18) is None
    m = ra.affine_matrix(ra.ROTATE, 30.0, 26, 18)
    assert m[0] == m[4] == round(np.cos(np.radians(30.0)), 15) and m[1] == -m[3]
    assert abs(m[0] * 13 + m[1] * 9 + m[2] - 13) < 1e-12 and abs(m[3] * 13 + m[4] * 9 + m[5] - 9) < 1e-12   # the centre stays


def check_restatement_against_pil():
    """Where Pillow is installed: the restatement against PIL itself, at a size the fixture does not have."""
    import pytest
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps
    g = np.random.RandomState(9)
    h, w = 37, 53
    frame = np.stack([g.randint(15 + 40 * c, 140 + 40 * c, (h, w)) for c in range(3)], axis=-1).astype(np.uint8)
    img = Image.fromarray(frame, "RGB")
    fill = (128, 128, 128)

    def pil(op, arg, resample):
        kw = dict(resample=resample, fillcolor=fill)
        if op == ra.AUTO_CONTRAST:
            return ImageOps.autocontrast(img)
        if op == ra.EQUALIZE:
            return ImageOps.equalize(img)
        if op == ra.INVERT:
            return ImageOps.invert(img)
        if op == ra.ROTATE:
            return img.rotate(arg, **kw)
        if op == ra.POSTERIZE:
            return img if arg >= 8 else ImageOps.posterize(img, int(arg))
        if op == ra.SOLARIZE:
            return ImageOps.solarize(img, int(arg))
        if op == ra.SOLARIZE_ADD:
            return img.point([min(255, i + int(arg)) if i < 128 else i for i in range(256)] * 3)
        if op in ra.ENHANCE_OPS:
            cls = {ra.COLOR: ImageEnhance.Color, ra.CONTRAST: ImageEnhance.Contrast, ra.BRIGHTNESS: ImageEnhance.Brightness,
                   ra.SHARPNESS: ImageEnhance.Sharpness}[op]
            return cls(img).enhance(arg)
        return img.transform(img.size, Image.AFFINE, ra.affine_matrix(op, arg, w, h), **kw)
    args = {ra.AUTO_CONTRAST: [0.0], ra.EQUALIZE: [0.0], ra.INVERT: [0.0], ra.ROTATE: [-27.3, 8.0, 30.0], ra.POSTERIZE: [0, 1, 4, 7, 8],
            ra.SOLARIZE: [0, 77, 256], ra.SOLARIZE_ADD: [0, 55, 110], ra.COLOR: [0.1, 0.73, 1.0, 1.9], ra.CONTRAST: [0.1, 0.73, 1.9],
            ra.BRIGHTNESS: [0.1, 0.73, 1.9], ra.SHARPNESS: [0.1, 0.73, 1.9], ra.SHEAR_X: [-0.3, 0.11], ra.SHEAR_Y: [-0.3, 0.11],
            ra.TRANSLATE_X_REL: [-0.45, 0.13], ra.TRANSLATE_Y_REL: [-0.45, 0.13]}
    for op, values in args.items():
        for arg in values:
            for name in (("bilinear", "bicubic") if op in ra.AFFINE_OPS else ("bicubic",)):
                want = np.asarray(pil(op, arg, Image.BICUBIC if name == "bicubic" else Image.BILINEAR))
                got = restate_clip(frame[None], [(op, False, arg)], ra.FILTERS[name])[0]
                assert differing(got, want) == 0, (ra.OP_NAMES[op], arg, name, differing(got, want))
