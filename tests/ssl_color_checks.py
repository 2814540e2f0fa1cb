"""SSL colour-augmentation checks shared by the CPU (host simulator) and GPU (-m gpu) test files (csrc/sf_sslcolor.h,
slowfast_amd/ssl_color.py).

tests/golden/ssl_color_contract.json holds what PIL itself did (tools/make_ssl_color_golden.py: ``ImageEnhance``, ``convert`` and
``ImageFilter`` on the (T * h) x w stack of a clip, the calls torchvision's PIL backend makes): per case the parameters, the seed,
the draw (one row per clip), how far the ``torch`` generator and ``random`` got, and PIL's output bytes.  Everything is compared
EXACTLY: the draw value for value, the generator positions by one more draw from each, the output byte for byte -- zero
differing bytes, no tolerance.  torchvision is not installed where the fixture was recorded: the DRAW in it is this package's own
restatement of torchvision's published behaviour (parity unpinned); ``restate_draw`` below is a second, independent statement
of it that the package's is held against.

``restate_clip`` is the numpy restatement of the rules in csrc/sf_sslcolor.h.  It is itself checked against the fixture on the CPU
and -- where Pillow is installed -- against PIL directly: the two HSV conversions over ALL 2^24 triples each, the blur over a sweep
of sigma in [0.1, 2.0].  The kernels are compared with it at shapes and tables the fixture does not reach.

Neither PIL (outside the two checks that are about it) nor anything of the reference is imported here.
"""
import base64
import json
import os
import random

import numpy as np
import torch

import slowfast_amd as sa
from slowfast_amd import lib as _sflib
from slowfast_amd import rand_augment as ra
from slowfast_amd import spatial_sampling as ss
from slowfast_amd import ssl_color as sc
from tests import rand_augment_checks as ra_checks
from tests.rand_augment_checks import blend, differing, luma
from tests.spatial_sampling_checks import padded

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssl_color_contract.json")
if os.path.exists(GOLDEN):                                  # the golden tool imports this module before the fixture exists
    with open(GOLDEN) as _f:
        CONTRACT = json.load(_f)
else:
    CONTRACT = {"cases": [], "T": 3}
CASES = CONTRACT["cases"]
NUM_GOLDEN_CASES = len(CASES)
T = CONTRACT["T"]
# one 24 x 40 buffer: a full sample, an odd one, one shorter than the blur's halo (the column pass crosses both frame seams
# inside one halo), one with an odd width only
SIZES = [(24, 40), (17, 23), (5, 9), (24, 37)]
HUE_SHIFTS = (0, 1, 38, 128, 255)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def case_frames(data_seed, sizes=SIZES, frames_per_clip=None):
    """uint8 (T, h, w, 3) frames per sample: another range per frame and channel (a statistic of the clip differs from one of a
    frame, a column of the stack changes at every seam), with a saturated and a grey patch in every frame."""
    g = np.random.RandomState(data_seed)
    out = []
    for h, w in sizes:
        f = np.stack([np.stack([g.randint(10 + 50 * t + 35 * c, 120 + 50 * t + 35 * c, (h, w)) for c in range(3)], axis=-1)
                      for t in range(frames_per_clip or T)]).astype(np.uint8)
        f[:, :2, :3] = g.randint(0, 256, (f.shape[0], min(2, h), min(3, w), 3))
        f[:, -1, -2:] = f[:, -1, -2:, :1]
        out.append(torch.from_numpy(f))
    return out


def case_want(case):
    raw = np.frombuffer(base64.b64decode(case["out"]), dtype=np.uint8)
    out, at = [], 0
    for h, w in case["sizes"]:
        out.append(torch.from_numpy(raw[at:at + T * h * w * 3].reshape(T, h, w, 3).copy()))
        at += T * h * w * 3
    assert at == len(raw)
    return out


def row_to_json(r):
    return [bool(r.jitter), [int(o) for o in r.order], r.brightness, r.contrast, r.saturation, r.hue, bool(r.gray), r.sigma]


def case_table(case):
    return sc.make_table(case["rows"], case["gray_first"])


def case_jitter(case):
    return sa.SslColorJitter(case["bri_con_sat"], case["hue"], case["p_convert_gray"], case["moco_v2_aug"])


# ---- numpy restatement of csrc/sf_sslcolor.h --------------------------------------------------------------------------
def rgb_to_hsv(rgb):
    """PIL's convert("HSV") of (..., 3) uint8 RGB."""
    v = rgb.astype(np.int64)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    f32, f64 = np.float32, np.float64
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    s = (cr / np.where(grey, 1, maxc).astype(f32)).astype(f32)
    rc = ((maxc - r).astype(f32) / cr).astype(f32)
    gc = ((maxc - g).astype(f32) / cr).astype(f32)
    bc = ((maxc - b).astype(f32) / cr).astype(f32)
    h = np.where(r == maxc, (bc - gc).astype(f32).astype(f64),
                 np.where(g == maxc, 2.0 + rc.astype(f64) - bc.astype(f64), 4.0 + gc.astype(f64) - rc.astype(f64))).astype(f32)
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """PIL's convert("RGB") of (..., 3) uint8 HSV."""
    x = hsv.astype(np.int64)
    h, s, v = x[..., 0], x[..., 1], x[..., 2]
    f32, f64 = np.float32, np.float64
    hf = h.astype(f64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int64)
    f = (hf - i.astype(f64)).astype(f32).astype(f64)
    fs = (s.astype(f64) / 255.0).astype(f32).astype(f64)
    vf = v.astype(f64)

    def rnd(a):                                             # C round() of a non-negative value, clipped
        return np.clip(np.floor(a + 0.5).astype(np.int64), 0, 255)
    p, q, t = rnd(vf * (1.0 - fs)), rnd(vf * (1.0 - fs * f)), rnd(vf * (1.0 - fs * (1.0 - f)))
    k = i % 6
    out = np.stack([np.choose(k, [v, q, p, p, t, v]), np.choose(k, [t, v, v, q, p, p]), np.choose(k, [p, p, t, v, v, q])], axis=-1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def shift_hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def box_pass(img, r, ww, fw, axis):
    """One iteration of PIL's extended box blur along ``axis``."""
    v = np.moveaxis(img.astype(np.int64), axis, 0)
    n = v.shape[0]
    idx = np.arange(n)
    acc = np.zeros_like(v)
    for k in range(-r, r + 1):
        acc += v[np.clip(idx + k, 0, n - 1)]
    far = v[np.clip(idx - r - 1, 0, n - 1)] + v[np.clip(idx + r + 1, 0, n - 1)]
    return np.moveaxis((acc * ww + far * fw + (1 << 23)) >> 24, 0, axis).astype(np.uint8)


def gaussian_blur(img, sigma):
    """PIL's ImageFilter.GaussianBlur(radius=sigma) of an (H, W, 3) uint8 image: three iterations along the rows, then three
    along the columns."""
    r, ww, fw = sc.box_blur_params(sigma)
    for axis in (1, 1, 1, 0, 0, 0):
        img = box_pass(img, r, ww, fw, axis)
    return img


def grey(img):
    return np.repeat(luma(img)[..., None], 3, axis=-1).astype(np.uint8)


def jitter(img, row, shift=None):
    for op in row.order:
        v = img.astype(np.int64)
        if op == sc.BRIGHTNESS and row.brightness is not None:
            img = blend(np.zeros_like(v), v, row.brightness).astype(np.uint8)
        elif op == sc.CONTRAST and row.contrast is not None:
            L = luma(img)
            m = int(int(L.sum()) / L.size + 0.5)            # over the whole stack: the clip
            img = blend(np.full_like(v, m), v, row.contrast).astype(np.uint8)
        elif op == sc.SATURATION and row.saturation is not None:
            img = blend(np.repeat(luma(img)[..., None], 3, axis=-1), v, row.saturation).astype(np.uint8)
        elif op == sc.HUE and row.hue is not None:
            img = shift_hue(img, sc.hue_shift(row.hue) if shift is None else shift)
    return img


def restate_clip(frames, row, gray_first, shift=None):
    """``row`` on the uint8 (T, h, w, 3) numpy frames of ONE clip, as the reference does it: on the (T * h, w, 3) stack."""
    frames = np.asarray(frames)
    img = frames.reshape(-1, frames.shape[2], 3)
    if gray_first and row.gray:
        img = grey(img)
    if row.jitter:
        img = jitter(img, row, shift)
    if not gray_first and row.gray:
        img = grey(img)
    if row.sigma is not None:
        img = gaussian_blur(img, row.sigma)
    return img.reshape(frames.shape)


def restate_batch(frames, table):
    return [torch.from_numpy(restate_clip(f.numpy(), table.rows[n], table.gray_first)) for n, f in enumerate(frames)]


def restate_draw(bri_con_sat, hue, p, moco, N):
    """torchvision's published behaviour, written down a second time: Compose([RandomApply([ColorJitter], 0.8), RandomGrayscale(p),
    RandomApply([GaussianBlur], 0.5)]) or Compose([RandomGrayscale(p), ColorJitter]), N times.  Rows as row_to_json gives them."""
    ranges = [None if v == 0 else (max(0.0, 1.0 - v), 1.0 + v) for v in bri_con_sat] + [None if hue == 0 else (-hue, hue)]

    def color_jitter():
        fn_idx = torch.randperm(4)
        vals = [None if rng is None else float(torch.empty(1).uniform_(rng[0], rng[1])) for rng in ranges]
        return [True, [int(i) for i in fn_idx]] + vals
    rows = []
    for _ in range(N):
        if moco:
            head = [False, [0, 1, 2, 3], None, None, None, None] if 0.8 < torch.rand(1) else color_jitter()
            g = bool(torch.rand(1) < p)
            sigma = None if 0.5 < torch.rand(1) else random.uniform(0.1, 2.0)
        else:
            g = bool(torch.rand(1) < p)
            head, sigma = color_jitter(), None
        rows.append(head + [g, sigma])
    return rows


def positions():
    """One more draw from each generator: where they stand."""
    return repr(float(torch.rand(1))), repr(random.random())


# ---- 1. the golden contract -------------------------------------------------------------------------------------------
def check_draw_case(index):
    case = CASES[index]
    N = len(case["sizes"])
    fn = case_jitter(case)
    torch.manual_seed(case["seed"])
    random.seed(case["seed"])
    table = fn.sample_batch(N)
    after = positions()
    assert isinstance(table, sa.SslTable) and all(isinstance(r, sa.SslRow) for r in table.rows)
    assert [row_to_json(r) for r in table.rows] == case["rows"], ("the draw differs from the recorded one", table.rows, case["rows"])
    assert table.gray_first == case["gray_first"] == (not case["moco_v2_aug"])
    assert list(after) == [case["torch_after"], case["py_after"]], "the generators were not consumed as recorded"
    return table


def check_restatement_golden(index):
    """CPU only: the numpy restatement reproduces PIL's recorded bytes."""
    case = CASES[index]
    got = restate_batch(case_frames(case["data_seed"], case["sizes"]), case_table(case))
    for n, want in enumerate(case_want(case)):
        assert differing(got[n], want) == 0, (case["name"], n, differing(got[n], want))


def check_golden_case(device, index):
    case = CASES[index]
    table = check_draw_case(index)
    frames = case_frames(case["data_seed"], case["sizes"])
    buf = padded(frames, fill=201)
    dev = buf.to(device)
    got = sa.ssl_color_clip(dev, table, case["sizes"]).cpu()
    assert torch.equal(dev.cpu(), buf), "frames must be left untouched"
    assert got.dtype == torch.uint8 and got.shape == buf.shape
    bad = 0
    for n, ((h, w), want) in enumerate(zip(case["sizes"], case_want(case))):
        bad += differing(got[n, :, :h, :w], want)
        mask = torch.ones(buf.shape[2:4], dtype=torch.bool)
        mask[:h, :w] = False
        assert torch.equal(got[n][:, mask], buf[n][:, mask]), "the padding must come out as it went in"
    print("case %d (%s): %d of %d bytes differ from PIL's" % (index, case["name"], bad, sum(T * h * w * 3 for h, w in case["sizes"])))
    assert bad == 0, (index, case["name"], bad)
    torch.manual_seed(case["seed"])                          # the object draws for itself when no table is given
    random.seed(case["seed"])
    own = case_jitter(case)(dev, sizes=case["sizes"]).cpu()
    assert torch.equal(own, got) and list(positions()) == [case["torch_after"], case["py_after"]]


def check_fixture_covers():
    rows = [(c, r) for c in CASES for r in c["rows"]]
    assert {c["moco_v2_aug"] for c in CASES} == {True, False}
    assert any(r[0] for _, r in rows) and any(not r[0] for _, r in rows), "jitter applied and not applied"
    assert any(r[6] for _, r in rows) and any(not r[6] for _, r in rows), "grey applied and not applied"
    assert any(r[7] is not None for _, r in rows) and any(r[7] is None for c, r in rows if c["moco_v2_aug"]), "blur drawn and not"
    assert any(r[0] and r[3] is None for _, r in rows), "a zero jitter value"
    assert len({tuple(r[1]) for _, r in rows if r[0]}) >= 6, "op orders"
    assert os.path.getsize(GOLDEN) < 512 * 1024


# ---- 2. the draw ------------------------------------------------------------------------------------------------------
DRAW_CASES = [((0.6, 0.6, 0.6), 0.15, 0.2, True), ((0.4, 0.4, 0.4), 0.1, 0.0, False), ((0.6, 0.6, 0.6), 0.15, 0.0, True),
              ((0.6, 0.6, 0.6), 0.15, 1.0, True), ((0.4, 0.4, 0.4), 0.1, 1.0, False), ((0.4, 0.0, 0.4), 0.1, 0.5, False),
              ((0.0, 0.5, 0.0), 0.0, 0.5, True), ((0.0, 0.0, 0.0), 0.0, 0.3, False)]


def check_draw(which):
    """sample_batch consumes both generators as the second restatement does and draws the same rows."""
    bcs, hue, p, moco = DRAW_CASES[which]
    fn = sa.SslColorJitter(bcs, hue, p, moco)
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        random.seed(seed)
        want = restate_draw(bcs, hue, p, moco, 16)
        want_after = positions()
        torch.manual_seed(seed)
        random.seed(seed)
        table = fn.sample_batch(16)
        assert positions() == want_after, "the generators were not consumed as torchvision consumes them"
        got = [row_to_json(r) for r in table.rows]
        assert got == want, (got, want)
        assert table.gray_first == (not moco)
        if p in (0.0, 1.0):
            assert all(r.gray == (p == 1.0) for r in table.rows)
        if not moco:
            assert all(r.jitter and r.sigma is None for r in table.rows)
        for r in table.rows:
            for v, jit in zip((r.brightness, r.contrast, r.saturation), bcs):
                assert (v is None) == (jit == 0 or not r.jitter), "a zero jitter value draws nothing"
            assert (r.hue is None) == (hue == 0 or not r.jitter)
            assert r.sigma is None or 0.1 <= r.sigma <= 2.0
    if moco and p not in (0.0, 1.0):
        assert {r.jitter for r in table.rows} == {True, False} and {r.sigma is None for r in table.rows} == {True, False}


# ---- 3. restatement parity --------------------------------------------------------------------------------------------
def _row(order=(0, 1, 2, 3), b=None, c=None, s=None, hue=None, gray=False, sigma=None, jitter=True):
    return sc.SslRow(jitter, tuple(order), b, c, s, hue, gray, sigma)


NOTHING = _row(jitter=False)
FULL = dict(b=1.37, c=0.55, s=1.6, hue=0.12)
ORDERS = [(0, 1, 2, 3), (1, 0, 2, 3), (0, 2, 3, 1), (3, 2, 1, 0), (2, 3, 0, 1), (3, 1, 0, 2), (2, 0, 1, 3), (1, 3, 2, 0)]
# name -> (four rows, gray_first)
TABLES = {
    "brightness": ([_row(b=f) for f in (1.37, 0.4, 1.0, 1.6)], False),
    "contrast": ([_row(c=f) for f in (0.55, 1.6, 0.4, 1.21)], False),
    "saturation": ([_row(s=f) for f in (1.6, 0.4, 0.0, 1.3)], False),
    "hue": ([_row(hue=f) for f in (0.12, -0.15, 0.0, 0.5)], False),
    "grey": ([_row(jitter=False, gray=True)] * 4, False),
    "blur0.1": ([_row(jitter=False, sigma=0.1)] * 4, False),
    "blur0.75": ([_row(jitter=False, sigma=0.75)] * 4, False),
    "blur2.0": ([_row(jitter=False, sigma=2.0)] * 4, False),
    "moco": ([_row(ORDERS[4 + k], gray=k == 1, sigma=(1.9, 0.3, 1.1, 0.62)[k], **FULL) for k in range(4)], False),
    "grey_first": ([_row(ORDERS[k], gray=k != 2, **FULL) for k in range(4)], True),
    # every pass has clips to skip: nothing at all, blur only, grey only, everything
    "mixed": ([NOTHING, _row(jitter=False, sigma=1.3), _row(jitter=False, gray=True), _row((2, 1, 3, 0), gray=True, sigma=0.9, **FULL)], False),
    "zero_jitter": ([_row((1, 0, 3, 2), b=0.8, s=1.2), _row((3, 1, 0, 2), c=1.4, hue=-0.05), _row(), _row((2, 3, 1, 0), c=0.7)], False),
}
for _k in range(0, 8, 4):                                   # eight of the 24 orders, contrast first and contrast last among them
    TABLES["orders%d" % _k] = ([_row(ORDERS[_k + j], **FULL) for j in range(4)], False)
TABLE_NAMES = sorted(TABLES)


def named_table(name):
    rows, gray_first = TABLES[name]
    return sc.SslTable(tuple(rows), gray_first)


def check_parity(device, name):
    """The issue's shapes: N = 4, T = 3, one 24 x 40 buffer.  Valid regions equal the restatement, byte for byte; the padding
    comes out as it went in; the input is unchanged."""
    table = named_table(name)
    frames = case_frames(41)
    buf = padded(frames, fill=0)
    g = torch.Generator().manual_seed(5)
    pattern = torch.randint(0, 256, buf.shape, generator=g, dtype=torch.int64).to(torch.uint8)
    for n, (h, w) in enumerate(SIZES):
        pattern[n, :, :h, :w] = frames[n]
    dev = pattern.to(device)
    got = sa.ssl_color_clip(dev, table, SIZES).cpu()
    assert torch.equal(dev.cpu(), pattern), "frames must be unchanged"
    want = restate_batch(frames, table)
    bad = [differing(got[n, :, :h, :w], want[n]) for n, (h, w) in enumerate(SIZES)]
    print("%s: differing bytes per sample %s" % (name, bad))
    assert bad == [0, 0, 0, 0], (name, bad)
    for n, (h, w) in enumerate(SIZES):
        mask = torch.ones(buf.shape[2:4], dtype=torch.bool)
        mask[:h, :w] = False
        assert torch.equal(got[n][:, mask], pattern[n][:, mask]), "the padding must come out as it went in"
    changed = [not torch.equal(want[n], frames[n]) for n in range(4)]
    assert any(changed), "the table must change something"
    return got, pattern


def big_shapes():
    """(Hs, Ws): more than one chunk per frame, more than one column strip and several runs of stacked rows per clip -- once
    with a slab that is no multiple of 16 pixels (thread-per-pixel accesses; rows that are not 4-byte aligned either) and once
    with one that is (16-byte accesses); and a frame so wide that a row-blur workgroup holds 6 rows, not 8."""
    assert _sflib.get_lib().call("sf_randaug_chunk") == 4096, "choose the shapes again for another chunk size"
    return [(71, 67), (80, 67), (3, 600)]


def big_case(which):
    """(sizes, frames per sample, table, padded buffer) of ``check_parity_big``."""
    Hs, Ws = big_shapes()[which]
    if which < 2:
        assert Hs * Ws > 4096 and ((Hs * Ws) % 16 == 0) == (which == 1) and Ws > 64 and Ws % 4
        sizes = [(Hs, Ws), (Hs - 9, Ws - 4)]                # the second sample: its valid region ends inside the second chunk
    else:
        assert 12288 // (3 * Ws) == 6 and Ws % 4 == 0
        sizes = [(Hs, Ws), (Hs - 1, Ws - 85)]
    frames = case_frames(100 + which, sizes, frames_per_clip=2)
    table = sc.SslTable((_row((0, 2, 1, 3), gray=False, sigma=1.7, **FULL), _row((3, 1, 2, 0), gray=True, sigma=0.45, **FULL)), False)
    return sizes, frames, table, padded(frames, fill=201)


def check_parity_big(device, which):
    sizes, frames, table, buf = big_case(which)
    Hs, Ws = big_shapes()[which]
    got = sa.ssl_color_clip(buf.to(device), table, sizes).cpu()
    want = restate_batch(frames, table)
    bad = [differing(got[n, :, :h, :w], want[n]) for n, (h, w) in enumerate(sizes)]
    print("%d x %d: differing bytes per sample %s" % (Hs, Ws, bad))
    assert bad == [0, 0], (Hs, Ws, bad)
    assert torch.equal(got[1, :, sizes[1][0]:], buf[1, :, sizes[1][0]:]) and torch.equal(got[1, :, :, sizes[1][1]:], buf[1, :, :, sizes[1][1]:])


def check_in_place_big(device, which):
    """The streaming pass in place (``out`` is the frames) across more than one chunk, on the thread-per-pixel accesses
    (``which`` 0) and the 16-byte ones (1): a thread reads its pixels before it writes them, so the bytes are those of the
    out-of-place call."""
    sizes, _, table, buf = big_case(which)
    want = sa.ssl_color_clip(buf.to(device), table, sizes).cpu()
    dev = buf.clone().to(device)                            # on the CPU ``to`` returns the tensor itself
    res = sa.ssl_color_clip(dev, table, sizes, out=dev)
    assert res is dev and not torch.equal(want, buf), "the table must change something"
    bad = differing(dev.cpu(), want)
    print("%d x %d in place: %d bytes differ from the out-of-place result" % (big_shapes()[which] + (bad,)))
    assert bad == 0, (which, bad)


# ---- 4. HSV -----------------------------------------------------------------------------------------------------------
def all_triples():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def check_hsv_exhaustive(direction):
    """CPU only: the numpy restatement against PIL over all 2^24 triples, one 4096 x 4096 image."""
    import pytest
    Image = pytest.importorskip("PIL.Image")
    tri = all_triples()
    if direction == "rgb_to_hsv":
        want, got = np.asarray(Image.fromarray(tri, "RGB").convert("HSV")), rgb_to_hsv(tri)
    else:
        want, got = np.asarray(Image.fromarray(tri, "HSV").convert("RGB")), hsv_to_rgb(tri)
    bad = int((want != got).any(-1).sum())
    print("%s: %d of 2^24 triples differ from PIL's" % (direction, bad))
    assert bad == 0, (direction, bad)


def hue_colours():
    """2^16 colours of the 2^24: a stride coprime to 2^24 walks through all three channels; (256, 256, 3)."""
    a = (np.arange(1 << 16, dtype=np.uint64) * 1000003 + 12345) % (1 << 24)
    assert len(np.unique(a)) == 1 << 16
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8).reshape(256, 256, 3)


def check_hue_subset(device):
    """The kernel's HSV round trip against the numpy restatement: 2^16 colours x the shifts 0, 1, 38, 128, 255 (one clip per
    shift; 128 is no int(hue_factor * 255) of a factor in [-0.5, 0.5], so the shifts are written into the packed rows)."""
    colours = hue_colours()
    N = len(HUE_SHIFTS)
    frames = torch.from_numpy(colours)[None, None].repeat(N, 1, 1, 1, 1).contiguous()
    table = sc.SslTable(tuple(_row(hue=0.1) for _ in range(N)), False)
    host = sc.pack_words(table, [(256, 256)] * N).reshape(N, sc.ROW_WORDS)
    host[:, 5] = HUE_SHIFTS
    got = sc.apply_words(frames.to(device), np.ascontiguousarray(host.reshape(-1))).cpu().numpy()
    for n, shift in enumerate(HUE_SHIFTS):
        want = shift_hue(colours, shift)
        bad = int((got[n, 0] != want).any(-1).sum())
        print("hue shift %d: %d of 65536 colours differ" % (shift, bad))
        assert bad == 0, (shift, bad)
    assert (got[0, 0] != colours).any(), "a shift of 0 is not the identity: the round trip through 8-bit HSV loses information"
    for f, shift in ((0.0, 0), (0.004, 1), (0.15, 38), (-0.004, 255), (0.5, 127), (-0.5, 129), (-0.15, 218)):
        assert sc.hue_shift(f) == shift, (f, sc.hue_shift(f))


def check_blur_against_pil():
    """CPU only: the box parameters and the blur against PIL over a sweep of sigma in [0.1, 2.0], images narrower and shorter
    than the box among them."""
    import pytest
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    g = np.random.RandomState(0)
    for shape in ((15, 9), (72, 40), (3, 1), (1, 7), (2, 2)):
        img = g.randint(0, 256, shape + (3,)).astype(np.uint8)
        for sigma in list(np.linspace(0.1, 2.0, 96)) + [0.75, 1.0, 0.5]:
            want = np.asarray(Image.fromarray(img, "RGB").filter(ImageFilter.GaussianBlur(radius=float(sigma))))
            assert differing(gaussian_blur(img, float(sigma)), want) == 0, (shape, sigma)
    for sigma in np.linspace(0.1, 2.0, 400):
        r, ww, fw = sc.box_blur_params(float(sigma))
        assert r in (0, 1) and ww > 0 and fw >= 0 and (2 * r + 1) * ww + 2 * fw <= 1 << 24, (sigma, r, ww, fw)
    assert sc.box_blur_params(0.1) == (0, 16721291, 27962) and sc.box_blur_params(2.0) == (1, 4473924, 1677722)


# ---- 5. padding and out= ----------------------------------------------------------------------------------------------
def check_out_and_in_place(device):
    """``out`` may be another tensor or the frames themselves (in place); anything else that overlaps them is rejected."""
    import pytest
    for name in ("moco", "mixed", "blur0.75", "orders0"):
        got, pattern = check_parity(device, name)
        table = named_table(name)
        out = torch.full_like(pattern, 99).to(device)
        res = sa.ssl_color_clip(pattern.to(device), table, SIZES, out=out)
        assert res.data_ptr() == out.data_ptr() and torch.equal(res.cpu(), got)
        dev = pattern.to(device)
        res = sa.ssl_color_clip(dev, table, SIZES, out=dev)
        assert res is dev and torch.equal(dev.cpu(), got), "in place must give the same bytes"
    dev = pattern.to(device)
    flat = torch.zeros(2 * dev.numel(), dtype=torch.uint8).to(device)
    with pytest.raises(sa.lib.SfError, match="overlap"):
        src = flat[:dev.numel()].view(dev.shape)
        sa.ssl_color_clip(src, table, SIZES, out=flat[3 * SIZES[0][1]:3 * SIZES[0][1] + dev.numel()].view(dev.shape))


# ---- 6. determinism ---------------------------------------------------------------------------------------------------
def check_determinism(device):
    frames = padded(case_frames(3)).to(device)
    table = named_table("moco")
    a = sa.ssl_color_clip(frames, table, SIZES).cpu()
    b = sa.ssl_color_clip(frames, table, SIZES).cpu()
    assert torch.equal(a, b), "two calls must give the same bytes"


# ---- 7. launch counts -------------------------------------------------------------------------------------------------
def _logged(device, table, out_is_frames=False):
    frames = padded(case_frames(7)).to(device)
    keep = frames.cpu()
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        got = sa.ssl_color_clip(frames, table, SIZES, out=frames if out_is_frames else None)
    finally:
        _sflib.set_call_observer(None)
    want = restate_batch(case_frames(7), table)
    assert all(differing(got.cpu()[n, :, :h, :w], want[n]) == 0 for n, (h, w) in enumerate(SIZES))
    return calls, got, frames, keep


def check_launch_counts(device):
    """At most four launches; every pass only when a row asks for it; none for a table of no-ops, whose result is a copy."""
    calls, _, _, _ = _logged(device, named_table("moco"))
    assert calls == ["sf_sslcolor_hist_u8", "sf_sslcolor_stream_u8", "sf_sslcolor_blur_rows_u8", "sf_sslcolor_blur_cols_u8"], calls
    calls, _, _, _ = _logged(device, named_table("brightness"))
    assert calls == ["sf_sslcolor_stream_u8"], calls
    calls, _, _, _ = _logged(device, named_table("orders0"))
    assert calls == ["sf_sslcolor_hist_u8", "sf_sslcolor_stream_u8"], calls
    calls, _, _, _ = _logged(device, named_table("blur2.0"))          # the streaming pass copies; in place it is not needed
    assert calls == ["sf_sslcolor_stream_u8", "sf_sslcolor_blur_rows_u8", "sf_sslcolor_blur_cols_u8"], calls
    calls, _, _, _ = _logged(device, named_table("blur2.0"), out_is_frames=True)
    assert calls == ["sf_sslcolor_blur_rows_u8", "sf_sslcolor_blur_cols_u8"], calls
    # no-ops: jitter not applied, no grey, no blur -- and a jitter whose four values are all zero
    for rows in ([NOTHING] * 4, [NOTHING, _row(), NOTHING, _row((3, 2, 1, 0))]):
        calls, got, frames, keep = _logged(device, sc.SslTable(tuple(rows), False))
        assert calls == [], calls
        assert got.data_ptr() != frames.data_ptr() and torch.equal(got.cpu(), keep), "a table of no-ops gives a COPY of the frames"
        calls, got, frames, keep = _logged(device, sc.SslTable(tuple(rows), False), out_is_frames=True)
        assert calls == [] and got is frames and torch.equal(got.cpu(), keep)


# ---- 8. composition ---------------------------------------------------------------------------------------------------
def check_composition(device):
    """jit -> RandAugment -> pack_pathways_u8(crop=) as the README loop chains them, against the two numpy restatements chained
    and packed by the same last call: equal model inputs, bit for bit."""
    frames = case_frames(23)
    table = named_table("moco")
    aug = ra.make_table([[(ra.ROTATE, False, 17.0), (ra.CONTRAST, False, 1.4)], [(ra.EQUALIZE, False, 0.0), (ra.SHARPNESS, False, 1.7)],
                         [(ra.SHEAR_X, False, 0.2), (ra.COLOR, False, 0.5)], [(ra.SOLARIZE, False, 120), (ra.TRANSLATE_Y_REL, False, 0.2)]])
    crop = ss.make_table([(24, 40, 0, 0, 24, 40, 12, 20, 3, 5, 0), (17, 23, 0, 0, 17, 23, 10, 14, 2, 1, 1),
                          (5, 9, 0, 0, 5, 9, 8, 14, 1, 2, 0), (24, 37, 0, 0, 24, 37, 13, 19, 0, 3, 1)], 6)
    cfg = sa.get_preset("C2D_8x8_R50", ["DATA.MEAN", [0.45, 0.40, 0.35], "DATA.STD", [0.225, 0.25, 0.2]])
    jit, rand = sa.SslColorJitter(moco_v2_aug=True), sa.RandAugment()
    dev = padded(frames).to(device)
    got = sa.pack_pathways_u8(rand(jit(dev, table, SIZES), aug, SIZES), cfg, crop=crop)
    restated = ra_checks.restate_batch(restate_batch(frames, table), aug)
    want = sa.pack_pathways_u8(padded(restated).to(device), cfg, crop=crop)
    assert len(got) == len(want) == 1
    assert torch.equal(got[0].cpu().view(torch.int16), want[0].cpu().view(torch.int16))
    plain = sa.pack_pathways_u8(rand(dev, aug, SIZES), cfg, crop=crop)
    assert not torch.equal(got[0].cpu().view(torch.int16), plain[0].cpu().view(torch.int16)), "the colour stage must show"


# ---- 9. rejections ----------------------------------------------------------------------------------------------------
def check_rejects(device):
    import pytest
    frames = padded(case_frames(3))
    fd = frames.to(device)
    good = named_table("moco")
    fn = sa.SslColorJitter((0.6, 0.6, 0.6), 0.15, 0.2, True)
    torch.manual_seed(5)
    random.seed(5)
    t_state, p_state = torch.get_rng_state(), random.getstate()

    def untouched():
        return torch.equal(torch.get_rng_state(), t_state) and random.getstate() == p_state
    calls = []
    _sflib.set_call_observer(lambda name, thunk, work: calls.append(name) or thunk())
    try:
        for bad in (fd.float(), fd.to(torch.int8), fd[0], fd[..., :2], fd[:, :, :, ::2], fd.transpose(2, 3)):
            for call in (lambda: fn(bad), lambda: fn(bad, good), lambda: sa.ssl_color_clip(bad, good)):
                with pytest.raises(sa.lib.SfError):
                    call()
            assert untouched(), "a rejected call must not consume random numbers"
        for n in (1, 3, 5):                                 # a table of the wrong length
            with pytest.raises(sa.lib.SfError, match="drawn for %d samples" % n):
                sa.ssl_color_clip(fd, sc.SslTable(tuple([good.rows[0]] * n), False))
        for sizes in ([(25, 40)] + SIZES[1:], [(24, 41)] + SIZES[1:], [(0, 40)] + SIZES[1:], [(24, 0)] + SIZES[1:], SIZES[:3]):
            with pytest.raises(sa.lib.SfError):
                sa.ssl_color_clip(fd, good, sizes)
            with pytest.raises(sa.lib.SfError):
                fn(fd, None, sizes)
            assert untouched()
        for row, what in ((_row((0, 1, 2, 2), **FULL), "no permutation"), (_row(b=float("nan")), "brightness factor"),
                          (_row(c=-0.1), "contrast factor"), (_row(hue=0.6), "hue factor"),
                          (_row(jitter=False, sigma=2.5), "sigma"), (_row(jitter=False, sigma=0.05), "sigma")):
            with pytest.raises(sa.lib.SfError, match=what):
                sa.ssl_color_clip(fd, sc.SslTable((row,) + good.rows[1:], False))
        with pytest.raises(sa.lib.SfError):
            sa.ssl_color_clip(fd, (good.rows, False))
        with pytest.raises(sa.lib.SfError):
            sa.ssl_color_clip(fd, good, out=torch.empty_like(fd)[:, :, :, :20])
        with pytest.raises(sa.lib.SfError):
            sa.ssl_color_clip(fd, good, out=torch.empty_like(fd).float())
        assert calls == [], "a rejected call never reaches the library"
        # the library's own checks (the Python side's are bypassed)
        lib = _sflib.get_lib()
        stream = sa.ops._stream(fd)
        host = sc.pack_words(good, SIZES).reshape(4, sc.ROW_WORDS)
        dev = torch.from_numpy(host.reshape(-1).copy()).to(device)
        out, hist = torch.empty_like(fd), torch.zeros(4 * 256, dtype=torch.int32).to(device)

        def entry(name, words, dst=out, h=hist):
            words = np.ascontiguousarray(words.reshape(-1))
            head = (fd.data_ptr(),) if name == "sf_sslcolor_hist_u8" else (fd.data_ptr(), dst.data_ptr())
            tail = (None if h is None else h.data_ptr(),) if name in names[:2] else ()
            lib.call(name, *head, 4, T, 24, 40, words.ctypes.data, dev.data_ptr(), *tail, stream)

        def edited(word, value, n=0):
            w = host.copy()
            w[n, word] = value
            return w
        names = ("sf_sslcolor_hist_u8", "sf_sslcolor_stream_u8", "sf_sslcolor_blur_rows_u8", "sf_sslcolor_blur_cols_u8")
        for words, what in ((edited(0, 16), "unknown flags"), (edited(1, 0x3214), "unknown op code"), (edited(1, 0x3200), "drawn twice"),
                            (edited(3, 0x7f800000), "finite"), (edited(5, 256), "hue shift"), (edited(6, 2), "box radius"),
                            (edited(7, 0), "box weights"), (edited(7, 1 << 23), "box weights"), (edited(9, 25), "not inside"),
                            (edited(10, 0, n=2), "not inside")):
            for name in names:
                with pytest.raises(sa.lib.SfError, match=what):
                    entry(name, words)
        with pytest.raises(sa.lib.SfError, match="needs the histograms"):
            entry("sf_sslcolor_stream_u8", host, h=None)
        for name in names[2:]:
            with pytest.raises(sa.lib.SfError, match="another buffer"):
                entry(name, host, dst=fd)
    finally:
        _sflib.set_call_observer(None)
    assert torch.equal(fd.cpu(), frames), "a rejected call wrote the frames"
    assert untouched()


def check_host_tensor_rejected():
    """With the gfx950 library a host tensor raises (there is no torch fallback) and consumes no random number."""
    import pytest
    frames = padded(case_frames(3))
    fn = sa.SslColorJitter(moco_v2_aug=True)
    good = named_table("moco")
    torch.manual_seed(5)
    random.seed(5)
    t_state, p_state = torch.get_rng_state(), random.getstate()
    for call in (lambda: fn(frames), lambda: fn(frames, good), lambda: sa.ssl_color_clip(frames, good)):
        with pytest.raises(sa.lib.SfError):
            call()
    assert torch.equal(torch.get_rng_state(), t_state) and random.getstate() == p_state


# ---- 10. host only ----------------------------------------------------------------------------------------------------
def check_byte_round_trip():
    """The reference's / 255 -> ToPILImage (mul(255).byte()) -> ... -> ToTensor (/ 255) round trip is the identity on bytes."""
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal((v.float() / 255).mul(255).byte(), v)
    assert torch.equal((v.float().div(255)).mul(255).byte().float().div(255), v.float() / 255)


def check_config():
    import pytest
    cfg = sa.get_cfg()
    d = cfg.DATA
    assert (d.SSL_COLOR_JITTER, d.SSL_COLOR_BRI_CON_SAT, d.SSL_COLOR_HUE, d.COLOR_RND_GRAYSCALE, d.SSL_MOCOV2_AUG, d.SSL_BLUR_SIGMA_MIN,
            d.SSL_BLUR_SIGMA_MAX) == (False, [0.4, 0.4, 0.4], 0.1, 0.0, False, [0.0, 0.1], [0.0, 2.0])     # the reference's defaults
    for mode in ("train", "val", "test"):
        assert sa.construct_ssl_color_jitter(cfg, mode) is None
    cfg.DATA.SSL_COLOR_JITTER = True
    assert sa.construct_ssl_color_jitter(cfg, "val") is None and sa.construct_ssl_color_jitter(cfg, "test") is None
    fn = sa.construct_ssl_color_jitter(cfg, "train")

    def fields(f):
        return (f.brightness, f.contrast, f.saturation, f.hue, f.p_convert_gray, f.moco_v2_aug)
    assert isinstance(fn, sa.SslColorJitter) and fields(fn) == ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1), 0.0, False)
    # the contrastive recipes; the two blur keys are not read (the reference never reads them either)
    cfg.merge_from_dict({"DATA": {"SSL_MOCOV2_AUG": True, "COLOR_RND_GRAYSCALE": 0.2, "SSL_COLOR_HUE": 0.15,
                                  "SSL_COLOR_BRI_CON_SAT": [0.6, 0.6, 0.6], "SSL_BLUR_SIGMA_MIN": [0.0, 0.5], "SSL_BLUR_SIGMA_MAX": [0.0, 0.6]}})
    fn = sa.construct_ssl_color_jitter(cfg, "train")
    assert fields(fn) == ((0.4, 1.6), (0.4, 1.6), (0.4, 1.6), (-0.15, 0.15), 0.2, True) and sc.BLUR_SIGMA == (0.1, 2.0)
    random.seed(0)
    torch.manual_seed(0)
    sigmas = [r.sigma for r in fn.sample_batch(64).rows if r.sigma is not None]
    assert min(sigmas) < 0.5 and max(sigmas) > 0.6, "the blur's range is hard-wired to [0.1, 2.0]"
    assert fields(sa.SslColorJitter((2.0, 0.0, 0.3), 0.0))[:4] == ((0.0, 3.0), None, (0.7, 1.3), None)
    for bad in (dict(bri_con_sat=(-0.1, 0.4, 0.4)), dict(hue=0.6), dict(hue=-0.1), dict(bri_con_sat=(0.4, 0.4))):
        with pytest.raises(sa.lib.SfError):
            sa.SslColorJitter(**bad)
    assert sa.SslColorJitter().sample_batch(0) == sc.SslTable((), True)
    with pytest.raises(sa.lib.SfError):
        sc.make_table([(True, (0, 1, 2, 3), None)])
    # the packed words
    w = sc.pack_words(named_table("mixed"), SIZES).reshape(4, sc.ROW_WORDS)
    assert w[:, 0].tolist() == [0, 4, 2, 7] and w[:, 9].tolist() == [24, 17, 5, 24] and w[:, 10].tolist() == [40, 23, 9, 37]
    assert w[3, 1] == 2 | 1 << 4 | 3 << 8 | 0 << 12 and w[3, 5] == 30 and tuple(w[1, 6:9]) == sc.box_blur_params(1.3)
    assert w[3, 2:5].view(np.float32).tolist() == [np.float32(1.37), np.float32(0.55), np.float32(1.6)]
    w = sc.pack_words(named_table("zero_jitter"), SIZES).reshape(4, sc.ROW_WORDS)
    assert w[:, 0].tolist() == [1, 1, 0, 1] and w[0, 1] == 7 | 0 << 4 | 7 << 8 | 2 << 12
    assert sc.pack_words(named_table("grey_first"), SIZES).reshape(4, sc.ROW_WORDS)[:, 0].tolist() == [11, 11, 1, 11]
