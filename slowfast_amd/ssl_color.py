"""SSL colour augmentation of a training batch on the device (``transform.color_jitter_video_ssl``,
slowfast/datasets/transform.py:1073-1121 with ``GaussianBlur`` at :1145-1157; switched on by ``DATA.SSL_COLOR_JITTER`` and applied
at datasets/kinetics.py:378-387 to the decoded uint8 frames, in FRONT of RandAugment).

The reference turns a clip into ONE PIL image, the (T * h) x w stack of its frames, and runs torchvision's PIL transforms on
it.  Here the DRAW stays on the host and the arithmetic runs on the device, on the dense uint8 (N, T, Hs, Ws, 3) buffer
``rand_augment`` takes (RGB byte order, every sample padded to the batch's largest frame).  The result is a uint8 buffer of the
same shape: what ``RandAugment.__call__``, ``sample_clip`` and ``data.pack_pathways_u8(..., crop=...)`` take.  The reference's
``/ 255`` -> ``ToPILImage`` (``mul(255).byte()``) -> ... -> ``ToTensor`` round trip is the identity on bytes, so nothing is lost
by staying in uint8.  Inside a sample's valid h x w region the bytes are PIL's, bit for bit (pinned by
tests/golden/ssl_color_contract.json, recorded with PIL itself); outside it they are a copy of the input.

Because the image is the stack, Contrast's mean is the CLIP's (all T * h * w pixels), and the blur's column passes run across the
frame seams: rows are replicated only above frame 0 and below frame T - 1.

The draw -- PARITY UNPINNED.  torchvision is not installed where this was written, so ``sample_params`` restates its published
behaviour (``ColorJitter.get_params``, ``RandomApply``, ``RandomGrayscale``) and nothing pins it against torchvision itself, as
batchnorm.py is unpinned against pytorchvideo.  Everything comes from the global ``torch`` CPU generator, except the blur's sigma,
which comes from Python's ``random``:

* ``moco_v2_aug`` (DATA.SSL_MOCOV2_AUG), in this order: ``RandomApply(ColorJitter, p=0.8)`` -- one ``torch.rand(1)``; the jitter is
  applied unless ``0.8 < u``, and only then draws ``torch.randperm(4)`` and one ``torch.empty(1).uniform_(lo, hi)`` each for
  brightness, contrast, saturation (``[max(0, 1 - v), 1 + v]``) and hue (``[-hue, hue]``); ``RandomGrayscale`` -- one
  ``torch.rand(1)``, grey if ``u < p``; ``RandomApply(GaussianBlur, p=0.5)`` -- one ``torch.rand(1)``, blur unless ``0.5 < u``, and only
  then ``random.uniform(0.1, 2.0)``.
* otherwise: ``RandomGrayscale`` first, then ``ColorJitter`` always; no blur.
* a jitter value of zero: torchvision holds ``None`` for it, draws nothing and skips the op (the permutation is still drawn).

The four ops are applied in the permutation's order (0 brightness, 1 contrast, 2 saturation, 3 hue): PIL's ``ImageEnhance``
blends, and for hue PIL's ``convert("HSV")``, ``H += int(hue_factor * 255)`` in uint8, ``convert("RGB")`` -- also for a shift of 0,
which is NOT the identity (the round trip through 8-bit HSV loses information).  The rules are written out in
csrc/sf_sslcolor.h.

``ssl_color_clip`` launches at most four passes: the clip histograms (only when a row drew contrast), the streaming pass,
the blur's row pass and its column pass (only when a row drew the blur).  A table whose rows are all no-ops launches nothing:
the result is then a COPY of the frames (``out`` filled by a device copy), or the frames themselves when ``out`` is the frames.
``out`` may be the frames tensor itself: the call then works in place.  Any other overlap is rejected.

Not restated: ``DATA.TIME_DIFF_PROB`` (``augment_raw_frames``; no recipe sets it) and ``TRAIN_JITTER_MOTION_SHIFT``.
"""
import collections
import math
import random

import numpy as np
import torch

from . import spatial_sampling
from .lib import SfError, get_lib

ROW_WORDS = 16          # csrc/sf_sslcolor.h: SF_SSLCOLOR_ROW_WORDS
FLAG_JITTER, FLAG_GREY, FLAG_BLUR, FLAG_GREY_FIRST = 1, 2, 4, 8
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)
NOP = 7                 # an order field whose op was not drawn
# The reference passes DATA.SSL_BLUR_SIGMA_MIN / _MAX into color_jitter_video_ssl and never reads them there: the blur's range is
# hard-wired (transform.py:1098).  So it is here; the two keys exist in the config and are not read.
BLUR_SIGMA = (0.1, 2.0)
MAX_WIDTH = 4096        # csrc/sf_sslcolor.h: SF_SSLCOLOR_MAX_W (the row blur keeps a row in LDS)

# one clip's draw.  jitter: ColorJitter is applied; order: the permutation (four op codes; meaningless without jitter);
# brightness, contrast, saturation: the blend factors, hue: the hue factor -- each None when its jitter value is zero or the
# jitter is not applied; gray: RandomGrayscale is applied; sigma: the blur's sigma, None without blur
SslRow = collections.namedtuple("SslRow", ["jitter", "order", "brightness", "contrast", "saturation", "hue", "gray", "sigma"])
# rows: a tuple of N SslRows; gray_first: grey comes before the jitter (the non-MoCo branch)
SslTable = collections.namedtuple("SslTable", ["rows", "gray_first"])


def make_table(rows, gray_first=False):
    """An explicit SslTable from N SslRow-like tuples."""
    out = []
    for r in rows:
        if len(r) != 8:
            raise SfError("SslColorJitter: a row is (jitter, order, brightness, contrast, saturation, hue, gray, sigma)")
        jitter, order, b, c, s, hue, gray, sigma = r
        out.append(SslRow(bool(jitter), tuple(int(o) for o in order), *(None if v is None else float(v) for v in (b, c, s, hue)),
                          bool(gray), None if sigma is None else float(sigma)))
    return SslTable(tuple(out), bool(gray_first))


def hue_shift(hue_factor):
    """What torchvision's PIL backend adds to the H channel: ``np.uint8(hue_factor * 255)``, truncated toward zero, mod 256."""
    return int(hue_factor * 255) % 256


def box_blur_params(sigma):
    """PIL's ``GaussianBlur(radius=sigma)`` as three iterations of an extended box blur: (r, ww, fw) -- the integer radius, the 8.24
    fixed-point weight of a full tap and that of the two fractional taps at distance r + 1.  PIL works in C floats: sigma arrives
    as one, ``sigma2 = sigma * sigma / 3``, ``L = sqrt(12 * sigma2 + 1)`` and ``l = floor((L - 1) / 2)`` in double rounded to float,
    ``a = (2l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1)^2))`` and the box radius ``l + a`` in float;
    ``ww = (uint32)(2^24 / (2 * radius + 1))`` in float, ``fw = (2^24 - (2r + 1) * ww) / 2`` in integers."""
    f32 = np.float32
    sigma = f32(sigma)
    sigma2 = f32(f32(sigma * sigma) / f32(3))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    radius = f32(l + a)
    r = int(radius)
    ww = int(f32(f32(1 << 24) / f32(f32(radius * f32(2)) + f32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _check_table(table, N):
    """The draw itself, before any launch."""
    if not (isinstance(table, SslTable) and isinstance(table.rows, tuple) and all(isinstance(r, SslRow) for r in table.rows)):
        raise SfError("SslColorJitter: a table is an SslTable of SslRows (make_table builds one)")
    if len(table.rows) != N:
        raise SfError("SslColorJitter: the table was drawn for %d samples, the batch has %d" % (len(table.rows), N))
    for n, r in enumerate(table.rows):
        if r.jitter:
            if sorted(r.order) != [0, 1, 2, 3]:
                raise SfError("SslColorJitter: row %d: the op order %r is no permutation of 0 .. 3" % (n, r.order))
            for name, v in (("brightness", r.brightness), ("contrast", r.contrast), ("saturation", r.saturation)):
                if v is not None and not (math.isfinite(v) and v >= 0):
                    raise SfError("SslColorJitter: row %d: the %s factor %r is not a finite non-negative number" % (n, name, v))
            if r.hue is not None and not -0.5 <= r.hue <= 0.5:
                raise SfError("SslColorJitter: row %d: the hue factor %r is not in [-0.5, 0.5]" % (n, r.hue))
        if r.sigma is not None and not BLUR_SIGMA[0] <= r.sigma <= BLUR_SIGMA[1]:
            raise SfError("SslColorJitter: row %d: the blur's sigma %r is not in [%s, %s]" % ((n, r.sigma) + BLUR_SIGMA))


def pack_words(table, sizes):
    """SslTable + the samples' (h, w) -> the int32 words of csrc/sf_sslcolor.h, row n at n * ROW_WORDS."""
    N = len(table.rows)
    words = np.zeros((N, ROW_WORDS), dtype=np.int32)
    for n, r in enumerate(table.rows):
        row = words[n]
        row[9], row[10] = sizes[n]
        flags = 0
        if r.jitter:
            drawn = {BRIGHTNESS: r.brightness, CONTRAST: r.contrast, SATURATION: r.saturation, HUE: r.hue}
            fields = [op if drawn[op] is not None else NOP for op in r.order]
            if any(f != NOP for f in fields):
                flags |= FLAG_JITTER
                row[1] = sum(f << (4 * k) for k, f in enumerate(fields))
                row[2:5].view(np.float32)[:] = [np.float32(1.0 if v is None else v) for v in (r.brightness, r.contrast, r.saturation)]
                row[5] = 0 if r.hue is None else hue_shift(r.hue)
        if r.gray:
            flags |= FLAG_GREY | (FLAG_GREY_FIRST if table.gray_first else 0)
        if r.sigma is not None:
            flags |= FLAG_BLUR
            row[6], row[7], row[8] = box_blur_params(r.sigma)
        row[0] = flags
    return np.ascontiguousarray(words.reshape(-1))


def _needs_hist(row):
    return bool(row[0] & FLAG_JITTER) and any(((int(row[1]) >> (4 * k)) & 15) == CONTRAST for k in range(4))


def apply_words(frames, host, out=None):
    """The launches for the packed rows ``host`` (``pack_words``; the library validates them): see ``ssl_color_clip``."""
    stream = spatial_sampling.check_frames(frames, "SslColorJitter")
    N, T, Hs, Ws, _ = frames.shape
    spatial_sampling.check_out(frames, out, "SslColorJitter", in_place=True)
    in_place = out is frames
    if out is None:
        out = torch.empty_like(frames)
    rows = host.reshape(-1, ROW_WORDS)
    if host.dtype != np.int32 or len(rows) != N:
        raise SfError("SslColorJitter: %d int32 rows of %d words, not %s %s" % (N, ROW_WORDS, host.dtype, host.shape))
    flags = rows[:, 0]
    any_blur = bool(np.any(flags & FLAG_BLUR))
    if any_blur and Ws > MAX_WIDTH:
        raise SfError("SslColorJitter: the blur keeps a row in LDS: frames wider than %d pixels are not supported" % MAX_WIDTH)
    if frames.numel() == 0 or not np.any(flags & (FLAG_JITTER | FLAG_GREY | FLAG_BLUR)):
        return out if in_place else out.copy_(frames)
    dev = torch.from_numpy(host).to(frames.device)          # one host-to-device copy
    tmp, hist = spatial_sampling.frame_scratch(frames, "SslColorJitter", ((N, 256), torch.int32))   # the blur's buffer, L
    lib = get_lib()
    args = (N, T, Hs, Ws, host.ctypes.data, dev.data_ptr())
    need_hist = any(_needs_hist(r) for r in rows)
    if need_hist:
        lib.call("sf_sslcolor_hist_u8", frames.data_ptr(), *args, hist.data_ptr(), stream, work=dict(bytes=1.0 * frames.numel()))
    if not in_place or np.any(flags & (FLAG_JITTER | FLAG_GREY)):
        lib.call("sf_sslcolor_stream_u8", frames.data_ptr(), out.data_ptr(), *args, hist.data_ptr() if need_hist else None, stream,
                 work=dict(bytes=2.0 * frames.numel()))
    if any_blur:                                            # out -> tmp -> out, inside the blurred clips' valid regions only
        lib.call("sf_sslcolor_blur_rows_u8", out.data_ptr(), tmp.data_ptr(), *args, stream, work=dict(bytes=2.0 * frames.numel()))
        lib.call("sf_sslcolor_blur_cols_u8", tmp.data_ptr(), out.data_ptr(), *args, stream, work=dict(bytes=2.0 * frames.numel()))
    return out


def ssl_color_clip(frames, table, sizes=None, out=None):
    """Applies ``table`` to the dense uint8 (N, T, Hs, Ws, 3) device buffer; ``sizes[n] = (h, w)``: the valid frame size of
    sample n (default: the whole buffer).  Returns a uint8 tensor of the same shape: ``out`` when given (it may be ``frames``
    itself: in place), a new tensor otherwise; ``frames`` is left untouched unless it is ``out``.  At most one histogram pass, one
    streaming pass, one row and one column blur pass; nothing when every row is a no-op (the result is then a copy of the
    frames, or the frames themselves in place)."""
    spatial_sampling.check_frames(frames, "SslColorJitter")
    _check_table(table, frames.shape[0])
    sizes = spatial_sampling.check_sizes(frames, sizes, "SslColorJitter")
    spatial_sampling.check_out(frames, out, "SslColorJitter", in_place=True)
    return apply_words(frames, pack_words(table, sizes), out)


def _jitter_range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
    """torchvision's ColorJitter._check_input: None when the range is the single point ``center``."""
    if isinstance(value, (int, float)):
        if value < 0:
            raise SfError("SslColorJitter: %s must be non-negative (got %r)" % (name, value))
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        value = [float(value[0]), float(value[1])]
    else:
        raise SfError("SslColorJitter: %s is a number or a (min, max) pair (got %r)" % (name, value))
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise SfError("SslColorJitter: the %s range %r is not inside %r" % (name, value, bound))
    return None if value[0] == value[1] == center else tuple(value)


class SslColorJitter:
    """``color_jitter_video_ssl(frames, bri_con_sat, hue, p_convert_gray, moco_v2_aug)`` for a batch."""

    def __init__(self, bri_con_sat=(0.4, 0.4, 0.4), hue=0.1, p_convert_gray=0.0, moco_v2_aug=False):
        if len(bri_con_sat) != 3:
            raise SfError("SslColorJitter: bri_con_sat holds the brightness, contrast and saturation jitter (got %r)" % (bri_con_sat,))
        self.brightness = _jitter_range(bri_con_sat[0], "brightness")
        self.contrast = _jitter_range(bri_con_sat[1], "contrast")
        self.saturation = _jitter_range(bri_con_sat[2], "saturation")
        self.hue = _jitter_range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        self.p_convert_gray = float(p_convert_gray)
        self.moco_v2_aug = bool(moco_v2_aug)

    # ---- the draw (host) ------------------------------------------------------------------------------------------
    def _jitter_params(self):
        """ColorJitter.get_params: the permutation, then one uniform per op that has a range."""
        order = tuple(int(i) for i in torch.randperm(4))
        values = [None if rng is None else float(torch.empty(1).uniform_(rng[0], rng[1]))
                  for rng in (self.brightness, self.contrast, self.saturation, self.hue)]
        return (order,) + tuple(values)

    def sample_params(self):
        """One clip's draw: an SslRow."""
        none = ((0, 1, 2, 3), None, None, None, None)
        if self.moco_v2_aug:
            jitter = not bool(0.8 < torch.rand(1))
            params = self._jitter_params() if jitter else none
            gray = bool(torch.rand(1) < self.p_convert_gray)
            blur = not bool(0.5 < torch.rand(1))
            sigma = random.uniform(BLUR_SIGMA[0], BLUR_SIGMA[1]) if blur else None
            return SslRow(jitter, *params, gray, sigma)
        gray = bool(torch.rand(1) < self.p_convert_gray)
        return SslRow(True, *self._jitter_params(), gray, None)

    def sample_batch(self, N):
        """The draws of clips 0 .. N-1 in that order, as a single dataset worker would make them: an SslTable."""
        return SslTable(tuple(self.sample_params() for _ in range(int(N))), not self.moco_v2_aug)

    # ---- the device side ------------------------------------------------------------------------------------------
    def __call__(self, frames, table=None, sizes=None, out=None):
        """Augments the uint8 (N, T, Hs, Ws, 3) frames; draws when no table is given."""
        spatial_sampling.check_frames(frames, "SslColorJitter")    # before the draw: a rejected call consumes no random numbers
        spatial_sampling.check_sizes(frames, sizes, "SslColorJitter")
        if table is None:
            table = self.sample_batch(frames.shape[0])
        return ssl_color_clip(frames, table, sizes, out)


def construct_ssl_color_jitter(cfg, mode):
    """The colour stage of Kinetics.__getitem__ (datasets/kinetics.py:378-387): an object for "train" with DATA.SSL_COLOR_JITTER,
    None otherwise."""
    if mode != "train" or not cfg.DATA.SSL_COLOR_JITTER:
        return None
    return SslColorJitter(bri_con_sat=cfg.DATA.SSL_COLOR_BRI_CON_SAT, hue=cfg.DATA.SSL_COLOR_HUE,
                          p_convert_gray=cfg.DATA.COLOR_RND_GRAYSCALE, moco_v2_aug=cfg.DATA.SSL_MOCOV2_AUG)
