"""RandAugment of a training batch on the device (slowfast/datasets/rand_augment.py ``rand_augment_transform`` as
``transform.create_random_augment`` calls it, applied at datasets/kinetics.py:389-400 to the decoded uint8 frames in front of
``tensor_normalize``, ``spatial_sampling`` and ``RandomErasing``).

The reference runs a PIL loop on the host: T frames x ``n`` ops per clip.  Here the DRAW stays on the host and the 15 ops run
on the device, on the dense uint8 (N, T, Hs, Ws, 3) buffer ``spatial_sampling.check_frames`` accepts (RGB byte order, every
sample padded to the batch's largest frame).  The result is a uint8 buffer of the same shape: what ``sample_clip`` and
``data.pack_pathways_u8(..., crop=...)`` take.  Inside a sample's valid h x w region the bytes are PIL's, bit for bit (pinned by
tests/golden/rand_augment_contract.json); outside it they are a copy of the input.

The draw.  ``sample_params()`` consumes ``np.random`` and Python's ``random`` in exactly the reference's order:

* one ``np.random.choice`` over the 15 ops for the ``n`` layers (``replace=True`` and no weights without a ``w`` section,
  ``replace=False`` with the normalised weights of set 0 with ``w0``);
* per chosen op, in order: ``random.random()`` against the probability 0.5 -- when it is larger the op is skipped and nothing
  more is drawn for it; ``random.gauss(m, mstd)`` when ``mstd > 0`` (``random.gauss`` itself: it caches a second value); the
  magnitude clipped to [0, 10]; then the op's level function, which draws one more ``random.random()`` for the sign of Rotate,
  ShearX / Y, TranslateXRel / YRel and the four ``*Increasing`` enhance ops.

The draw is per CLIP (every frame gets the same ops with the same arguments) and holds op codes and arguments only: degrees,
shear factor, translate percentage, blend factor, bit count, threshold, added value -- nothing that depends on the frame size.
``sample_batch`` files N draws in an ``AugTable``.  ``rand_augment_clip`` turns it into the int32 words of csrc/sf_randaug.h for
the batch's frame sizes (PIL's inverse affine matrix as fp64 bit pairs, computed here in Python doubles: no trigonometry on the
device) and applies it layer by layer.

Not supported: ``interpolation="random"`` (a filter drawn per FRAME inside the PIL loop), ``auto_augment`` policies other than
``rand``, and the ImageNet loader's use of the transform (one image, ``translate_const`` ops).
"""
import collections
import math
import random
import re
import struct

import numpy as np
import torch

from . import spatial_sampling
from .lib import SfError, get_lib

ROW_WORDS = 20          # csrc/sf_randaug.h: SF_RANDAUG_ROW_WORDS
# slowfast/config/defaults.py:193, :196 -- the reference's defaults of AUG.AA_TYPE and AUG.INTERPOLATION, which
# construct_rand_augment reads from the cfg when it carries them (a merged recipe does: config.CfgNode keeps every key)
AA_TYPE_DEFAULT, INTERPOLATION_DEFAULT = "rand-m9-mstd0.5-inc1", "bicubic"
MAX_LEVEL = 10.0

# op codes: the position in the reference's transform lists (the plain and the increasing list name the same 15 ops)
(AUTO_CONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X,
 SHEAR_Y, TRANSLATE_X_REL, TRANSLATE_Y_REL) = range(15)
OP_NAMES = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
            "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
NUM_OPS = len(OP_NAMES)
# the choice weights of set 0 (``w0``), in op-code order
CHOICE_WEIGHTS_0 = (0.025, 0.005, 0, 0.3, 0, 0.005, 0.005, 0.025, 0.005, 0.005, 0.025, 0.2, 0.2, 0.1, 0.1)

# op classes of a table row (csrc/sf_randaug.h)
CLS_COPY, CLS_LUT, CLS_COLOR, CLS_SHARPNESS, CLS_AFFINE = range(5)
LUT_OPS = (AUTO_CONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, CONTRAST, BRIGHTNESS)
HIST_OPS = (AUTO_CONTRAST, EQUALIZE, CONTRAST)
AFFINE_OPS = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X_REL, TRANSLATE_Y_REL)
ENHANCE_OPS = (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS)
INT_OPS = (POSTERIZE, SOLARIZE, SOLARIZE_ADD)
FILTERS = {"bilinear": 0, "bicubic": 1}

# one layer of one clip's draw.  op: the op code; skip: the probability draw skipped it (arg is 0.0 then); arg: degrees (Rotate),
# the shear factor, the translate percentage, the blend factor (Color, Contrast, Brightness, Sharpness), the bit count
# (Posterize), the threshold (Solarize), the added value (SolarizeAdd), 0.0 for the ops without an argument
AugRow = collections.namedtuple("AugRow", ["op", "skip", "arg"])
# ops: int32 (N, L); skip: bool (N, L); args: float64 (N, L); filter: 0 bilinear / 1 bicubic (what the affine ops resample with)
AugTable = collections.namedtuple("AugTable", ["ops", "skip", "args", "filter"])


def _filter_id(interpolation):
    if interpolation == "random":
        raise NotImplementedError("RandAugment: interpolation='random' draws a filter per frame inside the reference's PIL loop; "
                                  "the per-clip table has no place for it")
    if interpolation not in FILTERS:
        raise SfError("RandAugment: interpolation must be 'bicubic' or 'bilinear' (got %r; PIL's transform refuses lanczos and "
                      "hamming as well)" % (interpolation,))
    return FILTERS[interpolation]


def make_table(rows, interpolation="bicubic"):
    """An explicit AugTable from N clips' rows: each a sequence of L AugRow-like (op, skip, arg) tuples."""
    rows = [[tuple(r) for r in clip] for clip in rows]
    L = len(rows[0]) if rows else 0
    if any(len(clip) != L for clip in rows) or any(len(r) != 3 for clip in rows for r in clip):
        raise SfError("RandAugment: every clip of a table has the same number of (op, skip, arg) rows")
    ops = np.array([[int(r[0]) for r in clip] for clip in rows], dtype=np.int32).reshape(len(rows), L)
    skip = np.array([[bool(r[1]) for r in clip] for clip in rows], dtype=bool).reshape(len(rows), L)
    args = np.array([[float(r[2]) for r in clip] for clip in rows], dtype=np.float64).reshape(len(rows), L)
    return AugTable(ops, skip, args, _filter_id(interpolation))


def _bits64(v):
    lo, hi = struct.unpack("<ii", struct.pack("<d", float(v)))
    return lo, hi


def affine_matrix(op, arg, w, h):
    """PIL's inverse affine matrix (a0 .. a5) of a geometric op on a w x h image, in Python doubles; None when Rotate's angle
    is a multiple of 360 (PIL returns a copy)."""
    if op == SHEAR_X:
        return (1.0, float(arg), 0.0, 0.0, 1.0, 0.0)
    if op == SHEAR_Y:
        return (1.0, 0.0, 0.0, float(arg), 1.0, 0.0)
    if op == TRANSLATE_X_REL:
        return (1.0, 0.0, float(arg) * w, 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y_REL:
        return (1.0, 0.0, 0.0, 0.0, 1.0, float(arg) * h)
    angle = float(arg) % 360.0                              # Image.rotate
    if angle == 0:
        return None
    if angle in (90, 180, 270):
        raise SfError("RandAugment: Rotate by %r degrees takes PIL's transpose shortcut, which is not restated (the draw cannot "
                      "produce it)" % (arg,))
    cx, cy = w / 2, h / 2
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def _check_table(table, N):
    """The draw itself, before any launch."""
    if not (isinstance(table, AugTable) and isinstance(table.ops, np.ndarray) and table.ops.ndim == 2
            and table.ops.dtype == np.int32 and np.shape(table.skip) == table.ops.shape and np.shape(table.args) == table.ops.shape):
        raise SfError("RandAugment: a table is an AugTable of (N, L) ops, skips and arguments (make_table builds one)")
    if len(table.ops) != N:
        raise SfError("RandAugment: the table was drawn for %d samples, the batch has %d" % (len(table.ops), N))
    if table.filter not in (0, 1):
        raise SfError("RandAugment: filter %r is neither 0 (bilinear) nor 1 (bicubic)" % (table.filter,))
    for n in range(N):
        for l in range(table.ops.shape[1]):
            op, arg = int(table.ops[n, l]), float(table.args[n, l])
            if op < 0 or op >= NUM_OPS:
                raise SfError("RandAugment: row %d layer %d: unknown op code %d" % (n, l, op))
            if table.skip[n, l]:
                continue
            if not math.isfinite(arg):
                raise SfError("RandAugment: row %d layer %d: the argument is not finite" % (n, l))
            if op in INT_OPS and arg != int(arg):
                raise SfError("RandAugment: row %d layer %d: %s takes an integer (got %r)" % (n, l, OP_NAMES[op], arg))
            if op == POSTERIZE and not 0 <= arg <= 8:
                raise SfError("RandAugment: row %d layer %d: Posterize keeps 0 .. 8 bits (got %d)" % (n, l, arg))
            if op == SOLARIZE and not 0 <= arg <= 256:
                raise SfError("RandAugment: row %d layer %d: Solarize takes a threshold of 0 .. 256 (got %d)" % (n, l, arg))
            if op == SOLARIZE_ADD and not 0 <= arg <= 255:
                raise SfError("RandAugment: row %d layer %d: SolarizeAdd adds 0 .. 255 (got %d)" % (n, l, arg))


def pack_words(table, sizes):
    """AugTable + the samples' (h, w) -> the int32 words of csrc/sf_randaug.h, layer-major: row (l, n) at (l * N + n)."""
    N, L = table.ops.shape
    words = np.zeros((L, N, ROW_WORDS), dtype=np.int32)
    for n in range(N):
        h, w = sizes[n]
        for l in range(L):
            op, arg = int(table.ops[n, l]), float(table.args[n, l])
            row = words[l, n]
            row[1], row[5], row[6] = op, h, w
            row[4] = table.filter
            if table.skip[n, l]:
                continue                                    # class 0: a copy
            if op in LUT_OPS:
                row[0] = CLS_LUT
            elif op == COLOR:
                row[0] = CLS_COLOR
            elif op == SHARPNESS:
                row[0] = CLS_SHARPNESS
            else:
                m = affine_matrix(op, arg, w, h)
                if m is None:
                    continue                                # Rotate by a multiple of 360 degrees: PIL copies
                if not all(math.isfinite(v) for v in m):
                    raise SfError("RandAugment: row %d layer %d: the affine matrix is not finite" % (n, l))
                row[0] = CLS_AFFINE
                for k, v in enumerate(m):
                    row[8 + 2 * k], row[9 + 2 * k] = _bits64(v)
            if op in INT_OPS:
                row[2] = int(arg)
            if op in ENHANCE_OPS:
                row[3:4].view(np.float32)[0] = np.float32(arg)
    return np.ascontiguousarray(words.reshape(-1))


def rand_augment_clip(frames, table, sizes=None, out=None):
    """Applies ``table`` to the dense uint8 (N, T, Hs, Ws, 3) device buffer; ``sizes[n] = (h, w)``: the valid frame size of
    sample n (default: the whole buffer).  Returns a uint8 tensor of the same shape (``out``: the tensor to write into) and
    leaves ``frames`` untouched.  At most one histogram pass and one streaming pass per layer."""
    stream = spatial_sampling.check_frames(frames, "RandAugment")
    N, T, Hs, Ws, _ = frames.shape
    _check_table(table, N)
    sizes = spatial_sampling.check_sizes(frames, sizes, "RandAugment")
    spatial_sampling.check_out(frames, out, "RandAugment")
    if out is None:
        out = torch.empty_like(frames)
    host = pack_words(table, sizes)
    L = table.ops.shape[1]
    if L == 0 or frames.numel() == 0:
        return out.copy_(frames)
    dev = torch.from_numpy(host).to(frames.device)          # every layer's rows: one host-to-device copy
    # the ping-pong buffer, the histograms (R, G, B, L) and the lookup tables of every frame
    tmp, hist, lut = spatial_sampling.frame_scratch(frames, "RandAugment", ((N * T, 4, 256), torch.int32),
                                                    ((N * T, 3, 256), torch.uint8))
    lib = get_lib()
    rows = host.reshape(L, N, ROW_WORDS)
    src = frames
    for l in range(L):
        dst = out if (L - 1 - l) % 2 == 0 else tmp           # ping-pong so that the last layer writes ``out``
        host_l, dev_l = rows[l].ctypes.data, dev.data_ptr() + 4 * l * N * ROW_WORDS
        need_hist = bool(np.any((rows[l, :, 0] == CLS_LUT) & np.isin(rows[l, :, 1], HIST_OPS)))
        if need_hist:
            lib.call("sf_randaug_hist_u8", src.data_ptr(), N, T, Hs, Ws, host_l, dev_l, hist.data_ptr(), stream,
                     work=dict(bytes=1.0 * frames.numel()))
        lib.call("sf_randaug_layer_u8", src.data_ptr(), dst.data_ptr(), N, T, Hs, Ws, host_l, dev_l,
                 hist.data_ptr() if need_hist else None, lut.data_ptr(), stream, work=dict(bytes=2.0 * frames.numel()))
        src = dst
    return out


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


class RandAugment:
    """``rand_augment_transform(config_str, {"interpolation": ...})``: the sections ``m`` (magnitude, default 10), ``n`` (layers,
    default 2), ``mstd`` (magnitude noise), ``inc`` (the increasing set -- whenever the section is present, whatever its digit:
    the reference tests ``bool`` of a non-empty string) and ``w`` (the weighted choice without replacement; set 0 only)."""

    def __init__(self, config_str="rand-m9-mstd0.5-inc1", interpolation="bicubic"):
        self.filter = _filter_id(interpolation)
        self.interpolation = interpolation
        config = str(config_str).split("-")
        if config[0] != "rand":
            raise NotImplementedError("RandAugment: only the 'rand' policy is restated (got %r)" % (config_str,))
        self.magnitude, self.num_layers, self.magnitude_std, self.increasing, weight_idx = MAX_LEVEL, 2, 0.0, False, None
        std_set = False
        for c in config[1:]:
            cs = re.split(r"(\d.*)", c)
            if len(cs) < 2:
                continue
            key, val = cs[:2]
            if key == "mstd":
                if not std_set:                             # hparams.setdefault: the first mstd section holds
                    self.magnitude_std, std_set = float(val), True
            elif key == "inc":
                if bool(val):
                    self.increasing = True
            elif key == "m":
                self.magnitude = int(val)
            elif key == "n":
                self.num_layers = int(val)
            elif key == "w":
                weight_idx = int(val)
        self.choice_weights = None
        if weight_idx is not None:
            if weight_idx != 0:
                raise SfError("RandAugment: only the choice weights of set 0 exist (got w%d)" % weight_idx)
            probs = list(CHOICE_WEIGHTS_0)
            self.choice_weights = probs / np.sum(probs)
        self.config_str = config_str

    # ---- the draw (host) ------------------------------------------------------------------------------------------
    def _level_arg(self, op, level):
        """The op's level function: magnitude in [0, 10] -> the argument."""
        if op in (AUTO_CONTRAST, EQUALIZE, INVERT):
            return 0.0
        if op == ROTATE:
            return _randomly_negate((level / MAX_LEVEL) * 30.0)
        if op in (SHEAR_X, SHEAR_Y):
            return _randomly_negate((level / MAX_LEVEL) * 0.3)
        if op in (TRANSLATE_X_REL, TRANSLATE_Y_REL):
            return _randomly_negate((level / MAX_LEVEL) * 0.45)
        if op == POSTERIZE:
            bits = int((level / MAX_LEVEL) * 4)
            return float(4 - bits if self.increasing else bits)
        if op == SOLARIZE:
            th = int((level / MAX_LEVEL) * 256)
            return float(256 - th if self.increasing else th)
        if op == SOLARIZE_ADD:
            return float(int((level / MAX_LEVEL) * 110))
        if self.increasing:                                 # Color, Contrast, Brightness, Sharpness
            return 1.0 + _randomly_negate((level / MAX_LEVEL) * 0.9)
        return (level / MAX_LEVEL) * 1.8 + 0.1

    def sample_params(self):
        """One clip's draw: a tuple of ``num_layers`` AugRows."""
        chosen = np.random.choice(NUM_OPS, self.num_layers, replace=self.choice_weights is None, p=self.choice_weights)
        rows = []
        for op in chosen:
            op = int(op)
            if random.random() > 0.5:
                rows.append(AugRow(op, True, 0.0))
                continue
            magnitude = self.magnitude
            if self.magnitude_std and self.magnitude_std > 0:
                magnitude = random.gauss(magnitude, self.magnitude_std)
            magnitude = min(MAX_LEVEL, max(0, magnitude))
            rows.append(AugRow(op, False, float(self._level_arg(op, magnitude))))
        return tuple(rows)

    def sample_batch(self, N):
        """The draws of clips 0 .. N-1 in that order, as a single dataset worker would make them: an AugTable."""
        rows = [self.sample_params() for _ in range(int(N))]
        if not rows:
            return AugTable(np.zeros((0, self.num_layers), np.int32), np.zeros((0, self.num_layers), bool),
                            np.zeros((0, self.num_layers)), self.filter)
        return make_table(rows, self.interpolation)

    # ---- the device side ------------------------------------------------------------------------------------------
    def __call__(self, frames, table=None, sizes=None, out=None):
        """Augments the uint8 (N, T, Hs, Ws, 3) frames; draws when no table is given."""
        spatial_sampling.check_frames(frames, "RandAugment")   # before the draw: a rejected call consumes no random numbers
        spatial_sampling.check_sizes(frames, sizes, "RandAugment")
        if table is None:
            table = self.sample_batch(frames.shape[0])
        return rand_augment_clip(frames, table, sizes, out)


def construct_rand_augment(cfg, mode):
    """The RandAugment stage of Kinetics.__init__ / __getitem__ (datasets/kinetics.py:75-80, :389-400): an object for "train"
    with AUG.ENABLE and a non-empty AUG.AA_TYPE, None otherwise.  An AA_TYPE that is no ``rand`` policy raises, as
    create_random_augment does.  A cfg without the two keys (``get_cfg()`` before a recipe is merged) stands for the
    reference's defaults."""
    aa_type = getattr(cfg.AUG, "AA_TYPE", AA_TYPE_DEFAULT)
    if mode != "train" or not cfg.AUG.ENABLE or not aa_type:
        return None
    if not str(aa_type).startswith("rand"):
        raise NotImplementedError("RandAugment: AUG.AA_TYPE %r is no 'rand' policy" % (aa_type,))
    return RandAugment(aa_type, getattr(cfg.AUG, "INTERPOLATION", INTERPOLATION_DEFAULT))
