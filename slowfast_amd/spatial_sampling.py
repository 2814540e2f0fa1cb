"""Spatial sampling of a training batch on the device (slowfast/datasets/utils.py:114-185 ``spatial_sampling``, applied at
datasets/kinetics.py:410-435 to the normalised fp32 clip between ``tensor_normalize`` and ``RandomErasing``).

The reference resizes every frame of every clip on the host with a bilinear ``F.interpolate`` in fp32, then crops and flips.
Here the DRAW stays on the host and the resize, crop and flip happen on the device, straight from the decoded uint8 frames:
``sample_clip`` writes the dense fp32 clip that ``erase_clip`` / ``mix_clip`` take in place, and
``data.pack_pathways_u8(..., crop=table)`` samples, erases and mixes while it packs.

The draw.  ``sample_params(height, width)`` consumes ``np.random`` and Python's ``random`` in exactly the reference's order,
so a loop seeded like the reference's takes the same boxes (pinned by tests/golden/spatial_sampling_contract.json):

* jitter (``aspect_ratio is None and scale is None``): one ``np.random.uniform(min_scale, max_scale)`` (with
  ``inverse_uniform_sampling`` ``uniform(1 / max, 1 / min)`` and a reciprocal), ``int(round(.))``; the new size by
  ``random_short_side_scale_jitter``'s floor arithmetic, unchanged when the short side already has that size; then
  ``np.random.randint(0, h - S)`` only when ``h > S`` and ``np.random.randint(0, w - S)`` only when ``w > S``, neither when the
  resized frame is already S x S; then ``np.random.uniform()`` for the flip only when ``random_horizontal_flip``.
* resized crop, up to 10 attempts: ``random.uniform(*scale)``, ``random.uniform`` of the log ratio, one ``np.random.uniform()``
  (the reference evaluates it before ``and switch_hw``, so it is always consumed), on success ``random.randint`` twice;
  otherwise the reference's central fallback; then the flip draw.
* test (``spatial_idx`` 0, 1, 2): the ``np.random.uniform(s, s)`` of the jitter call is still consumed; ``uniform_crop``'s
  offsets are ``ceil((len - S) / 2)``, index 0 / 2 move the crop to the ends of the long axis (``height > width`` decides).

The result is one ``CropRow`` per sample; ``sample_batch`` files them in a ``CropTable`` that travels to the device as one int32
buffer (csrc/sf_sample.h holds the coordinate rule the kernels apply to it).  A resized frame that would be smaller than the
crop raises ``SfError`` before any draw (the reference would return a clip that is not S x S).  ``motion_shift`` and multigrid
crop sizes are not supported.
"""
import collections
import math
import random

import numpy as np
import torch

from . import ops
from .lib import SfError, get_lib

ROW_WORDS = 12          # csrc/sf_sample.h: SF_CROP_ROW_WORDS

# src_h, src_w: valid size of the sample's frames; win_*: the source window that is resized (the whole frame on the jitter and
# test paths, (i, j, h, w) on the resized-crop path); res_h, res_w: the size it is resized to; off_y, off_x: the crop offset in
# the resized image (0, 0 on the resized-crop path); flip: 0 / 1
CropRow = collections.namedtuple("CropRow", ["src_h", "src_w", "win_y", "win_x", "win_h", "win_w", "res_h", "res_w", "off_y",
                                             "off_x", "flip"])
# rows: int32 (N, 11), sample n in row n; crop_size: S
CropTable = collections.namedtuple("CropTable", ["rows", "crop_size"])


def make_table(rows, crop_size):
    """An explicit CropTable from N CropRow-like tuples."""
    return CropTable(np.asarray(rows, dtype=np.int32).reshape(-1, len(CropRow._fields)), int(crop_size))


def _pack_table(table, N):
    """CropTable -> the int32 words of csrc/sf_sample.h; the rows themselves are checked by the library."""
    if len(table.rows) != N:
        raise SfError("SpatialSampling: the crop table was drawn for %d samples, the batch has %d" % (len(table.rows), N))
    words = np.zeros((N, ROW_WORDS), dtype=np.int32)
    words[:, :len(CropRow._fields)] = table.rows
    return np.ascontiguousarray(words.reshape(-1))


def upload_table(table, N, device):
    """(host words, device words) of a table for a batch of N: one small host-to-device copy."""
    host = _pack_table(table, N)
    return host, torch.from_numpy(host).to(device)


def check_frames(frames, who="SpatialSampling"):
    """The uint8 (N, T, Hs, Ws, 3) source buffer; returns the stream (raises for a CPU tensor with the gfx950 library)."""
    if not (torch.is_tensor(frames) and frames.dim() == 5 and frames.dtype == torch.uint8 and frames.shape[-1] == 3
            and frames.is_contiguous()):
        raise SfError("%s: the frames must be a dense uint8 (N, T, H, W, 3) device tensor (got %s)" % (
            who, "%s %s%s" % (frames.dtype, tuple(frames.shape), "" if frames.is_contiguous() else " non-contiguous")
            if torch.is_tensor(frames) else type(frames).__name__))
    return ops._stream(frames)


# ---- what the uint8 passes over the frame buffer share (rand_augment, ssl_color) ----------------------------------------------
def check_sizes(frames, sizes, who):
    """``sizes[n] = (h, w)``: the valid frame size of sample n inside the (N, T, Hs, Ws, 3) buffer; None: the whole buffer."""
    N, _, Hs, Ws, _ = frames.shape
    if sizes is None:
        return [(Hs, Ws)] * N
    sizes = [(int(s[0]), int(s[1])) for s in sizes]
    if len(sizes) != N:
        raise SfError("%s: sizes has %d entries, the batch has %d samples" % (who, len(sizes), N))
    for n, (h, w) in enumerate(sizes):
        if not (0 < h <= Hs and 0 < w <= Ws):
            raise SfError("%s: sample %d: valid size %d x %d is not inside the %d x %d buffer" % (who, n, h, w, Hs, Ws))
    return sizes


def check_out(frames, out, who, in_place=False):
    """``out`` of a pass over ``frames``: None, another dense uint8 tensor of their shape, or -- where the pass can work
    ``in_place`` -- the frames themselves or a tensor that does not overlap them."""
    if out is None or (in_place and out is frames):
        return
    ok = (torch.is_tensor(out) and out.shape == frames.shape and out.dtype == torch.uint8 and out.is_contiguous()
          and out.device == frames.device and (in_place or out.data_ptr() != frames.data_ptr()))
    if not ok:
        raise SfError("%s: out must be %s dense uint8 %s tensor on the frames' device" % (
            who, "a" if in_place else "another", tuple(frames.shape)))
    a, b, nbytes = frames.data_ptr(), out.data_ptr(), frames.numel()
    if in_place and a < b + nbytes and b < a + nbytes:
        raise SfError("%s: out must be the frames tensor itself (in place) or must not overlap it" % who)


_scratch = {}           # (who, device, N, T, Hs, Ws) -> (a buffer like the frames, the pass's tables)


def frame_scratch(frames, who, *tables):
    """A second buffer like ``frames`` and one tensor per (shape, dtype) of ``tables``, uninitialised; allocated on the first
    call for a (device, N, T, Hs, Ws) and kept: no allocation afterwards."""
    key = (who, frames.device) + tuple(frames.shape[:4])
    if key not in _scratch:
        _scratch[key] = (torch.empty_like(frames),) + tuple(torch.empty(shape, dtype=dtype, device=frames.device)
                                                            for shape, dtype in tables)
    return _scratch[key]


def sample_clip(frames, table, mean, std, out=None):
    """uint8 (N, T, Hs, Ws, 3) frames (every sample padded to the batch's largest frame) -> the normalised, resized, cropped and
    flipped dense fp32 (N, 3, T, S, S) clip of ``table``, channels in ``mean`` order: one launch.  ``out``: a tensor of that
    shape to write into."""
    stream = check_frames(frames)
    N, T, Hs, Ws, _ = frames.shape
    S = int(table.crop_size)
    if out is None:
        out = torch.empty((N, 3, T, S, S), dtype=torch.float32, device=frames.device)
    elif not (torch.is_tensor(out) and tuple(out.shape) == (N, 3, T, S, S) and out.dtype == torch.float32 and out.is_contiguous()
              and out.device == frames.device):
        raise SfError("SpatialSampling: out must be a dense float32 (N, 3, T, S, S) = %s tensor on the frames' device" % (
            (N, 3, T, S, S),))
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    host, dev = upload_table(table, N, frames.device)
    get_lib().call("sf_sample_clip_u8", frames.data_ptr(), N, T, Hs, Ws, host.ctypes.data, dev.data_ptr(), S, mean[0], mean[1],
                   mean[2], std[0], std[1], std[2], out.data_ptr(), stream,
                   work=dict(bytes=3.0 * N * T * Hs * Ws + 4.0 * out.numel()))
    return out


class SpatialSampling:
    """The arguments of slowfast/datasets/utils.py:spatial_sampling without ``frames``."""

    def __init__(self, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224, random_horizontal_flip=True,
                 inverse_uniform_sampling=False, aspect_ratio=None, scale=None, motion_shift=False, force_flip=False):
        if motion_shift:
            raise NotImplementedError("SpatialSampling: motion_shift (per-frame boxes) is not supported")
        if spatial_idx not in (-1, 0, 1, 2):
            raise SfError("SpatialSampling: spatial_idx must be -1, 0, 1 or 2 (got %r)" % (spatial_idx,))
        if (aspect_ratio is None) != (scale is None):
            raise SfError("SpatialSampling: the resized-crop path needs both aspect_ratio and scale")
        if int(crop_size) <= 0:
            raise SfError("SpatialSampling: crop_size must be positive")
        self.spatial_idx = spatial_idx
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.crop_size = int(crop_size)
        self.random_horizontal_flip = random_horizontal_flip
        self.inverse_uniform_sampling = inverse_uniform_sampling
        self.aspect_ratio = None if aspect_ratio is None else tuple(aspect_ratio)
        self.scale = None if scale is None else tuple(scale)
        self.motion_shift = False
        # AVA.TEST_FORCE_FLIP (construct_ava_sampling): every row of the test path flips.  The reference's
        # horizontal_flip(1, ...) still compares one np.random.uniform() with 1, so one is consumed here too.
        self.force_flip = bool(force_flip)

    # ---- the draw (host) ------------------------------------------------------------------------------------------
    @staticmethod
    def _jitter_size(height, width, size):
        """random_short_side_scale_jitter after its draw: the size the frame is resized to."""
        if (width <= height and width == size) or (height <= width and height == size):
            return height, width
        if width < height:
            return int(math.floor((float(height) / width) * size)), size
        return size, int(math.floor((float(width) / height) * size))

    def _resized_crop_window(self, height, width):
        """_get_param_spatial_crop(scale, ratio, height, width): (i, j, h, w)."""
        scale, ratio = self.scale, self.aspect_ratio
        for _ in range(10):
            area = height * width
            target_area = random.uniform(*scale) * area
            log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
            aspect = math.exp(random.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            np.random.uniform()                             # the reference's `np.random.uniform() < 0.5 and switch_hw`
            if 0 < w <= width and 0 < h <= height:
                i = random.randint(0, height - h)
                j = random.randint(0, width - w)
                return i, j, h, w
        in_ratio = float(width) / float(height)             # the central fallback
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def _draw(self, height, width, idx):
        S = self.crop_size
        if idx == -1 and self.scale is not None:
            i, j, h, w = self._resized_crop_window(height, width)
            if not (0 < h and 0 < w and 0 <= i and 0 <= j and i + h <= height and j + w <= width):
                raise SfError("SpatialSampling: the central fallback window (%d, %d, %d, %d) does not fit the %d x %d frame"
                              % (i, j, h, w, height, width))
            flip = int(np.random.uniform() < 0.5) if self.random_horizontal_flip else 0
            return CropRow(height, width, i, j, h, w, S, S, 0, 0, flip)
        if idx == -1 and self.inverse_uniform_sampling:
            size = int(round(1.0 / np.random.uniform(1.0 / self.max_scale, 1.0 / self.min_scale)))
        else:                                               # the test path calls the jitter without inverse sampling
            size = int(round(np.random.uniform(self.min_scale, self.max_scale)))
        rh, rw = self._jitter_size(height, width, size)
        if rh < S or rw < S:
            raise SfError("SpatialSampling: the frame resized to %d x %d is smaller than the crop %d" % (rh, rw, S))
        if idx == -1:                                       # random_crop
            oy = ox = 0
            if not (rh == S and rw == S):
                if rh > S:
                    oy = int(np.random.randint(0, rh - S))
                if rw > S:
                    ox = int(np.random.randint(0, rw - S))
            flip = int(np.random.uniform() < 0.5) if self.random_horizontal_flip else 0
        else:                                               # uniform_crop
            oy = int(math.ceil((rh - S) / 2))
            ox = int(math.ceil((rw - S) / 2))
            if rh > rw:
                oy = 0 if idx == 0 else (rh - S if idx == 2 else oy)
            else:
                ox = 0 if idx == 0 else (rw - S if idx == 2 else ox)
            flip = 0
            if self.force_flip:
                np.random.uniform()
                flip = 1
        return CropRow(height, width, 0, 0, height, width, rh, rw, oy, ox, flip)

    def _check(self, height, width, idx):
        """What can be rejected before the first draw."""
        if idx not in (-1, 0, 1, 2):
            raise SfError("SpatialSampling: spatial_idx must be -1, 0, 1 or 2 (got %r)" % (idx,))
        if not (int(height) == height and int(width) == width and height > 0 and width > 0):
            raise SfError("SpatialSampling: bad frame size %r x %r" % (height, width))
        if idx != -1 and self.min_scale != self.max_scale:
            raise SfError("SpatialSampling: the test path needs min_scale == max_scale")
        if idx != -1 or self.scale is None:
            # the short side becomes the drawn size (>= round(min_scale)) and the long side is never shorter
            if int(round(self.min_scale)) < self.crop_size:
                raise SfError("SpatialSampling: a frame resized to a short side of %d is smaller than the crop %d" % (
                    int(round(self.min_scale)), self.crop_size))

    def sample_params(self, height, width, spatial_idx=None):
        """One clip's draw for frames of ``height`` x ``width``: a CropRow.  ``spatial_idx`` overrides the constructor's (the
        test loader's per-item index)."""
        idx = self.spatial_idx if spatial_idx is None else spatial_idx
        self._check(height, width, idx)
        state = (random.getstate(), np.random.get_state())
        try:
            return self._draw(int(height), int(width), idx)
        except SfError:                                     # a rejected draw consumes no random number
            random.setstate(state[0])
            np.random.set_state(state[1])
            raise

    def sample_batch(self, sizes, spatial_idx=None):
        """The draws of clips 0 .. N-1 in that order, as a single dataset worker would make them, for ``sizes`` = N (height,
        width) pairs: a CropTable.  ``spatial_idx``: one index for all, or one per sample."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        idx = list(spatial_idx) if isinstance(spatial_idx, (list, tuple)) else [spatial_idx] * len(sizes)
        if len(idx) != len(sizes):
            raise SfError("SpatialSampling: %d spatial indices for %d samples" % (len(idx), len(sizes)))
        for (h, w), i in zip(sizes, idx):
            self._check(h, w, self.spatial_idx if i is None else i)
        state = (random.getstate(), np.random.get_state())
        try:
            return make_table([self.sample_params(h, w, i) for (h, w), i in zip(sizes, idx)], self.crop_size)
        except SfError:
            random.setstate(state[0])
            np.random.set_state(state[1])
            raise

    # ---- the device side ------------------------------------------------------------------------------------------
    def __call__(self, frames, mean, std, sizes=None, out=None):
        """Samples the uint8 (N, T, Hs, Ws, 3) device batch into the dense fp32 (N, 3, T, S, S) clip: every clip drawn in order
        (``sizes``: the valid (height, width) of every sample, default the whole buffer), one table upload, one launch."""
        check_frames(frames)                                # before the draw: a rejected call consumes no random numbers
        N, T, Hs, Ws, _ = frames.shape
        return sample_clip(frames, self.sample_batch([(Hs, Ws)] * N if sizes is None else sizes), mean, std, out=out)


def construct_spatial_sampling(cfg, mode):
    """The ``spatial_sampling`` arguments of datasets/kinetics.py:197-237 and :410-434 for ``mode`` "train", "val" or "test".
    In test mode the loader passes its per-item index ``idx % TEST.NUM_SPATIAL_CROPS`` to ``sample_params``; the constructed
    default is the centre crop (what NUM_SPATIAL_CROPS 1 uses)."""
    if cfg.MULTIGRID.get("DEFAULT_S", 0) > 0:
        raise SfError("construct_spatial_sampling: multigrid crop sizes (MULTIGRID.DEFAULT_S > 0) are not supported")
    if mode in ("train", "val"):
        spatial_idx = -1
        min_scale, max_scale = cfg.DATA.TRAIN_JITTER_SCALES[0], cfg.DATA.TRAIN_JITTER_SCALES[1]
        crop_size = cfg.DATA.TRAIN_CROP_SIZE
    elif mode == "test":
        spatial_idx = 1
        if cfg.TEST.NUM_SPATIAL_CROPS > 1:
            min_scale = max_scale = crop_size = cfg.DATA.TEST_CROP_SIZE
        else:
            min_scale = max_scale = cfg.DATA.TRAIN_JITTER_SCALES[0]
            crop_size = cfg.DATA.TEST_CROP_SIZE
    else:
        raise NotImplementedError("Does not support {} mode".format(mode))
    scl, asp = cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE
    return SpatialSampling(
        spatial_idx=spatial_idx, min_scale=min_scale, max_scale=max_scale, crop_size=crop_size,
        random_horizontal_flip=cfg.DATA.RANDOM_FLIP, inverse_uniform_sampling=cfg.DATA.INV_UNIFORM_SAMPLE,
        aspect_ratio=None if (mode != "train" or len(asp) == 0) else asp,
        scale=None if (mode != "train" or len(scl) == 0) else scl,
        motion_shift=cfg.DATA.TRAIN_JITTER_MOTION_SHIFT if mode == "train" else False)


# ---- AVA: the boxes follow the crop ---------------------------------------------------------------------------------------
def _clip_boxes(boxes, height, width):
    out = boxes.copy()
    out[:, [0, 2]] = np.minimum(width - 1.0, np.maximum(0.0, boxes[:, [0, 2]]))
    out[:, [1, 3]] = np.minimum(height - 1.0, np.maximum(0.0, boxes[:, [1, 3]]))
    return out


def transform_boxes(row, boxes, crop_size):
    """The boxes of a clip carried through its ``CropRow`` as Ava._images_and_boxes_preprocessing carries them
    (datasets/ava_dataset.py:255-302, :335): ``boxes`` is a (K, 4) array of [x1, y1, x2, y2] in [0, 1]; they are scaled to the
    source frame and clipped to it, scaled with the short-side resize (skipped when the row resizes nothing), moved by the
    crop offset, mirrored when the row flips and clipped to the crop.  numpy, in the reference's operations and order: float64
    boxes come out bit for bit.  The input is not modified."""
    r = CropRow(*[int(v) for v in row])
    S = int(crop_size)
    if (r.win_y, r.win_x, r.win_h, r.win_w) != (0, 0, r.src_h, r.src_w):
        raise SfError("transform_boxes: the row must resize the whole frame (the jitter and test paths), not a window of it")
    boxes = np.array(boxes, copy=True)
    if boxes.ndim != 2 or boxes.shape[1] != 4 or not np.issubdtype(boxes.dtype, np.floating):
        raise SfError("transform_boxes: boxes must be a floating (K, 4) array of [x1, y1, x2, y2]")
    boxes[:, [0, 2]] *= r.src_w
    boxes[:, [1, 3]] *= r.src_h
    boxes = _clip_boxes(boxes, r.src_h, r.src_w)
    if (r.res_h, r.res_w) != (r.src_h, r.src_w):
        if r.src_w < r.src_h:
            boxes = boxes * float(r.res_h) / r.src_h
        else:
            boxes = boxes * float(r.res_w) / r.src_w
    moved = boxes.copy()
    moved[:, [0, 2]] = boxes[:, [0, 2]] - r.off_x
    moved[:, [1, 3]] = boxes[:, [1, 3]] - r.off_y
    boxes = moved
    if r.flip:
        flipped = boxes.copy()
        flipped[:, [0, 2]] = S - boxes[:, [2, 0]] - 1
        boxes = flipped
    return _clip_boxes(boxes, S, S)


def collate_boxes(list_of_boxes):
    """The (R, 5) float32 tensor [batch index, x1, y1, x2, y2] that loader.detection_collate builds from every sample's (K_n, 4)
    boxes: the ``bboxes`` input of ResNetRoIHead.  A sample without boxes contributes no row."""
    rows = []
    for n, boxes in enumerate(list_of_boxes):
        boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        rows.append(np.concatenate([np.full((boxes.shape[0], 1), float(n)), boxes], axis=1))
    out = np.concatenate(rows, axis=0) if rows else np.zeros((0, 5))
    return torch.tensor(out).float()


def construct_ava_sampling(cfg, split):
    """The crop arguments of Ava.__init__ / Ava._images_and_boxes_preprocessing (datasets/ava_dataset.py:37-48, :262-290):
    "train" jitters at DATA.TRAIN_JITTER_SCALES, crops TRAIN_CROP_SIZE at random and draws the flip; "val" resizes the short
    side to TEST_CROP_SIZE and takes the centre crop, with AVA.TEST_FORCE_FLIP every row flips (the reference's
    horizontal_flip(1, ...) consumes one np.random.uniform() whose value cannot matter; so does the draw here).
    "test" is not cropped by the reference (the clip is not square) and is not supported; neither is
    DATA.TRAIN_JITTER_MOTION_SHIFT."""
    if split == "train":
        return SpatialSampling(spatial_idx=-1, min_scale=cfg.DATA.TRAIN_JITTER_SCALES[0], max_scale=cfg.DATA.TRAIN_JITTER_SCALES[1],
                               crop_size=cfg.DATA.TRAIN_CROP_SIZE, random_horizontal_flip=True)
    if split == "val":
        S = cfg.DATA.TEST_CROP_SIZE
        return SpatialSampling(spatial_idx=1, min_scale=S, max_scale=S, crop_size=S, random_horizontal_flip=False,
                               force_flip=bool(cfg.AVA.TEST_FORCE_FLIP))
    raise NotImplementedError("construct_ava_sampling: the {} split is not supported".format(split))
