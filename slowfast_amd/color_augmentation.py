"""Colour augmentation of an AVA training batch on the device (slowfast/datasets/transform.py ``color_jitter``,
``lighting_jitter``, ``color_normalization`` and the BGR -> RGB reordering, applied at datasets/ava_dataset.py:306-333 to the
[0, 1] clip after scale jitter, crop and flip).

The reference jitters every clip on the host in fp32.  Here the DRAW stays on the host and the arithmetic happens on the device,
in place on the dense fp32 (N, 3, T, S, S) clip that ``spatial_sampling.sample_clip(frames, table, mean=(0, 0, 0),
std=(1, 1, 1))`` writes: with that mean and std the clip is ``byte / 255.0f`` -- the reference's image after jitter, crop and
flip, channels in the frames' byte order.  That order is BGR for AVA; the grey weights and the indexing of the PCA term assume
it, as the reference does.  The arithmetic is the ``pytorch`` backend's (``AVA.IMG_PROC_BACKEND`` is not read).

The draw.  ``sample_params()`` consumes ``np.random`` in exactly the reference's order, so a loop seeded like the reference's
jitters alike (pinned by tests/golden/color_augmentation_contract.json):

* the ops whose ratio is not zero are listed in the order brightness, contrast, saturation; when the list is not empty one
  ``np.random.permutation(np.arange(len(list)))``, then for each op in the permuted order one ``np.random.uniform(-var, var)``:
  ``alpha = 1.0 + u``;
* when ``alphastd != 0`` one ``np.random.normal(0, alphastd, size=(1, 3))``; the added term is
  ``rgb = sum(eigvec * alpha * eigval, axis=1)`` with eigval / eigvec as float32 arrays, and input channel ``c`` receives
  ``rgb[2 - c]``.

The result is one ``ColorRow`` per sample; ``sample_batch`` files them in a ``ColorTable`` that travels to the device as one
buffer of 32-bit words (csrc/sf_color.h holds the layout and the arithmetic).  Contrast blends a frame with the mean of its
grey values, a reduction over the sampled frame: rows with a contrast op cost a reduction launch (``sf_color_frame_means_f32``)
in front of the streaming pass (``sf_color_clip_f32``); a recipe without contrast (PCA only, or nothing) is one launch.
"""
import collections

import numpy as np
import torch

from . import ops
from .lib import SfError, get_lib

ROW_WORDS = 16          # csrc/sf_color.h: SF_COLOR_ROW_WORDS
BRIGHTNESS, CONTRAST, SATURATION, NONE = 0, 1, 2, -1

# order: the op codes in application order (three slots, NONE where fewer ops run); alpha: the blend factor of every slot as the
# host's double (1.0 for an empty slot); add: what input channel 0, 1, 2 receives, as doubles (zeros without lighting)
ColorRow = collections.namedtuple("ColorRow", ["order", "alpha", "add"])
# words: int32 (N, 16), sample n in row n, the floats as their bits (layout: csrc/sf_color.h)
ColorTable = collections.namedtuple("ColorTable", ["words"])

_scratch = {}           # (device, N, T, HW) -> (partials, means)


def _row_words(row):
    order, alpha, add = row
    order = [int(v) for v in order] + [NONE] * (3 - len(order))
    alpha = [float(v) for v in alpha] + [1.0] * (3 - len(alpha))
    if len(order) != 3 or len(alpha) != 3 or len(add) != 3:
        raise SfError("ColorAugmentation: a row is (up to three op codes, as many alphas, three additions)")
    w = np.zeros(ROW_WORDS, dtype=np.int32)
    f = w.view(np.float32)
    w[0:3] = order
    for s in range(3):                                      # alpha and 1 - alpha: the difference in double, each rounded once
        f[4 + 2 * s] = np.float32(alpha[s])
        f[5 + 2 * s] = np.float32(1.0 - alpha[s])
    f[10:13] = [np.float32(float(v)) for v in add]
    return w


def make_table(rows):
    """An explicit ColorTable from N ColorRow-like (order, alpha, add) tuples."""
    rows = list(rows)
    return ColorTable(np.stack([_row_words(r) for r in rows]) if rows else np.zeros((0, ROW_WORDS), dtype=np.int32))


def _check_rows(words, N):
    """The host copy, row by row, before any launch (the library checks it again)."""
    words = np.asarray(words)
    if words.dtype != np.int32 or words.ndim != 2 or words.shape[1] != ROW_WORDS:
        raise SfError("ColorAugmentation: a colour table is int32 (N, %d) words" % ROW_WORDS)
    if len(words) != N:
        raise SfError("ColorAugmentation: the colour table was drawn for %d samples, the batch has %d" % (len(words), N))
    floats = words.view(np.float32)
    for n in range(N):
        ops_ = [int(v) for v in words[n, 0:3]]
        if any(v < -1 or v > 2 for v in ops_):
            raise SfError("ColorAugmentation: colour row %d: ops %s are not all of -1, 0, 1, 2" % (n, ops_))
        used = [v for v in ops_ if v >= 0]
        if len(set(used)) != len(used):
            raise SfError("ColorAugmentation: colour row %d: an op appears twice in %s" % (n, ops_))
        if not np.all(np.isfinite(floats[n, 4:13])):
            raise SfError("ColorAugmentation: colour row %d holds a float that is not finite" % n)
    return np.ascontiguousarray(words.reshape(-1))


def upload_table(table, N, device):
    """(host words, device words) of a table for a batch of N: one small host-to-device copy."""
    host = _check_rows(table.words, N)
    return host, torch.from_numpy(host).to(device)


def check_clip(clip, who="ColorAugmentation"):
    """The dense fp32 (N, 3, T, H, W) clip; returns the stream (raises for a CPU tensor with the gfx950 library)."""
    if not (torch.is_tensor(clip) and clip.dim() == 5 and clip.dtype == torch.float32 and clip.shape[1] == 3
            and clip.is_contiguous()):
        raise SfError("%s: the clip must be a dense float32 (N, 3, T, H, W) device tensor (got %s)" % (
            who, "%s %s%s" % (clip.dtype, tuple(clip.shape), "" if clip.is_contiguous() else " non-contiguous")
            if torch.is_tensor(clip) else type(clip).__name__))
    return ops._stream(clip)


def _scratch_for(clip, chunks):
    N, _, T, H, W = clip.shape
    key = (clip.device, N, T, H * W)
    if key not in _scratch:
        _scratch[key] = (torch.empty((N * T, chunks), dtype=torch.float32, device=clip.device),
                         torch.empty((N * T,), dtype=torch.float32, device=clip.device))
    return _scratch[key]


def frame_means(clip, table, means=None):
    """The per-frame grey means contrast blends with, for the frames of every sample whose row has a contrast op: a float32
    (N * T,) tensor (``means``: the tensor to write into; entries of the other samples are left as they are).  Returns None
    and launches nothing when no row has one."""
    stream = check_clip(clip)
    N, _, T, H, W = clip.shape
    host, dev = upload_table(table, N, clip.device)
    return _frame_means(clip, host, dev, stream, means)


def _frame_means(clip, host, dev, stream, means=None):
    N, _, T, H, W = clip.shape
    if not np.any(host.reshape(N, ROW_WORDS)[:, 0:3] == CONTRAST):
        return None
    lib = get_lib()
    partials, cached = _scratch_for(clip, lib.call("sf_color_chunks", H * W))
    means = cached if means is None else means
    if not (torch.is_tensor(means) and means.dtype == torch.float32 and means.numel() == N * T and means.is_contiguous()
            and means.device == clip.device):
        raise SfError("ColorAugmentation: means must be a dense float32 tensor of N * T = %d elements on the clip's device" % (N * T))
    lib.call("sf_color_frame_means_f32", clip.data_ptr(), N, T, H * W, host.ctypes.data, dev.data_ptr(), partials.data_ptr(),
             means.data_ptr(), stream, work=dict(bytes=4.0 * clip.numel() + 4.0 * partials.numel()))
    return means


def color_clip(clip, table, mean, std, reverse=True):
    """Applies ``table`` to the dense fp32 (N, 3, T, S, S) clip in place: the jitter ops of every row in its order, the
    lighting term, ``(v - mean[c]) / std[c]`` with mean / std indexed by INPUT channel, and -- ``reverse`` -- the channel
    reordering [2, 1, 0].  One launch, two when a row has a contrast op.  Returns ``clip``."""
    stream = check_clip(clip)
    N, _, T, H, W = clip.shape
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise SfError("ColorAugmentation: mean and std have three entries")
    host, dev = upload_table(table, N, clip.device)
    means = _frame_means(clip, host, dev, stream)
    get_lib().call("sf_color_clip_f32", clip.data_ptr(), N, T, H * W, host.ctypes.data, dev.data_ptr(),
                   None if means is None else means.data_ptr(), mean[0], mean[1], mean[2], std[0], std[1], std[2],
                   int(bool(reverse)), stream, work=dict(bytes=8.0 * clip.numel()))
    return clip


class ColorAugmentation:
    """The arguments of transform.color_jitter / lighting_jitter / color_normalization and the final channel reversal."""

    def __init__(self, brightness=0.4, contrast=0.4, saturation=0.4, alphastd=0.1, eigval=(0.225, 0.224, 0.229),
                 eigvec=((-0.5675, 0.7192, 0.4009), (-0.5808, -0.0045, -0.8140), (-0.5836, -0.6948, 0.4203)),
                 mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), reverse=True):
        self.brightness, self.contrast, self.saturation = float(brightness), float(contrast), float(saturation)
        self.alphastd = alphastd
        self.eigval = np.array(eigval).astype(np.float32)
        self.eigvec = np.array(eigvec).astype(np.float32)
        if self.eigval.shape != (3,) or self.eigvec.shape != (3, 3):
            raise SfError("ColorAugmentation: eigval has 3 entries and eigvec 3 x 3")
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        if len(self.mean) != 3 or len(self.std) != 3 or any(v == 0.0 for v in self.std):
            raise SfError("ColorAugmentation: mean and std have three entries and no std is zero")
        self.reverse = bool(reverse)

    # ---- the draw (host) ------------------------------------------------------------------------------------------
    def sample_params(self):
        """One clip's draw: a ColorRow."""
        ratios = [(code, var) for code, var in ((BRIGHTNESS, self.brightness), (CONTRAST, self.contrast),
                                                (SATURATION, self.saturation)) if var != 0]
        order, alpha = [], []
        if ratios:
            for i in np.random.permutation(np.arange(len(ratios))):
                code, var = ratios[int(i)]
                order.append(code)
                alpha.append(1.0 + np.random.uniform(-var, var))
        add = (0.0, 0.0, 0.0)
        if self.alphastd != 0:
            a = np.random.normal(0, self.alphastd, size=(1, 3))
            rgb = np.sum(self.eigvec * a * self.eigval.reshape(1, 3), axis=1)
            add = tuple(float(rgb[2 - c]) for c in range(3))
        return ColorRow(tuple(order + [NONE] * (3 - len(order))), tuple(alpha + [1.0] * (3 - len(alpha))), add)

    def sample_batch(self, N):
        """The draws of clips 0 .. N-1 in that order, as a single dataset worker would make them: a ColorTable."""
        return make_table([self.sample_params() for _ in range(int(N))])

    # ---- the device side ------------------------------------------------------------------------------------------
    def __call__(self, clip, table=None):
        """Jitters, normalises and reorders the dense fp32 (N, 3, T, S, S) clip in place; draws when no table is given."""
        check_clip(clip)                                    # before the draw: a rejected call consumes no random numbers
        if table is None:
            table = self.sample_batch(clip.shape[0])
        else:
            _check_rows(table.words, clip.shape[0])
        return color_clip(clip, table, self.mean, self.std, self.reverse)


def construct_color_augmentation(cfg, split):
    """The colour stage of Ava.__init__ / Ava._images_and_boxes_preprocessing (datasets/ava_dataset.py:34-48, :306-333) for
    ``split``: jitter only for "train" with AVA.TRAIN_USE_COLOR_AUGMENTATION, lighting alone with AVA.TRAIN_PCA_JITTER_ONLY.
    Always returns an object: with nothing switched on it only normalises and reorders channels, and draws nothing."""
    jitter = split == "train" and cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION
    ratio = 0.4 if jitter and not cfg.AVA.TRAIN_PCA_JITTER_ONLY else 0.0
    return ColorAugmentation(brightness=ratio, contrast=ratio, saturation=ratio, alphastd=0.1 if jitter else 0.0,
                             eigval=cfg.DATA.TRAIN_PCA_EIGVAL, eigvec=cfg.DATA.TRAIN_PCA_EIGVEC, mean=cfg.DATA.MEAN,
                             std=cfg.DATA.STD, reverse=not cfg.AVA.BGR)
