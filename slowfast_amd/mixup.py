"""MixUp / CutMix of a training batch on the device (slowfast/datasets/mixup.py, applied at tools/train_net.py:109-111).

The reference mixes ``inputs[0]`` on the GPU with torch ops: ``x.flip(0)`` copy, ``mul_``, ``mul_``, ``add_`` -- about nine
clip-sized transfers -- and builds the soft labels with ``full`` / ``scatter_`` / ``flip`` / ``mul`` / ``add``.  ``MixUp`` here
has the same constructor and the same ``__call__`` contract; the clip is mixed by one in-place launch (csrc/sf_mixup.h: a thread
owns one element of sample i and of sample B-1-i, every byte read once and written once) and the labels by one more.

The random draw stays on the host and consumes ``np.random`` in exactly the reference's order -- ``rand()`` against
``mix_prob``; ``rand()`` against ``switch_prob`` only when both alphas are positive; one ``beta``; for cutmix ``randint``
for cy, then for cx (``rand_bbox``) and the ``correct_lam`` update -- so a loop seeded like the reference's mixes the same
samples with the same lam and the same box (pinned by tests/golden/mixup_contract.json).  ``sample_params`` exposes the draw
for loaders that mix while packing uint8 frames (``data.pack_pathways_u8(..., mix=params)``).
"""
import collections

import numpy as np
import torch

from . import ops
from .lib import SfError, get_lib

# lam: the double the reference returns (after correct_lam); use_cutmix / box (yl, yh, xl, xh) describe what happens to the
# clip.  lam == 1.0 leaves the clip alone: an unmixed draw reports (1.0, False, None), a cutmix whose clipped box came out
# empty reports that box with lam corrected to 1.0.
MixParams = collections.namedtuple("MixParams", ["lam", "use_cutmix", "box"])


def _f32_pair(lam):
    """(lam, 1 - lam) as the two fp32 factors of ``x.mul_(lam)`` / ``x.flip(0).mul_(1.0 - lam)``: the difference is taken in
    double and rounded once -- ``1.0f - (float)lam`` is a different number in the last bit for some lam."""
    lam = float(lam)
    return lam, 1.0 - lam


def _check_clip(x, out):
    if not (torch.is_tensor(x) and x.dim() == 5 and x.dtype == torch.float32 and x.is_contiguous()):
        raise SfError("MixUp: the clip must be a dense float32 (B, C, T, H, W) device tensor (got %s)" % (
            "%s %s%s" % (x.dtype, tuple(x.shape), "" if x.is_contiguous() else " non-contiguous") if torch.is_tensor(x)
            else type(x).__name__))
    if out is not None and out is not x:
        if not (torch.is_tensor(out) and out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
                and out.device == x.device):
            raise SfError("MixUp: out must be a dense float32 tensor of the clip's shape on the clip's device")
    return ops._stream(x)           # raises for a CPU tensor with the gfx950 library: there is no torch fallback


def mix_clip(x, params, out=None):
    """The clip half of ``MixUp.__call__`` for a given draw: mixes dense fp32 NCTHW ``x`` in place, or into ``out``."""
    stream = _check_clip(x, out)
    dst = x if out is None else out
    if params.lam == 1.0:
        if dst is not x and dst.data_ptr() != x.data_ptr():
            dst.copy_(x)
        return dst
    B, C, T, H, W = x.shape
    lam, oml = _f32_pair(params.lam)
    yl, yh, xl, xh = params.box if params.use_cutmix else (0, 0, 0, 0)
    get_lib().call("sf_mix_clip_f32", x.data_ptr(), dst.data_ptr(), B, C, T, H, W, int(bool(params.use_cutmix)), lam, oml,
                   int(yl), int(yh), int(xl), int(xh), stream,
                   work=dict(bytes=8.0 * (x.numel() if not params.use_cutmix or dst is not x
                                          else (B // 2) * 2 * C * T * (yh - yl) * (xh - xl))))
    return dst


class MixUp:
    """Mixup and/or cutmix of videos at batch level; constructor of slowfast/datasets/mixup.py:MixUp plus ``rng``: the source
    of the draw, the global ``np.random`` by default (as the reference) or a ``np.random.RandomState``."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, mix_prob=1.0, switch_prob=0.5, correct_lam=True, label_smoothing=0.1,
                 num_classes=1000, rng=None):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.mix_prob = mix_prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.correct_lam = correct_lam
        self.rng = np.random if rng is None else rng

    # ---- the draw (host) ------------------------------------------------------------------------------------------
    def _get_mixup_params(self):
        lam, use_cutmix, rng = 1.0, False, self.rng
        if rng.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = rng.rand() < self.switch_prob
                alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
                lam = float(rng.beta(alpha, alpha))
            elif self.mixup_alpha > 0.0:
                lam = float(rng.beta(self.mixup_alpha, self.mixup_alpha))
            elif self.cutmix_alpha > 0.0:
                use_cutmix = True
                lam = float(rng.beta(self.cutmix_alpha, self.cutmix_alpha))
        return lam, bool(use_cutmix)

    def _cutmix_bbox(self, shape, lam):
        """rand_bbox + get_cutmix_bbox (margin 0, one box)."""
        img_h, img_w = int(shape[-2]), int(shape[-1])
        ratio = np.sqrt(1 - lam)
        cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
        cy = self.rng.randint(0, img_h)
        cx = self.rng.randint(0, img_w)
        yl, yh = int(np.clip(cy - cut_h // 2, 0, img_h)), int(np.clip(cy + cut_h // 2, 0, img_h))
        xl, xh = int(np.clip(cx - cut_w // 2, 0, img_w)), int(np.clip(cx + cut_w // 2, 0, img_w))
        if self.correct_lam:
            lam = float(1.0 - ((yh - yl) * (xh - xl)) / float(img_h * img_w))
        return (yl, yh, xl, xh), lam

    def sample_params(self, shape):
        """One draw for a batch of clips of ``shape`` (only its last two dims matter): MixParams(lam, use_cutmix, box)."""
        if self.mix_prob == 0.0:
            return MixParams(1.0, False, None)          # the reference draws nothing
        if self.mix_prob < 0.0:
            raise NotImplementedError
        lam, use_cutmix = self._get_mixup_params()
        if lam == 1.0:
            return MixParams(1.0, False, None)
        if use_cutmix:
            box, lam = self._cutmix_bbox(shape, lam)
            return MixParams(lam, True, box)
        return MixParams(lam, False, None)

    # ---- the device side ------------------------------------------------------------------------------------------
    def mix_targets(self, target, lam, out=None):
        """mixup_target(target, num_classes, lam, label_smoothing): (B, K) float32 soft labels, written into ``out`` when
        given (e.g. a captured TrainStep's static labels)."""
        if not (torch.is_tensor(target) and target.dim() == 1 and target.dtype == torch.int64):
            raise SfError("MixUp: the labels must be a 1-D int64 device tensor of class indices")
        target = target.contiguous()
        B, K = int(target.shape[0]), int(self.num_classes)
        if out is None:
            out = torch.empty((B, K), dtype=torch.float32, device=target.device)
        elif not (torch.is_tensor(out) and tuple(out.shape) == (B, K) and out.dtype == torch.float32 and out.is_contiguous()
                  and out.device == target.device):
            raise SfError("MixUp: target_out must be a dense float32 (%d, %d) tensor on the labels' device" % (B, K))
        off_value = self.label_smoothing / K
        on_value = 1.0 - self.label_smoothing + off_value
        lam, oml = _f32_pair(lam)
        get_lib().call("sf_mix_targets", target.data_ptr(), B, K, on_value, off_value, lam, oml, out.data_ptr(),
                       ops._stream(target), work=dict(bytes=4.0 * B * K))
        return out

    def __call__(self, x, target, out=None, target_out=None):
        """``x, target = mixup_fn(x, target)`` of the reference: ``x`` (dense float32 NCTHW on the device) is mixed in place
        unless ``out`` is given; returns (mixed clip, (B, K) float32 soft labels)."""
        if self.mix_prob > 0.0:
            assert len(x) > 1, "Batch size should be greater than 1 for mixup."
        _check_clip(x, out)                             # before the draw: a rejected call consumes no random numbers
        params = self.sample_params(tuple(x.shape))
        x = mix_clip(x, params, out=out)
        return x, self.mix_targets(target, params.lam, out=target_out)


def construct_mixup(cfg):
    """The ``mixup_fn`` of tools/train_net.py:62-70 (None when cfg.MIXUP.ENABLE is off)."""
    if not cfg.MIXUP.ENABLE:
        return None
    return MixUp(mixup_alpha=cfg.MIXUP.ALPHA, cutmix_alpha=cfg.MIXUP.CUTMIX_ALPHA, mix_prob=cfg.MIXUP.PROB,
                 switch_prob=cfg.MIXUP.SWITCH_PROB, label_smoothing=cfg.MIXUP.LABEL_SMOOTH_VALUE,
                 num_classes=cfg.MODEL.NUM_CLASSES)
