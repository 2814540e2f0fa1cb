"""Mask tables of masked-feature pre-training, drawn on the host (slowfast/datasets/transform.py:776-945,
slowfast/datasets/kinetics.py:470-504).

The loader of the reference draws one mask per clip with Python's global ``random``: cube masks (``MaskingGenerator3D``, the
default), a 2-D block mask tiled over 8 frames (``AUG.MASK_TUBE``, ``MaskingGenerator``; its window is the two spatial sizes)
or whole frames (``AUG.MASK_FRAMES``, one ``random.sample``).  The generators here consume ``random`` in exactly the same
order, so a loop seeded like the reference's masks the same windows.  ``sample_batch(N)`` stacks N draws into the uint8
``(N, Tw, Hw, Ww)`` table the model takes as ``inputs[2]`` (masked.MaskMViT): one small host tensor per step.
"""
import math
import random

import numpy as np
import torch


# slowfast/config/defaults.py:210-226 -- the reference's defaults of the AUG mask keys, which stand in for a cfg that does not
# carry them (config.get_cfg() keeps the AUG section to the keys of the augmentations; the MaskFeat preset sets these)
AUG_MASK_DEFAULTS = {"GEN_MASK_LOADER": False, "MASK_TUBE": False, "MASK_FRAMES": False, "MASK_WINDOW_SIZE": [8, 7, 7],
                     "MASK_RATIO": 0.0, "MAX_MASK_PATCHES_PER_BLOCK": None}


def _aug(cfg, key):
    return getattr(cfg.AUG, key, AUG_MASK_DEFAULTS[key])


class MaskingGenerator:
    """2-D block masks (transform.py:776-859)."""

    def __init__(self, mask_window_size, num_masking_patches, min_num_patches=16, max_num_patches=None, min_aspect=0.3,
                 max_aspect=None):
        if not isinstance(mask_window_size, (list, tuple)):
            mask_window_size = (mask_window_size,) * 2
        self.height, self.width = mask_window_size
        self.num_patches = self.height * self.width
        self.num_masking_patches = num_masking_patches
        self.min_num_patches = min_num_patches
        self.max_num_patches = num_masking_patches if max_num_patches is None else max_num_patches
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))

    def get_shape(self):
        return self.height, self.width

    def _mask(self, mask, max_mask_patches):
        delta = 0
        for _ in range(10):
            target_area = random.uniform(self.min_num_patches, max_mask_patches)
            aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < self.width and h < self.height:
                top = random.randint(0, self.height - h)
                left = random.randint(0, self.width - w)
                box = mask[top:top + h, left:left + w]
                if 0 < h * w - box.sum() <= max_mask_patches:
                    delta += int((box == 0).sum())
                    box[...] = 1
                if delta > 0:
                    break
        return delta

    def __call__(self):
        mask = np.zeros(shape=self.get_shape(), dtype=int)
        mask_count = 0
        while mask_count < self.num_masking_patches:
            max_mask_patches = min(self.num_masking_patches - mask_count, self.max_num_patches)
            delta = self._mask(mask, max_mask_patches)
            if delta == 0:
                break
            mask_count += delta
        return mask


class MaskingGenerator3D:
    """Cube masks (transform.py:869-945)."""

    def __init__(self, mask_window_size, num_masking_patches, min_num_patches=16, max_num_patches=None, min_aspect=0.3,
                 max_aspect=None):
        self.temporal, self.height, self.width = mask_window_size
        self.num_masking_patches = num_masking_patches
        self.min_num_patches = min_num_patches
        self.max_num_patches = num_masking_patches if max_num_patches is None else max_num_patches
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))

    def get_shape(self):
        return self.temporal, self.height, self.width

    def _mask(self, mask, max_mask_patches):
        delta = 0
        for _ in range(100):
            target_area = random.uniform(self.min_num_patches, self.max_num_patches)
            aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            t = random.randint(1, self.temporal)
            if w < self.width and h < self.height:
                top = random.randint(0, self.height - h)
                left = random.randint(0, self.width - w)
                front = random.randint(0, self.temporal - t)
                box = mask[front:front + t, top:top + h, left:left + w]
                if 0 < h * w * t - box.sum() <= max_mask_patches:
                    delta += int((box == 0).sum())
                    box[...] = 1
                if delta > 0:
                    break
        return delta

    def __call__(self):
        mask = np.zeros(shape=self.get_shape(), dtype=int)
        mask_count = 0
        while mask_count < self.num_masking_patches:
            delta = self._mask(mask, self.num_masking_patches - mask_count)
            if delta == 0:
                break
            mask_count += delta
        return mask


class MaskSampler:
    """``Kinetics._gen_mask`` for a cfg: ``sampler()`` is one clip's int mask, ``sample_batch(N)`` the step's table."""

    def __init__(self, cfg):
        self.window = list(_aug(cfg, "MASK_WINDOW_SIZE"))
        self.ratio = _aug(cfg, "MASK_RATIO")
        self.mode = "tube" if _aug(cfg, "MASK_TUBE") else ("frames" if _aug(cfg, "MASK_FRAMES") else "cube")
        self.generator = None
        if self.mode == "tube":
            n = round(np.prod(self.window) * self.ratio)
            self.generator = MaskingGenerator(mask_window_size=self.window, num_masking_patches=n, max_num_patches=None,
                                              min_num_patches=n // 5)
        elif self.mode == "cube":
            n = round(np.prod(self.window) * self.ratio)
            max_mask = np.prod(self.window[1:])
            self.generator = MaskingGenerator3D(mask_window_size=self.window, num_masking_patches=n, max_num_patches=max_mask,
                                                min_num_patches=max_mask // 5)

    def __call__(self):
        if self.mode == "tube":
            return np.tile(self.generator(), (8, 1, 1))
        if self.mode == "frames":
            mask = np.zeros(shape=self.window, dtype=int)
            n_mask = round(self.window[0] * self.ratio)
            mask[random.sample(range(0, self.window[0]), n_mask), :, :] += 1
            return mask
        return self.generator()

    def sample_batch(self, n):
        """uint8 (n, Tw, Hw, Ww) host tensor: n draws in loader order."""
        return torch.from_numpy(np.stack([self() for _ in range(n)]).astype(np.uint8))


class MaeMaskGenerator:
    """The random masking of MAE (slowfast/models/masked.py:283-317, MASK.MAE_RND_MASK) drawn on the host:
    ``sample_batch(N)`` is the int32 ``(N, L)`` ids_restore table -- argsort(argsort(noise)) of ``torch.rand(N, L)`` on torch's
    CPU generator, so a loop seeded with ``torch.manual_seed`` like a CPU run of the reference keeps and removes the same
    tokens.  Row l of sample b is kept iff ``ids_restore[b][l] < len_keep``.  (A stable sort: equal noise values, which the
    reference orders as its sort happens to, keep their order here.)"""

    def __init__(self, num_tokens, mask_ratio):
        self.num_tokens, self.mask_ratio = int(num_tokens), float(mask_ratio)
        self.len_keep = int(self.num_tokens * (1 - self.mask_ratio))       # the reference's expression: 64 * (1 - 0.9) -> 6
        assert self.len_keep > 1

    def sample_batch(self, n):
        noise = torch.rand(n, self.num_tokens)
        ids_shuffle = torch.argsort(noise, dim=1, stable=True)
        return torch.argsort(ids_shuffle, dim=1, stable=True).to(torch.int32)

    def mask(self, ids_restore):
        """The reference's binary mask of a table: 1.0 on removed rows."""
        return (ids_restore >= self.len_keep).float()


def construct_mae_mask_generator(cfg):
    """The ids_restore source of a cfg with MASK.MAE_ON and MASK.MAE_RND_MASK (None otherwise)."""
    if not (cfg.MASK.MAE_ON and cfg.MASK.MAE_RND_MASK):
        return None
    stride = cfg.MVIT.PATCH_STRIDE
    tokens = ((cfg.DATA.NUM_FRAMES // stride[0]) * (cfg.DATA.TRAIN_CROP_SIZE // stride[1])
              * (cfg.DATA.TRAIN_CROP_SIZE // stride[2]))
    return MaeMaskGenerator(tokens, _aug(cfg, "MASK_RATIO"))


def construct_mask_generator(cfg):
    """The mask source of a cfg with AUG.GEN_MASK_LOADER (None otherwise)."""
    if not _aug(cfg, "GEN_MASK_LOADER"):
        return None
    return MaskSampler(cfg)
