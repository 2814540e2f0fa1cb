"""Masked-feature pre-training: ``MaskMViT`` with HOG targets (slowfast/models/masked.py, operators.py:62-112 HOGLayerC,
head_helper.py:566-672 MSSeparateHead; configs/masked_ssl/k400_MVITv2_*_MaskFeat_PT.yaml).

The backbone is ``mvit.MViT`` with the blocks after ``MASK.PRETRAIN_DEPTH[-1]`` removed; around it this module adds
  * ``hog_targets``: the regression targets of the clip in ONE launch (csrc/sf_hog.h), fp32 whatever the activation type,
  * the mask-token substitution after the patch embedding (tokens.MaskTokenFn, csrc/sf_tokens.h),
  * the prediction head: LayerNorm through the token LayerNorm kernel, the Linear to 27*u*u outputs as a torch fp32 op.

Built path: ``MASK.PRED_HOG``, ``HEAD_TYPE: "separate"``, masks from the loader (``masking.construct_mask_generator``), any
number of ``PRETRAIN_DEPTH`` entries.  ``MASK.MAE_ON``, ``MASK.MAE_RND_MASK``, pixel targets, ``separate_xformer`` and
``MVIT.PATCH_2D`` raise NotImplementedError.

Two call forms.  ``model([clip, meta, mask])`` returns ``(preds, labels)`` exactly as the reference: rows gathered by the
boolean mask, ``labels[i] = (target_rows, 1.0, "mse")`` -- eager only, the shapes depend on the mask.  With
``model.dense = True`` nothing is gathered: ``preds[i]`` is ``(B, N_i, C_i)`` and ``labels[i] = (targets, 1.0, "mse", mask_i)``
with ``mask_i`` a ``(B, N_i)`` float tensor (losses.MultipleMSELoss) -- fixed shapes, the form a captured step uses.
"""
import math

import torch
import torch.nn as nn
from torch.nn.init import trunc_normal_

from . import engine, ops
from .lib import SfError, get_lib
from .mvit import MViT
from .mvit_engine import NormUnit, TokenNormFn
from .registry import MODEL_REGISTRY
from .tokens import MaskTokenFn

HOG_CELL, HOG_BINS = 8, 9


def hog_targets(clip, ts, fs, out=None):
    """HOG targets of a dense fp32 (B, 3, T, H, W) clip: frames 0, ts, 2 ts, ...; 8 x 8 cells, 9 bins; ``fs`` tokens per
    side.  Returns fp32 (B, T'*fs*fs, 27*u*u), u = (H / 8) / fs, in the row / feature order of ``_get_hog_label_3d``."""
    if getattr(clip, "_sf_wpairs", False):
        raise NotImplementedError("hog_targets: a clip in the packed W-pair layout (_sf_wpairs) has pixels already rounded to "
                                  "16 bits; the targets are computed from the dense float32 clip")
    if not (torch.is_tensor(clip) and clip.dim() == 5 and clip.shape[1] == 3 and clip.dtype == torch.float32
            and clip.is_contiguous()):
        raise SfError("hog_targets: the clip must be a dense float32 (B, 3, T, H, W) device tensor (got %s)" % (
            "%s %s" % (clip.dtype, tuple(clip.shape)) if torch.is_tensor(clip) else type(clip).__name__))
    stream = ops._stream(clip)          # raises for a CPU tensor with the gfx950 library: there is no torch fallback
    B, _, T, H, W = (int(v) for v in clip.shape)
    ts, fs = int(ts), int(fs)
    if H != W:
        raise SfError("hog_targets: H != W (%d x %d): the targets are defined for square clips" % (H, W))
    if ts <= 0 or fs <= 0 or H % (HOG_CELL * fs):
        raise SfError("hog_targets: H %% (8 * fs) != 0 (H=%d, fs=%d): u = (H / 8) / fs must be a whole number >= 1" % (H, fs))
    Tu, u = (T + ts - 1) // ts, (H // HOG_CELL) // fs
    shape = (B, Tu * fs * fs, 3 * HOG_BINS * u * u)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=clip.device)
    elif not (tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == clip.device):
        raise SfError("hog_targets: out must be a dense float32 %s tensor on the clip's device" % (shape,))
    get_lib().call("sf_hog_targets_f32", clip.data_ptr(), B, T, H, W, ts, fs, out.data_ptr(), stream,
                   work=dict(bytes=4.0 * (B * 3 * Tu * H * W + out.numel())))
    return out


def calc_mvit_feature_geometry(cfg):
    """slowfast/models/utils.py:185-212: per block, the (T, H, W) token grid and its stride in pixels."""
    m = cfg.MVIT
    t = cfg.DATA.NUM_FRAMES // m.PATCH_STRIDE[0] if len(m.PATCH_STRIDE) > 2 else 1
    feat_size = [[t, cfg.DATA.TRAIN_CROP_SIZE // m.PATCH_STRIDE[-2], cfg.DATA.TRAIN_CROP_SIZE // m.PATCH_STRIDE[-1]]
                 for _ in range(m.DEPTH)]
    feat_stride = [[m.PATCH_STRIDE[0] if len(m.PATCH_STRIDE) > 2 else 1, m.PATCH_STRIDE[-2], m.PATCH_STRIDE[-1]]
                   for _ in range(m.DEPTH)]
    for x in m.POOL_Q_STRIDE:
        for i in range(m.DEPTH):
            if i >= x[0]:
                for j in range(3):
                    feat_size[i][j] = feat_size[i][j] // x[j + 1]
                    feat_stride[i][j] = feat_stride[i][j] * x[j + 1]
    return feat_size, feat_stride


class HOGLayerC(nn.Module):
    """The state of the reference's HOG layer (operators.py:62-77): its two Sobel filters are registered buffers, so they are
    keys of a MaskMViT checkpoint (``hogs.0.weight_x`` / ``weight_y``).  The targets themselves come from ``hog_targets``,
    whose arithmetic is fixed (csrc/sf_hog.h) and does not read these buffers."""

    def __init__(self, nbins=HOG_BINS, pool=HOG_CELL):
        super().__init__()
        self.nbins, self.pool = nbins, pool
        weight_x = torch.tensor([[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]]).view(1, 1, 3, 3).repeat(3, 1, 1, 1)
        self.register_buffer("weight_x", weight_x)
        self.register_buffer("weight_y", weight_x.transpose(2, 3).contiguous())

    def forward(self, clip, ts, fs):
        return hog_targets(clip, ts, fs)


class MSSeparateHead(nn.Module):
    """One LayerNorm + Linear per pre-training depth (head_helper.py:566-672, HEAD_TYPE "separate")."""

    def __init__(self, blocks, cfg, num_classes, feat_sz):
        super().__init__()
        head_type = cfg.MASK.HEAD_TYPE.split("_")
        assert head_type[0] == "separate"
        if len(head_type) > 1:
            raise NotImplementedError("MASK.HEAD_TYPE %r: the transformer decoder head (separate_xformer) is not built"
                                      % (cfg.MASK.HEAD_TYPE,))
        if cfg.MVIT.NORM != "layernorm":
            raise NotImplementedError("Only supports layernorm.")
        self.cls_embed_on = cfg.MVIT.CLS_EMBED_ON
        self.transforms, self.projections = nn.ModuleList(), nn.ModuleList()
        for depth, num_class in zip(cfg.MASK.PRETRAIN_DEPTH, num_classes):
            head_dim = blocks[depth].dim_out
            self.transforms.append(nn.Sequential(nn.LayerNorm(head_dim, eps=1e-6)))
            self.projections.append(nn.Linear(head_dim, num_class, bias=True))
        self.apply(self._init_weights)
        for seq in self.transforms:
            seq._norm_unit = NormUnit(seq[0])

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward(self, block_outputs, output_masks, return_all, thw=None):
        outs = []
        for idx, x in enumerate(block_outputs):
            seq = self.transforms[idx]
            x = TokenNormFn.apply(x, seq, self.cls_embed_on, seq[0].weight, seq[0].bias).float()    # cls row dropped
            if not return_all:
                x = x[output_masks[idx]]
            outs.append(self.projections[idx](x))
        return outs


@MODEL_REGISTRY.register()
class MaskMViT(MViT):
    """MaskFeat pre-training model; forward(x=[clip NCTHW, meta, mask (B, Tw, Hw, Ww) uint8]) -> (preds, labels)."""

    def __init__(self, cfg):
        k = cfg.MASK
        for key, bad in (("MASK.MAE_ON", k.MAE_ON), ("MASK.MAE_RND_MASK", k.MAE_RND_MASK),
                         ("MASK.PRED_HOG False (pixel targets)", not k.PRED_HOG),
                         ("MASK.HEAD_TYPE separate_xformer", k.HEAD_TYPE != "separate"),
                         ("MVIT.PATCH_2D", cfg.MVIT.PATCH_2D)):
            if bad:
                raise NotImplementedError("MaskMViT: %s is outside the built path (HOG targets, separate head, loader masks)"
                                          % key)
        super().__init__(cfg)
        self.pretrain_depth = list(k.PRETRAIN_DEPTH)
        if self.pretrain_depth[-1] + 1 < cfg.MVIT.DEPTH:
            del self.blocks[self.pretrain_depth[-1] + 1:]
        del self.norm
        del self.head
        del self._norm_unit
        self.feat_size, self.feat_stride = calc_mvit_feature_geometry(cfg)
        self.head_type = k.HEAD_TYPE.split("_")
        feat_sz = [self.feat_size[d] for d in self.pretrain_depth]
        self.nbins, self.cell_sz = HOG_BINS, HOG_CELL
        self.hogs = nn.ModuleList([HOGLayerC(nbins=self.nbins, pool=self.cell_sz)])
        self.ncells = [(self.feat_stride[d][-1] // self.cell_sz) ** 2 for d in self.pretrain_depth]
        self.pred_head = MSSeparateHead(self.blocks, cfg, [3 * self.nbins * n for n in self.ncells], feat_sz)
        self.hog_loss = "mse"
        self.sep_pos_embed_decoder = k.DECODER_SEP_POS_EMBED
        self.mask_token = nn.Parameter(torch.zeros(1, 1, cfg.MVIT.EMBED_DIM))
        trunc_normal_(self.mask_token, std=0.02)
        if k.SCALE_INIT_BY_DEPTH:
            self.fix_init_weight()
        self.pred_pixel_wt, self.pred_hog_wt = 0.0, 1.0
        self.dense = False

    def no_weight_decay(self):
        names = []
        if self.cfg.MVIT.ZERO_DECAY_POS_CLS:       # masked.py:130-147
            if self.use_abs_pos:
                names += (["dec_pos_embed_spatial", "dec_pos_embed_temporal", "dec_pos_embed_class"]
                          if self.sep_pos_embed_decoder else ["pos_embed_decoder"])
            if self.cls_embed_on:
                names.append("cls_token")
        return names

    def fix_init_weight(self):
        for layer_id, layer in enumerate(self.blocks):        # masked.py:149-163 (the separate head has no attention blocks)
            layer.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
            layer.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))

    def _multiscale_mask(self, mask):
        """_get_multiscale_mask: the window table at every pre-training depth's grid, (B, Tw * fs * fs) uint8 each -- the
        nearest-neighbour index map of F.interpolate for integer ratios, which is the one the mask-token kernels use."""
        Hw, Ww = int(mask.shape[2]), int(mask.shape[3])
        outs = []
        for d in self.pretrain_depth:
            fs = self.feat_size[d][-1]
            if not ((fs % Hw == 0 or Hw % fs == 0) and (fs % Ww == 0 or Ww % fs == 0)):
                raise SfError("MaskMViT: the mask window grid %d x %d and the %d x %d grid of depth %d are not integer "
                              "multiples" % (Hw, Ww, fs, fs, d))
            ih = (torch.arange(fs, device=mask.device) * Hw) // fs
            iw = (torch.arange(fs, device=mask.device) * Ww) // fs
            outs.append(mask[:, :, ih][:, :, :, iw].flatten(1))
        return outs

    def forward(self, x, return_all=False):
        if not (isinstance(x, (list, tuple)) and len(x) == 3 and torch.is_tensor(x[2])):
            raise NotImplementedError("MaskMViT takes [clip, meta, mask] with the loader's mask table (AUG.GEN_MASK_LOADER); "
                                      "masks drawn inside the model (MASK.MAE_RND_MASK) are not built")
        clip, _, mask = x
        if engine.SEGMENTS is not None and len(self.pretrain_depth) > 1:
            raise NotImplementedError("MaskMViT: a segmented backward with more than one MASK.PRETRAIN_DEPTH entry")
        ts = self.patch_stride[0]
        targets = {}
        for d in self.pretrain_depth:              # one launch per distinct grid
            fs = self.feat_size[d][-1]
            if fs not in targets:
                targets[fs] = self.hogs[0](clip, ts, fs)
        pos = self._pos_embed()
        tok, bcthw = self.patch_embed(clip, self.cls_token if self.cls_embed_on else None, pos)
        T, H, W = bcthw[-3], bcthw[-2], bcthw[-1]
        assert (T, H, W) == (self.T, self.H, self.W), bcthw
        if mask.dtype != torch.uint8:
            mask = mask.to(torch.uint8)
        mask = mask.contiguous()
        tok = MaskTokenFn.apply(tok, mask, (T, H, W), int(self.cls_embed_on), self.mask_token, pos)
        output_masks = self._multiscale_mask(mask)
        _, thw, block_outputs = self._run_blocks(tok, [T, H, W], self._resid_side(tok, pos), collect=self.pretrain_depth)
        dense = self.dense or return_all
        bool_masks = [m.to(torch.bool) for m in output_masks]
        preds = self.pred_head(block_outputs, bool_masks, return_all=dense, thw=thw)
        labels = []
        for d, m, mb, p in zip(self.pretrain_depth, output_masks, bool_masks, preds):
            t = targets[self.feat_size[d][-1]]
            if t.shape[1] != m.shape[1]:
                raise SfError("MaskMViT: %d target rows for %d tokens at depth %d (temporal pooling before a pre-training "
                              "depth is not built)" % (t.shape[1], m.shape[1], d))
            labels.append((t, self.pred_hog_wt, self.hog_loss, m.float()) if self.dense
                          else (t[mb], self.pred_hog_wt, self.hog_loss))
        return preds, labels
