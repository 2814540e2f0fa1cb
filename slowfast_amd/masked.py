"""Masked-feature pre-training: ``MaskMViT`` with HOG targets (slowfast/models/masked.py, operators.py:62-112 HOGLayerC,
head_helper.py:566-672 MSSeparateHead; configs/masked_ssl/k400_MVITv2_*_MaskFeat_PT.yaml).

The backbone is ``mvit.MViT`` with the blocks after ``MASK.PRETRAIN_DEPTH[-1]`` removed; around it this module adds
  * ``hog_targets``: the regression targets of the clip in ONE launch (csrc/sf_hog.h), fp32 whatever the activation type,
  * the mask-token substitution after the patch embedding (tokens.MaskTokenFn, csrc/sf_tokens.h),
  * the prediction head: LayerNorm through the token LayerNorm kernel, the Linear to 27*u*u outputs as a torch fp32 op.

Built path (MaskFeat): ``MASK.PRED_HOG``, ``HEAD_TYPE: "separate"``, masks from the loader
(``masking.construct_mask_generator``), any number of ``PRETRAIN_DEPTH`` entries.  On that path ``MASK.MAE_RND_MASK``, pixel
targets, ``separate_xformer`` and ``MVIT.PATCH_2D`` raise NotImplementedError.

Built path (MAE, configs/masked_ssl/k400_VIT_*_MAE_PT.yaml): ``MASK.MAE_ON`` with ``MAE_RND_MASK``, ``PRED_HOG False``,
``HEAD_TYPE: "separate_xformer"``, one ``PRETRAIN_DEPTH`` entry, a backbone without q / kv pooling and relative positions and
learned absolute positions (``SEP_POS_EMBED`` or a plain ``pos_embed``).  The encoder runs on the KEPT tokens only
(tokens.TokenKeepFn after the patch embedding), the decoder input is assembled in one launch (tokens.TokenRestoreFn) and the
normalised pixel targets come from ``pixel_targets`` (csrc/sf_pixel.h), one pass over the clip.  ``model([clip, meta, ids])``
with ``ids`` an int32 / int64 ``(B, L)`` ids_restore table (masking.MaeMaskGenerator) uses that table; any other third
element, or none, draws ``torch.rand(N, L, device=clip.device)`` and argsorts it as the reference does -- eager only, and the
device's random stream is not the CPU's: a seeded reference run is reproduced through the table form, not through this one.
Everything else (``PER_FRAME_MASKING``, ``AUG.MASK_TUBE``, ``MAE_RND_MASK False``, ``USE_FIXED_SINCOS_POS``, ``VIS_MASK``,
``PATCH_2D``) raises NotImplementedError naming the key.

Two call forms.  ``model([clip, meta, mask])`` returns ``(preds, labels)`` exactly as the reference: rows gathered by the
boolean mask, ``labels[i] = (target_rows, 1.0, "mse")`` -- eager only, the shapes depend on the mask.  With
``model.dense = True`` nothing is gathered: ``preds[i]`` is ``(B, N_i, C_i)`` and ``labels[i] = (targets, 1.0, "mse", mask_i)``
with ``mask_i`` a ``(B, N_i)`` float tensor (losses.MultipleMSELoss) -- fixed shapes, the form a captured step uses.
"""
import math
from functools import partial

import torch
import torch.nn as nn
from torch.nn.init import trunc_normal_

from . import engine, ops
from .lib import SfError, get_lib
from . import masking
from .mvit import MultiScaleBlock, MViT
from .mvit_engine import LinearUnit, NormUnit, TokenNormFn, _notify, param_grads
from .registry import MODEL_REGISTRY
from .tokens import MaskTokenFn, TokenKeepFn, TokenRestoreFn, _f16

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



def pixel_targets(clip, ts, u, p, norm, out=None):
    """Pixel targets of a dense fp32 (B, 3, T, H, W) clip for ALL tokens (``_patchify`` + the normalisation of
    ``_get_pixel_label_3d``): p x p patches, temporal patch stride ``ts``; ``u = 1`` takes frames 0, ts, 2 ts, ...
    (MASK.TIME_STRIDE_LOSS), ``u = ts`` all frames.  Returns fp32 (B, (T/ts)(H/p)(W/p), u*p*p*3); with ``norm`` each row is
    (x - mean) / sqrt(var_unbiased + 1e-6) in the shifted arithmetic of csrc/sf_pixel.h (a constant patch gives exact zeros)."""
    if getattr(clip, "_sf_wpairs", False):
        raise NotImplementedError("pixel_targets: a clip in the packed W-pair layout (_sf_wpairs) has pixels already rounded to "
                                  "16 bits; the targets are computed from the dense float32 clip")
    if not (torch.is_tensor(clip) and clip.dim() == 5 and clip.shape[1] == 3 and clip.dtype == torch.float32
            and clip.is_contiguous()):
        raise SfError("pixel_targets: the clip must be a dense float32 (B, 3, T, H, W) device tensor (got %s)" % (
            "%s %s" % (clip.dtype, tuple(clip.shape)) if torch.is_tensor(clip) else type(clip).__name__))
    stream = ops._stream(clip)          # raises for a CPU tensor with the gfx950 library: there is no torch fallback
    B, _, T, H, W = (int(v) for v in clip.shape)
    ts, u, p = int(ts), int(u), int(p)
    if H != W:
        raise SfError("pixel_targets: H != W (%d x %d): the targets are defined for square clips" % (H, W))
    if ts <= 0 or p <= 0 or H % p:
        raise SfError("pixel_targets: H %% p != 0 (H=%d, p=%d)" % (H, p))
    if T % ts:
        raise SfError("pixel_targets: T %% ts != 0 (T=%d, ts=%d)" % (T, ts))
    if u not in (1, ts):
        raise SfError("pixel_targets: u = %d frames per token: u must be 1 (TIME_STRIDE_LOSS) or ts = %d" % (u, ts))
    shape = (B, (T // ts) * (H // p) * (W // p), u * p * p * 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=clip.device)
    elif not (tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == clip.device):
        raise SfError("pixel_targets: out must be a dense float32 %s tensor on the clip's device" % (shape,))
    # (a row beyond the staged length is rejected by the launcher)
    get_lib().call("sf_pixel_targets_f32", clip.data_ptr(), B, T, H, W, ts, u, p, int(bool(norm)), out.data_ptr(), stream,
                   work=dict(bytes=4.0 * (B * 3 * (T // ts) * u * H * W + out.numel())))
    return out


class TokenLinearFn(torch.autograd.Function):
    """nn.Linear on a token tensor through its LinearUnit (the GEMM kernels): MAE's ``decoder_embed``."""

    @staticmethod
    def forward(ctx, x, unit, *params):
        engine.record_params(ctx, params)
        ctx.unit, ctx.x = unit, x
        return unit.forward(x)

    @staticmethod
    @engine.delivers_grads
    def backward(ctx, dy):
        dy = dy if dy.dtype == _f16 else dy.to(_f16)
        dx = ctx.unit.backward(ctx.x, dy.contiguous())
        _notify(ctx.unit.params())
        ctx.x = None
        return (dx, None) + param_grads(ctx, 2)


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
    """Per pre-training depth: [MASK.DECODER_DEPTH MultiScaleBlocks (HEAD_TYPE "separate_xformer") +] LayerNorm + Linear
    (head_helper.py:566-672)."""

    def __init__(self, blocks, cfg, num_classes, feat_sz):
        super().__init__()
        head_type = cfg.MASK.HEAD_TYPE.split("_")
        assert head_type[0] == "separate"
        xformer = len(head_type) > 1
        if xformer and head_type[1] != "xformer":
            raise NotImplementedError("MASK.HEAD_TYPE %r: the transforms are separate and separate_xformer" % (cfg.MASK.HEAD_TYPE,))
        if cfg.MVIT.NORM != "layernorm":
            raise NotImplementedError("Only supports layernorm.")
        if xformer:
            if list(cfg.MASK.DEC_KV_KERNEL) or list(cfg.MASK.DEC_KV_STRIDE):
                raise NotImplementedError("MASK.DEC_KV_KERNEL / MASK.DEC_KV_STRIDE: key / value pooling in the decoder is not built")
            assert cfg.MASK.DECODER_DEPTH > 0
            if cfg.MASK.DECODER_EMBED_DIM % 64:
                raise NotImplementedError("MASK.DECODER_EMBED_DIM %d: the decoder blocks have DECODER_EMBED_DIM // 64 heads of 64 "
                                          "channels" % cfg.MASK.DECODER_EMBED_DIM)
        self.cls_embed_on = cfg.MVIT.CLS_EMBED_ON
        self.transforms, self.projections = nn.ModuleList(), nn.ModuleList()
        for depth, num_class, feature_size in zip(cfg.MASK.PRETRAIN_DEPTH, num_classes, feat_sz):
            head_dim = cfg.MASK.DECODER_EMBED_DIM if cfg.MASK.MAE_ON else blocks[depth].dim_out
            op = []
            for _ in range(cfg.MASK.DECODER_DEPTH if xformer else 0):
                dim_out = cfg.MASK.DECODER_EMBED_DIM
                op.append(MultiScaleBlock(
                    dim=head_dim, dim_out=dim_out, input_size=feature_size, num_heads=dim_out // 64,
                    mlp_ratio=cfg.MVIT.MLP_RATIO, qkv_bias=cfg.MVIT.QKV_BIAS, drop_rate=cfg.MVIT.DROPOUT_RATE, drop_path=0.0,
                    norm_layer=partial(nn.LayerNorm, eps=1e-6), kernel_q=[], kernel_kv=[], stride_q=[], stride_kv=[],
                    mode=cfg.MVIT.MODE, has_cls_embed=self.cls_embed_on, pool_first=cfg.MVIT.POOL_FIRST))
                head_dim = dim_out
            op.append(nn.LayerNorm(head_dim, eps=1e-6))
            self.transforms.append(nn.Sequential(*op))
            self.projections.append(nn.Linear(head_dim, num_class, bias=True))
        self.apply(self._init_weights)
        for seq in self.transforms:
            seq._norm_unit = NormUnit(seq[-1])

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
            for blk in list(seq)[:-1]:             # separate_xformer: the decoder blocks (all tokens, no pooling)
                x, thw = blk(x, thw)
            x = TokenNormFn.apply(x, seq, self.cls_embed_on, seq[-1].weight, seq[-1].bias).float()  # cls row dropped
            if not return_all:
                x = x[output_masks[idx]]
            outs.append(self.projections[idx](x))
        return outs


@MODEL_REGISTRY.register()
class MaskMViT(MViT):
    """Masked pre-training model.  MaskFeat: forward(x=[clip NCTHW, meta, mask (B, Tw, Hw, Ww) uint8]) -> (preds, labels);
    MAE (MASK.MAE_ON): forward(x=[clip, meta, ids_restore (B, L) int32 / int64]) or forward(x=[clip]) -> (preds, labels)."""

    @staticmethod
    def _check_cfg(cfg):
        """NotImplementedError, naming the key, for everything outside the two built paths."""
        k = cfg.MASK
        if not k.MAE_ON:
            bad = (("MASK.MAE_RND_MASK", k.MAE_RND_MASK), ("MASK.PRED_HOG False (pixel targets)", not k.PRED_HOG),
                   ("MASK.HEAD_TYPE separate_xformer", k.HEAD_TYPE != "separate"), ("MVIT.PATCH_2D", cfg.MVIT.PATCH_2D))
            path = "the built MaskFeat path (HOG targets, separate head, loader masks)"
        else:
            m = cfg.MVIT
            bad = (("MASK.MAE_RND_MASK False (MAE with loader masks)", not k.MAE_RND_MASK),
                   ("MASK.PRED_HOG (HOG targets with MAE)", k.PRED_HOG),
                   ("MASK.HEAD_TYPE %r (MAE is built with separate_xformer)" % (k.HEAD_TYPE,), k.HEAD_TYPE != "separate_xformer"),
                   ("MASK.PRETRAIN_DEPTH with %d entries (MAE takes one)" % len(k.PRETRAIN_DEPTH), len(k.PRETRAIN_DEPTH) != 1),
                   ("MASK.PER_FRAME_MASKING", k.PER_FRAME_MASKING), ("AUG.MASK_TUBE", masking._aug(cfg, "MASK_TUBE")),
                   ("MVIT.USE_FIXED_SINCOS_POS", m.USE_FIXED_SINCOS_POS), ("VIS_MASK.ENABLE", cfg.VIS_MASK.ENABLE),
                   ("MVIT.PATCH_2D", m.PATCH_2D),
                   ("MVIT.USE_ABS_POS False (the decoder adds a learned position embedding)", not m.USE_ABS_POS),
                   ("MVIT.REL_POS_SPATIAL / REL_POS_TEMPORAL", m.REL_POS_SPATIAL or m.REL_POS_TEMPORAL),
                   ("MVIT.POOL_Q_STRIDE (q pooling)", any(math.prod(e[1:]) > 1 for e in m.POOL_Q_STRIDE)),
                   ("MVIT.POOL_KV_STRIDE / POOL_KV_STRIDE_ADAPTIVE / POOL_KVQ_KERNEL (kv pooling)",
                    bool(m.POOL_KV_STRIDE) or m.POOL_KV_STRIDE_ADAPTIVE is not None or m.POOL_KVQ_KERNEL is not None))
            path = ("the built MASK.MAE_ON path (MAE_RND_MASK, pixel targets, separate_xformer, one PRETRAIN_DEPTH entry, no pooling, no "
                    "relative positions)")
        for key, is_bad in bad:
            if is_bad:
                raise NotImplementedError("MaskMViT: %s is outside %s" % (key, path))

    def __init__(self, cfg):
        k = cfg.MASK
        self._check_cfg(cfg)
        super().__init__(cfg)
        self.mae_on = bool(k.MAE_ON)
        self.pretrain_depth = list(k.PRETRAIN_DEPTH)
        if self.pretrain_depth[-1] + 1 < cfg.MVIT.DEPTH:
            del self.blocks[self.pretrain_depth[-1] + 1:]
        del self.norm
        del self.head
        del self._norm_unit
        self.feat_size, self.feat_stride = calc_mvit_feature_geometry(cfg)
        self.head_type = k.HEAD_TYPE.split("_")
        feat_sz = [self.feat_size[d] for d in self.pretrain_depth]
        self.sep_pos_embed_decoder = k.DECODER_SEP_POS_EMBED
        if not self.mae_on:
            self.nbins, self.cell_sz = HOG_BINS, HOG_CELL
            self.hogs = nn.ModuleList([HOGLayerC(nbins=self.nbins, pool=self.cell_sz)])
            self.ncells = [(self.feat_stride[d][-1] // self.cell_sz) ** 2 for d in self.pretrain_depth]
            self.pred_head = MSSeparateHead(self.blocks, cfg, [3 * self.nbins * n for n in self.ncells], feat_sz)
            self.hog_loss = "mse"
            self.mask_token = nn.Parameter(torch.zeros(1, 1, cfg.MVIT.EMBED_DIM))
            self.pred_pixel_wt, self.pred_hog_wt = 0.0, 1.0
        else:
            if any(b.attn.pool_q is not None or b.attn.pool_k is not None or b.pool_skip is not None for b in self.blocks):
                raise NotImplementedError("MaskMViT: MVIT.POOL_Q_STRIDE / POOL_KV_STRIDE (pooling blocks) is outside the built MAE "
                                          "path: the encoder runs on the kept tokens only")
            # masked.py:37-47, 78-121: pixel classes, the encoder's final norm, the decoder embedding and its positions
            self.time_stride_loss, self.norm_pred_pixel = bool(k.TIME_STRIDE_LOSS), bool(k.NORM_PRED_PIXEL)
            self.pred_t_sz = 1 if self.time_stride_loss else self.patch_stride[0]
            self.mask_ratio = float(masking._aug(cfg, "MASK_RATIO"))
            num_classes = [self.pred_t_sz * (self.feat_stride[d][-1] ** 2) * 3 for d in self.pretrain_depth]
            self.pred_head = MSSeparateHead(self.blocks, cfg, num_classes, feat_sz)
            dim_in, dec = self.blocks[-1].dim_out, k.DECODER_EMBED_DIM
            self.norm = nn.LayerNorm(dim_in, eps=1e-6)
            self._norm_unit = NormUnit(self.norm)
            self.decoder_embed = nn.Linear(dim_in, dec, bias=True)
            self._decoder_embed = LinearUnit(self.decoder_embed)
            if self.sep_pos_embed_decoder:
                self.dec_pos_embed_spatial = nn.Parameter(torch.zeros(1, self.patch_dims[1] * self.patch_dims[2], dec))
                self.dec_pos_embed_temporal = nn.Parameter(torch.zeros(1, self.patch_dims[0], dec))
                if self.cls_embed_on:
                    self.dec_pos_embed_class = nn.Parameter(torch.zeros(1, 1, dec))
            else:
                self.decoder_pos_embed = nn.Parameter(torch.zeros(1, math.prod(self.patch_dims) + int(self.cls_embed_on), dec))
            self.mask_token = nn.Parameter(torch.zeros(1, 1, dec))
            for name in ("dec_pos_embed_spatial", "dec_pos_embed_temporal", "dec_pos_embed_class", "decoder_pos_embed"):
                if hasattr(self, name):
                    trunc_normal_(getattr(self, name), std=0.02)
            self.pred_pixel_wt, self.pred_hog_wt = 1.0, 0.0
        trunc_normal_(self.mask_token, std=0.02)
        if k.SCALE_INIT_BY_DEPTH:
            self.fix_init_weight()
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
        for layer_id, layer in enumerate(self.blocks):        # masked.py:149-163
            layer.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
            layer.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
        for trans in self.pred_head.transforms:               # the decoder blocks of separate_xformer, as the reference scales them
            for layer_id, layer in enumerate(trans):
                if hasattr(layer, "attn"):
                    layer.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1 + len(self.blocks))))
                    layer.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))

    def _dec_pos_embed(self):
        """The [1, cls + THW, Cd] decoder position embedding (masked.py:416-436); tiny parameter algebra."""
        if not self.sep_pos_embed_decoder:
            return self.decoder_pos_embed
        pos = self.dec_pos_embed_spatial.repeat(1, self.patch_dims[0], 1) + torch.repeat_interleave(
            self.dec_pos_embed_temporal, self.patch_dims[1] * self.patch_dims[2], dim=1)
        if self.cls_embed_on:
            pos = torch.cat([self.dec_pos_embed_class, pos], 1)
        return pos

    def _mae_forward(self, x):
        """_mae_forward (masked.py:319-476) with the encoder on the kept rows only."""
        clip = x[0] if isinstance(x, (list, tuple)) else x
        L = self.T * self.H * self.W
        K = int(L * (1 - self.mask_ratio))                     # exactly the reference's expression
        assert K > 1
        B = int(clip.shape[0])
        ids = x[2] if isinstance(x, (list, tuple)) and len(x) == 3 else None
        if (torch.is_tensor(ids) and ids.dim() == 2 and ids.dtype in (torch.int32, torch.int64)
                and tuple(ids.shape) == (B, L)):
            ids = ids.to(device=clip.device, dtype=torch.int32).contiguous()
        else:       # _mae_random_masking: drawn on the clip's device (eager only; not the CPU generator's stream)
            noise = torch.rand(B, L, device=clip.device)
            ids = torch.argsort(torch.argsort(noise, dim=1), dim=1).to(torch.int32).contiguous()
        s = int(self.cls_embed_on)
        ts, psz = self.patch_stride[0], self.feat_stride[self.pretrain_depth[0]][-1]
        targets = pixel_targets(clip, ts, self.pred_t_sz, psz, self.norm_pred_pixel)
        pos = self._pos_embed()
        tok, bcthw = self.patch_embed(clip, self.cls_token if self.cls_embed_on else None, pos)
        assert tuple(bcthw[-3:]) == (self.T, self.H, self.W), bcthw
        if targets.shape[1] != L:
            raise SfError("MaskMViT: %d target rows for %d tokens" % (targets.shape[1], L))
        kept = TokenKeepFn.apply(tok, ids, K, s)
        # blocks without pooling or relative positions do not look at the token grid: the K kept tokens are a (1, 1, K) grid
        z, _, _ = self._run_blocks(kept, [1, 1, K], self._resid_side(kept, pos))
        z = TokenNormFn.apply(z, self, False, self.norm.weight, self.norm.bias)
        e = TokenLinearFn.apply(z, self._decoder_embed, self.decoder_embed.weight, self.decoder_embed.bias)
        y = TokenRestoreFn.apply(e, ids, s, self.mask_token, self._dec_pos_embed())
        mask = ids >= K                                        # (B, L): True on removed rows
        preds = self.pred_head([y], [mask], return_all=self.dense, thw=[self.T, self.H, self.W])
        wt = self.pred_pixel_wt / len(self.pretrain_depth)
        if self.dense:
            return preds, [(targets, wt, "mse", mask.float())]
        return preds, [(targets[mask], wt)]

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
        if self.mae_on:
            return self._mae_forward(x)
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
