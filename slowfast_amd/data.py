"""Input side of the hot path: decoded uint8 frames -> the stems' operand layout in one kernel per
pathway.

The reference normalises on the host in fp32 (``utils.tensor_normalize``, slowfast/datasets/utils.py:278-297), permutes
T,H,W,C -> C,T,H,W (datasets/kinetics.py:375-408), builds the pathway list (``pack_pathway_output``,
datasets/utils.py:78-111: Slow = ``index_select(frames, 1, linspace(0, T-1, T//ALPHA).long())``, optional BGR reversal)
and ships float32 clips to the GPU, where this engine would convert them to fp16 W-pair rows again.
``pack_pathways_u8`` takes the cropped uint8 clip batch (N, T, H, W, 3) on the device and writes, per pathway, the
normalised fp16 N,T,H,W,4 buffer the stems read directly (``engine.StemConvUnit`` skips its own conversion for tensors
produced here) -- a quarter of the bytes over PCIe and no fp32 clip in HBM."""
import torch

from . import lib as _sflib

from . import ops
from .lib import get_lib

_f16 = _sflib.act_dtype()        # fp16, or bf16 under SF_ACT_DTYPE=bf16 (lib.ACT_MODE)


def pathway_frame_indices(cfg, num_frames):
    """Source-frame indices of every pathway, as pack_pathway_output builds them (datasets/utils.py:89-105)."""
    if cfg.MODEL.ARCH in cfg.MODEL.SINGLE_PATHWAY_ARCH:
        return [None]
    if cfg.MODEL.ARCH in cfg.MODEL.MULTI_PATHWAY_ARCH:
        return [torch.linspace(0, num_frames - 1, num_frames // cfg.SLOWFAST.ALPHA).long(), None]
    raise NotImplementedError(f"Model arch {cfg.MODEL.ARCH} is not in "
                              f"{cfg.MODEL.SINGLE_PATHWAY_ARCH + cfg.MODEL.MULTI_PATHWAY_ARCH}")


def pack_pathways_u8(frames, cfg, out=None, mix=None, erase=None, crop=None):
    """frames: uint8 (N, T, H, W, 3) device tensor (decoded, sampled, cropped).  Returns the model input list: one
    channels-last fp16 tensor per pathway in the W-pair view (N, 8, T', H, W/2), tagged so that the stems use it as is.
    ``out``: tensors of a previous call (e.g. the static input buffers of a captured step.TrainStep) to write into.
    ``mix``: a ``mixup.MixParams`` (``MixUp.sample_params``): MixUp / CutMix of the batch, applied in fp32 between the
    normalisation and the 16-bit rounding -- what the reference's ``mixup_fn`` does to the fp32 clip.  It applies to pathway 0
    ONLY: the reference mixes ``inputs[0]`` and nothing else (tools/train_net.py:109-111), so the Fast pathway of a SlowFast
    model stays unmixed.  ``mix=None`` (or a draw with lam == 1.0) is the unmixed kernel.
    ``erase``: a ``random_erasing.EraseTable`` (``RandomErasing.sample_batch(N, (T, 3, H, W))``): random erasing of the
    normalised clip, in fp32 before the mixing and the rounding.  It applies to EVERY pathway -- the reference erases in the
    dataset before ``pack_pathway_output`` (datasets/kinetics.py:437-449) -- and sample ``i`` and its mixing partner
    ``N-1-i`` are each erased with their own rows before they are blended.  Erased values are indexed by the source frame and
    by the channel in DATA.MEAN order, so the Slow pathway stays the ``index_select`` of the Fast one and
    DATA.REVERSE_INPUT_CHANNEL permutes them with the image.  ``erase=None`` (or a table without rows) reaches the kernels
    above unchanged.
    ``crop``: a ``spatial_sampling.CropTable`` (``SpatialSampling.sample_batch(sizes)``): the frames are then the DECODED
    (N, T, Hs, Ws, 3) buffer, every sample padded to the batch's largest frame, and each sample is resized, cropped and flipped
    through its own row (csrc/sf_sample.h) to S x S = ``crop.crop_size`` (even) before the erasing and the mixing -- the
    reference's order (datasets/kinetics.py:402-449).  ``erase`` must then be drawn for the CROPPED clip (T, 3, S, S), the
    cutmix box of ``mix`` lies in the S x S plane, and the mixing partner is sampled with its own row before the blend.
    ``crop=None`` reaches the kernels above exactly as before."""
    from . import random_erasing, spatial_sampling
    mean, std = [float(v) for v in cfg.DATA.MEAN], [float(v) for v in cfg.DATA.STD]
    if crop is None:
        assert frames.dtype == torch.uint8 and frames.dim() == 5 and frames.shape[-1] == 3 and frames.shape[3] % 2 == 0
        frames = frames.contiguous()
        stream = ops._stream(frames)
        N, T, H, W, _ = frames.shape
        Ho, Wo, clip = H, W, "frames are"
    else:                                   # everything is checked before the first launch; a rejected call raises SfError
        stream = spatial_sampling.check_frames(frames, "pack_pathways_u8")
        N, T, H, W, _ = frames.shape
        Ho = Wo = int(crop.crop_size)
        if Ho <= 0 or Ho % 2:
            raise _sflib.SfError("pack_pathways_u8: the crop size must be even (got %d)" % Ho)
        chost, cdev = spatial_sampling.upload_table(crop, N, frames.device)
        clip = "cropped clip is"
    ehost = edev = None
    rows = words = emode = 0
    if erase is not None and len(erase.rows):
        if tuple(erase.shape) != (T, 3, Ho, Wo):
            raise _sflib.SfError("pack_pathways_u8: the erase table was drawn for (T, C, H, W) = %s, the %s %s" % (
                tuple(erase.shape), clip, (T, 3, Ho, Wo)))
        ehost, edev, rows = random_erasing.upload_table(erase, N, frames.device)
        words, emode = int(ehost.size), random_erasing.MODES[erase.mode]
    dst, out = out, []
    for i, idx in enumerate(pathway_frame_indices(cfg, T)):
        Tout = T if idx is None else int(idx.numel())
        idx_dev = None if idx is None else idx.to(device=frames.device, dtype=torch.int32).contiguous()
        if dst is None:
            base = torch.empty((N, Tout, Ho, Wo // 2, 8), dtype=_f16, device=frames.device)
        else:
            base = dst[i].permute(0, 2, 3, 4, 1)
            fits = tuple(base.shape) == (N, Tout, Ho, Wo // 2, 8) and base.is_contiguous() and base.dtype == _f16
            if crop is None:
                assert fits, "out[i] must be a tensor a previous pack_pathways_u8 call returned for the same clip geometry"
            elif not fits:
                raise _sflib.SfError("pack_pathways_u8: out[%d] must be a tensor a previous call returned for the same cropped "
                                     "clip geometry" % i)
        mixing = i == 0 and mix is not None and mix.lam != 1.0
        lam = float(mix.lam) if mixing else 1.0
        box = [int(v) for v in (mix.box if mixing and mix.use_cutmix else (0, 0, 0, 0))]
        # the entry point with the fewest stages that holds this call's, and its argument list after ``out``
        tail = [int(bool(mix.use_cutmix)) if mixing else -1, lam, 1.0 - lam] + box
        etail = [emode, None if ehost is None else ehost.ctypes.data, ops._ptr(edev), rows, words]
        pixels = float(N * Tout * Ho * Wo)
        if crop is not None:                # four taps of three bytes per sampled pixel, of the partner too under mixup
            name, tail = "sf_pack_clip_u8_sample", [chost.ctypes.data, cdev.data_ptr(), Ho] + etail + tail
            read = (24.0 if mixing and not mix.use_cutmix else 12.0) * pixels
        elif ehost is not None:
            name, tail = "sf_pack_clip_u8_aug", etail + tail
            read = (6.0 if mixing and not mix.use_cutmix else 3.0) * pixels
        elif mixing:
            name = "sf_pack_clip_u8_mix"
            read = (3.0 if mix.use_cutmix else 6.0) * pixels
        else:
            name, tail = "sf_pack_clip_u8", []
            read = 3.0 * pixels
        get_lib().call(name, frames.data_ptr(), N, T, H, W, ops._ptr(idx_dev), Tout, mean[0], mean[1], mean[2], std[0], std[1],
                       std[2], int(bool(cfg.DATA.REVERSE_INPUT_CHANNEL)), base.data_ptr(), *tail, stream,
                       work=dict(bytes=read + 2.0 * base.numel()))
        x = base.permute(0, 4, 1, 2, 3)
        x._sf_wpairs = True                 # already the operand layout of engine.StemConvUnit
        out.append(x)
    return out
