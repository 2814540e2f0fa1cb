"""Pin the CPU oracle to the real reference and write tests/golden/*.json (run in the build container).

For each case: build the UNMODIFIED reference model (via oracle/refshim.py) from its own YAML + overrides,
load deterministic parameters (oracle.video_ref.randomize_state), run forward + cross-entropy + backward
on a seeded synthetic batch, run the oracle restatement on the same state_dict/batch, REQUIRE agreement
to fp32 round-off, and store the reference's numbers (logits, loss, grad-norm, per-parameter grad norms,
updated BN running statistics checksums).  The fixtures let the GPU box (which has no /root/reference)
check the oracle -- and through it the HIP engine -- against the reference's own outputs.

    python -m oracle.make_golden [case ...]        (reference_contract: tests/golden/reference_contract.json)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import mvit_ref, refshim, video_ref  # noqa: E402

TINY = ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 32,
        "RESNET.WIDTH_PER_GROUP", 16, "RESNET.DEPTH", 18]
CASES = {
    # name: (reference yaml, overrides, batch)
    "slowfast_tiny": ("configs/Kinetics/SLOWFAST_8x8_R50.yaml",
                      TINY + ["DATA.NUM_FRAMES", 8, "SLOWFAST.BETA_INV", 2,
                              "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2, 2], [2, 2], [2, 2], [2, 2]]"], 2),
    "c2d_tiny": ("configs/Kinetics/C2D_8x8_R50.yaml",
                 TINY + ["DATA.NUM_FRAMES", 4, "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2], [2], [2], [2]]"], 2),
    "slow_tiny": ("configs/Kinetics/SLOW_8x8_R50.yaml",
                  TINY + ["DATA.NUM_FRAMES", 4, "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2], [2], [2], [2]]"], 2),
    # RESNET.TRANS_FUNC basic_transform (resnet_helper.py:27-115; ResNet-18/34 style blocks: Tx3x3 -> 1x3x3), I3D
    # temporal kernels so that the first convolution of res2..res5 blocks is a true 3x3x3
    "i3d_basic_tiny": ("configs/Kinetics/I3D_8x8_R50.yaml",
                       ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                        "RESNET.WIDTH_PER_GROUP", 8, "RESNET.DEPTH", 18, "DATA.NUM_FRAMES", 4,
                        "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2], [2], [2], [2]]", "RESNET.TRANS_FUNC", "basic_transform"], 4),
    # full-width R50 models at reduced clip size, batch chosen so every BatchNorm sees >= 100 samples
    # (a BN over a handful of samples amplifies fp16 round-off and would test conditioning, not kernels)
    "slowfast_r50_mid": ("configs/Kinetics/SLOWFAST_8x8_R50.yaml",
                         ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DATA.TRAIN_CROP_SIZE", 96,
                          "DATA.NUM_FRAMES", 16], 4),
    "c2d_r50_mid": ("configs/Kinetics/C2D_8x8_R50.yaml",
                    ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DATA.TRAIN_CROP_SIZE", 96, "DATA.NUM_FRAMES", 8], 4),
    "i3d_r50_mid": ("configs/Kinetics/I3D_8x8_R50.yaml",
                    ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DATA.TRAIN_CROP_SIZE", 96, "DATA.NUM_FRAMES", 8], 4),
    # Nonlocal blocks: C2D-NLN (softmax affinity, (1,2,2) pooling) and SlowFast-NLN (dot-product affinity)
    "c2d_nln_mid": ("configs/Kinetics/C2D_NLN_8x8_R50.yaml",
                    ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DATA.TRAIN_CROP_SIZE", 96, "DATA.NUM_FRAMES", 8], 4),
    "slowfast_nln_tiny": ("configs/Kinetics/SLOWFAST_NLN_8x8_R50.yaml",
                          TINY + ["DATA.NUM_FRAMES", 8, "SLOWFAST.BETA_INV", 2, "DATA.TRAIN_CROP_SIZE", 64,
                                  "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2, 2], [2, 2], [2, 2], [2, 2]]",
                                  "NONLOCAL.LOCATION", "[[[], []], [[1], []], [[1], []], [[], []]]",
                                  "NONLOCAL.POOL", "[[[2, 2, 2], [2, 2, 2]], [[2, 2, 2], [2, 2, 2]], [[2, 2, 2], [2, 2, 2]], [[2, 2, 2], [2, 2, 2]]]"], 4),
    # NONLOCAL.GROUP 2: the Slow pathway's frames are folded into the batch around the Nonlocal blocks
    "slowfast_nln_group_tiny": ("configs/Kinetics/SLOWFAST_NLN_8x8_R50.yaml",
                                TINY + ["DATA.NUM_FRAMES", 16, "SLOWFAST.BETA_INV", 2, "DATA.TRAIN_CROP_SIZE", 64,
                                        "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2, 2], [2, 2], [2, 2], [2, 2]]",
                                        "NONLOCAL.LOCATION", "[[[], []], [[1], []], [[1], []], [[], []]]",
                                        "NONLOCAL.GROUP", "[[1, 1], [2, 1], [2, 1], [1, 1]]",
                                        "NONLOCAL.POOL", "[[[1, 2, 2], [1, 2, 2]], [[1, 2, 2], [1, 2, 2]], [[1, 2, 2], [1, 2, 2]], [[1, 2, 2], [1, 2, 2]]]"], 4,
                                {"final_bn_gamma_scale": 0.25}),     # better conditioned: fp16-storage deviation 3x lower
    # BN.NORM_TYPE sub_batchnorm (multigrid training): statistics per half of the batch, running statistics per split
    "slowfast_subbn_tiny": ("configs/Kinetics/SLOWFAST_8x8_R50.yaml",
                            TINY + ["DATA.NUM_FRAMES", 8, "SLOWFAST.BETA_INV", 2, "DATA.TRAIN_CROP_SIZE", 64,
                                    "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2, 2], [2, 2], [2, 2], [2, 2]]",
                                    "BN.NORM_TYPE", "sub_batchnorm", "BN.NUM_SPLITS", 2], 8,
                            {"final_bn_gamma_scale": 0.25}),
    # BASELINE config 5 backbone: SlowFast-R101 (23 res4 blocks, the first 6 temporal), dot-product Nonlocal after res4
    # blocks 6/13/20 with (2,2,2) pooling, res5 at stride 1 / dilation 2; closed with the basic head (global pooling)
    "slowfast_r101_nl_tiny": ("configs/AVA/c2/SLOWFAST_32x2_R101_50_50.yaml",
                              ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DETECTION.ENABLE", False,
                               "MULTIGRID.SHORT_CYCLE", True, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                               "DATA.NUM_FRAMES", 8, "RESNET.WIDTH_PER_GROUP", 16, "SLOWFAST.BETA_INV", 2], 4,
                              {"final_bn_gamma_scale": 0.25}),
    # BASELINE config 5 with its true AVA head: ResNetRoIHead (temporal average pool -> ROIAlign 7x7 @ 1/16 -> max pool ->
    # Linear -> sigmoid), 3 boxes per clip, BCE on multi-hot labels.  ROIAlign runs on the oracle's restatement inside
    # the reference model as well (detectron2 is not installed): it is the one op of this case that is not pinned.
    "slowfast_ava_roi_tiny": ("configs/AVA/c2/SLOWFAST_32x2_R101_50_50.yaml",
                              ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                               "DATA.TRAIN_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "RESNET.WIDTH_PER_GROUP", 16,
                               "RESNET.DEPTH", 50, "SLOWFAST.BETA_INV", 2,
                               "NONLOCAL.LOCATION", "[[[], []], [[], []], [[1], []], [[], []]]"], 4,
                              {"final_bn_gamma_scale": 0.25, "boxes": 3}),
    # X3D-M (depthwise 3x3x3, SE, Swish, channel widths 54/108 that are not multiples of 8) at reduced clip size
    "x3d_m_mid": ("configs/Kinetics/X3D_M.yaml",
                  ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DATA.TRAIN_CROP_SIZE", 96, "DATA.NUM_FRAMES", 8], 4),
    "x3d_tiny": ("configs/Kinetics/X3D_M.yaml",
                 ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                  "DATA.NUM_FRAMES", 4, "X3D.DEPTH_FACTOR", 1.0, "X3D.DIM_C5", 256], 4),
    # X3D.BN_LIN5: BatchNorm between the head's lin_5 and its ReLU (head_helper.py:440-443)
    "x3d_bnlin5_tiny": ("configs/Kinetics/X3D_M.yaml",
                        ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                         "DATA.NUM_FRAMES", 4, "X3D.DEPTH_FACTOR", 1.0, "X3D.DIM_C5", 256, "X3D.BN_LIN5", True], 4),
    # MViTv2: a 4-block miniature (every block type: q-pooling, dim change, k/v pooling, rel-pos) and the full
    # 16-block MViTv2-S at a reduced clip size
    "mvit_tiny": ("configs/Kinetics/MVITv2_S_16x4.yaml",
                  ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                   "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
                   "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                   "MVIT.POOL_Q_STRIDE", "[[0, 1, 1, 1], [1, 1, 2, 2], [2, 1, 1, 1], [3, 1, 2, 2]]",
                   "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]", "MIXUP.ENABLE", False], 2),
    # MViTv1 family (configs/Kinetics/MVIT_B_16x4_CONV.yaml): separate learned position embeddings, dimension change after
    # the Mlp, blocks 0 and 2 without q pooling, no relative positions, no residual pooling
    "mvit_v1_tiny": ("configs/Kinetics/MVIT_B_16x4_CONV.yaml",
                     ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                      "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
                      "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                      "MVIT.POOL_Q_STRIDE", "[[1, 1, 2, 2], [3, 1, 2, 2]]", "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]",
                      "MIXUP.ENABLE", False], 2),
    # plain video ViT as the masked-SSL fine-tuning configs build it (configs/masked_ssl/k400_VIT_B_16x4_FT.yaml): no
    # pooling anywhere, separate position embeddings, mean pooling of the patch tokens before the final norm
    "vit_tiny": ("configs/masked_ssl/k400_VIT_B_16x4_FT.yaml",
                 ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                  "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 2,
                  "MVIT.EMBED_DIM", 64, "MVIT.NUM_HEADS", 2, "MIXUP.ENABLE", False], 2),
    # MViTv2 without the cls token (CLS_EMBED_ON False: norm -> mean over all tokens feeds the head) and with separate
    # q / k / v Linears (SEPARATE_QKV), as configs/ImageNet/MVITv2_*.yaml and the reversible configs select them
    "mvit_nocls_sepqkv_tiny": ("configs/Kinetics/MVITv2_S_16x4.yaml",
                  ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                   "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
                   "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                   "MVIT.POOL_Q_STRIDE", "[[0, 1, 1, 1], [1, 1, 2, 2], [2, 1, 1, 1], [3, 1, 2, 2]]",
                   "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]", "MIXUP.ENABLE", False,
                   "MVIT.CLS_EMBED_ON", False, "MVIT.SEPARATE_QKV", True], 2),
    # odd pooled extents (72^2 crop: 18 -> 9 -> 5 tokens per side): block 3's relative-position tables are constructed with
    # 2*4-1 rows (9 // 2) but used at 2*5-1 -> get_rel_pos interpolation (attention.py:48-61), as in MViTv2-L 40x3 at 312^2
    "mvit_relinterp_tiny": ("configs/Kinetics/MVITv2_S_16x4.yaml",
                  ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                   "DATA.TRAIN_CROP_SIZE", 72, "DATA.TEST_CROP_SIZE", 72, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
                   "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                   "MVIT.POOL_Q_STRIDE", "[[0, 1, 1, 1], [1, 1, 2, 2], [2, 1, 2, 2], [3, 1, 1, 1]]",
                   "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]", "MIXUP.ENABLE", False], 2),
    # Reversible MViT (configs/Kinetics/REV_MVIT_B_16x4_CONV.yaml; the shipped yaml keeps CLS_EMBED_ON True, which the
    # reference's own constructor rejects -- "rev does not allow cls token" -- so the override is part of the family):
    # two-stream reversible blocks, stage-transition blocks at the q-pooling layers, norm over the concatenated streams
    "mvit_rev_tiny": ("configs/Kinetics/REV_MVIT_B_16x4_CONV.yaml",
                      ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                       "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 5,
                       "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                       "MVIT.POOL_Q_STRIDE", "[[1, 1, 2, 2], [3, 1, 2, 2]]", "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]",
                       "MVIT.REV.BUFFER_LAYERS", "[1, 3]", "MVIT.CLS_EMBED_ON", False, "MIXUP.ENABLE", False], 2),
    # MViT detection (video_model_builder.py:1034-1045, 1218-1226): the final norm on every token, tokens back to
    # (B, C, T, H, W), ResNetRoIHead on 3 boxes per clip with BCE (ROIAlign: the oracle's restatement, as in slowfast_ava_roi_tiny)
    "mvit_ava_roi_tiny": ("configs/Kinetics/MVITv2_S_16x4.yaml",
                  ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                   "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
                   "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                   "MVIT.POOL_Q_STRIDE", "[[0, 1, 1, 1], [1, 1, 2, 2], [2, 1, 1, 1], [3, 1, 2, 2]]",
                   "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]", "MIXUP.ENABLE", False, "DETECTION.ENABLE", True,
                   "MODEL.HEAD_ACT", "sigmoid", "MODEL.LOSS_FUNC", "bce"], 2, {"boxes": 3}),
    # POOL_FIRST (attention.py:296-301, 339-351): the normed block input is folded into heads and pooled before the
    # q / k / v Linears; MViTv1 layout (the family POOL_FIRST was introduced with), cls token on
    "mvit_poolfirst_tiny": ("configs/Kinetics/MVIT_B_16x4_CONV.yaml",
                     ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "MODEL.NUM_CLASSES", 10,
                      "DATA.TRAIN_CROP_SIZE", 64, "DATA.TEST_CROP_SIZE", 64, "DATA.NUM_FRAMES", 8, "MVIT.DEPTH", 4,
                      "MVIT.EMBED_DIM", 32, "MVIT.DIM_MUL", "[[1, 2.0], [3, 2.0]]", "MVIT.HEAD_MUL", "[[1, 2.0], [3, 2.0]]",
                      "MVIT.POOL_Q_STRIDE", "[[1, 1, 2, 2], [3, 1, 2, 2]]", "MVIT.POOL_KV_STRIDE_ADAPTIVE", "[1, 4, 4]",
                      "MIXUP.ENABLE", False, "MVIT.POOL_FIRST", True], 2),
    # WELL-CONDITIONED cases: every BatchNorm sees >= 1000 samples per channel (batch 8, 64^2 crops, 16 / 8
    # frames: the deepest stage still has 8 clips x T x 2 x 2 positions) and the block-final gammas are scaled by 0.05 so that
    # the residual stream stays O(1) and rounding noise is not amplified through 16-33 blocks.  On these the north star's
    # 1e-3 is asserted DIRECTLY on logits / loss / grad-norm -- no yardstick (tests/test_model_gpu.py::test_well_conditioned).
    # "head_weight_abs": the classifier weights are made non-negative: its inputs are post-ReLU (non-negative) features, so
    # with random-sign weights every logit is a cancelling sum whose relative fp16 noise is |w|.|f| / |logit| ~ 2x the
    # per-element noise (1e-3 exactly at the bar, pass or fail by luck); without cancellation the logits are a
    # well-conditioned function of the features and the comparison tests the backbone, not the conditioning of a random FC.
    "slowfast_wc": ("configs/Kinetics/SLOWFAST_8x8_R50.yaml",       # full R50 width (the Fast pathway keeps 8 real channels)
                    ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                     "DATA.NUM_FRAMES", 16], 8,
                    {"final_bn_gamma_scale": 0.05, "head_weight_abs": True}),
    "c2d_wc": ("configs/Kinetics/C2D_8x8_R50.yaml",
               ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                "RESNET.WIDTH_PER_GROUP", 16, "DATA.NUM_FRAMES", 8], 8, {"final_bn_gamma_scale": 0.05, "head_weight_abs": True}),
    "x3d_wc": ("configs/Kinetics/X3D_M.yaml",
               ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64,
                "DATA.NUM_FRAMES", 8], 8, {"final_bn_gamma_scale": 0.05, "head_weight_abs": True}),
    "r101nl_wc": ("configs/AVA/c2/SLOWFAST_32x2_R101_50_50.yaml",
                  ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "DETECTION.ENABLE", False, "MULTIGRID.SHORT_CYCLE", True,
                   "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 64, "DATA.NUM_FRAMES", 16, "RESNET.WIDTH_PER_GROUP", 16,
                   "SLOWFAST.BETA_INV", 4], 8, {"final_bn_gamma_scale": 0.05, "head_weight_abs": True}),
    "mvit_s_mid": ("configs/Kinetics/MVITv2_S_16x4.yaml",
                   ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MVIT.DROPPATH_RATE", 0.0, "DATA.TRAIN_CROP_SIZE", 96,
                    "DATA.TEST_CROP_SIZE", 96, "DATA.NUM_FRAMES", 8, "MIXUP.ENABLE", False], 2),
}


def _family(cfg):
    return mvit_ref if cfg.MODEL.MODEL_NAME == "MViT" else video_ref


def run_case(name):
    yaml_rel, opts, batch = CASES[name][:3]
    tweaks = CASES[name][3] if len(CASES[name]) > 3 else {}
    cfg = refshim.reference_cfg(yaml_rel, opts)
    torch.manual_seed(0)
    model = refshim.reference_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    fam = _family(cfg)
    sd = fam.randomize_state(shapes, seed=1234)
    if "final_bn_gamma_scale" in tweaks:
        video_ref.scale_final_bn(sd, tweaks["final_bn_gamma_scale"])
    if tweaks.get("head_weight_abs"):
        sd["head.projection.weight"] = sd["head.projection.weight"].abs()
    model.load_state_dict(sd)
    model.train()
    inputs, labels = video_ref.synthetic_batch(cfg, batch, seed=4321)
    bboxes = None
    if tweaks.get("boxes"):
        bboxes = video_ref.synthetic_boxes(cfg, batch, seed=77, per_clip=tweaks["boxes"])
        g = torch.Generator().manual_seed(78)
        labels = (torch.rand((bboxes.shape[0], cfg.MODEL.NUM_CLASSES), generator=g) < 0.2).float()
        logits = model([x.clone() for x in inputs], bboxes)
        loss = torch.nn.functional.binary_cross_entropy(logits, labels)
    else:
        logits = model([x.clone() for x in inputs])
        loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    ref_grads = {k: p.grad for k, p in model.named_parameters()}
    ref_stats = {k: v for k, v in model.state_dict().items() if "running" in k}

    o_logits, o_loss, o_grads, o_stats = (fam.loss_and_grads(sd, cfg, inputs, labels, bboxes=bboxes) if bboxes is not None
                                          else fam.loss_and_grads(sd, cfg, inputs, labels))
    err = float((o_logits - logits.detach()).abs().max() / logits.detach().abs().max())
    assert err < 1e-5, f"{name}: oracle logits differ from the reference ({err:.2e})"
    assert abs(float(o_loss) - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
    worst = 0.0
    gmax = max(float(g.abs().max()) for g in ref_grads.values())
    for k, g in ref_grads.items():
        # parameters whose true gradient vanishes identically (e.g. MViT norm_k.bias: a constant added to every key
        # shifts all scores of a query equally) carry round-off only: measure against the global gradient scale
        e = float((o_grads[k] - g).abs().max() / (g.abs().max() + 1e-3 * gmax))
        worst = max(worst, e)
    assert worst < 1e-4, f"{name}: oracle gradients differ from the reference ({worst:.2e})"
    for k, v in ref_stats.items():
        assert torch.allclose(o_stats.get(k, sd[k]), v, rtol=1e-5, atol=1e-6), k   # untouched buffers keep their value
    gn = float(video_ref.grad_norm(ref_grads))
    print(f"{name}: params {sum(v.numel() for v in ref_grads.values())/1e6:.3f} M  loss {float(loss):.6f}  "
          f"grad_norm {gn:.6f}  oracle-vs-reference logits {err:.1e} grads {worst:.1e}")
    return {
        "reference_yaml": yaml_rel, "opts": opts, "batch": batch, "param_seed": 1234, "data_seed": 4321,
        "state_tweaks": tweaks,
        "logits": logits.detach().tolist(), "loss": float(loss), "grad_norm": gn,
        "param_grad_norms": {k: float(g.norm()) for k, g in ref_grads.items()},
        "running_stat_sums": {k: float(v.double().sum()) for k, v in ref_stats.items()},
        "num_params": sum(v.numel() for v in ref_grads.values()),
        "torch_version": torch.__version__,
    }


# Eval / multi-view test path (tools/test_net.py:25-151): the reference model in eval mode (running-statistics
# BatchNorm, activation + spatial mean in the head) on DATA.TEST_CROP_SIZE clips.  name: (training case whose yaml /
# overrides / parameters are reused, test crop).  A test crop larger than the training crop makes the heads run
# fully-convolutionally (AvgPool3d window < feature extent), as the Kinetics configs do (224 -> 256).
EVAL_CASES = {
    "eval_slowfast_tiny": ("slowfast_tiny", 64),
    "eval_c2d_tiny": ("c2d_tiny", 64),
    "eval_slowfast_nln_tiny": ("slowfast_nln_tiny", 96),
    "eval_slowfast_r50_mid": ("slowfast_r50_mid", 128, {"final_bn_gamma_scale": 0.25}),   # residual stream stays O(1)
    "eval_i3d_basic_tiny": ("i3d_basic_tiny", 96),
    "eval_x3d_tiny": ("x3d_tiny", 96),
    "eval_mvit_tiny": ("mvit_tiny", 64),
}


def run_eval_case(name):
    base, crop = EVAL_CASES[name][:2]
    yaml_rel, opts, batch = CASES[base][:3]
    tweaks = dict(CASES[base][3] if len(CASES[base]) > 3 else {})
    tweaks.update(EVAL_CASES[name][2] if len(EVAL_CASES[name]) > 2 else {})
    cfg = refshim.reference_cfg(yaml_rel, list(opts) + ["DATA.TEST_CROP_SIZE", crop])
    torch.manual_seed(0)
    model = refshim.reference_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    fam = _family(cfg)
    sd = fam.randomize_state(shapes, seed=1234)
    if "final_bn_gamma_scale" in tweaks:
        video_ref.scale_final_bn(sd, tweaks["final_bn_gamma_scale"])
    inputs, _ = video_ref.synthetic_batch(cfg, batch, seed=4321, crop=crop)
    if fam is video_ref:
        sd = video_ref.calibrate_running_stats(sd, cfg, inputs)
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        probs = model([x.clone() for x in inputs])
        o_probs = eval_forward(sd, cfg, inputs)
    err = float((o_probs - probs).abs().max() / probs.abs().max())
    assert err < 1e-5, f"{name}: oracle eval outputs differ from the reference ({err:.2e})"
    assert float((probs.sum(1) - 1).abs().max()) < 1e-5
    print(f"{name}: probs {tuple(probs.shape)} max {float(probs.max()):.4f}  oracle-vs-reference {err:.1e}")
    return {"base_case": base, "reference_yaml": yaml_rel, "opts": list(opts) + ["DATA.TEST_CROP_SIZE", crop],
            "batch": batch, "test_crop": crop, "param_seed": 1234, "data_seed": 4321, "state_tweaks": tweaks,
            "probs": probs.tolist(), "torch_version": torch.__version__}


def eval_forward(sd, cfg, inputs):
    """The oracle's eval-mode forward of whichever family ``cfg`` names."""
    if cfg.MODEL.MODEL_NAME == "MViT":
        return mvit_ref.mvit_forward(sd, cfg, inputs, training=False)
    fwd = video_ref.x3d_forward if cfg.MODEL.MODEL_NAME == "X3D" else video_ref.video_forward
    return fwd(sd, cfg, inputs, training=False)


# tests/test_oracle.py: the reference models whose state_dict keys / shapes the drop-ins must expose, the reference YAMLs whose
# values the built-in presets must carry, and the frames the data oracle is checked on -- recorded from the reference into
# tests/golden/reference_contract.json, so that the tests hold wherever the reference tree is absent
_SUB_BN = ["BN.NORM_TYPE", "sub_batchnorm", "BN.NUM_SPLITS", 2]
STATE_DICT_CASES = [("configs/Kinetics/SLOWFAST_8x8_R50.yaml", "SLOWFAST_8x8_R50", []),
                    ("configs/Kinetics/C2D_8x8_R50.yaml", "C2D_8x8_R50", []),
                    ("configs/Kinetics/SLOW_8x8_R50.yaml", "SLOW_8x8_R50", []),
                    ("configs/Kinetics/I3D_8x8_R50.yaml", "I3D_8x8_R50", []),
                    ("configs/Kinetics/MVITv2_S_16x4.yaml", "MVITv2_S_16x4", []),
                    ("configs/Kinetics/MVIT_B_16x4_CONV.yaml", "MVIT_B_16x4_CONV", []),
                    ("configs/masked_ssl/k400_VIT_B_16x4_FT.yaml", "k400_VIT_B_16x4_FT", []),
                    ("configs/Kinetics/MVITv2_S_16x4.yaml", "MVITv2_S_16x4", ["MVIT.CLS_EMBED_ON", False, "MVIT.SEPARATE_QKV", True]),
                    ("configs/Kinetics/MVIT_B_16x4_CONV.yaml", "MVIT_B_16x4_CONV", ["MVIT.POOL_FIRST", True, "MVIT.CLS_EMBED_ON", False]),
                    ("configs/Kinetics/REV_MVIT_B_16x4_CONV.yaml", "REV_MVIT_B_16x4_CONV", ["MVIT.CLS_EMBED_ON", False]),
                    ("configs/Kinetics/X3D_M.yaml", "X3D_M", []),
                    ("configs/Kinetics/C2D_NLN_8x8_R50.yaml", "C2D_NLN_8x8_R50", []),
                    ("configs/Kinetics/SLOWFAST_NLN_8x8_R50.yaml", "SLOWFAST_NLN_8x8_R50", []),
                    ("configs/Kinetics/SLOWFAST_8x8_R50.yaml", "SLOWFAST_8x8_R50", _SUB_BN),
                    ("configs/Kinetics/X3D_M.yaml", "X3D_M", _SUB_BN),
                    ("configs/Kinetics/SLOW_8x8_R50.yaml", "SLOW_8x8_R50", ["BN.NORM_TYPE", "sync_batchnorm", "BN.NUM_SYNC_DEVICES", 1])]
# reference YAML -> the config sections the preset tests compare (plus CFG_DATA_KEYS of DATA for every one)
_RESNET_SECTIONS, _MVIT_SECTIONS = ("RESNET", "SLOWFAST", "NONLOCAL", "MODEL", "BN"), ("MVIT",)
CFG_YAMLS = {**{f"configs/Kinetics/{n}.yaml": _RESNET_SECTIONS for n in ("SLOWFAST_8x8_R50", "C2D_8x8_R50", "SLOW_8x8_R50",
                                                                         "I3D_8x8_R50", "C2D_NLN_8x8_R50", "SLOWFAST_NLN_8x8_R50")},
             **{y: _MVIT_SECTIONS for y in ("configs/Kinetics/MVITv2_S_16x4.yaml", "configs/Kinetics/MVIT_B_16x4_CONV.yaml",
                                            "configs/Kinetics/REV_MVIT_B_16x4_CONV.yaml", "configs/masked_ssl/k400_VIT_B_16x4_FT.yaml")}}
CFG_DATA_KEYS = ("NUM_FRAMES", "SAMPLING_RATE", "TRAIN_CROP_SIZE", "TEST_CROP_SIZE", "INPUT_CHANNEL_NUM")
DATA_CASES = (("slowfast", False), ("slowfast", True), ("c2d", False))


def state_dict_case_key(yaml_rel, opts):
    return yaml_rel + " " + json.dumps(opts)


def plain(v):
    """A config value as JSON holds it (CfgNode -> dict, tuple -> list)."""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def data_case(arch, reverse):
    """The preset and the seeded uint8 frames (2 clips x 8 x 6 x 10 x 3) of one data-oracle case."""
    import slowfast_amd as sa
    cfg = sa.get_preset("SLOWFAST_8x8_R50" if arch == "slowfast" else "C2D_8x8_R50",
                        ["DATA.MEAN", [0.45, 0.40, 0.35], "DATA.STD", [0.225, 0.25, 0.2], "DATA.REVERSE_INPUT_CHANNEL", reverse])
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (2, 8, 6, 10, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    return cfg, frames


def state_dict_digest(sd):
    """Number of entries + sha256 over the (key, shape) list of a state_dict, in order."""
    import hashlib
    entries = [[k, list(v.shape)] for k, v in sd.items()]
    return {"entries": len(entries), "sha256": hashlib.sha256(json.dumps(entries).encode()).hexdigest()}


def tensor_digest(t):
    """Shape + sha256 of the contiguous float32 bytes: equal digests == torch.equal."""
    import hashlib
    t = t.detach().to(torch.float32).contiguous()
    return {"shape": list(t.shape), "sha256": hashlib.sha256(t.numpy().tobytes()).hexdigest()}


def reference_contract():
    """The record tests/golden/reference_contract.json holds, computed from the reference tree."""
    import re
    rec = {"state_dict": {}, "cfg": {}, "data": {}}
    for yaml_rel, _preset, opts in STATE_DICT_CASES:
        sd = refshim.reference_model(refshim.reference_cfg(yaml_rel, ["NUM_GPUS", 0] + opts)).state_dict()
        rec["state_dict"][state_dict_case_key(yaml_rel, opts)] = state_dict_digest(sd)
    for yaml_rel, sections in CFG_YAMLS.items():
        ref = refshim.reference_cfg(yaml_rel)
        c = {sec: plain(ref[sec]) for sec in sections}
        c["DATA"] = {k: plain(ref.DATA[k]) for k in CFG_DATA_KEYS}
        rec["cfg"][yaml_rel] = c
    # slowfast/datasets/utils.py imports decoders / logging the data path does not need: execute only the two pure functions
    src = open(os.path.join(refshim.REFERENCE_ROOT, "slowfast", "datasets", "utils.py")).read()
    ns = {}
    for fn in ("pack_pathway_output", "tensor_normalize"):
        m = re.search(r"^def " + fn + r"\(.*?(?=^def |\Z)", src, re.S | re.M)
        exec("import torch\n" + m.group(0), ns)
    for arch, reverse in DATA_CASES:
        cfg, frames = data_case(arch, reverse)
        rec["data"][f"{arch}_reverse{int(reverse)}"] = [
            [tensor_digest(r) for r in ns["pack_pathway_output"](
                cfg, ns["tensor_normalize"](frames[n], cfg.DATA.MEAN, cfg.DATA.STD).permute(3, 0, 1, 2))]
            for n in range(frames.shape[0])]
    return rec


def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    for name in (sys.argv[1:] or list(CASES) + list(EVAL_CASES) + ["reference_contract"]):
        if name == "reference_contract":
            rec = reference_contract()
            with open(os.path.join(out_dir, name + ".json"), "w") as f:      # one line per case
                f.write("{\n" + ",\n".join(f" {json.dumps(part)}: {{\n" + ",\n".join(
                    f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in rec[part].items()) + "\n }" for part in rec) + "\n}\n")
            continue
        rec = run_eval_case(name) if name in EVAL_CASES else run_case(name)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(rec, f)
    print("wrote", out_dir)


if __name__ == "__main__":
    main()
