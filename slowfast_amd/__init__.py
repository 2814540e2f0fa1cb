"""slowfast_amd -- MI355X-native forward/backward engine for the PySlowFast video backbones.

Hand-written gfx950 HIP kernels behind a C ABI (include/sfamd.h, csrc/), wrapped as torch.nn.Module
drop-ins with the reference's constructor signatures, cfg keys and state_dict names.
"""
from .config import CfgNode, get_cfg, get_preset  # noqa: F401
from .registry import MODEL_REGISTRY, build_model  # noqa: F401

__version__ = "0.1.0"
from . import video_models  # noqa: F401,E402  (registers SlowFast / ResNet in MODEL_REGISTRY)
from . import mvit  # noqa: F401,E402  (registers MViT)
from . import x3d  # noqa: F401,E402  (registers X3D, the x3d_stem and x3d_transform factories)
from . import masked  # noqa: F401,E402  (registers MaskMViT: MaskFeat pre-training with HOG targets)
from .masking import MaskingGenerator, MaskingGenerator3D, construct_mask_generator  # noqa: F401,E402  (loader masks)
from .masking import MaeMaskGenerator, construct_mae_mask_generator  # noqa: F401,E402  (MAE random masking: ids_restore tables)
from .data import pack_pathways_u8  # noqa: F401,E402  (uint8 frames -> stem operand layout)
from .mixup import MixUp, construct_mixup  # noqa: F401,E402  (MixUp / CutMix of the batch on the device)
from .random_erasing import RandomErasing, ErasePlan, construct_random_erasing  # noqa: F401,E402  (random erasing on the device)
from .spatial_sampling import (SpatialSampling, CropRow, CropTable, construct_spatial_sampling,  # noqa: F401,E402
                               sample_clip)  # (scale jitter / crop / flip from uint8 on the device)
from .spatial_sampling import transform_boxes, collate_boxes, construct_ava_sampling  # noqa: F401,E402  (AVA: boxes follow the crop)
from .color_augmentation import (ColorAugmentation, ColorRow, ColorTable, construct_color_augmentation,  # noqa: F401,E402
                                 color_clip)  # (colour jitter / PCA lighting / normalisation of the AVA clip on the device)
from .rand_augment import (RandAugment, AugRow, AugTable, construct_rand_augment,  # noqa: F401,E402
                           rand_augment_clip)  # (RandAugment of the decoded uint8 frames on the device)
from .ssl_color import (SslColorJitter, SslRow, SslTable, construct_ssl_color_jitter,  # noqa: F401,E402
                        ssl_color_clip)  # (SSL colour jitter / grey / blur of the decoded uint8 frames on the device)
from .losses import get_loss_func  # noqa: F401,E402
from . import contrastive  # noqa: F401,E402  (registers ContrastiveModel: MoCo pre-training)
from .contrastive import (ByolSimFn, ContrastiveModel, MoCoNceFn, SimclrNtXentFn, byol_sim, contrastive_forward,  # noqa: F401,E402
                          contrastive_parameter_surgery, ema_update, enqueue, l2norm_rows, moco_nce,
                          simclr_ntxent)  # (MoCo / BYOL / SimCLR step glue)
