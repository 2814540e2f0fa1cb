"""Loss table of the training loop (slowfast/models/losses.py:61-80) for the losses the hot path trains with.

``soft_cross_entropy`` is what every MIXUP.ENABLE recipe selects: the mixed (B, K) soft labels of ``mixup.MixUp`` against the
logits.  It works on a B x K tensor and is not a hot path: plain torch ops, captured with the step like ``F.cross_entropy``."""
from functools import partial

import torch
import torch.nn as nn


class SoftTargetCrossEntropyLoss(nn.Module):
    """pytorchvideo.losses.soft_target_cross_entropy.SoftTargetCrossEntropyLoss: sum(-target * log_softmax(x)) per sample."""

    def __init__(self, ignore_index=-100, reduction="mean", normalize_targets=True):
        super().__init__()
        if reduction not in ("mean", "none"):
            raise NotImplementedError('reduction must be "mean" or "none" (got %r)' % (reduction,))
        self.ignore_index, self.reduction, self.normalize_targets = ignore_index, reduction, normalize_targets

    def forward(self, x, target):
        if target.shape != x.shape:
            raise ValueError("soft_cross_entropy needs (B, K) soft labels of the logits' shape %s (got %s)"
                             % (tuple(x.shape), tuple(target.shape)))
        if self.normalize_targets:
            target = target / (target.sum(-1, keepdim=True) + 1e-6)
        loss = torch.sum(-target * torch.nn.functional.log_softmax(x, dim=-1), dim=-1)
        return loss.mean() if self.reduction == "mean" else loss


_LOSSES = {
    "cross_entropy": nn.CrossEntropyLoss,
    "bce": nn.BCELoss,
    "bce_logit": nn.BCEWithLogitsLoss,
    "soft_cross_entropy": partial(SoftTargetCrossEntropyLoss, normalize_targets=False),
}


def get_loss_func(loss_name):
    """The loss class of ``cfg.MODEL.LOSS_FUNC``; instantiate it as ``get_loss_func(name)(reduction="mean")``."""
    if loss_name not in _LOSSES.keys():
        raise NotImplementedError("Loss {} is not supported".format(loss_name))
    return _LOSSES[loss_name]
