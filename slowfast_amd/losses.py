"""Loss table of the training loop (slowfast/models/losses.py:61-80) for the losses the hot path trains with.

``soft_cross_entropy`` is what every MIXUP.ENABLE recipe selects: the mixed (B, K) soft labels of ``mixup.MixUp`` against the
logits.  It works on a B x K tensor and is not a hot path: plain torch ops, captured with the step like ``F.cross_entropy``.

``multi_mse`` is the loss of masked-feature pre-training (losses.py:24-58): one MSE per prediction scale.  A label is the
reference's ``(target_rows, weight[, "mse"])`` against gathered prediction rows, or the fixed-shape form of a captured step,
``(targets_dense, weight, "mse", mask)`` against dense ``(B, N, C)`` predictions: sum(mask * (x - y)^2) / (max(sum(mask), 1) * C),
which is the value and the gradient of the mean over the gathered rows whenever a row is masked, and 0 when none is."""
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


class MultipleMSELoss(nn.Module):
    """Several MSE losses; returns (weighted sum, [losses]) as the reference."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError('multi_mse: reduction must be "mean" (got %r)' % (reduction,))
        self.mse_func = nn.MSELoss(reduction=reduction)

    def forward(self, x, y):
        loss_sum = 0.0
        multi_loss = []
        for xt, yt in zip(x, y):
            mask = None
            if isinstance(yt, tuple):
                if len(yt) == 2:
                    (yt, wt), lt = yt, "mse"
                elif len(yt) == 3:
                    yt, wt, lt = yt
                elif len(yt) == 4:
                    yt, wt, lt, mask = yt
                else:
                    raise NotImplementedError
            else:
                wt, lt = 1.0, "mse"
            if lt != "mse":
                raise NotImplementedError
            if mask is None:
                loss = self.mse_func(xt, yt)
            else:
                m = mask.to(xt.dtype)
                d = xt - yt
                loss = (d * d * m.unsqueeze(-1)).sum() / (m.sum().clamp(min=1.0) * xt.shape[-1])
            loss_sum = loss_sum + loss * wt
            multi_loss.append(loss)
        return loss_sum, multi_loss


class ContrastiveLoss(nn.Module):
    """InfoNCE on ready-made logits whose column 0 is the positive (losses.py:13-21): cross entropy against class 0.  The MoCo
    training path does not go through it -- ``contrastive.moco_nce`` produces logits, loss and gradient in one pass over the
    queue -- it is the loss the table names for ``MODEL.LOSS_FUNC: contrastive_loss`` and what the meters call on logits."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction = reduction

    def forward(self, inputs, dummy_labels=None):
        targets = torch.zeros(inputs.shape[0], dtype=torch.long, device=inputs.device)
        return nn.functional.cross_entropy(inputs, targets, reduction=self.reduction)


_LOSSES = {
    "cross_entropy": nn.CrossEntropyLoss,
    "bce": nn.BCELoss,
    "bce_logit": nn.BCEWithLogitsLoss,
    "soft_cross_entropy": partial(SoftTargetCrossEntropyLoss, normalize_targets=False),
    "contrastive_loss": ContrastiveLoss,
    "mse": nn.MSELoss,
    "multi_mse": MultipleMSELoss,
}


def get_loss_func(loss_name):
    """The loss class of ``cfg.MODEL.LOSS_FUNC``; instantiate it as ``get_loss_func(name)(reduction="mean")``."""
    if loss_name not in _LOSSES.keys():
        raise NotImplementedError("Loss {} is not supported".format(loss_name))
    return _LOSSES[loss_name]
