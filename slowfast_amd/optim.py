"""Optimizer + loss scaling on the flat gradient memory.

Replaces, for the GradReducer / TrainStep path, what tools/train_net.py:150-172 runs between ``loss.backward()`` and the
next iteration -- ``scaler.unscale_``, ``clip_grad_norm_`` / ``clip_grad_value_``, ``optimizer.get_grad_norm_``,
``scaler.step(optimizer)``, ``scaler.update()`` and ``misc.check_nan_losses`` -- and ``optimizer.step()`` itself
(slowfast/models/optimizer.py:100-140: SGD with momentum / dampening / Nesterov, AdamW).  Three libsfamd launches per
iteration (csrc/sf_optim.h), no host synchronisation: the dynamic loss scale, the overflow flag and the gradient norm live in
an 8-word control block in device memory.

Parameters are re-pointed to views of ONE flat fp32 buffer laid out like GradReducer.flat (gradients) and the optimizer
state, so the update is a single pass over contiguous memory.  ``param_groups`` mirrors torch.optim (lists of dicts with
"lr" / "weight_decay" / "layer_decay" / "apply_LARS"), so the reference's ``optim.set_lr(optimizer, lr)``
(slowfast/models/optimizer.py:251-259, ``set_lr`` below) keeps working on it.

Two update paths (FlatOptimizer.table_path).  Up to 8 groups without LARS: sf_flat_sgd / sf_flat_adamw, lr / weight decay as
kernel arguments.  More groups (SOLVER.LAYER_DECAY < 1 makes 2 * (MVIT.DEPTH + 2) of them) or LARS: sf_flat_sgd_tab /
sf_flat_adamw_tab read ``hyper`` -- a DEVICE table [ngroups][4] = lr, weight decay, lars_group, reserved -- so a new learning
rate reaches a captured launch on its next replay; LARS (optimizer.py:262-359) adds sf_flat_lars_trust (two launches: per-block
norms, per-parameter trust ratio) between the control launch and the update.
"""
from ctypes import c_float

import numpy as np
import torch

from . import engine
from .lib import get_lib

_SEG_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("group", "<i4"), ("pad", "<i4")])
_BLOCK = 1024       # elements per workgroup of the update kernels (SF_OPT_BLOCK_ELEMS)
_MAX_ARG_GROUPS = 8 # SF_OPT_MAX_GROUPS: what sf_flat_sgd / sf_flat_adamw carry by value
_SEG_LARS = 1       # segment flags word (the table's `pad`), bit 0: LARS adapts this parameter (it is not 1-D)
CTL_SCALE, CTL_TRACKER, CTL_FOUND_INF, CTL_GRAD_NORM, CTL_MULT, CTL_STEPS, CTL_SKIPPED = range(7)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None


class FlatOptimizer:
    def __init__(self, param_groups, reducer, method="sgd", momentum=0.0, dampening=0.0, nesterov=False, betas=(0.9, 0.999),
                 eps=1e-8, loss_scale=1.0, dynamic_loss_scale=False, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, clip_grad_l2norm=None, clip_grad_val=None, lars=False, trust_coefficient=0.001,
                 lars_eps=1e-8):
        assert method in ("sgd", "adamw")
        groups = [dict(g) for g in param_groups]
        assert len(groups) >= 1, "at least one parameter group"
        for g in groups:
            g.setdefault("layer_decay", 1.0)                # optimizer.py:58-77, :202-212
            g.setdefault("apply_LARS", bool(lars))          # LARS.step(): a group without the key is adapted
        self.param_groups = groups
        self.lars, self.trust_coefficient, self.lars_eps = bool(lars), float(trust_coefficient), float(lars_eps)
        assert not self.lars or (self.trust_coefficient > 0.0 and self.lars_eps >= 0.0)
        self.table_path = self.lars or len(groups) > _MAX_ARG_GROUPS
        self.method, self.momentum, self.dampening, self.nesterov = method, float(momentum), float(dampening), bool(nesterov)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.dynamic = bool(dynamic_loss_scale)
        self.growth, self.backoff, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        # tools/train_net.py:154-163: CLIP_GRAD_VAL takes precedence, the L2-norm clip only runs when no value clip is set
        self.clip_val = float(clip_grad_val) if clip_grad_val else 0.0
        self.clip_norm = float(clip_grad_l2norm) if (clip_grad_l2norm and not self.clip_val) else 0.0
        self.reducer = reducer
        flat_g = reducer.flat
        dev = flat_g.device
        group_of = {}
        for gi, g in enumerate(groups):
            for p in g["params"]:
                group_of[p] = gi
        # parameters become views of one flat buffer with the gradient buffer's layout
        self.flat_param = torch.empty_like(flat_g)
        segs, blk_seg, blk_off, seg_row = [], [], [], []
        self._seg_of = {}
        off = 0
        for p in reducer.params:
            n = p.numel()
            assert p in group_of, "every parameter of the reducer must belong to a parameter group"
            view = self.flat_param[off:off + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            si = self._seg_of[id(p)] = len(segs)
            segs.append((off, off + n, group_of[p], _SEG_LARS if p.dim() != 1 else 0))    # LARS(ignore_1d_param=True)
            seg_row.append(len(blk_seg))
            for b in range(0, n, _BLOCK):
                blk_seg.append(si)
                blk_off.append(b)
            off += n
        assert off == flat_g.numel()
        self.m1 = torch.zeros_like(flat_g) if (method == "adamw" or self.momentum != 0.0) else None
        self.m2 = torch.zeros_like(flat_g) if method == "adamw" else None
        self.segs = torch.from_numpy(np.array(segs, dtype=_SEG_DTYPE).view(np.uint8).copy()).to(dev)
        self.blk_seg = torch.tensor(blk_seg, dtype=torch.int32, device=dev)
        self.blk_off = torch.tensor(blk_off, dtype=torch.int32, device=dev)
        self.nblocks = len(blk_seg)
        self.ctl = torch.zeros(8, dtype=torch.float32, device=dev)
        self.ctl[CTL_SCALE] = float(loss_scale)
        self.init_loss_scale = float(loss_scale)
        # partial rows of the norm / overflow pass: one range per gradient bucket (finish_and_step), rows simply add up
        lib = get_lib()
        self._bucket_rows = []
        r = 0
        for s0, e0, _ in reducer.buckets:
            nb = lib.call("sf_flat_blocks", e0 - s0)
            self._bucket_rows.append((r, nb))
            r += nb
        self._part = torch.empty((max(r, lib.call("sf_flat_blocks", flat_g.numel())), 2), dtype=torch.float32, device=dev)
        self._rows_bucketed = r
        self.hyper = self._hyper_host = None
        if self.table_path:
            self.hyper = torch.zeros((len(groups), 4), dtype=torch.float32, device=dev)
            self._hyper_host = None                          # what `hyper` holds (numpy), None: nothing uploaded yet
            self._stage, self._stage_i = [None, None], 0     # pinned staging buffers + the event of their last upload
            self.sync_hyper()
        if self.lars:
            self.seg_row = torch.tensor(seg_row + [len(blk_seg)], dtype=torch.int32, device=dev)
            self.trust = torch.zeros(len(segs), dtype=torch.float32, device=dev)
            self._lars_part = torch.empty((self.nblocks, 2), dtype=torch.float64, device=dev)

    # -- what the training loop touches ---------------------------------------------------------------------------
    @property
    def loss_scale(self):
        """0-d device tensor: multiply the loss by it (``(loss * opt.loss_scale).backward()``); under a captured graph the
        replay reads the current value from device memory, so a scale change needs no re-capture."""
        return self.ctl[CTL_SCALE]

    @property
    def grad_norm(self):
        """Global L2 norm of the unscaled, rank-averaged gradients of the last step (device tensor; inf on overflow)."""
        return self.ctl[CTL_GRAD_NORM]

    @property
    def found_inf(self):
        return self.ctl[CTL_FOUND_INF]

    def _hyper_rows(self):
        return np.array([[float(g["lr"]), float(g.get("weight_decay", 0.0)), float(self.lars and bool(g["apply_LARS"])), 0.0]
                         for g in self.param_groups], dtype=np.float32)

    def sync_hyper(self):
        """Upload lr / weight decay / LARS membership of ``param_groups`` into the device table the table-driven kernels read,
        if a value changed since the last upload.  step() calls it; call it yourself between replays of a graph that captured
        step() (never inside a capture: the upload is a copy, not a kernel).  The copy is asynchronous on the current stream
        from one of two pinned staging buffers, so a per-iteration learning-rate schedule costs no host synchronisation."""
        if not self.table_path:
            return False
        rows = self._hyper_rows()
        if self._hyper_host is not None and np.array_equal(rows, self._hyper_host):
            return False
        if self.hyper.is_cuda:
            assert not torch.cuda.is_current_stream_capturing(), "sync_hyper() inside a graph capture"
            i = self._stage_i = self._stage_i ^ 1
            if self._stage[i] is None:
                self._stage[i] = [torch.empty(rows.shape, dtype=torch.float32).pin_memory(), None]
            buf, ev = self._stage[i]
            if ev is not None:
                ev.synchronize()                             # two uploads ago: long done
            buf.copy_(torch.from_numpy(rows))
            self.hyper.copy_(buf, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.hyper.device))
            self._stage[i][1] = ev
        else:
            self.hyper.copy_(torch.from_numpy(rows))
        self._hyper_host = rows
        return True

    def trust_ratio(self, p):
        """LARS trust ratio parameter ``p`` took in the last clean step (0-d device tensor; 0: its gradient was not scaled)."""
        return self.trust[self._seg_of[id(p)]]

    def _sumsq_bucket(self, bi):
        """Bucket bi's share of the norm / overflow pass (its own rows of the partial table)."""
        s0, e0, _ = self.reducer.buckets[bi]
        r0, _ = self._bucket_rows[bi]
        g = self.reducer.flat
        get_lib().call("sf_flat_sumsq", g.data_ptr() + 4 * s0, e0 - s0, self._part.data_ptr() + 8 * r0, _stream(g),
                       work=dict(bytes=4.0 * (e0 - s0)))

    def finish_and_step(self):
        """GradReducer.finish(loss_scale=None) + step(), with the norm / overflow pass taken bucket by bucket as the collectives
        complete: the pass over the early buckets runs under the exchange of the late ones, and the update waits only for the
        control launch (only the ~30 us pass moves -- the update itself needs the global norm)."""
        self.reducer.finish(loss_scale=None, on_bucket=self._sumsq_bucket)
        self.step(_sumsq_rows=self._rows_bucketed)

    def step(self, _sumsq_rows=None):
        """Call after the gradient all-reduce finished (GradReducer.finish(loss_scale=None)): norm + overflow check,
        GradScaler update, clipped / unscaled parameter update -- skipped as a whole on overflow.  ``_sumsq_rows``: the partial
        table already holds that many rows (finish_and_step)."""
        lib, g = get_lib(), self.reducer.flat
        s = _stream(g)
        nrows = _sumsq_rows
        if nrows is None:
            nrows = lib.call("sf_flat_blocks", g.numel())
            lib.call("sf_flat_sumsq", g.data_ptr(), g.numel(), self._part.data_ptr(), s, work=dict(bytes=4.0 * g.numel()))
        lib.call("sf_step_control", self._part.data_ptr(), nrows, self.ctl.data_ptr(), float(self.reducer.world),
                 self.clip_norm, int(self.dynamic), self.growth, self.backoff, self.growth_interval, s)
        if self.table_path:
            self._step_table(lib, g, s)
            engine.PARAM_EPOCH += 1
            return
        ng = len(self.param_groups)
        lr = (c_float * ng)(*[float(gp["lr"]) for gp in self.param_groups])
        wd = (c_float * ng)(*[float(gp.get("weight_decay", 0.0)) for gp in self.param_groups])
        if self.method == "sgd":
            lib.call("sf_flat_sgd", self.flat_param.data_ptr(), g.data_ptr(), self.m1.data_ptr() if self.m1 is not None else None,
                     self.segs.data_ptr(), self.blk_seg.data_ptr(), self.blk_off.data_ptr(), self.nblocks, self.ctl.data_ptr(),
                     lr, wd, ng, self.clip_val, self.momentum, self.dampening, int(self.nesterov), s,
                     work=dict(bytes=4.0 * g.numel() * (3 + 2 * int(self.m1 is not None))))
        else:
            lib.call("sf_flat_adamw", self.flat_param.data_ptr(), g.data_ptr(), self.m1.data_ptr(), self.m2.data_ptr(),
                     self.segs.data_ptr(), self.blk_seg.data_ptr(), self.blk_off.data_ptr(), self.nblocks, self.ctl.data_ptr(),
                     lr, wd, ng, self.clip_val, self.betas[0], self.betas[1], self.eps, s, work=dict(bytes=4.0 * g.numel() * 7))
        engine.PARAM_EPOCH += 1         # the kernels wrote the parameters without bumping tensor._version: packed-weight
                                        # caches of the eager path must not be reused (a captured graph re-packs anyway)

    def _step_table(self, lib, g, s):
        """[LARS trust ratios +] table-driven update: hyper-parameters from device memory."""
        if not (g.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.sync_hyper()
        n = g.numel()
        tables = (self.segs.data_ptr(), self.blk_seg.data_ptr(), self.blk_off.data_ptr(), self.nblocks)
        trust = None
        if self.lars:
            lib.call("sf_flat_lars_trust", self.flat_param.data_ptr(), g.data_ptr(), *tables, self.seg_row.data_ptr(),
                     self.trust.numel(), self.ctl.data_ptr(), self.hyper.data_ptr(), self._lars_part.data_ptr(),
                     self.trust.data_ptr(), self.clip_val, self.trust_coefficient, self.lars_eps, s, work=dict(bytes=8.0 * n))
            trust = self.trust.data_ptr()
        if self.method == "sgd":
            lib.call("sf_flat_sgd_tab", self.flat_param.data_ptr(), g.data_ptr(), self.m1.data_ptr() if self.m1 is not None else None,
                     *tables, self.ctl.data_ptr(), self.hyper.data_ptr(), trust, self.clip_val, self.momentum, self.dampening,
                     int(self.nesterov), s, work=dict(bytes=4.0 * n * (3 + 2 * int(self.m1 is not None))))
        else:
            lib.call("sf_flat_adamw_tab", self.flat_param.data_ptr(), g.data_ptr(), self.m1.data_ptr(), self.m2.data_ptr(),
                     *tables, self.ctl.data_ptr(), self.hyper.data_ptr(), trust, self.clip_val, self.betas[0], self.betas[1],
                     self.eps, s, work=dict(bytes=4.0 * n * 7))

    def zero_grad(self, set_to_none=False):
        self.reducer.zero_grad()

    # -- checkpoint surface (utils/checkpoint.py saves optimizer.state_dict()) ---------------------------------------------
    def state_dict(self):
        return {"ctl": self.ctl.detach().cpu(), "m1": None if self.m1 is None else self.m1.detach().cpu(),
                "m2": None if self.m2 is None else self.m2.detach().cpu(),
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        self.ctl.copy_(sd["ctl"])
        if self.m1 is not None and sd.get("m1") is not None:
            self.m1.copy_(sd["m1"])
        if self.m2 is not None and sd.get("m2") is not None:
            self.m2.copy_(sd["m2"])
        for g, s in zip(self.param_groups, sd.get("param_groups", [])):
            g.update(s)


def _flat_groups(inner, cfg, lr, lars):
    """The LAYER_DECAY == 1 grouping (slowfast/models/optimizer.py:27-78)."""
    skip = inner.no_weight_decay() if hasattr(inner, "no_weight_decay") else ()
    bn, rest, zero = [], [], []
    seen = set()
    for name_m, m in inner.named_modules():
        is_bn = isinstance(m, torch.nn.modules.batchnorm._NormBase)
        for name_p, p in m.named_parameters(recurse=False):
            name = "{}.{}".format(name_m, name_p).strip(".")
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            if is_bn:
                bn.append(p)
            elif any(k in name for k in skip):
                zero.append(p)
            elif cfg.SOLVER.ZERO_WD_1D_PARAM and (p.dim() == 1 or name.endswith(".bias")):
                zero.append(p)
            else:
                rest.append(p)
    return [g for g in ({"params": bn, "weight_decay": cfg.BN.WEIGHT_DECAY, "lr": lr, "layer_decay": 1.0, "apply_LARS": False},
                        {"params": rest, "weight_decay": cfg.SOLVER.WEIGHT_DECAY, "lr": lr, "layer_decay": 1.0, "apply_LARS": lars},
                        {"params": zero, "weight_decay": 0.0, "lr": lr, "layer_decay": 1.0, "apply_LARS": lars}) if g["params"]]


def set_lr(optimizer, new_lr):
    """slowfast/models/optimizer.py:251-259: every group's lr becomes ``new_lr * group["layer_decay"]`` (the per-layer scale of
    SOLVER.LAYER_DECAY is applied here and nowhere else).  On the table path the new values reach the device with the next
    step() / sync_hyper()."""
    for param_group in optimizer.param_groups:
        param_group["lr"] = new_lr * param_group["layer_decay"]


def _layer_decay_groups(inner, cfg):
    """get_param_groups (slowfast/models/optimizer.py:146-237): one group per (layer id, decayed or not), in order of first
    appearance; layer ids cls_token / mask_token / pos_embed* / patch_embed* -> 0, blocks.N.* -> N + 1, the rest
    MVIT.DEPTH + 1; ``layer_decay = SOLVER.LAYER_DECAY ** (MVIT.DEPTH + 1 - layer id)``.  ``name in skip`` is an exact match
    here (the LAYER_DECAY == 1 branch tests substrings)."""
    for m in inner.modules():
        assert not isinstance(m, torch.nn.modules.batchnorm._NormBase), "BN is not supported with layer decay"
    depth, decay = int(cfg.MVIT.DEPTH), float(cfg.SOLVER.LAYER_DECAY)
    skip = inner.no_weight_decay() if hasattr(inner, "no_weight_decay") else {}

    def layer_id(name):
        if name in ("cls_token", "mask_token") or name.startswith("pos_embed") or name.startswith("patch_embed"):
            return 0
        if name.startswith("blocks"):
            return int(name.split(".")[1]) + 1
        return depth + 1

    groups, counted = {}, 0
    for name, p in inner.named_parameters():
        counted += 1
        if not p.requires_grad:
            continue
        name = name[len("module."):] if name.startswith("module.") else name
        zero = name in skip or ((p.dim() == 1 or name.endswith(".bias")) and cfg.SOLVER.ZERO_WD_1D_PARAM)
        lid = layer_id(name)
        key = "layer_%d_%s" % (lid, "zero" if zero else "non_bn")
        if key not in groups:
            groups[key] = {"params": [], "weight_decay": 0.0 if zero else cfg.SOLVER.WEIGHT_DECAY,
                           "layer_decay": decay ** (depth + 1 - lid)}
        groups[key]["params"].append(p)
    assert counted == len(list(inner.parameters())), "parameter size does not match"
    return list(groups.values())


def construct_optimizer(model, cfg, reducer, loss_scale=1.0, dynamic_loss_scale=None):
    """FlatOptimizer configured as slowfast/models/optimizer.py:9-143 configures torch's.

    ``SOLVER.LAYER_DECAY == 1`` (:26-92): BatchNorm parameters get BN.WEIGHT_DECAY; parameters whose dotted name contains an
    entry of ``model.no_weight_decay()`` (MViT: pos_embed* / rel_pos_* / cls_token under MVIT.ZERO_DECAY_POS_CLS) get no decay;
    so do 1-D parameters and every ``*.bias`` when SOLVER.ZERO_WD_1D_PARAM; the rest SOLVER.WEIGHT_DECAY.  Every group carries
    ``layer_decay 1.0`` and ``apply_LARS`` (False for BatchNorm, SOLVER.LARS_ON for the other two).
    ``0 < SOLVER.LAYER_DECAY < 1`` (:146-237, get_param_groups): one group per layer id and decay class, each with its
    ``layer_decay``; the lr of every group starts at BASE_LR and the per-layer scale is applied by ``set_lr`` -- as in the
    reference.  These are more than 8 groups for any real depth: FlatOptimizer takes its table-driven path.
    SOLVER.LARS_ON (:141-142, :262-359): ``FlatOptimizer(lars=True, trust_coefficient=0.001)``, clip=False semantics.
    SOLVER.OPTIMIZING_METHOD "sgd" (momentum / dampening / nesterov) or "adamw" / "mt_adamw" (SOLVER.BETAS, eps 1e-8);
    clipping from SOLVER.CLIP_GRAD_L2NORM / CLIP_GRAD_VAL; the dynamic loss scale defaults to TRAIN.MIXED_PRECISION
    (GradScaler's constants).  "adam" (L2-coupled decay) is not built into the fused kernels and raises instead of silently
    changing the update rule."""
    layer_decay = float(cfg.SOLVER.get("LAYER_DECAY", 1.0))
    if not 0.0 < layer_decay <= 1.0:
        raise ValueError("Layer decay should be in (0, 1], but is {}".format(layer_decay))
    lars = bool(cfg.SOLVER.get("LARS_ON", False))
    inner = model.module if hasattr(model, "module") and isinstance(model.module, torch.nn.Module) else model
    lr = cfg.SOLVER.BASE_LR
    if layer_decay != 1.0:
        groups = _layer_decay_groups(inner, cfg)
        for g in groups:
            g["lr"] = lr
    else:
        groups = _flat_groups(inner, cfg, lr, lars)
    dyn = bool(cfg.TRAIN.MIXED_PRECISION) if dynamic_loss_scale is None else dynamic_loss_scale
    kw = dict(loss_scale=loss_scale, dynamic_loss_scale=dyn, clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM,
              clip_grad_val=cfg.SOLVER.CLIP_GRAD_VAL, lars=lars, trust_coefficient=0.001)
    method = cfg.SOLVER.OPTIMIZING_METHOD
    if method in ("adamw", "mt_adamw"):
        betas = tuple(cfg.SOLVER.get("BETAS", (0.9, 0.999)))
        return FlatOptimizer(groups, reducer, method="adamw", betas=betas, eps=1e-8, **kw)
    if method == "sgd":
        return FlatOptimizer(groups, reducer, method="sgd", momentum=cfg.SOLVER.MOMENTUM, dampening=cfg.SOLVER.DAMPENING,
                             nesterov=cfg.SOLVER.NESTEROV, **kw)
    raise NotImplementedError("Does not support {} optimizer".format(method))
