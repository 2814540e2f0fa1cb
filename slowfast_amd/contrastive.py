"""MoCo, BYOL and SimCLR pre-training (slowfast/models/contrastive.py, tools/train_net.py:118-172): ``ContrastiveModel`` with
``CONTRASTIVE.TYPE == "moco"``, ``"byol"`` or ``"simclr"`` on the engine's backbones, on one device, and the step glue the reference runs as
torch ops on the device.

Per iteration the reference makes three passes per parameter tensor for the momentum update, four small passes per feature matrix
for ``Normalize``, an ``einsum`` against a clone of the queue, an ``einsum`` / ``unsqueeze`` / ``cat`` per key view, a ``cat``
over views, a ``div`` and ``CrossEntropyLoss`` (whose backward reads the probabilities and the queue again), and synchronises the
host on ``int(self.ptr.item())``.  Here (csrc/sf_moco.h, all fp32, no floating-point atomics):

* ``l2norm_rows``  one launch: ``x / |x|`` per row, gathering through the ``_batch_unshuffle`` permutation when given.  No epsilon,
  as ``Normalize`` has none: a zero row gives NaN.
* ``moco_nce``     two launches: the logits in the reference's row order (view-major), the loss, and d(loss)/d(f) for the raw
  query features, from ONE pass over the queue.  ``MoCoNceFn.backward`` is ``grad_out * df``.
* ``enqueue``      one launch: the ring write of ``_dequeue_and_enqueue``; pointer and error word live in device memory.
* ``ema_update``   one launch over the flat parameter memory: ``hist = p * (1 - m) + hist * m`` with torch's bits.

Nothing reads ``ptr`` or ``iter`` back per iteration: the iteration-0 copy ``hist = p`` is decided from a host mirror of
``iter`` (refreshed by ``load_state_dict``), and a pointer that would leave the queue turns the enqueue into a no-op that
raises an error word the host looks at where it synchronises anyway (``state_dict()``, ``eval()``).

BYOL (``TYPE == "byol"``: predictor heads on the projection, no queue in the loss, no batch shuffle) shares the momentum
encoder, the annealing and ``l2norm_rows`` for the keys.  Its loss is, per key view, ``Normalize`` of the predictor output, an
``einsum``, a ``div``, a ``mean`` and a negation, then a sum over views and a division, with the autograd mirror of each.  Here
(csrc/sf_byol.h, fp32, no floating-point atomics):

* ``byol_sim``     two launches: the loss of one query against all its key views and d(loss)/d(p) for the RAW predictor output.
  ``ByolSimFn.backward`` is ``grad_out * df``.

SimCLR (``TYPE == "simclr"``: no momentum encoder, no queue) runs two query forwards per pair of adjacent crops.  Its loss is
``cat``, ``mm``, ``exp``, an off-diagonal mask, ``masked_select`` (a data-dependent shape: a host synchronisation that cannot be
captured), ``sum``, the positives, ``div``, ``log``, ``mean`` and autograd back through all of them.  Here (csrc/sf_simclr.h,
fp32, no floating-point atomics):

* ``simclr_ntxent`` three launches: the loss over the 2 n rows of both crops and d(loss)/d(a), d(loss)/d(b) for the RAW head
  outputs; ``Normalize(a)`` for the kNN memory comes out of the first launch.  ``SimclrNtXentFn.backward`` scales the two
  stored gradients by ``grad_out``.

The dummy logits the reference builds twice per step (9999 in column 0) are built once per (rows, QUEUE_LEN, device).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import engine, ops
from .lib import SfError, get_lib
from .losses import get_loss_func
from .registry import MODEL_REGISTRY
from .video_models import ResNet, SlowFast

_MODEL_TYPES = {"slowfast": SlowFast, "slow": ResNet, "c2d": ResNet, "i3d": ResNet, "slow_c2d": ResNet}
_UNSUPPORTED_TYPES = ("mem", "self", "swav")


def _dense_f32(t, what, dim=2):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == dim and t.is_contiguous()):
        raise SfError("%s must be a dense float32 %d-D tensor (got %s)" % (
            what, dim, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    return t


def _host_perm(perm, n):
    """The ``_batch_unshuffle`` gather as int32, checked on the host to be a permutation of 0 .. n-1 (the kernel reads row
    perm[r] without looking at it again)."""
    p = torch.as_tensor(perm)
    if p.is_cuda:
        raise SfError("l2norm_rows: perm is checked on the host before upload: pass a host tensor")
    p = p.reshape(-1).to(torch.int64)
    if p.numel() != n or not torch.equal(torch.sort(p).values, torch.arange(n)):
        raise SfError("l2norm_rows: perm is not a permutation of 0 .. %d" % (n - 1))
    return p.to(torch.int32)


def l2norm_rows(x, perm=None):
    """``Normalize()(x)[perm]`` for a float32 (n, C) matrix whose rows may be pitched (``x.stride(0) >= C``)."""
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]):
        raise SfError("l2norm_rows: x must be a float32 (n, C) matrix with unit column stride")
    stream = ops._stream(x)
    n, C = x.shape
    idx = None if perm is None else _host_perm(perm, n).to(x.device)
    out = torch.empty((n, C), dtype=torch.float32, device=x.device)
    get_lib().call("sf_l2norm_rows", n, C, x.data_ptr(), x.stride(0), ops._ptr(idx), out.data_ptr(), stream,
                   work=dict(bytes=8.0 * n * C))
    return out


_workspaces = {}


def _workspace(device, n, V, K, C):
    """Per-slab softmax partials of the fused loss, allocated once per shape."""
    key = (device, n, V, K, C)
    ws = _workspaces.get(key)
    if ws is None:
        nbytes = get_lib().call("sf_moco_nce_workspace", n, V, K, C)
        ws = _workspaces[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return ws


class MoCoNceFn(torch.autograd.Function):
    """(logits, loss) = f(raw query features (n, C), normalised keys (V, n, C), queue (K, C), T); differentiable w.r.t. the
    query features through the loss only (the reference's logits are a training-meter input, detached there too)."""

    @staticmethod
    def forward(ctx, f, keys, queue, T):
        _dense_f32(f, "moco_nce: f")
        _dense_f32(keys, "moco_nce: keys", 3)
        _dense_f32(queue, "moco_nce: queue")
        stream = ops._stream(f)
        n, C = f.shape
        V, K = keys.shape[0], queue.shape[0]
        if tuple(keys.shape[1:]) != (n, C) or queue.shape[1] != C or keys.device != f.device or queue.device != f.device:
            raise SfError("moco_nce: keys %s / queue %s do not match f %s" % (tuple(keys.shape), tuple(queue.shape), tuple(f.shape)))
        lib = get_lib()
        ws = _workspace(f.device, n, V, K, C)          # raises for a shape the kernels do not take, before anything is allocated
        logits = torch.empty((V * n, 1 + K), dtype=torch.float32, device=f.device)
        df = torch.empty_like(f)
        loss = torch.empty((1,), dtype=torch.float32, device=f.device)
        args = (n, V, K, C, f.data_ptr(), keys.data_ptr(), queue.data_ptr(), 1.0 / float(T), logits.data_ptr(), df.data_ptr(),
                loss.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream)
        lib.call("sf_moco_nce_slabs", *args, work=dict(bytes=4.0 * (K * C + V * n * K), flops=4.0 * n * K * C))
        lib.call("sf_moco_nce_finalize", *args, work=dict(bytes=1.0 * ws.numel() * 4))
        ctx.save_for_backward(df)
        ctx.mark_non_differentiable(logits)
        return logits, loss.view(())

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        (df,) = ctx.saved_tensors
        return dloss * df, None, None, None


def moco_nce(f, keys, queue, T):
    """The moco branch of ``ContrastiveModel.forward`` after the backbone: ``keys`` is a (V, n, C) tensor or a list of V
    normalised (n, C) key matrices.  Returns (logits (V n, 1 + K), loss)."""
    if not torch.is_tensor(keys):
        keys = torch.stack([k for k in keys], 0)
    return MoCoNceFn.apply(f, keys.detach(), queue.detach(), T)


_byol_workspaces = {}


def _byol_workspace(device, n, V, C):
    """Per-row loss terms of ``byol_sim``, allocated once per shape."""
    key = (device, n, V, C)
    ws = _byol_workspaces.get(key)
    if ws is None:
        nbytes = get_lib().call("sf_byol_sim_workspace", n, V, C)
        ws = _byol_workspaces[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return ws


class ByolSimFn(torch.autograd.Function):
    """loss = f(raw predictor output p (n, C), normalised keys (V, n, C), T): ``sum_v sim_loss(Normalize(p), key_v) / V`` of the
    byol branch; differentiable w.r.t. p.  The rows of p may be pitched (``p.stride(0) >= C``)."""

    @staticmethod
    def forward(ctx, p, keys, T):
        if not (torch.is_tensor(p) and p.dtype == torch.float32 and p.dim() == 2 and p.stride(1) == 1 and p.stride(0) >= p.shape[1]):
            raise SfError("byol_sim: p must be a float32 (n, C) matrix with unit column stride (got %s)" % (
                "%s %s" % (p.dtype, tuple(p.shape)) if torch.is_tensor(p) else type(p).__name__,))
        _dense_f32(keys, "byol_sim: keys", 3)
        stream = ops._stream(p)
        n, C = p.shape
        V = keys.shape[0]
        if tuple(keys.shape[1:]) != (n, C) or keys.device != p.device:
            raise SfError("byol_sim: keys %s do not match p %s" % (tuple(keys.shape), tuple(p.shape)))
        lib = get_lib()
        ws = _byol_workspace(p.device, n, V, C)         # raises for a shape the kernels do not take, before anything is allocated
        df = torch.empty((n, C), dtype=torch.float32, device=p.device)
        loss = torch.empty((1,), dtype=torch.float32, device=p.device)
        args = (n, V, C, p.data_ptr(), p.stride(0), keys.data_ptr(), 1.0 / float(T), df.data_ptr(), loss.data_ptr(),
                ws.data_ptr(), ws.numel() * 4, stream)
        lib.call("sf_byol_sim_rows", *args, work=dict(bytes=4.0 * n * C * (V + 2), flops=4.0 * n * C * (V + 1)))
        lib.call("sf_byol_sim_finalize", *args, work=dict(bytes=4.0 * n))
        ctx.save_for_backward(df)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        (df,) = ctx.saved_tensors
        return dloss * df, None, None


def byol_sim(p, keys, T):
    """The loss of the byol branch of ``ContrastiveModel.forward`` for one query: ``p`` is the RAW predictor output (the
    normalisation and its backward are inside), ``keys`` a (V, n, C) tensor or a list of V normalised (n, C) key matrices."""
    if not torch.is_tensor(keys):
        keys = list(keys)
        if not keys:
            raise SfError("byol_sim: no key views")
        keys = keys[0].unsqueeze(0) if len(keys) == 1 else torch.stack(keys, 0)
    return ByolSimFn.apply(p, keys.detach(), T)


_simclr_workspaces = {}


def _simclr_workspace(device, n, C):
    """q, the norms, D, the row terms and the M x M matrix E of ``simclr_ntxent``, allocated once per shape.  Scratch only: what
    a call returns (loss, da, db, q) lives in tensors of its own, so a later call of the same shape invalidates nothing."""
    key = (device, n, C)
    ws = _simclr_workspaces.get(key)
    if ws is None:
        nbytes = get_lib().call("sf_simclr_workspace", n, C)
        ws = _simclr_workspaces[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return ws


def _pitched_f32(t, what):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        raise SfError("%s must be a float32 (n, C) matrix with unit column stride (got %s)" % (
            what, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    return t


class SimclrNtXentFn(torch.autograd.Function):
    """(loss, q) = f(raw features a (n, C), raw features b (n, C), T): the NT-Xent loss of the simclr branch over the 2 n rows
    of [a; b], differentiable w.r.t. a and b; q = Normalize(a) (not differentiable: the kNN memory's input) or None.  The rows
    of a and b may be pitched (``stride(0) >= C``, each its own).  Three launches (csrc/sf_simclr.h); both gradients are
    computed here and kept for the backward, which scales them."""

    @staticmethod
    def forward(ctx, a, b, T, want_q):
        _pitched_f32(a, "simclr_ntxent: a")
        _pitched_f32(b, "simclr_ntxent: b")
        stream = ops._stream(a)
        n, C = a.shape
        if tuple(b.shape) != (n, C) or b.device != a.device:
            raise SfError("simclr_ntxent: b %s on %s does not match a %s on %s" % (tuple(b.shape), b.device, tuple(a.shape), a.device))
        lib = get_lib()
        ws = _simclr_workspace(a.device, n, C)          # raises for a shape the kernels do not take, before anything is allocated
        da = torch.empty((n, C), dtype=torch.float32, device=a.device)
        db = torch.empty((n, C), dtype=torch.float32, device=a.device)
        loss = torch.empty((1,), dtype=torch.float32, device=a.device)
        q = torch.empty((n, C), dtype=torch.float32, device=a.device) if want_q else None
        M = 2 * n
        args = (n, C, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), 1.0 / float(T), da.data_ptr(), db.data_ptr(),
                loss.data_ptr(), ops._ptr(q), ws.data_ptr(), ws.numel() * 4, stream)
        lib.call("sf_simclr_norm", *args, work=dict(bytes=8.0 * M * C))
        lib.call("sf_simclr_rows", *args, work=dict(bytes=4.0 * (M * C + M * M), flops=2.0 * M * M * C))
        lib.call("sf_simclr_grad", *args, work=dict(bytes=4.0 * (2 * M * C + M * M), flops=2.0 * M * M * C))
        ctx.save_for_backward(da, db)
        if want_q:
            ctx.mark_non_differentiable(q)
        return loss.view(()), q

    @staticmethod
    def backward(ctx, dloss, _dq):
        da, db = ctx.saved_tensors
        return dloss * da, dloss * db, None, None


def simclr_ntxent(a, b, T, return_q=False):
    """The loss of the simclr branch of ``ContrastiveModel.forward`` after the two backbone calls: ``a`` and ``b`` are the RAW
    head outputs of ``clips[0]`` and ``clips[1]`` (both normalisations and their backward are inside).  Returns the loss, or
    (loss, Normalize(a)) with ``return_q``."""
    loss, q = SimclrNtXentFn.apply(a, b, T, bool(return_q))
    return (loss, q) if return_q else loss


_err_words = {}


def queue_error_word(device):
    """The device int32 [1] the enqueue kernel raises (one per device unless a caller brings its own)."""
    w = _err_words.get(device)
    if w is None:
        w = _err_words[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return w


def enqueue(queue, ptr, keys_list, err=None):
    """``_dequeue_and_enqueue``: the key matrices of ``keys_list`` (each (rows, C)) are written at the device pointer one after
    the other, the pointer wrapping to 0 at the end of the queue.  One launch, no read-back."""
    _dense_f32(queue, "enqueue: queue")
    stream = ops._stream(queue)
    keys_list = list(keys_list) if not torch.is_tensor(keys_list) else [keys_list]
    assert len(keys_list) > 0, "need to have multiple views for adding them to queue"
    K, C = queue.shape
    rows = int(keys_list[0].shape[0])
    if rows <= 0 or K % rows != 0:
        raise SfError("enqueue: K %% rows != 0 (K=%d, rows=%d)" % (K, rows))
    for k in keys_list:
        if tuple(k.shape) != (rows, C) or k.dtype != torch.float32 or k.device != queue.device:
            raise SfError("enqueue: every key matrix must be float32 (%d, %d) on the queue's device" % (rows, C))
    keys = keys_list[0].contiguous() if len(keys_list) == 1 else torch.cat(keys_list, 0)
    if not (ptr.dtype == torch.int64 and ptr.numel() == 1 and ptr.device == queue.device):
        raise SfError("enqueue: ptr must be an int64 [1] tensor on the queue's device")
    err = queue_error_word(queue.device) if err is None else err
    get_lib().call("sf_queue_enqueue", K, C, rows, len(keys_list), keys.data_ptr(), queue.data_ptr(), ptr.data_ptr(),
                   err.data_ptr(), stream, work=dict(bytes=8.0 * keys.numel()))


def check_queue_error(err=None, device=None):
    """Reads the error word (a host synchronisation: call it where one happens anyway) and raises if an enqueue found its
    pointer outside the queue; the word is cleared."""
    err = queue_error_word(device) if err is None else err
    if int(err.item()) != 0:
        err.zero_()
        raise SfError("enqueue: a queue pointer outside [0, K - rows] was found; that call wrote nothing")


def momentum_words(m):
    """(fp32(m), fp32(1.0 - m)): the two scalars of ``p * (1.0 - m) + hist * m``, the difference taken in double."""
    m = float(m)
    return torch.tensor([m, 1.0 - m], dtype=torch.float64).to(torch.float32)


def ema_update(p_flat, hist_flat, mm):
    """hist = fl(fl(p * mm[1]) + fl(hist * mm[0])) in place over two float32 buffers of one size; ``mm`` = device float [2]."""
    if not (torch.is_tensor(p_flat) and torch.is_tensor(hist_flat) and p_flat.dtype == hist_flat.dtype == torch.float32
            and p_flat.numel() == hist_flat.numel() and p_flat.is_contiguous() and hist_flat.is_contiguous()
            and p_flat.device == hist_flat.device == mm.device and mm.dtype == torch.float32 and mm.numel() == 2):
        raise SfError("ema_update: p and hist must be dense float32 buffers of one size, mm a float32 [2] tensor, on one device")
    stream = ops._stream(hist_flat)
    n = hist_flat.numel()
    if n:
        get_lib().call("sf_ema_update", n, p_flat.data_ptr(), hist_flat.data_ptr(), mm.data_ptr(), stream,
                       work=dict(bytes=12.0 * n))


def _normalize(x, dim):
    return x.div(x.pow(2).sum(dim, keepdim=True).pow(0.5))


class Memory(nn.Module):
    """The kNN memory bank (contrastive.py:887-987) on plain torch ops: it is touched once per iteration with a batch of rows."""

    def __init__(self, length, duration, dim, cfg):
        super().__init__()
        self.length, self.duration, self.dim = length, duration, dim
        stdv = 1.0 / math.sqrt(dim / 3)
        self.register_buffer("memory", torch.rand(length, duration, dim).mul_(2 * stdv).add_(-stdv))
        self.num_gpus = cfg.NUM_GPUS

    def resize(self, length, duration, dim):
        self.length, self.duration, self.dim = length, duration, dim
        stdv = 1.0 / math.sqrt(dim / 3)
        device = self.memory.device
        del self.memory
        self.memory = torch.rand(length, duration, dim).mul_(2 * stdv).add_(-stdv).to(device)

    def get(self, ind, time, interp=False):
        if interp:
            raise NotImplementedError("CONTRASTIVE.INTERP_MEMORY")
        with torch.no_grad():
            sel = self.memory[ind.view(-1), time.long().view(-1), :]
        return sel.view(ind.size(0), -1, self.dim)

    def update(self, mem, momentum, ind, time, interp=False):
        if interp:
            raise NotImplementedError("CONTRASTIVE.INTERP_MEMORY")
        with torch.no_grad():
            mem = mem.view(mem.size(0), 1, -1)
            old = self.get(ind, time)
            new = _normalize(mem * momentum + old * (1 - momentum), 2)
            self.memory[ind.view(-1), time.long().view(-1), :] = new.squeeze()

    def forward(self, inputs):
        pass


def _check_cfg(cfg):
    c = cfg.CONTRASTIVE
    if c.TYPE in _UNSUPPORTED_TYPES:
        raise NotImplementedError("CONTRASTIVE.TYPE %r: only \"moco\", \"byol\" and \"simclr\" run on this engine" % (c.TYPE,))
    if c.TYPE not in ("moco", "byol", "simclr"):
        raise NotImplementedError("CONTRASTIVE.TYPE %r" % (c.TYPE,))
    if c.TYPE == "byol":
        depths = list(c.PREDICTOR_DEPTHS)
        if not depths:                      # the reference raises the same kind of error in forward (contrastive.py:514)
            raise NotImplementedError("CONTRASTIVE.TYPE \"byol\": the predictor is missing (no depth in PREDICTOR_DEPTHS)")
        if len(depths) != 1:                # the reference asserts len(predictors) == 1 in forward (:515)
            raise NotImplementedError("CONTRASTIVE.PREDICTOR_DEPTHS %r: BYOL takes exactly one predictor" % (depths,))
        if c.BN_SYNC_MLP and (cfg.BN.NUM_SYNC_DEVICES != 1 or cfg.BN.GLOBAL_SYNC):
            raise NotImplementedError("CONTRASTIVE.BN_SYNC_MLP with BN.NUM_SYNC_DEVICES %d, BN.GLOBAL_SYNC %s: the MLP heads' "
                                      "BatchNorm is per device" % (cfg.BN.NUM_SYNC_DEVICES, bool(cfg.BN.GLOBAL_SYNC)))
    elif c.TYPE == "simclr":
        if list(c.PREDICTOR_DEPTHS):
            raise NotImplementedError("CONTRASTIVE.TYPE \"simclr\" with CONTRASTIVE.PREDICTOR_DEPTHS %r: predictor heads belong to "
                                      "BYOL" % (list(c.PREDICTOR_DEPTHS),))
        if c.MOCO_MULTI_VIEW_QUEUE:         # a MoCo key: SimCLR has no queue, a recipe that sets it is a mistake
            raise NotImplementedError("CONTRASTIVE.TYPE \"simclr\" with CONTRASTIVE.MOCO_MULTI_VIEW_QUEUE: SimCLR has no queue")
        if c.BN_SYNC_MLP and (cfg.BN.NUM_SYNC_DEVICES != 1 or cfg.BN.GLOBAL_SYNC):
            raise NotImplementedError("CONTRASTIVE.BN_SYNC_MLP with BN.NUM_SYNC_DEVICES %d, BN.GLOBAL_SYNC %s: the MLP heads' "
                                      "BatchNorm is per device" % (cfg.BN.NUM_SYNC_DEVICES, bool(cfg.BN.GLOBAL_SYNC)))
        if cfg.NUM_GPUS * cfg.NUM_SHARDS > 1:
            raise NotImplementedError("NUM_GPUS * NUM_SHARDS > 1: the cross-rank gather of the features (AllGatherWithGradient) "
                                      "is not built")
    else:
        if list(c.PREDICTOR_DEPTHS):
            raise NotImplementedError("CONTRASTIVE.PREDICTOR_DEPTHS: predictor heads belong to BYOL")
        if c.BN_SYNC_MLP:
            raise NotImplementedError("CONTRASTIVE.BN_SYNC_MLP: the MLP head's BatchNorm is per device")
    if cfg.NUM_GPUS * cfg.NUM_SHARDS > 1:
        raise NotImplementedError("NUM_GPUS * NUM_SHARDS > 1: the cross-rank batch shuffle and key all-gather are not built")
    if cfg.MODEL.ARCH not in _MODEL_TYPES:
        raise NotImplementedError("MODEL.ARCH %r: ContrastiveModel runs on %s" % (cfg.MODEL.ARCH, sorted(_MODEL_TYPES)))


@MODEL_REGISTRY.register()
class ContrastiveModel(nn.Module):
    """The reference's constructor, ``forward(clips, index, time, epoch_exact, keys)`` and state_dict (``backbone.*``,
    ``backbone_hist.*``, ``ptr``, ``queue_x``, ``iter``, ``knn_mem.memory``) for ``CONTRASTIVE.TYPE == "moco"`` and ``"byol"``
    (the reference registers the queue buffers for byol too; with predictors the backbones' heads carry
    ``head.predictors.0.projection.*``).  ``"simclr"`` has no momentum encoder, queue or counters, as in the reference
    (contrastive.py:117-119): its state_dict is ``backbone.*`` plus ``knn_mem.memory`` under ``KNN_ON``, ``bind_flat`` binds
    nothing, and ``_update_history`` / ``set_momentum`` are never reached.  The reference's ``pos_mask`` / ``neg_mask``
    precompute feeds only a dead branch (``distributed_loss = False``) and is not built; ``CONTRASTIVE.SIMCLR_DIST_ON`` is read
    and ignored."""

    def __init__(self, cfg):
        super().__init__()
        _check_cfg(cfg)
        self.backbone = _MODEL_TYPES[cfg.MODEL.ARCH](cfg)
        self.type = cfg.CONTRASTIVE.TYPE
        self.T = cfg.CONTRASTIVE.T
        self.dim = cfg.CONTRASTIVE.DIM
        self.length = cfg.CONTRASTIVE.LENGTH
        self.k = cfg.CONTRASTIVE.QUEUE_LEN
        self.mmt = cfg.CONTRASTIVE.MOMENTUM
        self.momentum_annealing = cfg.CONTRASTIVE.MOMENTUM_ANNEALING
        self.duration = 1
        self.cfg = cfg
        self.num_gpus = cfg.NUM_GPUS
        self.knn_num_imgs = 0
        self.knn_on = cfg.CONTRASTIVE.KNN_ON
        self.train_labels = np.zeros((0,), dtype=np.int32)
        self.num_pos = 2
        self.num_crops = cfg.DATA.TRAIN_CROP_NUM_TEMPORAL * cfg.DATA.TRAIN_CROP_NUM_SPATIAL
        self.nce_loss_fun = get_loss_func("contrastive_loss")(reduction="mean")
        assert cfg.MODEL.LOSS_FUNC == "contrastive_loss"
        if self.type != "simclr":           # contrastive.py:117-119: simclr has no momentum encoder, queue or counters
            self.backbone_hist = _MODEL_TYPES[cfg.MODEL.ARCH](cfg)
            for p in self.backbone_hist.parameters():
                p.requires_grad = False
            self.register_buffer("ptr", torch.tensor([0]))
            stdv = 1.0 / math.sqrt(self.dim / 3)
            self.register_buffer("queue_x", torch.rand(self.k, self.dim).mul_(2 * stdv).add_(-stdv))
            self.register_buffer("iter", torch.zeros([1], dtype=torch.long))
            self._batch_shuffle_on = not (("sync" in cfg.BN.NORM_TYPE and cfg.BN.NUM_SYNC_DEVICES == cfg.NUM_GPUS)
                                          or self.type == "byol")
        self.simclr_dist_on = cfg.CONTRASTIVE.SIMCLR_DIST_ON    # read and ignored: it only feeds the reference's dead branch
        if self.knn_on:
            self.knn_mem = Memory(self.length, 1, self.dim, cfg)
        # device-side step state that is no part of a checkpoint: the two momentum words and the enqueue's error word
        self.register_buffer("_mm", momentum_words(self.mmt), persistent=False)
        self.register_buffer("_err", torch.zeros(1, dtype=torch.int32), persistent=False)
        self._mm_host = float(self.mmt)
        self._mm_stage, self._mm_stage_i = [None, None], 0
        self._iter_host = 0             # mirror of `iter`: nothing reads the buffer back per iteration
        self._flat = None               # (flat parameters, flat history) once bind_flat() ran

    # ---- checkpoint surface ---------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        if self.type != "simclr":
            self._iter_host = int(self.iter.item())
        engine.PARAM_EPOCH += 1
        return out

    def state_dict(self, *args, **kwargs):
        self.check_queue_error()        # a checkpoint synchronises anyway
        return super().state_dict(*args, **kwargs)

    def eval(self):
        self.check_queue_error()
        return super().eval()

    def check_queue_error(self):
        check_queue_error(self._err)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._mm_host = None            # the buffers may have moved: upload the momentum again before the next update
        return out

    # ---- momentum encoder -----------------------------------------------------------------------------------------
    def bind_flat(self, optimizer):
        """After ``construct_optimizer``: ``backbone_hist``'s parameters become views of one flat buffer laid out like
        ``optimizer.flat_param`` (matched by name), so that ``_update_history`` is one launch."""
        if self.type == "simclr":           # no momentum encoder: nothing to bind (the training loop reads the same)
            return self
        names = {id(p): n for n, p in self.backbone.named_parameters()}
        hist = dict(self.backbone_hist.named_parameters())
        flat = optimizer.flat_param
        hist_flat = torch.empty_like(flat)
        off, bound = 0, set()
        for p in optimizer.reducer.params:
            name = names.get(id(p))
            if name is None or name not in hist:
                raise SfError("bind_flat: the optimizer holds a parameter that is not one of backbone's")
            h, n = hist[name], p.numel()
            view = hist_flat[off:off + n].view_as(h)
            view.copy_(h.data)
            h.data = view
            bound.add(name)
            off += n
        if off != flat.numel() or len(bound) != len(hist):
            raise SfError("bind_flat: %d of backbone_hist's %d parameters have a counterpart in the optimizer" % (len(bound), len(hist)))
        self._flat = (flat, hist_flat)
        engine.PARAM_EPOCH += 1
        return self

    def set_momentum(self, m):
        """Uploads (m, 1 - m) when ``m`` changed since the last upload (asynchronously, from one of two pinned buffers)."""
        m = float(m)
        if self._mm_host is not None and m == self._mm_host:
            return False
        words = momentum_words(m)
        if self._mm.is_cuda:
            assert not torch.cuda.is_current_stream_capturing(), "set_momentum() inside a graph capture"
            i = self._mm_stage_i = self._mm_stage_i ^ 1
            if self._mm_stage[i] is None:
                self._mm_stage[i] = [torch.empty(2, dtype=torch.float32).pin_memory(), None]
            buf, ev = self._mm_stage[i]
            if ev is not None:
                ev.synchronize()        # two uploads ago: long done
            buf.copy_(words)
            self._mm.copy_(buf, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self._mm.device))
            self._mm_stage[i][1] = ev
        else:
            self._mm.copy_(words)
        self._mm_host = m
        return True

    @torch.no_grad()
    def _update_history(self):
        first = self._iter_host == 0
        self.set_momentum(self.mmt)
        if self._flat is not None:
            flat, hist_flat = self._flat
            if first:
                hist_flat.copy_(flat)
            ema_update(flat, hist_flat, self._mm)
        else:
            dist = dict(self.backbone.named_parameters())
            for name, h in self.backbone_hist.named_parameters():
                p = dist[name]
                if not h.data.is_contiguous():
                    h.data = h.data.contiguous()
                if first:
                    h.data.copy_(p.data)
                ema_update(p.data.contiguous(), h.data, self._mm)
        # the kernel wrote the key encoder's weights without bumping tensor._version: its packed 16-bit copies are stale
        engine.PARAM_EPOCH += 1

    @torch.no_grad()
    def momentum_anneal_cosine(self, epoch_exact):
        self.mmt = 1 - (1 - self.cfg.CONTRASTIVE.MOMENTUM) * (
            math.cos(math.pi * epoch_exact / self.cfg.SOLVER.MAX_EPOCH) + 1.0) * 0.5

    # ---- batch shuffle (single device: a permutation of the local batch, drawn on the CPU generator as the reference) --
    @torch.no_grad()
    def _batch_shuffle(self, x):
        idx_randperm = torch.randperm(x[0].shape[0])
        dev_idx = idx_randperm.to(x[0].device)
        out = [t[dev_idx] for t in x]
        idx_restore = torch.argsort(idx_randperm.view(-1)).view(1, -1)
        return out, idx_restore

    @torch.no_grad()
    def _batch_unshuffle(self, x, idx_restore):
        return x[idx_restore[0, :].to(x.device)]

    @torch.no_grad()
    def batch_clips(self, clips):
        clips_batched = [None] * len(clips[0])
        for i, clip in enumerate(clips):
            for j, view in enumerate(clip):
                clips_batched[j] = view if i == 0 else torch.cat([clips_batched[j], view], dim=0)
        return clips_batched

    @torch.no_grad()
    def compute_key_feat(self, clips_k, compute_predictor_keys=False, batched_inference=True):
        assert self.training
        if compute_predictor_keys:
            raise NotImplementedError("compute_predictor_keys=True: nothing in the reference calls it (both callers pass False), "
                                      "and its batched branch slices a list of key matrices as if it were one")
        self._update_history()
        self.iter += 1
        self._iter_host += 1
        n_clips = len(clips_k)
        bsz = clips_k[0][0].shape[0]
        if n_clips * bsz * clips_k[0][0].numel() > 4 * 64 * 3 * 8 * 224 * 224:
            batched_inference = False
        assert n_clips > 0
        batched = batched_inference and all(clips_k[i][j].shape[1:] == clips_k[0][j].shape[1:]
                                            for i in range(len(clips_k)) for j in range(len(clips_k[i])))
        if batched:
            clips_k = [self.batch_clips(clips_k)]
        keys = []
        for clip_k in clips_k:
            idx_restore = None
            clip_k = list(clip_k)
            if self._batch_shuffle_on:
                clip_k, idx_restore = self._batch_shuffle(clip_k)
            # the engine's training-mode forward under no_grad: batch statistics, running statistics updated, nothing kept
            # for a backward (the forward of every stage joins its own side streams; BatchNorm-partial tags are made by
            # backward nodes only)
            hist_feat = self.backbone_hist(clip_k)
            if isinstance(hist_feat, list):         # [projection, predictor outputs]: the keys are the projection
                hist_feat = hist_feat[0]
            # Normalize + _batch_unshuffle in one launch
            keys.append(l2norm_rows(hist_feat.float(), None if idx_restore is None else idx_restore[0]))
        if batched:
            assert len(keys) == 1, "batched input uses single clip"
            batched_key = keys[0]
            keys = [batched_key[k * bsz:(k + 1) * bsz] for k in range(n_clips)]
        return keys

    @torch.no_grad()
    def _dequeue_and_enqueue(self, keys, extra_keys=None):
        if not self.cfg.CONTRASTIVE.MOCO_MULTI_VIEW_QUEUE:
            upd = [keys[0]]
        else:
            assert len(keys) > 0, "need to have multiple views for adding them to queue"
            upd = list(keys)
            if extra_keys:
                upd += [item for sublist in extra_keys for item in sublist]
        assert self.k % int(upd[0].size(0)) == 0
        enqueue(self.queue_x, self.ptr, upd, err=self._err)

    # ---- kNN monitor ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def knn_mem_update(self, q_knn, index):
        if self.knn_on:
            self.knn_mem.update(q_knn, momentum=1.0, ind=index, time=torch.zeros_like(index), interp=False)

    @torch.no_grad()
    def init_knn_labels(self, train_loader):
        self.num_imgs = len(train_loader.dataset._labels)
        labels = np.zeros((self.num_imgs,), dtype=np.int32)
        for i in range(self.num_imgs):
            labels[i] = train_loader.dataset._labels[i]
        self.train_labels = torch.LongTensor(labels).to(self._err.device)
        if self.length != self.num_imgs:
            self.knn_mem.resize(self.num_imgs, 1, self.dim)

    @torch.no_grad()
    def eval_knn(self, q_knn, knn_k=200):
        dist = torch.einsum("nc,mc->nm", q_knn.view(q_knn.size(0), -1),
                            self.knn_mem.memory.view(self.knn_mem.memory.size(0), -1))
        return dist.topk(knn_k, dim=1, largest=True, sorted=True)

    # ---- forward --------------------------------------------------------------------------------------------------
    def forward(self, clips, index=None, time=None, epoch_exact=None, keys=None):
        if epoch_exact is not None and self.momentum_annealing:
            self.momentum_anneal_cosine(epoch_exact)
        if self.type == "byol":
            return self._forward_byol(clips, index, keys)
        if self.type == "simclr":
            return self._forward_simclr(clips, index)
        if isinstance(clips[0], list):
            clip_q, clips_k = clips[0], list(clips[1:])
        else:
            clip_q, clips_k = clips, None
        feat_q = self.backbone(clip_q)
        if isinstance(feat_q, list):
            raise NotImplementedError("CONTRASTIVE.PREDICTOR_DEPTHS")
        if index is None:
            return feat_q
        feat_q = feat_q.float().contiguous()
        if not self.training:
            return self.eval_knn(l2norm_rows(feat_q.detach()))
        if keys is None:
            keys = self.compute_key_feat(clips_k, compute_predictor_keys=False)
            auto_enqueue_keys = True
        else:
            auto_enqueue_keys = False
        # the enqueue below is ordered after the loss on the stream and the backward reads df, never the queue: no clone
        logits, loss = moco_nce(feat_q, keys, self.queue_x, self.T)
        if auto_enqueue_keys:
            self._dequeue_and_enqueue(keys)
        if self.knn_on:
            self.knn_mem_update(l2norm_rows(feat_q.detach()), index)
        return logits, loss

    def _forward_simclr(self, clips, index):
        """The simclr branch (contrastive.py:692-754).  ``index is None`` returns the NORMALISED rows, as the reference does
        here (its moco and byol branches return the raw features), detached.  Training runs the backbone on ``clips[0]`` and on
        ``clips[1]`` in two separate calls, as there: BatchNorm statistics move twice.  Returns (dummy logits, loss); the dummy
        logits are shared between calls (``dummy_logits``)."""
        many = isinstance(clips[0], list)
        feat_q = self.backbone(clips[0] if many else clips)
        if isinstance(feat_q, list):
            raise NotImplementedError("CONTRASTIVE.PREDICTOR_DEPTHS")
        if index is None:
            return l2norm_rows(feat_q.detach().float().contiguous())      # detached: a feature-extraction call
        if not self.training:
            return self.eval_knn(l2norm_rows(feat_q.detach().float().contiguous()))
        assert many and len(clips) >= 2, "training takes a list of two clips"
        feat_q2 = self.backbone(clips[1])
        if self.knn_on:
            loss, q = simclr_ntxent(feat_q.float(), feat_q2.float(), self.T, return_q=True)
            self.knn_mem_update(q, index)          # the kernel's own Normalize(clips[0]): no second normalisation launch
        else:
            loss = simclr_ntxent(feat_q.float(), feat_q2.float(), self.T)
        return dummy_logits(len(index), self.k, feat_q.device), loss

    def _forward_byol(self, clips, index, keys):
        """The byol branch (contrastive.py:485-568).  Returns (dummy logits, loss); the dummy logits are a tensor shared between
        calls (``dummy_logits``): callers must not write to it."""
        many = isinstance(clips[0], list)
        feat_q = self.backbone(clips[0] if many else clips)
        if not isinstance(feat_q, list):
            raise NotImplementedError("BYOL: predictor is missing")
        assert len(feat_q) == 2, "BYOL takes exactly one predictor"
        proj, pred = feat_q
        if index is None:
            return proj
        if not self.training:
            return self.eval_knn(l2norm_rows(proj.detach().float().contiguous()))
        assert many, "training takes a list of clips"
        if keys is None:
            keys = self.compute_key_feat([list(clip) for clip in clips], compute_predictor_keys=False)
        if self.cfg.CONTRASTIVE.SEQUENTIAL:
            loss = byol_sim(pred.float(), keys, self.T)        # sum_v sim_loss(predictor, key_v) / V in one call
        else:
            assert len(clips) == 2, "the symmetric loss takes exactly two crops"
            loss_q1 = byol_sim(pred.float(), [keys[1]], self.T)
            feat_q2 = self.backbone(clips[1])
            assert len(feat_q2) == 2
            loss_q2 = byol_sim(feat_q2[1].float(), [keys[0]], self.T)
            loss = loss_q1 + loss_q2
        if self.knn_on:
            self.knn_mem_update(l2norm_rows(proj.detach().float().contiguous()), index)
        return dummy_logits(len(index), self.k, proj.device), loss


_dummy_logits = {}


def dummy_logits(rows, K, device):
    """The (rows, 1 + K) matrix the byol branch returns in place of logits: 9999 in column 0, zeros elsewhere, so that the
    training meter's top-1 reads 100 %.  Built once per (rows, K, device) -- 16.8 MB at the recipe's shapes, which the reference
    allocates and fills twice per step -- and SHARED between calls: treat it as read-only (``torch.cat`` of it, as
    ``contrastive_forward`` does, makes a new tensor)."""
    key = (rows, K, torch.device(device))
    t = _dummy_logits.get(key)
    if t is None:
        t = torch.zeros((rows, 1 + K), dtype=torch.float32, device=device)
        t[:, 0] = 9999.0
        _dummy_logits[key] = t
    return t


def contrastive_parameter_surgery(model, cfg, epoch_exact, cur_iter):
    """contrastive.py:1031-1055: for moco no parameter update while the queue fills during the first epoch; byol updates from
    the first iteration."""
    iters_noupdate = 0
    if cfg.MODEL.MODEL_NAME == "ContrastiveModel" and cfg.CONTRASTIVE.TYPE == "moco":
        assert cfg.CONTRASTIVE.QUEUE_LEN % (cfg.TRAIN.BATCH_SIZE * cfg.NUM_SHARDS) == 0
        iters_noupdate = cfg.CONTRASTIVE.QUEUE_LEN // cfg.TRAIN.BATCH_SIZE // cfg.NUM_SHARDS
    update_param = not (cur_iter < iters_noupdate and epoch_exact < 1)
    return model, update_param


def contrastive_forward(model, cfg, inputs, index, time, epoch_exact, scaler=None):
    """contrastive.py:1058-1100: with CONTRASTIVE.SEQUENTIAL every crop is the query once against the keys of the others (and
    is backpropagated here: ``perform_backward`` comes back False); ``scaler`` is a GradScaler, a callable ``loss -> scaled
    loss`` or None."""
    if cfg.CONTRASTIVE.SEQUENTIAL:
        perform_backward = False
        mdl = getattr(model, "module", model)
        simclr = cfg.CONTRASTIVE.TYPE == "simclr"
        if simclr:                              # no key encoder: pair k is crops (k, k + 1), the last crop opens no pair
            keys = [None] * len(inputs)
        else:
            keys = mdl.compute_key_feat(inputs, compute_predictor_keys=False, batched_inference=len(inputs) < 2)
        for k, vid in enumerate(inputs):
            other_keys = keys[:k] + keys[k + 1:]
            time_cur = None if time is None else torch.cat([time[:, k:k + 1, :], time[:, :k, :], time[:, k + 1:, :]], 1)
            vids = [vid]
            if simclr:
                if k < len(inputs) - 1:
                    vids = inputs[k:k + 2]
                else:
                    break
            lgt_k, loss_k = model(vids, index, time_cur, epoch_exact, keys=other_keys)
            scaled = loss_k if scaler is None else (scaler.scale(loss_k) if hasattr(scaler, "scale") else scaler(loss_k))
            scaled.backward()
            if k == 0:
                preds, partial_loss = lgt_k, loss_k.detach().clone()
            else:
                preds = torch.cat([preds, lgt_k], dim=0)
                partial_loss += loss_k.detach()
        partial_loss /= len(inputs) * 2.0       # to have same loss as symm model
        if cfg.CONTRASTIVE.TYPE == "moco":      # byol keeps the queue buffers but never writes them (contrastive.py:1095)
            mdl._dequeue_and_enqueue(keys)
    else:
        perform_backward = True
        preds, partial_loss = model(inputs, index, time, epoch_exact, keys=None)
    return model, preds, partial_loss, perform_backward
