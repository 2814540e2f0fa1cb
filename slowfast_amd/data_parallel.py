"""Data-parallel gradient reduction over RCCL/xGMI (replaces the reference's torch DDP wrap,
slowfast/models/build.py:64-80, and its optional fp16_compress_hook).

One process per GPU, replicated model, per-GPU local BatchNorm statistics (BN.NORM_TYPE "batchnorm").
All parameter gradients live in ONE flat fp32 buffer; ``param.grad`` are views into it, so the engine's
backward kernels write gradients in place.  The buffer is cut into a few large buckets in backward order
(xGMI is point-to-point, 7 links x ~153 GB/s per GPU: few large collectives beat many small ones).
The engine announces which parameters are final after each block's backward
(engine.add_grad_ready_listener); when a bucket is complete its all-reduce is enqueued asynchronously
(c10d "nccl" == RCCL on ROCm, its own HIP stream) and overlaps the rest of backward.  ``finish()`` waits
for the collectives and applies 1/(world_size*loss_scale) in a single pass over the flat buffer.
"""
import torch
import torch.distributed as dist

from . import engine


class GradReducer:
    def __init__(self, model, bucket_mb=48, process_group=None, comm_dtype=None, force_collectives=False):
        self.model = model
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        # world 1 normally skips the collectives; tests force them to drive the RCCL calls on a single GPU
        self.collectives = self.world > 1 or (force_collectives and dist.is_available() and dist.is_initialized())
        self.comm_dtype = comm_dtype            # torch.float16 mirrors MODEL.FP16_ALLREDUCE
        params = [p for p in model.parameters() if p.requires_grad]
        self.params = params[::-1]              # reverse registration order ~ order in which backward finishes them
        total = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._views, self._bucket_of = {}, {}
        self.buckets = []                       # (start, end, [params])
        off, bstart, bparams = 0, 0, []
        limit = int(bucket_mb * 1024 * 1024 / 4)
        for p in self.params:
            n = p.numel()
            self._views[p] = self.flat[off:off + n].view_as(p)
            bparams.append(p)
            off += n
            if off - bstart >= limit:
                self.buckets.append((bstart, off, bparams))
                bstart, bparams = off, []
        if bparams:
            self.buckets.append((bstart, off, bparams))
        for bi, (_, _, ps) in enumerate(self.buckets):
            for p in ps:
                self._bucket_of[p] = bi
        self._pending = [0] * len(self.buckets)
        self._handles = []
        self._torch_hooks = []
        self._prescale, self._prescaled = 1.0 / self.world, set()   # compressed buckets are averaged before the cast
        def listener(params):
            self._on_ready(params)
        # the other pathway's / branch's gradients may still be running on their own stream when a block announces its
        # parameters.  The join (engine.join_side_streams) is made where a collective is actually launched (_launch: a bucket
        # is complete), not on every announcement -- joining per block serialised the Slow and Fast pathways' backward in the
        # eager multi-GPU path
        listener.needs_join = lambda: False
        self._listener = engine.add_grad_ready_listener(listener)
        # parameters owned by plain torch modules (the head) announce themselves through autograd hooks
        self._hooked = set()
        self.capturing = False                  # True while TrainStep records the HIP graph: no collectives
        self.zero_grad()

    # -- per-iteration protocol -------------------------------------------------------------------------
    def zero_grad(self):
        """Clear the flat buffer and (re)attach the gradient views; call before every forward."""
        engine.GRADS_VIA_AUTOGRAD = False       # this model's gradients are written in place (see wrap_ddp)
        self.flat.zero_()
        for p, v in self._views.items():
            if p.grad is not v:
                p.grad = v
        self._pending = [len(ps) for _, _, ps in self.buckets]
        self._ready = set()
        self._handles = []
        self._prescaled = set()

    def begin_replay(self):
        """Before replaying a captured forward/backward (slowfast_amd.step.TrainStep): the captured work clears
        the flat buffer and writes every gradient, but none of the Python-side readiness callbacks run, so all
        buckets are reduced by finish()."""
        self._pending = [len(ps) for _, _, ps in self.buckets]
        self._ready = set()
        self._handles = []
        self._prescaled = set()

    def attach_torch_param_hooks(self, params):
        for p in params:
            if p in self._views and p not in self._hooked:
                self._hooked.add(p)
                self._torch_hooks.append(p.register_post_accumulate_grad_hook(lambda q: self._on_ready([q])))

    def _on_ready(self, params):
        for p in params:
            bi = self._bucket_of.get(p)
            if bi is None or p in self._ready:
                continue
            self._ready.add(p)
            self._pending[bi] -= 1
            if self._pending[bi] == 0:
                self._launch(bi)

    def _launch(self, bi):
        if not self.collectives or self.capturing:
            return
        engine.join_side_streams()              # every stream that wrote a gradient of this bucket, before RCCL reads it
        s, e, _ = self.buckets[bi]
        view = self.flat[s:e]
        if self.comm_dtype is not None:
            # divide by the world size in fp32 BEFORE compressing (torch's fp16_compress_hook order), so the SUM over ranks
            # cannot leave the fp16 range when every rank's value is inside it.  The loss scale is NOT removed here (it is
            # dynamic and lives on the device): a loss-scaled |g| * S > 65504 overflows to inf in the cast exactly as it does
            # under torch's hook; FlatOptimizer's inf check then skips the step and backs the scale off.
            low = (view * self._prescale).to(self.comm_dtype)
            h = dist.all_reduce(low, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self._handles.append((h, view, low, bi))
            self._prescaled.add(bi)
        else:
            h = dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self._handles.append((h, None, None, bi))

    def finish(self, loss_scale=1.0, on_bucket=None):
        """Wait for outstanding collectives; gradients become mean over ranks of the unscaled gradients.
        ``loss_scale=None``: only wait -- the buffer keeps the loss-scaled SUM over ranks, which is what
        slowfast_amd.optim.FlatOptimizer.step() expects (it folds 1 / (world * scale) into its single update pass).
        ``on_bucket(bi)``: called right after bucket bi's collective has been waited for (a stream-level wait under RCCL), in
        launch order -- FlatOptimizer takes the bucket's share of the gradient norm / overflow check there, so that pass runs
        under the exchange of the buckets still in flight instead of after all of them."""
        done = set()
        if self.collectives:
            for bi, n in enumerate(self._pending):
                if n > 0:                         # parameters that got no gradient this iteration
                    self._pending[bi] = 0
                    self._launch(bi)
            for h, view, low, bi in self._handles:
                h.wait()
                if low is not None:
                    view.copy_(low)
                    if loss_scale is None and bi in self._prescaled:
                        # the caller (FlatOptimizer.finish_and_step) reads the bucket inside on_bucket and expects the
                        # loss-scaled SUM over ranks: undo the 1/world of the compressed exchange BEFORE handing it over
                        view.mul_(float(self.world))
                        self._prescaled.discard(bi)
                if on_bucket is not None:
                    on_bucket(bi)
                    done.add(bi)
            self._handles = []
        if on_bucket is not None:                 # buckets without a collective (world 1, capture replay of a single rank)
            for bi in range(len(self.buckets)):
                if bi not in done:
                    on_bucket(bi)
        if loss_scale is None:
            for bi in self._prescaled:      # compressed buckets were averaged before the cast: back to a sum
                s, e, _ = self.buckets[bi]
                self.flat[s:e].mul_(float(self.world))
            self._prescaled = set()
            return
        if self._prescaled:             # compressed buckets already carry 1/world: only the loss scale is left for them
            for bi, (s, e, _) in enumerate(self.buckets):
                k = 1.0 / loss_scale if bi in self._prescaled else 1.0 / (self.world * loss_scale)
                if k != 1.0:
                    self.flat[s:e].mul_(k)
            self._prescaled = set()
            return
        k = 1.0 / (self.world * loss_scale)
        if k != 1.0:
            self.flat.mul_(k)

    def grad_norm(self):
        """Global L2 norm of all gradients (slowfast/models/optimizer.py:362-379) in one pass."""
        return torch.linalg.vector_norm(self.flat)

    def close(self):
        engine.remove_grad_ready_listener(self._listener)
        for h in self._torch_hooks:
            h.remove()


# ---------------------------------------------------------------------------------------------------------------------
# The reference's own boundary: torch DDP + comm hook (slowfast/models/build.py:64-80)
def xgmi_allreduce_hook(state, bucket):
    """DDP communication hook (``register_comm_hook(state, hook)`` API: hook(state, GradBucket) -> Future[Tensor]):
    mean all-reduce of the bucket in fp32 over the process group in ``state`` (None = default group).  Semantically DDP's
    built-in allreduce_hook; installed explicitly so that the bucket size chosen in wrap_ddp (large buckets: xGMI links
    are point-to-point, a ring is bound per link, so few large collectives beat many 25 MiB ones) travels with it."""
    group = state if state is not None else dist.group.WORLD
    world = dist.get_world_size(group)
    t = bucket.buffer()
    t.div_(world)
    fut = dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=True).get_future()
    return fut.then(lambda f: f.value()[0])


def fp16_compress_hook(state, bucket):
    """MODEL.FP16_ALLREDUCE (build.py:77-80 installs torch's fp16_compress_hook): divide by the world size FIRST, then
    compress to fp16, all-reduce, decompress into the bucket -- the division before the cast is what keeps loss-scaled
    gradients inside the fp16 range."""
    group = state if state is not None else dist.group.WORLD
    world = dist.get_world_size(group)
    buf = bucket.buffer()
    low = (buf / world).to(torch.float16)
    fut = dist.all_reduce(low, op=dist.ReduceOp.SUM, group=group, async_op=True).get_future()

    def decompress(f):
        buf.copy_(f.value()[0])
        return buf
    return fut.then(decompress)


def wrap_ddp(model, device=None, find_unused_parameters=False, fp16_allreduce=False, bucket_cap_mb=64, process_group=None):
    """torch.nn.parallel.DistributedDataParallel around the drop-in model, as slowfast/models/build.py:64-80 wraps the
    reference model.  Switches the engine to autograd-delivered parameter gradients (engine.GRADS_VIA_AUTOGRAD): DDP's
    reducer hooks the parameters' AccumulateGrad nodes, so gradients written straight into ``param.grad`` would never be
    all-reduced.  The switch says which mode the model that is running its FORWARD is in: the wrapper's forward pre-hook turns
    it on, GradReducer.zero_grad() (first call of every in-place iteration) turns it off, and every engine Function records
    the value it saw at forward time and runs its backward under that (engine.record_params / delivers_grads) -- a DDP-wrapped
    model and a GradReducer-driven one can interleave their forward and backward passes in one process."""
    engine.GRADS_VIA_AUTOGRAD = True

    def _via_autograd(module, args):
        engine.GRADS_VIA_AUTOGRAD = True
    kw = dict(find_unused_parameters=find_unused_parameters, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True,
              process_group=process_group)
    if device is not None:
        kw.update(device_ids=[device], output_device=device)
    ddp = torch.nn.parallel.DistributedDataParallel(module=model, **kw)
    ddp.register_comm_hook(state=process_group, hook=fp16_compress_hook if fp16_allreduce else xgmi_allreduce_hook)
    ddp.register_forward_pre_hook(_via_autograd)
    return ddp
