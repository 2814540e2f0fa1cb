"""Random erasing of a training batch on the device (slowfast/datasets/random_erasing.py, applied at datasets/kinetics.py:437-447
to the normalised fp32 clip just before ``pack_pathway_output``).

The reference erases on the host, so the erased clip travels to the GPU as fp32.  Here the DRAW stays on the host and the
erasing happens on the device, either on the dense fp32 batch (``RandomErasing.__call__`` / ``erase_clip``: one launch that
writes only the erased elements) or while uint8 frames are packed (``data.pack_pathways_u8(..., erase=table)``: in fp32 between
the normalisation and the 16-bit rounding, before MixUp / CutMix -- the reference's order).

The draw.  ``sample_params((T, C, H, W))`` consumes Python's global ``random`` in exactly the reference's order:
``random()`` against ``probability``; ``randint(min_count, max_count)`` only when the counts differ; per box up to 100
attempts (10 per frame with ``cube=False``) of ``uniform`` for the area, ``uniform`` for the log aspect and -- only when
``h < H and w < W`` -- ``randint`` for ``top``, then for ``left``.  A loop seeded like the reference's erases the same boxes
(pinned by tests/golden/random_erasing_contract.json).  It returns an ``ErasePlan`` whose rows are
``(t_start, t_end, top, left, h, w)`` in draw order; ``cube=True`` gives one row per box over frames
``T // num_splits if num_splits > 1 else 0 .. T``, ``cube=False`` one row per frame per box.

The values.  ``const`` writes 0.  ``rand`` makes the reference's ``torch.empty((C, 1, 1)).normal_()`` calls on the host in the
reference's order (one per frame per box, global CPU generator) and carries the colours in the plan: bit-exact against the
reference, and the torch generator advances as the reference's does.  ``pixel`` is where the contract DIFFERS from the
reference: the reference fills every frame of a box with ``C*h*w`` normals of the CPU generator; this class consumes no torch
random numbers at all and instead gives every row a 64-bit key from a private ``random.Random(noise_seed)``; the device
derives the noise from (key, element index) with Philox4x32-10 and Box-Muller (csrc/sf_erase.h).  The boxes --
and the global ``random`` stream -- stay aligned with the reference, the noise values do not.
"""
import collections
import math
import random

import numpy as np
import torch

from . import ops
from .lib import SfError, get_lib

MODES = {"const": 0, "rand": 1, "pixel": 2}
ROW_WORDS = 12          # csrc/sf_erase.h: SF_ERASE_ROW_WORDS

# rows: [(t_start, t_end, top, left, h, w)] in draw order; keys: one 64-bit noise key per row (pixel mode, else 0);
# colours: one float32 (t_end - t_start, C) array per row (rand mode, else None); mode: "const" / "rand" / "pixel"
ErasePlan = collections.namedtuple("ErasePlan", ["rows", "keys", "colours", "mode"])
# the batch table of sample_batch: rows int32 (R, 7) = (n, t_start, t_end, top, left, h, w) with samples ascending; keys uint64
# (R,); colours float32 (sum of frames, C), row r owning the next t_end - t_start lines; shape = the (T, C, H, W) it was drawn for
EraseTable = collections.namedtuple("EraseTable", ["rows", "keys", "colours", "mode", "shape"])


def make_table(rows, mode, shape, keys=None, colours=None):
    """An explicit EraseTable: ``rows`` = (n, t_start, t_end, top, left, h, w) tuples (samples ascending, later rows win where
    they overlap), ``keys`` one integer per row (pixel mode), ``colours`` one (frames, C) array per row (rand mode)."""
    T, C, H, W = (int(v) for v in shape)
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 7)
    keys = np.zeros(len(rows), dtype=np.uint64) if keys is None else np.asarray(keys, dtype=np.uint64).reshape(-1)
    if colours is None:
        colours = np.zeros((int((rows[:, 2] - rows[:, 1]).clip(min=0).sum()) if mode == "rand" else 0, C), dtype=np.float32)
    elif not isinstance(colours, np.ndarray) or colours.ndim != 2:
        colours = (np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1, C) for c in colours], 0) if len(colours)
                   else np.zeros((0, C), dtype=np.float32))
    return EraseTable(rows, keys, np.ascontiguousarray(colours, dtype=np.float32), mode, (T, C, H, W))


def _pack_table(table, N):
    """EraseTable -> the int32 words of csrc/sf_erase.h (rows, first_row[N + 1], colours as float bits).  Rows must be filed
    by ascending sample; everything else is checked by the library against the clip."""
    if table.mode not in MODES:
        raise SfError("RandomErasing: unknown mode %r" % (table.mode,))
    rows, R, C = table.rows, len(table.rows), table.shape[1]
    if len(table.keys) != R:
        raise SfError("RandomErasing: the table needs one key per row")
    n = rows[:, 0] if R else np.zeros(0, dtype=np.int32)
    if R and (np.any(np.diff(n) < 0) or n[0] < 0 or n[-1] >= N):
        raise SfError("RandomErasing: table rows must be filed by ascending sample index within the batch of %d" % N)
    first = np.searchsorted(n, np.arange(N + 1)).astype(np.int32)
    head = R * ROW_WORDS + N + 1
    words = np.zeros((R, ROW_WORDS), dtype=np.int32)
    if R:
        words[:, :7] = rows
        words[:, 7] = (table.keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        words[:, 8] = (table.keys >> np.uint64(32)).astype(np.uint32).view(np.int32)
        words[:, 10] = first[n + 1]
        if table.mode == "rand":
            frames = (rows[:, 2] - rows[:, 1]).clip(min=0).astype(np.int64)
            if int(frames.sum()) != len(table.colours):
                raise SfError("RandomErasing: rand mode needs one colour line per erased frame of every row")
            words[:, 9] = head + (np.cumsum(frames) - frames) * C
    col = table.colours.reshape(-1).view(np.int32) if table.mode == "rand" else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(np.concatenate([words.reshape(-1), first, col])), R


def upload_table(table, N, device):
    """(host words, device words, rows) of a table for a batch of N: one small host-to-device copy."""
    host, R = _pack_table(table, N)
    return host, torch.from_numpy(host).to(device), R


def _check_clip(x, out):
    if not (torch.is_tensor(x) and x.dim() == 5 and x.dtype == torch.float32 and x.is_contiguous()):
        raise SfError("RandomErasing: the batch must be a dense float32 (N, C, T, H, W) device tensor (got %s)" % (
            "%s %s%s" % (x.dtype, tuple(x.shape), "" if x.is_contiguous() else " non-contiguous") if torch.is_tensor(x)
            else type(x).__name__))
    if out is not None and out is not x:
        if not (torch.is_tensor(out) and out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
                and out.device == x.device):
            raise SfError("RandomErasing: out must be a dense float32 tensor of the batch's shape on the batch's device")
    return ops._stream(x)           # raises for a CPU tensor with the gfx950 library: there is no torch fallback


def erase_clip(x, table, out=None):
    """The device half of ``RandomErasing.__call__`` for an explicit ``EraseTable``: erases the dense fp32 (N, C, T, H, W)
    batch ``x`` in place (only the erased elements are written; a table without rows launches nothing), or into ``out``
    (the whole batch is read once and written once)."""
    stream = _check_clip(x, out)
    dst = x if out is None else out
    N, C, T, H, W = x.shape
    if tuple(table.shape) != (T, C, H, W):
        raise SfError("RandomErasing: the table was drawn for (T, C, H, W) = %s, the batch is %s" % (
            tuple(table.shape), (T, C, H, W)))
    inplace = dst is x or dst.data_ptr() == x.data_ptr()
    host, R = _pack_table(table, N)
    if R == 0 and inplace:
        return dst
    dev = torch.from_numpy(host).to(x.device)
    erased = int((table.rows[:, 2] - table.rows[:, 1]).clip(min=0).astype(np.int64) @ (
        table.rows[:, 5].astype(np.int64) * table.rows[:, 6])) * C if R else 0
    get_lib().call("sf_erase_clip_f32", x.data_ptr(), dst.data_ptr(), N, C, T, H, W, MODES[table.mode], host.ctypes.data,
                   dev.data_ptr(), R, int(host.size), stream,
                   work=dict(bytes=4.0 * erased if inplace else 8.0 * x.numel()))
    return dst


class RandomErasing:
    """Constructor of slowfast/datasets/random_erasing.py:RandomErasing without ``device`` (the erasing always runs where the
    batch lives) and with ``noise_seed``: the seed of the private generator of the pixel-mode noise keys."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode="const",
                 min_count=1, max_count=None, num_splits=0, cube=True, noise_seed=None):
        self.probability = probability
        self.min_area = min_area
        self.max_area = max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count = min_count
        self.max_count = max_count or min_count
        self.num_splits = num_splits
        mode = mode.lower()
        self.rand_color = mode == "rand"
        self.per_pixel = mode == "pixel"
        assert self.rand_color or self.per_pixel or not mode or mode == "const"
        self.mode = "rand" if self.rand_color else ("pixel" if self.per_pixel else "const")
        self.cube = cube
        self.noise_seed = noise_seed
        self._noise_rng = random.Random(noise_seed)

    # ---- the draw (host) ------------------------------------------------------------------------------------------
    def _draw_boxes(self, img_h, img_w, attempts, on_box):
        """_erase / _erase_cube up to the assignment: ``on_box(top, left, h, w)`` stands for it."""
        if random.random() > self.probability:
            return
        area = img_h * img_w
        count = self.min_count if self.min_count == self.max_count else random.randint(self.min_count, self.max_count)
        for _ in range(count):
            for _ in range(attempts):
                target_area = random.uniform(self.min_area, self.max_area) * area / count
                aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < img_w and h < img_h:
                    top = random.randint(0, img_h - h)
                    left = random.randint(0, img_w - w)
                    on_box(top, left, h, w)
                    break

    def sample_params(self, shape):
        """One clip's draw for the per-clip geometry ``shape`` = (T, C, H, W): an ErasePlan (no rows when nothing is erased)."""
        T, C, H, W = (int(v) for v in shape)
        rows, keys, colours = [], [], []

        def add(t0, t1):
            def on_box(top, left, h, w):
                rows.append((t0, t1, top, left, h, w))
                keys.append(self._noise_rng.getrandbits(64) if self.per_pixel else 0)
                if self.rand_color:     # _get_pixels once per frame, as the reference's loop over the frames does
                    colours.append(np.stack([torch.empty((C, 1, 1), dtype=torch.float32).normal_().view(C).numpy()
                                             for _ in range(t0, t1)], 0) if t1 > t0 else np.zeros((0, C), np.float32))
            return on_box

        t_start = T // self.num_splits if self.num_splits > 1 else 0
        if self.cube:
            self._draw_boxes(H, W, 100, add(t_start, T))
        else:
            for t in range(t_start, T):
                self._draw_boxes(H, W, 10, add(t, t + 1))
        return ErasePlan(rows, keys, colours if self.rand_color else None, self.mode)

    def sample_batch(self, N, shape):
        """The draws of clips 0 .. N-1 in that order, as a single dataset worker would make them: an EraseTable."""
        T, C, H, W = (int(v) for v in shape)
        rows, keys, colours = [], [], []
        for n in range(int(N)):
            plan = self.sample_params((T, C, H, W))
            rows += [(n,) + tuple(r) for r in plan.rows]
            keys += plan.keys
            colours += plan.colours or []
        return make_table(rows, self.mode, (T, C, H, W), keys=keys, colours=colours if self.rand_color else None)

    # ---- the device side ------------------------------------------------------------------------------------------
    def __call__(self, x, out=None):
        """Erases the dense fp32 (N, C, T, H, W) device batch ``x`` in place, or into ``out``: every clip drawn in order,
        one table upload, one launch.  A 3-D single image (the reference's other branch) is not supported."""
        if torch.is_tensor(x) and x.dim() == 3:
            raise SfError("RandomErasing: single images are not supported, pass the (N, C, T, H, W) batch")
        _check_clip(x, out)                             # before the draw: a rejected call consumes no random numbers
        N, C, T, H, W = x.shape
        return erase_clip(x, self.sample_batch(N, (T, C, H, W)), out=out)


def construct_random_erasing(cfg):
    """The ``erase_transform`` of datasets/kinetics.py:437-444 (None unless cfg.AUG.ENABLE and cfg.AUG.RE_PROB > 0), including
    the reference's ``num_splits=cfg.AUG.RE_COUNT``: with RE_COUNT 2 the first T // 2 frames of every clip stay clean."""
    if not (cfg.AUG.ENABLE and cfg.AUG.RE_PROB > 0):
        return None
    return RandomErasing(cfg.AUG.RE_PROB, mode=cfg.AUG.RE_MODE, max_count=cfg.AUG.RE_COUNT, num_splits=cfg.AUG.RE_COUNT,
                         noise_seed=cfg.RNG_SEED)
