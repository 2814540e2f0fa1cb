"""Per-element parity checks of the convolution family (csrc/sf_igemm.h, sf_igemm2.h, sf_wgrad2.h, the first-generation weight
gradient, the direct convolutions of sf_stem.h, and their launchers in sf_api.hip), shared by tests/test_conv_elem_hostsim.py and
the -m gpu file tests/test_conv_elem_gpu.py.

Method and notation of tests/token_elem_checks.py and tests/attn_elem_checks.py: the reference is torch float64 on the CPU
evaluated on exactly the operands the MFMAs see; every comparison is PER ELEMENT, no element is excluded; u16 = lib.act_eps(),
u32 = 2^-24, TINY = the smallest subnormal of the storage type, ACT the storage type.  Every comparison prints max err / bound.

Operands.  Activations are drawn in ACT.  Weights are fp32 and rounded to ACT exactly as sf_prep_weights rounds them ((f16)v, round
to nearest even == torch's .to(ACT)); rows Cow..Co and columns Cw..Ci of both packed operands are zero (sf_pool.h: prep_element).
Bias, scale and shift are fp32 and taken as they are.  Input channels Cw..Ci hold random finite values: only the zero weight columns
keep them out of the result.

Design roundings restated on the host (the kernels' definition, not their error):
  * in_affine (sf_common.h: bn_act8): a = max((ACT)((float)x * scale + shift), 0) per element, applied to taps INSIDE the input only
    (sf_igemm.h: `has_tf && st.ok[j]`; sf_wgrad_kernel: `has_tf && rb_ok[j]`) -- a padding tap contributes 0, not relu(shift).  The
    expression may or may not be contracted to one fused multiply-add by the compiler, so it is restated twice, a_fma (one rounding
    to fp32) and a_mul (product and sum rounded separately), both then rounded to ACT.  The reference uses a_fma; where the two
    differ (about one element in 2^13 in fp16) the kernel may hold either, which adds conv(|a_fma - a_mul|, |w|) to the bound --
    zero for almost every output.  (a_fma is formed in fp64: the product of an ACT and an fp32 number is exact there, the sum is
    rounded at 2^-53 before the rounding to fp32; a double rounding needs a 2^-29 coincidence and is ignored.)
  * residual epilogues (sf_igemm.h:420-426, i2_epilogue): the tile is rounded to ACT (staged through LDS), THEN the residual is added
    in fp32 and the sum rounded to ACT again.  The tile itself is not observable, so the reference is t + r in fp64 (t = the fp64
    convolution + bias) and the bound gets the first rounding as a term: u16 |t| (+ TINY / 2) and u32 |t + r| for the fp32 sum.
    resid_bits: residual element (m, c) counts only when bit c % 8 of byte [m][c / 8] is set.  ReLU (act_mode 3, the stem's fmaxf) is
    1-Lipschitz and commutes with the rounding: same bound.
  * forward statistics (sf_igemm.h:329-349, i2_epilogue, sf_stem.h:206) are sums of the fp32 ACCUMULATORS (bias included), not of
    the stored values: their reference is the UNROUNDED fp64 convolution.  The BatchNorm that later normalises the stored tensor
    therefore uses statistics taken before the rounding it reads (documented in DESIGN.md and sf_igemm.h).
  * bnb_part of sf_conv_dgrad_bn sums the kernel's OWN STORED dx (read back here), times the mask, and times y: its reference is
    built from the stored tensor.  The recomputed mask is (float)y * scale + shift > 0 in fp32; both evaluations (fused or not) are
    formed and a draw on which they disagree anywhere is rejected by an assert (none of the fixed seeds does).

Bounds, read off the code (nothing is fitted to an observed error):
  E32   = L u32 A for every value that leaves an fp32 accumulator.  A is the same convolution of absolute values, conv(|x|, |w|) in
          fp64 (+ |bias|), likewise for the two gradients; L is the number of terms chained onto one accumulator in whatever
          order: taps x padded channels (Ci forward, Co data gradient; K-padding columns multiply zeros and add nothing), + 1 for
          the bias (acc * alpha + b, alpha = 1 exact), + 1 for the residual.
  stored: |got - ref| <= 2 u16 |ref| + TINY + E32 (1 + u16) (``_assert_stored``); with a residual E32 grows by the terms above.
  fp32  : |got - ref| <= E32 (``_assert_fp32``).
  weight gradient: L = rows chained by one workgroup (rows of one split: chunks_per_split x 32 first generation, rows_per_split
          second generation, twice that + 1 for the LDS sum of the dual kernel, tiles_per_block x 512 tile positions for
          sf_stem_wgrad_kernel) + the slabs sf_wgrad_reduce_kernel sums + 2 (out_scale, accumulate), all from the restated plans
          below; E32 = L u32 (|out_scale| A + |prior dw|).
  tile sums: a sum of n fp32 terms in any order is within (n - 1) u32 sum|term| of the exact sum of the same terms, so D = the
          positions of one partial row (128; 256 for bnb_part of the second generation) covers the lane chain, the wave butterfly and
          the fixed-order sum over waves.  Forward: the terms are accumulators with error E32 each, hence
          |s - ref| <= sum E32 + D u32 sum|ref| and |q - ref| <= sum (2 |ref| E32 + E32^2) + (D + 1) u32 sum ref^2 (+ 1: the square).
          bnb_part: the terms are exact (stored values, products of two ACT numbers are exact in fp32): D u32 sum|term|.
          The direct convolutions of sf_stem.h keep one partial row per 4 x 8 x 16 output TILE (and zero the rows no workgroup owns),
          not per 128 positions, and the sliding forward kernel one per run of tiles: the forward tables are compared as TOTALS
          under the bound of the longer chain, D = all positions (+ the rows summed here).  bnb_part of the thin3 data gradient
          only ever comes from the tile kernels (row b = tile b): it is compared per tile with D = 512.
Padded channels: with Cow < Co the packed weight rows are zero, so the padded output columns are exactly (ACT)bias (0 without a
bias) and their statistics exactly n * bias (0): asserted bit for bit.  dw has exactly Cow x Cw x taps elements (ops.conv_wgrad
asserts the size): it is placed between two guard regions that must stay bit-identical.

Poison and canaries: inputs with a pitch are views of NaN-filled buffers (a stray read poisons the result); outputs are views into a
buffer filled with the bit pattern CANARY, with a guard region before and after, compared bit for bit afterwards.

Which kernel ran: run_igemm, try_igemm2, launch_igemm2_auto, try_igemm2_strided_dgrad, igemm_glds_ok, plan_stem with the forward
launch choice, plan_wgrad and plan_wgrad2 of sf_api.hip are restated below as plain functions that return a variant name.  Every
case states the variant it is there for and the check asserts it; the restatement is cross-checked against
sf_conv_wgrad_rowtab_bytes, sf_conv_wgrad_workspace, sf_conv_fwd_mtiles, the row count sf_conv_dgrad_bn returns and, in one child
process (SF_TRACE is read once), the trace lines of the library.
"""
import os
import subprocess
import sys
from ctypes import byref

import torch
import torch.nn.functional as F

from slowfast_amd import ops, tokens
from slowfast_amd.lib import get_lib
from tests.kernel_checks import ACT
from tests.token_elem_checks import _assert_stored, _pitched
from tests.x3d_checks import TINY, U16, U32, _assert_fp32, _expect_error

NAN = float("nan")
CANARY = 0x5A5B                      # 16-bit pattern of untouched output memory (a finite number in both storage types)
CANARY32 = 0x5A5B5C5D
GUARD = 64                           # elements before and after an output buffer (keeps the 16-byte alignment)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V2 = {"SF_IGEMM2": "1", "SF_IGEMM2_MINK": "32", "SF_IGEMM2_MINROWS": "1"}
W2 = {"SF_WGRAD2": "1", "SF_WGRAD2_MINK": "32", "SF_WGRAD2_MINROWS": "1", "SF_WGRAD2_BLOCKS": "6"}
W2T = dict(W2, SF_WGRAD2T="1", SF_WGRAD2T_MINROWS="1", SF_WGRAD2T_BLOCKS="5")
KNOBS = ("SF_IGEMM2", "SF_IGEMM2_MINK", "SF_IGEMM2_MINROWS", "SF_IGEMM2_T128", "SF_WGRAD2", "SF_WGRAD2_MINK", "SF_WGRAD2_MINROWS",
         "SF_WGRAD2_BLOCKS", "SF_WGRAD2_DUAL", "SF_WGRAD2_DUAL_STEPS", "SF_WGRAD2T", "SF_WGRAD2T_MINROWS", "SF_WGRAD2T_BLOCKS",
         "SF_STEM_SLIDE")

WORST = {}                           # check name -> largest max err / bound seen in this process (the parity report reads it)


def _note(name, got, ref, bound):
    r = float(((got - ref).abs() / bound.clamp(min=1e-300)).max()) if ref.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), r)


def _cdiv(a, b):
    return -(-a // b)


def _roundup(a, b):
    return _cdiv(a, b) * b


def _hook(name, default):
    e = os.environ.get(name)
    return int(e) if e else default


# ------------------------------------------------------------------------------------------------
# sf_api.hip restated
SF_I2_MAXTAPS = 32
STEM_TT, STEM_TH, STEM_TW, STEM_PC, STEM_CHUNKS, STEM_CHUNKS_SMALL, STEM_MAX_SLICES = 4, 8, 16, 19, 3328, 768, 40


def is_pointwise(g):
    return g.k[1] == 1 and g.k[2] == 1 and g.s == (1, 1, 1) and g.p[1] == 0 and g.p[2] == 0 and g.Ho == g.Hi and g.Wo == g.Wi


def igemm_glds_ok(pw, affine, Ktot, C, ld, padT):
    return bool(pw and not affine and Ktot == C and Ktot % 32 == 0 and ld % 8 == 0 and padT == 0)


def igemm2_operands_ok(g, C, ld, affine):
    if affine or g.taps > SF_I2_MAXTAPS or C % 32 != 0 or ld % 8 != 0:
        return False
    return all((g.k[a] - 1) * g.d[a] <= 127 for a in range(3))


def launch_igemm2_auto(M, Nout, C, linear=False, sums=False):
    tiles = _cdiv(M, 256) * _cdiv(Nout, 128 if Nout > 64 else 64)
    bk64 = C % 64 == 0 and tiles <= 320
    t128 = _hook("SF_IGEMM2_T128", 1)
    if t128 and linear and Nout > 64 and not sums and (not bk64 or t128 == 2):
        return "igemm2_t128"
    return "igemm2_bn%d_bk%d" % (128 if Nout > 64 else 64 if Nout > 32 else 32, 64 if bk64 else 32)


def strided_classes(g):
    """try_igemm2_strided_dgrad: (rows, taps) of every non-empty stride-residue class of input positions, in launch order."""
    ext = (g.Ti, g.Hi, g.Wi)
    out = []
    for rt in range(g.s[0]):
        for rh in range(g.s[1]):
            for rw in range(g.s[2]):
                r, cnt = (rt, rh, rw), []
                for a in range(3):
                    num = g.p[a] - r[a]
                    q0 = _cdiv(num, g.s[a]) if num > 0 else 0
                    top = ext[a] - 1 + g.p[a] - r[a]
                    q1 = top // g.s[a] if top >= 0 else -1
                    cnt.append(q1 - q0 + 1)
                if min(cnt) <= 0:
                    continue
                nt = 0
                for kt in range(g.k[0]):
                    for kh in range(g.k[1]):
                        for kw in range(g.k[2]):
                            kk = (kt, kh, kw)
                            nt += all((r[a] - kk[a] * g.d[a]) % g.s[a] == 0 for a in range(3))
                out.append((g.N * cnt[0] * cnt[1] * cnt[2], nt))
    return out


def run_igemm(g, mode, ld, affine=False, sums=False, act=False):
    """run_igemm of sf_api.hip: (variant, rows per M tile | 0).  mode 0 forward (rows = output positions, C = Ci), 1 data gradient."""
    C, Nout, M = (g.Ci, g.Co, g.out_rows) if mode == 0 else (g.Co, g.Ci, g.N * g.Ti * g.Hi * g.Wi)
    Ktot = g.taps * C
    on = _hook("SF_IGEMM2", 1) != 0
    mink, minrows = _hook("SF_IGEMM2_MINK", 512), _hook("SF_IGEMM2_MINROWS", 4096)
    unit = g.s == (1, 1, 1)
    if on and igemm2_operands_ok(g, C, ld, affine) and Ktot >= mink and Nout > 32 and M >= minrows and (mode == 0 or unit):
        return launch_igemm2_auto(M, Nout, C, sums=sums), 256
    if on and mode == 1 and not unit and igemm2_operands_ok(g, C, ld, False) and Nout > 16 and M >= minrows and not act:
        return "igemm2_strided[%s]" % ",".join(str(t) for _, t in strided_classes(g)), 0
    pw = is_pointwise(g)
    gl = igemm_glds_ok(pw, affine, Ktot, C, ld, g.p[0])
    return "igemm_bn%d_%s" % (128 if Nout > 64 else 64 if Nout > 32 else 32 if Nout > 16 else 16,
                              "gl" if gl else "pw" if pw else "gather"), 128


class _D:
    """the descriptor fields plan_stem reads"""

    def __init__(self, g):
        self.Ci, self.Cw, self.Co, self.Cow = g.Ci, g.Cw, g.Co, g.Cow
        self.k, self.s, self.p, self.d = g.k, g.s, g.p, g.d
        self.N, self.To, self.Ho, self.Wo = g.N, g.To, g.Ho, g.Wo


def plan_stem(d):
    stemlike = d.k[2] == 4 and d.p[2] == 2
    thin3 = d.k[2] == 3 and d.p[2] == 1 and d.s[1] == 1 and d.s[0] == 1
    if d.Ci != 8 or d.Cw != 8 or not (stemlike or thin3) or d.s[2] != 1 or d.d != (1, 1, 1):
        return None
    if d.Co > 16 or d.Co % 8 != 0 or (d.Cow and d.Cow != d.Co) or d.k[0] * d.k[1] > STEM_MAX_SLICES:
        return None
    s = dict(thin3=thin3, F=(STEM_TT - 1) * d.s[0] + d.k[0], PR=(STEM_TH - 1) * d.s[1] + d.k[1])
    if s["F"] * s["PR"] * STEM_PC > STEM_CHUNKS:
        return None
    s["small"] = s["F"] * s["PR"] * STEM_PC <= STEM_CHUNKS_SMALL
    s["tiles_t"] = _cdiv(d.To, STEM_TT)
    s["ntiles"] = d.N * s["tiles_t"] * _cdiv(d.Ho, STEM_TH) * _cdiv(d.Wo, STEM_TW)
    gmax = 1024 if s["small"] else 512
    s["tiles_per_block"] = _cdiv(s["ntiles"], min(s["ntiles"], gmax))
    s["wg_blocks"] = _cdiv(s["ntiles"], s["tiles_per_block"])
    s["Kpad"] = _roundup(d.k[0] * d.k[1] * 32, 128)
    nsl = d.k[0] * d.k[1]
    s["wgroups"] = 8 // nsl if nsl <= 4 else 1
    s["ws_bytes"] = s["wg_blocks"] * s["wgroups"] * 16 * s["Kpad"] * 4
    return s


def stem_fwd_launch(d, sp, bnb=False):
    """SF_STEM_FWD_LAUNCH"""
    sg = _hook("SF_STEM_SLIDE", 4)
    if sg > 0 and d.s[1] == 2 and d.k[1] == 7 and not sp["small"] and d.s[0] == 1 and 1 < d.k[0] <= 5 and d.Co <= 8 and not bnb:
        return "stem_slide"
    if d.s[1] == 2 and d.k[1] == 7 and not sp["small"]:
        return "stem_rows_2_7"
    if d.s[1] == 1 and d.k[1] == 3 and sp["small"]:
        return "stem_small_rows_1_3"
    return "stem_small_generic" if sp["small"] else "stem_generic"


def fwd_variant(g, ldx, affine=False, bias=False, stats=True, fused=False, resid=False):
    """sf_conv_fwd / sf_conv_fwd_fused"""
    sp = plan_stem(_D(g))
    if fused:
        if not resid and sp:
            return stem_fwd_launch(_D(g), sp)
    elif not affine and not bias and sp and (not stats or sp["ntiles"] <= _cdiv(g.out_rows, 128)):
        return stem_fwd_launch(_D(g), sp)
    return run_igemm(g, 0, ldx, affine=affine, sums=stats and not fused, act=fused)[0]


def dgrad_variant(g, ldy, resid=False, bn=False):
    """conv_dgrad_impl: (variant, rows of the bnb_part table | None)"""
    M = g.N * g.Ti * g.Hi * g.Wi
    fuse = bn and g.s == (1, 1, 1)
    if not resid and g.Co == 8 and (g.To, g.Ho, g.Wo) == (g.Ti, g.Hi, g.Wi):
        dd = _D(g)
        dd.Ci, dd.Cw, dd.Co, dd.Cow = g.Co, g.Co, g.Ci, 0
        dd.p = tuple(g.k[a] - 1 - g.p[a] for a in range(3))
        dd.To, dd.Ho, dd.Wo = g.Ti, g.Hi, g.Wi
        sp = plan_stem(dd)
        if sp and sp["thin3"] and (not fuse or sp["ntiles"] <= _cdiv(M, 128)):
            return "dgrad_" + stem_fwd_launch(dd, sp, bnb=fuse), (sp["ntiles"] if fuse else None)
    name, bm = run_igemm(g, 1, ldy, sums=fuse)
    return name, (_cdiv(M, bm) if fuse and bm > 0 else None)


def plan_wgrad(g):
    Ktot, M = g.taps * g.Ci, g.out_rows
    w = dict(BMW=128 if g.Co >= 128 else 64 if g.Co >= 64 else 32 if g.Co >= 32 else 16)
    KS = 4 if w["BMW"] <= 32 else 1
    tiles_k, tiles_c = _cdiv(Ktot, 128), _cdiv(g.Co, w["BMW"])
    slab = tiles_c * w["BMW"] * tiles_k * 128 * 4
    nchunks = _cdiv(M, 32)
    splits = _cdiv(1024, tiles_k * tiles_c)
    cap = (256 << 20) // slab
    if splits > cap:
        splits = max(cap, 1)
    nstages = _cdiv(nchunks, KS)
    splits = max(1, min(splits, nstages))
    cps = _cdiv(nstages, splits) * KS
    w["splits"] = _cdiv(nchunks, cps)
    w["rows"] = cps * 32
    w["ws_bytes"] = slab * w["splits"]
    return w


def plan_wgrad2(g):
    if _hook("SF_WGRAD2", 1) == 0:
        return None
    mink, minrows, target = _hook("SF_WGRAD2_MINK", 192), _hook("SF_WGRAD2_MINROWS", 4096), _hook("SF_WGRAD2_BLOCKS", 512)
    Ktot, M = g.taps * g.Ci, g.out_rows
    if g.taps > SF_I2_MAXTAPS or M < minrows or any((g.k[a] - 1) * g.d[a] > 127 for a in range(3)) or plan_stem(_D(g)):
        return None
    tab = _roundup(M * 8, 256) + 1280
    if g.Co <= 32:
        if _hook("SF_WGRAD2T", 1) == 0 or M < _hook("SF_WGRAD2T_MINROWS", 16384):
            return None
        BMW, BKW = (16 if g.Co <= 16 else 32), (32 if Ktot <= 32 else 128)
        tiles_k = _cdiv(Ktot, BKW)
        splits = max(1, _hook("SF_WGRAD2T_BLOCKS", 512 if BKW == 128 else 768 if BMW == 32 else 1024) // tiles_k)
        rps = _roundup(_cdiv(M, splits), 128)
        splits = _cdiv(M, rps)
        return dict(name="wgrad2t_%d_%d" % (BMW, BKW), thin=True, dual=False, rows=rps, splits=splits, slabs=splits, tiles_k=tiles_k,
                    tiles_c=1, tab_bytes=tab, ws_bytes=tab + BMW * tiles_k * BKW * 4 * splits)
    if Ktot < mink:
        return None
    BMW = 128 if g.Co > 64 else 64
    tiles_k, tiles_c = _cdiv(Ktot, 256), _cdiv(g.Co, BMW)
    slab = tiles_c * BMW * tiles_k * 256 * 4
    splits = target // (tiles_k * tiles_c)
    cap = (256 << 20) // slab
    if splits > cap:
        splits = max(cap, 1)
    splits = max(splits, 1)
    dual = False
    if splits >= 2 and _hook("SF_WGRAD2_DUAL", 1) != 0:
        pairs = (target // 2) // (tiles_k * tiles_c)
        steps = _cdiv(_cdiv(M, splits), 32)
        if pairs >= 1 and 2 * pairs * 10 >= max(splits, 2 * pairs) * 9 and steps <= _hook("SF_WGRAD2_DUAL_STEPS", 80):
            dual = True
            splits = min(splits, 2 * pairs)
    rps = _roundup(_cdiv(M, splits), 32)
    splits = _cdiv(M, rps)
    dual = dual and splits >= 2
    return dict(name="wgrad2_%s_%d" % ("dual" if dual else "single", BMW), thin=False, dual=dual, rows=rps, splits=splits,
                slabs=_cdiv(splits, 2) if dual else splits, tiles_k=tiles_k, tiles_c=tiles_c, tab_bytes=tab,
                ws_bytes=tab + slab * splits)


def wgrad_variant(g, affine=False):
    """sf_conv_wgrad: (variant, L of the bound, workspace bytes, row-table bytes)"""
    w1, w2, sp = plan_wgrad(g), plan_wgrad2(g), plan_stem(_D(g))
    ws = max(w1["ws_bytes"], w2["ws_bytes"] if w2 else 0, sp["ws_bytes"] if sp else 0)
    tab = w2["tab_bytes"] if w2 else 0
    if w2 and not affine:
        return w2["name"], w2["rows"] * (2 if w2["dual"] else 1) + int(w2["dual"]) + w2["slabs"] + 2, ws, tab
    if sp and not affine:
        return ("stem_wgrad_%d_%s" % (8 if g.Co <= 8 else 16, "small" if sp["small"] else "big"),
                sp["tiles_per_block"] * STEM_TT * STEM_TH * STEM_TW + sp["wg_blocks"] * sp["wgroups"] + 2, ws, tab)
    return "wgrad_bmw%d" % w1["BMW"], w1["rows"] + w1["splits"] + 2, ws, tab


# ------------------------------------------------------------------------------------------------
# operands, buffers
def _rows(t):
    """NCTHW -> [positions, C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def _cl_in(x, device, extra, off=0):
    """NCTHW values of the storage type -> channels-last view whose pitch is `extra` wider than C, padding filled with NaN; `off`:
    the view starts at channel `off` of the wider rows (a channel slice, as the SlowFast lateral fuse reads and writes)."""
    N, C, T, H, W = x.shape
    if off == 0:
        _, base = _pitched(_rows(x), device, extra)
    else:
        base = torch.full((N * T * H * W, C + extra), NAN, dtype=ACT, device=device)
        base[:, off:off + C] = _rows(x).to(ACT).to(device)
    return base.view(N, T, H, W, C + extra)[..., off:off + C].permute(0, 4, 1, 2, 3)


class _Out:
    """An output tensor of logical shape `shape` at pitch C + extra inside a CANARY-filled buffer with guards on both sides."""

    def __init__(self, shape, device, extra, dtype=None):
        N, C, T, H, W = shape
        self.M, self.C, self.ld = N * T * H * W, C, C + extra
        self.flat = torch.full((2 * GUARD + self.M * self.ld,), CANARY, dtype=torch.int16, device=device).view(ACT)
        self.view = self.flat[GUARD:GUARD + self.M * self.ld].view(N, T, H, W, self.ld)[..., :C].permute(0, 4, 1, 2, 3)

    def rows(self):
        return self.flat[GUARD:GUARD + self.M * self.ld].view(self.M, self.ld)[:, :self.C].detach().cpu().double()

    def assert_canaries(self, name, untouched=False):
        bits = self.flat.detach().cpu().view(torch.int16)
        body = bits[GUARD:GUARD + self.M * self.ld].view(self.M, self.ld)
        assert bool((bits[:GUARD] == CANARY).all()) and bool((bits[-GUARD:] == CANARY).all()), f"{name}: wrote outside its buffer"
        assert bool((body[:, self.C:] == CANARY).all()), f"{name}: wrote into the pitch padding of its output"
        if untouched:
            assert bool((body == CANARY).all()), f"{name}: a rejected call wrote to its output"


def _draw(seed, shape, Cow, k, Cw):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).to(ACT).double()
    w = torch.randn((Cow, Cw) + tuple(k), generator=g) / (Cw * k[0] * k[1] * k[2]) ** 0.5
    return g, x, w


def _f32(t):
    return t.to(torch.float32)


def _affine(g, x):
    """(scale, shift, a_fma, a_mul): the fused input BatchNorm + ReLU of bn_act8 restated in both legal evaluations."""
    C = x.shape[1]
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    s5, h5 = sc.view(1, -1, 1, 1, 1), sh.view(1, -1, 1, 1, 1)
    a_fma = _f32(x * s5.double() + h5.double()).to(ACT).double().clamp(min=0)
    a_mul = (_f32(x) * s5 + h5).to(ACT).double().clamp(min=0)
    return sc, sh, a_fma, a_mul


def _conv64(x, w, g):
    y = F.conv3d(x, w, None, g.s, g.p, g.d)
    return y[:, :, :g.To, :g.Ho, :g.Wo]


def _dgrad64(dy, w, g):
    """d conv3d / d input in fp64 (the convolution is linear: its autograd gradient at zero is the transposed convolution)"""
    x0 = torch.zeros((g.N, w.shape[1], g.Ti, g.Hi, g.Wi), dtype=torch.float64, requires_grad=True)
    _conv64(x0, w, g).backward(dy)
    return x0.grad


def _wgrad64(x, dy, wshape, g):
    w0 = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    _conv64(x, w0, g).backward(dy)
    return w0.grad


def _pad_cols(t, C):
    return torch.cat([t, torch.zeros((t.shape[0], C - t.shape[1]), dtype=t.dtype)], 1) if t.shape[1] < C else t


def _bits_image(g, M, C):
    """random [M, C / 8] bit mask and its boolean [M, C] image"""
    bits = torch.randint(0, 256, (M, C // 8), generator=g, dtype=torch.int32)
    keep = ((bits.unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(M, C).bool()
    return bits.to(torch.uint8), keep


def _tile_sums(t, rows):
    """[M, C] -> [ceil(M / rows), C]: sums over the positions each partial row owns"""
    M, C = t.shape
    nt = _cdiv(M, rows)
    return torch.cat([t, torch.zeros((nt * rows - M, C), dtype=t.dtype)]).view(nt, rows, C).sum(1)


def _stem_tile_sums(t, dims):
    """[M, C] -> [tiles, C]: sums over the positions of each 4 x 8 x 16 tile of sf_stem.h, tiles numbered (n, t, h, w) as stem_tile()"""
    N, T, H, W = dims
    tt, th, tw = _cdiv(T, STEM_TT), _cdiv(H, STEM_TH), _cdiv(W, STEM_TW)
    n, a, b, c = torch.meshgrid(torch.arange(N), torch.arange(T) // STEM_TT, torch.arange(H) // STEM_TH, torch.arange(W) // STEM_TW,
                                indexing="ij")
    tile = (((n * tt + a) * th + b) * tw + c).reshape(-1)
    return torch.zeros((N * tt * th * tw, t.shape[1]), dtype=t.dtype).index_add_(0, tile, t)


def _assert_variant(got, want):
    assert got == want, f"this case is there for {want}, the dispatch restated from sf_api.hip takes {got}"


# ------------------------------------------------------------------------------------------------
def check_fwd(device, shape, Co, k, s=(1, 1, 1), p=(0, 0, 0), d=(1, 1, 1), want=None, Cw=None, affine=False, bias=False, xpad=0,
              ypad=0, xoff=0, seed=0):
    """sf_conv_fwd with its statistics epilogue: y and stat_part per element / per partial row (module docstring)."""
    geom = ops.ConvGeom(shape, Co, k, s, p, d, Cw=Cw)
    gen, x, w = _draw(seed, shape, Co, geom.k, geom.Cw)
    w16 = w.to(ACT).double()
    wf, _ = ops.prep_weights(w.to(device), geom, need_dgrad=False)
    xin, in_affine, da = x, None, None
    if affine:
        sc, sh, xin, a_mul = _affine(gen, x)
        in_affine, da = (sc.to(device), sh.to(device), True), (xin - a_mul).abs()
    b = torch.randn(geom.Co, generator=gen) * 0.5 if bias else None
    xc = _cl_in(x, device, xpad, xoff)
    _assert_variant(fwd_variant(geom, xc.stride(4) if shape[4] > 1 else ops.cl_ld(xc), affine, bias), want)
    M = geom.out_rows
    assert get_lib().call("sf_conv_fwd_mtiles", byref(geom.desc(geom.Ci, geom.Co))) == _cdiv(M, 128)
    out = _Out(geom.out_shape, device, ypad)
    y, part = ops.conv_fwd(xc, wf, geom, in_affine=in_affine, bias=None if b is None else b.to(device), stats=True, out=out.view)
    assert y is out.view and tuple(part.shape) == (_cdiv(M, 128), 2, geom.Co)
    # reference
    ref = _pad_cols(_rows(_conv64(xin[:, :geom.Cw], w16, geom)), geom.Co)
    A = _pad_cols(_rows(_conv64(xin[:, :geom.Cw].abs(), w16.abs(), geom)), geom.Co)
    L = geom.taps * geom.Ci + int(bias)
    if b is not None:
        ref, A = ref + b.double(), A + b.double().abs()
    E = L * U32 * A
    if da is not None:
        E = E + _pad_cols(_rows(_conv64(da[:, :geom.Cw], w16.abs(), geom)), geom.Co)
    name = f"conv_fwd[{want}]"
    got = out.rows()
    out.assert_canaries(name)
    _note("fwd y", got, ref, 2 * U16 * ref.abs() + TINY + E * (1 + U16))
    _assert_stored(name + " y", got, ref, E * (1 + U16))
    part = part.detach().cpu().double()
    if geom.Cow < geom.Co:
        pad_ref = torch.zeros(()) if b is None else b[geom.Cow:].to(ACT).double()
        assert bool((got[:, geom.Cow:] == pad_ref).all()), "padded output columns must be exactly (ACT)bias"
        if b is None:
            assert bool((part[:, :, geom.Cow:] == 0).all()), "statistics of the padded output columns must be exactly 0"
    # statistics: sums of the fp32 accumulators -> the unrounded fp64 convolution
    if want.startswith("stem"):
        D = M
        s_ref, q_ref = ref.sum(0, keepdim=True), (ref * ref).sum(0, keepdim=True)
        s_b = E.sum(0, keepdim=True) + D * U32 * ref.abs().sum(0, keepdim=True)
        q_b = (2 * ref.abs() * E + E * E).sum(0, keepdim=True) + (D + 1) * U32 * q_ref
        s_got, q_got = part[:, 0].sum(0, keepdim=True), part[:, 1].sum(0, keepdim=True)
        s_b, q_b = s_b + part.shape[0] * U32 * ref.abs().sum(0, keepdim=True), q_b + part.shape[0] * U32 * q_ref   # the sum here
    else:
        D = 128
        s_ref, q_ref = _tile_sums(ref, 128), _tile_sums(ref * ref, 128)
        s_b = _tile_sums(E, 128) + D * U32 * _tile_sums(ref.abs(), 128)
        q_b = _tile_sums(2 * ref.abs() * E + E * E, 128) + (D + 1) * U32 * q_ref
        s_got, q_got = part[:, 0], part[:, 1]
    _note("fwd stat sum", s_got, s_ref, s_b)
    _note("fwd stat sumsq", q_got, q_ref, q_b)
    _assert_fp32(name + " stat sum", s_got, s_ref, s_b)
    _assert_fp32(name + " stat sumsq", q_got, q_ref, q_b)


def check_fwd_fused(device, shape, Co, k, s=(1, 1, 1), p=(0, 0, 0), d=(1, 1, 1), want=None, bias=False, resid=False, relu=False,
                    xpad=0, ypad=0, rpad=0, seed=0):
    """sf_conv_fwd_fused: relu?(conv + bias (+ resid)), the tile rounded to ACT before the residual is added."""
    geom = ops.ConvGeom(shape, Co, k, s, p, d)
    gen, x, w = _draw(seed, shape, Co, geom.k, geom.Cw)
    w16 = w.to(ACT).double()
    wf, _ = ops.prep_weights(w.to(device), geom, need_dgrad=False)
    b = torch.randn(geom.Co, generator=gen) * 0.5 if bias else None
    xc = _cl_in(x, device, xpad)
    _assert_variant(fwd_variant(geom, ops.cl_ld(xc), bias=bias, fused=True, resid=resid), want)
    t = _pad_cols(_rows(_conv64(x, w16, geom)), geom.Co)
    A = _pad_cols(_rows(_conv64(x.abs(), w16.abs(), geom)), geom.Co)
    if b is not None:
        t, A = t + b.double(), A + b.double().abs()
    E = (geom.taps * geom.Ci + int(bias)) * U32 * A
    ref, rc = t, None
    if resid:
        r = torch.randn(geom.out_shape, generator=gen).to(ACT).double()
        rc = _cl_in(r, device, rpad)
        ref = t + _rows(r)
        E = (E + U16 * t.abs() + TINY / 2) * (1 + U16) + U32 * ref.abs()
    if relu:
        ref = ref.clamp(min=0)
    out = _Out(geom.out_shape, device, ypad)
    ops.conv_fwd_fused(xc, wf, geom, bias=None if b is None else b.to(device), resid=rc, relu=relu, out=out.view)
    name = f"conv_fwd_fused[{want}]"
    got = out.rows()
    out.assert_canaries(name)
    if relu:
        assert float(got.min()) >= 0.0
    _note("fused y", got, ref, 2 * U16 * ref.abs() + TINY + E * (1 + U16))
    _assert_stored(name, got, ref, E * (1 + U16))


def check_dgrad(device, shape, Co, k, s=(1, 1, 1), p=(0, 0, 0), d=(1, 1, 1), want=None, Cw=None, resid=False, bits=False, bn=None,
                dypad=0, xpad=0, rpad=0, bnpad=0, seed=0):
    """sf_conv_dgrad / sf_conv_dgrad_bn: dx per element; ``bn`` = "affine" | "bits": bnb_part per partial row from the stored dx."""
    geom = ops.ConvGeom(shape, Co, k, s, p, d, Cw=Cw)
    gen, _, w = _draw(seed, shape, Co, geom.k, geom.Cw)
    w16 = w.to(ACT).double()
    _, wd = ops.prep_weights(w.to(device), geom)
    gen = torch.Generator().manual_seed(seed + 2)
    dy = torch.randn(geom.out_shape, generator=gen).to(ACT).double()       # channels Cow..Co random: zero weight rows only
    dyc = _cl_in(dy, device, dypad)
    variant, bn_rows = dgrad_variant(geom, ops.cl_ld(dyc), resid=resid, bn=bn is not None)
    _assert_variant(variant, want)
    Mi, Ci = geom.N * geom.Ti * geom.Hi * geom.Wi, geom.Ci
    t = _pad_cols(_rows(_dgrad64(dy[:, :geom.Cow], w16, geom)), Ci)
    A = _pad_cols(_rows(_dgrad64(dy[:, :geom.Cow].abs(), w16.abs(), geom)), Ci)
    E = geom.taps * geom.Co * U32 * A
    ref, rc, rb = t, None, None
    if resid:
        r = torch.randn(shape, generator=gen).to(ACT).double()
        rc = _cl_in(r, device, rpad)
        rr = _rows(r)
        if bits:
            rb, keep = _bits_image(gen, Mi, Ci)
            rr, rb = rr * keep, rb.to(device)
        ref = t + rr
        E = (E + U16 * t.abs() + TINY / 2) * (1 + U16) + U32 * ref.abs()
    out = _Out(shape, device, xpad)
    name = f"conv_dgrad[{want}]"
    part = None
    if bn is None:
        ops.conv_dgrad(dyc, wd, geom, resid=rc, out=out.view, resid_bits=rb)
    else:
        ybn = torch.randn(shape, generator=gen).to(ACT).double()
        yc = _cl_in(ybn, device, bnpad)
        if bn == "affine":
            sc, sh = torch.rand(Ci, generator=gen) + 0.5, torch.randn(Ci, generator=gen) * 0.3
            yr = _rows(ybn)
            mask = _f32(yr * sc.double() + sh.double()) > 0
            assert torch.equal(mask, (_f32(yr) * sc + sh) > 0), "the draw leaves the recomputed mask ambiguous"
            arg = (yc, sc.to(device), sh.to(device))
        else:
            mb, mask = _bits_image(gen, Mi, Ci)
            arg = {"bits": mb.contiguous().to(device), "y0": yc}
        _, part = ops.conv_dgrad(dyc, wd, geom, resid=rc, out=out.view, resid_bits=rb, bn=arg)
        assert (None if part is None else part.shape[0]) == bn_rows, "rows of the bnb_part table"
    got = out.rows()
    out.assert_canaries(name)
    _note("dgrad dx", got, ref, 2 * U16 * ref.abs() + TINY + E * (1 + U16))
    _assert_stored(name + " dx", got, ref, E * (1 + U16))
    if geom.Cw < Ci and not resid:
        assert bool((got[:, geom.Cw:] == 0).all()), "gradient of the padded input channels must be exactly 0"
    if part is not None:
        part = part.detach().cpu().double()
        tg, tgy = got * mask, got * mask * _rows(ybn)
        if want.startswith("dgrad_stem"):       # the tile kernels write row b for tile b: one row per 4 x 8 x 16 tile of input positions
            D, dims = STEM_TT * STEM_TH * STEM_TW, (geom.N, geom.Ti, geom.Hi, geom.Wi)
            pairs = [(part[:, 0], _stem_tile_sums(tg, dims), D * U32 * _stem_tile_sums(tg.abs(), dims)),
                     (part[:, 1], _stem_tile_sums(tgy, dims), D * U32 * _stem_tile_sums(tgy.abs(), dims))]
        else:
            bm = 256 if want.startswith("igemm2") else 128
            assert bn_rows == _cdiv(Mi, bm)
            pairs = [(part[:, 0], _tile_sums(tg, bm), bm * U32 * _tile_sums(tg.abs(), bm)),
                     (part[:, 1], _tile_sums(tgy, bm), bm * U32 * _tile_sums(tgy.abs(), bm))]
        for (pg, pr, pb), what in zip(pairs, ("sum g", "sum g y")):
            _note(f"bnb_part {what}", pg, pr, pb)
            _assert_fp32(f"{name} bnb_part[{bn}] {what}", pg, pr, pb)
    return variant


def check_wgrad(device, shape, Co, k, s=(1, 1, 1), p=(0, 0, 0), d=(1, 1, 1), want=None, Cw=None, affine=False, out_scale=1.0,
                accumulate=False, xpad=0, dypad=0, seed=0):
    """sf_conv_wgrad: dw (+)= out_scale * dL/dw per element, the plan restated and cross-checked, guards around dw."""
    ops._rowtabs.clear()
    geom = ops.ConvGeom(shape, Co, k, s, p, d, Cw=Cw)
    gen, x, w = _draw(seed, shape, Co, geom.k, geom.Cw)
    gen = torch.Generator().manual_seed(seed + 3)
    dy = torch.randn(geom.out_shape, generator=gen).to(ACT).double()
    xin, in_affine, da = x, None, None
    if affine:
        sc, sh, xin, a_mul = _affine(gen, x)
        in_affine, da = (sc.to(device), sh.to(device), True), (xin - a_mul).abs()
    xc, dyc = _cl_in(x, device, xpad), _cl_in(dy, device, dypad)
    variant, L, ws_bytes, tab_bytes = wgrad_variant(geom, affine)
    _assert_variant(variant, want)
    desc = geom.desc(ops.cl_ld(xc), ops.cl_ld(dyc))
    lib = get_lib()
    assert lib.call("sf_conv_wgrad_workspace", byref(desc)) == ws_bytes, "sf_conv_wgrad_workspace against the restated plans"
    assert lib.call("sf_conv_wgrad_rowtab_bytes", byref(desc)) == tab_bytes, "sf_conv_wgrad_rowtab_bytes against plan_wgrad2"
    n = w.numel()
    flat = torch.full((2 * GUARD + n,), CANARY32, dtype=torch.int32, device=device).view(torch.float32)
    dw = flat[GUARD:GUARD + n].view(w.shape)
    prior = torch.randn(w.shape, generator=gen) if accumulate else torch.full(w.shape, 7.0)
    dw.copy_(prior)
    ops.conv_wgrad(xc, dyc, geom, dw, in_affine=in_affine, out_scale=out_scale, zero_first=not accumulate)
    sc32 = float(torch.tensor(out_scale, dtype=torch.float32))
    G = _wgrad64(xin[:, :geom.Cw], dy[:, :geom.Cow], w.shape, geom)
    A = _wgrad64(xin[:, :geom.Cw].abs(), dy[:, :geom.Cow].abs(), w.shape, geom)
    ref = sc32 * G + (prior.double() if accumulate else 0.0)
    E = L * U32 * (abs(sc32) * A + (prior.double().abs() if accumulate else 0.0))
    if da is not None:
        E = E + abs(sc32) * _wgrad64(da[:, :geom.Cw], dy[:, :geom.Cow].abs(), w.shape, geom)
    bits = flat.detach().cpu().view(torch.int32)
    assert bool((bits[:GUARD] == CANARY32).all()) and bool((bits[-GUARD:] == CANARY32).all()), "sf_conv_wgrad wrote outside dw"
    got = dw.detach().cpu().double()
    _note("wgrad dw", got, ref, E)
    _assert_fp32(f"conv_wgrad[{want}] L = {L}", got, ref, E)


def check_linear_t128(device, M=257, K=64, N=136, seed=0):
    """The `linear` 128 x 128 tile of the second generation (SF_IGEMM2_T128=2) through tokens.gemm with bias and residual."""
    g = torch.Generator().manual_seed(seed)
    a, r = (torch.randn((M, n), generator=g).to(ACT).double() for n in (K, N))
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(ACT)
    b = torch.randn(N, generator=g) * 0.5
    assert launch_igemm2_auto(M, N, K, linear=True) == "igemm2_t128" and K >= _hook("SF_IGEMM2_MINK", 512) and M >= _hook("SF_IGEMM2_MINROWS", 4096)
    av, _ = _pitched(a, device, 8)
    rv, _ = _pitched(r, device, 64)
    flat = torch.full((2 * GUARD + M * (N + 8),), CANARY, dtype=torch.int16, device=device).view(ACT)
    out = flat[GUARD:GUARD + M * (N + 8)].view(M, N + 8)[:, :N]
    tokens.gemm(av, w.to(device), bias=b.to(device), resid=rv, out=out)
    t = a @ w.double().t() + b.double()
    ref = t + r
    E = (K + 1) * U32 * (a.abs() @ w.double().abs().t() + b.double().abs())
    E = (E + U16 * t.abs() + TINY / 2) * (1 + U16) + U32 * ref.abs()
    bits = flat.detach().cpu().view(torch.int16)
    body = bits[GUARD:-GUARD].view(M, N + 8)
    assert bool((bits[:GUARD] == CANARY).all()) and bool((bits[-GUARD:] == CANARY).all()) and bool((body[:, N:] == CANARY).all())
    got = out.detach().cpu().double()
    _note("linear t128", got, ref, 2 * U16 * ref.abs() + TINY + E * (1 + U16))
    _assert_stored("gemm[igemm2_t128]", got, ref, E * (1 + U16))


# ------------------------------------------------------------------------------------------------
def check_rejects(device):
    """Every rejected call returns an error and leaves its outputs untouched."""
    lib = get_lib()
    shape, Co, k, p = (1, 16, 1, 6, 6), 16, (1, 3, 3), (0, 1, 1)
    geom = ops.ConvGeom(shape, Co, k, 1, p)
    gen, x, w = _draw(0, shape, Co, geom.k, geom.Cw)
    wf, wd = ops.prep_weights(w.to(device), geom)
    xc = _cl_in(x, device, 8)
    dyc = _cl_in(torch.randn(geom.out_shape, generator=gen).to(ACT).double(), device, 8)
    st = ops._stream(xc)
    sc = torch.ones(16, device=device)

    def fwd(desc, scale=None, shift=None):
        out = _Out(geom.out_shape, device, 8)
        lib_call = lambda: lib.call("sf_conv_fwd", byref(desc), xc.data_ptr(), wf.data_ptr(), ops._ptr(scale), ops._ptr(shift), 1,  # noqa: E731
                                    None, out.view.data_ptr(), None, st)
        return out, lib_call

    def bad(**kw):
        g2 = ops.ConvGeom(shape, Co, k, 1, p)
        for key, v in kw.items():
            setattr(g2, key, v)
        return g2
    for desc, match in ((geom.desc(28, 24), "bad row pitch"), (geom.desc(8, 24), "bad row pitch"), (geom.desc(24, 20), "bad row pitch"),
                        (geom.desc(24, 8), "bad row pitch"), (bad(Cw=24).desc(24, 24), "Cw must be in"),
                        (bad(Ho=7).desc(24, 24), "exceed the geometry"), (bad(To=2).desc(24, 24), "exceed the geometry")):
        out, call = fwd(desc)
        _expect_error(call, match)
        out.assert_canaries("rejected sf_conv_fwd", untouched=True)
    out, call = fwd(geom.desc(24, 24), scale=sc)
    _expect_error(call, "in_scale/in_shift must come together")
    out.assert_canaries("rejected sf_conv_fwd", untouched=True)
    # data gradient: residual pitch
    out = _Out(shape, device, 8)
    for ldr in (20, 8):
        _expect_error(lambda: lib.call("sf_conv_dgrad", byref(geom.desc(24, 24)), dyc.data_ptr(), wd.data_ptr(), xc.data_ptr(), ldr,
                                       None, out.view.data_ptr(), st), "bad residual pitch")
    out.assert_canaries("rejected sf_conv_dgrad", untouched=True)
    # weight gradient
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=device)

    def wgrad(g2, xt, dyt, dw, scale=None, shift=None, ws_bytes=None, rowtab=None):
        return lambda: lib.call("sf_conv_wgrad", byref(g2.desc(ops.cl_ld(xt), ops.cl_ld(dyt))), xt.data_ptr(), ops._ptr(scale),
                                ops._ptr(shift), 1, dyt.data_ptr(), dw.data_ptr(), 1.0, 1, ws.data_ptr(),
                                ws.numel() if ws_bytes is None else ws_bytes, rowtab, st)
    dw = torch.full(w.shape, 7.0, device=device)
    _expect_error(wgrad(geom, xc, dyc, dw, scale=sc), "in_scale/in_shift must come together")
    _expect_error(wgrad(geom, xc, dyc, dw, ws_bytes=64), "workspace too small")
    big = ops.ConvGeom((1, 520, 1, 2, 2), 16, (1, 1, 1))
    xb = _cl_in(torch.zeros((1, 520, 1, 2, 2), dtype=torch.float64), device, 0)
    dyb = _cl_in(torch.zeros(big.out_shape, dtype=torch.float64), device, 0)
    scb = torch.ones(520, device=device)
    dwb = torch.full((16, 520, 1, 1, 1), 7.0, device=device)
    _expect_error(wgrad(big, xb, dyb, dwb, scale=scb, shift=scb), "supports Ci <= 512")
    assert bool((dwb == 7.0).all())
    for key, v in dict(W2, SF_WGRAD2_BLOCKS="2").items():
        os.environ[key] = v                     # the caller's monkeypatch restores the environment
    g64 = ops.ConvGeom((1, 64, 1, 6, 6), 64, (1, 3, 3), 1, (0, 1, 1))
    assert plan_wgrad2(g64) is not None
    x64 = _cl_in(torch.zeros(g64.in_shape, dtype=torch.float64), device, 0)
    dy64 = _cl_in(torch.zeros(g64.out_shape, dtype=torch.float64), device, 0)
    dw64 = torch.full((64, 64, 1, 3, 3), 7.0, device=device)
    _expect_error(wgrad(g64, x64, dy64, dw64, ws_bytes=1024), "workspace too small")
    tab = torch.empty(plan_wgrad2(g64)["tab_bytes"] + 16, dtype=torch.uint8, device=device)
    _expect_error(wgrad(g64, x64, dy64, dw64, rowtab=tab.data_ptr() + 8), "rowtab must be 16-byte aligned")
    _expect_error(lambda: lib.call("sf_conv_wgrad_rowtab", byref(g64.desc(64, 64)), tab.data_ptr() + 8, st), "16-byte aligned")
    assert bool((dw == 7.0).all()) and bool((dw64 == 7.0).all()), "a rejected sf_conv_wgrad wrote to dw"


# ------------------------------------------------------------------------------------------------
# SF_TRACE: read once per process by two of the launchers, so every trace line is checked in ONE child process
TRACE_ENV = dict(V2, **W2T, SF_TRACE="1")


def _trace_main(kind):
    """child process: run one case per traced launcher, print the lines the restated plans expect; the parent compares them with
    what the library wrote to stderr."""
    device = torch.device("cuda:0" if kind == "gpu" else "cpu")
    exp = []

    def i2(g, mode, **kw):
        C, Nout, M = (g.Ci, g.Co, g.out_rows) if mode == 0 else (g.Co, g.Ci, g.N * g.Ti * g.Hi * g.Wi)
        bk = launch_igemm2_auto(M, Nout, C, **kw).rsplit("bk", 1)[1]
        exp.append("igemm2: M=%d N=%d C=%d taps=%d BK=%s omap=0" % (M, Nout, C, g.taps, bk))
    # BK 64 and BK 32 on 64 channels: the `tiles <= 320` rule, not C % 64
    c = ((1, 64, 2, 9, 9), 64, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    check_fwd(device, *c, want="igemm2_bn64_bk64")
    i2(ops.ConvGeom(*c), 0, sums=True)
    c = ((321, 64, 1, 16, 16), 64, (1, 1, 1))
    check_fwd(device, *c, want="igemm2_bn64_bk32")
    i2(ops.ConvGeom(*c), 0, sums=True)
    c = ((1, 96, 1, 8, 8), 96, (1, 3, 3), (1, 1, 1), (0, 2, 2), (1, 2, 2))
    check_dgrad(device, *c, want="igemm2_bn128_bk32")
    i2(ops.ConvGeom(*c), 1)
    # strided data gradient: one line per residue class
    c = ((1, 64, 2, 10, 10), 64, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    check_dgrad(device, *c, want="igemm2_strided[4,2,2,1]")
    for rows, taps in strided_classes(ops.ConvGeom(*c)):
        exp.append("igemm2: M=%d N=64 C=64 taps=%d BK=64 omap=1" % (rows, taps))
    # weight gradients
    for c, blocks, want in ((((2, 64, 3, 12, 12), 136, (1, 3, 3), (1, 1, 1), (0, 1, 1)), "48", "wgrad2_dual_128"),
                            (((1, 64, 2, 9, 9), 64, (1, 3, 3), (1, 1, 1), (0, 1, 1)), "15", "wgrad2_single_64"),
                            (((2, 16, 3, 10, 10), 16, (1, 3, 3), (1, 1, 1), (0, 1, 1)), "6", "wgrad2t_16_128")):
        os.environ["SF_WGRAD2_BLOCKS"] = blocks
        check_wgrad(device, *c, want=want)
        g = ops.ConvGeom(*c)
        w2 = plan_wgrad2(g)
        exp.append("wgrad2: M=%d Co=%d K=%d tiles %dx%d splits %d%s" % (g.out_rows, g.Co, g.taps * g.Ci, w2["tiles_c"], w2["tiles_k"],
                                                                        w2["splits"], " (two per workgroup)" if w2["dual"] else ""))
    c = ((2, 8, 6, 36, 22), 8, (5, 7, 4), (1, 2, 1), (2, 3, 2))
    check_wgrad(device, *c, want="stem_wgrad_8_big")
    check_fwd(device, *c, want="stem_slide")
    sp = plan_stem(_D(ops.ConvGeom(*c)))
    exp.append("stem_wgrad: %d workgroups x %d tiles" % (sp["wg_blocks"], sp["tiles_per_block"]))
    g = ops.ConvGeom(*c)
    seg = min(4, sp["tiles_t"])
    exp.append("stem_fwd: %d tiles, patch %dx%dx%d chunks" % (sp["ntiles"], sp["F"], sp["PR"], STEM_PC))
    exp.append("stem_fwd_slide: %d runs of %d groups" % (sp["ntiles"] // sp["tiles_t"] * _cdiv(sp["tiles_t"], seg), seg))
    for line in exp:
        print("EXPECT [sfamd] " + line)


def check_trace(kind):
    env = dict(os.environ, **TRACE_ENV)
    for key in ("SF_IGEMM2_T128", "SF_STEM_SLIDE", "SF_WGRAD2_DUAL", "SF_WGRAD2_DUAL_STEPS"):
        env.pop(key, None)
    if kind == "gpu":
        env.pop("SFAMD_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", f"from tests import conv_elem_checks as cc; cc._trace_main({kind!r})"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    want = [line[len("EXPECT "):] for line in r.stdout.splitlines() if line.startswith("EXPECT ")]
    got = [line for line in r.stderr.splitlines() if line.startswith("[sfamd] ") and
           any(tag in line for tag in ("igemm2:", "wgrad2:", "stem_wgrad:", "stem_fwd_slide:", "stem_fwd:"))]
    assert len(want) >= 12 and got == want, "trace lines of the library against the restated plans:\n" + "\n".join(
        f"  {a!s:70} | {b!s}" for a, b in zip(got + [None] * len(want), want + [None] * len(got)) if a or b)


# ------------------------------------------------------------------------------------------------
# Cases: (id, check, (in_shape, Co, kernel, stride, pad, dilation), environment, variant the case is there for, options)
def _case(cid, check, args, env, want, **kw):
    return (cid, check, args, env, want, kw)


def _pads(i):
    """every case of a shape list runs pitched: 8 / 64 elements wider than the channel count, alternating"""
    return (8, 64) if i % 2 == 0 else (64, 8)


def _from_lists():
    from tests.test_igemm2_hostsim import BORDER_CASES, CASES, STRIDED, THIN_CASES, WGRAD2_CASES, WGRAD2_DUAL_CASES, WGRAD2T_CASES
    from tests.test_kernels_hostsim import CONV_CASES, STEM_CASES
    fwd, dgrad, wgrad = [], [], []

    def add(tag, cases, env, wf=None, wd=None, ww=None, **kw):
        for i, c in enumerate(cases):
            a, b = _pads(i)
            if wf:
                fwd.append(_case(f"{tag}{i}", "fwd", c, env, wf[i], xpad=a, ypad=b, **kw))
            if wd:
                dgrad.append(_case(f"{tag}{i}", "dgrad", c, env, wd[i], dypad=a, xpad=b, **kw))
            if ww:
                wgrad.append(_case(f"{tag}{i}", "wgrad", c, env, ww[i], xpad=a, dypad=b, **kw))
    add("conv", CONV_CASES, {},
        ["igemm_bn32_pw", "igemm_bn64_gather", "igemm_bn16_pw", "stem_small_rows_1_3", "igemm_bn32_gather", "igemm_bn16_gather",
         "igemm_bn16_gather", "igemm_bn128_pw"],
        ["igemm_bn16_gl", "igemm_bn32_gather", "igemm_bn16_pw", "dgrad_stem_small_rows_1_3", "igemm_bn16_gather", "igemm_bn16_gather",
         "igemm_bn16_gather", "igemm_bn128_pw"],
        ["wgrad_bmw32", "wgrad_bmw64", "wgrad_bmw16", "stem_wgrad_8_small", "wgrad_bmw16", "wgrad_bmw16", "wgrad_bmw16", "wgrad_bmw128"])
    add("stem", STEM_CASES, {}, ["stem_slide", "stem_rows_2_7", "stem_generic"], None,
        ["stem_wgrad_8_big", "stem_wgrad_16_big", "stem_wgrad_8_big"], Cw=8)
    add("stem_noslide", STEM_CASES[:1], {"SF_STEM_SLIDE": "0"}, ["stem_rows_2_7"], Cw=8)
    add("v2_", CASES, V2,
        ["igemm2_bn64_bk64", "igemm2_bn128_bk64", "igemm2_bn64_bk64", "igemm2_bn64_bk32", "igemm2_bn128_bk32", "igemm2_bn128_bk64",
         "igemm2_bn128_bk64", "igemm2_bn128_bk64"],
        ["igemm2_bn64_bk64", "igemm_bn64_gather", "igemm2_bn128_bk64", "igemm_bn32_gather", "igemm_bn128_gather",
         "igemm2_strided[2,2,2,1]", "igemm2_bn128_bk64", "igemm2_bn64_bk32"])
    add("border", BORDER_CASES[3:4] + BORDER_CASES[5:], V2, ["igemm2_bn128_bk32", "igemm2_bn64_bk32", "igemm2_bn128_bk32"],
        ["igemm2_bn128_bk32", "igemm_bn32_gather", "igemm2_bn128_bk64"])
    add("strided", STRIDED, V2, None, ["igemm2_strided[4,2,2,1]", "igemm2_strided[1,0,0,0]", "igemm2_strided[2,2,2,1]",
                                       "igemm2_strided[9,0,0,0]", "igemm2_strided[8,4,4,2,4,2,2,1]"])
    add("thin", THIN_CASES, {},
        ["stem_small_rows_1_3", "igemm_bn16_pw", "igemm_bn32_pw", "igemm_bn16_pw", "igemm_bn32_gather", "igemm_bn16_gather",
         "igemm_bn16_gather", "igemm_bn16_gather"],
        ["dgrad_stem_small_rows_1_3", "igemm_bn32_pw", "igemm_bn16_gl", "igemm_bn16_pw", "igemm_bn16_gather",
         "dgrad_stem_small_rows_1_3", "igemm_bn16_gather", "igemm_bn16_gather"])
    add("w2_", WGRAD2_CASES, W2, None, None,
        ["wgrad2_dual_64", "wgrad2_single_128", "wgrad2_single_64", "wgrad2_single_64", "wgrad2_single_128", "wgrad2_single_128",
         "wgrad2_single_128", "wgrad2_single_128", "wgrad2_dual_64"])
    # of the four WGRAD2_DUAL_CASES only the first still plans two splits per workgroup: since the pairs must fill the chip as
    # well as the single splits did (sf_api.hip: 2 * pairs * 10 >= splits * 9) the block counts 30 / 12 / 15 plan single splits
    for i, ((c, blocks), want) in enumerate(zip(WGRAD2_DUAL_CASES, ["wgrad2_dual_128", "wgrad2_single_128", "wgrad2_single_128",
                                                                    "wgrad2_single_64"])):
        env = dict(W2, SF_WGRAD2_BLOCKS=str(blocks))
        wgrad.append(_case(f"w2dual{i}", "wgrad", c, env, want, xpad=8, dypad=64))
        wgrad.append(_case(f"w2dual{i}_off", "wgrad", c, dict(env, SF_WGRAD2_DUAL="0"), want.replace("dual", "single")))
    add("w2t_", WGRAD2T_CASES, W2T, None, None,
        ["wgrad2t_16_128", "wgrad2t_16_128", "wgrad2t_32_32", "wgrad2t_16_32", "wgrad2t_16_128", "wgrad2t_32_128", "wgrad2t_32_128",
         "wgrad2t_16_128"])
    return fwd, dgrad, wgrad


_P1, _P3, _D1 = (0, 1, 1), (1, 3, 3), (1, 1, 1)
S1, S2 = (1, 1, 1), (1, 2, 2)
FWD_CASES, DGRAD_CASES, WGRAD_CASES = _from_lists()
FWD_CASES += [
    # the two ragged thin3 shapes of test_kernels_gpu.py
    _case("thin3_co16", "fwd", ((2, 8, 5, 30, 30), 16, _P3, S1, _P1), {}, "stem_small_rows_1_3", xpad=8, ypad=64),
    _case("thin3_333", "fwd", ((2, 8, 6, 14, 14), 8, (3, 3, 3), S1, (1, 1, 1)), {}, "stem_generic", xpad=64, ypad=8),
    # ---- first generation: the four column tiles, direct-to-LDS pointwise (K % 32 == 0) and register-staged pointwise (K = 8, 16, 24,
    # 40), 128 k + 1 rows, fewer than 16 rows
    _case("bn16_gl_129rows", "fwd", ((1, 32, 1, 3, 43), 8, S1), {}, "igemm_bn16_gl", xpad=8, ypad=8),
    _case("bn32_pw_K8_9rows", "fwd", ((1, 8, 1, 3, 3), 24, S1), {}, "igemm_bn32_pw", xpad=64, ypad=64),
    _case("bn64_pw_K16_129rows", "fwd", ((1, 16, 1, 3, 43), 40, S1), {}, "igemm_bn64_pw", xpad=8, ypad=64, bias=True),
    _case("bn128_pw_K24", "fwd", ((1, 24, 1, 5, 5), 72, S1), {}, "igemm_bn128_pw", xpad=64, ypad=8),
    _case("bn16_pw_K40", "fwd", ((1, 40, 1, 5, 5), 16, S1), {}, "igemm_bn16_pw", xpad=8, ypad=64),
    _case("bn128_gl_9rows_2ntiles", "fwd", ((1, 64, 1, 3, 3), 136, S1), {}, "igemm_bn128_gl", xpad=64, ypad=8),
    _case("bn64_gl_54to56_bias", "fwd", ((1, 32, 1, 5, 5), 54, S1), {}, "igemm_bn64_gl", xpad=8, ypad=8, bias=True),     # Cow < Co
    _case("bn64_gather", "fwd", ((1, 8, 1, 5, 5), 40, _P3, S1, _P1), {}, "igemm_bn64_gather", xpad=8, ypad=64),
    _case("bn128_gather_bias", "fwd", ((1, 16, 1, 5, 5), 72, _P3, S1, _P1), {}, "igemm_bn128_gather", ypad=8, bias=True),
    # ---- in_affine: padding taps must contribute 0 (spatial padding through the gather, temporal through the pointwise decode);
    # it keeps a pointwise layer off the direct-to-LDS copies
    _case("affine_pad_taps", "fwd", ((1, 16, 1, 7, 7), 16, _P3, S1, _P1), {}, "igemm_bn16_gather", affine=True, xpad=8, ypad=8),
    _case("affine_temporal_pad", "fwd", ((1, 16, 3, 3, 3), 16, (3, 1, 1), S1, (1, 0, 0)), {}, "igemm_bn16_pw", affine=True, xpad=64),
    _case("affine_no_gl_bias", "fwd", ((1, 32, 1, 5, 5), 32, S1), {}, "igemm_bn32_pw", affine=True, bias=True, ypad=64),
    _case("affine_keeps_gen1", "fwd", ((1, 64, 2, 9, 9), 64, _P3, S1, _P1), V2, "igemm_bn64_gather", affine=True, xpad=8),
    # ---- Cw < Ci: the stem's 3 channels in 8 (the other 5 input channels hold random values)
    _case("stem_3in8", "fwd", ((1, 8, 1, 12, 12), 8, (1, 7, 7), S2, (0, 3, 3)), {}, "igemm_bn16_gather", Cw=3, xpad=8, ypad=8),
    _case("stem_3in8_co64", "fwd", ((1, 8, 1, 12, 12), 64, (1, 7, 7), S2, (0, 3, 3)), {}, "igemm_bn64_gather", Cw=3, ypad=64),
    # ---- a channel slice at a non-zero channel offset of a wider tensor (the lateral fuse), both generations
    _case("slice_gen1", "fwd", ((1, 16, 1, 6, 6), 32, S1), {}, "igemm_bn32_pw", xpad=24, xoff=8, ypad=8),
    _case("slice_gen1_gl", "fwd", ((1, 32, 1, 6, 6), 32, S1), {}, "igemm_bn32_gl", xpad=16, xoff=8, ypad=8),
    _case("slice_igemm2", "fwd", ((1, 64, 1, 9, 9), 64, _P3, S1, _P1), V2, "igemm2_bn64_bk64", xpad=32, xoff=16, ypad=64),
    # ---- second generation: M = 257 (a second tile with one live row, a third statistics row with one position); padded channels
    _case("i2_M257", "fwd", ((1, 64, 1, 1, 257), 64, (1, 1, 3), S1, (0, 0, 1)), V2, "igemm2_bn64_bk64", xpad=8, ypad=8),
    _case("i2_136_bias", "fwd", ((1, 32, 1, 5, 27), 136, S1), V2, "igemm2_bn128_bk32", xpad=8, ypad=8, bias=True),
    _case("i2_54to56", "fwd", ((1, 64, 1, 5, 27), 54, S1), V2, "igemm2_bn64_bk64", xpad=64, ypad=8),
    # ---- stem forward by geometry and by SF_STEM_SLIDE=0: row-major 2 / 7 (kT = 1: never slides), the small patch with the generic
    # loop (kH = 1), the small row-major 1 / 3, the generic loop on the big patch
    _case("stem_small_generic", "fwd", ((1, 8, 4, 8, 32), 8, (1, 1, 3), S1, (0, 0, 1)), {}, "stem_small_generic", xpad=8, ypad=64),
    _case("stem_co16_noslide", "fwd", ((1, 8, 3, 20, 20), 16, (1, 7, 4), (1, 2, 1), (0, 3, 2)), {"SF_STEM_SLIDE": "0"}, "stem_rows_2_7",
          Cw=8, xpad=64, ypad=8),
    _case("stem_slide_1group", "fwd", ((1, 8, 9, 20, 20), 8, (5, 7, 4), (1, 2, 1), (2, 3, 2)), {"SF_STEM_SLIDE": "1"}, "stem_slide",
          Cw=8, xpad=8, ypad=8),
]
DGRAD_CASES += [
    _case("thin3_ci16", "dgrad", ((2, 16, 5, 30, 30), 8, _P3, S1, _P1), {}, "dgrad_stem_small_rows_1_3", dypad=8, xpad=64),
    _case("thin3_333", "dgrad", ((2, 8, 6, 14, 14), 8, (3, 3, 3), S1, (1, 1, 1)), {}, "dgrad_stem_generic", dypad=64, xpad=8),
    # ---- first generation: column tiles by Ci, 129 rows, 9 rows, residual and its bit mask, every operand pitched
    _case("bn16_gl_129rows_resid", "dgrad", ((1, 8, 1, 3, 43), 32, S1), {}, "igemm_bn16_gl", resid=True, dypad=8, xpad=8, rpad=64),
    _case("bn64_pw_9rows_bits", "dgrad", ((1, 40, 1, 3, 3), 24, S1), {}, "igemm_bn64_pw", resid=True, bits=True, dypad=64, xpad=64, rpad=8),
    _case("bn128_gather_resid", "dgrad", ((1, 72, 1, 5, 5), 16, _P3, S1, _P1), {}, "igemm_bn128_gather", resid=True, xpad=8, rpad=8),
    _case("bn32_gather_3in8", "dgrad", ((1, 8, 1, 12, 12), 24, (1, 7, 7), S2, (0, 3, 3)), {}, "igemm_bn16_gather", Cw=3, dypad=8),
    # ---- the fused BatchNorm-backward sums per partial row, both mask forms: first generation (129 rows: a second row of one
    # position), second generation (257 rows), the thin3 direct convolution (totals)
    _case("bnb_gen1_affine", "dgrad", ((1, 16, 1, 3, 43), 32, S1), {}, "igemm_bn16_gl", bn="affine", dypad=8, xpad=8, bnpad=64),
    _case("bnb_gen1_bits_resid", "dgrad", ((1, 40, 1, 3, 43), 16, _P3, S1, _P1), {}, "igemm_bn64_gather", bn="bits", resid=True, bits=True,
          dypad=64, xpad=64, rpad=8, bnpad=8),
    _case("bnb_i2_affine", "dgrad", ((1, 64, 1, 1, 257), 64, (1, 1, 3), S1, (0, 0, 1)), V2, "igemm2_bn64_bk64", bn="affine", resid=True,
          dypad=8, xpad=64, rpad=8, bnpad=8),
    _case("bnb_i2_bits", "dgrad", ((1, 136, 2, 9, 9), 64, _P3, S1, _P1), V2, "igemm2_bn128_bk64", bn="bits", dypad=64, xpad=8, bnpad=64),
    _case("bnb_thin3_affine", "dgrad", ((2, 8, 3, 10, 10), 8, _P3, S1, _P1), {}, "dgrad_stem_small_rows_1_3", bn="affine", dypad=8,
          xpad=8, bnpad=64),
    _case("bnb_thin3_bits", "dgrad", ((1, 8, 4, 8, 32), 8, (3, 3, 3), S1, (1, 1, 1)), {}, "dgrad_stem_generic", bn="bits", dypad=64,
          xpad=64, bnpad=8),
    _case("bnb_strided_none", "dgrad", ((1, 32, 2, 9, 9), 64, S1, S2), V2, "igemm2_strided[1,0,0,0]", bn="affine", bnpad=8),
    # ---- second generation: residual with and without its bit mask, strided classes with a residual (tap-less classes then store
    # the residual alone; without one, zeros), the 32-wide tile (24 input channels)
    _case("i2_resid_bits", "dgrad", ((1, 64, 2, 9, 9), 64, _P3, S1, _P1), V2, "igemm2_bn64_bk64", resid=True, bits=True, dypad=8, xpad=8,
          rpad=64),
    _case("i2_M257_resid", "dgrad", ((1, 128, 1, 1, 257), 64, S1), V2, "igemm2_bn128_bk64", resid=True, dypad=64, xpad=64, rpad=8),
    _case("strided_tapless_resid", "dgrad", ((1, 32, 2, 9, 9), 64, S1, S2), V2, "igemm2_strided[1,0,0,0]", resid=True, dypad=8, xpad=8,
          rpad=64),
    _case("strided_taps_resid_bits", "dgrad", ((1, 32, 9, 4, 4), 64, (7, 1, 1), (4, 1, 1), (3, 0, 0)), V2, "igemm2_strided[2,2,2,1]",
          resid=True, bits=True, dypad=64, xpad=64, rpad=8),
    _case("strided_bn32_resid", "dgrad", ((2, 24, 3, 8, 8), 96, (3, 3, 3), (2, 2, 2), (1, 1, 1)), V2,
          "igemm2_strided[8,4,4,2,4,2,2,1]", resid=True, xpad=8, rpad=8),
]
WGRAD_CASES += [
    # ---- first generation: in_affine always takes it (also under the lowered second-generation thresholds); K < 192
    _case("gen1_affine_under_w2", "wgrad", ((1, 64, 2, 9, 9), 64, _P3, S1, _P1), W2, "wgrad_bmw64", affine=True, xpad=8, dypad=64),
    _case("gen1_affine_acc_scale", "wgrad", ((1, 16, 1, 7, 7), 16, _P3, S1, _P1), {}, "wgrad_bmw16", affine=True, out_scale=0.25,
          accumulate=True, xpad=64, dypad=8),
    _case("gen1_bmw128_acc", "wgrad", ((1, 16, 1, 5, 27), 136, S1), {}, "wgrad_bmw128", accumulate=True, out_scale=-0.5, xpad=8, dypad=8),
    _case("gen1_3in8", "wgrad", ((1, 8, 1, 12, 12), 8, (1, 7, 7), S2, (0, 3, 3)), {}, "wgrad_bmw16", Cw=3, xpad=8, dypad=64),
    _case("gen1_54", "wgrad", ((1, 32, 1, 5, 5), 54, S1), {}, "wgrad_bmw32", xpad=64, dypad=8),                        # Cow < Co
    # ---- second generation, two splits per workgroup with an ODD split count: the last pair's second half has no rows
    _case("dual64_5splits", "wgrad", ((1, 64, 2, 8, 9), 64, _P3, S1, _P1), dict(W2, SF_WGRAD2_BLOCKS="18"), "wgrad2_dual_64",
          xpad=8, dypad=64, accumulate=True, out_scale=0.25),
    _case("dual128_7splits", "wgrad", ((2, 64, 3, 12, 12), 136, _P3, S1, _P1), dict(W2, SF_WGRAD2_BLOCKS="48"), "wgrad2_dual_128",
          xpad=64, dypad=8),
    _case("single64_5splits_acc", "wgrad", ((1, 64, 2, 8, 9), 64, _P3, S1, _P1), dict(W2, SF_WGRAD2_BLOCKS="18", SF_WGRAD2_DUAL="0"),
          "wgrad2_single_64", accumulate=True, out_scale=2.0),
    # ---- the thin kernel accumulating; the four sf_stem_wgrad_kernel instances (two above: 8_small, 8_big, 16_big)
    _case("w2t_acc_scale", "wgrad", ((2, 8, 2, 9, 9), 32, S1), W2T, "wgrad2t_32_32", accumulate=True, out_scale=0.25, xpad=8, dypad=8),
    _case("stem16_small", "wgrad", ((1, 8, 2, 9, 17), 16, _P3, S1, _P1), {}, "stem_wgrad_16_small", xpad=8, dypad=64),
    _case("stem8_small_acc", "wgrad", ((1, 8, 2, 9, 17), 8, _P3, S1, _P1), {}, "stem_wgrad_8_small", accumulate=True, out_scale=0.5,
          xpad=64, dypad=8),
    _case("stem16_big_acc", "wgrad", ((1, 8, 3, 20, 20), 16, (1, 7, 4), (1, 2, 1), (0, 3, 2)), {}, "stem_wgrad_16_big", Cw=8,
          accumulate=True, xpad=8, dypad=8),
]
# sf_conv_fwd_fused: bias, residual and ReLU each alone and together, on both generations and on the stem kernel (no residual there:
# a residual keeps the stem shapes on the implicit GEMM)
_FUSED_OPTS = [dict(bias=True), dict(resid=True), dict(relu=True), dict(bias=True, resid=True, relu=True)]
FUSED_CASES = []
for _i, _o in enumerate(_FUSED_OPTS):
    _a, _b = _pads(_i)
    _tag = "_".join(sorted(_o))
    FUSED_CASES += [
        _case(f"gen1_{_tag}", "fused", ((1, 16, 1, 3, 43), 40, S1), {}, "igemm_bn64_pw", xpad=_a, ypad=_b, rpad=_a, **_o),
        _case(f"i2_{_tag}", "fused", ((1, 64, 2, 9, 9), 72, _P3, S1, _P1), V2, "igemm2_bn128_bk64", xpad=_b, ypad=_a, rpad=_b, **_o),
        _case(f"stem_{_tag}", "fused", ((1, 8, 9, 20, 20), 8, (5, 7, 4), (1, 2, 1), (2, 3, 2)), {},
              "igemm_bn16_gather" if "resid" in _o else "stem_slide", xpad=_a, ypad=_b, rpad=_b, **_o),
    ]
FUSED_CASES.append(_case("thin3_bias_relu", "fused", ((1, 8, 2, 9, 17), 16, _P3, S1, _P1), {}, "stem_small_rows_1_3", bias=True, relu=True,
                         xpad=8, ypad=8))
# GPU only -- the product's own thresholds, one shape just above each and one just below (the first-generation kernel)
UNFORCED_CASES = [
    _case("igemm2_at_K576_M4096", "fwd", ((1, 64, 1, 64, 64), 64, _P3, S1, _P1), {}, "igemm2_bn64_bk64", xpad=8, ypad=8),
    _case("igemm2_dgrad_at", "dgrad", ((1, 64, 1, 64, 64), 64, _P3, S1, _P1), {}, "igemm2_bn64_bk64", bn="affine", dypad=8, xpad=8),
    _case("below_M4095", "fwd", ((1, 64, 1, 63, 65), 64, _P3, S1, _P1), {}, "igemm_bn64_gather", xpad=8, ypad=8),
    _case("below_K288", "fwd", ((1, 32, 1, 64, 64), 64, _P3, S1, _P1), {}, "igemm_bn64_gather", ypad=8),
    _case("below_N32", "fwd", ((1, 64, 1, 64, 64), 32, _P3, S1, _P1), {}, "igemm_bn32_gather", xpad=8),
    _case("wgrad2_at", "wgrad", ((1, 64, 1, 64, 64), 64, _P3, S1, _P1), {}, "wgrad2_dual_64", xpad=8, dypad=8),
    _case("wgrad2_below_M4095", "wgrad", ((1, 64, 1, 63, 65), 64, _P3, S1, _P1), {}, "wgrad_bmw64", dypad=8),
    _case("wgrad2_below_K160", "wgrad", ((1, 160, 1, 64, 64), 64, S1), {}, "wgrad_bmw64", xpad=8),
    _case("wgrad2t_at_M16384", "wgrad", ((1, 16, 4, 64, 64), 16, S1), {}, "wgrad2t_16_32", xpad=8, dypad=8),
    _case("wgrad2t_below_M16383", "wgrad", ((1, 16, 3, 43, 127), 16, S1), {}, "wgrad_bmw16", dypad=8),
    _case("strided_at_M4096", "dgrad", ((1, 32, 1, 64, 64), 64, S1, S2), {}, "igemm2_strided[1,0,0,0]", resid=True, dypad=8, xpad=8, rpad=8),
    _case("strided_below_M4095", "dgrad", ((1, 32, 1, 63, 65), 64, S1, S2), {}, "igemm_bn32_gather", dypad=8),
]
CHECKS = {"fwd": check_fwd, "fused": check_fwd_fused, "dgrad": check_dgrad, "wgrad": check_wgrad}


def run_case(device, monkeypatch, case):
    """One case under its thresholds (the dispatcher reads them per call): no cached row table or workspace size leaks between plans."""
    cid, check, args, env, want, kw = case
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ops._rowtabs.clear()
    CHECKS[check](device, *args, want=want, **kw)


def ids(cases):
    return [c[0] for c in cases]
