"""Per-element parity checks of sf_conv_c_bwd (csrc/sf_cbwd.h: the block-final BatchNorm backward fused into both gradients of the
block's last 1x1x1 convolution), shared by tests/test_cbwd_hostsim.py and the -m gpu file tests/test_cbwd_gpu.py.

Method, notation, operand draws, poison and canaries of tests/conv_elem_checks.py; its bound functions are imported, none is new.

What is compared.  The kernel forms dy = (ACT)(k1 * g + k2 + k3 * yc), g = dz under the 1-bit mask, per row tile on chip and feeds
  d_in[m][ci] = sum_co dy[m][co] * wd[ci][co]     and     dw[co][ci] (+)= out_scale * sum_m dy[m][co] * act[m][ci]
from that tile.  The reference is torch float64 on the HOST REPLICA of the rounded dy: the same expression in float32.  The compiler
may contract either product with the following sum into one fused multiply-add (one rounding) or not, so the replica is formed in
all four evaluations (fused ones in fp64, where the product of an fp32 and an ACT number is exact; a double rounding needs a 2^-29
coincidence and is ignored, as in conv_elem_checks).  The reference uses the doubly fused one; da = the largest deviation of the
others after the rounding to ACT (zero for almost every element) enters the bounds through the linear maps: + da . |wd| for d_in,
+ |out_scale| da^T . |act| for dw.  coef comes from the library's own finalize (ops.bn_bwd_coef) and is read back.

Bounds (the functions of conv_elem_checks.check_dgrad with bn=, and check_wgrad):
  d_in   : stored,  |got - ref| <= 2 u16 |ref| + TINY + E32 (1 + u16),  E32 = Co u32 (|dy| . |wd|) + da . |wd|
  dw     : fp32,    E32 = L u32 (|out_scale| |dy|^T . |act| + |prior dw|) + |out_scale| da^T . |act|,
           L = rows of one workgroup (+ 3: the sum over its four waves at Co = 32) + slabs + 2
  part   : the sums of the kernel's OWN STORED d_in under the recomputed mask: 128 * u32 * sum|term| per partial row (128 positions).
The three-launch path (SF_CBWD=0: sf_bn_bwd_apply, sf_conv_wgrad, sf_conv_dgrad_bn) on the same inputs must satisfy the same bounds
with its own restated plans (conv_elem_checks.wgrad_variant / dgrad_variant); its materialised dy must be one of the four replicas
element by element, and dgamma / dbeta of the two paths are bit-identical (the same finalize launch on the same table).
"""
from ctypes import byref, c_int32

import torch

from slowfast_amd import ops
from slowfast_amd.lib import get_lib
from tests import conv_elem_checks as cc
from tests.conv_elem_checks import CANARY32, GUARD, _assert_fp32, _assert_stored, _bits_image, _cdiv, _cl_in, _f32, _Out, _rows, _tile_sums
from tests.kernel_checks import ACT
from tests.x3d_checks import U16, U32

DIMS = (2, 2, 5, 7)          # M = 140: no multiple of any tile height, three tiles at (64, 256), a short last tile, five workgroups of 32 rows
SHAPES = [(8, 32), (16, 64), (64, 256)]
# (pitched, fused inner-BatchNorm reduction, zero_first): every option both ways for every shape
OPTIONS = [(False, True, True), (True, False, False), (True, True, False), (False, False, True)]
CASES = [dict(id=f"ci{ci}_co{co}_{'pitch' if pd else 'dense'}_{'bn' if bn else 'nobn'}_{'zero' if zf else 'acc'}", Ci=ci, Co=co,
              pitched=pd, bn=bn, zero_first=zf) for ci, co in SHAPES for pd, bn, zf in OPTIONS]
CASES.append(dict(id="m24_below_one_tile", Ci=16, Co=64, dims=(1, 1, 4, 6), pitched=True, bn=True, zero_first=True))
CASES.append(dict(id="two_workgroups_walk_tiles", Ci=64, Co=256, pitched=False, bn=True, zero_first=False, wgs=2))
# the round-robin order of the thin weight-gradient kernel (Co <= 32, at least 16384 rows in the product) at 396 rows: its thresholds
# lowered by the test hooks of conv_elem_checks, two workgroups of two 128-row stages each, the last stage short
CASES.append(dict(id="thin_round_robin", Ci=8, Co=32, dims=(2, 2, 9, 11), pitched=True, bn=True, zero_first=True,
                  env=dict(cc.W2T, SF_WGRAD2T_BLOCKS="2")))
OUT_SCALE = 0.625            # non-unit, exact in fp32


TABLE_ROWS = 128             # positions per row of the inner BatchNorm's partial table (the data gradient's 128-row tiles)


def row_plan(geom, wgs):
    """sf_conv_c_bwd restated: (rows per workgroup, workgroups).  The rows are dealt as plan_wgrad deals them to its splits (the
    thin round-robin plan of plan_wgrad2 needs 16384 rows: none of these cases); SF_CBWD_WGS sets the workgroup count."""
    if wgs:
        rps = cc._roundup(_cdiv(geom.out_rows, wgs), 32)
        return rps, _cdiv(geom.out_rows, rps)
    w2 = cc.plan_wgrad2(geom)
    if w2 is not None and w2["thin"]:
        return w2["rows"], w2["splits"]                 # stages z, z + splits, ...: at most this many rows per workgroup
    assert w2 is None
    w = cc.plan_wgrad(geom)
    return w["rows"], w["splits"]


def _dy_replicas(dz, keep, yc, coef):
    """The four legal float32 evaluations of k1 * g + k2 + k3 * y, rounded to ACT (fp64 tensors)."""
    k1, k2, k3 = (coef[i].double().view(1, -1) for i in range(3))
    g = dz * keep
    a_fma = _f32(k1 * g + k2).double()
    a_mul = (_f32(_f32(k1 * g).double() + k2)).double()
    out = []
    for a in (a_fma, a_mul):
        out.append(_f32(a + k3 * yc).to(ACT).double())                      # second product fused
        out.append(_f32(a + _f32(k3 * yc).double()).to(ACT).double())       # rounded separately
    return out


def check_cbwd(device, monkeypatch, Ci, Co, dims=DIMS, pitched=False, bn=True, zero_first=True, wgs=None, seed=0, id=None, env=None):
    for key in ("SF_CBWD", "SF_CBWD_WGS") + cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    if wgs:
        monkeypatch.setenv("SF_CBWD_WGS", str(wgs))
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, v)
    N, T, H, W = dims
    shape = (N, Ci, T, H, W)
    geom = ops.ConvGeom(shape, Co, (1, 1, 1))
    M = geom.out_rows
    R = TABLE_ROWS
    rps, nwg = row_plan(geom, wgs)
    plan = ops.conv_c_bwd_plan(geom)
    assert plan is not None and plan[0] == R, f"planner: {plan}, restated tile rows {R}"
    ntiles = _cdiv(M, R)
    pad = 8 if pitched else 0
    gen = torch.Generator().manual_seed(seed + 11)
    w = torch.randn((Co, Ci, 1, 1, 1), generator=gen) / Ci ** 0.5
    w16 = w.to(ACT).double().view(Co, Ci)
    _, wd = ops.prep_weights(w.to(device), geom)
    act = torch.randn(shape, generator=gen).to(ACT).double()
    dz = torch.randn(geom.out_shape, generator=gen).to(ACT).double()
    yc = torch.randn(geom.out_shape, generator=gen).to(ACT).double()
    yb = torch.randn(shape, generator=gen).to(ACT).double()
    bits, keep = _bits_image(gen, M, Co)               # about half the bits set
    gamma, mean, rstd = torch.rand(Co, generator=gen) + 0.5, torch.randn(Co, generator=gen) * 0.1, torch.rand(Co, generator=gen) + 0.5
    sc, sh = torch.rand(Ci, generator=gen) + 0.5, torch.randn(Ci, generator=gen) * 0.3
    prior = torch.randn(w.shape, generator=gen) if not zero_first else torch.full(w.shape, 7.0)
    actc, dzc, ycc, ybc = (_cl_in(t, device, pad) for t in (act, dz, yc, yb))
    bitsd = bits.contiguous().to(device)
    gd, md, rd, scd, shd = (t.to(device) for t in (gamma, mean, rstd, sc, sh))
    lib = get_lib()

    def dw_buffer():
        flat = torch.full((2 * GUARD + w.numel(),), CANARY32, dtype=torch.int32, device=device).view(torch.float32)
        dw = flat[GUARD:GUARD + w.numel()].view(w.shape)
        dw.copy_(prior)
        return flat, dw

    def dw_intact(flat, name):
        b = flat.detach().cpu().view(torch.int32)
        assert bool((b[:GUARD] == CANARY32).all()) and bool((b[-GUARD:] == CANARY32).all()), f"{name}: wrote outside dw"

    # ---- the fused path: finalize (coef, dgamma, dbeta), then ONE launch; the part table sits between guards as well
    dgam, dbet = torch.empty(Co, device=device), torch.empty(Co, device=device)
    coef = ops.bn_bwd_coef(dzc, ycc, gd, md, rd, dgam, dbet, zmask=bitsd)
    ws = ops._workspace(device, plan[1])

    def fused():
        out = _Out(shape, device, pad)
        flat, dw = dw_buffer()
        pflat = torch.full((2 * GUARD + ntiles * 2 * Ci,), CANARY32, dtype=torch.int32, device=device).view(torch.float32)
        part = pflat[GUARD:GUARD + ntiles * 2 * Ci].view(ntiles, 2, Ci)
        nrows = c_int32(-1)
        lib.call("sf_conv_c_bwd", byref(geom.desc(ops.cl_ld(actc), Co)), dzc.data_ptr(), ops.cl_ld(dzc), bitsd.data_ptr(),
                 ycc.data_ptr(), ops.cl_ld(ycc), coef.data_ptr(), actc.data_ptr(), wd.data_ptr(),
                 scd.data_ptr() if bn else None, shd.data_ptr() if bn else None, ybc.data_ptr() if bn else None,
                 ops.cl_ld(ybc) if bn else 0, part.data_ptr() if bn else None, ntiles if bn else 0, byref(nrows),
                 out.view.data_ptr(), ops.cl_ld(out.view), dw.data_ptr(), OUT_SCALE, int(zero_first), ws.data_ptr(), ws.numel(),
                 ops._stream(dzc))
        assert nrows.value == (ntiles if bn else 0), "rows of the part table"
        name = f"conv_c_bwd[{id}]"
        out.assert_canaries(name)
        dw_intact(flat, name)
        pb = pflat.detach().cpu().view(torch.int32)
        assert bool((pb[:GUARD] == CANARY32).all()) and bool((pb[-GUARD:] == CANARY32).all()), f"{name}: wrote outside the part table"
        if not bn:
            assert bool((pb == CANARY32).all()), f"{name}: wrote a part table nobody asked for"
        return out, dw.detach().cpu().double(), part.detach().cpu().double()

    out, dw_got, part_got = fused()
    coef_h = coef.detach().cpu()
    assert bool(torch.isfinite(coef_h).all())

    # ---- references
    dzr, ycr, actr, ybr = _rows(dz), _rows(yc), _rows(act), _rows(yb)
    reps = _dy_replicas(dzr, keep.double(), ycr, coef_h)
    dy16 = reps[0]
    da = torch.stack([(r - dy16).abs() for r in reps[1:]]).max(0).values
    wabs = w16.abs()
    d_ref, d_E = dy16 @ w16, Co * U32 * (dy16.abs() @ wabs) + da @ wabs
    sc32 = float(torch.tensor(OUT_SCALE, dtype=torch.float32))
    pr = prior.double().view(Co, Ci)
    w_ref = sc32 * (dy16.t() @ actr) + (0.0 if zero_first else pr)
    w_A = abs(sc32) * (dy16.abs().t() @ actr.abs()) + (0.0 if zero_first else pr.abs())
    w_da = abs(sc32) * (da.t() @ actr.abs())
    mask = _f32(ybr * sc.double() + sh.double()) > 0
    assert torch.equal(mask, (_f32(ybr) * sc + sh) > 0), "the draw leaves the recomputed mask ambiguous"

    def compare(name, got_rows, dw_rows, part, L, bm):
        _assert_stored(name + " d_in", got_rows, d_ref, d_E * (1 + U16))
        _assert_fp32(f"{name} dw L = {L}", dw_rows.view(Co, Ci), w_ref, L * U32 * w_A + w_da)
        if bn:
            tg, tgy = got_rows * mask, got_rows * mask * ybr
            assert part.shape[0] == _cdiv(M, bm), "rows of the part table"
            _assert_fp32(name + " part sum g", part[:, 0], _tile_sums(tg, bm), bm * U32 * _tile_sums(tg.abs(), bm))
            _assert_fp32(name + " part sum g y", part[:, 1], _tile_sums(tgy, bm), bm * U32 * _tile_sums(tgy.abs(), bm))

    L = rps + 3 + nwg + 2          # one workgroup's rows (+ the sum over its four waves at Co = 32) + the slabs + out_scale, accumulate
    compare(f"conv_c_bwd[{id}]", out.rows(), dw_got, part_got, L, R)

    # ---- determinism: a second launch is bit-identical
    out2, dw2, part2 = fused()
    assert torch.equal(out.rows(), out2.rows()) and torch.equal(dw_got, dw2), "two launches differ"
    assert not bn or torch.equal(part_got, part2), "two launches differ in the part table"

    # ---- the wrapper the engine calls gives the same bits
    flat3, dw3 = dw_buffer()
    d3, p3 = ops.conv_c_bwd(dzc, bitsd, ycc, coef, actc, wd, geom, dw3, bn=(ybc, scd, shd) if bn else None, out_scale=OUT_SCALE,
                            zero_first=zero_first)
    assert torch.equal(_rows(d3.detach().cpu().double()), out.rows()) and torch.equal(dw3.detach().cpu().double(), dw_got)
    assert (p3 is None) == (not bn) and (p3 is None or torch.equal(p3.detach().cpu().double(), part_got))
    dw_intact(flat3, "ops.conv_c_bwd")

    # ---- the three-launch path on the same inputs
    monkeypatch.setenv("SF_CBWD", "0")
    assert ops.conv_c_bwd_plan(geom) is None, "SF_CBWD=0 keeps the three launches"
    dgam0, dbet0 = torch.empty(Co, device=device), torch.empty(Co, device=device)
    dy_old = ops.bn_bwd(dzc, ycc, gd, md, rd, dgam0, dbet0, zmask=bitsd)
    assert torch.equal(dgam0, dgam) and torch.equal(dbet0, dbet), "dgamma / dbeta differ between the two paths"
    dyo = _rows(dy_old.detach().cpu().double())
    assert bool(((dyo - dy16).abs() <= da).all()), "the materialised dy is none of the restated evaluations"
    flat0, dw0 = dw_buffer()
    ops._rowtabs.clear()
    ops.conv_wgrad(actc, dy_old, geom, dw0, out_scale=OUT_SCALE, zero_first=zero_first)
    dw_intact(flat0, "sf_conv_wgrad")
    out0 = _Out(shape, device, pad)
    if bn:
        _, part0 = ops.conv_dgrad(dy_old, wd, geom, out=out0.view, bn=(ybc, scd, shd))
    else:
        ops.conv_dgrad(dy_old, wd, geom, out=out0.view)
        part0 = None
    out0.assert_canaries("sf_conv_dgrad_bn")
    variant, bn_rows = cc.dgrad_variant(geom, ops.cl_ld(dy_old), bn=bn)
    _, L0, _, _ = cc.wgrad_variant(geom)
    bm0 = 256 if variant.startswith("igemm2") else 128
    assert not bn or (part0 is not None and part0.shape[0] == bn_rows)
    # the same rounded dy through the same chain of 32-deep MFMA steps: d_in of the two paths is the same bit pattern
    ndiff = int((out0.rows() != out.rows()).sum())
    print(f"d_in elements that differ between the two paths: {ndiff} of {out.rows().numel()}")
    assert ndiff == 0, "d_in differs between the fused launch and the three launches: dy is not rounded as sf_bn_bwd_apply stores it"
    # the rows are dealt to the workgroups as sf_conv_wgrad deals them to its splits, 32-row step by 32-row step, and the table keeps
    # the data gradient's 128-row tiles and per-thread order: dw and the table are the same bit patterns too (not at Co = 32 below
    # 16384 rows, where the three-launch path takes another weight-gradient kernel than the one whose order is kept, nor with the
    # workgroup count forced)
    if (Co > 32 or env) and not wgs:
        assert torch.equal(dw0.detach().cpu().double(), dw_got), "dw differs between the fused launch and the three launches"
    if bn:
        assert torch.equal(part0.detach().cpu().double(), part_got), "the inner BatchNorm's table differs between the two paths"
    compare(f"three launches[{id}]", out0.rows(), dw0.detach().cpu().double(), None if part0 is None else part0.detach().cpu().double(),
            L0, bm0)
    monkeypatch.delenv("SF_CBWD")


def check_rejects(device, monkeypatch):
    """The planner: accepts the production shapes whatever the row count, rejects what the kernel was not written for."""
    for key in ("SF_CBWD", "SF_CBWD_WGS"):
        monkeypatch.delenv(key, raising=False)

    def plan(shape, Co, k=(1, 1, 1), s=(1, 1, 1), p=(0, 0, 0), **kw):
        return ops.conv_c_bwd_plan(ops.ConvGeom(shape, Co, k, s, p), **kw)

    for ci, co in SHAPES + [(32, 128), (24, 96)]:
        for dims in ((1, 1, 1, 1), (2, 2, 5, 7)):
            got = plan((dims[0], ci) + dims[1:], co)
            assert got is not None and got[0] == TABLE_ROWS and got[1] > 0, (ci, co, dims, got)
    assert plan((2, 72, 2, 5, 7), 256) is None, "Ci = 72"
    assert plan((2, 64, 2, 5, 7), 288) is None, "Co = 288"
    assert plan((2, 64, 2, 6, 8), 256, s=(1, 2, 2)) is None, "stride 2"
    assert plan((2, 64, 2, 5, 7), 256, k=(1, 3, 3), p=(0, 1, 1)) is None, "a 1x3x3 kernel"
    assert plan((2, 64, 2, 5, 7), 256, in_affine=True) is None, "an input affine"
    assert plan((2, 64, 2, 5, 7), 256, mask_bits=False) is None, "a full-width mask"
    assert plan((2, 64, 2, 5, 7), 40) is None, "Co % 32"
    # a rejected geometry is an error of the entry point, not a silent other path
    geom = ops.ConvGeom((2, 72, 2, 5, 7), 256, (1, 1, 1))
    z = torch.zeros(8, dtype=torch.float32, device=device)
    cc._expect_error(lambda: get_lib().call(
        "sf_conv_c_bwd", byref(geom.desc(72, 256)), z.data_ptr(), 256, z.data_ptr(), z.data_ptr(), 256, z.data_ptr(), z.data_ptr(),
        z.data_ptr(), None, None, None, 0, None, 0, byref(c_int32(0)), z.data_ptr(), 72, z.data_ptr(), 1.0, 1, z.data_ptr(), 32, None),
        "sf_conv_c_bwd_plan == 0")


def ids(cases):
    return [c["id"] for c in cases]


def run_case(device, monkeypatch, case):
    check_cbwd(device, monkeypatch, **case)
