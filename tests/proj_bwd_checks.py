"""Per-element parity checks of sf_conv_proj_bwd (csrc/sf_cbwd.h: the BatchNorm backward of a projection shortcut, branch1 + branch1_bn,
fused into both gradients of its 1x1x1 convolution at stride 1 or (1,2,2)), shared by tests/test_proj_bwd_hostsim.py and the -m gpu
file tests/test_proj_bwd_gpu.py.

Method, references and bounds of tests/cbwd_checks.py (its functions and those of tests/conv_elem_checks.py are imported, none is new):
the reference is torch float64 on the host replica of the rounded dy = (ACT)(k1 * g + k2 + k3 * y1), formed in all four legal float32
evaluations; da = the largest deviation between them enters the bounds through the linear maps.
  d_in   : stored,  |got - ref| <= 2 u16 |ref| + TINY + E32 (1 + u16),  E32 = Co u32 (|dy| . |wd|) + da . |wd|   at the sampled input
           rows; the rows a stride of 2 never samples have ref = 0 and E32 = 0
  dw     : fp32,    E32 = L u32 (|out_scale| |dy|^T . |x| + |prior dw|) + |out_scale| da^T . |x|  (x at the sampled rows),
           L = rows of one workgroup (+ 3: the sum over its four waves at Co = 32) + slabs + 2
Bit equality with the three launches the call replaces (SF_CBWD=0: sf_bn_bwd_apply, sf_conv_wgrad, sf_conv_dgrad) on the same inputs:
d_in as int16 images (a -0 in a zero row would show, and so would a row nobody wrote: the buffer is poisoned), dgamma / dbeta, and dw
wherever the three-launch path takes the weight-gradient kernel whose order is kept (cbwd_checks: not at Co = 32 below 16384 rows
without the thin hooks, nor with the workgroup count forced).
"""
from ctypes import byref

import torch

from slowfast_amd import ops
from slowfast_amd.lib import get_lib, set_call_observer
from tests import cbwd_checks as cb
from tests import conv_elem_checks as cc
from tests.conv_elem_checks import CANARY32, GUARD, _assert_fp32, _assert_stored, _bits_image, _cl_in, _f32, _Out, _rows
from tests.kernel_checks import ACT, cl_to_host, host_to_cl
from tests.x3d_checks import U16, U32

# the five projections of a SlowFast-8x8-R50 step that take the path: (Ci, Co, spatial stride)
PRODUCTION = [(80, 256, 1), (8, 32, 1), (32, 64, 2), (64, 128, 2), (128, 256, 2)]
# INPUT dims (N, T, H, W).  Stride 1: 140 rows, three tiles at Co 256, a short last tile.  Stride 2: 48 output rows (below one
# tile), and 360 output rows (runs cross image-row, frame and sample boundaries, the last tile is short)
DIMS = {1: [(2, 2, 5, 7)], 2: [(2, 2, 6, 8), (2, 3, 12, 20)]}
# (pitched, zero_first, forced workgroups): every option both ways for every shape; SF_CBWD_WGS=2 makes a workgroup walk several
# tiles and (140 and 360 rows) a 128-row table tile straddle two runs
OPTIONS = [(False, True, None), (True, False, None), (True, True, 2)]
CASES = [dict(id=f"ci{ci}_co{co}_s{st}_{'x'.join(map(str, dims))}_{'pitch' if pd else 'dense'}_{'zero' if zf else 'acc'}"
                 + (f"_wgs{wgs}" if wgs else ""), Ci=ci, Co=co, stride=st, dims=dims, pitched=pd, zero_first=zf, wgs=wgs)
         for ci, co, st in PRODUCTION for dims in DIMS[st] for pd, zf, wgs in OPTIONS]
# the round-robin order of the thin weight-gradient kernel for 8 -> 32, with the hooks of cbwd_checks' case
CASES.append(dict(id="thin_round_robin", Ci=8, Co=32, stride=1, dims=(2, 2, 9, 11), pitched=True, zero_first=True,
                  env=dict(cc.W2T, SF_WGRAD2T_BLOCKS="2")))
# stride 2 against the residue-class launches of the strided data gradient (the production path, taken from 4096 rows on: the hooks
# of conv_elem_checks lower its thresholds)
CASES += [dict(id=f"ci{ci}_co{co}_s2_classes", Ci=ci, Co=co, stride=2, dims=(2, 3, 12, 20), pitched=False, zero_first=True, env=dict(cc.V2))
          for ci, co, st in PRODUCTION if st == 2]
OUT_SCALE = cb.OUT_SCALE


def _geom(Ci, Co, stride, dims):
    N, T, H, W = dims
    return ops.ConvGeom((N, Ci, T, H, W), Co, (1, 1, 1), (1, stride, stride), (0, 0, 0))


def _image(out):
    """the logical [M, C] region of an _Out buffer as raw 16-bit patterns"""
    return out.flat.detach().cpu().view(torch.int16)[GUARD:GUARD + out.M * out.ld].view(out.M, out.ld)[:, :out.C]


def check_proj_bwd(device, monkeypatch, Ci, Co, stride, dims, pitched=False, zero_first=True, wgs=None, seed=0, id=None, env=None):
    for key in ("SF_CBWD", "SF_CBWD_WGS") + cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    if wgs:
        monkeypatch.setenv("SF_CBWD_WGS", str(wgs))
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, v)
    geom = _geom(Ci, Co, stride, dims)
    shape = geom.in_shape
    rps, nwg = cb.row_plan(geom, wgs)
    ws_bytes = ops.conv_proj_bwd_plan(geom)
    assert ws_bytes is not None and ws_bytes > 0, "the planner rejects a production shape"
    pad = 8 if pitched else 0
    gen = torch.Generator().manual_seed(seed + 23)
    w = torch.randn((Co, Ci, 1, 1, 1), generator=gen) / Ci ** 0.5
    w16 = w.to(ACT).double().view(Co, Ci)
    _, wd = ops.prep_weights(w.to(device), geom)
    x = torch.randn(shape, generator=gen).to(ACT).double()
    dz = torch.randn(geom.out_shape, generator=gen).to(ACT).double()
    y1 = torch.randn(geom.out_shape, generator=gen).to(ACT).double()
    Mo = geom.out_rows
    bits, keep = _bits_image(gen, Mo, Co)
    gamma, mean, rstd = torch.rand(Co, generator=gen) + 0.5, torch.randn(Co, generator=gen) * 0.1, torch.rand(Co, generator=gen) + 0.5
    prior = torch.randn(w.shape, generator=gen) if not zero_first else torch.full(w.shape, 7.0)
    xc, dzc, y1c = (_cl_in(t, device, pad) for t in (x, dz, y1))
    bitsd = bits.contiguous().to(device)
    gd, md, rd = (t.to(device) for t in (gamma, mean, rstd))
    lib = get_lib()

    def dw_buffer():
        flat = torch.full((2 * GUARD + w.numel(),), CANARY32, dtype=torch.int32, device=device).view(torch.float32)
        dw = flat[GUARD:GUARD + w.numel()].view(w.shape)
        dw.copy_(prior)
        return flat, dw

    def dw_intact(flat, name):
        b = flat.detach().cpu().view(torch.int32)
        assert bool((b[:GUARD] == CANARY32).all()) and bool((b[-GUARD:] == CANARY32).all()), f"{name}: wrote outside dw"

    dgam, dbet = torch.empty(Co, device=device), torch.empty(Co, device=device)
    coef = ops.bn_bwd_coef(dzc, y1c, gd, md, rd, dgam, dbet, zmask=bitsd)
    ws = ops._workspace(device, ws_bytes)
    name = f"conv_proj_bwd[{id}]"

    def fused():
        out = _Out(shape, device, pad)
        flat, dw = dw_buffer()
        lib.call("sf_conv_proj_bwd", byref(geom.desc(ops.cl_ld(xc), Co)), dzc.data_ptr(), ops.cl_ld(dzc), bitsd.data_ptr(),
                 y1c.data_ptr(), ops.cl_ld(y1c), coef.data_ptr(), xc.data_ptr(), wd.data_ptr(), out.view.data_ptr(),
                 ops.cl_ld(out.view), dw.data_ptr(), OUT_SCALE, int(zero_first), ws.data_ptr(), ws_bytes, ops._stream(dzc))
        out.assert_canaries(name)
        dw_intact(flat, name)
        return out, dw.detach().cpu().double()

    out, dw_got = fused()
    coef_h = coef.detach().cpu()
    assert bool(torch.isfinite(coef_h).all())

    # ---- references: the sampled input rows carry the product, every other input row is zero
    xs = _rows(x[:, :, :, ::stride, ::stride])
    reps = cb._dy_replicas(_rows(dz), keep.double(), _rows(y1), coef_h)
    dy16 = reps[0]
    da = torch.stack([(r - dy16).abs() for r in reps[1:]]).max(0).values
    wabs = w16.abs()
    N, T, H, W = dims
    Ho, Wo = H // stride, W // stride

    def scatter(t):
        full = torch.zeros((N, T, H, W, Ci), dtype=torch.float64)
        full[:, :, ::stride, ::stride] = t.view(N, T, Ho, Wo, Ci)
        return full.view(-1, Ci)

    d_ref, d_E = scatter(dy16 @ w16), scatter(Co * U32 * (dy16.abs() @ wabs) + da @ wabs)
    sc32 = float(torch.tensor(OUT_SCALE, dtype=torch.float32))
    pr = prior.double().view(Co, Ci)
    w_ref = sc32 * (dy16.t() @ xs) + (0.0 if zero_first else pr)
    w_A = abs(sc32) * (dy16.abs().t() @ xs.abs()) + (0.0 if zero_first else pr.abs())
    w_da = abs(sc32) * (da.t() @ xs.abs())

    def compare(who, got_rows, dw_rows, L):
        _assert_stored(who + " d_in", got_rows, d_ref, d_E * (1 + U16))
        _assert_fp32(f"{who} dw L = {L}", dw_rows.view(Co, Ci), w_ref, L * U32 * w_A + w_da)

    compare(name, out.rows(), dw_got, rps + 3 + nwg + 2)

    # ---- determinism, and the wrapper the engine calls
    out2, dw2 = fused()
    assert torch.equal(_image(out), _image(out2)) and torch.equal(dw_got, dw2), "two launches differ"
    flat3, dw3 = dw_buffer()
    d3 = ops.conv_proj_bwd(dzc, bitsd, y1c, coef, xc, wd, geom, dw3, out_scale=OUT_SCALE, zero_first=zero_first)
    assert torch.equal(_rows(d3.detach().cpu()).view(torch.int16), _image(out)) and torch.equal(dw3.detach().cpu().double(), dw_got)
    dw_intact(flat3, "ops.conv_proj_bwd")

    # ---- the three launches on the same inputs
    monkeypatch.setenv("SF_CBWD", "0")
    assert ops.conv_proj_bwd_plan(geom) is None, "SF_CBWD=0 keeps the three launches"
    dgam0, dbet0 = torch.empty(Co, device=device), torch.empty(Co, device=device)
    dy_old = ops.bn_bwd(dzc, y1c, gd, md, rd, dgam0, dbet0, zmask=bitsd)
    assert torch.equal(dgam0.view(torch.int32), dgam.view(torch.int32)) and torch.equal(dbet0.view(torch.int32), dbet.view(torch.int32)), \
        "dgamma / dbeta differ between the two paths"
    dyo = _rows(dy_old.detach().cpu().double())
    assert bool(((dyo - dy16).abs() <= da).all()), "the materialised dy is none of the restated evaluations"
    flat0, dw0 = dw_buffer()
    ops._rowtabs.clear()
    ops.conv_wgrad(xc, dy_old, geom, dw0, out_scale=OUT_SCALE, zero_first=zero_first)
    dw_intact(flat0, "sf_conv_wgrad")
    out0 = _Out(shape, device, pad)
    ops.conv_dgrad(dy_old, wd, geom, out=out0.view)
    out0.assert_canaries("sf_conv_dgrad")
    if env and "SF_IGEMM2_MINROWS" in env:
        assert cc.dgrad_variant(geom, ops.cl_ld(dy_old))[0].startswith("igemm2"), "the hooks did not select the residue-class launches"
    _, L0, _, _ = cc.wgrad_variant(geom)
    ndiff = int((_image(out0) != _image(out)).sum())
    print(f"d_in 16-bit patterns that differ between the two paths: {ndiff} of {_image(out).numel()}")
    assert ndiff == 0, "d_in differs between the fused launch and the three launches"
    if (Co > 32 or env) and not wgs:
        assert torch.equal(dw0.detach().cpu().view(torch.int32), dw_got.float().view(torch.int32)), \
            "dw differs between the fused launch and the three launches"
    compare(f"three launches[{id}]", out0.rows(), dw0.detach().cpu().double(), L0)
    monkeypatch.delenv("SF_CBWD")


def check_planner(device, monkeypatch):
    """Accepts the five production pairs whatever the row count; rejects what the kernel was not written for; sf_conv_c_bwd_plan is
    what it was."""
    for key in ("SF_CBWD", "SF_CBWD_WGS"):
        monkeypatch.delenv(key, raising=False)

    def plan(shape, Co, k=(1, 1, 1), s=(1, 1, 1), p=(0, 0, 0), **kw):
        return ops.conv_proj_bwd_plan(ops.ConvGeom(shape, Co, k, s, p), **kw)

    for ci, co, st in PRODUCTION:
        for dims in ((1, 1, 2, 2), (2, 2, 6, 8)):
            got = plan((dims[0], ci) + dims[1:], co, s=(1, st, st))
            assert got is not None and got > 0, (ci, co, st, dims, got)
    assert plan((2, 64, 2, 5, 8), 128, s=(1, 2, 2)) is None, "odd Hi"
    assert plan((2, 64, 2, 6, 7), 128, s=(1, 2, 2)) is None, "odd Wi"
    assert plan((2, 64, 2, 6, 8), 128, s=(2, 1, 1)) is None, "stride (2,1,1)"
    assert plan((2, 136, 2, 5, 7), 256) is None, "Ci = 136"
    assert plan((2, 64, 2, 5, 7), 288) is None, "Co = 288"
    assert plan((2, 64, 2, 5, 7), 256, k=(1, 3, 3), p=(0, 1, 1)) is None, "a 1x3x3 kernel"
    assert plan((2, 64, 2, 5, 7), 256, in_affine=True) is None, "an input affine"
    assert plan((2, 64, 2, 5, 7), 256, mask_bits=False) is None, "a full-width mask"
    monkeypatch.setenv("SF_CBWD", "0")
    for ci, co, st in PRODUCTION:
        assert plan((2, ci, 2, 6, 8), co, s=(1, st, st)) is None, "SF_CBWD=0 switches the family off"
    monkeypatch.delenv("SF_CBWD")
    # the block-final planner keeps its own domain
    assert ops.conv_c_bwd_plan(ops.ConvGeom((2, 72, 2, 5, 7), 256, (1, 1, 1))) is None, "sf_conv_c_bwd_plan: Ci = 72"
    assert ops.conv_c_bwd_plan(ops.ConvGeom((2, 64, 2, 6, 8), 256, (1, 1, 1), (1, 2, 2))) is None, "sf_conv_c_bwd_plan: stride 2"
    # a rejected geometry is an error of the entry point, not a silent other path
    geom = ops.ConvGeom((2, 136, 2, 5, 7), 256, (1, 1, 1))
    z = torch.zeros(8, dtype=torch.float32, device=device)
    cc._expect_error(lambda: get_lib().call(
        "sf_conv_proj_bwd", byref(geom.desc(136, 256)), z.data_ptr(), 256, z.data_ptr(), z.data_ptr(), 256, z.data_ptr(), z.data_ptr(),
        z.data_ptr(), z.data_ptr(), 136, z.data_ptr(), 1.0, 1, z.data_ptr(), 32, None), "sf_conv_proj_bwd_plan == 0")


# ------------------------------------------------------------------------------------------------
# block level: the first block of a stage (projection shortcut), default against SF_CBWD=0
# (dim_out 64: at 32 output channels and so few rows the three-launch path takes another weight-gradient kernel than the one whose
# order the fused launch keeps, see the module docstring)
BLOCKS = [dict(id="stride1", dim_in=32, dim_out=64, stride=1, inner=16, shape=(2, 32, 2, 6, 8)),
          dict(id="stride2", dim_in=32, dim_out=64, stride=2, inner=16, shape=(2, 32, 2, 6, 8))]


def _run_block(device, dim_in, dim_out, stride, inner, shape, seed):
    from oracle import video_ref
    from slowfast_amd.resblocks import BottleneckTransform, ResBlock
    torch.manual_seed(seed)
    blk = ResBlock(dim_in, dim_out, 3, stride, BottleneckTransform, inner)
    blk.load_state_dict(video_ref.randomize_state({k: tuple(v.shape) for k, v in blk.state_dict().items()}, seed))
    blk = blk.to(device).train()
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(shape, generator=gen).to(ACT).float()
    xc = host_to_cl(x, device).requires_grad_(True)
    out = blk(xc)
    dout = torch.randn(tuple(out.shape), generator=gen).to(ACT).float()
    log = []

    def observer(name, thunk, work):
        log.append(name)
        return thunk()

    set_call_observer(observer)
    try:
        out.backward(host_to_cl(dout, device))
    finally:
        set_call_observer(None)
    grads = {k: p.grad.detach().cpu().clone() for k, p in blk.named_parameters()}
    return log, cl_to_host(xc.grad).to(ACT), grads


def check_block(device, monkeypatch, dim_in, dim_out, stride, inner, shape, seed=7, id=None):
    for key in ("SF_CBWD", "SF_CBWD_WGS") + cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    log, dx, grads = _run_block(device, dim_in, dim_out, stride, inner, shape, seed)
    monkeypatch.setenv("SF_CBWD", "0")
    log0, dx0, grads0 = _run_block(device, dim_in, dim_out, stride, inner, shape, seed)
    monkeypatch.delenv("SF_CBWD")
    # three BatchNorms of the transform + branch1_bn: the fused paths leave the apply pass to a_bn and b_bn only
    assert log.count("sf_conv_proj_bwd") == 1 and log.count("sf_conv_c_bwd") == 1, log
    assert log.count("sf_bn_bwd_apply") == 2, "branch1_bn still runs its apply pass: %s" % log
    assert log0.count("sf_conv_proj_bwd") == 0 and log0.count("sf_conv_c_bwd") == 0 and log0.count("sf_bn_bwd_apply") == 4, log0
    assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16)), "dx differs between the default path and SF_CBWD=0"
    assert set(grads) == set(grads0) and "branch1.weight" in grads and "branch1_bn.weight" in grads
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), grads0[k].view(torch.int32)), f"{k}.grad differs between the default path and SF_CBWD=0"


def ids(cases):
    return [c["id"] for c in cases]


def run_case(device, monkeypatch, case):
    check_proj_bwd(device, monkeypatch, **case)


def run_block(device, monkeypatch, case):
    check_block(device, monkeypatch, **case)
