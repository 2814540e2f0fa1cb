"""Checks of the grouped (1,3,3) convolution on block-diagonal bundles (csrc/sf_gconv.h, the BUNDLED form of sf_igemm2_kernel, the
sf_gconv_* launchers of sf_api.hip, ops.gconv_*, engine.GroupedConvUnit), shared by tests/test_gconv_hostsim.py and the -m gpu
file tests/test_gconv_gpu.py.

Kernel level: the method and notation of tests/conv_elem_checks.py (its helpers are imported, not copied).  The reference is torch
float64 ``F.conv3d(..., groups=G)`` and its autograd gradients on the CPU, evaluated on exactly the operands the MFMAs see:
activations drawn in ACT, weights rounded to ACT as sf_gconv_prep_kernel rounds them ((f16)v == torch's .to(ACT)).  Every
comparison is PER ELEMENT, no element is excluded, and each prints max err / bound.  u16 = lib.act_eps(), u32 = 2^-24, TINY = the
smallest subnormal of the storage type.

Bounds, read off the kernels (nothing is fitted to an observed error):
  forward / data gradient: one fp32 accumulator of sf_igemm2_kernel<.., BUNDLED> chains K = 9 taps x B products, B = max(32, Cg) the
      bundle width (the off-diagonal zeros of the packed operand multiply finite numbers and add exact zeros; they are counted as
      chain terms all the same, as conv_elem_checks counts padded channels), + 1 for the bias (acc * alpha + b, alpha = 1 exact):
      L = 9 B (+ 1), E32 = L u32 A with A the same grouped convolution of absolute values (+ |bias|) in fp64;
      stored: |got - ref| <= 2 u16 |ref| + TINY + E32 (1 + u16) (``_assert_stored``).  ReLU (act_mode 3) is 1-Lipschitz and commutes
      with the rounding: same bound.
  statistics (i2_epilogue): sums of the fp32 ACCUMULATORS per 128 positions -> the reference is the UNROUNDED fp64 convolution;
      a sum of n fp32 terms in any order is within (n - 1) u32 sum|term| of the exact sum of the same terms, D = 128:
      |s - ref| <= sum E32 + D u32 sum|ref|,  |q - ref| <= sum (2 |ref| E32 + E32^2) + (D + 1) u32 sum ref^2.
  weight gradient: the BUNDLED form of the dense weight-gradient kernels (bundle = blockIdx.y) leaves `slabs` partial tile sets of
      every bundle's B x 9B product; sf_gconv_wgrad_reduce_kernel sums the slabs of the diagonal blocks (four interleaved chains,
      then a tree: any order), multiplies by out_scale and adds the prior dw.  L = rows chained by one workgroup + slabs + 2, from
      plan_gconv_wgrad restated here (``wgrad_plan``, cross-checked against sf_gconv_wgrad_workspace);
      E32 = L u32 (|out_scale| A + |prior dw|) (``_assert_fp32``).
  packed operands: compared bit for bit with a host restatement -- every off-diagonal zero (+0) and, for the data-gradient
      operand, the transposition within each block and the tap mirror.

Poison and canaries as in conv_elem_checks: pitched inputs are channel-slice views of NaN-filled wider buffers, outputs are views
into CANARY-filled buffers with guards; dw sits between two guard regions that must stay bit-identical.

Block level: ResBlock + BottleneckTransform(num_groups=8, dim_inner=64) through engine.ResBlockFn against the same block in torch
fp32 on the CPU (``_ref_block``: nn.functional conv3d(groups=8) + batch_norm + ReLU from the same parameters), with the method and
the tolerance of tests/block_checks.py for its bottleneck cases: the reference's backward runs under the ReLU masks the engine
used, every compared quantity within block_checks.TOL relative L2 (``block_checks._compare``), flipped elements bounded by
block_checks.MAX_FLIP_FRACTION.

Model level: see ``check_model`` -- the grouped model equals the NUM_GROUPS 1 / WIDTH_PER_GROUP G*w model whose b weights are the
block-diagonal expansion, and dw_grouped is the diagonal blocks of dw_dense, so the existing oracle serves unchanged.
"""
import torch
import torch.nn.functional as F

from slowfast_amd import ops
from tests import conv_elem_checks as cc
from tests.conv_elem_checks import (CANARY32, GUARD, TINY, U16, U32, _Out, _assert_fp32, _assert_stored, _cdiv, _cl_in, _expect_error,
                                    _rows, _tile_sums)
from tests.kernel_checks import ACT

WORST = {}          # check name -> largest max err / bound seen in this process
BASE = (2, 2, 9, 11)            # N, T, H, W: odd extents, a border on every side, M = 396 = one full and one ragged 256-row tile
# (C, Cg, spatial stride, dilation): two bundles of 32 at every Cg < 64, two bundles of 64, four bundles, stride 2, dilation 2
KERNEL_CASES = [(64, 4, 1, 1), (64, 8, 1, 1), (64, 16, 1, 1), (64, 32, 1, 1), (128, 64, 1, 1), (128, 4, 1, 1), (64, 8, 2, 1),
                (64, 16, 1, 2)]


def case_id(c):
    return "C%d_Cg%d_s%d_d%d" % c


def _note(name, got, ref, bound):
    r = float(((got - ref).abs() / bound.clamp(min=1e-300)).max()) if ref.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), r)


def _geom(C, Cg, s, d, shape=BASE):
    N, T, H, W = shape
    return ops.GroupedConvGeom((N, C, T, H, W), C // Cg, (1, 3, 3), (1, s, s), (0, d, d), (1, d, d))


def _draw(seed, geom):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(geom.in_shape, generator=g).to(ACT).double()
    w = torch.randn((geom.Co, geom.Cg) + geom.k, generator=g) / (geom.Cg * geom.taps) ** 0.5
    dy = torch.randn(geom.out_shape, generator=g).to(ACT).double()
    return g, x, w, dy


def _conv64(x, w, geom):
    return F.conv3d(x, w, None, geom.s, geom.p, geom.d, geom.groups)


def _dgrad64(dy, w, geom):
    x0 = torch.zeros(geom.in_shape, dtype=torch.float64, requires_grad=True)
    _conv64(x0, w, geom).backward(dy)
    return x0.grad


def _wgrad64(x, dy, wshape, geom):
    w0 = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    _conv64(x, w0, geom).backward(dy)
    return w0.grad


# ------------------------------------------------------------------------------------------------
def pack_host(w, geom):
    """sf_gconv_prep_kernel restated: (wf, wd), each [C][9 * B] in ACT."""
    C, Cg, B, taps = geom.Co, geom.Cg, geom.B, geom.taps
    w16 = w.to(ACT).reshape(C, Cg, taps)
    dense = torch.zeros((C, C, taps), dtype=ACT)                  # the block-diagonal weight, [co][ci][tap]
    for g in range(C // Cg):
        dense[g * Cg:(g + 1) * Cg, g * Cg:(g + 1) * Cg] = w16[g * Cg:(g + 1) * Cg]
    wf = torch.zeros((C, taps * B), dtype=ACT)
    wd = torch.zeros((C, taps * B), dtype=ACT)
    for b in range(C // B):
        blk = dense[b * B:(b + 1) * B, b * B:(b + 1) * B]         # [co local][ci local][tap]
        wf[b * B:(b + 1) * B] = blk.permute(0, 2, 1).reshape(B, taps * B)                     # column tap * B + ci
        wd[b * B:(b + 1) * B] = blk.flip(2).permute(1, 2, 0).reshape(B, taps * B)             # row ci, column (8 - tap) * B + co
    return wf, wd


def check_prep(device, C, Cg, seed=0):
    geom = _geom(C, Cg, 1, 1)
    _, _, w, _ = _draw(seed, geom)
    wf, wd = ops.gconv_prep_weights(w.to(device), geom)
    hf, hd = pack_host(w, geom)
    assert tuple(wf.shape) == tuple(hf.shape) == (C, 9 * max(32, Cg))
    assert torch.equal(wf.cpu().view(torch.int16), hf.view(torch.int16)), "forward operand differs from the host restatement"
    assert torch.equal(wd.cpu().view(torch.int16), hd.view(torch.int16)), "data-gradient operand differs from the host restatement"
    nz = C * Cg * 9
    assert int((hf != 0).sum()) == nz == int((hd != 0).sum()), "the draw holds no zero weight: every zero is an off-diagonal one"
    wf2, none = ops.gconv_prep_weights(w.to(device), geom, need_dgrad=False)
    assert none is None and torch.equal(wf2.cpu().view(torch.int16), hf.view(torch.int16))


# ------------------------------------------------------------------------------------------------
def check_fwd(device, C, Cg, s, d, stats=True, bias=False, relu=False, xpad=0, xoff=0, ypad=0, seed=0):
    """sf_gconv_fwd: y per element, stat_part per partial row (module docstring)."""
    geom = _geom(C, Cg, s, d)
    gen, x, w, _ = _draw(seed, geom)
    w16 = w.to(ACT).double()
    wf, _ = ops.gconv_prep_weights(w.to(device), geom, need_dgrad=False)
    b = torch.randn(C, generator=gen) * 0.5 if bias else None
    xc = _cl_in(x, device, xpad, xoff)
    out = _Out(geom.out_shape, device, ypad)
    M = geom.out_rows
    y, part = ops.gconv_fwd(xc, wf, geom, bias=None if b is None else b.to(device), relu=relu, stats=stats, out=out.view)
    assert y is out.view
    t = _rows(_conv64(x, w16, geom))
    A = _rows(_conv64(x.abs(), w16.abs(), geom))
    if b is not None:
        t, A = t + b.double(), A + b.double().abs()
    E = (9 * geom.B + int(bias)) * U32 * A
    ref = t.clamp(min=0) if relu else t
    name = "gconv_fwd[%s%s%s]" % (case_id((C, Cg, s, d)), " bias" if bias else "", " relu" if relu else "")
    got = out.rows()
    out.assert_canaries(name)
    if relu:
        assert float(got.min()) >= 0.0
    _note("fwd y", got, ref, 2 * U16 * ref.abs() + TINY + E * (1 + U16))
    _assert_stored(name + " y", got, ref, E * (1 + U16))
    if not stats:
        assert part is None
        return
    assert tuple(part.shape) == (_cdiv(M, 128), 2, C)
    part = part.detach().cpu().double()
    D = 128
    s_ref, q_ref = _tile_sums(t, 128), _tile_sums(t * t, 128)
    s_b = _tile_sums(E, 128) + D * U32 * _tile_sums(t.abs(), 128)
    q_b = _tile_sums(2 * t.abs() * E + E * E, 128) + (D + 1) * U32 * q_ref
    _note("fwd stat sum", part[:, 0], s_ref, s_b)
    _note("fwd stat sumsq", part[:, 1], q_ref, q_b)
    _assert_fp32(name + " stat sum", part[:, 0], s_ref, s_b)
    _assert_fp32(name + " stat sumsq", part[:, 1], q_ref, q_b)


def check_dgrad(device, C, Cg, s, d, dypad=0, xpad=0, seed=0):
    """sf_gconv_dgrad: dx per element.  The BatchNorm-backward reduction is not fused into this data gradient: the engine is handed
    part = None (asserted through GroupedConvUnit in check_unit_contract)."""
    geom = _geom(C, Cg, s, d)
    _, _, w, dy = _draw(seed, geom)
    w16 = w.to(ACT).double()
    _, wd = ops.gconv_prep_weights(w.to(device), geom)
    dyc = _cl_in(dy, device, dypad)
    out = _Out(geom.in_shape, device, xpad)
    ops.gconv_dgrad(dyc, wd, geom, out=out.view)
    ref = _rows(_dgrad64(dy, w16, geom))
    A = _rows(_dgrad64(dy.abs(), w16.abs(), geom))
    E = 9 * geom.B * U32 * A
    name = "gconv_dgrad[%s]" % case_id((C, Cg, s, d))
    got = out.rows()
    out.assert_canaries(name)
    _note("dgrad dx", got, ref, 2 * U16 * ref.abs() + TINY + E * (1 + U16))
    _assert_stored(name + " dx", got, ref, E * (1 + U16))


def _bundle_geom(geom):
    return ops.ConvGeom((geom.N, geom.B, geom.Ti, geom.Hi, geom.Wi), geom.B, geom.k, geom.s, geom.p, geom.d)


def wgrad_plan(geom):
    """plan_gconv_wgrad of sf_api.hip restated on the dense plans conv_elem_checks restates: (variant, L of the bound, workspace
    bytes).  The dense planner picks path and tiles for one bundle's B -> B geometry; the nb bundles share one grid, so each takes
    1 / nb of that plan's splits, one split per workgroup."""
    bg, nb, M = _bundle_geom(geom), geom.Ci // geom.B, geom.out_rows
    w2 = cc.plan_wgrad2(bg)
    if w2 is not None:
        per_split = (w2["ws_bytes"] - w2["tab_bytes"]) // w2["splits"]
        rps = cc._roundup(_cdiv(M, max(1, w2["splits"] // nb)), 128 if w2["thin"] else 32)
        splits = _cdiv(M, rps)
        name = w2["name"].replace("dual", "single")
        return name, rps + splits + 2, w2["tab_bytes"] + nb * splits * per_split
    w1 = cc.plan_wgrad(bg)
    KS = 4 if w1["BMW"] <= 32 else 1
    nchunks = _cdiv(M, 32)
    nstages = _cdiv(nchunks, KS)
    cps = _cdiv(nstages, max(1, min(w1["splits"] // nb, nstages))) * KS
    splits = _cdiv(nchunks, cps)
    return "wgrad_bmw%d" % w1["BMW"], cps * 32 + splits + 2, nb * splits * (w1["ws_bytes"] // w1["splits"])


def check_wgrad(device, C, Cg, s, d, out_scale=1.0, accumulate=False, xpad=0, dypad=0, zero_group=None, want=None, seed=0):
    """sf_gconv_wgrad: dw (+)= out_scale * dL/dw per element, guards around dw, two runs bit-equal.  ``zero_group``: the input channels
    of that group are zero -> exact zeros in that group's dw (zero_first), and only there.  ``want``: the dense weight-gradient
    variant the bundle's geometry takes under the environment of the case (conv_elem_checks.wgrad_variant)."""
    geom = _geom(C, Cg, s, d)
    gen, x, w, dy = _draw(seed, geom)
    if zero_group is not None:
        x[:, zero_group * Cg:(zero_group + 1) * Cg] = 0.0
    xc, dyc = _cl_in(x, device, xpad), _cl_in(dy, device, dypad)
    variant, L, ws_bytes = wgrad_plan(geom)
    if want is not None:
        cc._assert_variant(variant, want)
    from ctypes import byref
    assert ops.get_lib().call("sf_gconv_wgrad_workspace", byref(geom.desc(geom.Ci, geom.Co))) == ws_bytes, "the restated plan"
    n = w.numel()
    prior = torch.randn(w.shape, generator=gen) if accumulate else torch.full(w.shape, 7.0)
    runs = []
    for _ in range(2):
        flat = torch.full((2 * GUARD + n,), CANARY32, dtype=torch.int32, device=device).view(torch.float32)
        dw = flat[GUARD:GUARD + n].view(w.shape)
        dw.copy_(prior)
        ops.gconv_wgrad(xc, dyc, geom, dw, out_scale=out_scale, zero_first=not accumulate)
        bits = flat.detach().cpu().view(torch.int32)
        assert bool((bits[:GUARD] == CANARY32).all()) and bool((bits[-GUARD:] == CANARY32).all()), "sf_gconv_wgrad wrote outside dw"
        runs.append(bits[GUARD:GUARD + n].clone())
    assert torch.equal(runs[0], runs[1]), "two runs of sf_gconv_wgrad differ"
    got = runs[0].view(torch.float32).view(w.shape).double()
    sc32 = float(torch.tensor(out_scale, dtype=torch.float32))
    G = _wgrad64(x, dy, w.shape, geom)
    A = _wgrad64(x.abs(), dy.abs(), w.shape, geom)
    ref = sc32 * G + (prior.double() if accumulate else 0.0)
    E = L * U32 * (abs(sc32) * A + (prior.double().abs() if accumulate else 0.0))
    name = "gconv_wgrad[%s %s] L = %d" % (case_id((C, Cg, s, d)), variant, L)
    _note("wgrad dw", got, ref, E)
    _assert_fp32(name, got, ref, E)
    if zero_group is not None and not accumulate:
        zero = torch.zeros(w.shape, dtype=torch.bool)
        zero[zero_group * Cg:(zero_group + 1) * Cg] = True
        assert bool((got[zero] == 0).all()), "a group with zero input channels must have an exactly zero weight gradient"
        assert bool((got[~zero] != 0).all()), "... and only that group"


# ------------------------------------------------------------------------------------------------
def check_rejects(device):
    """Every unsupported request fails with a message that names what was asked for and writes nothing."""
    N, T, H, W = 1, 1, 6, 6
    cases = [  # (C, groups, kernel, stride, padding, message)
        (64, 32, (1, 3, 3), (1, 1, 1), (0, 1, 1), "2 channels per group"),
        (48, 4, (1, 3, 3), (1, 1, 1), (0, 1, 1), "12 channels per group"),
        (16, 2, (1, 3, 3), (1, 1, 1), (0, 1, 1), "C=16 with Cg=8"),
        (64, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1), "kernel (3,3,3)"),
        (64, 8, (1, 3, 3), (1, 3, 3), (0, 1, 1), "stride (1,3,3)"),
    ]
    for C, G, k, s, p, msg in cases:
        geom = ops.GroupedConvGeom((N, C, T, H, W), G, k, s, p, 1)
        gen = torch.Generator().manual_seed(1)
        x = _cl_in(torch.randn(geom.in_shape, generator=gen).to(ACT).double(), device, 8)
        dy = _cl_in(torch.randn(geom.out_shape, generator=gen).to(ACT).double(), device, 8)
        w = torch.randn((C, C // G) + geom.k, generator=gen).to(device)
        wcan = torch.full((C, geom.ldw), cc.CANARY, dtype=torch.int16, device=device).view(ACT)
        lib = ops.get_lib()
        st = ops._stream(x)
        from ctypes import byref
        desc = geom.desc(ops.cl_ld(x), ops.cl_ld(dy))
        wf, wd = wcan.clone(), wcan.clone()
        _expect_error(lambda: lib.call("sf_gconv_prep_weights", byref(desc), w.data_ptr(), wf.data_ptr(), wd.data_ptr(), st), msg)
        assert torch.equal(wf.view(torch.int16), wcan.view(torch.int16)) and torch.equal(wd.view(torch.int16), wcan.view(torch.int16))
        out = _Out(geom.out_shape, device, 8)
        _expect_error(lambda: ops.gconv_fwd(x, wcan, geom, out=out.view), msg)
        out.assert_canaries("rejected sf_gconv_fwd", untouched=True)
        dx = _Out(geom.in_shape, device, 8)
        _expect_error(lambda: ops.gconv_dgrad(dy, wcan, geom, out=dx.view), msg)
        dx.assert_canaries("rejected sf_gconv_dgrad", untouched=True)
        dw = torch.full(w.shape, 7.0, device=device)
        _expect_error(lambda: ops.gconv_wgrad(x, dy, geom, dw), msg)
        assert bool((dw == 7.0).all()), "a rejected sf_gconv_wgrad wrote to dw"


def check_builder_rejects():
    """The Python builder names the cfg keys (no native call is made)."""
    import pytest
    from slowfast_amd.resblocks import BasicTransform, BottleneckTransform
    for inner, groups, why in ((24, 3, "Cg = 8, 24 channels are no whole 32-channel bundle"), (64, 32, "Cg = 2"), (48, 4, "Cg = 12")):
        with pytest.raises(NotImplementedError, match=r"RESNET\.NUM_GROUPS / RESNET\.WIDTH_PER_GROUP"):
            BottleneckTransform(64, 256, 1, 1, inner, groups)
    import slowfast_amd as sa
    cfg = model_cfg(["RESNET.NUM_GROUPS", 3])                   # inner widths 12 .. 96: no whole 32-channel bundles of 4-channel groups
    with pytest.raises(NotImplementedError, match=r"groups=3 .*RESNET\.NUM_GROUPS / RESNET\.WIDTH_PER_GROUP"):
        sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    # the reference's BasicTransform takes num_groups and ignores it (resnet_helper.py:27-115): so does the drop-in
    t = BasicTransform(64, 64, 1, 1, dim_inner=32, num_groups=8)
    assert t.a.groups == 1 and t.b.groups == 1


# ------------------------------------------------------------------------------------------------
# block level
def _ref_block(x, p, stride, groups, masks, stats):
    """relu(shortcut(x) + c_bn(c(relu(b_bn(b(relu(a_bn(a(x))))))))) in torch fp32 from the parameters ``p`` (keys of ResBlock's
    state_dict under "blk."), train mode; b is nn.functional.conv3d(groups=groups).  The ReLUs' backward masks are handed in."""
    from oracle.video_ref import _ReluFixedMask

    def bn(y, name):
        rm, rv = p[name + ".running_mean"].clone(), p[name + ".running_var"].clone()
        y = F.batch_norm(y, rm, rv, p[name + ".weight"], p[name + ".bias"], True, 0.1, 1e-5)
        stats[name + ".running_mean"], stats[name + ".running_var"] = rm, rv
        return y
    b2 = "blk.branch2"
    y = _ReluFixedMask.apply(bn(F.conv3d(x, p[b2 + ".a.weight"]), b2 + ".a_bn"), masks["a"])
    y = F.conv3d(y, p[b2 + ".b.weight"], None, (1, stride, stride), (0, 1, 1), 1, groups)
    y = _ReluFixedMask.apply(bn(y, b2 + ".b_bn"), masks["b"])
    y = bn(F.conv3d(y, p[b2 + ".c.weight"]), b2 + ".c_bn")
    sc = x
    if "blk.branch1.weight" in p:
        sc = bn(F.conv3d(x, p["blk.branch1.weight"], None, (1, stride, stride)), "blk.branch1_bn")
    return _ReluFixedMask.apply(sc + y, masks["out"])


def check_block(device, dim_in, dim_out, stride, shape, groups=8, inner=64, seed=3):
    """ResBlock + BottleneckTransform(num_groups=groups, dim_inner=inner) forward and backward through engine.ResBlockFn in train
    mode against ``_ref_block``; method and tolerance of block_checks.check_resblock (module docstring)."""
    from slowfast_amd import engine
    from slowfast_amd.resblocks import BottleneckTransform, ResBlock
    from tests import block_checks as bc
    from tests.kernel_checks import cl_to_host, host_to_cl
    torch.manual_seed(seed)
    blk = ResBlock(dim_in, dim_out, 1, stride, BottleneckTransform, inner, num_groups=groups)
    assert isinstance(blk.branch2._b, engine.GroupedConvUnit) and tuple(blk.branch2.b.weight.shape) == (inner, inner // groups, 1, 3, 3)
    sd = bc._load(blk, seed)
    blk = blk.to(device).train()
    x = torch.randn(shape).to(ACT).float()
    N, _, T, H, W = shape
    dout = torch.randn((N, dim_out, T, (H - 1) // stride + 1, (W - 1) // stride + 1)).to(ACT).float()
    xc = host_to_cl(x, device).requires_grad_(True)
    engine.CAPTURE = []
    try:
        out = blk(xc)
        cap = engine.CAPTURE[-1]
    finally:
        engine.CAPTURE = None
    out.backward(host_to_cl(dout, device))
    masks = {key: bc._pre_mask(raw, sc, sh) for key, raw, (sc, sh) in zip(("a", "b"), cap["raw"], cap["bn"])}
    masks["out"] = (cl_to_host(cap["out"]) > 0).float()

    def body(p, st):
        xr = x.clone().requires_grad_(True)
        o = _ref_block(xr, p, stride, groups, masks, st)
        o.backward(dout)
        return {"out": o.detach(), "dx": xr.grad}
    ref, rg, st = bc._oracle_run(bc._Case(sd, "blk.", body))
    flips = bc._flip_fraction(masks["out"], (ref["out"] > 0).float())
    assert flips <= bc.MAX_FLIP_FRACTION, flips
    errs = bc._compare(blk, "blk.", {"out": cl_to_host(out), "dx": cl_to_host(xc.grad)}, ref, rg, st)
    print("gconv block %s: worst rel L2 = %.2e (tol %.1e), flipped %.1e" % (
        "proj s%d" % stride if dim_in != dim_out or stride != 1 else "identity", max(v for v in errs.values()), bc.TOL, flips))
    return errs


def check_unit_contract(device):
    """What engine.ResBlockFn asks of unit b: no fused reductions (fused_c_geom / fused_proj_geom None, part None under bn_fuse), a
    weight re-packed when its version changes and on every forward under FORCE_WEIGHT_PREP, never in a WeightPackPlan record."""
    from slowfast_amd import engine
    from tests.kernel_checks import host_to_cl
    conv = torch.nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1), groups=8, bias=False).to(device)
    bn = torch.nn.BatchNorm3d(64).to(device)
    u = engine.GroupedConvUnit(conv, bn)
    x = host_to_cl(torch.randn(1, 64, 1, 6, 6), device)
    assert u.fused_c_geom(x) is None and u.fused_proj_geom(x) is None
    engine.PACK_RECORD = rec = []
    try:
        y, st = u.forward(x, None, True)
        w0 = u._w[0]
        u.forward(x, None, True)
        assert u._w[0] is w0, "an unchanged weight is not packed again"
        with torch.no_grad():
            conv.weight.mul_(2.0)
        y2, _ = u.forward(x, None, True)
        assert u._w[0] is not w0 and torch.equal(u._w[0].cpu().view(torch.int16), pack_host(conv.weight.detach().cpu(), u.geom(x.shape))[0].view(torch.int16))
        engine.FORCE_WEIGHT_PREP = True
        w1 = u._w[0]
        u.forward(x, None, True)
        assert u._w[0] is not w1, "FORCE_WEIGHT_PREP re-packs on every forward (a captured step replays the pack)"
    finally:
        engine.PACK_RECORD, engine.FORCE_WEIGHT_PREP = None, False
    assert rec == [], "grouped units stay out of WeightPackPlan"
    dy = torch.randn_like(y)
    dx, part = u.backward(x, None, dy, need_dx=True, bn_fuse=(y, st))
    assert part is None and tuple(dx.shape) == tuple(x.shape)
    assert conv.weight.grad is not None and tuple(conv.weight.grad.shape) == (64, 8, 1, 3, 3)


# ------------------------------------------------------------------------------------------------
# model level
MODEL_OPTS = ["RESNET.NUM_GROUPS", 8, "RESNET.WIDTH_PER_GROUP", 4, "RESNET.DEPTH", 50, "MODEL.NUM_CLASSES", 10, "MODEL.DROPOUT_RATE", 0.0,
              "DATA.NUM_FRAMES", 4, "DATA.TRAIN_CROP_SIZE", 64]
MODEL_PRESET, MODEL_BATCH, PARAM_SEED, DATA_SEED = "SLOW_8x8_R50", 2, 31, 32
_model_ref = {}


def model_cfg(extra=()):
    import slowfast_amd as sa
    return sa.get_preset(MODEL_PRESET, MODEL_OPTS + list(extra))


def is_grouped_b(key, v):
    return key.endswith(".branch2.b.weight") and v.shape[1] != v.shape[0]


def expand_b(w):
    """grouped [C][Cg][1][3][3] -> the dense block-diagonal [C][C][1][3][3]"""
    C, Cg = w.shape[:2]
    dense = torch.zeros((C, C) + tuple(w.shape[2:]), dtype=w.dtype)
    for g in range(C // Cg):
        dense[g * Cg:(g + 1) * Cg, g * Cg:(g + 1) * Cg] = w[g * Cg:(g + 1) * Cg]
    return dense


def extract_b(dense, Cg):
    """the diagonal blocks of a dense [C][C][...] tensor as [C][Cg][...]"""
    C = dense.shape[0]
    return torch.cat([dense[g * Cg:(g + 1) * Cg, g * Cg:(g + 1) * Cg] for g in range(C // Cg)], 0)


def dense_state(sd):
    return {k: expand_b(v) if is_grouped_b(k, v) else v for k, v in sd.items()}


def model_reference():
    """The existing oracle (oracle.video_ref, a function of the state alone: it takes its widths from the weights) on the
    dense-equivalent state of the grouped model; computed once per process and shared.  The b gradients come back through the
    diagonal extraction.  Also the oracle's fp16-storage-model yardstick of the case (model_checks.storage_model_yardstick)."""
    if _model_ref:
        return _model_ref
    import slowfast_amd as sa
    from oracle import video_ref
    from tests import model_checks as mc
    cfg = model_cfg()
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    cgs = sorted({s[1] for k, s in shapes.items() if k.endswith(".branch2.b.weight")})
    assert cgs == [4, 8, 16, 32], cgs
    sd = video_ref.randomize_state(shapes, PARAM_SEED)
    inputs, labels = video_ref.synthetic_batch(cfg, MODEL_BATCH, DATA_SEED)
    dsd = dense_state(sd)
    logits, loss, grads, stats = video_ref.loss_and_grads(dsd, cfg, inputs, labels)
    yard = mc.storage_model_yardstick("resnext_slow_g8w4", dsd, cfg, inputs, labels, logits, loss, grads, stats)
    grads = {k: extract_b(g, sd[k].shape[1]) if is_grouped_b(k, sd[k]) else g for k, g in grads.items()}
    # the yardstick's worst parameter is taken over the dense gradients: the off-diagonal blocks of a b gradient are not parameters of
    # the grouped model, so it can only overstate "param_grad_worst" through them; that entry is recomputed on the grouped set
    with video_ref.fp16_storage_model():
        _, _, g16, _ = video_ref.loss_and_grads(dsd, cfg, inputs, labels)
    g16 = {k: extract_b(g, sd[k].shape[1]) if is_grouped_b(k, sd[k]) else g for k, g in g16.items()}
    ogn = float(video_ref.grad_norm(grads))
    yard = dict(yard, param_grad_worst=mc._param_worst(g16, grads, ogn)[0], grad_global=mc._global_rel(g16, grads),
                grad_norm=abs(float(video_ref.grad_norm(g16)) - ogn) / ogn)
    _model_ref.update(cfg=cfg, sd=sd, dsd=dsd, inputs=inputs, labels=labels, logits=logits, loss=loss, grads=grads, stats=stats, yard=yard)
    return _model_ref


def check_model(device, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=1e-3, tol_param=2e-2, tol_stats=2e-3, tol_global=1e-2):
    """Forward + CE + backward of the grouped drop-in model against the dense-equivalent oracle run: the quantities, the bound rule
    (max(tol, YARD x the oracle's fp16-storage-model deviation)) and the default tolerances of model_checks.check_engine."""
    import slowfast_amd as sa
    from oracle import video_ref
    from tests import model_checks as mc
    r = model_reference()
    tols = {k: t * mc.EPS_SCALE for k, t in dict(logits=tol_logits, loss=tol_loss, grad_norm=tol_gnorm, param_grad_worst=tol_param,
                                                 running_stats=tol_stats, grad_global=tol_global).items()}
    model = sa.MODEL_REGISTRY.get(r["cfg"].MODEL.MODEL_NAME)(r["cfg"])
    model.load_state_dict(r["sd"])
    model = model.to(device).train()
    logits, loss, table = mc._engine_run(model, r["inputs"], r["labels"], device, 1.0, True)
    o_logits, o_grads = r["logits"], r["grads"]
    grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    assert set(grads) == set(o_grads)
    gn, ogn = float(video_ref.grad_norm(grads)), float(video_ref.grad_norm(o_grads))
    msd = model.state_dict()
    res = {"logits": float((logits.detach().float().cpu() - o_logits).abs().max() / o_logits.abs().max()),
           "loss": abs(float(loss.detach()) - float(r["loss"])) / max(1.0, abs(float(r["loss"]))),
           "grad_norm": abs(gn - ogn) / ogn, "grad_global": mc._global_rel(grads, o_grads),
           "running_stats": max(float((msd[k].float().cpu() - v).abs().max() / (v.abs().max() + 1e-6)) for k, v in r["stats"].items())}
    res["param_grad_worst"], res["param_grad_worst_name"] = mc._param_worst(grads, o_grads, ogn)
    bound = {k: max(t, mc.YARD * r["yard"][k]) for k, t in tols.items()}
    bound["grad_norm"] = max(bound["grad_norm"], 0.5 * bound["grad_global"] ** 2)
    for k in bound:
        print("gconv model %s: %.3e (bound %.3e)" % (k, res[k], bound[k]))
    for k in bound:
        assert res[k] <= bound[k], (k, res, bound)
    # The gradient VECTOR under the engine's own ReLU masks / pool routes (model_checks.masked_grad_global, restated here because the b
    # gradients pass through the diagonal extraction in between): flipped elements excluded, every other element of every parameter
    # gradient must agree -- TOL_GRAD_GLOBAL, or YARD x the oracle's fp16 storage model under the same masks when that is larger.
    def grouped(gr):
        return {k: extract_b(g, r["sd"][k].shape[1]) if is_grouped_b(k, r["sd"][k]) else g for k, g in gr.items()}
    with video_ref.handed_masks(table):
        _, _, m_grads, _ = video_ref.loss_and_grads(r["dsd"], r["cfg"], list(r["inputs"]), r["labels"])
    m_grads = grouped(m_grads)
    val, b_masked = mc._global_rel(grads, m_grads), mc.TOL_GRAD_GLOBAL * mc.EPS_SCALE
    if val > b_masked:
        with video_ref.fp16_storage_model(), video_ref.handed_masks(table):
            _, _, s_grads, _ = video_ref.loss_and_grads(r["dsd"], r["cfg"], list(r["inputs"]), r["labels"])
        b_masked = max(b_masked, mc.YARD * mc._global_rel(grouped(s_grads), m_grads))
    bkeys = [k for k in grads if is_grouped_b(k, r["sd"][k])]
    worst_b = max(float((grads[k] - m_grads[k]).norm() / m_grads[k].norm()) for k in bkeys)
    print("gconv model masked grad_global: %.3e (bound %.3e); worst grouped b.weight gradient: %.3e" % (val, b_masked, worst_b))
    res["masked_grad_global"], res["masked_worst_b"] = val, worst_b
    assert val <= b_masked, (val, b_masked)
    return res


def check_model_eval(device, tol=2e-3):
    """fuse_for_inference on the grouped model against the oracle's eval logits of the dense-equivalent state (running statistics
    calibrated as model_checks.check_eval calibrates them); check_eval's rule: max |p - p_ref| <= max(tol, 2.5 x the oracle's
    fp16-storage-model deviation) * max p_ref (no autocast entry exists for this case, so the storage model alone)."""
    import slowfast_amd as sa
    from oracle import video_ref
    from oracle.make_golden import eval_forward
    from slowfast_amd import inference
    r = model_reference()
    cfg, inputs = r["cfg"], r["inputs"]
    dsd = video_ref.calibrate_running_stats(dict(r["dsd"]), cfg, inputs)
    with torch.no_grad():
        o_probs = eval_forward(dsd, cfg, inputs)
        with video_ref.fp16_storage_model():
            yard = float((eval_forward(dsd, cfg, inputs) - o_probs).abs().max() / o_probs.max())
    sd = {k: extract_b(v, r["sd"][k].shape[1]) if is_grouped_b(k, r["sd"][k]) else v for k, v in dsd.items()}
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    model.load_state_dict(sd)
    model = model.to(device).eval()
    with torch.no_grad():
        plain = model([x.to(device) for x in inputs]).float().cpu()
    inference.fuse_for_inference(model)
    assert model.__dict__["_sf_fused_modules"] > 0
    with torch.no_grad():
        probs = model([x.to(device) for x in inputs]).float().cpu()
    inference.unfuse(model)
    assert not any("_sf_infer" in m.__dict__ for m in model.modules())
    res = {"fused": float((probs - o_probs).abs().max() / o_probs.max()), "unfused": float((plain - o_probs).abs().max() / o_probs.max())}
    print("gconv model eval: fused %.3e unfused %.3e (bound %.3e)" % (res["fused"], res["unfused"], max(tol, 2.5 * yard)))
    assert probs.shape == o_probs.shape and float((probs.sum(1) - 1).abs().max()) <= 2e-3
    assert res["fused"] <= max(tol, 2.5 * yard) and res["unfused"] <= max(tol, 2.5 * yard), res
    return res


# ------------------------------------------------------------------------------------------------
# pinned to the reference (tests/golden/resnext_contract.json, recorded by tools/make_resnext_golden.py)
REFERENCE_YAML = "configs/Kinetics/SLOW_8x8_R50.yaml"
CONTRACT = "resnext_contract"


def reference_record():
    """What the UNMODIFIED reference ResNet of the model-level cfg gives on the case of ``model_reference`` (needs the reference tree,
    oracle.refshim): state_dict keys and shapes, logits, loss, gradient norm, per-parameter gradient norms, running-statistic sums."""
    from oracle import refshim, video_ref
    cfg = refshim.reference_cfg(REFERENCE_YAML, ["NUM_GPUS", 0] + MODEL_OPTS)
    torch.manual_seed(0)
    model = refshim.reference_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = video_ref.randomize_state(shapes, PARAM_SEED)
    model.load_state_dict(sd)
    model.train()
    inputs, labels = video_ref.synthetic_batch(cfg, MODEL_BATCH, DATA_SEED)
    logits = model([x.clone() for x in inputs])
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    return {"reference_yaml": REFERENCE_YAML, "opts": MODEL_OPTS, "batch": MODEL_BATCH, "param_seed": PARAM_SEED, "data_seed": DATA_SEED,
            "state_dict": [[k, list(s)] for k, s in shapes.items()],
            "logits": logits.detach().tolist(), "loss": float(loss.detach()), "grad_norm": float(video_ref.grad_norm(grads)),
            "param_grad_norms": {k: float(g.norm()) for k, g in grads.items()},
            "running_stat_sums": {k: float(v.double().sum()) for k, v in model.state_dict().items() if "running" in k},
            "num_params": sum(g.numel() for g in grads.values()), "torch_version": torch.__version__}


def check_contract(rec):
    """The drop-in's state_dict list equals the recorded one, the reference's keys load strictly, and the dense-equivalent oracle
    reproduces the recorded reference numbers to fp32 round-off: the relative bounds model_checks.check_oracle_against_golden holds
    the oracle to on its existing goldens (1e-5 logits and loss, 1e-4 gradient norm, 2e-4 per parameter with its floor, 1e-4 on the
    running-statistic sums), not new numbers."""
    import slowfast_amd as sa
    from oracle import video_ref
    assert rec["opts"] == MODEL_OPTS and (rec["batch"], rec["param_seed"], rec["data_seed"]) == (MODEL_BATCH, PARAM_SEED, DATA_SEED)
    r = model_reference()
    model = sa.MODEL_REGISTRY.get(r["cfg"].MODEL.MODEL_NAME)(r["cfg"])
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == rec["state_dict"]
    ref_state = {k: torch.zeros(s) if len(s) else torch.zeros((), dtype=torch.long) for k, s in rec["state_dict"]}
    model.load_state_dict(ref_state, strict=True)
    logits, loss, grads, stats = r["logits"], r["loss"], r["grads"], r["stats"]
    ref_logits = torch.tensor(rec["logits"])
    assert float((logits - ref_logits).abs().max() / ref_logits.abs().max()) < 1e-5
    assert abs(float(loss) - rec["loss"]) < 1e-5 * max(1.0, abs(rec["loss"]))
    assert abs(float(video_ref.grad_norm(grads)) - rec["grad_norm"]) < 1e-4 * rec["grad_norm"]
    assert sum(g.numel() for g in grads.values()) == rec["num_params"], "the diagonal extraction has the grouped parameter count"
    for k, n in rec["param_grad_norms"].items():
        assert abs(float(grads[k].norm()) - n) <= 2e-4 * max(n, 1e-3 * rec["grad_norm"]), k
    for k, s in rec["running_stat_sums"].items():
        assert abs(float(stats.get(k, r["sd"][k]).double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


# ------------------------------------------------------------------------------------------------
def check_train_step(device, steps=3):
    """step.TrainStep on the grouped model: the captured-graph iterations (weights re-packed inside the graph by the grouped units' own
    launches) against the eager ones, bit for bit -- every loss, every parameter and every buffer, as tests/test_step.py asserts for
    the dense models."""
    import slowfast_amd as sa
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.step import TrainStep
    r = model_reference()

    def run(use_graph):
        model = sa.MODEL_REGISTRY.get(r["cfg"].MODEL.MODEL_NAME)(r["cfg"])
        model.load_state_dict(r["sd"])
        model = model.to(device).train()
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
        red = GradReducer(model)
        step = TrainStep(model, red, opt, F.cross_entropy, loss_scale=8.0, use_graph=use_graph, warmup=1)
        g = torch.Generator().manual_seed(9)
        losses = []
        for _ in range(steps):
            x = [(v + 0.1 * torch.randn(v.shape, generator=g)).to(device) for v in r["inputs"]]
            losses.append(step(x, r["labels"].to(device)).detach().float().cpu().clone())
        red.close()
        return losses, [t.detach().float().cpu().clone() for t in list(model.parameters()) + list(model.buffers())]
    le, se = run(False)
    lg, sg = run(True)
    print("gconv train step losses:", [float(v) for v in le])
    for a, b in zip(le, lg):
        assert torch.equal(a, b), (le, lg)
    assert not torch.equal(le[0], le[-1]), "the optimizer update must reach the packed grouped weights"
    for a, b in zip(se, sg):
        assert torch.equal(a, b)
