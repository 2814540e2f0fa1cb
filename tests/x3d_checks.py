"""Kernel-level parity checks of the X3D entry points (csrc/sf_x3d.h and their launchers: per-sample sums, the SE gate, the
gate * BatchNorm -> Swish/ReLU pass with its backward forms, sf_outer_sum, sf_bn_bwd_apply_sample), shared by the host-simulator
file (tests/test_x3d_kernels_hostsim.py) and the -m gpu file (tests/test_x3d_kernels_gpu.py).

Reference = plain torch in float64 on the CPU, evaluated on the operands the kernel sees (activations already rounded to the
storage type; fp32 scale / shift / gate / weights as they are).  Every comparison is PER ELEMENT; the bounds are derived from the
number formats, with u16 = lib.act_eps() (unit roundoff of the storage type, one ulp at 1.0 = kernel_checks.F16_EPS = 2 * u16)
and u32 = 2^-24:

* stored 16-bit outputs (z, du, du0, dy): |got - ref| <= 2 * u16 * |ref| + tiny -- half an ulp from the store plus the chance that
  the fp32 arithmetic moves the value across a rounding boundary; tiny = the smallest subnormal of the type.  The backward forms
  add 8 * u32 * (|dz| * |g| + |dmean| / S), evaluated from the operands: expf, the fp32 rounding of 1 / S and of the two-term sum,
  which matter where dz * act'(g * u) * g is close to zero or cancels against dmean / S.
* fp32 sums over positions: |got - ref| <= D * u32 * sum|term| (sum|term| in fp64), D = the longest chain of additions,
  ``chain_len``: passes + 8 + chunks / 2 + 2 under the tile rule of ``tile_plan``.
* sums of stored values (sums[:, 1:], bn_part): the terms are the kernel's OWN stored du0 / du, read back, times the stored y -- what
  the BatchNorm backward relies on; same bound.
* SE gate: (K + 4) * u32 * (sum|w * x| + |b|) per dot product of length K, propagated through sigmoid (slope <= 1/4) and ReLU.

Ties are a condition on the inputs, not a tolerance (``_draw``): the BatchNorm output u = y * scale + shift stays away from zero
by at least 2^-10 * (|y * scale| + |shift|) -- below that the fp32 rounding of u (u32 * (|y * scale| + |shift|), not contracted
on the host simulator) is no longer small against one 16-bit ulp of act(g * u) -- and |gate * u| >= 1e-4, so a ReLU never flips.
"""
import types

import torch

from slowfast_amd import lib as _sflib
from slowfast_amd import ops, x3d
from slowfast_amd.lib import SfError, get_lib
from tests.kernel_checks import ACT, F16_EPS

U16 = _sflib.act_eps()
assert F16_EPS == 2 * U16
U32 = 2.0 ** -24
TINY = float(torch.finfo(ACT).smallest_normal) * float(torch.finfo(ACT).eps)       # smallest subnormal: 2^-24 fp16, 2^-133 bf16
MAX_DRAWS = 3

# (id, N, C, S, ld_extra): the smallest shapes that reach each path of the row-tile kernels
ROWS = [
    ("head_S1", 3, 432, 1, 0),              # one position per sample (the head's pooled map)
    ("one_group", 2, 8, 5, 0),              # fewer rows than one pass, one column group (wave-butterfly reduce)
    ("G7_boundary", 3, 56, 45, 0),          # G = 7 does not divide 256 (54 -> 56), sample boundary inside a tile, 2 chunks
    ("ragged_chunk", 2, 112, 199, 0),       # 108 -> 112, 12 chunks of 18 rows, the last one holds a single row
    ("two_passes", 2, 432, 338, 0),         # rpi = 4, S > 256: two passes per workgroup in the per-sample sum, 43 chunks
    ("full_width", 2, 2048, 70, 0),         # rpi = 1, full-width column tile, two passes
    ("C2056", 1, 2056, 3, 0),               # blockIdx.y = 1 of RowTile; the per-sample sums reject C > 2048
    ("pitch8", 2, 56, 45, 8),               # row pitch wider than C
    ("pitch64", 2, 56, 45, 64),
]
BIG_ROW = ("two_row_passes", 3, 432, 3000, 0)   # M > rpi * 2048: two passes in the row kernels (gate_act bwd_bn, apply_sample)
MODES = [(True, True), (True, False), (False, True), (False, False)]        # (gated, swish)
SE_CASES = [(3, 54, 56, 8), (2, 108, 112, 8), (1, 432, 432, 32), (2, 1024, 1024, 1024), (1, 1000, 1024, 72)]
OUTER_CASES = [
    # N, I, J, with_b, accumulate, lda_extra, ldb_extra, scale
    (3, 54, 8, True, 0, 2, 0, 1.0),         # fc2.weight: a = dpre2 [N][Cp = 56], b = h [N][8]; I * J = 432
    (3, 54, 1, False, 0, 2, 0, 1.0),        # fc2.bias: b = None, J = 1
    (2, 8, 108, True, 1, 0, 4, 0.5),        # fc1.weight: b = m [N][Cp = 112], accumulated onto an earlier gradient
    (4, 8, 1, False, 1, 0, 0, 1.0),
    (5, 37, 19, True, 0, 3, 5, -2.0),       # I * J = 703: three workgroups, the last one ragged
    (1, 300, 1, False, 0, 0, 0, 1.0),       # two workgroups without b
]
CHAIN_CASES = [(4, 54, 196), (2, 432, 50)]


def tile_plan(M, C, max_blocks):
    """The row-tile rule of make_rowtile (sf_api.hip): G = C / 8 column groups, TG = min(G, 256) threads across a row,
    rpi = 256 // TG rows per pass, passes = max(1, ceil(M / (rpi * max_blocks))), rows_per_block = rpi * passes,
    chunks (workgroups along the rows) = ceil(M / rows_per_block).  Returns (rpi, passes, chunks)."""
    G = C // 8
    TG = min(G, 256)
    rpi = 256 // TG
    passes = max(1, -(-M // (rpi * max_blocks)))
    return rpi, passes, -(-M // (rpi * passes))


def chain_len(passes, chunks):
    """D: ``passes`` additions in a thread's register sum, 8 in the workgroup reduction (6 shuffle steps + 2 over the waves),
    chunks / 2 in the two-accumulator fold over the chunk partials (0 when the test folds them in fp64), 2 for joining the
    accumulators and the final scaling."""
    return passes + 8 + chunks / 2.0 + 2


def _rows_to_cl(x2d, N, S, device, ld_extra=0):
    """[N * S, C] values -> channels-last (N, C, 1, 1, S) activation of the storage type on ``device`` with row pitch C + ld_extra;
    the pitch padding holds NaN, so a kernel that strays into it poisons its result."""
    C = x2d.shape[1]
    base = torch.full((N, 1, 1, S, C + ld_extra), float("nan"), dtype=ACT, device=device)
    t = base[..., :C].permute(0, 4, 1, 2, 3)
    t.copy_(x2d.to(ACT).view(N, 1, 1, S, C).permute(0, 4, 1, 2, 3))
    return t, base


def _rows_of(t):
    """channels-last 5-D activation -> its [rows, C] values in fp64 on the CPU."""
    return t.detach().permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).cpu().double()


def _act(s, swish):
    return s * torch.sigmoid(s) if swish else s.clamp(min=0)


def _act_grad(s, swish):
    if swish:
        sg = torch.sigmoid(s)
        return sg * (1 + s * (1 - sg))
    return (s > 0).double()


def _draw(N, C, S, gated, seed, condition=True, swish=None):
    """Operands of one case, fp64 on the CPU (y and dz hold values of the storage type).  With ``condition`` the BatchNorm output
    u = y * scale + shift is kept away from zero (module docstring): elements within 0.03 of it are moved to +-0.125.
    ``swish`` (True / False, for the checks of fp32 sums): every TERM of the sum is well conditioned as well, so that its own fp32
    evaluation stays within a few u32 of it and D * u32 * sum|term| is a bound even for a sum of one term -- y * scale and shift do
    not cancel (|u| >= (|y * scale| + |shift|) / 4), and in Swish mode s = gate * u avoids (-2, -0.55), where act'(s) crosses
    zero, and s < -3.2, where |s act''(s) / act'(s)| grows like |s|; an element that fails takes the first of -y, 2y, -2y, y/2,
    -y/2, 4y, -4y that passes, else the y that gives u = max(0.5, 2 |shift|).  The draw is repeated with the next seed until every condition holds; that they hold, and that at
    most 3 draws were needed, is asserted."""
    for draw in range(MAX_DRAWS):
        g = torch.Generator().manual_seed(seed + draw)
        y = (torch.randn((N * S, C), generator=g) * 1.5 + 0.3).to(ACT).double()
        sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
        sc = ((torch.rand(C, generator=g) + 0.5) * sign).float()
        sh = (torch.randn(C, generator=g) * 0.3).float()
        gate = (0.1 + 0.85 * torch.rand((N, C), generator=g)).float() if gated else None
        dz = torch.randn((N * S, C), generator=g).to(ACT).double()
        dmean = (torch.randn((N, C), generator=g) * (0.5 * S)).float()
        if not condition:
            break
        scd, shd = sc.double(), sh.double()
        grow = 1.0 if gate is None else gate.double().repeat_interleave(S, 0)

        def holds(yv):
            u = yv * scd + shd
            ok = (u.abs() >= 2.0 ** -10 * ((yv * scd).abs() + shd.abs())) & ((u * grow).abs() >= 1e-4)
            if swish is not None:
                ok &= u.abs() >= 0.25 * ((yv * scd).abs() + shd.abs())
                if swish:
                    sv = u * grow
                    ok &= ((sv <= -2.0) | (sv >= -0.55)) & (sv >= -3.2)
            return ok
        u = y * scd + shd
        y = torch.where(u.abs() < 0.03, ((torch.where(u < 0, -0.125, 0.125) - shd) / scd).to(ACT).double(), y)
        if swish is not None:
            y0 = y
            for f in (-1.0, 2.0, -2.0, 0.5, -0.5, 4.0, -4.0):
                y = torch.where(holds(y), y, f * y0)
            safe = ((torch.maximum(2 * shd.abs(), torch.tensor(0.5, dtype=torch.float64)) - shd) / scd).to(ACT).double()
            y = torch.where(holds(y), y, safe.expand_as(y))         # u = max(0.5, 2 |shift|) > 0
        if bool(holds(y).all()):
            break
    else:
        raise AssertionError(f"no well-conditioned draw in {MAX_DRAWS} seeds")
    return dict(y=y, sc=sc, sh=sh, gate=gate, dz=dz, dmean=dmean)


def _per_row(v, S):
    return v.double().repeat_interleave(S, 0)


def _assert_stored(name, got, ref, extra=None):
    """one ulp of the storage type per element (+ the operand-evaluated fp32 term of the backward forms)."""
    bound = F16_EPS * ref.abs() + TINY
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"{name}: max err / bound = {worst:.3f}")
    assert worst <= 1.0, f"{name}: max |got - ref| / bound = {worst:.3f} at flat index {int((err / bound).argmax())}"


def _assert_sum(name, got, ref, abs_sum, D):
    bound = D * U32 * abs_sum
    err = (got.double() - ref).abs()
    ok = err <= bound
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{name}: D = {D}, max err / bound = {worst:.3f}")
    assert bool(ok.all()), f"{name}: max |got - ref| / (D u32 sum|term|) = {worst:.3f} (D = {D})"


def _dev(t, device):
    return None if t is None else t.to(device)


def _expect_error(fn, match):
    lib = get_lib()
    try:
        fn()
    except SfError as e:
        assert match in str(e), str(e)
        assert lib.cdll.sf_last_error().decode() != ""
        return
    raise AssertionError(f"expected an SfError mentioning {match!r}")


# ------------------------------------------------------------------------------------------------
def check_sample_mean(device, N, C, S, relu, affine, ld_extra=0, seed=0):
    """x3d.sample_mean (sf_sample_chunks + sf_sample_mean) against the fp64 mean over the positions of relu?(y * scale + shift), with
    and without the affine map (scale = shift = None must run); bound D * u32 * sum|term| / S with D = chain_len(passes, chunks) of
    tile_plan(S, C, 64) -- the chunk count is also compared with what sf_sample_chunks reports.  C > 2048 is rejected."""
    d = _draw(N, C, S, False, seed, condition=affine, swish=False)
    ycl, _ = _rows_to_cl(d["y"], N, S, device, ld_extra)
    sc, sh = (_dev(d["sc"], device), _dev(d["sh"], device)) if affine else (None, None)
    if C > 2048:
        _expect_error(lambda: x3d.sample_mean(ycl, sc, sh, relu), "C > 2048")
        return
    _, passes, chunks = tile_plan(S, C, 64)
    assert get_lib().call("sf_sample_chunks", S, C) == chunks
    D = chain_len(passes, chunks)
    assert D < 64
    u = d["y"] * d["sc"].double() + d["sh"].double() if affine else d["y"]
    if relu:
        u = u.clamp(min=0)
    u = u.view(N, S, C)
    got = x3d.sample_mean(ycl, sc, sh, relu)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, C)
    _assert_sum("sample_mean", got.cpu(), u.sum(1) / S, u.abs().sum(1) / S, D)


def check_gate_act(device, N, C, S, gated, swish, dmean, ld_extra=0, seed=1):
    """gate_act_fwd against fp64 act(g * u); gate_act_bwd without and (``dmean``) with the squeeze term against fp64
    dz * act'(g * u) * g + dmean / S, one ulp each; gate_act_bwd(..., bn_part=True): the same du value for value, one partial row
    per workgroup of tile_plan(N * S, C, 2048), and the rows summed in fp64 match the sums of the STORED du and of du * y within
    chain_len(passes, 0) * u32 * sum|term|.  With a wide pitch the entry points are also called with a wide OUTPUT pitch: same
    values, padding untouched."""
    d = _draw(N, C, S, gated, seed)
    y, dz = d["y"], d["dz"]
    ycl, _ = _rows_to_cl(y, N, S, device, ld_extra)
    dzcl, _ = _rows_to_cl(dz, N, S, device, ld_extra)
    sc, sh, gate = _dev(d["sc"], device), _dev(d["sh"], device), _dev(d["gate"], device)
    g = _per_row(d["gate"], S) if gated else torch.ones_like(y)
    u = y * d["sc"].double() + d["sh"].double()
    z = x3d.gate_act_fwd(ycl, sc, sh, gate, swish)
    _assert_stored("gate_act_fwd", _rows_of(z), _act(g * u, swish))
    du0_ref = dz * _act_grad(g * u, swish) * g
    du0 = x3d.gate_act_bwd(ycl, sc, sh, gate, swish, dzcl, None)
    _assert_stored("gate_act_bwd", _rows_of(du0), du0_ref, extra=8 * U32 * dz.abs() * g.abs())
    dm = _dev(d["dmean"], device) if dmean else None
    du = du0
    if dmean:
        add = _per_row(d["dmean"], S) / S
        du = x3d.gate_act_bwd(ycl, sc, sh, gate, swish, dzcl, dm)
        _assert_stored("gate_act_bwd dmean", _rows_of(du), du0_ref + add, extra=8 * U32 * (dz.abs() * g.abs() + add.abs()))
    du2, part = x3d.gate_act_bwd(ycl, sc, sh, gate, swish, dzcl, dm, bn_part=True)
    assert torch.equal(du2, du), "the fused reduction must not change the stored gradient"
    _, passes, rows = tile_plan(N * S, C, 2048)
    assert tuple(part.shape) == (rows, 2, C) and get_lib().call("sf_gate_act_bwd_bn_rows", N, S, C) == rows
    stored = _rows_of(du2)
    tot = part.double().sum(0).cpu()
    D = chain_len(passes, 0)
    _assert_sum("bn_part sum du", tot[0], stored.sum(0), stored.abs().sum(0), D)
    _assert_sum("bn_part sum du*y", tot[1], (stored * y).sum(0), (stored * y).abs().sum(0), D)
    if ld_extra:
        lib, s = get_lib(), ops._stream(ycl)
        out, base = _rows_to_cl(torch.zeros_like(y), N, S, device, ld_extra)
        lib.call("sf_gate_act_fwd", N, S, C, ycl.data_ptr(), ops.cl_ld(ycl), sc.data_ptr(), sh.data_ptr(), ops._ptr(gate),
                 int(swish), out.data_ptr(), ops.cl_ld(out), s)
        assert torch.equal(out, z) and bool(torch.isnan(base[..., C:]).all())
        out, base = _rows_to_cl(torch.zeros_like(y), N, S, device, ld_extra)
        lib.call("sf_gate_act_bwd", N, S, C, ycl.data_ptr(), ops.cl_ld(ycl), sc.data_ptr(), sh.data_ptr(), ops._ptr(gate),
                 int(swish), dzcl.data_ptr(), ops.cl_ld(dzcl), ops._ptr(dm), out.data_ptr(), ops.cl_ld(out), s)
        assert torch.equal(out, du) and bool(torch.isnan(base[..., C:]).all())


def check_gate_sums(device, N, C, S, gated, swish, ld_extra=0, seed=2):
    """gate_grad against fp64 sum_pos dz * act'(g * u) * u; gate_bwd_sums: du0 within one ulp of fp64 AND equal in value to
    gate_act_bwd(dmean=None) (both round the same fp32 product (dz * act') * g; adding the absent squeeze term 0 * (1 / S) changes
    nothing, contracted into a fused multiply-add or not), sums[:, 0] against fp64, sums[:, 1] / sums[:, 2] against the sums of the
    stored du0 / du0 * y.  All sums within chain_len(passes, chunks) * u32 * sum|term| of tile_plan(S, C, 64).  C > 2048 is
    rejected by both entry points."""
    d = _draw(N, C, S, gated, seed, swish=swish)
    y, dz = d["y"], d["dz"]
    ycl, _ = _rows_to_cl(y, N, S, device, ld_extra)
    dzcl, _ = _rows_to_cl(dz, N, S, device, ld_extra)
    sc, sh, gate = _dev(d["sc"], device), _dev(d["sh"], device), _dev(d["gate"], device)
    if C > 2048:
        _expect_error(lambda: x3d.gate_grad(ycl, sc, sh, dzcl, gate, swish), "C > 2048")
        _expect_error(lambda: x3d.gate_bwd_sums(ycl, sc, sh, gate, swish, dzcl), "C > 2048")
        return
    _, passes, chunks = tile_plan(S, C, 64)
    assert get_lib().call("sf_sample_chunks", S, C) == chunks
    D = chain_len(passes, chunks)
    assert D < 64
    g = _per_row(d["gate"], S) if gated else torch.ones_like(y)
    u = y * d["sc"].double() + d["sh"].double()
    t = (dz * _act_grad(g * u, swish) * u).view(N, S, C)
    dgate = x3d.gate_grad(ycl, sc, sh, dzcl, gate, swish)
    _assert_sum("gate_grad", dgate.cpu(), t.sum(1), t.abs().sum(1), D)
    du0, sums = x3d.gate_bwd_sums(ycl, sc, sh, gate, swish, dzcl)
    assert tuple(sums.shape) == (N, 3, C)
    stored = _rows_of(du0)
    _assert_stored("gate_bwd_sums du0", stored, dz * _act_grad(g * u, swish) * g, extra=8 * U32 * dz.abs() * g.abs())
    assert torch.equal(du0, x3d.gate_act_bwd(ycl, sc, sh, gate, swish, dzcl, None)), "du0 differs from gate_act_bwd(dmean=None)"
    sums = sums.cpu()
    _assert_sum("sums[:, 0]", sums[:, 0], t.sum(1), t.abs().sum(1), D)
    s1, s2 = stored.view(N, S, C), (stored * y).view(N, S, C)
    _assert_sum("sums[:, 1]", sums[:, 1], s1.sum(1), s1.abs().sum(1), D)
    _assert_sum("sums[:, 2]", sums[:, 2], s2.sum(1), s2.abs().sum(1), D)


# ------------------------------------------------------------------------------------------------
def _draw_se(N, C, Cp, F, seed):
    """SE operands with no fc1 pre-activation within 1e-4 of zero (next seed until it holds, at most 3 draws)."""
    for draw in range(MAX_DRAWS):
        g = torch.Generator().manual_seed(seed + draw)
        m = torch.randn((N, Cp), generator=g)
        w1, b1 = torch.randn((F, C), generator=g) / C ** 0.5, torch.randn(F, generator=g) * 0.5
        w2, b2 = torch.randn((C, F), generator=g) / F ** 0.5, torch.randn(C, generator=g) * 0.5
        dgate = torch.randn((N, Cp), generator=g)
        m[:, C:] = 1000.0            # pad channels of the inputs must be ignored
        dgate[:, C:] = 1000.0
        pre1 = m[:, :C].double() @ w1.double().t() + b1.double()
        if float(pre1.abs().min()) >= 1e-4:
            return m, w1, b1, w2, b2, dgate
    raise AssertionError(f"fc1 pre-activation within 1e-4 of zero in {MAX_DRAWS} draws")


def _se_call_fwd(N, C, Cp, F, m, w1, b1, w2, b2, h, gate):
    get_lib().call("sf_se_gate_fwd", N, C, Cp, F, m.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                   h.data_ptr(), gate.data_ptr(), ops._stream(m))


def _se_call_bwd(N, C, Cp, F, gate, h, w1, w2, dgate, dpre2, dpre1, dm):
    get_lib().call("sf_se_gate_bwd", N, C, Cp, F, gate.data_ptr(), h.data_ptr(), w1.data_ptr(), w2.data_ptr(), dgate.data_ptr(),
                   dpre2.data_ptr(), dpre1.data_ptr(), dm.data_ptr(), ops._stream(gate))


def _assert_fp32(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{name}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{name}: max |got - ref| / bound = {worst:.3f}"


def check_se_gate(device, N, C, Cp, F, seed=3):
    """sf_se_gate_fwd / sf_se_gate_bwd against fp64 sigmoid(W2 relu(W1 m + b1) + b2) and its autograd.  Bounds: a dot product of
    length K is within (K + 4) * u32 * (sum|w * x| + |b|); it passes through ReLU unchanged, through sigmoid with slope <= 1/4 plus
    4 * u32 for expf, the addition and the division; an operand that carries a bound of its own contributes sum|w| * bound.  The
    backward kernel is given the forward kernel's gate and h, as in the product, and their bounds are propagated likewise
    (d(g(1-g))/dg <= 1).  Pad channels (C <= c < Cp) of gate, dpre2 and dm are exactly 0 whatever the inputs hold there."""
    m, w1, b1, w2, b2, dgate = _draw_se(N, C, Cp, F, seed)
    md, w1d, b1d, w2d, b2d, dgd = (t.to(device) for t in (m, w1, b1, w2, b2, dgate))
    h = torch.full((N, F), 7.0, device=device)
    gate = torch.full((N, Cp), 7.0, device=device)
    _se_call_fwd(N, C, Cp, F, md, w1d, b1d, w2d, b2d, h, gate)
    # fp64 reference and autograd
    mr = m[:, :C].double().requires_grad_(True)
    W1, B1, W2, B2 = w1.double(), b1.double(), w2.double(), b2.double()
    pre1 = mr @ W1.t() + B1
    hr = pre1.clamp(min=0)
    pre2 = hr @ W2.t() + B2
    gr = torch.sigmoid(pre2)
    dg = dgate[:, :C].double()
    pre1.retain_grad(), pre2.retain_grad()
    (gr * dg).sum().backward()
    with torch.no_grad():
        mabs = m[:, :C].double().abs()
        b_h = (C + 4) * U32 * (mabs @ W1.abs().t() + B1.abs())
        b_pre2 = (F + 4) * U32 * (hr.abs() @ W2.abs().t() + B2.abs()) + b_h @ W2.abs().t()
        b_gate = b_pre2 / 4 + 4 * U32 * gr
        _assert_fp32("se h", h.cpu(), hr, b_h)
        _assert_fp32("se gate", gate.cpu()[:, :C], gr, b_gate)
        assert float(gate.cpu()[:, C:].abs().max() if Cp > C else 0.0) == 0.0, "pad channels of gate"
    dpre2, dm = torch.full((N, Cp), 7.0, device=device), torch.full((N, Cp), 7.0, device=device)
    dpre1 = torch.full((N, F), 7.0, device=device)
    _se_call_bwd(N, C, Cp, F, gate, h, w1d, w2d, dgd, dpre2, dpre1, dm)
    with torch.no_grad():
        b_d2 = dg.abs() * b_gate + 3 * U32 * pre2.grad.abs()
        b_d1 = (C + 4) * U32 * (pre2.grad.abs() @ W2.abs()) + b_d2 @ W2.abs()
        b_dm = (F + 4) * U32 * (pre1.grad.abs() @ W1.abs()) + b_d1 @ W1.abs()
        _assert_fp32("se dpre2", dpre2.cpu()[:, :C], pre2.grad, b_d2)
        _assert_fp32("se dpre1", dpre1.cpu(), pre1.grad, b_d1)
        _assert_fp32("se dm", dm.cpu()[:, :C], mr.grad, b_dm)
        if Cp > C:
            assert float(dpre2.cpu()[:, C:].abs().max()) == 0.0 and float(dm.cpu()[:, C:].abs().max()) == 0.0, "pad channels"


def check_se_limits(device):
    """The SE kernels keep m / h / dpre2 / dpre1 in 1024-entry LDS arrays: Cp = F = 1024 is accepted (SE_CASES), Cp = 1032 or
    F = 1032 is an error with a message, and no output is written."""
    for N, C, Cp, F in ((1, 1000, 1032, 8), (1, 8, 8, 1032)):
        m, w1, b1, w2, b2, dgate = (t.to(device) for t in _draw_se(N, C, Cp, F, 5))
        h, gate = torch.full((N, F), 7.0, device=device), torch.full((N, Cp), 7.0, device=device)
        _expect_error(lambda: _se_call_fwd(N, C, Cp, F, m, w1, b1, w2, b2, h, gate), "<= 1024")
        assert bool((h == 7.0).all()) and bool((gate == 7.0).all())
        gin, hin = torch.rand((N, Cp), device=device), torch.rand((N, F), device=device)
        outs = [torch.full(s, 7.0, device=device) for s in ((N, Cp), (N, F), (N, Cp))]
        _expect_error(lambda: _se_call_bwd(N, C, Cp, F, gin, hin, w1, w2, dgate, *outs), "<= 1024")
        assert all(bool((o == 7.0).all()) for o in outs)


def check_outer_sum(device, N, I, J, with_b, accumulate, lda_extra=0, ldb_extra=0, scale=1.0, seed=4):
    """sf_outer_sum against fp64 scale * a^T b (b = None: a column of ones, J = 1), written or accumulated onto the previous value:
    (N + 2) * u32 * |scale| * sum_n|a b| for the dot product and the scaling, u32 * |result| for the accumulation."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((N, I + lda_extra), generator=g)
    b = torch.randn((N, J + ldb_extra), generator=g) if with_b else None
    assert with_b or J == 1
    prev = torch.randn((I, J), generator=g)
    ad, bd, out = a.to(device), _dev(b, device), prev.clone().to(device)
    get_lib().call("sf_outer_sum", ad.data_ptr(), I + lda_extra, ops._ptr(bd), J + ldb_extra if with_b else 0, N, I, J,
                   out.data_ptr(), float(scale), int(accumulate), ops._stream(ad))
    A = a[:, :I].double()
    B = b[:, :J].double() if with_b else torch.ones((N, 1), dtype=torch.float64)
    ref = scale * (A.t() @ B) + (prev.double() if accumulate else 0)
    bound = (N + 2) * U32 * abs(scale) * (A.abs().t() @ B.abs()) + U32 * ref.abs()
    _assert_fp32("outer_sum", out.cpu(), ref, bound)


def check_bn_apply_sample(device, N, C, S, seed=6):
    """sf_bn_bwd_apply_sample: dy = k1 * (dz + add[n]) + k2 + k3 * y against fp64 with coef = [k1; k2; k3] ([3][C], the layout
    sf_bn_bwd_finalize writes for ops.bn_bwd), one ulp.  The three terms may cancel, and fp32 rounds them by up to
    4 * u32 * T, T = |k1| (|dz| + |add|) + |k2| + |k3 y|: y is drawn so that |dy| >= 2^-10 * T (elements below are moved to
    |dy| ~ 0.125), where that error is an eighth of a 16-bit ulp.  An all-zero sample_add equals sf_bn_bwd_apply value for value;
    rows that are not whole samples are rejected."""
    lib = get_lib()
    M = N * S
    for draw in range(MAX_DRAWS):
        g = torch.Generator().manual_seed(seed + draw)
        y = (torch.randn((M, C), generator=g) * 1.5 + 0.3).to(ACT).double()
        dz = torch.randn((M, C), generator=g).to(ACT).double()
        k1 = (torch.rand(C, generator=g) + 0.5).float()
        k2 = (torch.randn(C, generator=g) * 0.3).float()
        k3 = ((torch.rand(C, generator=g) * 0.5 + 0.2) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)).float()
        add = (torch.randn((N, C), generator=g) * 0.5).float()
        rest = k1.double() * (dz + _per_row(add, S)) + k2.double()
        ref = rest + k3.double() * y
        y = torch.where(ref.abs() < 0.05, ((torch.where(ref < 0, -0.125, 0.125) - rest) / k3.double()).to(ACT).double(), y)
        ref = rest + k3.double() * y
        T = k1.double().abs() * (dz.abs() + _per_row(add, S).abs()) + k2.double().abs() + (k3.double() * y).abs()
        if bool((ref.abs() >= 2.0 ** -10 * T).all()):
            break
    else:
        raise AssertionError(f"no well-conditioned draw in {MAX_DRAWS} seeds")
    ycl, _ = _rows_to_cl(y, N, S, device)
    dzcl, _ = _rows_to_cl(dz, N, S, device)
    coef = torch.stack((k1, k2, k3)).contiguous().to(device)
    s = ops._stream(ycl)

    def apply_sample(addt, rows=M, per=S):
        dy = ops.cl_empty(ycl.shape, device, zero=True)
        lib.call("sf_bn_bwd_apply_sample", rows, C, dzcl.data_ptr(), ops.cl_ld(dzcl), ycl.data_ptr(), ops.cl_ld(ycl),
                 coef.data_ptr(), addt.data_ptr(), per, dy.data_ptr(), ops.cl_ld(dy), s)
        return dy
    _assert_stored("bn_bwd_apply_sample", _rows_of(apply_sample(add.to(device))), ref)
    plain = ops.cl_empty(ycl.shape, device)
    lib.call("sf_bn_bwd_apply", M, C, dzcl.data_ptr(), ops.cl_ld(dzcl), None, 0, ycl.data_ptr(), ops.cl_ld(ycl), None, None, 0,
             coef.data_ptr(), plain.data_ptr(), ops.cl_ld(plain), None, 0, s)
    assert torch.equal(apply_sample(torch.zeros((N, C), device=device)), plain), "zero sample_add != sf_bn_bwd_apply"
    _expect_error(lambda: apply_sample(add.to(device), per=M + 1), "whole samples")


# ------------------------------------------------------------------------------------------------
def _chain_reference(y, dz, N, S, prm, dtype, store):
    """y -> BatchNorm (batch statistics) -> SE gate -> * gate -> Swish, loss = sum(z * dz), in torch ``dtype`` on the CPU; the
    output z and the gradient du into the BatchNorm are rounded to the storage type when ``store`` (the engine stores both)."""
    y = y.to(dtype).clone().requires_grad_(True)
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in prm.items()}
    mean, var = y.mean(0), y.var(0, unbiased=False)
    u = (y - mean) / torch.sqrt(var + 1e-5) * p["gamma"] + p["beta"]
    ul = u.detach().requires_grad_(True)
    m = ul.view(N, S, -1).mean(1)
    pre1 = m @ p["w1"].t() + p["b1"]
    gate = torch.sigmoid(pre1.clamp(min=0) @ p["w2"].t() + p["b2"])
    s = gate.repeat_interleave(S, 0) * ul
    z = s * torch.sigmoid(s)
    (z * dz.to(dtype)).sum().backward()
    du = ul.grad
    du0 = dz.to(dtype) * _act_grad(s.detach().double(), True).to(dtype) * gate.detach().repeat_interleave(S, 0)
    zs = z.detach()
    if store:
        du, zs = du.to(ACT).to(dtype), zs.to(ACT).to(dtype)
    u.backward(du)
    out = {"z": zs, "dy": y.grad, "dgamma": p["gamma"].grad, "dbeta": p["beta"].grad, "dw1": p["w1"].grad, "db1": p["b1"].grad,
           "dw2": p["w2"].grad, "db2": p["b2"].grad}
    aux = {"du": ul.grad.detach(), "du0": du0.detach(), "pre1": pre1.detach(), "mean": mean.detach(), "var": var.detach()}
    return {k: v.detach().double() for k, v in out.items()}, aux


def _chain_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.pow(2).mean().sqrt())


def check_se_chain(device, monkeypatch, N, C_real, S, seed=7):
    """The mini-chain y -> BatchNorm(train) -> SE gate -> * gate -> Swish of an X3D block on the PADDED channel count, built from the
    product wrappers only (BNUnit.finalize = ops.bn_finalize, sample_mean, SE.gate_fwd, gate_act_fwd) and run backward through
    x3d.gate_bn_backward under both schedules (x3d.GATE_ONE_PASS True: sf_gate_bwd_sums + sf_bn_bwd_apply_sample; False:
    sf_gate_grad + sf_gate_act_bwd_bn + sf_bn_bwd_apply; which entry points ran is checked), against fp64 autograd of the same
    chain: z, dy into the BatchNorm, dgamma, dbeta and the four SE gradients.

    The tolerance against fp64 is MEASURED: the yardstick is the same chain in torch fp32 on the CPU with du rounded to the storage
    type where the engine stores it (y is a 16-bit operand already, z is rounded as well); its deviation
    from fp64 is taken per tensor as max|err| / rms(ref), and the engine gets 4 x that because its accumulation order differs.
    Yardstick values measured on the host, max|err| / rms(ref) of the fp32 chain (the host simulator's deviation in brackets):
      fp16 (4, 54, 196): z 2.8e-3 (2.8e-3), dy 2.9e-3 (4.2e-3), dgamma 4.4e-4 (4.4e-4), dbeta 5.7e-4 (6.3e-4), dw1 2.0e-6 (1.7e-6),
                         db1 6.6e-7 (7.5e-7), dw2 6.9e-7 (1.1e-6), db2 3.8e-7 (5.5e-7)
      fp16 (2, 432, 50): z 3.2e-3 (3.2e-3), dy 4.1e-3 (5.0e-3), dgamma 7.8e-4 (1.0e-3), dbeta 7.4e-4 (6.9e-4), dw1 3.3e-6 (4.0e-6),
                         db1 1.0e-6 (1.2e-6), dw2 3.4e-6 (9.8e-6), db2 5.4e-7 (8.0e-7)
      bf16 (4, 54, 196): z 2.2e-2 (2.2e-2), dy 2.6e-2 (4.1e-2), dgamma 3.2e-3 (4.9e-3), dbeta 3.0e-3 (4.5e-3), dw1 1.4e-6 (3.1e-6),
                         db1 5.2e-7 (1.4e-6), dw2 1.6e-6 (1.8e-6), db2 5.3e-7 (4.0e-7)
      bf16 (2, 432, 50): z 2.4e-2 (2.4e-2), dy 2.8e-2 (3.2e-2), dgamma 6.6e-3 (6.3e-3), dbeta 5.7e-3 (5.7e-3), dw1 4.0e-6 (4.9e-6),
                         db1 1.1e-6 (1.0e-6), dw2 2.7e-6 (1.1e-5), db2 6.5e-7 (1.0e-6)
    (dw2 of the 432-channel case is the closest: 2.9 x / 3.9 x its yardstick on the host simulator, whose u = y * scale + shift is
    not contracted into one fused multiply-add.)

    The two schedules differ by where du is rounded to 16 bits (du0, the squeeze term added back in fp32, against du0 + dmean / S):
    with k1 = gamma * rstd, |dy_A - dy_B| <= k1 * u16 * (|du0| + |du|) (the two roundings) + 2 * u16 * |dy| + tiny (the stores of dy)
    + k1 * 2 * u16 * (mean|du| + |xhat| * mean|du * xhat|) (the per-channel sums of the rounded gradients behind k2 and k3) -- "one
    ulp" of the 16-bit gradient, propagated.  Pad channels of dy are exactly 0."""
    from torch import nn
    Cp = (C_real + 7) // 8 * 8
    M = N * S
    se = x3d.SE(C_real, 0.0625)
    F = se.dim_fc
    for draw in range(MAX_DRAWS):
        g = torch.Generator().manual_seed(seed + draw)
        y = (torch.randn((M, Cp), generator=g) * 1.5 + 0.3).to(ACT).double()
        dz = torch.randn((M, Cp), generator=g).to(ACT).double()
        y[:, C_real:] = 0
        dz[:, C_real:] = 0
        prm = {"gamma": torch.rand(C_real, generator=g) + 0.5, "beta": torch.randn(C_real, generator=g) * 0.2,
               "w1": torch.randn((F, C_real), generator=g) / C_real ** 0.5, "b1": torch.randn(F, generator=g) * 0.5,
               "w2": torch.randn((C_real, F), generator=g) / F ** 0.5, "b2": torch.randn(C_real, generator=g) * 0.5}
        ref, aux = _chain_reference(y[:, :C_real], dz[:, :C_real], N, S, prm, torch.float64, False)
        if float(aux["pre1"].abs().min()) >= 1e-4:
            break
    else:
        raise AssertionError(f"fc1 pre-activation within 1e-4 of zero in {MAX_DRAWS} draws")
    yard, _ = _chain_reference(y[:, :C_real], dz[:, :C_real], N, S, prm, torch.float32, True)
    tol = {k: 4 * _chain_err(yard[k], ref[k]) for k in ref}

    bn = nn.BatchNorm3d(C_real)
    with torch.no_grad():
        bn.weight.copy_(prm["gamma"]), bn.bias.copy_(prm["beta"])
        se.fc1.weight.copy_(prm["w1"].view_as(se.fc1.weight)), se.fc1.bias.copy_(prm["b1"])
        se.fc2.weight.copy_(prm["w2"].view_as(se.fc2.weight)), se.fc2.bias.copy_(prm["b2"])
    bn, se = bn.to(device).train(), se.to(device).train()
    unit = x3d.BNUnit(bn)
    ycl, _ = _rows_to_cl(y, N, S, device)
    dzcl, _ = _rows_to_cl(dz, N, S, device)
    part = torch.stack((y.sum(0), (y * y).sum(0))).float().view(1, 2, Cp).to(device)
    st = unit.finalize(part, M, Cp, True)
    m = x3d.sample_mean(ycl, st.scale, st.shift, relu=False)
    h, gate = se.gate_fwd(m)
    z = x3d.gate_act_fwd(ycl, st.scale, st.shift, gate, True)
    zr = _rows_of(z)
    assert float(zr[:, C_real:].abs().max() if Cp > C_real else 0.0) == 0.0, "pad channels of z"
    ysum = y.view(N, S, Cp).sum(1).float().to(device)
    t = types.SimpleNamespace(_se=se, _b_bn=unit, _swish_inner=True)
    params = {"dgamma": bn.weight, "dbeta": bn.bias, "dw1": se.fc1.weight, "db1": se.fc1.bias, "dw2": se.fc2.weight,
              "db2": se.fc2.bias}
    dys = {}
    for one_pass in (True, False):
        monkeypatch.setattr(x3d, "GATE_ONE_PASS", one_pass)
        for p in params.values():
            p.grad = None
        seen = []
        _sflib.set_call_observer(lambda name, thunk, work: (seen.append(name), thunk())[1])
        try:
            dy = x3d.gate_bn_backward(t, ycl, st, gate, (m, h), ysum, dzcl)
        finally:
            _sflib.set_call_observer(None)
        if one_pass:
            assert "sf_gate_bwd_sums" in seen and "sf_bn_bwd_apply_sample" in seen and "sf_gate_grad" not in seen, seen
        else:
            assert "sf_gate_grad" in seen and "sf_gate_act_bwd_bn" in seen and "sf_gate_bwd_sums" not in seen, seen
        dyr = _rows_of(dy)
        if Cp > C_real:
            assert float(dyr[:, C_real:].abs().max()) == 0.0, "pad channels of dy"
        dys[one_pass] = dyr[:, :C_real]
        got = {k: p.grad.detach().cpu().double().reshape(ref[k].shape) for k, p in params.items()}
        got["dy"], got["z"] = dys[one_pass], zr[:, :C_real]
        for k in ref:
            e = _chain_err(got[k], ref[k])
            print(f"se_chain one_pass={one_pass} {k}: engine {e:.3e}, yardstick {tol[k] / 4:.3e}")
        for k in ref:
            e = _chain_err(got[k], ref[k])
            assert e <= tol[k], f"one_pass={one_pass} {k}: max|err| / rms(ref) = {e:.3e} > 4 x yardstick {tol[k] / 4:.3e}"
    k1 = (prm["gamma"].double() / torch.sqrt(aux["var"] + 1e-5)).abs()
    xhat = (y[:, :C_real] - aux["mean"]) / torch.sqrt(aux["var"] + 1e-5)
    du, du0 = aux["du"].double(), aux["du0"].double()
    bound = (k1 * U16 * (du0.abs() + du.abs()) + F16_EPS * ref["dy"].abs() + TINY
             + k1 * F16_EPS * (du.abs().mean(0) + xhat.abs() * (du * xhat).abs().mean(0)))
    worst = float(((dys[True] - dys[False]).abs() / bound).max())
    print(f"se_chain schedules: max |dy_A - dy_B| / bound = {worst:.3f}")
    assert worst <= 1.0, f"the two backward schedules differ by {worst:.3f} x the propagated 16-bit ulp"
