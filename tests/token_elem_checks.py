"""Per-element parity checks of the token-space kernels (csrc/sf_tokens.h and their launchers in sf_api.hip: LayerNorm, column
sums and their finalizes, GELU, the pooled-attention softmax, the rel-pos gather / scatter / pack / unpack, transpose_heads,
row_scale_add), shared by tests/test_token_elem_hostsim.py and the -m gpu file tests/test_token_elem_gpu.py.

Method and notation of tests/x3d_checks.py: the reference is torch float64 on the CPU evaluated on exactly the operands the kernel
sees (activations already rounded to the storage type, fp32 parameters as they are); every comparison is PER ELEMENT, no element is
excluded; u16 = lib.act_eps(), u32 = 2^-24, TINY = the smallest subnormal of the storage type.

* stored 16-bit outputs: |got - ref| <= 2 u16 |ref| + TINY + E32, with E32 the fp32 evaluation error of the kernel's own expression
  computed from the operands in fp64 -- u32 |term| per rounded fp32 operation, 8 u32 x magnitude for an expression that holds
  expf / erff / a reciprocal / sqrtf.  Each check states its E32.
* fp32 sums: |got - ref| <= D u32 sum|term| with D the longest chain of fp32 additions read off the code (rows per thread + the LDS
  fold / workgroup reduction + 2; the finalizes run in double and add one rounding).  ``ln_bwd_plan`` / ``colsum_plan`` restate the
  launchers' tiling, and the block count they predict is compared with what the library reports.
* sums of stored values (layernorm_bwd sums=): the terms are the kernel's OWN stored dx, read back.
* data movement (rel-pos pack / unpack / gather / scatter, transpose_heads, zero-scale rows, pad columns) is bit-exact.
* every pitched input holds NaN in its padding; outputs are pre-filled with NaN (or a sentinel that must survive outside the
  written region).
"""
import math

import torch

from slowfast_amd import tokens
from slowfast_amd.lib import get_lib
from tests.kernel_checks import ACT
from tests.x3d_checks import TINY, U16, U32, _assert_fp32, _assert_sum, _expect_error

SQRT1_2 = 0.70710678118654752
NAN = float("nan")

# LayerNorm widths on the template boundaries of layernorm_fwd_impl / layernorm_bwd_impl
LN_WIDTHS = [8, 96, 128, 136, 256, 264, 384, 512, 520, 768, 776, 1024]
LN_GRID_STRIDE = (2048 * 32 + 5, 8)             # more than SF_LN_FWD_BLOCKS = 2048 workgroups of 32 rows
LN_BWD_TWO_PASSES = (2 * 12288 + 3, 8)          # 768 workgroups of 48 rows: two trips of the 32-row loop
COLSUM_WIDTHS = [8, 56, 2048, 2056]
# rows per thread 1 .. 9 of sf_colsum_kernel: `passes` rows in a full workgroup, `last` / `last - 1` in the ragged last one
COLSUM_PASSES = [(3, 2), (6, 5), (9, 8)]
FIN_NBLK = [1, 256, 257, 2048, 2049, 5000]
# (id, B, heads, cls, q_thw, k_thw, lds_extra, with_rq)
SOFTMAX_CASES = [
    ("nsm1_13keys", 2, 3, 1, (1, 2, 3), (2, 2, 3), 0, True),
    ("nsm1_pad8", 2, 3, 1, (1, 2, 3), (2, 2, 3), 8, True),          # lds = roundup(Nk, 8) + 8
    ("nsm2", 1, 2, 1, (1, 3, 2), (3, 13, 14), 0, True),             # Nk = 547 -> lds = 552
    ("nsm2_pad8", 1, 2, 1, (1, 3, 2), (3, 13, 14), 8, True),
    ("nsm4", 1, 2, 1, (1, 2, 3), (2, 17, 31), 0, True),             # Nk = 1055 -> lds = 1056
    ("nsm4_pad8", 1, 1, 1, (1, 1, 5), (2, 17, 31), 8, True),        # rows = 6: not a multiple of 4
    ("R64", 1, 1, 1, (1, 1, 3), (2, 31, 31), 0, True),              # kH + kW + kT = 64, lds = 1928
    ("Nk2", 1, 2, 1, (1, 3, 3), (1, 1, 1), 0, True),
    ("no_rq", 2, 2, 1, (1, 2, 3), (2, 2, 3), 0, False),
    ("no_cls", 2, 3, 0, (1, 2, 3), (2, 3, 5), 0, True),
    ("grid_stride", 1, 4, 1, (1, 128, 128), (1, 1, 1), 0, True),    # rows = 65540 > 4 * 16384
]
# (id, B, heads, cls, q_thw, k_thw, pitch): pitch <= 256 takes the LDS kernels, above the global ones
RELPOS_CASES = [
    ("lds_33rows", 1, 3, 1, (1, 2, 5), (2, 3, 4), 64),              # 33 rows: a ragged 32-row chunk
    ("global_33rows", 1, 3, 1, (1, 2, 5), (2, 3, 4), 264),
    ("no_cls", 2, 2, 0, (2, 3, 4), (1, 5, 2), 64),
    ("no_cls_global", 2, 2, 0, (2, 3, 4), (1, 5, 2), 264),
    ("grid_stride", 1, 2, 1, (2, 256, 256), (1, 1, 2), 8),          # 262146 rows = 8193 chunks > 8192 workgroups
]


def _h(x, device):
    return x.to(ACT).to(device)


def _f64(t):
    return t.detach().cpu().double()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pitched(x, device, extra):
    """[M, C] values of the storage type -> (view, base): the view of a [M, C + extra] tensor whose padding holds NaN."""
    M, C = x.shape
    base = torch.full((M, C + extra), NAN, dtype=ACT, device=device)
    base[:, :C] = _h(x, device)
    return base[:, :C], base


def _randn16(shape, g, std=1.0, mean=0.0):
    return (torch.randn(shape, generator=g) * std + mean).to(ACT).double()


def _assert_stored(name, got, ref, e32):
    bound = 2 * U16 * ref.abs() + TINY + e32
    err = (got - ref).abs()
    ratio = err / bound
    worst = float(ratio.max())
    print(f"{name}: max err / bound = {worst:.3f}")
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    assert worst <= 1.0, f"{name}: max |got - ref| / bound = {worst:.3f} at flat index {int(ratio.argmax())}"


# ------------------------------------------------------------------------------------------------
# LayerNorm
def ln_template(C, fwd):
    """(L, NS, RU) of the kernel the launchers pick for width C."""
    if fwd and C == 768:
        return 32, 3, 2
    if C <= 128:
        return 16, 1, 2
    if C <= 256:
        return 32, 1, 2
    if C <= 512:
        return 64, 1, 2
    return 64, 2, 1


def ln_rows_per_pass(C):
    L, _, RU = ln_template(C, True)
    return 256 // L * RU


def ln_bwd_plan(M, C):
    """ln_bwd_plan of sf_api.hip: (workgroups, rows per workgroup, rows per thread)."""
    L, _, RU = ln_template(C, False)
    rpb = 256 // L
    max_blocks = 768 if C <= 512 else 1024
    blocks = min(-(-M // rpb), max_blocks)
    rows_per_block = -(-(-(-M // blocks)) // rpb) * rpb
    trips = -(-rows_per_block // (rpb * RU))
    return -(-M // rows_per_block), rows_per_block, trips * RU


def _ln_operands(M, C, seed, hard=False):
    g = torch.Generator().manual_seed(seed)
    x = _randn16((M, C), g, 1.3, 0.2)
    if hard and M >= 3:
        x[0] = float(torch.tensor(1.7).to(ACT))                     # constant row: variance 0
        x[1] = _randn16((C,), g, 0.05, 30.0)                        # |mean| ~ 30, standard deviation ~ 0.05
        x[2] = _randn16((C,), g, 0.05, -30.0)
    sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    gamma = ((torch.rand(C, generator=g) + 0.5) * sign).float()
    beta = (torch.randn(C, generator=g) * 0.2).float()
    return g, x, gamma, beta


def _ln_stats(x, eps):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return mu, var, 1.0 / torch.sqrt(var + eps)


def check_layernorm_fwd(device, M, C, ld_extra=0, save_stats=True, hard=False, seed=0, eps=1e-6):
    """sf_layernorm_fwd against fp64 (x - mean) * rstd * gamma + beta with the two-pass variance.
    E32 = 8 u32 (|xh gamma| + |beta|) + 8 u32 (|x| + |mean|) rstd |gamma|: the first term covers sqrtf, the reciprocal, the two
    products and the sum; the second the rounding of the fp32 mean and of x - mean, amplified by rstd * gamma (what a row of
    mean 30 and deviation 0.05 is about).  mean: (log2(C) + 4) u32 mean|x|.  rstd, on every row: relative
    (Dv / 2 + 8) u32 + em^2 rstd^2 / 2 with Dv = 8 NS + log2(L) + 6 (the squares carry 3 roundings, the register and shuffle sum
    8 NS + log2(L), 1 / C and + eps three more; halved by the square root, 8 for sqrtf and the reciprocal) and em the bound on
    the mean (a shifted mean changes the variance by its square only)."""
    _, x, gamma, beta = _ln_operands(M, C, seed, hard)
    xd, xbase = _pitched(x, device, ld_extra)
    ybase = torch.full((M, C + ld_extra), NAN, dtype=ACT, device=device)
    y, mean, rstd = tokens.layernorm_fwd(xd, gamma.to(device), beta.to(device), eps, out=ybase[:, :C], save_stats=save_stats)
    assert (mean is None) == (not save_stats) and (rstd is None) == (not save_stats)
    mu, var, rs = _ln_stats(x, eps)
    xh = (x - mu) * rs
    gd, bd = gamma.double(), beta.double()
    ref = xh * gd + bd
    e32 = 8 * U32 * ((xh * gd).abs() + bd.abs()) + 8 * U32 * (x.abs() + mu.abs()) * rs * gd.abs()
    _assert_stored(f"ln fwd C={C} M={M}", _f64(ybase[:, :C]), ref, e32)
    if ld_extra:
        assert bool(torch.isnan(ybase[:, C:]).all()), "ln fwd wrote into the pitch padding"
    if save_stats:
        L, NS, _ = ln_template(C, True)
        em = (math.log2(C) + 4) * U32 * x.abs().mean(1)
        _assert_fp32(f"ln mean C={C}", mean.cpu(), mu[:, 0], em)
        Dv = 8 * NS + math.log2(L) + 6
        rsr = rs[:, 0]
        _assert_fp32(f"ln rstd C={C}", rstd.cpu(), rsr, rsr * ((Dv / 2 + 8) * U32 + 0.5 * em ** 2 * rsr ** 2))


def check_layernorm_rejects(device):
    """C = 12 (not a multiple of 8) and C = 1032 (> 1024) are errors with a message, forward and backward."""
    lib = get_lib()
    for C in (12, 1032):
        x = torch.zeros((4, C), dtype=ACT, device=device)
        w = torch.ones(C, device=device)
        st = torch.ones(4, device=device)
        part = torch.zeros((4, 4, C), device=device)
        args = (4, C, x.data_ptr(), C, w.data_ptr(), w.data_ptr(), 1e-6, x.data_ptr(), C, None, None, None)
        _expect_error(lambda: lib.call("sf_layernorm_fwd", *args), "multiple of 8, <= 1024")
        _expect_error(lambda: lib.call("sf_layernorm_bwd_blocks", 4, C), "multiple of 8, <= 1024")
        _expect_error(lambda: lib.call("sf_layernorm_bwd", 4, C, x.data_ptr(), C, x.data_ptr(), C, w.data_ptr(), st.data_ptr(),
                                       st.data_ptr(), None, 0, x.data_ptr(), C, part.data_ptr(), None), "multiple of 8, <= 1024")


def check_layernorm_bwd(device, M, C, resid=True, ld_extra=0, accumulate=False, sums=None, seed=1, eps=1e-6):
    """sf_layernorm_bwd / sf_layernorm_bwd_sums against fp64 dx = rstd (g - mean_c(g) - xh mean_c(g xh)) + resid, g = dy gamma,
    xh = (x - mean) rstd, with mean / rstd the fp32 vectors the kernel is handed.  From the kernel's expression
    (xh: 2 roundings, g: 1, the row sums s1 / s2: Ds = 8 NS + log2(L) + 6 with the term products and 1 / C):
      E32 = rstd (4 u32 (|g| + |s1| + |xh s2|) + Ds u32 (mean|g| + |xh| mean|g xh|)) + 2 u32 (|rstd t| + |resid|),
    t the bracket.  dgamma / dbeta: D u32 sum|term| with D = rows per thread (ln_bwd_plan) + RPB (the LDS fold) + 2, + 3 for
    the rounded dy * xh of dgamma, + 1 when accumulated onto an earlier value; the block count of the plan is asserted.
    ``sums`` = (accumulate_resid | None, accumulate_dx | None): the column sums of resid and of the kernel's own STORED dx,
    read back, under the same D; dx is bit-equal with and without them.  With ``ld_extra`` dy, x and resid are pitched
    (NaN padding) and dx lands in a slice of a wider NaN tensor."""
    g, x, gamma, _ = _ln_operands(M, C, seed)
    dy = _randn16((M, C), g)
    res = _randn16((M, C), g) if resid else None
    mu, _, rs = _ln_stats(x, eps)
    mean32, rstd32 = mu[:, 0].float(), rs[:, 0].float()
    mu, rs = mean32.double()[:, None], rstd32.double()[:, None]
    L, NS, _ = ln_template(C, False)
    nblk, rows_per_block, per_thread = ln_bwd_plan(M, C)
    assert get_lib().call("sf_layernorm_bwd_blocks", M, C) == nblk
    D = per_thread + 256 // L + 2
    Ds = 8 * NS + math.log2(L) + 6
    gd = gamma.double()
    xh = (x - mu) * rs
    gg = dy * gd
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    t = gg - s1 - xh * s2
    r = res if resid else torch.zeros_like(x)
    ref = rs * t + r
    e32 = (rs * (4 * U32 * (gg.abs() + s1.abs() + (xh * s2).abs())
                 + Ds * U32 * (gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True)))
           + 2 * U32 * ((rs * t).abs() + r.abs()))

    xd, _ = _pitched(x, device, ld_extra)
    dyd, _ = _pitched(dy, device, ld_extra)
    rd = _pitched(res, device, ld_extra)[0] if resid else None
    gam, m32, r32 = gamma.to(device), mean32.to(device), rstd32.to(device)
    prev_g, prev_b = torch.randn(C, generator=g), torch.randn(C, generator=g)

    def run(sums_arg):
        obase = torch.full((M, C + ld_extra), NAN, dtype=ACT, device=device)
        dg, db = prev_g.clone().to(device), prev_b.clone().to(device)
        if not accumulate:
            dg.fill_(NAN), db.fill_(NAN)
        tokens.layernorm_bwd(dyd, xd, gam, m32, r32, dg, db, resid=rd, accumulate=accumulate, out=obase[:, :C], sums=sums_arg)
        return obase, dg, db

    obase, dg, db = run(None)
    tag = f"C={C} M={M}"
    _assert_stored(f"ln bwd dx {tag}", _f64(obase[:, :C]), ref, e32)
    if ld_extra:
        assert bool(torch.isnan(obase[:, C:]).all()), "ln bwd wrote into the pitch padding"
    pg, pb = (prev_g.double(), prev_b.double()) if accumulate else (0.0, 0.0)
    pga, pba = (prev_g.abs().double(), prev_b.abs().double()) if accumulate else (0.0, 0.0)
    acc = int(accumulate)
    _assert_sum(f"ln dgamma {tag}", dg.cpu(), (dy * xh).sum(0) + pg, (dy * xh).abs().sum(0) + pga, D + 3 + acc)
    _assert_sum(f"ln dbeta {tag}", db.cpu(), dy.sum(0) + pb, dy.abs().sum(0) + pba, D + acc)
    if sums is None:
        return
    acc_r, acc_x = sums
    prev_r, prev_x = torch.randn(C, generator=g), torch.randn(C, generator=g)
    sr = None if acc_r is None else (prev_r.clone() if acc_r else torch.full((C,), NAN)).to(device)
    sx = None if acc_x is None else (prev_x.clone() if acc_x else torch.full((C,), NAN)).to(device)
    obase2, dg2, db2 = run((None if sr is None else (sr, acc_r), None if sx is None else (sx, acc_x)))
    assert torch.equal(_bits(obase2[:, :C]), _bits(obase[:, :C])), "the extra column sums changed the stored dx"
    assert torch.equal(dg2, dg) and torch.equal(db2, db)
    stored = _f64(obase2[:, :C])
    if sr is not None:
        p = prev_r.double() if acc_r else 0.0
        pa = prev_r.abs().double() if acc_r else 0.0
        _assert_sum(f"ln sum resid {tag}", sr.cpu(), res.sum(0) + p, res.abs().sum(0) + pa, D + int(acc_r))
    if sx is not None:
        p = prev_x.double() if acc_x else 0.0
        pa = prev_x.abs().double() if acc_x else 0.0
        _assert_sum(f"ln sum of the stored dx {tag}", sx.cpu(), stored.sum(0) + p, stored.abs().sum(0) + pa, D + int(acc_x))


# ------------------------------------------------------------------------------------------------
# column sums and their finalizes
def colsum_plan(M, C):
    """make_rowtile(M, C, 1024) and rowtile_reduce_store: (workgroups, rows per thread, depth of the workgroup reduction) --
    a butterfly over the 64 / TG lanes that share a channel group plus two levels over the four waves when TG < 64 is a power
    of two, else rpi - 1 additions in a row."""
    G = C // 8
    TG = min(G, 256)
    rpi = 256 // TG
    passes = max(1, -(-M // (rpi * 1024)))
    depth = int(math.log2(64 // TG)) + 2 if TG < 64 and TG & (TG - 1) == 0 else rpi - 1
    return -(-M // (rpi * passes)), passes, depth, rpi


def check_bias_grad(device, M, C, fold=None, accumulate=False, ld_extra=0, seed=2):
    """tokens.bias_grad (sf_colsum + sf_colsum_finalize) against the fp64 column sums (folded over the C / fold channel copies):
    D u32 sum|x| with D = rows per thread + reduction depth + 2 (+ 1 accumulated); the block count of colsum_plan is asserted."""
    g = torch.Generator().manual_seed(seed)
    x = _randn16((M, C), g)
    nblk, passes, depth, _ = colsum_plan(M, C)
    assert get_lib().call("sf_colsum_blocks", M, C) == nblk
    xd, _ = _pitched(x, device, ld_extra)
    F = fold or C
    prev = torch.randn(F, generator=g)
    out = (prev.clone() if accumulate else torch.full((F,), NAN)).to(device)
    tokens.bias_grad(xd, out, accumulate=accumulate, fold=fold)
    ref, asum = x.sum(0).view(-1, F).sum(0), x.abs().sum(0).view(-1, F).sum(0)
    if accumulate:
        ref, asum = ref + prev.double(), asum + prev.abs().double()
    _assert_sum(f"bias_grad M={M} C={C} passes={passes}", out.cpu(), ref, asum, passes + depth + 2 + int(accumulate))


def colsum_rows_for(C, passes, last):
    """The row count at which a full workgroup gives every thread ``passes`` rows and the ragged last one ``last`` / ``last - 1``."""
    rpi = colsum_plan(8, C)[3]
    M = rpi * 1024 * (passes - 1) + rpi * (passes - 1) + 1            # just above (passes - 1) * rpi * 1024 rows
    full = M // (rpi * passes)
    M = full * rpi * passes + rpi * (last - 1) + max(1, rpi // 2)
    assert colsum_plan(M, C)[1] == passes
    return M


def _fin_reference(part, C, F, scale, which):
    col = part[:, which, :].double()
    return scale * col.sum(0).view(-1, F).sum(0), abs(scale) * col.abs().sum(0).view(-1, F).sum(0)


def check_colsum_finalize(device, nblk, C=40, fold=None, scale=1.0, accumulate=False, row_stride=1, outs=(True, True), seed=3):
    """tokens.colsum_finalize on a synthetic fp32 table [nblk][2 * row_stride][C]: the sums run in double, so the result carries
    the rounding of the stored value (+ one per folded group above kFoldAbove = 2048 rows, + one accumulated): D = 2, 3, 4."""
    g = torch.Generator().manual_seed(seed)
    F = fold or C
    table = torch.randn((nblk, 2 * row_stride, C), generator=g)
    td = table.clone().to(device)
    prev = [torch.randn(F, generator=g), torch.randn(F, generator=g)]
    out = [((prev[i].clone() if accumulate else torch.full((F,), NAN)).to(device) if outs[i] else None) for i in (0, 1)]
    tokens.colsum_finalize(td[:, 0:2], C, F, out[0], out[1], scale, accumulate, row_stride=row_stride)
    D = 2 + int(nblk > 2048) + int(accumulate)
    for i in (0, 1):
        if out[i] is None:
            continue
        ref, asum = _fin_reference(table, C, F, scale, i)
        if accumulate:
            ref, asum = ref + prev[i].double(), asum + prev[i].abs().double()
        _assert_sum(f"colsum_finalize nblk={nblk} out{i}", out[i].cpu(), ref, asum, D)


def check_finalize_batch(device, seed=4):
    """17 finalizes in one sf_colsum_finalize_batch call (two launches): short and long tables, different C / fold, a row
    stride, one output only, accumulation, scales; an item of 2049 rows is rejected."""
    g = torch.Generator().manual_seed(seed)
    items, want = [], []
    for i in range(17):
        nblk = (1, 300, 7, 256, 257, 2048, 33)[i % 7]
        C, F = ((8, 8), (40, 40), (128, 32), (24, 8), (72, 72))[i % 5]
        stride = 2 if i % 4 == 1 else 1
        scale = (1.0, 0.5, -2.0)[i % 3]
        accumulate = i % 3 == 2
        table = torch.randn((nblk, 2 * stride, C), generator=g)
        prev = [torch.randn(F, generator=g), torch.randn(F, generator=g)]
        use = ((True, True), (True, False), (False, True))[i % 3]
        out = [((prev[k].clone() if accumulate else torch.full((F,), NAN)).to(device) if use[k] else None) for k in (0, 1)]
        td = table.to(device)
        items.append((td[:, 0:2], C, F, out[0], out[1], scale, accumulate, stride, None))
        want.append((table, C, F, scale, accumulate, prev, out))
    tokens._finalize_batch(items)
    for i, (table, C, F, scale, accumulate, prev, out) in enumerate(want):
        for k in (0, 1):
            if out[k] is None:
                continue
            ref, asum = _fin_reference(table, C, F, scale, k)
            if accumulate:
                ref, asum = ref + prev[k].double(), asum + prev[k].abs().double()
            _assert_sum(f"finalize_batch item {i} out{k}", out[k].cpu(), ref, asum, 2 + int(accumulate))
    long = torch.zeros((2049, 2, 8), device=device)
    o = torch.zeros(8, device=device)
    _expect_error(lambda: tokens._finalize_batch([(long, 8, 8, o, None, 1.0, False, 1, None)]), "2049 partial rows")


def check_deferred_finalizes(device, seed=5):
    """Two finalizes into the same output inside one deferred_finalizes() context (overwrite, then accumulate), and an immediate
    long-table finalize into an output a pending one writes: the result equals the eager order bit for bit."""
    g = torch.Generator().manual_seed(seed)
    C = 40
    for n_second in (5, 2049):
        a = torch.randn((7, 2, C), generator=g).to(device)
        b = torch.randn((n_second, 2, C), generator=g).to(device)
        assert tokens._pending_fin is None
        eager0, eager1 = torch.full((C,), NAN, device=device), torch.full((C,), NAN, device=device)
        tokens.colsum_finalize(a.clone(), C, C, eager0, eager1, 1.0, False)
        tokens.colsum_finalize(b.clone(), C, C, eager0, None, 0.5, True)
        d0, d1 = torch.full((C,), NAN, device=device), torch.full((C,), NAN, device=device)
        with tokens.deferred_finalizes():
            tokens.colsum_finalize(a.clone(), C, C, d0, d1, 1.0, False)
            assert tokens._pending_fin is not None and len(tokens._pending_fin) == 1
            tokens.colsum_finalize(b.clone(), C, C, d0, None, 0.5, True)
        assert tokens._pending_fin is None
        assert torch.equal(_bits(d0), _bits(eager0)) and torch.equal(_bits(d1), _bits(eager1)), f"deferred != eager ({n_second})"
        ref = a[:, 0].double().sum(0).cpu() + 0.5 * b[:, 0].double().sum(0).cpu()
        asum = a[:, 0].double().abs().sum(0).cpu() + 0.5 * b[:, 0].double().abs().sum(0).cpu()
        _assert_sum(f"deferred finalizes ({n_second} rows)", d0.cpu(), ref, asum, 4)


# ------------------------------------------------------------------------------------------------
# GELU
_GELU_CACHE = {}


def gelu_all_values():
    """Every finite value of the storage type (63488 fp16 / 65280 bf16 patterns), zero-padded to the full 65536-entry table."""
    if "x" not in _GELU_CACHE:
        v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(ACT)
        v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
        n = int(torch.isfinite(torch.arange(65536, dtype=torch.int32).to(torch.int16).view(ACT)).sum())
        assert n == (63488 if ACT == torch.float16 else 65280) and v.numel() % 8 == 0
        x = v.double()
        cdf = 0.5 * torch.special.erfc(-x * SQRT1_2)
        _GELU_CACHE.update(x16=v, x=x, fwd=x * cdf, dfn=cdf + x * torch.exp(-0.5 * x * x) * 0.3989422804014327)
    return _GELU_CACHE


def check_gelu_exhaustive(device, seed=6):
    """sf_gelu_fwd / sf_gelu_bwd on every finite value of the storage type.  Forward against 0.5 x erfc(-x / sqrt 2):
    E32 = 2 u32 |x|, the cancellation of 1 + erff in the negative tail (the kernel keeps the reference's 0.5 x (1 + erf)).
    Backward with random da and with da = +-1 against da (Phi(x) + x phi(x)): E32 = 4 u32 |da|."""
    c = gelu_all_values()
    xd = c["x16"].to(device)
    _assert_stored("gelu fwd, all values", _f64(tokens.gelu_fwd(xd)), c["fwd"], 2 * U32 * c["x"].abs())
    g = torch.Generator().manual_seed(seed)
    ones = torch.where(torch.rand(65536, generator=g) < 0.5, -1.0, 1.0).double()
    for name, da in (("random da", _randn16((65536,), g)), ("da = +-1", ones)):
        got = _f64(tokens.gelu_bwd(xd, _h(da, device)))
        _assert_stored(f"gelu bwd, all values, {name}", got, da * c["dfn"], 4 * U32 * da.abs())


def check_gelu_small_and_rejects(device):
    """n = 8 (one thread), and n = 12 is an error."""
    c = gelu_all_values()
    idx = torch.tensor([0x3C00, 0xBC00, 0x0001, 0x8001, 0x4580, 0xC580, 0x3800, 0xB800], dtype=torch.int64)    # fp16: +-1, +-5.5 ...
    xd = c["x16"][idx].to(device)
    _assert_stored("gelu fwd n=8", _f64(tokens.gelu_fwd(xd)), c["fwd"][idx], 2 * U32 * c["x"][idx].abs())
    da = torch.ones(8, dtype=torch.float64)
    _assert_stored("gelu bwd n=8", _f64(tokens.gelu_bwd(xd, _h(da, device))), c["dfn"][idx], 4 * U32 * da)
    bad = torch.zeros(12, dtype=ACT, device=device)
    _expect_error(lambda: tokens.gelu_fwd(bad), "bad arguments")
    _expect_error(lambda: tokens.gelu_bwd(bad, bad), "bad arguments")


GELU_GRID_CAP = 65536          # pool_grid() of sf_api.hip: at most 65536 workgroups of 256 threads x 8 elements


def check_gelu_grid_stride(device):
    """n above the grid cap (65536 workgroups x 256 threads x 8 elements) runs the stride loop: the table of all values repeated
    2049 times; the kernels are element-wise, so every repeat must equal the one-table result bit for bit (which
    check_gelu_exhaustive compares with fp64)."""
    c = gelu_all_values()
    reps = GELU_GRID_CAP * 256 * 8 // 65536 + 1
    assert reps * 65536 > GELU_GRID_CAP * 256 * 8
    small = c["x16"].to(device)
    da_small = _h(torch.linspace(-2, 2, 65536, dtype=torch.float64), device)
    f_small, b_small = tokens.gelu_fwd(small), tokens.gelu_bwd(small, da_small)
    big = small.repeat(reps)
    out = tokens.gelu_fwd(big)
    assert torch.equal(out.view(reps, 65536).view(torch.int16), f_small.view(torch.int16).expand(reps, 65536)), "gelu fwd stride loop"
    out = tokens.gelu_bwd(big, da_small.repeat(reps))
    assert torch.equal(out.view(reps, 65536).view(torch.int16), b_small.view(torch.int16).expand(reps, 65536)), "gelu bwd stride loop"


# ------------------------------------------------------------------------------------------------
# softmax of pooled attention with the decomposed rel-pos bias
def _key_coords(cls, k_thw):
    kT, kH, kW = k_thw
    pos = torch.arange(kT * kH * kW)
    return pos // (kH * kW), (pos // kW) % kH, pos % kW


def check_softmax(device, B, heads, cls, q_thw, k_thw, lds_extra=0, with_rq=True, seed=7):
    """sf_softmax_fwd, then sf_softmax_bwd on the forward's STORED probabilities.
    Forward against fp64 softmax_k(scale S + bias), bias = rq[kh] + rq[kH + kw] + rq[kH + kW + kt] for non-cls queries and keys:
      E32 = P u32 (4 sum|score terms| + 4 |x - max| + 4 |max| + 8 + 2 log2(Nk));
    the columns [Nk, lds) hold NaN on entry and exactly 0 afterwards.  Scores are drawn at scale 6 (rows span many orders of
    magnitude) and row 1 has one dominant key: every other probability underflows to 0.
    Backward against fp64 scale P (dP - sum_k P dP) with NaN in the pad of dP and of P:
      E32 = scale P (16 u32 sum_k|P dP| + 2 u32 (|dP| + |dot|))   (8 register adds, 6 shuffle steps, 2).
    drq: sums of the unscaled dS over the keys that share kh | kw | kt, D u32 sum|dS| + sum E32 / scale with D = number of those
    keys + 4; exactly 0 on cls query rows."""
    g = torch.Generator().manual_seed(seed)
    kT, kH, kW = k_thw
    R = kH + kW + kT
    d = tokens.attn_desc(B, heads, 8, bool(cls), q_thw, k_thw)
    Nq, Nk = d.Nq, d.Nk
    lds = (Nk + 7) // 8 * 8 + lds_extra
    rows = B * heads * Nq
    scale = 0.35
    S = _randn16((B, heads, Nq, Nk), g, 6.0)
    if Nk > 2:
        S[0, 0, min(1, Nq - 1), Nk // 2] = float(torch.tensor(600.0).to(ACT))
    rq = torch.randn((B, Nq, heads, R), generator=g) if with_rq else None
    x = S * scale
    terms = x.abs()
    if with_rq:
        kt, kh, kw = _key_coords(cls, k_thw)
        rqd = rq.double().permute(0, 2, 1, 3)                       # score rows are (b, head, q), rq rows (b, q, head)
        bias = rqd[..., kh] + rqd[..., kH + kw] + rqd[..., kH + kW + kt]
        babs = rqd[..., kh].abs() + rqd[..., kH + kw].abs() + rqd[..., kH + kW + kt].abs()
        if cls:
            bias[:, :, 0], babs[:, :, 0] = 0.0, 0.0
        x[..., cls:] += bias
        terms[..., cls:] += babs
    mx = x.max(-1, keepdim=True).values
    P = torch.softmax(x, -1)
    e32 = P * U32 * (4 * terms + 4 * (x - mx).abs() + 4 * mx.abs() + 8 + 2 * math.log2(Nk))
    Sd = torch.full((B, heads, Nq, lds), NAN, dtype=ACT, device=device)
    Sd[..., :Nk] = _h(S, device)
    rq_dev = rq.reshape(-1, R).contiguous().to(device) if with_rq else None
    Pd = tokens.softmax_fwd(d, Sd, scale, rq_dev)
    tag = f"Nk={Nk} lds={lds} rows={rows}"
    _assert_stored(f"softmax fwd {tag}", _f64(Pd[..., :Nk]), P, e32)
    if lds > Nk:
        assert torch.equal(_bits(Pd[..., Nk:]), torch.zeros((B, heads, Nq, lds - Nk), dtype=torch.int16)), "pad columns of P"
    if Nk > 2:
        dom = _f64(Pd[0, 0, min(1, Nq - 1), :Nk])
        assert float(dom[Nk // 2]) == 1.0 and float(dom.sum()) == 1.0, "the dominant key must take the whole row"
    # backward, on the stored probabilities
    Ps = _f64(Pd[..., :Nk])
    dP = _randn16((B, heads, Nq, Nk), g)
    dPd = torch.full((B, heads, Nq, lds), NAN, dtype=ACT, device=device)
    dPd[..., :Nk] = _h(dP, device)
    Pin = Pd.clone()
    Pin[..., Nk:] = NAN
    dSd, drq = tokens.softmax_bwd(d, dPd, Pin, scale, want_drq=with_rq)
    dot = (Ps * dP).sum(-1, keepdim=True)
    dS = Ps * (dP - dot)
    eds = Ps * (16 * U32 * (Ps * dP).abs().sum(-1, keepdim=True) + 2 * U32 * (dP.abs() + dot.abs()))
    _assert_stored(f"softmax bwd {tag}", _f64(dSd[..., :Nk]), scale * dS, scale * eds)
    if lds > Nk:
        assert float(_f64(dSd[..., Nk:]).abs().max()) == 0.0, "pad columns of dS"
    if not with_rq:
        assert drq is None
        return
    kt, kh, kw = _key_coords(cls, k_thw)
    onehot = torch.zeros((kT * kH * kW, R), dtype=torch.float64)
    onehot[torch.arange(kT * kH * kW), kh] = 1
    onehot[torch.arange(kT * kH * kW), kH + kw] = 1
    onehot[torch.arange(kT * kH * kW), kH + kW + kt] = 1
    ref = (dS[..., cls:] @ onehot).permute(0, 2, 1, 3)                  # -> (b, q, head, R)
    asum = (dS[..., cls:].abs() @ onehot).permute(0, 2, 1, 3)
    prop = (eds[..., cls:] @ onehot).permute(0, 2, 1, 3)
    Dj = torch.cat([torch.full((kH,), kT * kW), torch.full((kW,), kT * kH), torch.full((kT,), kH * kW)]).double() + 4
    got = drq.cpu().view(B, Nq, heads, R)
    if cls:
        assert float(got[:, 0].abs().max()) == 0.0, "drq of cls query rows"
        ref[:, 0], asum[:, 0], prop[:, 0] = 0.0, 0.0, 0.0
    _assert_fp32(f"softmax drq {tag}", got, ref, Dj * U32 * asum + prop)


def check_softmax_rejects(device):
    """lds = 2056, lds not a multiple of 8, and kH + kW + kT = 65 with a bias are errors with a message."""
    d = tokens.attn_desc(1, 1, 8, True, (1, 1, 1), (2, 2, 3))
    s = torch.zeros((2, 2056), dtype=ACT, device=device)
    rq = torch.zeros((2, 128), device=device)
    lib = get_lib()
    for lds in (2056, 20):
        _expect_error(lambda: lib.call("sf_softmax_fwd", d, s.data_ptr(), lds, 1.0, None, None), "multiple of 8 in [Nk, 2048]")
        _expect_error(lambda: lib.call("sf_softmax_bwd", d, s.data_ptr(), s.data_ptr(), lds, 1.0, None, None),
                      "multiple of 8 in [Nk, 2048]")
    d65 = tokens.attn_desc(1, 1, 8, True, (1, 1, 1), (2, 31, 32))           # Nk = 1985, R = 65
    s = torch.zeros((2, 1992), dtype=ACT, device=device)
    _expect_error(lambda: lib.call("sf_softmax_fwd", d65, s.data_ptr(), 1992, 1.0, rq.data_ptr(), None), "<= 64")
    _expect_error(lambda: lib.call("sf_softmax_bwd", d65, s.data_ptr(), s.data_ptr(), 1992, 1.0, rq.data_ptr(), None), "<= 64")
    assert float(s.float().abs().max()) == 0.0 and float(rq.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------
# rel-pos tables, gather, scatter
def check_relpos_tables(device, D, rows, seed=8):
    """relpos_tables16 (sf_relpos_pack): t16 = the three tables rounded to the storage type, zero rows up to a multiple of 8,
    t16t its transpose, bit for bit.  sf_relpos_unpack: copy or one fp32 add per table (mixed flags), bit for bit."""
    g = torch.Generator().manual_seed(seed)
    tabs = [torch.randn((r, D), generator=g) for r in rows]
    t16, t16t = tokens.relpos_tables16([t.to(device) for t in tabs])
    TR = sum(rows)
    TRp = (TR + 7) // 8 * 8
    want = torch.zeros((TRp, D), dtype=ACT)
    want[:TR] = torch.cat(tabs).to(ACT)
    assert tuple(t16.shape) == (TRp, D) and tuple(t16t.shape) == (D, TRp)
    assert torch.equal(_bits(t16), _bits(want)), "t16"
    assert torch.equal(_bits(t16t), _bits(want.t().contiguous())), "t16t"
    dtab = torch.randn((TRp, D), generator=g)
    prev = [torch.randn((r, D), generator=g) for r in rows]
    for acc in ((0, 0, 0), (1, 0, 1), (0, 1, 0)):
        grads = [p.clone().to(device) for p in prev]
        dd = dtab.to(device)
        get_lib().call("sf_relpos_unpack", dd.data_ptr(), rows[0], rows[1], rows[2], D, grads[0].data_ptr(), grads[1].data_ptr(),
                       grads[2].data_ptr(), acc[0], acc[1], acc[2], None)
        r0 = 0
        for k in range(3):
            piece = dtab[r0:r0 + rows[k]]
            assert torch.equal(_bits(grads[k]), _bits(prev[k] + piece if acc[k] else piece)), f"unpack table {k} acc={acc}"
            r0 += rows[k]


def check_relpos_gather_scatter(device, B, heads, cls, q_thw, k_thw, pitch, seed=9):
    """sf_relpos_gather / sf_relpos_scatter on synthetic G / drq: rq[row][j] is the G entry of the table row that position j of the
    row's query selects (0 on cls rows), E is zero except drq rounded to the storage type at those columns -- bit for bit, with
    rq and E pre-filled with NaN.  ``pitch`` <= 256 runs the LDS kernels, above that the global ones."""
    from slowfast_amd.mvit_engine import _rel_index
    g = torch.Generator().manual_seed(seed)
    qT, qH, qW = q_thw
    kT, kH, kW = k_thw
    rows_h, rows_w, rows_t = 2 * max(qH, kH) - 1, 2 * max(qW, kW) - 1, 2 * max(qT, kT) - 1
    assert pitch >= rows_h + rows_w + rows_t or pitch == 8
    if pitch < rows_h + rows_w + rows_t:                            # the grid-stride case: tiny tables, two key positions
        rows_h, rows_w, rows_t = 1, 2, 1
    d = tokens.attn_desc(B, heads, 8, bool(cls), q_thw, k_thw, rows_h, rows_w, rows_t)
    R = kH + kW + kT
    nrows = B * d.Nq * heads
    if rows_h == 1 and qH > 1:
        ih, iw, it = torch.zeros((qH, kH), dtype=torch.int32), (torch.arange(qW)[:, None] + torch.arange(kW)[None]) % 2, \
            torch.zeros((qT, kT), dtype=torch.int32)
        iw = iw.to(torch.int32).contiguous()
    else:
        ih, iw, it = _rel_index(qH, kH, "cpu"), _rel_index(qW, kW, "cpu"), _rel_index(qT, kT, "cpu")
    assert int(ih.max()) < rows_h and int(iw.max()) < rows_w and int(it.max()) < rows_t
    # the column of G / E behind (row, j)
    tok = torch.arange(d.Nq).clamp(min=cls) - cls
    qt, qh, qw = tok // (qH * qW), (tok // qW) % qH, tok % qW
    col_tok = torch.cat([ih.long()[qh], rows_h + iw.long()[qw], rows_h + rows_w + it.long()[qt]], 1)          # [Nq, R]
    col = col_tok[None, :, None, :].expand(B, d.Nq, heads, R).reshape(nrows, R)
    is_cls = ((torch.arange(d.Nq) == 0) & bool(cls))[None, :, None].expand(B, d.Nq, heads).reshape(nrows)
    idx = [t.to(device) for t in (ih, iw, it)]
    lib = get_lib()
    # gather
    G = torch.randn((nrows, pitch), generator=g).to(ACT)
    Gd = G.to(device)
    rq = torch.full((nrows, R), NAN, device=device)
    lib.call("sf_relpos_gather", d, Gd.data_ptr(), pitch, idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(), rq.data_ptr(), None)
    want = torch.gather(G.float(), 1, col)
    want[is_cls] = 0.0
    assert torch.equal(_bits(rq), _bits(want)), "relpos gather"
    # scatter
    drq = torch.randn((nrows, R), generator=g)
    E = torch.full((nrows, pitch), NAN, dtype=ACT, device=device)
    lib.call("sf_relpos_scatter", d, drq.to(device).data_ptr(), idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(), E.data_ptr(),
             pitch, None)
    wantE = torch.zeros((nrows, pitch), dtype=ACT)
    assert int((torch.sort(col, 1).values.diff(dim=1) == 0).sum()) == 0, "two entries of a row share a column"
    src = drq.to(ACT)
    src[is_cls] = 0
    wantE.scatter_(1, col, src)
    assert torch.equal(_bits(E), _bits(wantE)), "relpos scatter"


def check_relpos_rejects(device):
    """kH + kW + kT = 65 is an error with a message in both entry points."""
    d = tokens.attn_desc(1, 1, 8, True, (1, 1, 1), (2, 31, 32), 63, 63, 3)
    z = torch.zeros(1024, device=device)
    i = torch.zeros(1024, dtype=torch.int32, device=device)
    lib = get_lib()
    _expect_error(lambda: lib.call("sf_relpos_gather", d, z.data_ptr(), 136, i.data_ptr(), i.data_ptr(), i.data_ptr(), z.data_ptr(),
                                   None), "<= 64")
    _expect_error(lambda: lib.call("sf_relpos_scatter", d, z.data_ptr(), i.data_ptr(), i.data_ptr(), i.data_ptr(), z.data_ptr(), 136,
                                   None), "<= 64")


# ------------------------------------------------------------------------------------------------
def check_transpose_heads(device, B=2, Nk=13, heads=3, D=8, ldk=24, seed=10):
    """transpose_heads on the middle slice of a [B, Nk, 3C] tensor: xt[b][head][c][k] = x[b][k][head * D + c] for k < Nk and zero
    in Nk <= k < ldk, bit for bit."""
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    big = torch.randn((B, Nk, 3 * C), generator=g).to(ACT)
    bigd = big.to(device)
    xt = tokens.transpose_heads(bigd[..., C:2 * C], B, Nk, heads, D, ldk)
    want = torch.zeros((B, heads, D, ldk), dtype=ACT)
    want[..., :Nk] = big[..., C:2 * C].view(B, Nk, heads, D).permute(0, 2, 3, 1)
    assert torch.equal(_bits(xt), _bits(want))


def check_row_scale_add(device, B, Ntok, C, resid, ld_extra=0, seed=11):
    """row_scale_add without side rows against fp64 resid + scale[sample] * x: E32 = 2 u32 (|scale x| + |resid|) (the product and
    the sum, fused or not).  The scale vector holds 0 (those rows are bit-equal to resid, or zero without one) and 1 / 0.9."""
    g = torch.Generator().manual_seed(seed)
    M = B * Ntok
    x = _randn16((M, C), g)
    r = _randn16((M, C), g, 3.0) if resid else None
    sc = torch.tensor([1.0 / 0.9, 0.0, 1.25, 0.0, 1.0 / 0.9][:B] + [1.0] * max(0, B - 5))
    xd, _ = _pitched(x, device, ld_extra)
    rd = _pitched(r, device, 2 * ld_extra)[0] if resid else None
    y = tokens.row_scale_add(xd, sc.to(device), Ntok, resid=rd)
    srow = sc.double().repeat_interleave(Ntok)[:, None]
    rr = r if resid else torch.zeros_like(x)
    _assert_stored(f"row_scale_add M={M} C={C}", _f64(y), rr + srow * x, 2 * U32 * ((srow * x).abs() + rr.abs()))
    zero = (srow[:, 0] == 0)
    assert bool(zero.any())
    assert torch.equal(_bits(y)[zero], _bits(rr.to(ACT))[zero]), "rows of scale 0 must be the residual, bit for bit"
