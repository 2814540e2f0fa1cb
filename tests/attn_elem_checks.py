"""Per-element parity checks of the fused attention kernels (csrc/sf_attn.h: sf_attn_fwd_kernel, sf_attn_bwd_dq_kernel,
sf_attn_bwd_dkv_kernel, sf_attn_reduce_kernel, and their launchers in sf_api.hip), shared by tests/test_attn_elem_hostsim.py and
the -m gpu file tests/test_attn_elem_gpu.py.

Method and notation of tests/token_elem_checks.py: the reference is torch float64 on the CPU evaluated on exactly the operands
the MFMAs see; every comparison is PER ELEMENT, no element is excluded; u16 = lib.act_eps(), u32 = 2^-24, TINY = the smallest
subnormal of the storage type.  ACT is the storage type.

Design roundings that are restated bit for bit on the host (they are the kernel's definition, not its error):
  * scale2 = fp32(scale) * fp32(log2 e);  query-side kernels (forward, dQ): qs = (ACT)((float)q * scale2), x = qs . k + bias;
    key-side kernel (dK / dV): ks = (ACT)((float)k * scale2), x' = q . ks + bias.  x and x' are logits in log2 units.
  * the rq split: t = rq * log2e in fp32, hi = (ACT)t, lo = (ACT)(t - hi); bias(q, key) = sum_j OH[key][j] (hi + lo)[q][j],
    zero on cls query rows, cls keys and beyond R = kH + kW + kT.
From those, in fp64 and by explicit formulas: lse = log2 sum_k 2^x, P = 2^(x - lse), O = P v (+ q on non-cls rows),
delta = sum_d dO (O - residual), dP = dO v^T, dS = P (dP - delta), dQ = scale dS k (+ dO), drq = dS OH, dV = P'^T dO,
dK = scale dS'^T q with P' = 2^(x' - lse), dS' = P' (dP - delta).  The backward reference takes what the kernels READ from
memory as it is: the forward kernel's stored O and lse, and for the key side the query-side kernel's stored delta.

Error terms, read off the code (every bound below is a sum of these; nothing is fitted to an observed error):
  EX    logit: Lx u32 T with T = sum|products| of the logit and Lx = D + 64 NKS the number of products chained onto one fp32
        accumulator (KD MFMAs of 32 + hi and lo MFMAs of 32 per 32-column half of rq, NKS = 1 | 2), whatever their order.
  eP    relative error of one exponential: ln2 (EX + u32 |x - m|) + 8 u32 -- the logit error and the rounded subtraction carried
        through 2^., 8 u32 for v_exp_f32; |x - m| <= xmax - x + 8 under the stale maximum, = |x - lse| in the backward kernels.
  eR    forward only, the rescales of earlier chunks: each alpha = exp2(m - cmax) carries ln2 u32 |m - cmax| + 8 u32 + 1 u32 (the
        product); m only grows, so the |m - cmax| add up to at most xmax - xmin of the row, over at most nch - 1 rescales.
  u16   P and dS enter the second MFMA rounded to ACT: u16 sum_k P |v| (likewise dS); not restated in the reference.
  FLUSH = TINY / 2 + 2^-126 per key: a P (dS) below the normal range of ACT is rounded with an absolute error of half a
        subnormal, and v_exp_f32 flushes results below 2^-126.  Under a stale maximum the frame's own l is >= 1 (the key that
        set m contributes 2^0) and later rescales only shrink earlier terms, so the flush reaches O as <= FLUSH sum_k |v|.
  sums  fp32 accumulation of n terms in any order: n u32 sum|term|.  l: 8 nch + 2 (eight adds per lane and chunk, two
        shuffles); O accumulators: 33 nch (32 products and one rescale per chunk); dQ / drq: 32 nch; dK / dV: 32 nchq + qsplits
        + 1 (the query chunks, the fixed-order sum of sf_attn_reduce_kernel, the scale); delta: D / 4 + 4.
  8 u32 for the reciprocal of l (log2f of l: an ulp of its argument moves it by u32 / ln2, covered by 8 u32 * 1).
Stored 16-bit outputs are then compared under 2 u16 |ref| + TINY + E32 (``_assert_stored``), fp32 outputs under their E32.
"""
import math

import torch

from slowfast_amd import tokens
from slowfast_amd.lib import get_lib
from slowfast_amd.ops import _stream
from tests.kernel_checks import ACT
from tests.token_elem_checks import NAN, _assert_stored, _bits, _f64
from tests.x3d_checks import TINY, U16, U32, _assert_fp32, _expect_error

LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))      # SF_LOG2E as the compiler rounds it
LN2 = math.log(2.0)
FLUSH = TINY / 2 + 2.0 ** -126
PAD = 8                                                                      # pitch of the packed operands: 3 C + PAD

# (id, B, heads, D, cls, q_thw, k_thw, rel, residual, pitched, (QT, KT, B2, qsplits))
# two-tile kernels: B * heads * cdiv(Nq, 128) >= 1024
TWO_TILE_CASES = [
    # the second tile of wave 0 and all of waves 1-3 are clamped rows
    ("D32_17q_10k", 16, 64, 32, 1, (1, 4, 4), (1, 3, 3), True, True, True, (2, 1, False, 1)),
    # two workgroups, the second with one live row; two key chunks, the second with one key
    ("D96_129q_33k", 8, 64, 96, 1, (2, 8, 8), (2, 4, 4), True, True, True, (2, 1, False, 1)),
    # R = 34: the second one-hot half under QT = 2; key-side KT = 2
    ("D32_R34_272k", 16, 64, 32, 0, (1, 1, 17), (1, 16, 17), True, True, True, (2, 2, True, 1)),
    # KD = 4 with KT = 1
    ("D128_17q_10k", 16, 64, 128, 1, (1, 4, 4), (1, 3, 3), True, True, True, (2, 1, False, 1)),
    # the plain path: no rel-pos, no residual, contiguous operands
    ("D64_plain", 16, 64, 64, 1, (1, 4, 4), (1, 3, 3), False, False, False, (2, 1, False, 1)),
]
# edges at B * heads <= 4
EDGE_CASES = [
    ("Nk2", 1, 2, 32, 1, (1, 2, 5), (1, 1, 1), True, True, True, (1, 1, False, 1)),
    ("Nk31", 1, 2, 32, 1, (1, 2, 5), (1, 5, 6), True, True, True, (1, 1, False, 1)),
    ("Nk32", 1, 2, 32, 1, (1, 2, 5), (1, 1, 31), True, True, True, (1, 1, True, 1)),        # R = 33
    ("Nk33", 1, 2, 32, 1, (1, 2, 5), (1, 4, 8), True, True, True, (1, 1, False, 1)),
    ("Nk64", 1, 2, 32, 1, (1, 2, 5), (1, 7, 9), True, True, True, (1, 1, False, 1)),
    ("Nk65", 1, 2, 32, 1, (1, 2, 5), (1, 8, 8), True, True, True, (1, 2, False, 1)),        # the KT switch; R = 17
    ("Nk129", 1, 2, 32, 1, (1, 2, 5), (2, 8, 8), True, True, True, (1, 2, False, 1)),
    ("Nq2", 2, 2, 32, 1, (1, 1, 1), (1, 4, 5), True, True, False, (1, 1, False, 1)),
    ("Nq63", 2, 2, 32, 1, (1, 2, 31), (1, 4, 5), True, True, False, (1, 1, False, 1)),
    ("Nq64", 2, 2, 32, 1, (1, 7, 9), (1, 4, 5), True, True, False, (1, 1, False, 1)),
    ("Nq65", 2, 2, 32, 1, (1, 8, 8), (1, 4, 5), True, True, True, (1, 1, False, 1)),
    ("no_cls_rel", 1, 3, 32, 0, (1, 3, 5), (1, 2, 5), True, True, True, (1, 1, False, 1)),
    ("R16", 1, 2, 32, 1, (1, 2, 5), (1, 8, 7), True, True, True, (1, 1, False, 1)),
    ("R32", 1, 1, 32, 1, (1, 2, 5), (2, 15, 15), True, True, True, (1, 2, False, 1)),
    ("R33", 1, 1, 32, 1, (1, 2, 5), (3, 15, 15), True, True, True, (1, 2, True, 1)),
    ("R48", 1, 1, 32, 1, (1, 1, 5), (2, 23, 23), True, True, True, (1, 2, True, 1)),
    ("split2_Nq513", 1, 2, 32, 1, (2, 16, 16), (1, 3, 3), True, True, True, (1, 1, False, 2)),   # last chunk: one row
    ("split4_nchq32", 1, 1, 32, 1, (1, 31, 33), (1, 3, 3), True, True, False, (1, 1, False, 4)),  # four exact splits
    ("split4_nchq33", 1, 1, 32, 1, (4, 16, 16), (1, 3, 3), True, True, True, (1, 1, False, 4)),   # four splits, ragged last
    ("D96_Nk65", 1, 2, 96, 1, (1, 2, 5), (1, 8, 8), True, True, True, (1, 2, False, 1)),     # one live key in the second workgroup
    ("D64_plain", 2, 2, 64, 1, (1, 4, 4), (1, 3, 3), False, False, False, (1, 1, False, 1)),
    ("D128_Nk65", 1, 2, 128, 1, (1, 2, 5), (1, 8, 8), True, False, True, (1, 1, False, 1)),  # KD = 4 never takes KT = 2
]
# (id, B, heads): the lazy rescale at QT = 1 and QT = 2; q (1, 4, 8) + cls = 33, k (2, 8, 16) + cls = 257 (nine chunks)
RESCALE_CASES = [("QT1", 1, 2, 1), ("QT2", 16, 64, 2)]


def _cdiv(a, b):
    return -(-a // b)


def attn_plan(d, rel):
    """fill_attn, attn_two_tiles and attn_dkv_kt of sf_api.hip restated: (QT, KT, B2, qsplits, chunks_per_split)."""
    kt = 1 if d.D > 96 else (2 if d.Nk > 64 else 1)
    ktiles = _cdiv(d.Nk, 64 * kt)
    nchq = _cdiv(d.Nq, 32)
    splits = max(1, min(_cdiv(512, d.B * d.heads * ktiles), nchq // 8))
    cps = _cdiv(nchq, splits)
    qt = 2 if d.B * d.heads * _cdiv(d.Nq, 128) >= 1024 else 1
    return qt, kt, bool(rel and d.kH + d.kW + d.kT > 32), _cdiv(nchq, cps), cps


def attn_workspace_bytes(d, rel):
    qsplits = attn_plan(d, rel)[3]
    part = qsplits * 2 * d.B * d.Nk * d.heads * d.D * 4 if qsplits > 1 else 0
    return part + (d.B * d.Nq * d.heads * 128 * 2 if rel else 0)


def _rows(q_thw, k_thw):
    return tuple(2 * max(q_thw[i], k_thw[i]) - 1 for i in (1, 2, 0))


def _desc(B, heads, D, cls, q_thw, k_thw, rel):
    return tokens.attn_desc(B, heads, D, bool(cls), q_thw, k_thw, *(_rows(q_thw, k_thw) if rel else (0, 0, 0)))


def _heads(t, heads):
    """[B, N, heads * D] -> [B, heads, N, D]"""
    B, N, C = t.shape
    return t.view(B, N, heads, C // heads).permute(0, 2, 1, 3)


def _round_act(t):
    """fp64 holding fp32-exact values -> the storage type, as (f16)(float) does, back in fp64"""
    return t.float().to(ACT).double()


def _draw(B, heads, D, cls, q_thw, k_thw, rel, seed):
    """Operands of the storage type as fp64 [B, N, C], rq fp32 [B, Nq, heads, R] (not 16-bit representable: the lo half matters)."""
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    Nq, Nk = cls + q_thw[0] * q_thw[1] * q_thw[2], cls + k_thw[0] * k_thw[1] * k_thw[2]
    q, k, v, do = (torch.randn((B, n, C), generator=g).to(ACT).double() for n in (Nq, Nk, Nk, Nq))
    rq = torch.randn((B, Nq, heads, k_thw[1] + k_thw[2] + k_thw[0]), generator=g) * 0.7 if rel else None
    return q, k, v, do, rq


class _Ref:
    """The fp64 forward reference of one problem (computed once, read by the forward and the backward comparison)."""

    def __init__(self, d, q, k, v, rq, scale, residual):
        heads, D, cls = d.heads, d.D, d.cls
        self.d, self.residual = d, residual
        self.scale32 = float(torch.tensor(scale, dtype=torch.float32))
        self.scale2 = float(torch.tensor(self.scale32, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32))
        self.qh, self.kh, self.vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
        self.qs = _round_act(self.qh.float() * torch.tensor(self.scale2, dtype=torch.float32))
        self.ks = _round_act(self.kh.float() * torch.tensor(self.scale2, dtype=torch.float32))
        self.R = d.kH + d.kW + d.kT if rq is not None else 0
        self.NKS = 2 if self.R > 32 else 1
        self.Lx = D + 64 * self.NKS if rq is not None else D
        self.nch = _cdiv(d.Nk, 32)
        self.res_rows = torch.zeros(d.Nq, dtype=torch.float64)
        if residual:
            self.res_rows[cls:] = 1.0
        self.res_rows = self.res_rows[None, None, :, None]
        if rq is not None:
            self.OH = tokens.attn_onehot(d, "cpu")[:d.Nk, :self.R].double()                  # [Nk, R]
            t = rq * torch.tensor(LOG2E32, dtype=torch.float32)                              # fp32 product
            hi = t.to(ACT)
            lo = (t - hi.float()).to(ACT)
            hl = (hi.double() + lo.double()).permute(0, 2, 1, 3).clone()                     # [B, heads, Nq, R]
            hla = (hi.double().abs() + lo.double().abs()).permute(0, 2, 1, 3).clone()
            hl[:, :, :cls], hla[:, :, :cls] = 0.0, 0.0
            self.bias, self.bias_abs = hl @ self.OH.t(), hla @ self.OH.t()
        else:
            self.OH = None
            self.bias = self.bias_abs = torch.zeros((d.B, heads, d.Nq, d.Nk), dtype=torch.float64)
        # query side
        self.x = self.qs @ self.kh.transpose(-1, -2) + self.bias
        self.EX = self.Lx * U32 * (self.qs.abs() @ self.kh.abs().transpose(-1, -2) + self.bias_abs)
        self.xmax = self.x.max(-1, keepdim=True).values
        self.lse = self.xmax[..., 0] + torch.log2(torch.exp2(self.x - self.xmax).sum(-1))
        self.P = torch.exp2(self.x - self.lse[..., None])
        self.Oattn = self.P @ self.vh
        self.O = self.Oattn + self.res_rows * self.qh


def _fwd_bounds(r):
    """(E32 of O, bound of lse).  With w_k the unnormalised weights the kernel sums: each carries the relative error
    e_k = eP + eR (module docstring); l = sum w_k carries el = sum_k P e_k + (8 nch + 2) u32.  Then
      E32(O) = sum_k P |v| (e_k + u16) + 33 nch u32 sum_k P |v| + FLUSH sum_k |v| + |P v| (el + 8 u32) + 2 u32 (|P v| + |q|)
    (the 16-bit P, the accumulation, the flush, the division by l, the final product and sum), and
      |lse - ref| <= el / ln2 + 8 u32 (1 + |xmax| + |lse - xmax| + 16) + u32 |lse|:  log2f on an argument one ulp off, the
    magnitudes of m (in [xmax - 8, xmax]) and of log2 l = lse - m, the final sum."""
    nch = r.nch
    spread = (r.xmax - r.x.min(-1, keepdim=True).values)
    eR = LN2 * U32 * spread + 9 * U32 * (nch - 1)
    e = LN2 * (r.EX + U32 * (r.xmax - r.x + 8)) + 8 * U32 + eR
    el = (r.P * e).sum(-1, keepdim=True) + (8 * nch + 2) * U32
    Pv = r.P @ r.vh.abs()
    e_o = ((r.P * (e + U16)) @ r.vh.abs() + 33 * nch * U32 * Pv + FLUSH * r.vh.abs().sum(-2, keepdim=True)
           + r.Oattn.abs() * (el + 8 * U32) + 2 * U32 * (r.Oattn.abs() + r.res_rows * r.qh.abs()))
    e_lse = el[..., 0] / LN2 + 8 * U32 * (17 + r.xmax[..., 0].abs() + (r.lse - r.xmax[..., 0]).abs()) + U32 * r.lse.abs()
    return e_o, e_lse


class _Dev:
    """The operands on the device.  ``pitched``: q, k, v are channel slices of [B, N, 3 C + PAD] tensors (ONE tensor when
    Nq = Nk) that hold NaN everywhere else; o, dO, dq, dk, dv are slices of NaN-filled tensors of that pitch."""

    def __init__(self, device, d, q, k, v, do, rq, pitched):
        B, C, Nq, Nk = d.B, d.heads * d.D, d.Nq, d.Nk
        self.device, self.C, self.pitched = device, C, pitched
        W = 3 * C + PAD if pitched else C
        self.W = W

        def buf(n):
            return torch.full((B, n, W), NAN, dtype=ACT, device=device)

        if pitched:
            self.qbase = buf(Nq)
            self.kvbase = self.qbase if Nq == Nk else buf(Nk)
            self.q, self.k, self.v = self.qbase[..., :C], self.kvbase[..., C:2 * C], self.kvbase[..., 2 * C:3 * C]
            self.dobase = buf(Nq)
            self.do = self.dobase[..., C:2 * C]
        else:
            self.qbase, self.kbase, self.vbase, self.dobase = buf(Nq), buf(Nk), buf(Nk), buf(Nq)
            self.q, self.k, self.v, self.do = self.qbase, self.kbase, self.vbase, self.dobase
        self.q.copy_(q.to(ACT)), self.k.copy_(k.to(ACT)), self.v.copy_(v.to(ACT)), self.do.copy_(do.to(ACT))
        self.rq = None if rq is None else rq.reshape(-1, rq.shape[-1]).contiguous().to(device)
        self.oh = tokens.attn_onehot(d, device) if rq is not None else None

    def out(self, n, which):
        """(NaN-filled base, the slice an output goes to)"""
        base = torch.full((self.q.shape[0], n, self.W), NAN, dtype=ACT, device=self.device)
        C = self.C
        return base, (base[..., which * C:(which + 1) * C] if self.pitched else base)

    def padding_is_nan(self, base, used):
        """every column of ``base`` outside the slices ``used`` still holds NaN"""
        keep = torch.ones(self.W, dtype=torch.bool)
        for w in used:
            keep[w * self.C:(w + 1) * self.C] = False
        return bool(torch.isnan(base.cpu()[..., keep]).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run_fwd(d, dev, scale, residual):
    obase, o = dev.out(d.Nq, 1)
    lse = torch.full((d.B * d.heads * d.Nq,), NAN, dtype=torch.float32, device=dev.device)
    get_lib().call("sf_attn_fwd", d, dev.q.data_ptr(), dev.W, dev.k.data_ptr(), dev.v.data_ptr(), dev.W, float(scale), _ptr(dev.rq),
                   _ptr(dev.oh), int(residual), o.data_ptr(), dev.W, lse.data_ptr(), _stream(dev.q))
    return obase, o, lse


def _run_bwd(d, dev, scale, residual, o, lse, ws_short=0):
    dqbase, dq = dev.out(d.Nq, 0)
    dkvbase = torch.full((d.B, d.Nk, dev.W), NAN, dtype=ACT, device=dev.device)
    if dev.pitched:
        dk, dv = dkvbase[..., dev.C:2 * dev.C], dkvbase[..., 2 * dev.C:3 * dev.C]
    else:
        dk, dv = dkvbase, torch.full((d.B, d.Nk, dev.W), NAN, dtype=ACT, device=dev.device)
    delta = torch.full_like(lse, NAN)
    drq = None if dev.rq is None else torch.full_like(dev.rq, NAN)
    nbytes = get_lib().call("sf_attn_bwd_workspace", d)
    ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dev.device)           # 0xFFFFFFFF: a NaN in fp32 and ACT
    get_lib().call("sf_attn_bwd", d, dev.q.data_ptr(), dev.W, dev.k.data_ptr(), dev.v.data_ptr(), dev.W, float(scale), _ptr(dev.rq),
                   _ptr(dev.oh), int(residual), o.data_ptr(), dev.do.data_ptr(), dev.W, lse.data_ptr(), delta.data_ptr(),
                   dq.data_ptr(), dev.W, dk.data_ptr(), dv.data_ptr(), dev.W, _ptr(drq), ws.data_ptr(), nbytes - ws_short,
                   _stream(dev.q))
    return dict(dqbase=dqbase, dq=dq, dkvbase=dkvbase, dk=dk, dv=dv, delta=delta, drq=drq)


def _check_plan(d, rel, expect):
    plan = attn_plan(d, rel)
    assert plan[:4] == tuple(expect), f"the case no longer reaches its kernel: (QT, KT, B2, qsplits) = {plan[:4]}, expected {expect}"
    assert get_lib().call("sf_attn_bwd_workspace", d) == attn_workspace_bytes(d, rel), "sf_attn_bwd_workspace != attn_plan"
    return plan


def _compare_fwd(tag, d, dev, r, obase, o, lse):
    """O per element against fp64 P v (+ q) and lse per row against fp64 log2 sum 2^x, under _fwd_bounds."""
    e_o, e_lse = _fwd_bounds(r)
    _assert_stored(f"attn fwd O {tag}", _heads(_f64(o), d.heads), r.O, e_o)
    _assert_fp32(f"attn fwd lse {tag}", lse.cpu().view(d.B, d.heads, d.Nq), r.lse, e_lse)
    if dev.pitched:
        assert dev.padding_is_nan(obase, [1]), "attn fwd wrote outside its slice of o"


def _compare_bwd(tag, d, dev, r, do, o, lse, out, plan):
    """delta, dQ, drq (query-side kernel) and dK, dV (key-side kernel + reduce) per element.  With O_st, lse, delta_k the stored
    values the kernels read, Ed = (D / 4 + 4) u32 sum_d |dO| (|O_st| + |q|) the bound of delta, eP = ln2 (EX + u32 |x - lse|) +
    8 u32 and EdP = D u32 sum_d |dO| |v|:
      E(dS) = |dS| (eP + 2 u32) + P (EdP + Ed + u32 (|dP| + |delta|))           (Ed only where the kernel recomputes delta)
      E32(dQ) = scale sum_k (E(dS) + u16 |dS| + FLUSH (1 + |dP - delta|)) |k| + (32 nch + 2) u32 scale sum_k |dS k|
                + 2 u32 (|scale dS k| + |dO|)
      E(drq)  = sum_k OH (E(dS) + u16 |dS| + FLUSH (1 + |dP - delta|)) + 32 nch u32 sum_k OH |dS|,  exactly 0 on cls rows
      E32(dV) = sum_q (P' eP' + u16 P' + FLUSH) |dO| + Lq u32 sum_q P' |dO|,   Lq = 32 nchq + qsplits + 1
      E32(dK) = scale sum_q (E(dS') + u16 |dS'| + FLUSH (1 + |dP - delta|)) |q| + Lq u32 scale sum_q |dS' q| + 2 u32 |dK|."""
    heads, D, cls = d.heads, d.D, d.cls
    doh = _heads(do, heads)
    O_st = _heads(_f64(o), heads)
    lse_k = lse.cpu().double().view(d.B, heads, d.Nq)
    assert bool(torch.isfinite(lse_k).all())
    resq = r.res_rows * r.qh
    delta = (doh * (O_st - resq)).sum(-1)
    Ed = (D // 4 + 4) * U32 * (doh.abs() * (O_st.abs() + resq.abs())).sum(-1)
    delta_k = out["delta"].cpu().view(d.B, heads, d.Nq)
    _assert_fp32(f"attn bwd delta {tag}", delta_k, delta, Ed)
    dP = doh @ r.vh.transpose(-1, -2)
    EdP = D * U32 * (doh.abs() @ r.vh.abs().transpose(-1, -2))
    scale = r.scale32
    # query side
    xl = r.x - lse_k[..., None]
    P = torch.exp2(xl)
    eP = LN2 * (r.EX + U32 * xl.abs()) + 8 * U32
    dd = dP - delta[..., None]
    dS = P * dd
    EdS = dS.abs() * (eP + 2 * U32) + P * (EdP + Ed[..., None] + U32 * (dP.abs() + delta.abs()[..., None]))
    op = EdS + U16 * dS.abs() + FLUSH * (1 + dd.abs())
    dSk = dS @ r.kh
    ref = scale * dSk + r.res_rows * doh
    e32 = (scale * (op @ r.kh.abs()) + (32 * r.nch + 2) * U32 * scale * (dS.abs() @ r.kh.abs())
           + 2 * U32 * ((scale * dSk).abs() + r.res_rows * doh.abs()))
    _assert_stored(f"attn bwd dQ {tag}", _heads(_f64(out["dq"]), heads), ref, e32)
    if r.OH is not None:
        got = out["drq"].cpu().view(d.B, d.Nq, heads, r.R).permute(0, 2, 1, 3)
        assert float(got[:, :, :cls].abs().max()) == 0.0 if cls else True, "drq of cls query rows must be exactly 0"
        live = torch.ones(d.Nq, dtype=torch.float64)
        live[:cls] = 0.0
        live = live[None, None, :, None]
        _assert_fp32(f"attn bwd drq {tag}", got, live * (dS @ r.OH), live * (op @ r.OH + 32 * r.nch * U32 * (dS.abs() @ r.OH)))
    else:
        assert out["drq"] is None
    # key side
    xk = r.qh @ r.ks.transpose(-1, -2) + r.bias
    EXk = r.Lx * U32 * (r.qh.abs() @ r.ks.abs().transpose(-1, -2) + r.bias_abs)
    xl = xk - lse_k[..., None]
    Pk = torch.exp2(xl)
    ePk = LN2 * (EXk + U32 * xl.abs()) + 8 * U32
    ddk = dP - delta_k.double()[..., None]
    dSk_ = Pk * ddk
    EdSk = dSk_.abs() * (ePk + 2 * U32) + Pk * (EdP + U32 * (dP.abs() + delta_k.double().abs()[..., None]))
    Lq = 32 * _cdiv(d.Nq, 32) + plan[3] + 1
    PT, dST = Pk.transpose(-1, -2), dSk_.transpose(-1, -2)
    ref = PT @ doh
    e32 = (Pk * ePk + U16 * Pk + FLUSH).transpose(-1, -2) @ doh.abs() + Lq * U32 * (PT @ doh.abs())
    _assert_stored(f"attn bwd dV {tag}", _heads(_f64(out["dv"]), heads), ref, e32)
    ref = scale * (dST @ r.qh)
    e32 = (scale * ((EdSk + U16 * dSk_.abs() + FLUSH * (1 + ddk.abs())).transpose(-1, -2) @ r.qh.abs())
           + Lq * U32 * scale * (dST.abs() @ r.qh.abs()) + 2 * U32 * ref.abs())
    _assert_stored(f"attn bwd dK {tag}", _heads(_f64(out["dk"]), heads), ref, e32)
    if dev.pitched:
        assert dev.padding_is_nan(out["dqbase"], [0]), "attn bwd wrote outside its slice of dq"
        assert dev.padding_is_nan(out["dkvbase"], [1, 2]), "attn bwd wrote outside its slices of dk / dv"


def _check(device, tag, d, q, k, v, do, rq, residual, pitched, expect, backward=True):
    rel = rq is not None
    plan = _check_plan(d, rel, expect)
    scale = d.D ** -0.5
    r = _Ref(d, q, k, v, rq, scale, residual)
    dev = _Dev(device, d, q, k, v, do, rq, pitched)
    obase, o, lse = _run_fwd(d, dev, scale, residual)
    _compare_fwd(tag, d, dev, r, obase, o, lse)
    if not backward:
        return r
    out = _run_bwd(d, dev, scale, residual, o, lse)
    _compare_bwd(tag, d, dev, r, do, o, lse, out, plan)
    again = _run_bwd(d, dev, scale, residual, o, lse)
    for name in ("dq", "dk", "dv", "delta", "drq"):
        if out[name] is not None:
            assert torch.equal(_bits(out[name]), _bits(again[name])), f"attn bwd {name}: two identical calls differ"
    return r


def check_attn(device, B, heads, D, cls, q_thw, k_thw, rel, residual, pitched, expect, seed=20, backward=True):
    """check_attn_fwd and check_attn_bwd of one case on random operands (the forward reference is shared): O and lse
    (_compare_fwd), then delta, dQ, drq, dK, dV through a direct sf_attn_bwd call on the forward's own o and lse (_compare_bwd),
    two identical backward calls bit for bit, the NaN padding of pitched outputs, and the kernel variant the case claims."""
    d = _desc(B, heads, D, cls, q_thw, k_thw, rel)
    q, k, v, do, rq = _draw(B, heads, D, cls, q_thw, k_thw, rel, seed)
    _check(device, f"D={D} B*h={B * heads} Nq={d.Nq} Nk={d.Nk}", d, q, k, v, do, rq, residual, pitched, expect, backward=backward)


def check_attn_fwd(device, *case, **kw):
    """The forward half of check_attn alone: O per element, lse per row."""
    check_attn(device, *case, backward=False, **kw)


check_attn_bwd = check_attn          # the backward comparison needs the forward kernel's own o and lse: one call checks both


# ------------------------------------------------------------------------------------------------
# the lazy rescale
RESCALE_Q_THW, RESCALE_K_THW = (1, 4, 8), (2, 8, 16)
_RESCALE_U_RAMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]                   # key chunk c carries U_RAMP[c] * g u + W_RAMP[c] * g w
_RESCALE_W_RAMP = [0, 2, 4, 6, 5.5, 6.5, 5, 6, 6.2]
# query i carries (a, b)[i % 4]: rises by 5 / 10 per chunk, falls, and climbs to chunk 3 then stays within +-8
_RESCALE_AB = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (2.0, 0.0)]


def rescale_operands(B, heads, seed=21):
    """Structured operands at D = 32: with u, w two orthogonal +-1 directions, key chunk c holds ramp[c] g u (+ w likewise) and
    query i holds a_i u + b_i w, so that x = scale2 * 32 g (a U_RAMP[c] + b W_RAMP[c]) = 5 (a U_RAMP[c] + b W_RAMP[c]) in log2
    units, plus noise of standard deviation 0.05 on every entry of q and k."""
    g = torch.Generator().manual_seed(seed)
    D, cls = 32, 1
    d = _desc(B, heads, D, cls, RESCALE_Q_THW, RESCALE_K_THW, True)
    scale2 = D ** -0.5 * LOG2E32
    gk = 5.0 / (scale2 * D)
    u = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0)
    w = torch.where(torch.arange(D) % 4 < 2, 1.0, -1.0)
    assert float(u @ w) == 0.0
    chunk = torch.arange(d.Nk) // 32
    kdir = gk * (torch.tensor(_RESCALE_U_RAMP)[chunk][:, None] * u + torch.tensor(_RESCALE_W_RAMP)[chunk][:, None] * w)
    ab = torch.tensor(_RESCALE_AB)[torch.arange(d.Nq) % 4]
    qdir = ab[:, :1] * u + ab[:, 1:] * w
    k = (kdir[None, :, None, :] + 0.05 * torch.randn((B, d.Nk, heads, D), generator=g)).reshape(B, d.Nk, -1).to(ACT).double()
    q = (qdir[None, :, None, :] + 0.05 * torch.randn((B, d.Nq, heads, D), generator=g)).reshape(B, d.Nq, -1).to(ACT).double()
    v, do = (torch.randn((B, n, heads * D), generator=g).to(ACT).double() for n in (d.Nk, d.Nq))
    rq = torch.randn((B, d.Nq, heads, d.kH + d.kW + d.kT), generator=g) * 0.3
    return d, q, k, v, do, rq


def rescale_replay(x):
    """The forward kernel's rule on fp64 logits x [..., Nq, Nk]: per 32-key chunk, m moves to the chunk maximum iff that exceeds
    m + 8.  Returns (rescales after chunk 0 per query, max P under a stale maximum per query, max P per query,
    mixed[..., tile]: a 16-query tile with growing and non-growing columns in one chunk >= 1)."""
    Nq, Nk = x.shape[-2:]
    m = torch.full(x.shape[:-1], -math.inf, dtype=torch.float64)
    count = torch.zeros(x.shape[:-1], dtype=torch.int64)
    stale_p = torch.zeros(x.shape[:-1], dtype=torch.float64)
    all_p = torch.zeros(x.shape[:-1], dtype=torch.float64)
    ntile = _cdiv(Nq, 16)
    mixed = torch.zeros(x.shape[:-2] + (ntile,), dtype=torch.bool)
    for c in range(_cdiv(Nk, 32)):
        cmax = x[..., 32 * c:32 * c + 32].max(-1).values
        grow = cmax > m + 8
        m = torch.where(grow, cmax, m)
        pmax = torch.exp2(cmax - m)
        all_p = torch.maximum(all_p, pmax)
        if c:
            count += grow
            stale_p = torch.maximum(stale_p, torch.where(grow, torch.zeros_like(pmax), pmax))
            for t in range(ntile):
                gt = grow[..., 16 * t:16 * t + 16]
                mixed[..., t] |= gt.any(-1) & ~gt.all(-1)
    return count, stale_p, all_p, mixed


def check_attn_rescale(device, B, heads, qt):
    """The lazy rescale of the forward kernel after the first key chunk, at QT = ``qt``: structured logits (rescale_operands)
    under the bounds of check_attn, forward and backward.  The conditions that make the case what it claims are asserted from
    the fp64 reference alone, before the kernel's result is looked at."""
    d, q, k, v, do, rq = rescale_operands(B, heads)
    expect = (qt, 2, False, 1)
    r = _Ref(d, q, k, v, rq, d.D ** -0.5, True)
    count, stale_p, all_p, mixed = rescale_replay(r.x)
    frac = float((count >= 2).double().mean())
    print(f"rescale: {frac:.2f} of the queries rescale twice or more, max stale P = {float(stale_p.max()):.1f}, "
          f"max P = {float(all_p.max()):.1f}, mixed tiles = {int(mixed.sum())} of {mixed.numel()}")
    assert frac >= 0.25, "at least a quarter of the queries must rescale twice or more after chunk 0"
    assert bool(mixed.any()), "a 16-query tile must hold growing and non-growing columns in one chunk"
    assert float(stale_p.max()) > 16.0, "some P must exceed 16 under a stale maximum"
    assert float(all_p.max()) <= 256.0, "no P may exceed 256"
    assert bool((count == 0).any()), "some queries must never rescale after chunk 0"
    assert float(q.abs().max()) < 64 and float(k.abs().max()) < 64
    _check(device, f"rescale QT={qt}", d, q, k, v, do, rq, True, True, expect)


# ------------------------------------------------------------------------------------------------
def check_attn_rejects(device):
    """R = 49, D = 48, D = 160, rq without onehot and a workspace one byte short are errors with a message, forward and backward;
    nothing is written."""
    lib = get_lib()

    def problem(D, k_thw, rel=True):
        d = _desc(1, 1, D, 1, (1, 1, 2), k_thw, rel)
        q, k, v, do, rq = _draw(1, 1, D, 1, (1, 1, 2), k_thw, rel, 22)
        return d, _Dev(device, d, q, k, v, do, rq, False)

    def both(d, dev, match, rq="keep", oh="keep", short=0):
        rqp = _ptr(dev.rq) if rq == "keep" else rq
        ohp = _ptr(dev.oh) if oh == "keep" else oh
        o = torch.full((1, d.Nq, d.D), NAN, dtype=ACT, device=device)
        st = torch.full((d.Nq,), NAN, device=device)
        dq, dk, dv = (torch.full((1, n, d.D), NAN, dtype=ACT, device=device) for n in (d.Nq, d.Nk, d.Nk))
        drq = None if rqp is None else torch.full((d.Nq, 64), NAN, device=device)
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
        if not short:
            _expect_error(lambda: lib.call("sf_attn_fwd", d, dev.q.data_ptr(), d.D, dev.k.data_ptr(), dev.v.data_ptr(), d.D, 0.1, rqp,
                                           ohp, 1, o.data_ptr(), d.D, st.data_ptr(), _stream(o)), match)
        nbytes = (lib.call("sf_attn_bwd_workspace", d) if short else 1 << 16) - short
        _expect_error(lambda: lib.call("sf_attn_bwd", d, dev.q.data_ptr(), d.D, dev.k.data_ptr(), dev.v.data_ptr(), d.D, 0.1, rqp, ohp,
                                       1, dev.do.data_ptr(), dev.do.data_ptr(), d.D, st.data_ptr(), st.data_ptr(), dq.data_ptr(), d.D,
                                       dk.data_ptr(), dv.data_ptr(), d.D, _ptr(drq), ws.data_ptr(), nbytes, _stream(o)), match)
        for t in (o, st, dq, dk, dv):
            assert bool(torch.isnan(t).all()), "a rejected call wrote to an output"

    d, dev = problem(32, (1, 24, 24))                              # R = 49
    both(d, dev, "exceeds 48")
    d, dev = problem(32, (1, 2, 2))
    for D in (48, 160):
        bad = _desc(1, 1, D, 1, (1, 1, 2), (1, 2, 2), True)
        both(bad, dev, "head dim must be 32, 64, 96 or 128")
        _expect_error(lambda: lib.call("sf_attn_bwd_workspace", bad), "head dim must be 32, 64, 96 or 128")
    both(d, dev, "come together", oh=None)
    both(d, dev, "workspace too small", short=1)
