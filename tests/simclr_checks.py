"""Checks of the SimCLR path (csrc/sf_simclr.h, slowfast_amd/contrastive.py), shared by tests/test_simclr_hostsim.py and the
-m gpu file tests/test_simclr_gpu.py.

Reference.  The reference's own op sequence (slowfast/models/contrastive.py: Normalize on both crops' features, then cat / mm /
exp / the off-diagonal mask / masked_select / sum / the positives / div / log / mean of the simclr branch :731-745) run in fp64,
pinned to tests/golden/simclr_contract.json, which tools/make_simclr_golden.py records from the unmodified reference; da and db
come from fp64 autograd.  Every comparison is per element.

Notation: x = [a; b] (M = 2 n rows), q = x / |x|, s_ij = q_i . q_j, p(i) = (i + n) mod M, E_ij = exp((s_ij - 1) / T) for
j != i, D_i = sum_j E_ij, P_ij = E_ij / D_i, t_i = (1 - s_i,p(i)) / T + log D_i (the row's loss term), loss = mean_i t_i,
g_k = sum_j (P_kj + E_kj / D_j) q_j - 2 q_p(k), dx_k = (g_k - q_k (q_k . g_k)) / (M T |x_k|).  The reference's exp(s / T) is
exp(1 / T) E: a common factor that leaves every relative error below as it is.

Bounds, read off the operation counts (u = 2^-24; nothing is fitted to an observed error; any summation order is covered).
They are absolute in the magnitudes of the TERMS, not relative to the result: the loss of M = 2 (pure cancellation to 0) and the
gradient of the `collapsed` kind are held to the rounding of what was cancelled.
  eq     relative error of an element of q: a C-term sum of squares ((C + 1) u, halved by the root), the root, the division:
         (C / 2 + 4) u.
  E_s    a similarity: a C-term fp32 dot in any order, (C + 1) u sum_c|q_ic q_jc|; the errors of both rows of q, 2 eq times the
         same sum; one to spare: (2 C + 10) u sum_c|q_ic q_jc|.
  E_A    the exponential's argument, (s - 1) / T here and s / T there: E_s / T; the rounded difference, 1 / T rounded to fp32
         and the product (or the one division there): 3 u (1 + |s|) / T.
  e      relative error of an exponential: it passes on the error of its argument, E_A, and adds 4 u of its own.
  e_D    relative error of D_i: the weighted mean sum_j P_ij e_ij of its terms' errors and an (M - 1)-term sum of positive terms
         in any order, M u.
  E_t    the row term.  Here: E_A of the positive (the same operations as an argument), e_D through the logarithm, logf's own
         2 u |log D|, the final sum u |t|.  There: the positive's exponential e_i,p(i), the division u, e_D, the logarithm
         2 u |t|.  Both are inside E_A,i,p(i) + e_D,i + 5 u + 3 u (|log D_i| + |t_i|).
  E_loss mean_i E_t,i; an M-term sum in any order and the division: (M + 2) u mean|t_i|.
  E_g    an element of g_k: every summand P_kj q_jc carries e_kj + e_D,k, every summand (E_kj / D_j) q_jc carries e_kj + e_D,j,
         both eq (q_j's own error) and 6 u (the reciprocal or division, the sum of the two reciprocals, the products, 1 / T and
         1 / M as autograd applies them there); the sums over j, M terms each in any order and their addition:
         (M + 2) u sum_j (P_kj + E_kj / D_j)|q_jc|; the positives' 2 q_p(k): (eq + 2 u) each; joining the parts: 2 u of all
         summands' magnitudes.
  E_d    d = q_k . g_k: the C-term dot ((C + 1) u), q's error (eq), one to spare: (1.5 C + 6) u sum_c|q_c g_c|; g's own error,
         sum_c|q_c| E_g,c.
  E_dx   the numerator g - q d: E_g; d's error times |q|; q's error in the product, eq |q d|; the product and the difference,
         3 u (|g| + |q d|).  The division by |x| (its relative error is below eq) and the factor 1 / (M T) however it is formed:
         (eq + 6 u) (|g| + |q d|).  All over M T |x|.  A grad_out scales dx and its bound by |grad_out| and adds one rounding.
The condition on these bounds is that the reference's OWN fp32 CPU run stays inside them on every recorded input (ratio <= 1):
asserted by the golden tool, recorded in the fixture, and checked again here on the CPU (check_reference_inside_bounds).
"""
import itertools
import json
import os

import torch

import slowfast_amd as sa
from slowfast_amd import contrastive as ct
from slowfast_amd import engine
from slowfast_amd.lib import SfError, get_lib
from tests import moco_checks as mc
from tests.moco_checks import U, count_calls, digest, f32_list, sample_index, state_list  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simclr_contract.json")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with open(GOLDEN) as f:
            _fx = json.load(f)
    return _fx


# ------------------------------------------------------------------------------------------------ the loss kernel
NTX_N = (1, 2, 5, 33, 67)   # M = 2: positives only, the loss cancels to 0; M = 66, 134: one and two 64-row chunks plus a tail,
#                             and more row terms than one wave of the loss workgroup holds
NTX_C = (64, 100, 128)      # 100: tail lanes, and zero-filled columns of the second staged 64-column step
NTX_T = (0.5, 0.1, 0.07)
NTX_SCALES = (1.0, 1e-3, 1e3)
NTX_KINDS = ("randn", "parallel", "antiparallel", "near", "onehot", "duplicate", "collapsed")
NTX_GRADS = (1.0, 1024.0)
NTX_SHAPES = tuple(itertools.product(NTX_N, NTX_C))
LAUNCHES = ["sf_simclr_norm", "sf_simclr_rows", "sf_simclr_grad"]
GRAD_SAMPLE = 2             # elements of da and of db recorded per case
PITCH_PAD_A, PITCH_PAD_B = 24, 40


def ntx_cases(n, C):
    """Every (T, scale, kind) of one shape."""
    return itertools.product(NTX_T, NTX_SCALES, NTX_KINDS)


def ntx_key(n, C, T, scale, kind):
    return "n%d_C%d_T%g_s%g_%s" % (n, C, T, scale, kind)


def shape_key(n, C):
    return "n%d_C%d" % (n, C)


def pack_record(loss, da_sample, db_sample, ratios):
    """One case of the fixture as a flat row: loss, GRAD_SAMPLE elements of da, as many of db, the three reference ratios.
    fp32 results are written with nine digits, which is what a float32 needs."""
    return [float("%.9g" % v) for v in [loss] + list(da_sample) + list(db_sample)] + [float("%.4g" % x) for x in ratios]


def ntx_records(fx, n, C):
    """{(T, scale, kind): dict(loss, da_sample, db_sample, reference_ratio)} of one shape; the rows are in ntx_cases order."""
    rows = fx[shape_key(n, C)]
    cases = list(ntx_cases(n, C))
    assert len(rows) == len(cases), "a case was skipped"
    g = GRAD_SAMPLE if n * C >= GRAD_SAMPLE else n * C
    return {c: dict(loss=r[0], da_sample=r[1:1 + g], db_sample=r[1 + g:1 + 2 * g], reference_ratio=r[1 + 2 * g:])
            for c, r in zip(cases, rows)}


def ntx_inputs(n, C, scale, kind, seed=91):
    """(a (n, C), b (n, C)), float32 on the CPU.  `parallel`: b = 2.5 a, every positive similarity is 1; `antiparallel`:
    b = -2.5 a; `near`: unit rows, b = a plus a 1e-3 perturbation; `onehot`: one-hot rows, so the negatives' similarities are
    exactly 0 or 1; `duplicate`: rows 0 and 1 of a are equal, a negative with similarity 1 (n = 1 has no second row and stays
    `randn`); `collapsed`: all 2 n rows equal, loss = log(M - 1) and a gradient that is pure cancellation.  The input scale
    multiplies a and b afterwards."""
    g = torch.Generator().manual_seed(seed + 7 * n + C)
    a = torch.randn((n, C), generator=g) * 3.0
    b = torch.randn((n, C), generator=g) * 3.0
    if kind == "parallel":
        b = a * 2.5
    elif kind == "antiparallel":
        b = a * -2.5
    elif kind == "near":
        a = mc._unit(a)
        b = a + 1e-3 * torch.randn((n, C), generator=g)
    elif kind == "onehot":
        a, b = torch.zeros((n, C)), torch.zeros((n, C))
        a[torch.arange(n), torch.randint(0, C, (n,), generator=g)] = 1.0
        b[torch.arange(n), torch.randint(0, C, (n,), generator=g)] = 1.0
    elif kind == "duplicate":
        if n > 1:
            a[1] = a[0]
    elif kind == "collapsed":
        a = a[:1].repeat(n, 1)
        b = a.clone()
    else:
        assert kind == "randn", kind
    return (a * scale).contiguous(), (b * scale).contiguous()


def reference_sequence(a, b, T):
    """The reference's torch-op sequence (contrastive.py:698-699, :705-706 with Normalize :881-884, then :731-745) in the dtype
    of its arguments.  ``a`` and ``b`` may require grad."""
    q = a.div(a.pow(2).sum(1, keepdim=True).pow(0.5))
    q2 = b.div(b.pow(2).sum(1, keepdim=True).pow(0.5))
    out = torch.cat([q, q2], dim=0)
    sim_matrix = torch.exp(torch.mm(out, out.t().contiguous()) / T)
    mask = (torch.ones_like(sim_matrix) - torch.eye(out.shape[0], device=sim_matrix.device)).bool()
    sim_matrix = sim_matrix.masked_select(mask).view(out.shape[0], -1)
    pos_sim = torch.exp(torch.sum(q * q2, dim=-1) / T)
    pos_sim = torch.cat([pos_sim, pos_sim], dim=0)
    return (-torch.log(pos_sim / sim_matrix.sum(dim=-1))).mean()


_ntx_cache = {}


def ntx_reference(n, C, T, scale, kind):
    """fp64: loss, da, db (autograd, grad_out 1) and the bounds of the module docstring.  Computed once per case and shared by
    the checks of its shape."""
    key = (n, C, T, scale, kind)
    if key in _ntx_cache:
        return _ntx_cache[key]
    if _ntx_cache and next(iter(_ntx_cache))[:2] != (n, C):
        _ntx_cache.clear()                  # one shape's cases at a time: the tests walk the grid shape by shape
    a, b = ntx_inputs(n, C, scale, kind)
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    loss = reference_sequence(ad, bd, T)
    loss.backward()
    loss, da, db = loss.detach(), ad.grad.detach(), bd.grad.detach()
    M = 2 * n
    with torch.no_grad():
        x = torch.cat([ad.detach(), bd.detach()], 0)
        nrm = x.pow(2).sum(1, keepdim=True).sqrt()
        q = x / nrm
        qa = q.abs()
        ar = torch.arange(M)
        p = (ar + n) % M
        eq = (C / 2 + 4) * U
        s = q @ q.t()
        E_s = (2 * C + 10) * U * (qa @ qa.t())
        E_A = E_s / T + 3 * U * (1 + s.abs()) / T
        e = E_A + 4 * U
        Ex = torch.exp((s - 1) / T)
        Ex[ar, ar] = 0.0
        D = Ex.sum(1)
        P = Ex / D[:, None]
        e_D = (P * e).sum(1) + M * U
        t = (1 - s[ar, p]) / T + D.log()
        E_t = E_A[ar, p] + e_D + 5 * U + 3 * U * (D.log().abs() + t.abs())
        E_loss = float(E_t.mean() + (M + 2) * U * t.abs().mean())
        W2 = Ex / D[None, :]
        r1 = e + e_D[:, None] + eq + 6 * U
        r2 = e + e_D[None, :] + eq + 6 * U
        mags = (P + W2) @ qa
        E_g = (P * r1 + W2 * r2) @ qa + (M + 2) * U * mags + 2 * (eq + 2 * U) * qa[p] + 2 * U * (mags + 2 * qa[p])
        g = (P + W2) @ q - 2 * q[p]
        d = (q * g).sum(1, keepdim=True)
        E_d = (1.5 * C + 6) * U * (qa * g.abs()).sum(1, keepdim=True) + (qa * E_g).sum(1, keepdim=True)
        mag = g.abs() + (q * d).abs()
        E_dx = (E_g + qa * E_d + eq * (q * d).abs() + 3 * U * mag + (eq + 6 * U) * mag) / (M * T * nrm)
        # the closed form of the kernels is the reference's arithmetic: its fp64 values agree with fp64 autograd
        dx = (g - q * d) / (M * T * nrm)
        assert abs(float(t.mean()) - float(loss)) <= 1e-9 * max(1.0, abs(float(loss))) + 1e-3 * E_loss
        assert bool(((dx - torch.cat([da, db], 0)).abs() <= 1e-3 * E_dx + 1e-300).all())
    out = dict(a=a, b=b, T=T, loss=loss, da=da, db=db, E_loss=E_loss, E_da=E_dx[:n], E_db=E_dx[n:])
    _ntx_cache[key] = out
    return out


def ntx_ratios(r, loss, da, db, grad_out=1.0):
    """Deviations from the fp64 reference in units of the bounds: (loss, da, db); da, db are the gradients for ``grad_out``."""
    g = abs(grad_out)
    out = [abs(float(loss.detach()) - float(r["loss"])) / r["E_loss"]]
    for got, want, E in ((da, r["da"], r["E_da"]), (db, r["db"], r["E_db"])):
        out.append(float(((got.detach().cpu().double() - want * grad_out).abs() / (E * g + U * (want * g).abs() + 1e-300)).max()))
    return tuple(out)


def reference_fp32_ratios(n, C, T, scale, kind):
    """The reference's own fp32 CPU run (its torch-op sequence and autograd) in units of the bounds."""
    r = ntx_reference(n, C, T, scale, kind)
    a, b = r["a"].clone().requires_grad_(True), r["b"].clone().requires_grad_(True)
    loss = reference_sequence(a, b, T)
    loss.backward()
    return ntx_ratios(r, loss, a.grad, b.grad)


def check_reference_inside_bounds():
    """CPU: the condition on the bounds over the whole grid, and the fp64 restatement against the recorded reference results."""
    fx = fixture()["ntx"]
    worst = [0.0, 0.0, 0.0]
    count = 0
    for n, C in NTX_SHAPES:
        recs = ntx_records(fx, n, C)
        for T, scale, kind in ntx_cases(n, C):
            ratios = reference_fp32_ratios(n, C, T, scale, kind)
            rec = recs[(T, scale, kind)]
            assert len(rec["reference_ratio"]) == 3
            assert max(ratios) <= 1.0, (n, C, T, scale, kind, ratios)
            assert max(rec["reference_ratio"]) <= 1.0
            r = ntx_reference(n, C, T, scale, kind)
            assert abs(float(r["loss"]) - rec["loss"]) <= r["E_loss"] + 1e-7 * abs(rec["loss"]), (rec["loss"], float(r["loss"]))
            idx = sample_index(n * C, 1, GRAD_SAMPLE)
            for name in ("da", "db"):
                got = r[name].flatten()[idx]
                want = torch.tensor(rec[name + "_sample"], dtype=torch.float64)
                assert bool(((got - want).abs() <= r["E_" + name].flatten()[idx] + 1e-7 * want.abs()).all()), (n, C, T, scale, kind)
            worst = [max(w, x) for w, x in zip(worst, ratios)]
            count += 1
    assert count == len(NTX_SHAPES) * len(NTX_T) * len(NTX_SCALES) * len(NTX_KINDS) == sum(len(v) for v in fx.values()), "a case was skipped"
    print("reference fp32 vs fp64 over %d cases: loss %.3f da %.3f db %.3f of the bounds" % ((count,) + tuple(worst)))
    return worst


def _device_leaf(x, device, pad):
    if not pad:
        return x.clone().to(device).requires_grad_(True)
    n, C = x.shape
    base = torch.full((n, C + pad), float("nan"))
    base[:, :C] = x
    return base.to(device).requires_grad_(True)         # a leaf; the operand is a pitched view of it


def run_ntx(device, r, pitched=False):
    """(loss, the two leaves)."""
    C = r["a"].shape[1]
    la = _device_leaf(r["a"], device, PITCH_PAD_A if pitched else 0)
    lb = _device_leaf(r["b"], device, PITCH_PAD_B if pitched else 0)
    xa, xb = (la[:, :C], lb[:, :C]) if pitched else (la, lb)
    if pitched:
        assert xa.stride(0) == C + PITCH_PAD_A and xb.stride(0) == C + PITCH_PAD_B
    return ct.simclr_ntxent(xa, xb, r["T"]), la, lb


def check_ntx(device, n, C, pitched, report=None):
    """Every (T, scale, kind, grad_out) of one shape: three launches, per-element parity, equal bits on a second call."""
    worst = [0.0, 0.0, 0.0]
    count = 0
    for T, scale, kind in ntx_cases(n, C):
        r = ntx_reference(n, C, T, scale, kind)
        with count_calls() as calls:
            loss, la, lb = run_ntx(device, r, pitched)
        launches = [c for c in calls if c != "sf_simclr_workspace"]
        assert launches == LAUNCHES and len(launches) <= 4, calls
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss2, la2, lb2 = run_ntx(device, r, pitched)
        assert torch.equal(loss.detach(), loss2.detach()), "two runs differ"
        for g in NTX_GRADS:
            ga, gb = torch.autograd.grad(loss, (la, lb), grad_outputs=torch.tensor(g).to(device), retain_graph=True)
            if pitched:
                assert bool((ga[:, C:] == 0).all()) and bool((gb[:, C:] == 0).all()), "the pad columns have no gradient"
            ratios = ntx_ratios(r, loss, ga[:, :C], gb[:, :C], g)
            if max(ratios) > 1.0 or report is not None:
                print("simclr_ntxent %s pitched=%s g=%g: loss %.3f da %.3f db %.3f of the bounds" % (
                    (ntx_key(n, C, T, scale, kind), pitched, g) + ratios))
            assert max(ratios) <= 1.0, (n, C, T, scale, kind, g, ratios)
            ga2, gb2 = torch.autograd.grad(loss2, (la2, lb2), grad_outputs=torch.tensor(g).to(device), retain_graph=True)
            assert torch.equal(ga[:, :C], ga2[:, :C]) and torch.equal(gb[:, :C], gb2[:, :C]), "two runs differ"
            worst = [max(w, x) for w, x in zip(worst, ratios)]
            count += 1
    assert count == len(NTX_T) * len(NTX_SCALES) * len(NTX_KINDS) * len(NTX_GRADS), "a case was skipped"
    print("simclr_ntxent n=%d C=%d pitched=%s, %d cases: loss %.3f da %.3f db %.3f of the bounds" % (
        (n, C, pitched, count) + tuple(worst)))
    if report is not None:
        report["n%d_C%d_pitched%d" % (n, C, int(pitched))] = worst
    return worst


def check_q_out(device):
    """return_q: the normalised rows of a from the first launch, the bits of l2norm_rows(a); None is not written."""
    for n, C in ((5, 100), (67, 128)):
        r = ntx_reference(n, C, 0.1, 1.0, "randn")
        a, b = r["a"].to(device), r["b"].to(device)
        with count_calls() as calls:
            loss, q = ct.simclr_ntxent(a, b, 0.1, return_q=True)
        assert [c for c in calls if c != "sf_simclr_workspace"] == LAUNCHES
        assert tuple(q.shape) == (n, C) and not q.requires_grad
        assert torch.equal(q, ct.l2norm_rows(a))
        ref, bound = mc.l2_reference(r["a"])
        assert bool(((q.cpu().double() - ref).abs() <= bound).all())
        assert torch.equal(loss, ct.simclr_ntxent(a, b, 0.1))


def check_second_call_keeps_the_first(device):
    """The symmetric use: a second loss of the same shape before the first is backpropagated; both backward passes give the
    gradients of a call made on its own (the workspace is scratch, the gradients live in tensors of their own)."""
    r1, r2 = ntx_reference(5, 100, 0.1, 1.0, "randn"), ntx_reference(5, 100, 0.1, 1.0, "near")
    alone = []
    for r in (r1, r2):
        loss, la, lb = run_ntx(device, r)
        alone.append((loss.detach().clone(),) + tuple(g.clone() for g in torch.autograd.grad(loss, (la, lb))))
    loss1, la1, lb1 = run_ntx(device, r1)
    loss2, la2, lb2 = run_ntx(device, r2)
    (loss1 + loss2).backward()
    for got, want in (((loss1.detach(), la1.grad, lb1.grad), alone[0]), ((loss2.detach(), la2.grad, lb2.grad), alone[1])):
        assert all(torch.equal(x, y) for x, y in zip(got, want))


def check_zero_row(device):
    """No epsilon: a zero row enters every D_j, so the loss and EVERY element of both gradients are NaN, as in the reference."""
    r = ntx_reference(5, 100, 0.5, 1.0, "randn")
    for which, row in (("a", 3), ("b", 0)):
        a, b = r["a"].clone(), r["b"].clone()
        (a if which == "a" else b)[row] = 0.0
        ra, rb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ref_loss = reference_sequence(ra, rb, 0.5)
        ref_loss.backward()
        assert bool(ref_loss.isnan()) and bool(ra.grad.isnan().all()) and bool(rb.grad.isnan().all())
        xa, xb = a.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
        loss = ct.simclr_ntxent(xa, xb, 0.5)
        ga, gb = torch.autograd.grad(loss, (xa, xb))
        assert bool(loss.isnan()) and bool(ga.isnan().all()) and bool(gb.isnan().all()), which


POISON = 7.0


def check_ntx_rejections(device):
    """Python surface: each raises SfError before a launch or a workspace.  Launcher: each bad argument returns an error from
    each of the three entry points and from the workspace query before anything is written (poisoned buffers, large enough for
    every shape named, stay as they were)."""
    def make(n, C, dtype=torch.float32):
        return torch.ones((n, C), dtype=dtype).to(device), torch.ones((n, C), dtype=dtype).to(device)

    cases = {"n = 0": lambda: ct.simclr_ntxent(*make(0, 64), 0.5),
             "n = 1025": lambda: ct.simclr_ntxent(*make(1025, 8), 0.5),
             "C = 0": lambda: ct.simclr_ntxent(*make(2, 0), 0.5),
             "C = 1025": lambda: ct.simclr_ntxent(*make(2, 1025), 0.5),
             "b of another n": lambda: ct.simclr_ntxent(make(2, 64)[0], make(3, 64)[1], 0.5),
             "b of another C": lambda: ct.simclr_ntxent(make(2, 64)[0], make(2, 100)[1], 0.5),
             "3-D a": lambda: ct.simclr_ntxent(make(2, 64)[0].unsqueeze(0), make(2, 64)[1], 0.5),
             "fp64 a": lambda: ct.simclr_ntxent(make(2, 64, torch.float64)[0], make(2, 64)[1], 0.5),
             "fp16 b": lambda: ct.simclr_ntxent(make(2, 64)[0], make(2, 64, torch.float16)[1], 0.5),
             "transposed a": lambda: ct.simclr_ntxent(make(64, 2)[0].t(), make(2, 64)[1], 0.5),
             "strided b": lambda: ct.simclr_ntxent(make(2, 64)[0], make(2, 128)[1][:, ::2], 0.5)}
    before = set(ct._simclr_workspaces)
    for what, fn in cases.items():
        with count_calls() as calls:
            try:
                fn()
            except SfError:
                pass
            else:
                raise AssertionError("%s accepted" % what)
        assert [c for c in calls if c != "sf_simclr_workspace"] == [], (what, calls)      # no launch: nothing was written
    assert set(ct._simclr_workspaces) == before, "a rejected shape left a workspace behind"

    lib = get_lib()
    big = 1025 * 1025
    a, b = torch.ones(big).to(device), torch.ones(big).to(device)
    outs = [torch.full((big,), POISON).to(device) for _ in range(3)]            # da, db, q_out
    loss = torch.full((1,), POISON).to(device)
    ws = torch.full((2050 * 1025 + 3 * 2052 + 2050 * 2050,), POISON).to(device)
    stream = ct.ops._stream(a)
    need = lib.call("sf_simclr_workspace", 2, 64)
    assert need == 4 * (4 * 64 + 3 * 4 + 16)
    bad = {"n = 0": dict(n=0), "n = 1025": dict(n=1025), "C = 0": dict(C=0), "C = 1025": dict(C=1025), "lda < C": dict(lda=63),
           "ldb < C": dict(ldb=63), "a workspace one float short": dict(ws_bytes=need - 4)}
    for what, kw in bad.items():
        v = dict(n=2, C=64, lda=64, ldb=64, ws_bytes=ws.numel() * 4)
        v.update(kw)
        for name in LAUNCHES:
            try:
                lib.call(name, v["n"], v["C"], a.data_ptr(), v["lda"], b.data_ptr(), v["ldb"], 2.0, outs[0].data_ptr(),
                         outs[1].data_ptr(), loss.data_ptr(), outs[2].data_ptr(), ws.data_ptr(), v["ws_bytes"], stream)
            except SfError:
                pass
            else:
                raise AssertionError("%s: %s accepted" % (name, what))
        if "n" in kw or "C" in kw:
            try:
                lib.call("sf_simclr_workspace", v["n"], v["C"])
            except SfError:
                pass
            else:
                raise AssertionError("sf_simclr_workspace: %s accepted" % what)
    for t in outs + [loss, ws]:
        assert bool((t == POISON).all()), "a rejected call wrote"
    # the limits themselves are taken
    for n, C in ((1024, 3), (2, 1024), (3, 1)):
        g = torch.Generator().manual_seed(n + C)
        xa, xb = torch.randn((n, C), generator=g), torch.randn((n, C), generator=g)
        got = ct.simclr_ntxent(xa.to(device), xb.to(device), 0.5)
        want = reference_sequence(xa.double(), xb.double(), 0.5)
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (n, C, float(got), float(want))


def check_rejects_host_tensors():
    """With the gfx950 library loaded, host tensors are refused (no torch fallback)."""
    try:
        ct.simclr_ntxent(torch.randn(2, 64), torch.randn(2, 64), 0.5)
    except SfError as e:
        assert "need CUDA/HIP tensors" in str(e)
    else:
        raise AssertionError("a host tensor was accepted by the gfx950 library")
    try:
        ct.simclr_ntxent(torch.randn(2, 64).cuda(), torch.randn(2, 64), 0.5)
    except SfError as e:
        assert "does not match" in str(e)
    else:
        raise AssertionError("a host b was accepted beside a device a")


# ------------------------------------------------------------------------------------------------ capture (GPU)
def check_capture(device, n=8, C=100, T=0.1, kinds=("randn", "near", "duplicate")):
    """The loss and its backward captured once with torch.cuda.graph, replayed on three input sets copied into the static
    buffers, against eager: loss, da and db bit for bit.  (The reference's masked_select synchronises the host and cannot be
    captured at all.)"""
    sets = [ntx_inputs(n, C, 1.0, k) for k in kinds]

    def step(a, b):
        loss = ct.simclr_ntxent(a, b, T)
        da, db = torch.autograd.grad(loss, (a, b))
        return loss, da, db

    eager = []
    for a, b in sets:
        out = step(a.to(device).requires_grad_(True), b.to(device).requires_grad_(True))
        eager.append(tuple(t.detach().clone() for t in out))
    sa_, sb_ = torch.zeros((n, C), device=device).requires_grad_(True), torch.zeros((n, C), device=device).requires_grad_(True)
    with torch.no_grad():
        sa_.copy_(sets[0][0]), sb_.copy_(sets[0][1])
    ct._simclr_workspace(device, n, C)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):          # warm-up off the default stream
        step(sa_, sb_)
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_loss, c_da, c_db = step(sa_, sb_)
    for it, (a, b) in enumerate(sets):
        with torch.no_grad():
            sa_.copy_(a), sb_.copy_(b)
        graph.replay()
        assert torch.equal(c_loss, eager[it][0]) and torch.equal(c_da, eager[it][1]) and torch.equal(c_db, eager[it][2]), it
    torch.cuda.synchronize(device)


# ------------------------------------------------------------------------------------------------ the model
# the recipe's head: three MLP layers, BN_SYNC_MLP set and BN_MLP left off, so the MLP has no BatchNorm1d (over a batch of 4 it
# would amplify the backbone's 16-bit rounding, and the recipe does not have it); num_batches_tracked is read off the backbone
SIMCLR_OPTS = ["CONTRASTIVE.TYPE", "simclr", "CONTRASTIVE.MOCO_MULTI_VIEW_QUEUE", False, "CONTRASTIVE.BN_SYNC_MLP", True]
MODEL_OPTS = mc.MODEL_OPTS + SIMCLR_OPTS   # later keys win: the MoCo keys of moco_checks.MODEL_OPTS are overridden
CROPS, BATCH = mc.CROPS, mc.BATCH          # 3 crops of batch 4: the pairs (0, 1) and (1, 2)
SEQUENTIAL = (True, True, False)
PARAM_SEED, DATA_SEED = 101, 102
PERTURB = mc.PERTURB


def model_cfg(extra=()):
    return sa.get_preset("SLOW_8x8_R50", MODEL_OPTS + list(extra))


def seeded_state(shapes):
    from oracle import video_ref
    return video_ref.randomize_state({k: s for k, s in shapes.items() if k != "knn_mem.memory"}, PARAM_SEED)


def model_inputs(cfg, it):
    g = torch.Generator().manual_seed(DATA_SEED + it)
    shape = (BATCH, 3, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_CROP_SIZE)
    return [[torch.randn(shape, generator=g)] for _ in range(CROPS)]


def batches_tracked(model):
    """[number of BatchNorm layers, the sorted set of their num_batches_tracked]."""
    vals = [int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")]
    return [len(vals), sorted(set(vals))]


def drive(model, cfg, device, forward_fn, perturb):
    """Two iterations of contrastive_forward with CONTRASTIVE.SEQUENTIAL, then one of the non-sequential form, as the golden
    tool drives the reference: per iteration the loss, the gradient norm over the backbone, the preds, perform_backward and
    num_batches_tracked of every BatchNorm layer.  ``perturb(model)`` scales the backbone between iterations (an exact
    fp32 operation)."""
    out = []
    index = torch.arange(BATCH).to(device)
    time = torch.zeros((BATCH, CROPS, 2)).to(device)
    for it, seq in enumerate(SEQUENTIAL):
        cfg.CONTRASTIVE.SEQUENTIAL = seq
        model.zero_grad(set_to_none=True)
        inputs = [[x.to(device) for x in clip] for clip in model_inputs(cfg, it)]
        _, preds, loss, perform_backward = forward_fn(model, cfg, inputs, index, time, 0.0)
        if perform_backward:
            loss.backward()
        grads = [p.grad.detach().float().cpu() for p in model.parameters() if p.grad is not None]
        gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads)))
        out.append(dict(loss=float(loss.detach()), grad_norm=gn, perform_backward=bool(perform_backward),
                        preds=preds.detach().float().cpu(), grads=len(grads), batches_tracked=batches_tracked(model)))
        perturb(model)
    cfg.CONTRASTIVE.SEQUENTIAL = True
    return out


def perturb_backbone(model):
    with torch.no_grad():
        for p in model.backbone.parameters():
            p.data.mul_(PERTURB)
    engine.PARAM_EPOCH += 1


def build_model(device, extra=()):
    cfg = model_cfg(extra)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    own = model.state_dict()
    sd = seeded_state({k: tuple(v.shape) for k, v in own.items()})
    sd.update({k: v for k, v in own.items() if k not in sd})           # the kNN memory keeps its own initialisation
    model.load_state_dict(sd)
    return cfg, model.to(device).train()


def check_state_dict(device):
    rec = fixture()["model"]
    cfg, model = build_model(device)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == rec["state"], "keys, shapes and the reference's order"
    keys = set(model.state_dict())
    assert all(k.startswith("backbone.") for k in keys), sorted(k for k in keys if not k.startswith("backbone."))
    assert not keys & {"ptr", "queue_x", "iter"} and not any(k.startswith("backbone_hist.") for k in keys)
    assert not hasattr(model, "backbone_hist")
    # KNN_ON adds the memory bank and nothing else
    m2 = sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(["CONTRASTIVE.KNN_ON", True, "CONTRASTIVE.LENGTH", 7]))
    assert set(m2.state_dict()) - keys == {"knn_mem.memory"} and tuple(m2.state_dict()["knn_mem.memory"].shape) == (7, 1, 64)
    # a reference-shaped checkpoint loads strictly
    sd = {k: torch.zeros(s, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32)
          for k, s in ((k, tuple(s)) for k, s in rec["state"])}
    model.load_state_dict(sd)


def check_model(device, report=None):
    rec = fixture()["model"]
    cfg, model = build_model(device)
    with count_calls() as calls:
        runs = drive(model, cfg, device, ct.contrastive_forward, perturb_backbone)
    # two pairs per sequential iteration, one in the non-sequential one: three launches each, no momentum encoder, no queue
    for name in LAUNCHES:
        assert calls.count(name) == 2 + 2 + 1, (name, calls.count(name))
    assert not {"sf_ema_update", "sf_queue_enqueue", "sf_moco_nce_slabs", "sf_byol_sim_rows", "sf_l2norm_rows"} & set(calls)
    b = mc.model_bounds()
    res = []
    K = cfg.CONTRASTIVE.QUEUE_LEN
    tracked = 0
    for it, (got, want) in enumerate(zip(runs, rec["iterations"])):
        r = dict(loss=abs(got["loss"] - want["loss"]) / max(1.0, abs(want["loss"])),
                 grad_norm=abs(got["grad_norm"] - want["grad_norm"]) / want["grad_norm"])
        print("simclr tiny model, iteration %d (sequential %s): loss %.6f (reference %.6f) grad_norm %.6f (%.6f): %s (bounds %s)" % (
            it, SEQUENTIAL[it], got["loss"], want["loss"], got["grad_norm"], want["grad_norm"], r, {k: b[k] for k in r}))
        res.append(r)
        for k, v in r.items():
            assert v <= b[k], (it, k, v, b[k])
        assert got["perform_backward"] == want["perform_backward"] == (not SEQUENTIAL[it])
        rows = BATCH * ((CROPS - 1) if SEQUENTIAL[it] else 1)
        assert list(got["preds"].shape) == want["preds_shape"] == [rows, 1 + K]
        assert bool((got["preds"][:, 0] == 9999.0).all()) and bool((got["preds"][:, 1:] == 0).all())
        assert got["grads"] == want["grads"]
        # the middle crop passes through the backbone twice: 2 (CROPS - 1) calls per sequential iteration, 2 otherwise
        tracked += 2 * (CROPS - 1) if SEQUENTIAL[it] else 2
        assert got["batches_tracked"] == want["batches_tracked"] and got["batches_tracked"][0] > 0, got["batches_tracked"]
        assert got["batches_tracked"][1] == [tracked], (got["batches_tracked"], tracked)
    assert len(runs) == len(rec["iterations"]) == 3
    if report is not None:
        report["model"] = res


def check_model_surface(device):
    """index None (the normalised rows, as the reference returns here), a single clip not wrapped in a list, eval -> eval_knn,
    the kNN memory fed by the kernel's q_out, the shared dummy logits, bind_flat."""
    cfg, model = build_model(device, ["CONTRASTIVE.KNN_ON", True, "CONTRASTIVE.LENGTH", 256])
    clips = [[x.to(device) for x in clip] for clip in model_inputs(cfg, 0)]
    with torch.no_grad():
        q0 = model(clips[0])                # index None, the clip itself: Normalize(backbone(clip))
    assert torch.is_tensor(q0) and tuple(q0.shape) == (BATCH, cfg.CONTRASTIVE.DIM) and not q0.requires_grad
    assert float((q0.pow(2).sum(1).sqrt() - 1).abs().max()) < 1e-5
    with torch.no_grad():
        assert tuple(model([clips[0], clips[1]]).shape) == (BATCH, cfg.CONTRASTIVE.DIM)        # a list of clips, index None
    index = torch.tensor([3, 200, 17, 255]).to(device)
    mem0 = model.knn_mem.memory.detach().clone()
    seen = []
    orig = ct.simclr_ntxent
    try:
        def spy(*a, **k):
            out = orig(*a, **k)
            seen.append(out)
            return out
        ct.simclr_ntxent = spy
        with count_calls() as calls:
            logits, loss = model(clips[:2], index, None, None)
    finally:
        ct.simclr_ntxent = orig
    assert [c for c in calls if c in LAUNCHES] == LAUNCHES and "sf_l2norm_rows" not in calls    # no second normalisation
    assert logits is ct.dummy_logits(BATCH, cfg.CONTRASTIVE.QUEUE_LEN, device) and loss.requires_grad
    assert tuple(logits.shape) == (BATCH, 1 + cfg.CONTRASTIVE.QUEUE_LEN)
    assert len(seen) == 1 and len(seen[0]) == 2
    q = seen[0][1]                          # the kernel's q_out
    assert float((q - q0).abs().max()) < 1e-5, "the same batch in training mode: the same rows"
    rows = model.knn_mem.memory[index, 0]
    assert torch.equal(rows, ct._normalize(q.view(BATCH, 1, -1) * 1.0 + mem0[index] * 0.0, 2).squeeze(1)), "Memory.update of q_out"
    assert float((rows - q).abs().max()) < 1e-6
    untouched = torch.ones(256, dtype=torch.bool)
    untouched[index.cpu()] = False
    assert torch.equal(model.knn_mem.memory[untouched.to(device)], mem0[untouched.to(device)])
    loss.backward()
    assert all(p.grad is not None for p in model.backbone.parameters())
    assert model.bind_flat(object()) is model
    model.eval()
    yd, yi = model(clips[0], index)
    assert tuple(yd.shape) == tuple(yi.shape) == (BATCH, 200) and bool((yd[:, :-1] >= yd[:, 1:]).all())


# ------------------------------------------------------------------------------------------------ recipe plumbing, rejections
def check_recipe():
    """The SimCLR_SlowR50_8x8 preset: build_model, construct_optimizer (LARS), bind_flat, the parameter surgery.  Construction
    only: no forward at recipe size."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import FlatOptimizer, construct_optimizer
    cfg = sa.get_preset("SimCLR_SlowR50_8x8", ["NUM_GPUS", 0])
    c = cfg.CONTRASTIVE
    assert (c.TYPE, c.T, c.DIM, c.NUM_MLP_LAYERS, c.MLP_DIM, list(c.PREDICTOR_DEPTHS)) == ("simclr", 0.1, 128, 3, 2048, [])
    assert c.BN_SYNC_MLP and c.SIMCLR_DIST_ON and c.SEQUENTIAL and not c.BN_MLP and not c.MOCO_MULTI_VIEW_QUEUE
    assert c.NUM_CLASSES_DOWNSTREAM == 400
    m = cfg.MODEL
    assert (m.NUM_CLASSES, m.ARCH, m.HEAD_ACT, m.DROPOUT_RATE, m.MODEL_NAME) == (128, "slow", "none", 0.0, "ContrastiveModel")
    assert cfg.TASK == "ssl"
    d = cfg.DATA
    assert d.TRAIN_CROP_NUM_TEMPORAL == 4 and d.TRAIN_CROP_NUM_SPATIAL == 1 and d.SSL_COLOR_JITTER and d.SSL_MOCOV2_AUG
    assert d.COLOR_RND_GRAYSCALE == 0.2 and d.SSL_COLOR_HUE == 0.15 and list(d.SSL_COLOR_BRI_CON_SAT) == [0.6, 0.6, 0.6]
    assert list(d.TRAIN_JITTER_SCALES) == [224, 224] and list(d.TRAIN_JITTER_SCALES_RELATIVE) == [0.2, 0.766]
    assert cfg.BN.NORM_TYPE == "sync_batchnorm" and cfg.BN.NUM_SYNC_DEVICES == 1 and cfg.BN.WEIGHT_DECAY == 0.0
    s = cfg.SOLVER
    assert s.LARS_ON and s.LR_POLICY == "cosine" and s.MAX_EPOCH == 200 and s.WARMUP_EPOCHS == 35.0
    assert s.WARMUP_START_LR == 0.001 and s.WEIGHT_DECAY == 1e-6 and s.BASE_LR == 1.2
    assert sa.get_preset("SimCLR_SlowR50_8x8").NUM_GPUS == 1
    model = sa.build_model(cfg)
    assert type(model).__name__ == "ContrastiveModel" and model.type == "simclr" and not hasattr(model, "backbone_hist")
    head = model.backbone.head
    assert len(head.predictors) == 0 and tuple(head.projection.projection[0].weight.shape) == (2048, 2048)
    assert tuple(head.projection.projection[-1].weight.shape) == (128, 2048)
    reducer = GradReducer(model)
    try:
        opt = construct_optimizer(model, cfg, reducer)
        assert isinstance(opt, FlatOptimizer) and opt.lars
        assert model.bind_flat(opt) is model and model._flat is None
        assert opt.flat_param.numel() == sum(p.numel() for p in model.backbone.parameters())
    finally:
        engine.remove_grad_ready_listener(reducer._listener)
    assert ct.contrastive_parameter_surgery(model, cfg, 0.0, 0) == (model, True)
    assert ct.contrastive_parameter_surgery(model, cfg, 1.5, 7)[1] is True


REJECTED = ((["CONTRASTIVE.MOCO_MULTI_VIEW_QUEUE", True], "MOCO_MULTI_VIEW_QUEUE"),
            (["CONTRASTIVE.PREDICTOR_DEPTHS", "[2]"], "PREDICTOR_DEPTHS"),
            (["NUM_GPUS", 2], "NUM_GPUS"), (["NUM_SHARDS", 2], "NUM_SHARDS"),
            (["BN.NUM_SYNC_DEVICES", 2], "BN_SYNC_MLP"), (["BN.NUM_SYNC_DEVICES", 2], "NUM_SYNC_DEVICES"),
            (["MODEL.ARCH", "x3d"], "MODEL.ARCH"))


def check_rejections():
    for extra, key in REJECTED:
        try:
            sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(extra))
        except NotImplementedError as e:
            assert key in str(e), (extra, str(e))
            if key in ("MOCO_MULTI_VIEW_QUEUE", "PREDICTOR_DEPTHS"):
                assert "CONTRASTIVE.TYPE \"simclr\"" in str(e), str(e)
        else:
            raise AssertionError("%r accepted" % (extra,))
    for typ in ("mem", "self", "swav"):
        try:
            sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(["CONTRASTIVE.TYPE", typ]))
        except NotImplementedError as e:
            assert "CONTRASTIVE.TYPE" in str(e)
        else:
            raise AssertionError("%r accepted" % (typ,))
    # what the recipe sets is taken: BN_SYNC_MLP on one device, with and without BatchNorm in the MLP
    for extra in ([], ["CONTRASTIVE.BN_MLP", True]):
        assert sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(extra)).type == "simclr"
