"""Checks of the MoCo step glue (csrc/sf_moco.h, slowfast_amd/contrastive.py), shared by tests/test_moco_hostsim.py and the
-m gpu file tests/test_moco_gpu.py.

Reference.  An fp64 restatement of the reference's arithmetic (slowfast/models/contrastive.py: Normalize, the einsum / cat /
div / CrossEntropyLoss sequence of the moco branch), pinned to tests/golden/moco_contract.json, which tools/make_moco_golden.py
records from the unmodified reference; df comes from fp64 autograd.  Every comparison is per element.

Bounds, read off the operation counts (u = 2^-24; nothing is fitted to an observed error; any summation order is covered):
  eq     relative error of an element of q = f / |f|: a C-term sum of squares ((C + 1) u, halved by the root), the root, the
         division: (C / 2 + 4) u.
  EL     a logit (q . k) / T: a C-term fp32 dot in any order, (C + 1) u sum|q_c k_c|; q's own error, eq sum|q_c k_c|; 1 / T
         rounded to fp32 and the product, 2 u:  EL = (1.5 C + 8) u sum_c|q_c k_c| / T.
  e_w    relative error of one negative's weight exp(l_j - M) as it enters the sums, M the running maximum of its row:
         EL_j (the logit), u |l_j - M| (the rounded difference), 4 u (expf), and the rescales exp(M_old - M_new) of an online
         softmax: their exponents add up to at most the row's spread twice over (inside a slab, then between slabs), 2 u spread,
         and each of the at most ceil(K / 64) + 1 factors costs 5 u (expf and the product).  The reference has no rescale; its
         error is inside the same bound.
  sums   a K-term fp32 sum in any order: K u sum|terms|.
  lse    relative error of Z = sum_j exp(l_j): el = sum_j p_j e_w,j + p_0 (EL_0 + u |l_0 - m| + 4 u) + (K + 8) u; the log, the
         maximum added back and the final sum: E_lse = el + 4 u (1 + |lse| + |M|).
  loss   mean over R rows of lse - l_0: mean(E_lse + EL_0) + (R + 2) u mean|lse - l_0|.
  df     dq = 1 / (R T) sum_v [(p_0 - 1) key + sum_j p_j queue_j]: every p_j carries e_w,j + E_lse + u |M - lse| + 6 u, p_0 carries
         EL_0 + E_lse + u |l_0 - lse| + 4 u, the K-term sums (K + 2) u, each product 3 u, the sum over views (V + 2) u.  Then
         df = (dq - q (q . dq)) / |f| propagates E_dq through the C-term dot ((C + 2) u sum|q dq|), q's own error (eq, three
         times) and 4 u for the remaining operations; 1 / |f| costs eq + 2 u more.  A grad_out g scales df and its bound by |g|
         and adds one rounding.
The condition on these bounds is that the reference's OWN fp32 CPU run stays inside them on every recorded input (ratio <= 1):
asserted by the golden tool, recorded in the fixture, and checked again here on the CPU (check_reference_inside_bounds).
"""
import hashlib
import json
import math
import os
import re

import torch

import slowfast_amd as sa
from slowfast_amd import contrastive as ct
from slowfast_amd import engine, lib
from slowfast_amd.lib import SfError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moco_contract.json")
U = 2.0 ** -24
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with open(GOLDEN) as f:
            _fx = json.load(f)
    return _fx


def digest(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def f32_list(t):
    return [float(v) for v in t.detach().cpu().flatten().tolist()]


def sample_index(numel, seed, count):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, numel, (min(count, numel),), generator=g)


class count_calls:
    """Names of the native calls made inside the block (wraps lib.call as tests/test_optim_layer_decay_hostsim.py does)."""

    def __enter__(self):
        self.names = []
        self._lib = lib.get_lib()
        self._orig = self._lib.call

        def call(name, *a, **k):
            self.names.append(name)
            return self._orig(name, *a, **k)

        self._lib.call = call
        return self.names

    def __exit__(self, *exc):
        del self._lib.call


# ------------------------------------------------------------------------------------------------ l2norm_rows
L2_CASES = ((1, 64), (3, 128), (5, 256))
L2_SCALES = (1.0, 1e-3, 1e3)


def l2_input(n, C, scale, seed=11):
    g = torch.Generator().manual_seed(seed + 131 * n + C)
    return torch.randn((n, C), generator=g) * scale


def l2_perm(n, seed=5):
    g = torch.Generator().manual_seed(seed + n)
    return torch.randperm(n, generator=g)


def l2_reference(x):
    xd = x.double()
    ref = xd / xd.pow(2).sum(1, keepdim=True).sqrt()
    return ref, (x.shape[1] / 2 + 4) * U * ref.abs()


def check_l2norm(device, n, C, scale, with_perm, padded):
    x = l2_input(n, C, scale)
    ref, bound = l2_reference(x)
    perm = l2_perm(n) if with_perm else None
    if padded:
        base = torch.full((n, C + 24), float("nan"))
        base[:, :C] = x
        xd = base.to(device)[:, :C]
        assert xd.stride(0) == C + 24
    else:
        xd = x.to(device)
    with count_calls() as calls:
        out = ct.l2norm_rows(xd, perm)
    assert calls == ["sf_l2norm_rows"], calls
    want, b = (ref[perm], bound[perm]) if with_perm else (ref, bound)
    err = (out.cpu().double() - want).abs()
    ratio = float((err / b).max())
    print("l2norm n=%d C=%d scale=%g perm=%s padded=%s: %.3f of the bound" % (n, C, scale, with_perm, padded, ratio))
    assert ratio <= 1.0, ratio
    assert torch.equal(out, ct.l2norm_rows(xd, perm)), "two runs differ"
    return ratio


def check_l2norm_zero_row_and_bad_perm(device):
    """No epsilon: a zero row is NaN, as the reference's Normalize gives; a perm that is no permutation never reaches the device."""
    x = l2_input(3, 64, 1.0)
    x[1] = 0.0
    out = ct.l2norm_rows(x.to(device)).cpu()
    assert bool(out[1].isnan().all()) and bool(out[0].isfinite().all()) and bool(out[2].isfinite().all())
    for bad in ([0, 1, 1], [0, 1, 3], [0, 1], [-1, 0, 1]):
        try:
            ct.l2norm_rows(x.to(device), torch.tensor(bad))
        except SfError as e:
            assert "permutation" in str(e)
        else:
            raise AssertionError("perm %r accepted" % (bad,))


# ------------------------------------------------------------------------------------------------ the fused loss
NCE_SHAPES = ((1, 1, 1), (3, 1, 24), (3, 3, 96), (8, 3, 4096), (64, 2, 192))     # (n, V, K)
NCE_C = (64, 128)
NCE_KINDS = ("randn", "late_max", "key_is_q", "queue_is_minus_q")
T_RECIPE, T_ADVERSARIAL = 0.1, 0.07


def _unit(x):
    return x / x.pow(2).sum(-1, keepdim=True).sqrt()


def nce_inputs(n, V, K, C, kind="randn", seed=23):
    """(f, keys (V, n, C), queue (K, C), T), float32 on the CPU."""
    g = torch.Generator().manual_seed(seed + 7 * n + 13 * V + 17 * K + C)
    f = torch.randn((n, C), generator=g) * 3.0
    keys = _unit(torch.randn((V, n, C), generator=g))
    queue = _unit(torch.randn((K, C), generator=g))
    T = T_RECIPE
    if kind != "randn":
        T = T_ADVERSARIAL
        q = _unit(f)
        if kind == "late_max":              # the largest negative of row 0 is the queue's last row: the rescale fires last
            queue[K - 1] = q[0]
        elif kind == "key_is_q":            # the positive dominates lse
            keys = q.unsqueeze(0).repeat(V, 1, 1).contiguous()
        elif kind == "queue_is_minus_q":
            queue = (-q[0]).unsqueeze(0).repeat(K, 1).contiguous()
    return f, keys, queue, T


def reference_sequence(f, keys, queue, T):
    """The reference's torch-op sequence (contrastive.py:452-477 with Normalize :881-884) in the dtype of its arguments:
    (logits, loss).  ``f`` may require grad."""
    q = f.div(f.pow(2).sum(1, keepdim=True).pow(0.5))
    queue_neg = torch.einsum("nc,kc->nk", [q, queue.clone().detach()])
    logits = None
    for k in range(keys.shape[0]):
        out_pos = torch.einsum("nc,nc->n", [q, keys[k]]).unsqueeze(-1)
        lgt_k = torch.cat([out_pos, queue_neg], dim=1)
        logits = lgt_k if k == 0 else torch.cat([logits, lgt_k], dim=0)
    logits = torch.div(logits, T)
    targets = torch.zeros(logits.shape[0], dtype=torch.long, device=logits.device)
    return logits, torch.nn.functional.cross_entropy(logits, targets, reduction="mean")


_nce_cache = {}


def nce_reference(n, V, K, C, kind):
    """fp64: logits, loss, df (autograd, grad_out 1) and the per-element bounds of the module docstring.  Computed once per
    case and shared."""
    key = (n, V, K, C, kind)
    if key in _nce_cache:
        return _nce_cache[key]
    f, keys, queue, T = nce_inputs(n, V, K, C, kind)
    fd = f.double().requires_grad_(True)
    kd, qd = keys.double(), queue.double()
    logits, loss = reference_sequence(fd, kd, qd, T)
    loss.backward()
    logits, loss, df = logits.detach(), loss.detach(), fd.grad.detach()
    R = V * n
    with torch.no_grad():
        nrm = fd.pow(2).sum(1, keepdim=True).sqrt()
        q = fd / nrm
        qa, ka = q.abs(), qd.abs()
        eq = (C / 2 + 4) * U
        cl = (1.5 * C + 8) * U
        EL_neg = cl * (qa @ ka.t()) / T                                   # (n, K)
        EL_pos = (cl * (qa.unsqueeze(0) * kd.abs()).sum(-1) / T).reshape(R)   # row v n + i
        E_logits = torch.cat([EL_pos.unsqueeze(1), EL_neg.repeat(V, 1)], 1)
        neg = logits[:n, 1:]
        pos = logits[:, 0]
        M = neg.max(1).values                                             # (n)
        spread = M - neg.min(1).values
        eR = 2 * U * spread + 5 * U * (math.ceil(K / 64) + 1)
        e_w = EL_neg + U * (M.unsqueeze(1) - neg) + 4 * U + eR.unsqueeze(1)   # (n, K)
        lse = torch.logsumexp(logits, 1)
        p = torch.exp(logits - lse.unsqueeze(1))
        Mr, e_wr = M.repeat(V), e_w.repeat(V, 1)
        el = (p[:, 1:] * e_wr).sum(1) + p[:, 0] * (EL_pos + U * (pos - torch.maximum(Mr, pos)).abs() + 4 * U) + (K + 8) * U
        E_lse = el + 4 * U * (1 + lse.abs() + Mr.abs())
        E_loss = float((E_lse + EL_pos).mean() + (R + 2) * U * (lse - pos).abs().mean())
        ep = e_wr + (E_lse + U * (Mr - lse).abs() + 6 * U).unsqueeze(1)    # (R, K)
        e0 = EL_pos + E_lse + U * (pos - lse).abs() + 4 * U
        sc = 1.0 / (R * T)
        keyr = kd.reshape(R, C)
        pn = p[:, 1:]
        rows_abs = (p[:, 0] - 1).abs().unsqueeze(1) * keyr.abs() + pn @ ka             # (R, C)
        rows_err = (p[:, 0] * e0).unsqueeze(1) * keyr.abs() + (pn * (ep + (K + 2) * U)) @ ka + 3 * U * rows_abs
        dq = sc * ((p[:, 0] - 1).unsqueeze(1) * keyr + pn @ qd).reshape(V, n, C).sum(0)
        dq_abs = sc * rows_abs.reshape(V, n, C).sum(0)
        E_dq = sc * rows_err.reshape(V, n, C).sum(0) + (V + 2) * U * dq_abs
        qdq = (q * dq).sum(1, keepdim=True)
        aqdq = (qa * dq_abs).sum(1, keepdim=True)
        E_num = E_dq + qa * ((qa * E_dq).sum(1, keepdim=True) + ((C + 2) * U + 2 * eq) * aqdq) + eq * qa * qdq.abs()
        E_df = (E_num + 4 * U * (dq_abs + qa * aqdq)) / nrm + (eq + 2 * U) * df.abs()
    out = dict(f=f, keys=keys, queue=queue, T=T, logits=logits, loss=loss, df=df, E_logits=E_logits, E_loss=E_loss, E_df=E_df)
    _nce_cache[key] = out
    return out


def nce_ratios(r, logits, loss, df, grad_out=1.0):
    """Deviations from the fp64 reference in units of the bounds: (logits, loss, df)."""
    a = float(((logits.detach().cpu().double() - r["logits"]).abs() / r["E_logits"]).max())
    b = abs(float(loss.detach()) - float(r["loss"])) / r["E_loss"]
    g = abs(grad_out)
    c = float(((df.detach().cpu().double() - r["df"] * grad_out).abs() / (r["E_df"] * g + U * (r["df"] * g).abs() + 1e-300)).max())
    return a, b, c


def reference_fp32_ratios(n, V, K, C, kind):
    """The reference's own fp32 CPU run (its torch-op sequence and autograd) in units of the bounds."""
    r = nce_reference(n, V, K, C, kind)
    f = r["f"].clone().requires_grad_(True)
    logits, loss = reference_sequence(f, r["keys"], r["queue"], r["T"])
    loss.backward()
    return nce_ratios(r, logits, loss, f.grad)


def nce_key(n, V, K, C, kind):
    return "n%d_V%d_K%d_C%d_%s" % (n, V, K, C, kind)


def nce_recorded_cases():
    for C in NCE_C:
        for (n, V, K) in NCE_SHAPES:
            yield n, V, K, C, "randn"
    for kind in NCE_KINDS[1:]:
        yield 3, 3, 96, 64, kind
        yield 8, 3, 4096, 128, kind


def check_reference_inside_bounds():
    """CPU: the condition on the bounds, and the fp64 restatement against the recorded reference results."""
    fx = fixture()["nce"]
    for n, V, K, C, kind in nce_recorded_cases():
        if n * K * C > 3 * 96 * 128 * 4 and kind != "randn":
            continue                    # the large adversarial cases are checked by the tool; here the small ones (time)
        ratios = reference_fp32_ratios(n, V, K, C, kind)
        rec = fx[nce_key(n, V, K, C, kind)]
        assert max(ratios) <= 1.0, (n, V, K, C, kind, ratios)
        r = nce_reference(n, V, K, C, kind)
        assert abs(float(r["loss"]) - rec["loss"]) <= r["E_loss"] + 1e-7 * abs(rec["loss"]), (rec["loss"], float(r["loss"]))
        idx = sample_index(r["logits"].numel(), 1, 64)
        got = r["logits"].flatten()[idx]
        want = torch.tensor(rec["logits_sample"], dtype=torch.float64)
        assert bool(((got - want).abs() <= r["E_logits"].flatten()[idx] + 1e-7 * want.abs()).all())
        assert max(rec["reference_ratio"]) <= 1.0


def run_nce(device, r, grad_out=1.0):
    f = r["f"].clone().to(device).requires_grad_(True)       # a fresh leaf: .to() of a host tensor on the host is the tensor itself
    logits, loss = ct.moco_nce(f, r["keys"].to(device), r["queue"].to(device), r["T"])
    (loss * grad_out).backward()
    return logits, loss.detach(), f.grad


def check_nce(device, n, V, K, C, kind="randn", grad_out=1.0, report=None):
    r = nce_reference(n, V, K, C, kind)
    with count_calls() as calls:
        logits, loss, df = run_nce(device, r, grad_out)
    assert calls == ["sf_moco_nce_workspace"] * calls.count("sf_moco_nce_workspace") + ["sf_moco_nce_slabs", "sf_moco_nce_finalize"], calls
    assert tuple(logits.shape) == (V * n, 1 + K)
    ratios = nce_ratios(r, logits, loss, df, grad_out)
    print("nce n=%d V=%d K=%d C=%d %s g=%g: logits %.3f loss %.3f df %.3f of the bounds" % ((n, V, K, C, kind, grad_out) + ratios))
    if report is not None:
        report[nce_key(n, V, K, C, kind) + ("_g%g" % grad_out)] = ratios
    assert max(ratios) <= 1.0, ratios
    # the negatives do not depend on the view: every view's rows agree bit for bit in columns 1 .. K
    lg = logits.view(V, n, 1 + K)
    for v in range(1, V):
        assert torch.equal(lg[v, :, 1:], lg[0, :, 1:])
    # determinism
    logits2, loss2, df2 = run_nce(device, r, grad_out)
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2) and torch.equal(df, df2), "two runs differ"
    return ratios


def check_nce_rejections(device):
    def run(n, V, K, C):
        return ct.moco_nce(torch.randn(n, C).to(device), torch.randn(V, n, C).to(device), torch.randn(K, C).to(device), 0.1)

    for shape, what in (((2, 1, 8, 96), "multiple of 64"), ((2, 1, 8, 63), "multiple of 64"), ((2, 1, 8, 320), "multiple of 64"),
                        ((65, 1, 8, 128), "n \\* C"), ((129, 1, 8, 64), "n \\* C"), ((2, 17, 8, 64), "key views")):
        try:
            run(*shape)
        except SfError as e:
            assert re.search(what, str(e)), (shape, str(e))
        else:
            raise AssertionError("shape %r accepted" % (shape,))
    try:
        ct.moco_nce(torch.randn(2, 64).to(device), torch.randn(1, 3, 64).to(device), torch.randn(8, 64).to(device), 0.1)
    except SfError as e:
        assert "do not match" in str(e)
    else:
        raise AssertionError("mismatched keys accepted")


# ------------------------------------------------------------------------------------------------ enqueue
def reference_enqueue(queue, ptr, keys, multi_view):
    """_dequeue_and_enqueue (contrastive.py:255-281) restated on host tensors: returns the pointer."""
    K = queue.shape[0]
    p = int(ptr)
    for key in (list(keys) if multi_view else [keys[0]]):
        num = int(key.size(0))
        assert K % num == 0 and p + num <= K
        queue[p:p + num, :] = key
        p += num
        if p == K:
            p = 0
    return p


def enqueue_inputs(K=12, rows=4, C=64, views=3, seed=31):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((K, C), generator=g), [torch.randn((rows, C), generator=g) for _ in range(views)]


def check_enqueue(device, views, multi_view, start=0, K=12, rows=4, C=64):
    queue0, keys = enqueue_inputs(K, rows, C, views)
    want = queue0.clone()
    p = reference_enqueue(want, start, keys, multi_view)
    rec = fixture()["enqueue"]["views%d_multi%d_start%d" % (views, int(multi_view), start)]
    assert digest(want) == rec["queue_sha256"] and p == rec["ptr"], "the restatement does not give the reference's queue"
    queue = queue0.to(device)
    ptr = torch.tensor([start], dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    upd = [k.to(device) for k in (keys if multi_view else keys[:1])]
    with count_calls() as calls:
        ct.enqueue(queue, ptr, upd, err)
    assert calls == ["sf_queue_enqueue"], calls
    assert torch.equal(queue.cpu(), want) and int(ptr) == p and int(err) == 0, (int(ptr), p, int(err))
    return p


def check_enqueue_bad_pointer(device, K=12, rows=4, C=64, guard=8):
    """A hand-set out-of-range pointer: a defined no-op that raises the error word.  The queue sits inside a larger buffer
    whose rows after it stay as they were."""
    queue0, keys = enqueue_inputs(K, rows, C, 3)
    # (6, 2): the first block would fit (rows 6 .. 9), the second would not (10 + 4 > 12): nothing at all is written
    for bad, views in ((10, 1), (-1, 1), (K, 1), (6, 2), (2 ** 40, 1), (-2 ** 40, 3)):
        whole = torch.full((K + guard, C), -7.0)
        whole[:K] = queue0
        whole = whole.to(device)
        queue = whole[:K]
        ptr = torch.tensor([bad], dtype=torch.int64, device=device)
        err = torch.zeros(1, dtype=torch.int32, device=device)
        ct.enqueue(queue, ptr, [k.to(device) for k in keys[:views]], err)
        assert int(err) == 1 and int(ptr) == bad, (bad, int(err), int(ptr))
        assert torch.equal(whole[:K].cpu(), queue0) and bool((whole[K:] == -7.0).all()), bad
        try:
            ct.check_queue_error(err)
        except SfError:
            pass
        else:
            raise AssertionError("the error word was not reported")
        assert int(err) == 0
    try:
        ct.enqueue(queue0.to(device), torch.tensor([0], device=device), [torch.randn(5, C).to(device)])
    except SfError as e:
        assert "K % rows" in str(e)
    else:
        raise AssertionError("K % rows != 0 accepted")


# ------------------------------------------------------------------------------------------------ ema_update
EMA_SIZES = (1, 1023, 1024, 4097)
EMA_M = (0.5, 0.994, 0.999, 1 - 1e-7)


def ema_inputs(n, seed=41):
    g = torch.Generator().manual_seed(seed + n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def check_ema(device, n, m):
    p, h = ema_inputs(n)
    want = p * (1.0 - m) + h * m                     # the reference's expression on the CPU: three rounded fp32 operations
    rec = fixture()["ema"].get("n%d_m%r" % (n, m))
    if rec is not None:
        assert digest(want) == rec, "the torch expression does not give the reference's _update_history"
    pd, hd = p.clone().to(device), h.clone().to(device)
    mm = ct.momentum_words(m).to(device)
    with count_calls() as calls:
        ct.ema_update(pd, hd, mm)
    assert calls == ["sf_ema_update"], calls
    assert torch.equal(hd.cpu(), want), float((hd.cpu() - want).abs().max())
    # an unaligned range of a larger buffer (per-tensor path on views of a flat buffer)
    if n > 8:
        big_p, big_h = torch.zeros(n + 3).to(device), torch.zeros(n + 3).to(device)
        big_p[3:] = p.to(device)
        big_h[1:n + 1] = h.to(device)
        ct.ema_update(big_p[3:], big_h[1:n + 1], mm)
        assert torch.equal(big_h[1:n + 1].cpu(), want) and float(big_h[0]) == 0.0 and float(big_h[n + 1:].abs().sum()) == 0.0


def check_rejects_host_tensors():
    """With the gfx950 library loaded, host tensors are refused by every entry (no torch fallback)."""
    for fn in (lambda: ct.l2norm_rows(torch.randn(2, 64)),
               lambda: ct.moco_nce(torch.randn(2, 64), torch.randn(1, 2, 64), torch.randn(8, 64), 0.1),
               lambda: ct.enqueue(torch.randn(8, 64), torch.tensor([0]), [torch.randn(2, 64)], torch.zeros(1, dtype=torch.int32)),
               lambda: ct.ema_update(torch.randn(8), torch.randn(8), torch.tensor([0.5, 0.5]))):
        try:
            fn()
        except SfError as e:
            assert "need CUDA/HIP tensors" in str(e)
        else:
            raise AssertionError("a host tensor was accepted by the gfx950 library")


# ------------------------------------------------------------------------------------------------ the model
MODEL_YAML = "configs/Kinetics/SLOW_8x8_R50.yaml"
# the slow_tiny overrides of oracle/make_golden.py, then the MoCo keys
MODEL_OPTS = ["NUM_GPUS", 0, "MODEL.DROPOUT_RATE", 0.0, "MODEL.NUM_CLASSES", 10, "DATA.TRAIN_CROP_SIZE", 32,
              "RESNET.WIDTH_PER_GROUP", 16, "RESNET.DEPTH", 18, "DATA.NUM_FRAMES", 4,
              "RESNET.NUM_BLOCK_TEMP_KERNEL", "[[2], [2], [2], [2]]",
              "MODEL.MODEL_NAME", "ContrastiveModel", "MODEL.LOSS_FUNC", "contrastive_loss", "MODEL.HEAD_ACT", "none",
              "MODEL.NUM_CLASSES", 64, "CONTRASTIVE.TYPE", "moco", "CONTRASTIVE.DIM", 64, "CONTRASTIVE.QUEUE_LEN", 48,
              "CONTRASTIVE.NUM_MLP_LAYERS", 3, "CONTRASTIVE.MLP_DIM", 32, "CONTRASTIVE.T", 0.1, "CONTRASTIVE.KNN_ON", False,
              "CONTRASTIVE.SEQUENTIAL", True, "CONTRASTIVE.MOCO_MULTI_VIEW_QUEUE", True, "CONTRASTIVE.MOMENTUM", 0.994,
              "TRAIN.BATCH_SIZE", 4, "DATA.TRAIN_CROP_NUM_TEMPORAL", 3, "NUM_GPUS", 1]
PARAM_SEED, DATA_SEED, SHUFFLE_SEED, CROPS, BATCH, ITERS = 61, 62, 63, 3, 4, 2
PERTURB = 0.98          # between the two iterations every backbone parameter is multiplied by this (an exact fp32 operation)
LOGITS_SAMPLE = 64


def model_cfg(extra=()):
    return sa.get_preset("SLOW_8x8_R50", MODEL_OPTS + list(extra))


def state_list(sd):
    return sorted([k, list(v.shape)] for k, v in sd.items())


def seeded_state(shapes, K, dim):
    from oracle import video_ref
    sd = video_ref.randomize_state({k: s for k, s in shapes.items() if k not in ("ptr", "iter", "queue_x")}, PARAM_SEED)
    g = torch.Generator().manual_seed(PARAM_SEED + 1)
    stdv = 1.0 / math.sqrt(dim / 3)
    sd["queue_x"] = torch.rand((K, dim), generator=g).mul_(2 * stdv).add_(-stdv)
    sd["ptr"] = torch.tensor([0])
    sd["iter"] = torch.zeros([1], dtype=torch.long)
    for k in list(sd):                      # the key encoder starts from other weights than the query encoder: the iteration-0
        if k.startswith("backbone_hist.") and sd[k].is_floating_point() and "running" not in k:   # copy must show
            sd[k] = sd[k] * 0.5
    return sd


def model_inputs(cfg, it):
    g = torch.Generator().manual_seed(DATA_SEED + it)
    shape = (BATCH, 3, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_CROP_SIZE)
    return [[torch.randn(shape, generator=g)] for _ in range(CROPS)]


def drive(model, cfg, device, forward_fn, iters=ITERS):
    """Two iterations of contrastive_forward with the shuffle on, as the golden tool drives the reference: per iteration the
    loss, the logits, the gradient norm over the backbone."""
    out = []
    index = torch.arange(BATCH).to(device)
    time = torch.zeros((BATCH, CROPS, 2)).to(device)
    for it in range(iters):
        model.zero_grad(set_to_none=True)
        inputs = [[x.to(device) for x in clip] for clip in model_inputs(cfg, it)]
        torch.manual_seed(SHUFFLE_SEED + it)
        _, preds, loss, perform_backward = forward_fn(model, cfg, inputs, index, time, 0.0)
        assert not perform_backward
        grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters() if p.grad is not None}
        gn = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
        out.append(dict(loss=float(loss), logits=preds.detach().float().cpu(), grad_norm=gn))
        with torch.no_grad():
            for p in model.backbone.parameters():
                p.data.mul_(PERTURB)
        engine.PARAM_EPOCH += 1
    return out


def build_model(device, extra=()):
    cfg = model_cfg(extra)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    model.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, cfg.CONTRASTIVE.QUEUE_LEN,
                                       cfg.CONTRASTIVE.DIM))
    return cfg, model.to(device).train()


def model_bounds():
    """The tolerances model_checks.check_engine uses for slow_tiny: max(tolerance, YARD x the case's yardstick)."""
    from tests import model_checks as mcx
    yard = mcx.autocast_yardstick("slow_tiny") or {}
    b = {k: max(t * mcx.EPS_SCALE, mcx.YARD * yard.get(k, 0.0))
         for k, t in (("logits", 4e-3), ("loss", 1e-3), ("grad_norm", 1e-3), ("grad_global", 1e-2))}
    b["grad_norm"] = max(b["grad_norm"], 0.5 * b["grad_global"] ** 2)
    return b


def check_state_dict(device):
    rec = fixture()["model"]
    cfg, model = build_model(device)
    assert state_list(model.state_dict()) == rec["state"]
    # KNN_ON adds the memory bank
    cfg2 = model_cfg(["CONTRASTIVE.KNN_ON", True, "CONTRASTIVE.LENGTH", 7])
    m2 = sa.MODEL_REGISTRY.get("ContrastiveModel")(cfg2)
    assert tuple(m2.state_dict()["knn_mem.memory"].shape) == (7, 1, 64)
    assert set(m2.state_dict()) - set(model.state_dict()) == {"knn_mem.memory"}
    # a reference-shaped checkpoint loads, and the host mirror of `iter` follows it
    sd = {k: torch.zeros(s, dtype=torch.long if k in ("ptr", "iter") or k.endswith("num_batches_tracked") else torch.float32)
          for k, s in ((k, tuple(s)) for k, s in rec["state"])}
    sd["iter"] = torch.tensor([5])
    model.load_state_dict(sd)
    assert model._iter_host == 5


def check_model(device, report=None):
    rec = fixture()["model"]
    cfg, model = build_model(device)
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    runs = drive(model, cfg, device, ct.contrastive_forward)
    b = model_bounds()
    res = []
    for it, (got, want) in enumerate(zip(runs, rec["iterations"])):
        idx = sample_index(got["logits"].numel(), 100 + it, LOGITS_SAMPLE)
        assert list(got["logits"].shape) == want["logits_shape"]
        ref = torch.tensor(want["logits_sample"])
        r = dict(logits=float((got["logits"].flatten()[idx] - ref).abs().max() / max(want["logits_absmax"], 1e-30)),
                 loss=abs(got["loss"] - want["loss"]) / max(1.0, abs(want["loss"])),
                 grad_norm=abs(got["grad_norm"] - want["grad_norm"]) / want["grad_norm"])
        print("moco tiny model, iteration %d: %s (bounds %s)" % (it, r, b))
        res.append(r)
        for k, v in r.items():
            assert v <= b[k], (it, k, v, b[k])
    if report is not None:
        report["model"] = res
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    # exact: pointer, iteration, which queue rows were written, the key encoder's parameters (an EMA of exact inputs)
    assert int(sd["ptr"]) == rec["ptr"] and int(sd["iter"]) == rec["iter"] and model._iter_host == rec["iter"]
    changed = [int(r) for r in range(sd["queue_x"].shape[0]) if not torch.equal(sd["queue_x"][r], sd0["queue_x"][r])]
    assert changed == rec["queue_rows_written"], changed
    keep = [r for r in range(sd["queue_x"].shape[0]) if r not in changed]
    assert digest(sd["queue_x"][keep]) == rec["queue_unwritten_sha256"]
    rows = sd["queue_x"][changed]
    assert float((rows.pow(2).sum(1).sqrt() - 1).abs().max()) < 1e-5, "enqueued keys are unit rows"
    hist = {k: v for k, v in sd.items() if k.startswith("backbone_hist.") and k in dict(model.named_parameters())}
    assert len(hist) == len(rec["hist_sha256"])
    for k, v in hist.items():
        assert digest(v) == rec["hist_sha256"][k], k


def check_bound_flat_matches_per_tensor(device):
    """bind_flat(): one launch over the flat buffers gives the bits of the per-tensor path; the iteration-0 copy."""
    from slowfast_amd.data_parallel import GradReducer
    from slowfast_amd.optim import construct_optimizer
    outs = []
    for bound in (False, True):
        cfg, model = build_model(device)
        if bound:
            reducer = GradReducer(model)
            opt = construct_optimizer(model, cfg, reducer)
            model.bind_flat(opt)
        names = [n for n, _ in model.backbone_hist.named_parameters()]
        model.mmt = 0.994
        with count_calls() as calls:
            model._update_history()
        assert calls.count("sf_ema_update") == (1 if bound else len(names)), calls
        dist = dict(model.backbone.named_parameters())
        for n, h in model.backbone_hist.named_parameters():     # iteration 0: hist = p first, then the update
            p = dist[n].detach().cpu()
            assert torch.equal(h.detach().cpu(), p * (1.0 - 0.994) + p * 0.994), n
        model._iter_host = 1
        with torch.no_grad():
            for p in model.backbone.parameters():
                p.data.mul_(PERTURB)
        before = {n: h.detach().cpu().clone() for n, h in model.backbone_hist.named_parameters()}
        model.mmt = 0.999
        epoch = engine.PARAM_EPOCH
        model._update_history()
        assert engine.PARAM_EPOCH > epoch
        for n, h in model.backbone_hist.named_parameters():
            assert torch.equal(h.detach().cpu(), dist[n].detach().cpu() * (1.0 - 0.999) + before[n] * 0.999), n
        outs.append({n: h.detach().cpu().clone() for n, h in model.backbone_hist.named_parameters()})
        if bound:
            engine.remove_grad_ready_listener(reducer._listener)
    for n in outs[0]:
        assert torch.equal(outs[0][n], outs[1][n]), n


def check_set_momentum_uploads_on_change(device):
    cfg, model = build_model(device)
    assert model.set_momentum(0.9) and not model.set_momentum(0.9) and model.set_momentum(0.95)
    assert torch.equal(model._mm.cpu(), ct.momentum_words(0.95))
    rec = fixture()["anneal"]
    cfg.SOLVER.MAX_EPOCH = rec["max_epoch"]
    for e, want in rec["values"]:
        model.momentum_anneal_cosine(e)
        assert model.mmt == want, (e, model.mmt, want)


def check_surgery():
    cfg = model_cfg()
    n = cfg.CONTRASTIVE.QUEUE_LEN // cfg.TRAIN.BATCH_SIZE
    flags = [ct.contrastive_parameter_surgery(None, cfg, it / 1000.0, it)[1] for it in range(n + 5)]
    assert flags == [False] * n + [True] * 5, flags
    assert ct.contrastive_parameter_surgery(None, cfg, 1.0, 0)[1] is True


def check_head_single_layer_unchanged(device):
    """ResNetBasicHead with NUM_MLP_LAYERS 1 produces the recorded bits of the parent commit's head (fp32 torch ops)."""
    from slowfast_amd.heads import MLPHead, ResNetBasicHead
    cfg = sa.get_preset("SLOW_8x8_R50", ["MODEL.NUM_CLASSES", 10, "MODEL.DROPOUT_RATE", 0.0])
    torch.manual_seed(3)
    head = ResNetBasicHead([32], 10, [None], cfg=cfg).to(device).train()
    assert isinstance(head.projection, torch.nn.Linear)
    x = torch.randn(2, 32, 2, 3, 3, generator=torch.Generator().manual_seed(4)).to(device)
    got = head([x])
    # what the parent's forward computes: pool -> permute -> Linear on (N, 1, 1, 1, C) -> view
    want = head.projection(x.float().mean((2, 3, 4)).view(2, 1, 1, 1, 32)).view(2, -1)
    assert tuple(got.shape) == (2, 10) and torch.equal(got, want)
    head.eval()
    ev = head([x])
    assert torch.equal(ev, torch.softmax(want.view(2, 1, 1, 1, 10), 4).mean([1, 2, 3]))
    cfg3 = model_cfg()
    h3 = ResNetBasicHead([32], 64, [None], cfg=cfg3)
    assert isinstance(h3.projection, MLPHead) and tuple(h3([x.cpu()]).shape) == (2, 64)
    assert sorted(k for k, _ in h3.named_parameters()) == ["projection.projection.%d.%s" % (i, s) for i in (0, 2, 4)
                                                             for s in ("bias", "weight")]
    cfg4 = model_cfg(["CONTRASTIVE.BN_MLP", True])
    h4 = ResNetBasicHead([32], 64, [None], cfg=cfg4)
    kinds = [type(m).__name__ for m in h4.projection.projection]
    assert kinds == ["Linear", "BatchNorm1d", "ReLU", "Linear", "BatchNorm1d", "ReLU", "Linear"], kinds
    assert h4.projection.projection[0].bias is None and h4.projection.projection[6].bias is not None


REJECTED = ((["CONTRASTIVE.TYPE", "mem"], "CONTRASTIVE.TYPE"), (["CONTRASTIVE.TYPE", "self"], "CONTRASTIVE.TYPE"),
            (["CONTRASTIVE.TYPE", "byol"], "CONTRASTIVE.TYPE"), (["CONTRASTIVE.TYPE", "swav"], "CONTRASTIVE.TYPE"),
            (["CONTRASTIVE.TYPE", "simclr"], "CONTRASTIVE.TYPE"), (["CONTRASTIVE.PREDICTOR_DEPTHS", "[2]"], "PREDICTOR_DEPTHS"),
            (["CONTRASTIVE.BN_SYNC_MLP", True], "BN_SYNC_MLP"), (["NUM_GPUS", 2], "NUM_GPUS"), (["NUM_SHARDS", 2], "NUM_GPUS"),
            (["MODEL.ARCH", "x3d"], "MODEL.ARCH"), (["MODEL.ARCH", "mvit"], "MODEL.ARCH"))


def check_rejections():
    for extra, key in REJECTED:
        try:
            sa.MODEL_REGISTRY.get("ContrastiveModel")(model_cfg(extra))
        except NotImplementedError as e:
            assert key in str(e), (extra, str(e))
        else:
            raise AssertionError("%r accepted" % (extra,))
    assert isinstance(sa.get_loss_func("contrastive_loss")(reduction="mean"), torch.nn.Module)
    lg = torch.randn(5, 9)
    assert torch.equal(sa.get_loss_func("contrastive_loss")()(lg),
                       torch.nn.functional.cross_entropy(lg, torch.zeros(5, dtype=torch.long)))


# ------------------------------------------------------------------------------------------------ capture (GPU)
def check_capture(device, n=8, V=2, K=64, C=64, size=4097, iters=3):
    """EMA -> loss -> backward of the loss -> enqueue on one stream, captured once and replayed with a new momentum each
    time, against the same three iterations run eagerly: queue, pointer, hist, loss and df bit for bit."""
    f0, keys, queue0, T = nce_inputs(n, V, K, C)
    p0, h0 = ema_inputs(size)
    ms = (0.5, 0.994, 0.999)

    def state():
        return dict(f=f0.to(device).requires_grad_(True), keys=keys.to(device), queue=queue0.to(device), p=p0.to(device),
                    h=h0.to(device), ptr=torch.zeros(1, dtype=torch.int64, device=device),
                    err=torch.zeros(1, dtype=torch.int32, device=device), mm=ct.momentum_words(ms[0]).to(device))

    def step(s):
        ct.ema_update(s["p"], s["h"], s["mm"])
        logits, loss = ct.moco_nce(s["f"], s["keys"], s["queue"], T)
        (df,) = torch.autograd.grad(loss, s["f"])
        ct.enqueue(s["queue"], s["ptr"], [s["keys"][v] for v in range(V)], s["err"])
        return loss, df

    eager, e_out = state(), []
    for it in range(iters):
        eager["mm"].copy_(ct.momentum_words(ms[it]).to(device))
        loss, df = step(eager)
        e_out.append((loss.detach().clone(), df.clone()))
    cap = state()
    ct._workspace(device, n, V, K, C)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):          # warm-up off the default stream, then restore the state it touched
        step(cap)
    torch.cuda.current_stream(device).wait_stream(side)
    cap["queue"].copy_(queue0.to(device)), cap["h"].copy_(h0.to(device)), cap["ptr"].zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_loss, c_df = step(cap)
    cap["queue"].copy_(queue0.to(device)), cap["h"].copy_(h0.to(device)), cap["ptr"].zero_()
    for it in range(iters):
        cap["mm"].copy_(ct.momentum_words(ms[it]).to(device))
        graph.replay()
        assert torch.equal(c_loss, e_out[it][0]) and torch.equal(c_df, e_out[it][1]), it
    torch.cuda.synchronize(device)
    for k in ("queue", "ptr", "h", "err"):
        assert torch.equal(cap[k], eager[k]), k
    assert int(cap["err"]) == 0
