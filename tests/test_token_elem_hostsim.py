"""CPU: per-element fp64 parity of the token-space kernels (csrc/sf_tokens.h) through the host functional simulator."""
import pytest

from tests import token_elem_checks as tc

SM_IDS = [c[0] for c in tc.SOFTMAX_CASES]
RP_IDS = [c[0] for c in tc.RELPOS_CASES]
SUMS = [(False, None), (None, True), (False, False), (True, False)]
SUMS_IDS = ["resid", "dx-acc", "both", "both-mixed"]


@pytest.mark.parametrize("C", tc.LN_WIDTHS)
def test_ln_fwd_widths(sim, C):
    rpp = tc.ln_rows_per_pass(C)
    for M in (1, rpp - 1, rpp + 1):
        tc.check_layernorm_fwd(sim, M, C, hard=True)


@pytest.mark.parametrize("C", [8, 264, 768, 1024])
def test_ln_fwd_pitched_no_stats(sim, C):
    tc.check_layernorm_fwd(sim, 37, C, ld_extra=16, hard=True)
    tc.check_layernorm_fwd(sim, 37, C, ld_extra=8, save_stats=False)


def test_ln_fwd_grid_stride(sim):
    tc.check_layernorm_fwd(sim, *tc.LN_GRID_STRIDE, hard=True)


def test_ln_rejects(sim):
    tc.check_layernorm_rejects(sim)


@pytest.mark.parametrize("C", tc.LN_WIDTHS)
def test_ln_bwd_widths(sim, C):
    rpb = 256 // tc.ln_template(C, False)[0]
    tc.check_layernorm_bwd(sim, 1, C, resid=False)
    tc.check_layernorm_bwd(sim, 3 * rpb + 1, C, resid=True, sums=(False, False))          # ragged last rows


def test_ln_bwd_two_passes(sim):
    tc.check_layernorm_bwd(sim, *tc.LN_BWD_TWO_PASSES, resid=True, sums=(False, True))


@pytest.mark.parametrize("sums", SUMS, ids=SUMS_IDS)
@pytest.mark.parametrize("C", [96, 1024])
def test_ln_bwd_sums(sim, C, sums):
    tc.check_layernorm_bwd(sim, 1000, C, resid=True, sums=sums)


@pytest.mark.parametrize("C", [136, 776])
def test_ln_bwd_pitched_accumulate(sim, C):
    tc.check_layernorm_bwd(sim, 531, C, resid=True, ld_extra=24, accumulate=True, sums=(True, True))
    tc.check_layernorm_bwd(sim, 531, C, resid=False, ld_extra=8, accumulate=True, sums=(None, False))


@pytest.mark.parametrize("C", tc.COLSUM_WIDTHS)
def test_bias_grad_widths(sim, C):
    tc.check_bias_grad(sim, 1, C)
    tc.check_bias_grad(sim, 517, C, ld_extra=8)
    tc.check_bias_grad(sim, 517, C, accumulate=True)


def test_bias_grad_fold(sim):
    tc.check_bias_grad(sim, 300, 128, fold=32)
    tc.check_bias_grad(sim, 300, 128, fold=32, accumulate=True, ld_extra=16)


@pytest.mark.parametrize("C,passes,last", [(8, 3, 2), (56, 6, 5), (2048, 9, 8)])
def test_bias_grad_rows_per_thread(sim, C, passes, last):
    tc.check_bias_grad(sim, tc.colsum_rows_for(C, passes, last), C)


@pytest.mark.parametrize("nblk", tc.FIN_NBLK)
def test_colsum_finalize(sim, nblk):
    tc.check_colsum_finalize(sim, nblk)
    tc.check_colsum_finalize(sim, nblk, C=128, fold=32, scale=0.25, accumulate=True)
    tc.check_colsum_finalize(sim, nblk, outs=(True, False), scale=-3.0)
    tc.check_colsum_finalize(sim, nblk, outs=(False, True), accumulate=True)
    if nblk <= 2048:
        tc.check_colsum_finalize(sim, nblk, row_stride=2, scale=0.5)


def test_finalize_batch(sim):
    tc.check_finalize_batch(sim)


def test_deferred_finalizes(sim):
    tc.check_deferred_finalizes(sim)


def test_gelu_exhaustive(sim):
    tc.check_gelu_exhaustive(sim)


def test_gelu_small_and_rejects(sim):
    tc.check_gelu_small_and_rejects(sim)


def test_gelu_grid_stride(sim):
    tc.check_gelu_grid_stride(sim)


@pytest.mark.parametrize("case", tc.SOFTMAX_CASES, ids=SM_IDS)
def test_softmax(sim, case):
    tc.check_softmax(sim, *case[1:])


def test_softmax_rejects(sim):
    tc.check_softmax_rejects(sim)


@pytest.mark.parametrize("D,rows", [(32, (5, 9, 3)), (96, (13, 13, 15)), (96, (27, 27, 15))], ids=["D32", "D96", "D96-69rows"])
def test_relpos_tables(sim, D, rows):
    tc.check_relpos_tables(sim, D, rows)


@pytest.mark.parametrize("case", tc.RELPOS_CASES, ids=RP_IDS)
def test_relpos_gather_scatter(sim, case):
    tc.check_relpos_gather_scatter(sim, *case[1:])


def test_relpos_rejects(sim):
    tc.check_relpos_rejects(sim)


def test_transpose_heads(sim):
    tc.check_transpose_heads(sim)
    tc.check_transpose_heads(sim, B=1, Nk=8, heads=2, D=16, ldk=8)


@pytest.mark.parametrize("resid", [True, False], ids=["resid", "no-resid"])
def test_row_scale_add(sim, resid):
    tc.check_row_scale_add(sim, 5, 7, 40, resid)
    tc.check_row_scale_add(sim, 3, 50, 8, resid, ld_extra=8)
