"""GPU (-m gpu): per-element fp64 parity of the token-space kernels (csrc/sf_tokens.h) on a real MI355X."""
import pytest

from tests import token_elem_checks as tc

pytestmark = pytest.mark.gpu

SM_IDS = [c[0] for c in tc.SOFTMAX_CASES]
RP_IDS = [c[0] for c in tc.RELPOS_CASES]
SUMS = [(False, None), (None, True), (False, False), (True, False)]
SUMS_IDS = ["resid", "dx-acc", "both", "both-mixed"]


@pytest.mark.parametrize("C", tc.LN_WIDTHS)
def test_ln_fwd_widths(gpu, C):
    rpp = tc.ln_rows_per_pass(C)
    for M in (1, rpp - 1, rpp + 1):
        tc.check_layernorm_fwd(gpu, M, C, hard=True)


@pytest.mark.parametrize("C", [8, 264, 768, 1024])
def test_ln_fwd_pitched_no_stats(gpu, C):
    tc.check_layernorm_fwd(gpu, 37, C, ld_extra=16, hard=True)
    tc.check_layernorm_fwd(gpu, 37, C, ld_extra=8, save_stats=False)


def test_ln_fwd_grid_stride(gpu):
    tc.check_layernorm_fwd(gpu, *tc.LN_GRID_STRIDE, hard=True)


def test_ln_rejects(gpu):
    tc.check_layernorm_rejects(gpu)


@pytest.mark.parametrize("C", tc.LN_WIDTHS)
def test_ln_bwd_widths(gpu, C):
    rpb = 256 // tc.ln_template(C, False)[0]
    tc.check_layernorm_bwd(gpu, 1, C, resid=False)
    tc.check_layernorm_bwd(gpu, 3 * rpb + 1, C, resid=True, sums=(False, False))          # ragged last rows


def test_ln_bwd_two_passes(gpu):
    tc.check_layernorm_bwd(gpu, *tc.LN_BWD_TWO_PASSES, resid=True, sums=(False, True))


@pytest.mark.parametrize("sums", SUMS, ids=SUMS_IDS)
@pytest.mark.parametrize("C", [96, 1024])
def test_ln_bwd_sums(gpu, C, sums):
    tc.check_layernorm_bwd(gpu, 1000, C, resid=True, sums=sums)


@pytest.mark.parametrize("C", [136, 776])
def test_ln_bwd_pitched_accumulate(gpu, C):
    tc.check_layernorm_bwd(gpu, 531, C, resid=True, ld_extra=24, accumulate=True, sums=(True, True))
    tc.check_layernorm_bwd(gpu, 531, C, resid=False, ld_extra=8, accumulate=True, sums=(None, False))


@pytest.mark.parametrize("C", tc.COLSUM_WIDTHS)
def test_bias_grad_widths(gpu, C):
    tc.check_bias_grad(gpu, 1, C)
    tc.check_bias_grad(gpu, 517, C, ld_extra=8)
    tc.check_bias_grad(gpu, 517, C, accumulate=True)


def test_bias_grad_fold(gpu):
    tc.check_bias_grad(gpu, 300, 128, fold=32)
    tc.check_bias_grad(gpu, 300, 128, fold=32, accumulate=True, ld_extra=16)


@pytest.mark.parametrize("C,passes,last", [(8, 3, 2), (56, 6, 5), (2048, 9, 8)])
def test_bias_grad_rows_per_thread(gpu, C, passes, last):
    tc.check_bias_grad(gpu, tc.colsum_rows_for(C, passes, last), C)


@pytest.mark.parametrize("nblk", tc.FIN_NBLK)
def test_colsum_finalize(gpu, nblk):
    tc.check_colsum_finalize(gpu, nblk)
    tc.check_colsum_finalize(gpu, nblk, C=128, fold=32, scale=0.25, accumulate=True)
    tc.check_colsum_finalize(gpu, nblk, outs=(True, False), scale=-3.0)
    tc.check_colsum_finalize(gpu, nblk, outs=(False, True), accumulate=True)
    if nblk <= 2048:
        tc.check_colsum_finalize(gpu, nblk, row_stride=2, scale=0.5)


def test_finalize_batch(gpu):
    tc.check_finalize_batch(gpu)


def test_deferred_finalizes(gpu):
    tc.check_deferred_finalizes(gpu)


def test_gelu_exhaustive(gpu):
    tc.check_gelu_exhaustive(gpu)


def test_gelu_small_and_rejects(gpu):
    tc.check_gelu_small_and_rejects(gpu)


def test_gelu_grid_stride(gpu):
    tc.check_gelu_grid_stride(gpu)


@pytest.mark.parametrize("case", tc.SOFTMAX_CASES, ids=SM_IDS)
def test_softmax(gpu, case):
    tc.check_softmax(gpu, *case[1:])


def test_softmax_rejects(gpu):
    tc.check_softmax_rejects(gpu)


@pytest.mark.parametrize("D,rows", [(32, (5, 9, 3)), (96, (13, 13, 15)), (96, (27, 27, 15))], ids=["D32", "D96", "D96-69rows"])
def test_relpos_tables(gpu, D, rows):
    tc.check_relpos_tables(gpu, D, rows)


@pytest.mark.parametrize("case", tc.RELPOS_CASES, ids=RP_IDS)
def test_relpos_gather_scatter(gpu, case):
    tc.check_relpos_gather_scatter(gpu, *case[1:])


def test_relpos_rejects(gpu):
    tc.check_relpos_rejects(gpu)


def test_transpose_heads(gpu):
    tc.check_transpose_heads(gpu)
    tc.check_transpose_heads(gpu, B=1, Nk=8, heads=2, D=16, ldk=8)


@pytest.mark.parametrize("resid", [True, False], ids=["resid", "no-resid"])
def test_row_scale_add(gpu, resid):
    tc.check_row_scale_add(gpu, 5, 7, 40, resid)
    tc.check_row_scale_add(gpu, 3, 50, 8, resid, ld_extra=8)
