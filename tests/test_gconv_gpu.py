"""GPU (-m gpu): the grouped (1,3,3) convolution on block-diagonal bundles (csrc/sf_gconv.h, sf_gconv_* of sf_api.hip,
engine.GroupedConvUnit) on a real MI355X: the host-simulator cases, and one TrainStep iteration eager against captured.
Method, bounds and cases: tests/gconv_checks.py."""
import pytest

from tests import conv_elem_checks as cc
from tests import gconv_checks as gc

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("case", gc.KERNEL_CASES, ids=[gc.case_id(c) for c in gc.KERNEL_CASES])


@pytest.mark.parametrize("C,Cg", [(64, 4), (64, 8), (64, 16), (64, 32), (128, 64), (128, 4)])
def test_gconv_prep_bits(gpu, C, Cg):
    gc.check_prep(gpu, C, Cg)


@CASES
def test_gconv_fwd_elem(gpu, case):
    gc.check_fwd(gpu, *case)


def test_gconv_fwd_forms(gpu):
    gc.check_fwd(gpu, 64, 8, 1, 1, stats=False)
    gc.check_fwd(gpu, 64, 8, 1, 1, stats=False, bias=True, relu=True)                  # the eval form
    gc.check_fwd(gpu, 128, 64, 1, 1, stats=False, bias=True, relu=True)
    gc.check_fwd(gpu, 64, 16, 1, 1, xpad=16, xoff=8, ypad=8)                            # channel-slice views of wider buffers
    gc.check_fwd(gpu, 128, 64, 2, 1, xpad=8, ypad=24, bias=True)


@CASES
def test_gconv_dgrad_elem(gpu, case):
    gc.check_dgrad(gpu, *case)


def test_gconv_dgrad_forms(gpu):
    gc.check_dgrad(gpu, 64, 8, 2, 1, dypad=8, xpad=16)
    gc.check_dgrad(gpu, 128, 64, 2, 1)
    gc.check_dgrad(gpu, 64, 4, 2, 2)                # residue classes without any tap store zeros


@CASES
def test_gconv_wgrad_elem(gpu, monkeypatch, case):
    for key in cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    gc.check_wgrad(gpu, *case)


def test_gconv_wgrad_forms(gpu, monkeypatch):
    for key in cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    gc.check_wgrad(gpu, 64, 8, 1, 1, out_scale=0.37, accumulate=True, xpad=8, dypad=16, want="wgrad_bmw32")
    gc.check_wgrad(gpu, 64, 8, 1, 1, out_scale=-2.5)
    gc.check_wgrad(gpu, 64, 16, 1, 1, zero_group=2)
    gc.check_wgrad(gpu, 128, 64, 1, 1, zero_group=1, want="wgrad_bmw64")
    # the bundles on the row-table kernels the full-size layers take (thresholds lowered as conv_elem_checks lowers them)
    for key, v in cc.W2T.items():
        monkeypatch.setenv(key, v)
    gc.check_wgrad(gpu, 64, 8, 1, 1, accumulate=True, xpad=8, want="wgrad2t_32_128")
    gc.check_wgrad(gpu, 64, 4, 2, 1, want="wgrad2t_32_128")
    gc.check_wgrad(gpu, 128, 64, 1, 1, out_scale=0.5, dypad=8, want="wgrad2_single_64")
    gc.check_wgrad(gpu, 128, 64, 1, 2, want="wgrad2_single_64")


def test_gconv_rejects(gpu):
    gc.check_rejects(gpu)


def test_grouped_unit_contract(gpu):
    gc.check_unit_contract(gpu)


def test_grouped_block_projection_stride2(gpu):
    gc.check_block(gpu, 128, 256, 2, (2, 128, 2, 16, 16))


def test_grouped_block_identity(gpu):
    gc.check_block(gpu, 256, 256, 1, (2, 256, 2, 8, 8))


def test_grouped_model_train(gpu):
    gc.check_model(gpu)


def test_grouped_model_eval_fused(gpu):
    gc.check_model_eval(gpu)


def test_grouped_train_step_graph_matches_eager(gpu):
    gc.check_train_step(gpu)
