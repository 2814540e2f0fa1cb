"""GPU (-m gpu): per-element fp64 parity of the convolution family (csrc/sf_igemm.h, sf_igemm2.h, sf_wgrad2.h, sf_stem.h and their
launchers) on a real MI355X: the host-simulator cases under the same lowered thresholds, and the product's own thresholds unforced.
Method, bounds and the restated dispatch: tests/conv_elem_checks.py."""
import pytest

from tests import conv_elem_checks as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cc.FWD_CASES, ids=cc.ids(cc.FWD_CASES))
def test_conv_fwd_elem(gpu, monkeypatch, case):
    cc.run_case(gpu, monkeypatch, case)


@pytest.mark.parametrize("case", cc.FUSED_CASES, ids=cc.ids(cc.FUSED_CASES))
def test_conv_fwd_fused_elem(gpu, monkeypatch, case):
    cc.run_case(gpu, monkeypatch, case)


@pytest.mark.parametrize("case", cc.DGRAD_CASES, ids=cc.ids(cc.DGRAD_CASES))
def test_conv_dgrad_elem(gpu, monkeypatch, case):
    cc.run_case(gpu, monkeypatch, case)


@pytest.mark.parametrize("case", cc.WGRAD_CASES, ids=cc.ids(cc.WGRAD_CASES))
def test_conv_wgrad_elem(gpu, monkeypatch, case):
    cc.run_case(gpu, monkeypatch, case)


@pytest.mark.parametrize("case", cc.UNFORCED_CASES, ids=cc.ids(cc.UNFORCED_CASES))
def test_unforced_dispatch(gpu, monkeypatch, case):
    cc.run_case(gpu, monkeypatch, case)


def test_linear_t128_tile(gpu, monkeypatch):
    for key, v in dict(cc.V2, SF_IGEMM2_T128="2").items():
        monkeypatch.setenv(key, v)
    cc.check_linear_t128(gpu)


def test_conv_rejects(gpu, monkeypatch):
    for key in cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key in cc.W2:
        monkeypatch.setenv(key, cc.W2[key])
    cc.check_rejects(gpu)


def test_trace_lines_match_the_restated_plans(gpu):
    cc.check_trace("gpu")
