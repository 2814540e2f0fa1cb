"""CPU: per-element fp64 parity of the convolution family (csrc/sf_igemm.h, sf_igemm2.h, sf_wgrad2.h, sf_stem.h and their launchers)
through the host functional simulator.  Method, bounds and the restated dispatch: tests/conv_elem_checks.py."""
import pytest

from tests import conv_elem_checks as cc


@pytest.mark.parametrize("case", cc.FWD_CASES, ids=cc.ids(cc.FWD_CASES))
def test_conv_fwd_elem(sim, monkeypatch, case):
    cc.run_case(sim, monkeypatch, case)


@pytest.mark.parametrize("case", cc.FUSED_CASES, ids=cc.ids(cc.FUSED_CASES))
def test_conv_fwd_fused_elem(sim, monkeypatch, case):
    cc.run_case(sim, monkeypatch, case)


@pytest.mark.parametrize("case", cc.DGRAD_CASES, ids=cc.ids(cc.DGRAD_CASES))
def test_conv_dgrad_elem(sim, monkeypatch, case):
    cc.run_case(sim, monkeypatch, case)


@pytest.mark.parametrize("case", cc.WGRAD_CASES, ids=cc.ids(cc.WGRAD_CASES))
def test_conv_wgrad_elem(sim, monkeypatch, case):
    cc.run_case(sim, monkeypatch, case)


def test_linear_t128_tile(sim, monkeypatch):
    for key, v in dict(cc.V2, SF_IGEMM2_T128="2").items():
        monkeypatch.setenv(key, v)
    cc.check_linear_t128(sim)


def test_conv_rejects(sim, monkeypatch):
    for key in cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("SF_WGRAD2", "1")            # check_rejects lowers the weight-gradient thresholds: restored by monkeypatch
    for key in cc.W2:
        monkeypatch.setenv(key, cc.W2[key])
    cc.check_rejects(sim)


def test_trace_lines_match_the_restated_plans(sim):
    cc.check_trace("sim")
