"""CPU: per-element fp64 parity of sf_conv_c_bwd (csrc/sf_cbwd.h) through the host functional simulator, against the host replica
of the rounded dy and against the three launches it replaces.  Method and bounds: tests/cbwd_checks.py."""
import pytest

from tests import cbwd_checks as cb


@pytest.mark.parametrize("case", cb.CASES, ids=cb.ids(cb.CASES))
def test_conv_c_bwd_elem(sim, monkeypatch, case):
    cb.run_case(sim, monkeypatch, case)


def test_conv_c_bwd_planner(sim, monkeypatch):
    cb.check_rejects(sim, monkeypatch)
