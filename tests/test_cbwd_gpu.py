"""GPU (-m gpu): per-element fp64 parity of sf_conv_c_bwd (csrc/sf_cbwd.h) on a real MI355X, against the host replica of the rounded
dy and against the three launches it replaces.  Method and bounds: tests/cbwd_checks.py."""
import pytest

from tests import cbwd_checks as cb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cb.CASES, ids=cb.ids(cb.CASES))
def test_conv_c_bwd_elem(gpu, monkeypatch, case):
    cb.run_case(gpu, monkeypatch, case)


def test_conv_c_bwd_planner(gpu, monkeypatch):
    cb.check_rejects(gpu, monkeypatch)
