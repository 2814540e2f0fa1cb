"""CPU: per-element fp64 parity of sf_conv_proj_bwd (csrc/sf_cbwd.h) through the host functional simulator, against the host replica of
the rounded dy and, bit for bit, against the three launches it replaces; its planner; the first block of a stage, default against
SF_CBWD=0.  Method and bounds: tests/proj_bwd_checks.py."""
import pytest

from tests import proj_bwd_checks as pb


@pytest.mark.parametrize("case", pb.CASES, ids=pb.ids(pb.CASES))
def test_conv_proj_bwd_elem(sim, monkeypatch, case):
    pb.run_case(sim, monkeypatch, case)


def test_conv_proj_bwd_planner(sim, monkeypatch):
    pb.check_planner(sim, monkeypatch)


@pytest.mark.parametrize("case", pb.BLOCKS, ids=pb.ids(pb.BLOCKS))
def test_first_block_backward(sim, monkeypatch, case):
    pb.run_block(sim, monkeypatch, case)
