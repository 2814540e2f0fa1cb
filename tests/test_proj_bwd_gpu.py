"""GPU (-m gpu): per-element fp64 parity of sf_conv_proj_bwd (csrc/sf_cbwd.h) on a real MI355X, against the host replica of the rounded
dy and, bit for bit, against the three launches it replaces; its planner; the first block of a stage, default against SF_CBWD=0.
Method and bounds: tests/proj_bwd_checks.py."""
import pytest

from tests import proj_bwd_checks as pb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", pb.CASES, ids=pb.ids(pb.CASES))
def test_conv_proj_bwd_elem(gpu, monkeypatch, case):
    pb.run_case(gpu, monkeypatch, case)


def test_conv_proj_bwd_planner(gpu, monkeypatch):
    pb.check_planner(gpu, monkeypatch)


@pytest.mark.parametrize("case", pb.BLOCKS, ids=pb.ids(pb.BLOCKS))
def test_first_block_backward(gpu, monkeypatch, case):
    pb.run_block(gpu, monkeypatch, case)
