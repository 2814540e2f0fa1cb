"""CPU: per-element fp64 parity of the fused attention kernels (csrc/sf_attn.h) through the host functional simulator."""
import pytest

from tests import attn_elem_checks as ac

# 1024 (batch, head) pairs of several key chunks take minutes in the simulator: those twins carry the ``slow`` marker
SLOW = {"D96_129q_33k", "D32_R34_272k", "QT2"}


def _params(cases):
    return [pytest.param(c, id=c[0], marks=[pytest.mark.slow] if c[0] in SLOW else []) for c in cases]


@pytest.mark.parametrize("case", _params(ac.TWO_TILE_CASES))
def test_attn_two_tiles(sim, case):
    ac.check_attn(sim, *case[1:])


@pytest.mark.parametrize("case", _params(ac.EDGE_CASES))
def test_attn_edges(sim, case):
    ac.check_attn(sim, *case[1:])


@pytest.mark.parametrize("case", _params(ac.RESCALE_CASES))
def test_attn_rescale(sim, case):
    ac.check_attn_rescale(sim, *case[1:])


def test_attn_rejects(sim):
    ac.check_attn_rejects(sim)
