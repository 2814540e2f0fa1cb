"""GPU (-m gpu): per-element fp64 parity of the fused attention kernels (csrc/sf_attn.h) on a real MI355X."""
import pytest

from tests import attn_elem_checks as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ac.TWO_TILE_CASES, ids=[c[0] for c in ac.TWO_TILE_CASES])
def test_attn_two_tiles(gpu, case):
    ac.check_attn(gpu, *case[1:])


@pytest.mark.parametrize("case", ac.EDGE_CASES, ids=[c[0] for c in ac.EDGE_CASES])
def test_attn_edges(gpu, case):
    ac.check_attn(gpu, *case[1:])


@pytest.mark.parametrize("case", ac.RESCALE_CASES, ids=[c[0] for c in ac.RESCALE_CASES])
def test_attn_rescale(gpu, case):
    ac.check_attn_rescale(gpu, *case[1:])


def test_attn_rejects(gpu):
    ac.check_attn_rejects(gpu)
