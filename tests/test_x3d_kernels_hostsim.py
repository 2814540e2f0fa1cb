"""CPU: the X3D SE / gate kernels (csrc/sf_x3d.h), each entry point on its own, through the host functional simulator."""
import pytest

from tests import x3d_checks as xc

ROW_IDS = [r[0] for r in xc.ROWS]
MODE_IDS = ["gate-swish", "gate-relu", "nogate-swish", "nogate-relu"]


@pytest.mark.parametrize("relu,affine", [(False, True), (True, True), (False, False), (True, False)],
                         ids=["affine", "affine-relu", "raw", "raw-relu"])
@pytest.mark.parametrize("row", xc.ROWS, ids=ROW_IDS)
def test_x3d_sample_mean(sim, row, relu, affine):
    _, N, C, S, ld_extra = row
    xc.check_sample_mean(sim, N, C, S, relu, affine, ld_extra)


@pytest.mark.parametrize("gated,swish", xc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("row", xc.ROWS, ids=ROW_IDS)
def test_x3d_gate_act(sim, row, gated, swish):
    _, N, C, S, ld_extra = row
    xc.check_gate_act(sim, N, C, S, gated, swish, gated, ld_extra)


@pytest.mark.parametrize("gated,swish", [(True, True), (False, False)], ids=["gate-swish", "nogate-relu"])
def test_x3d_gate_act_two_row_passes(sim, gated, swish):
    _, N, C, S, ld_extra = xc.BIG_ROW
    xc.check_gate_act(sim, N, C, S, gated, swish, gated, ld_extra)


@pytest.mark.parametrize("gated,swish", xc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("row", xc.ROWS, ids=ROW_IDS)
def test_x3d_gate_sums(sim, row, gated, swish):
    _, N, C, S, ld_extra = row
    xc.check_gate_sums(sim, N, C, S, gated, swish, ld_extra)


@pytest.mark.parametrize("case", xc.SE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_x3d_se_gate(sim, case):
    xc.check_se_gate(sim, *case)


def test_x3d_se_gate_limits(sim):
    xc.check_se_limits(sim)


@pytest.mark.parametrize("case", xc.OUTER_CASES, ids=lambda c: "x".join(map(str, c[:3])) + ("-b" if c[3] else "") + ("-acc" if c[4] else ""))
def test_x3d_outer_sum(sim, case):
    xc.check_outer_sum(sim, *case)


@pytest.mark.parametrize("row", [r for r in xc.ROWS if r[4] == 0] + [xc.BIG_ROW], ids=lambda r: r[0])
def test_x3d_bn_apply_sample(sim, row):
    _, N, C, S, _ = row
    xc.check_bn_apply_sample(sim, N, C, S)


@pytest.mark.parametrize("case", xc.CHAIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_x3d_se_chain(sim, monkeypatch, case):
    xc.check_se_chain(sim, monkeypatch, *case)
