"""CPU: the grouped (1,3,3) convolution on block-diagonal bundles (csrc/sf_gconv.h, sf_gconv_* of sf_api.hip, engine.GroupedConvUnit)
through the host functional simulator.  Method, bounds and cases: tests/gconv_checks.py."""
import pytest

from tests import conv_elem_checks as cc
from tests import gconv_checks as gc

CASES = pytest.mark.parametrize("case", gc.KERNEL_CASES, ids=[gc.case_id(c) for c in gc.KERNEL_CASES])


@pytest.mark.parametrize("C,Cg", [(64, 4), (64, 8), (64, 16), (64, 32), (128, 64), (128, 4)])
def test_gconv_prep_bits(sim, C, Cg):
    gc.check_prep(sim, C, Cg)


@CASES
def test_gconv_fwd_elem(sim, case):
    gc.check_fwd(sim, *case)


def test_gconv_fwd_forms(sim):
    gc.check_fwd(sim, 64, 8, 1, 1, stats=False)
    gc.check_fwd(sim, 64, 8, 1, 1, stats=False, bias=True, relu=True)                  # the eval form
    gc.check_fwd(sim, 128, 64, 1, 1, stats=False, bias=True, relu=True)
    gc.check_fwd(sim, 64, 16, 1, 1, xpad=16, xoff=8, ypad=8)                            # channel-slice views of wider buffers
    gc.check_fwd(sim, 128, 64, 2, 1, xpad=8, ypad=24, bias=True)


@CASES
def test_gconv_dgrad_elem(sim, case):
    gc.check_dgrad(sim, *case)


def test_gconv_dgrad_forms(sim):
    gc.check_dgrad(sim, 64, 8, 2, 1, dypad=8, xpad=16)
    gc.check_dgrad(sim, 128, 64, 2, 1)
    gc.check_dgrad(sim, 64, 4, 2, 2)                # residue classes without any tap store zeros


@CASES
def test_gconv_wgrad_elem(sim, monkeypatch, case):
    for key in cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    gc.check_wgrad(sim, *case)


def test_gconv_wgrad_forms(sim, monkeypatch):
    for key in cc.KNOBS:
        monkeypatch.delenv(key, raising=False)
    gc.check_wgrad(sim, 64, 8, 1, 1, out_scale=0.37, accumulate=True, xpad=8, dypad=16, want="wgrad_bmw32")
    gc.check_wgrad(sim, 64, 8, 1, 1, out_scale=-2.5)
    gc.check_wgrad(sim, 64, 16, 1, 1, zero_group=2)
    gc.check_wgrad(sim, 128, 64, 1, 1, zero_group=1, want="wgrad_bmw64")
    # the bundles on the row-table kernels the full-size layers take (thresholds lowered as conv_elem_checks lowers them)
    for key, v in cc.W2T.items():
        monkeypatch.setenv(key, v)
    gc.check_wgrad(sim, 64, 8, 1, 1, accumulate=True, xpad=8, want="wgrad2t_32_128")
    gc.check_wgrad(sim, 64, 4, 2, 1, want="wgrad2t_32_128")
    gc.check_wgrad(sim, 128, 64, 1, 1, out_scale=0.5, dypad=8, want="wgrad2_single_64")
    gc.check_wgrad(sim, 128, 64, 1, 2, want="wgrad2_single_64")


def test_gconv_rejects(sim):
    gc.check_rejects(sim)


def test_builder_rejects():
    gc.check_builder_rejects()


def test_grouped_unit_contract(sim):
    gc.check_unit_contract(sim)


def test_grouped_block_projection_stride2(sim):
    gc.check_block(sim, 128, 256, 2, (2, 128, 2, 16, 16))


def test_grouped_block_identity(sim):
    gc.check_block(sim, 256, 256, 1, (2, 256, 2, 8, 8))


def test_grouped_model_train(sim):
    gc.check_model(sim)


def test_grouped_model_eval_fused(sim):
    gc.check_model_eval(sim)


def test_resnext_contract_recorded(sim):
    """tests/golden/resnext_contract.json (the unmodified reference, tools/make_resnext_golden.py) against the drop-in's state_dict
    and the dense-equivalent oracle."""
    from tests import model_checks as mc
    gc.check_contract(mc.load_golden(gc.CONTRACT))


def test_resnext_contract_live_reference(sim):
    """The same against the reference tree itself, where it is present."""
    from oracle import refshim
    if not refshim.available():
        pytest.skip("reference tree not present")
    rec = gc.reference_record()
    gc.check_contract(rec)
    from tests import model_checks as mc
    gold = mc.load_golden(gc.CONTRACT)
    assert rec["state_dict"] == gold["state_dict"] and abs(rec["loss"] - gold["loss"]) < 1e-5 * max(1.0, abs(gold["loss"]))
