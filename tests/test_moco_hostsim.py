"""CPU (host functional simulator): the MoCo step glue -- csrc/sf_moco.h kernels per element against fp64, the ContrastiveModel
against the recorded reference.  Checks in tests/moco_checks.py; the same ones run on the MI355X in tests/test_moco_gpu.py."""
import pytest

from tests import moco_checks as checks


def test_reference_stays_inside_the_bounds():
    checks.check_reference_inside_bounds()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("scale", checks.L2_SCALES)
@pytest.mark.parametrize("n,C", checks.L2_CASES)
def test_l2norm_rows(sim, n, C, scale, with_perm, padded):
    ratio = checks.check_l2norm(sim, n, C, scale, with_perm, padded)
    assert checks.fixture()["l2norm"]["n%d_C%d_s%g" % (n, C, scale)] <= 1.0 and ratio <= 1.0


def test_l2norm_zero_row_and_bad_perm(sim):
    checks.check_l2norm_zero_row_and_bad_perm(sim)


@pytest.mark.parametrize("grad_out", [1.0, 1024.0])
@pytest.mark.parametrize("n,V,K", checks.NCE_SHAPES)
@pytest.mark.parametrize("C", checks.NCE_C)
def test_moco_nce(sim, C, n, V, K, grad_out):
    checks.check_nce(sim, n, V, K, C, "randn", grad_out)


@pytest.mark.parametrize("kind", checks.NCE_KINDS[1:])
@pytest.mark.parametrize("n,V,K,C", [(3, 3, 96, 64), (8, 3, 4096, 128)])
def test_moco_nce_adversarial(sim, n, V, K, C, kind):
    checks.check_nce(sim, n, V, K, C, kind)


def test_moco_nce_rejections(sim):
    checks.check_nce_rejections(sim)


@pytest.mark.parametrize("views,multi_view,start", [(3, True, 0), (1, True, 0), (3, False, 0), (3, False, 8), (1, True, 4)])
def test_enqueue(sim, views, multi_view, start):
    p = checks.check_enqueue(sim, views, multi_view, start)
    if views == 3 and multi_view:
        assert p == 0           # 0 -> 4 -> 8 -> 0


def test_enqueue_bad_pointer_is_a_noop(sim):
    checks.check_enqueue_bad_pointer(sim)


@pytest.mark.parametrize("m", checks.EMA_M)
@pytest.mark.parametrize("n", checks.EMA_SIZES)
def test_ema_update(sim, n, m):
    checks.check_ema(sim, n, m)


def test_state_dict_contract(sim):
    checks.check_state_dict(sim)


@pytest.mark.slow       # 80 s on the simulator (24 clips through two ResNet-18s, twice); runs on the MI355X in test_moco_gpu.py
def test_tiny_model_two_iterations(sim):
    checks.check_model(sim)


def test_bound_flat_history_matches_per_tensor(sim):
    checks.check_bound_flat_matches_per_tensor(sim)


def test_set_momentum_and_annealing(sim):
    checks.check_set_momentum_uploads_on_change(sim)


def test_parameter_surgery_warm_up():
    checks.check_surgery()


def test_head_single_layer_unchanged_and_mlp(sim):
    checks.check_head_single_layer_unchanged(sim)


def test_excluded_combinations_raise():
    checks.check_rejections()
