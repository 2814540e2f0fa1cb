"""MI355X: the MoCo step glue (csrc/sf_moco.h, slowfast_amd/contrastive.py).  Checks in tests/moco_checks.py."""
import pytest

from tests import moco_checks as checks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("scale", checks.L2_SCALES)
@pytest.mark.parametrize("n,C", checks.L2_CASES)
def test_l2norm_rows(gpu, n, C, scale, with_perm, padded):
    checks.check_l2norm(gpu, n, C, scale, with_perm, padded)


def test_l2norm_zero_row_and_bad_perm(gpu):
    checks.check_l2norm_zero_row_and_bad_perm(gpu)


@pytest.mark.parametrize("grad_out", [1.0, 1024.0])
@pytest.mark.parametrize("n,V,K", checks.NCE_SHAPES)
@pytest.mark.parametrize("C", checks.NCE_C)
def test_moco_nce(gpu, C, n, V, K, grad_out):
    checks.check_nce(gpu, n, V, K, C, "randn", grad_out)


@pytest.mark.parametrize("kind", checks.NCE_KINDS[1:])
@pytest.mark.parametrize("n,V,K,C", [(3, 3, 96, 64), (8, 3, 4096, 128)])
def test_moco_nce_adversarial(gpu, n, V, K, C, kind):
    checks.check_nce(gpu, n, V, K, C, kind)


def test_moco_nce_rejections(gpu):
    checks.check_nce_rejections(gpu)


def test_host_tensors_are_rejected(gpu):
    checks.check_rejects_host_tensors()


@pytest.mark.parametrize("views,multi_view,start", [(3, True, 0), (1, True, 0), (3, False, 0), (3, False, 8), (1, True, 4)])
def test_enqueue(gpu, views, multi_view, start):
    p = checks.check_enqueue(gpu, views, multi_view, start)
    if views == 3 and multi_view:
        assert p == 0           # 0 -> 4 -> 8 -> 0


def test_enqueue_bad_pointer_is_a_noop(gpu):
    checks.check_enqueue_bad_pointer(gpu)


@pytest.mark.parametrize("m", checks.EMA_M)
@pytest.mark.parametrize("n", checks.EMA_SIZES)
def test_ema_update(gpu, n, m):
    checks.check_ema(gpu, n, m)


def test_capture_replays_match_eager(gpu):
    checks.check_capture(gpu)


def test_state_dict_contract(gpu):
    checks.check_state_dict(gpu)


def test_tiny_model_two_iterations(gpu):
    checks.check_model(gpu)


def test_bound_flat_history_matches_per_tensor(gpu):
    checks.check_bound_flat_matches_per_tensor(gpu)


def test_set_momentum_and_annealing(gpu):
    checks.check_set_momentum_uploads_on_change(gpu)


def test_head_single_layer_unchanged_and_mlp(gpu):
    checks.check_head_single_layer_unchanged(gpu)
