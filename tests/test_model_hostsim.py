"""CPU: whole-model forward/backward of the drop-in modules through the host simulator vs the oracle.

These tiny models (batch 2, 32x32 crops) put only 4-16 samples under the deepest BatchNorms, which amplifies
fp16 round-off by 1-2 orders of magnitude; the bounds here are therefore loose and the test is a wiring check
(every block, lateral connection, pooling and the head in the right order with the right parameters).
Strict parity: tests/test_blocks_hostsim.py (well-conditioned blocks) and the -m gpu model tests."""
import pytest

from tests import model_checks as mc


@pytest.mark.parametrize("name", ["slowfast_tiny", "c2d_tiny", "i3d_basic_tiny"])       # i3d_basic: RESNET.TRANS_FUNC basic_transform
def test_engine_wiring_matches_oracle(sim, name):
    mc.check_engine(name, sim, tol_logits=0.15, tol_loss=0.02, tol_gnorm=0.35, tol_param=2.0, tol_stats=0.05)


def test_mvit_engine_matches_oracle(sim):
    """4-block MViTv2 miniature (q pooling, dimension change, k/v pooling, relative positions, residual pooling,
    cls token) through every token-space kernel, forward and backward."""
    # tol_param: the worst parameter is attn.norm_k.bias, whose true gradient vanishes identically (a constant added to
    # every key shifts all scores of a query equally): its computed value is pure round-off of the dK column sums
    mc.check_engine("mvit_tiny", sim, tol_logits=1e-2, tol_loss=2e-3, tol_gnorm=3e-3, tol_param=0.2, tol_global=2e-2)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("drop_path", [False, True])
def test_mvit_resid_side_rows(sim, drop_path, full):
    """fp32 side rows of the residual stream: class-token rows through every block, every row in the last stage."""
    mc.check_mvit_resid_side("mvit_tiny", sim, drop_path=drop_path, full=full)


def test_x3d_engine_matches_oracle(sim):
    """X3D (depth factor 1): W-pair-folded stem conv, depthwise (5,1,1) and 3x3x3 stencils with BatchNorm statistics
    epilogues, SE squeeze/gate, gate*BN->Swish, channel widths 54/108 padded to 56/112, X3DHead."""
    mc.check_engine("x3d_tiny", sim, tol_logits=1e-2, tol_loss=2e-3, tol_gnorm=2e-2, tol_param=0.5, tol_global=0.3,
                    tol_stats=5e-3)


def test_precise_bn_protocol_on_drop_ins(sim):
    """`calculate_and_update_precise_bn` (tools/train_net.py:425-446) hands the model to fvcore's ``update_bn_stats``, which
    relies on three properties of the BatchNorm modules it finds by isinstance: a train-mode forward under
    ``torch.no_grad()`` updates ``running_mean`` / ``running_var``, the update honours the module's CURRENT ``momentum``
    (fvcore sets it to 1.0 so that the buffers hold the batch statistics of the last forward), and the buffers are plain
    tensors it may overwrite afterwards.  Checked on the SlowFast drop-in against the oracle's batch statistics."""
    import torch
    import slowfast_amd as sa
    from oracle import video_ref
    gold = mc.load_golden("slowfast_tiny")
    cfg = mc.cfg_for(gold)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    sd = video_ref.randomize_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, gold["param_seed"])
    model.load_state_dict(sd)
    inputs, labels = video_ref.synthetic_batch(cfg, gold["batch"], gold["data_seed"])
    _, _, _, o_stats = video_ref.loss_and_grads(sd, cfg, inputs, labels)        # oracle: momentum 0.1 update of sd's buffers
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert len(bns) > 20
    for bn in bns:
        bn.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(inputs)
    msd = model.state_dict()
    worst = 0.0
    for k, new in o_stats.items():
        batch_stat = (new - 0.9 * sd[k]) / 0.1                  # what the oracle's update averaged in
        err = float((msd[k].float() - batch_stat).abs().max() / (batch_stat.abs().max() + 1e-6))
        worst = max(worst, err)
    assert worst < 5e-2 * mc.EPS_SCALE, worst                                  # tiny-model conditioning (see module docstring)
    for bn in bns:                                              # fvcore then writes its averages back and restores momentum
        bn.running_mean.copy_(torch.zeros_like(bn.running_mean))
        bn.momentum = 0.1
    with torch.no_grad():
        out = model.eval()(inputs)
    assert torch.isfinite(out.float()).all()


def test_x3d_bn_lin5_matches_oracle(sim):
    """X3D.BN_LIN5: BatchNorm between the head's lin_5 and its ReLU (head_helper.py:440-443, 470-471)."""
    mc.check_engine("x3d_bnlin5_tiny", sim, tol_logits=1e-2, tol_loss=2e-3, tol_gnorm=2e-2, tol_param=0.5, tol_global=0.3,
                    tol_stats=5e-3)


@pytest.mark.slow
def test_nonlocal_engine_matches_oracle(sim):
    """SlowFast with Nonlocal blocks (dot-product affinity, (2,2,2) max-pool of the phi/g input) on res3/res4."""
    mc.check_engine("slowfast_nln_tiny", sim, tol_logits=2e-2, tol_loss=5e-3, tol_gnorm=2e-2, tol_param=1.0, tol_global=0.5,
                    tol_stats=2e-2)


def test_mvit_drop_path_matches_oracle(sim):
    """MVIT.DROPPATH_RATE > 0: per-sample stochastic depth on both residual branches of every block."""
    mc.check_mvit_drop_path(sim)


def test_packed_uint8_input_equals_float_input(sim):
    """A SlowFast forward on clips packed by sf_pack_clip_u8 gives exactly the logits of the float path fed with the
    reference's normalised fp32 clips (oracle/data_ref.py): both round the same fp32 values to fp16 once."""
    import torch
    import slowfast_amd as sa
    from oracle import data_ref
    gold = mc.load_golden("slowfast_tiny")
    cfg = mc.cfg_for(gold)
    torch.manual_seed(0)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg).eval()
    g = torch.Generator().manual_seed(3)
    S = cfg.DATA.TRAIN_CROP_SIZE
    frames = torch.randint(0, 256, (2, cfg.DATA.NUM_FRAMES, S, S, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    with torch.no_grad():
        a = model(sa.pack_pathways_u8(frames, cfg))
        b = model(data_ref.pack_pathways(frames, cfg))
    assert torch.equal(a, b)


@pytest.mark.slow
def test_nonlocal_group_folding_matches_oracle(sim):
    """NONLOCAL.GROUP 2: the temporal fold around the Nonlocal block is a view of the channels-last rows."""
    rep = {}
    try:
        mc.check_engine("slowfast_nln_group_tiny", sim, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=2e-3, tol_param=0.1,
                        tol_global=1e-2, report=rep)
    finally:
        print(rep)


@pytest.mark.slow
def test_sub_batchnorm_matches_reference(sim):
    """BN.NORM_TYPE sub_batchnorm, NUM_SPLITS 2 (multigrid training): the engine's sub-batch passes (batchnorm.run_in_splits)
    vs the unmodified reference's SubBatchNorm3d -- logits, loss, every parameter gradient and the per-split running
    statistics; then aggregate_stats() + eval against the oracle's eval forward."""
    import torch
    import slowfast_amd as sa
    from oracle import video_ref
    rep = {}
    try:
        mc.check_engine("slowfast_subbn_tiny", sim, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=2e-3, tol_param=0.1,
                        tol_global=1e-2, report=rep)
    finally:
        print(rep)
    gold = mc.load_golden("slowfast_subbn_tiny")
    cfg = mc.cfg_for(gold)
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    sd = video_ref.randomize_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, 5)
    model.load_state_dict(sd)
    from slowfast_amd.batchnorm import SubBatchNorm3d
    subs = [m for m in model.modules() if isinstance(m, SubBatchNorm3d)]
    assert subs and all(m.num_splits == 2 for m in subs)
    for m in subs:
        m.aggregate_stats()
    m = subs[0]
    C = m.num_features
    means, vars_ = m.split_bn.running_mean.view(2, C), m.split_bn.running_var.view(2, C)
    assert torch.allclose(m.bn.running_mean, means.mean(0))
    assert torch.allclose(m.bn.running_var, vars_.mean(0) + ((means - means.mean(0)) ** 2).mean(0))
    inputs, _ = video_ref.synthetic_batch(cfg, 2, 11)
    ref = video_ref.video_forward(model.state_dict(), cfg, inputs, training=False)
    with torch.no_grad():
        out = model.eval()(inputs).float()
    assert float((out - ref).abs().max()) < 0.05 * float(ref.abs().max())     # tiny-model conditioning (see module docstring)


@pytest.mark.parametrize("name", ["mvit_v1_tiny", "vit_tiny"])
def test_mvit_v1_and_vit_match_reference(sim, name):
    """MViTv1 (configs/Kinetics/MVIT_B_16x4_CONV.yaml: separate learned position embeddings, dimension change after the
    Mlp, blocks without q pooling, no relative positions / residual pooling) and the plain video ViT of the masked-SSL
    fine-tuning configs (no pooling at all, mean pooling before the final norm) vs the unmodified reference."""
    rep = {}
    try:
        # tol_param: attn.norm_k.bias has an identically vanishing true gradient (see test_mvit_engine_matches_oracle)
        mc.check_engine(name, sim, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=2e-3, tol_param=0.2, tol_global=1e-2, report=rep)
    finally:
        print(rep)


@pytest.mark.parametrize("name", ["mvit_nocls_sepqkv_tiny", "mvit_poolfirst_tiny", "mvit_relinterp_tiny"])
@pytest.mark.parametrize("fused_attn", ["1", "0"])
def test_mvit_attention_options_match_reference(sim, name, fused_attn, monkeypatch):
    """MultiScaleAttention options vs the unmodified reference: no cls token (CLS_EMBED_ON False: pooling, relative
    positions, residual pooling and the skip max-pool over all rows; norm -> mean feeds the head), separate q / k / v
    Linears (SEPARATE_QKV: one GEMM against the concatenated operand) and POOL_FIRST (pooling convs of dim / heads
    channels on the block input, q / k / v Linears on the pooled tokens) and relative-position tables resampled by
    get_rel_pos (odd pooled extents, as in MViTv2-L 40x3 at 312^2), fused and unfused attention core."""
    monkeypatch.setenv("SF_ATTN_FUSED", fused_attn)
    rep = {}
    try:
        mc.check_engine(name, sim, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=2e-3, tol_param=0.2, tol_global=1e-2, report=rep)
    finally:
        print(rep)


def test_mvit_detection_matches_reference(sim):
    """MViT with DETECTION.ENABLE (video_model_builder.py:1034-1045, 1218-1226): final norm on every token, the token tensor
    viewed as the channels-last (B, C, T, H, W) feature map, ResNetRoIHead on 3 boxes per clip, BCE."""
    rep = {}
    try:
        mc.check_engine("mvit_ava_roi_tiny", sim, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=2e-3, tol_param=0.2, tol_global=1e-2,
                        report=rep)
    finally:
        print(rep)


def test_reversible_mvit_matches_reference(sim):
    """Reversible MViT (configs/Kinetics/REV_MVIT_B_16x4_CONV.yaml family): two-stream ReversibleBlocks, StageTransitionBlocks
    (stream average, residual through the attention's own pool_q + norm_q and res_proj), norm over the concatenated
    streams -> mean.  The golden numbers come from the reference's RevBackProp training path."""
    rep = {}
    try:
        mc.check_engine("mvit_rev_tiny", sim, tol_logits=4e-3, tol_loss=1e-3, tol_gnorm=2e-3, tol_param=0.2, tol_global=1e-2,
                        report=rep)
    finally:
        print(rep)


def test_reversible_mvit_drop_path(sim):
    print(mc.check_rev_mvit_drop_path(sim))


def test_x3d_sub_batchnorm_backbone_with_full_batch_head(sim):
    """X3D with BN.NORM_TYPE sub_batchnorm: the reference builds the backbone with SubBatchNorm3d but leaves the head's
    conv_5_bn a plain BatchNorm3d over the whole batch; the engine runs the backbone in sub-batch passes and the head once
    on the re-interleaved features.  Checked against the oracle (whose SubBatchNorm3d and X3D restatements are both pinned
    to the reference)."""
    import torch
    import slowfast_amd as sa
    from oracle import video_ref
    gold = mc.load_golden("x3d_tiny")
    cfg = mc.cfg_for(gold, ["BN.NORM_TYPE", "sub_batchnorm", "BN.NUM_SPLITS", 2])
    model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    sd = video_ref.randomize_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, 21)
    model.load_state_dict(sd)
    inputs, labels = video_ref.synthetic_batch(cfg, 4, 22)
    o_logits, o_loss, o_grads, o_stats = video_ref.loss_and_grads(sd, cfg, inputs, labels)
    model.train()
    logits = model(inputs)
    loss = torch.nn.functional.cross_entropy(logits.float(), labels)
    (loss * 64.0).backward()
    grads = {k: p.grad.float() / 64.0 for k, p in model.named_parameters()}
    assert float((logits.detach().float() - o_logits).abs().max()) < 2e-2 * mc.EPS_SCALE * float(o_logits.abs().max())
    gn, ogn = float(video_ref.grad_norm(grads)), float(video_ref.grad_norm(o_grads))
    assert abs(gn - ogn) < 5e-2 * mc.EPS_SCALE * ogn, (gn, ogn)
    num = sum(float((grads[k].double() - g.double()).pow(2).sum()) for k, g in o_grads.items())
    den = sum(float(g.double().pow(2).sum()) for g in o_grads.values())
    assert (num / den) ** 0.5 < min(1.0, 0.3 * mc.EPS_SCALE), (num / den) ** 0.5          # tiny-model conditioning (2 samples per split)
    msd = model.state_dict()
    for k, v in o_stats.items():
        assert float((msd[k].float() - v).abs().max()) <= 2e-2 * mc.EPS_SCALE * float(v.abs().max()) + 1e-4, k


def test_well_conditioned_1e3_no_yardstick(sim):
    """The north-star bar asserted directly (no yardstick) on a well-conditioned C2D-R50 (tests/golden/c2d_wc.json); the
    GPU suite runs the SlowFast / X3D / R101+Nonlocal cases as well."""
    mc.check_well_conditioned("c2d_wc", sim)


def test_lateral_concat_written_in_place(sim, monkeypatch):
    """The last Slow block of a stage writes its output into the lateral connection's concatenated buffer (engine.ResBlockFn
    `_cat_extra` / FuseFn): three full-tensor copies less per SlowFast forward, logits and every parameter gradient bit for bit
    what the copying schedule gives."""
    import torch
    import slowfast_amd as sa
    from slowfast_amd import engine, lib
    gold = mc.load_golden("slowfast_tiny")
    cfg = mc.cfg_for(gold)
    T, S = cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE
    g = torch.Generator().manual_seed(1)
    fast = torch.randn((2, 3, T, S, S), generator=g)
    slow = torch.index_select(fast, 2, torch.linspace(0, T - 1, T // cfg.SLOWFAST.ALPHA).long())
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(engine, "CAT_IN_PLACE", flag)
        torch.manual_seed(0)
        model = sa.MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg).train()
        calls = []
        lib.set_call_observer(lambda name, thunk, work: (calls.append(name), thunk())[1])
        try:
            out = model([slow, fast])
            out.float().sum().backward()
        finally:
            lib.set_call_observer(None)
        res[flag] = (out.detach().clone(), [p.grad.clone() for p in model.parameters()], calls.count("sf_bn_act"))
    assert res[False][2] - res[True][2] == 3, "one copy per lateral connection after res2 / res3 / res4"
    assert torch.equal(res[True][0], res[False][0])
    assert all(torch.equal(a, b) for a, b in zip(res[True][1], res[False][1]))


def test_end_of_backward_join_survives_a_failed_backward(monkeypatch):
    """engine._notify queues join_side_streams once per backward PASS.  A pass that raises never runs its end-of-pass callbacks;
    the passes after it must still queue -- and run -- their own join, and none may be left marked as queued (a process-wide
    "queued" flag stuck at True after the failure, and every later plain ``loss.backward(); optimizer.step()`` skipped the join
    of the Fast-pathway / k-v-branch streams)."""
    import torch
    from slowfast_amd import engine
    joined = []
    monkeypatch.setitem(engine._pathway_streams, ("dummy-device", 1), None)     # "a side stream exists"
    monkeypatch.setattr(engine, "_join_pathways", joined.append)                # join_side_streams and _notify stay real

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, fail):
            ctx.fail = fail
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            engine._notify([])
            if ctx.fail:
                raise ValueError("backward failed")
            return g, None

    x = torch.ones(2, requires_grad=True)
    Fn.apply(x, False).sum().backward()
    assert joined == ["dummy-device"]
    with pytest.raises(ValueError, match="backward failed"):
        Fn.apply(x, True).sum().backward()
    assert joined == ["dummy-device"]
    Fn.apply(x, False).sum().backward()
    assert joined == ["dummy-device"] * 2
    assert engine._join_task == -1, "a join is still marked as queued"
