"""The host-side rules the engines share (semantic_segmentation_amd/engine_common.py), on the CPU: no GPU, no native library
(ops.bn_finalize / ops.bn_eval_coeffs are replaced by recording fakes)."""
import pytest
import torch
from torch import nn

from semantic_segmentation_amd import engine_common as ec


@pytest.fixture
def calls(monkeypatch):
    """(kind, what the fake saw at call time): momentum, the running buffers as passed and a copy of the mean at that moment"""
    rec = []

    def bn_finalize(partials, ntiles, C, count, gamma, beta, rm, rv, momentum, eps, scale, shift, mean, invstd):
        rec.append(dict(kind="finalize", momentum=momentum, rm=rm, rv=rv, C=C, count=count, eps=eps, gamma=gamma, beta=beta,
                        rm_then=None if rm is None else rm.clone()))

    def bn_eval_coeffs(C, gamma, beta, rm, rv, eps, scale, shift, mean, invstd):
        rec.append(dict(kind="eval", rm=rm, rv=rv, C=C, eps=eps))
    monkeypatch.setattr(ec.ops, "bn_finalize", bn_finalize)
    monkeypatch.setattr(ec.ops, "bn_eval_coeffs", bn_eval_coeffs)
    return rec


def run(bn, training, **kw):
    return ec.bn_coeffs(bn, torch.zeros(8), 1, 4, 32, training, torch.device("cpu"), **kw)


def test_bn_coeffs_train_defers_the_counter_to_the_flush(calls):
    bn = nn.BatchNorm2d(4)
    pending = []
    coef, batch_stats = run(bn, True, nbt_pending=pending)
    assert batch_stats is True and tuple(coef.shape) == (4, 4) and coef.dtype == torch.float32
    assert int(bn.num_batches_tracked) == 0 and len(pending) == 1 and pending[0] is bn.num_batches_tracked
    (c,) = calls
    assert c["kind"] == "finalize" and c["momentum"] == 0.1 and c["eps"] == bn.eps and (c["C"], c["count"]) == (4, 32)
    assert c["rm"] is bn.running_mean and c["rv"] is bn.running_var
    assert c["gamma"].data_ptr() == bn.weight.data_ptr() and c["beta"].data_ptr() == bn.bias.data_ptr()
    assert not c["gamma"].requires_grad and not c["beta"].requires_grad
    ec._flush_nbt(pending)
    assert int(bn.num_batches_tracked) == 1 and pending == []
    ec._flush_nbt(pending)                                # nothing pending: no launch, no error
    assert int(bn.num_batches_tracked) == 1


def test_bn_coeffs_train_without_a_list_counts_at_once(calls):
    bn = nn.BatchNorm2d(4)
    run(bn, True)
    assert int(bn.num_batches_tracked) == 1
    run(bn, True)                                         # (UNet3D's shared decoder BatchNorm: two uses, two counts)
    assert int(bn.num_batches_tracked) == 2
    assert [c["momentum"] for c in calls] == [0.1, 0.1]


@pytest.mark.parametrize("with_list", [False, True])
def test_bn_coeffs_cumulative_average_counts_first(calls, with_list):
    bn = nn.BatchNorm2d(4, momentum=None)
    pending = [] if with_list else None
    run(bn, True, nbt_pending=pending)
    assert int(bn.num_batches_tracked) == 1 and not pending
    run(bn, True, nbt_pending=pending)
    assert int(bn.num_batches_tracked) == 2 and not pending
    assert [c["momentum"] for c in calls] == [1.0, 0.5]
    assert all(c["rm"] is bn.running_mean and c["rv"] is bn.running_var for c in calls)


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("training", [False, True])
def test_bn_coeffs_without_running_statistics(calls, momentum, training):
    bn = nn.BatchNorm2d(4, momentum=momentum, track_running_stats=False)
    pending = []
    _, batch_stats = run(bn, training, nbt_pending=pending)
    assert batch_stats is True and pending == []
    (c,) = calls
    assert c["kind"] == "finalize" and c["rm"] is None and c["rv"] is None
    assert c["momentum"] == (0.0 if momentum is None else momentum)
    run(bn, training)                                     # ... and without a list
    assert len(calls) == 2 and calls[1]["rm"] is None and calls[1]["rv"] is None


def test_bn_coeffs_eval_reads_the_running_buffers(calls):
    bn = nn.BatchNorm2d(4).eval()
    pending = []
    _, batch_stats = run(bn, False, nbt_pending=pending)
    assert batch_stats is False and pending == [] and int(bn.num_batches_tracked) == 0
    (c,) = calls
    assert c["kind"] == "eval" and c["rm"] is bn.running_mean and c["rv"] is bn.running_var and c["eps"] == bn.eps


def test_bn_coeffs_conv_bias(calls):
    bias = nn.Parameter(torch.tensor([1.0, -2.0, 0.5, 4.0]))
    bn = nn.BatchNorm2d(4, momentum=0.25)                 # (dyadic values: the sums below are exact in any order)
    with torch.no_grad():
        bn.running_mean.copy_(torch.tensor([0.25, 0.5, -1.0, 2.0]))
    before = bn.running_mean.clone()
    run(bn, True, conv_bias=bias)
    (c,) = calls
    assert c["rm"] is bn.running_mean and torch.equal(c["rm_then"], before)       # the fake ran first, on the untouched mean
    assert torch.equal(bn.running_mean, before + 0.25 * bias.detach())             # (the fake itself updates nothing)
    assert int(bn.num_batches_tracked) == 1
    # cumulative average: the same factor 1 / count for the statistics and for the bias
    bn2 = nn.BatchNorm2d(4, momentum=None)
    run(bn2, True, conv_bias=bias)
    run(bn2, True, conv_bias=bias)
    assert torch.equal(bn2.running_mean, 1.0 * bias.detach() + 0.5 * bias.detach())
    # eval: the statistics are those of conv + bias, the kernel's output lacks the bias
    calls.clear()
    now = bn.running_mean.clone()
    _, batch_stats = run(bn, False, conv_bias=bias)
    (c,) = calls
    assert batch_stats is False and c["kind"] == "eval" and c["rv"] is bn.running_var
    assert c["rm"] is not bn.running_mean and c["rm"].is_contiguous() and torch.equal(c["rm"], now - bias.detach())
    assert torch.equal(bn.running_mean, now)


def test_param_index_follows_the_owners():
    net = nn.Sequential(nn.Conv2d(1, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.Linear(4, 2)))
    idx = ec.ParamIndex(net)
    want = list(net.named_parameters())
    assert idx.param_names() == [n for n, _ in want]
    assert all(a is b for a, (_, b) in zip(idx.param_list(), want))
    assert [(n, id(p)) for n, p in idx.param_items()] == [(n, id(p)) for n, p in want]
    bufs = idx.buffer_dict()
    assert list(bufs) == [n for n, _ in net.named_buffers()] and bufs["1.running_mean"] is net[1].running_mean
    assert idx.submodule("2.0") is net[2][0] and idx.submodule("") is net

    lin = nn.Linear(3, 2)
    idx = ec.ParamIndex(lin)
    assert idx.param_list()[0] is lin.weight
    lin.weight = nn.Parameter(torch.ones(2, 3))           # a swapped Parameter object
    assert idx.param_list()[0] is lin.weight and dict(idx.param_items())["weight"] is lin.weight
    lin.double()                                          # a conversion of the whole module
    assert [p.dtype for p in idx.param_list()] == [torch.float64, torch.float64]
    assert all(a is b for a, b in zip(idx.param_list(), lin.parameters()))
    bn = nn.BatchNorm2d(4)
    idx = ec.ParamIndex(bn)
    bn.double()
    assert idx.buffer_dict()["running_var"] is bn.running_var and bn.running_var.dtype == torch.float64


def test_pack_key_and_reuse_policy(monkeypatch):
    monkeypatch.setattr(ec, "PACK_CACHE", True)           # the default policy ("safe"), whatever GSSEG_PACK_CACHE says here
    monkeypatch.setattr(ec, "PACK_CACHE_TRAINING", False)
    p = nn.Parameter(torch.zeros(3, 2))
    k = ec.pack_key(p)
    assert ec.pack_key(p) == k and k[:2] == (p.data_ptr(), p._version)
    with torch.no_grad():
        p.add_(1)
    assert ec.pack_key(p) != k
    assert ec.pack_key(p) != ec.pack_key(torch.zeros(3, 2))
    # (need_grad, trust_versions): only a forward that keeps a graph and whose owner does not vouch for the versions re-packs
    table = {(False, False): True, (False, True): True, (True, False): False, (True, True): True}
    for (need_grad, trust), want in table.items():
        assert ec.pack_reuse_allowed(need_grad, trust) is want
    assert ec.pack_reuse_allowed(True) is False and ec.pack_reuse_allowed(False) is True
    monkeypatch.setattr(ec, "PACK_CACHE_TRAINING", True)  # GSSEG_PACK_CACHE=versions
    assert ec.pack_reuse_allowed(True, False) is True
    monkeypatch.setattr(ec, "PACK_CACHE", False)          # GSSEG_PACK_CACHE=0: nothing is reused, no key equals another
    assert not any(ec.pack_reuse_allowed(g, t) for g in (False, True) for t in (False, True))
    assert ec.pack_key(p) != ec.pack_key(p)


def test_pix2pix_version_keys_follow_pack_key(monkeypatch):
    from semantic_segmentation_amd.models_pix2pix import pix2pix_engine
    monkeypatch.setattr(ec, "PACK_CACHE", True)
    a, b = nn.Parameter(torch.zeros(2)), torch.ones(3)
    assert pix2pix_engine._ver(a, b) == ((a.data_ptr(), a._version), (b.data_ptr(), b._version)) == pix2pix_engine._ver(a, b)
    b.add_(1)
    assert pix2pix_engine._ver(a, b) == ((a.data_ptr(), a._version), (b.data_ptr(), b._version))
    monkeypatch.setattr(ec, "PACK_CACHE", False)
    assert pix2pix_engine._ver(a) != pix2pix_engine._ver(a)


def test_pix2pix_norm_act_bwd_launch_sequence(monkeypatch):
    """The one norm + activation backward of the Pix2Pix plans (pix2pix_engine.norm_act_bwd), on recording fakes: BatchNorm is
    reduce -> coeffs -> apply with c1 / c2 all zeros where the stage ran on running statistics, InstanceNorm one gs_in_act_bwd
    and no parameter gradients, no norm the apply pass alone."""
    from semantic_segmentation_amd._lib import ACT_LEAKY02, ACT_NONE, ACT_RELU
    from semantic_segmentation_amd.models_pix2pix import pix2pix_engine as pe
    rec = []

    def bn_act_bwd_reduce(y, dz_a, sa, ca, dzp, scale, shift, mean, invstd, act, partials, **kw):
        rec.append(dict(kind="reduce", y=y, dz_a=dz_a, sa=sa, ca=ca, coef=(scale, shift, mean, invstd), act=act, partials=partials, kw=kw))

    def bn_bwd_coeffs(partials, ntiles, C, count, gscale, dgamma, dbeta, c1, c2):
        c1.fill_(3.0), c2.fill_(5.0)                      # (what the apply pass must not see after a stage on running statistics)
        rec.append(dict(kind="coeffs", partials=partials, ntiles=ntiles, C=C, count=count, gscale=gscale, dgamma=dgamma, dbeta=dbeta))

    def bn_act_bwd_apply(y, dz_a, sa, ca, dzp, scale, shift, mean, invstd, c1, c2, act, bn, dy, **kw):
        rec.append(dict(kind="apply", y=y, dz_a=dz_a, sa=sa, ca=ca, coef=(scale, shift, mean, invstd), bn=bn, dy=dy, act=act, kw=kw,
                        c1=None if c1 is None else c1.clone(), c2=None if c2 is None else c2.clone()))

    def in_act_bwd(y, mean, invstd, dz_a, sa, ca, act, dy, gmeans, ws=None, **kw):
        rec.append(dict(kind="in", y=y, mean=mean, invstd=invstd, dz_a=dz_a, sa=sa, ca=ca, act=act, dy=dy, gmeans=gmeans, ws=ws, kw=kw))
    for f in (bn_act_bwd_reduce, bn_bwd_coeffs, bn_act_bwd_apply, in_act_bwd):
        monkeypatch.setattr(pe.ops, f.__name__, f)
    monkeypatch.setattr(pe.ops, "bn_bwd_tiles", lambda N, H, W: 6)
    monkeypatch.setattr(pe.ops, "bn_bwd_tiles_used", lambda N, H, W, pooled: 5)
    monkeypatch.setattr(pe.ops, "bn_partials_numel", lambda ntiles, C: 2 * ntiles * C)
    monkeypatch.setattr(pe.ops, "in_workspace", lambda N, H, W, C, dev: ("ws", N, H, W, C))

    N, H, W, C = 2, 3, 4, 8
    y = torch.zeros((N, H, W, C), dtype=torch.float16)
    dz, dzb = torch.zeros((N, H, W, 2 * C), dtype=torch.float16), torch.zeros_like(y)
    coef = torch.zeros((4, C))
    keep = torch.ones((N, H, W, C), dtype=torch.uint8)
    kw = dict(dz_b=dzb, act_b=ACT_LEAKY02, keep_mask=keep, keep_scale=2.0)

    def is_dy(t):
        return t.shape == y.shape and t.dtype == y.dtype and t.is_contiguous()

    # BatchNorm on batch statistics, with both consumers and a keep-mask: every launch sees them
    dy, dgamma, dbeta = pe.norm_act_bwd(y, coef, None, True, dz, 2 * C, C, ACT_RELU, 0.25, N, dz_b=dzb, act_b=ACT_LEAKY02, keep=keep, kscale=2.0)
    assert [r["kind"] for r in rec] == ["reduce", "coeffs", "apply"]
    red, co, ap = rec
    for r in (red, ap):
        assert r["y"] is y and r["dz_a"] is dz and (r["sa"], r["ca"], r["act"]) == (2 * C, C, ACT_RELU) and r["kw"] == kw
        assert all(a.data_ptr() == coef[i].data_ptr() for i, a in enumerate(r["coef"]))
    assert red["partials"] is co["partials"] and red["partials"].numel() == 2 * 6 * C and red["partials"].dtype == torch.float32
    assert (co["ntiles"], co["C"], co["count"], co["gscale"]) == (5, C, N * H * W, 0.25)
    assert co["dgamma"] is dgamma and co["dbeta"] is dbeta and dgamma.shape == dbeta.shape == (C,) and dgamma.dtype == torch.float32
    assert ap["bn"] is True and ap["dy"] is dy and is_dy(dy)
    assert torch.equal(ap["c1"], torch.full((C,), 3.0)) and torch.equal(ap["c2"], torch.full((C,), 5.0))

    # BatchNorm on running statistics: the same three launches, c1 / c2 all zeros
    rec.clear()
    dy, dgamma, dbeta = pe.norm_act_bwd(y, coef, None, False, dz, 2 * C, 0, ACT_LEAKY02, 0.25, N)
    assert [r["kind"] for r in rec] == ["reduce", "coeffs", "apply"]
    assert rec[2]["bn"] is True and rec[2]["dy"] is dy and rec[1]["dgamma"] is dgamma and rec[1]["dbeta"] is dbeta
    assert rec[2]["c1"].shape == rec[2]["c2"].shape == (C,) and not rec[2]["c1"].any() and not rec[2]["c2"].any()
    assert rec[0]["kw"] == rec[2]["kw"] == dict(dz_b=None, act_b=ACT_NONE, keep_mask=None, keep_scale=1.0)

    # InstanceNorm: one launch on the per-sample view (an image batch: the tensor itself), nothing for gamma / beta
    rec.clear()
    mi = torch.zeros((2, N, C))
    dy, dgamma, dbeta = pe.norm_act_bwd(y, None, mi, True, dz, 2 * C, C, ACT_RELU, 0.25, N, dz_b=dzb, act_b=ACT_LEAKY02, keep=keep, kscale=2.0)
    (r,) = rec
    assert r["kind"] == "in" and r["y"] is y and r["dz_a"] is dz and (r["sa"], r["ca"], r["act"]) == (2 * C, C, ACT_RELU) and r["kw"] == kw
    assert r["mean"].data_ptr() == mi[0].data_ptr() and r["invstd"].data_ptr() == mi[1].data_ptr()
    assert r["gmeans"].shape == (2, N, C) and r["gmeans"].dtype == torch.float32 and r["ws"] == ("ws", N, H, W, C)
    assert r["dy"] is dy and is_dy(dy) and dgamma is None and dbeta is None
    # ... a volume stored as depth slices [N*D,H,W,C] goes in as [N, D*H, W, C]; dy keeps the slices' shape
    rec.clear()
    dy, _, _ = pe.norm_act_bwd(y, None, mi[:, :1], True, dzb, C, 0, ACT_RELU, 0.25, 1)
    (r,) = rec
    assert r["y"].shape == (1, N * H, W, C) and r["y"].data_ptr() == y.data_ptr() and r["ws"] == ("ws", 1, N * H, W, C)
    assert r["gmeans"].shape == (2, 1, C) and r["dy"] is dy and is_dy(dy)

    # no norm: the apply pass alone, without coefficients
    rec.clear()
    dy, dgamma, dbeta = pe.norm_act_bwd(y, None, None, False, dzb, C, 0, ACT_LEAKY02, 0.25, N)
    (r,) = rec
    assert r["kind"] == "apply" and r["bn"] is False and r["coef"] == (None,) * 4 and r["c1"] is None and r["c2"] is None
    assert r["y"] is y and r["dz_a"] is dzb and (r["sa"], r["ca"], r["act"]) == (C, 0, ACT_LEAKY02)
    assert r["dy"] is dy and is_dy(dy) and dgamma is None and dbeta is None


def test_compute_dtype(monkeypatch):
    monkeypatch.delenv("GSSEG_DTYPE", raising=False)
    assert ec.compute_dtype() == ("f16", torch.float16) == ec.compute_dtype("f16") == ec.compute_dtype("")
    assert ec.compute_dtype("bf16") == ("bf16", torch.bfloat16)
    monkeypatch.setenv("GSSEG_DTYPE", "bf16")
    assert ec.compute_dtype() == ("bf16", torch.bfloat16) and ec.compute_dtype("f16") == ("f16", torch.float16)
    for bad in ("fp32", "float16"):
        with pytest.raises(ValueError):
            ec.compute_dtype(bad)
    monkeypatch.setenv("GSSEG_DTYPE", "f32")
    with pytest.raises(ValueError):
        ec.compute_dtype()


def test_stage_keys_name_the_state_dict():
    from semantic_segmentation_amd.unet import UNet
    from semantic_segmentation_amd.unet.unet_engine import STAGES, _stage_keys
    sd = UNet(1, 2).state_dict()
    for st in STAGES:
        wkey, bnkey, transposed = _stage_keys(st)
        assert wkey in sd and sd[wkey].dim() == 4, st
        assert transposed == st.endswith(".up")
        if transposed:
            assert bnkey is None
        else:
            for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
                assert f"{bnkey}.{leaf}" in sd, (st, leaf)
            assert sd[bnkey + ".weight"].shape[0] == sd[wkey].shape[0]
    assert len({_stage_keys(st)[0] for st in STAGES}) == len(STAGES)
    assert _stage_keys("down2.3")[0] == "down2.maxpool_conv.1.double_conv.3.weight"
    assert _stage_keys("down2.3")[1] == "down2.maxpool_conv.1.double_conv.4"
    assert _stage_keys("inc.0") == ("inc.double_conv.0.weight", "inc.double_conv.1", False)
    assert _stage_keys("up3.conv.0") == ("up3.conv.double_conv.0.weight", "up3.conv.double_conv.1", False)
    assert _stage_keys("up1.up") == ("up1.up.weight", None, True)


def test_lo_len_rule_matches_the_run_time_layout():
    """One rule (UNetEngine._lo_len) serves the segment packs and the K / wrap the kernels are launched with.  The pair forward
    used to derive the latter from what the up-sampling wrote: the up half of a concat buffer has a lo plane unless a "1"
    transposed conv of a plan that is not all-"xw" (hi plane only), or a bilinear up-sampling whose consumer has no x_lo segment,
    wrote it.  Both give every decoder-entry stage the same (segments, K, wrap), for every mode of the stage and of its up-conv."""
    from types import SimpleNamespace
    from semantic_segmentation_amd.unet.unet_engine import STAGES, UNetEngine, _segs
    modes = ("1", "x", "w", "xw", "xw-")
    for bilinear in (False, True):
        net = SimpleNamespace(bilinear=bilinear)          # all the rule reads of the network
        for up_mode in modes:
            for mode in modes:
                for rest in ("1", "xw"):
                    plan = {s_: rest for s_ in STAGES}
                    plan["up2.up"], plan["up2.conv.0"] = up_mode, mode
                    eng = UNetEngine(net, "f16", precise=plan)
                    full = all(v == "xw" for v in plan.values())
                    cout_t = 256
                    if bilinear:
                        up_lo_valid = "x" in mode
                    else:
                        up_lo_valid = not (up_mode == "1" and not full)
                    was = _segs(mode, 2 * cout_t, None if up_lo_valid else cout_t)
                    assert _segs(mode, 2 * cout_t, eng._lo_len("up2.conv.0", eng.plan, 2 * cout_t)) == was, (bilinear, up_mode, mode, rest)
                    for st in STAGES:                     # every other stage reads a whole lo plane
                        if not st.endswith(".conv.0"):
                            assert eng._lo_len(st, eng.plan, 128) is None


def test_models_hand_the_engines_a_resolved_dtype(monkeypatch):
    """UNet / UNet3D pass `compute_dtype` (usually None) on; the engines resolve it BEFORE the numerics plan, which depends on it"""
    from semantic_segmentation_amd.unet import UNet
    from semantic_segmentation_amd.unet.unet_engine import MIXED_XW, resolve_plan
    from semantic_segmentation_amd.unet3d import UNet3D
    from semantic_segmentation_amd.unet3d.unet3d_engine import resolve_plan3d
    monkeypatch.delenv("GSSEG_DTYPE", raising=False)
    monkeypatch.delenv("GSSEG_PRECISE", raising=False)
    eng = UNet(1, 2).engine
    assert (eng.dtype, eng.tdt) == ("f16", torch.float16) and eng.plan == resolve_plan("auto", "f16")
    assert any(eng.plan[s_] != "1" for s_ in MIXED_XW) and "1" in eng.plan.values()       # the mixed plan, not all-"xw"
    eng3 = UNet3D(1, 2).engine
    assert (eng3.dtype, eng3.tdt) == ("f16", torch.float16) and eng3.plan == resolve_plan3d("auto", "f16")
    assert "1" in [v for k, v in eng3.plan.items() if not k.endswith("upconv1")]
    monkeypatch.setenv("GSSEG_DTYPE", "bf16")
    eng = UNet(1, 2).engine
    assert (eng.dtype, eng.tdt) == ("bf16", torch.bfloat16) and eng.plan == resolve_plan("auto", "bf16")
    assert UNet(1, 2, compute_dtype="f16").engine.dtype == "f16"
    with pytest.raises(ValueError):
        UNet(1, 2, compute_dtype="f32")
