"""What tests/test_disc3d_kernels_gpu.py and tests/test_disc3d_networks_gpu.py rest on, proven on the CPU (no GPU, no native library):

  * every kernel case of disc3d_reference (image side, head, generic engine) is exact: its fp32 evaluation equals fp64 bit for bit, in
    another accumulation order too, so zero tolerance is the right bound; the lists cover what the kernels branch on;
  * on those cases each stated wrong implementation (kz / ky exchanged, depth pad missing or on one side only, depth stride 1, depth taps
    un-flipped in the data gradient, sub-voxel classes exchanged along depth, bias gradient without the border) gives at least one
    wrong element, and where it is the right function at a shape the test says so;
  * the 3-D geometry builders of ops.py, run by a gather emulation of GsConvGeom in torch, equal F.conv3d and its data gradient, and the
    [Cout][Cin][16][4] / [8][8] views of a 5-D weight give the [64][Cout][Cin] slot order (kz*4 + ky)*4 + kx;
  * the fp64 statement of both 3-D discriminators under both norms equals torch.autograd through F.conv3d in double at 1e-9, dx
    included, and the fixture the reference's own GenSeg-3D classes made (tests/golden/pix2pix3d_disc.npz) at 1e-9;
  * the public surface that needs no device: get_norm_layer / define_D(threed=True), the reference's key sets and 5-D shapes, the
    refusals by name;
  * on the seeds and shapes of the network tests a right implementation with the engine's 16-bit stores passes the GPU bounds and each
    stated wrong one (also: InstanceNorm statistics per slice, BatchNorm count without D, c2 dropped) does not."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import grad_summary, tensor_checksum
from golden_util_disc3d import FIXTURES, fixture_dense, fixture_input, fixture_state_dict, perturbed_running
from tests import disc3d_reference as d3
from tests import exact_reference as er
from tests import instnorm_reference as ir
from tests import pix2pix_backward_replay as pr

torch.set_num_threads(min(torch.get_num_threads(), 16))
G = torch.nn.grad


# ================================================================================================ kernel cases
def test_the_case_lists_cover_what_the_kernels_branch_on():
    img = d3.IMG_CASES
    assert {c[0] for c in img} == {1, 2, 3, 5, 16} and {c[1] for c in img} == {8, 64, 72, 128} and {c[3] for c in img} == {1, 3}
    assert {c[4] for c in img if c[2] == 4} >= {(2, 2, 2), (5, 7, 9), (6, 10, 70)} and {c[4] for c in img if c[2] == 1} == {(3, 4, 5), (2, 3, 70)}
    patches = [c[3] * d3.img_out(c)[0] * -(-d3.img_out(c)[1] // 4) * -(-d3.img_out(c)[2] // 32) for c in img if c[2] == 4]
    assert min(patches) == 1 and max(patches) > 256, "one block ... blocks that walk several patches"
    assert any(d3.img_out(c)[2] > 32 and d3.img_out(c)[2] % 32 for c in img), "an output row that crosses a 32-column patch"
    assert {c[0] for c in d3.HEAD_CASES} == {8, 64, 512, 1024}
    assert {c[2] for c in d3.HEAD_CASES if c[1] == 4} == {(2, 2, 2), (3, 3, 3), (4, 5, 9)} and {c[2] for c in d3.HEAD_CASES if c[1] == 1} == {(3, 4, 5)}
    assert {d3.head_out(c) for c in d3.HEAD_CASES if c[1] == 4} == {(1, 1, 1), (2, 2, 2), (3, 4, 8)}
    assert {(c[0], c[1]) for c in d3.ENGINE_CASES} == {(8, 16), (64, 128)} and {c[2] for c in d3.ENGINE_CASES} == {1, 2}
    assert {c[3] for c in d3.ENGINE_CASES} == {(4, 6, 10), (7, 5, 9)}


def _permuted_channel_sum(x, w, s, p, seed=1):
    perm = torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(seed))
    return sum(F.conv3d(x[:, i:i + 1], w[:, i:i + 1], None, stride=s, padding=p) for i in perm.tolist())


@pytest.mark.parametrize("case", d3.IMG_CASES, ids=d3.img_id)
def test_image_side_cases_are_exact_in_fp32_in_any_order(case):
    Cin, Cout, k, N, vol = case
    s, p = d3.GEOM[k]
    for vset in ("S", "P"):
        c = d3.img_build(case, vset)                              # asserts the product bounds
        x, w, dy = c["x"], c["w"], c["dy"]
        assert torch.equal(F.conv3d(x, w, None, stride=s, padding=p).double(), c["y"])
        assert torch.equal(_permuted_channel_sum(x, w, s, p).double(), c["y"]), "channel by channel in a permuted order"
        assert torch.equal(G.conv3d_weight(x, w.shape, dy, stride=s, padding=p).double(), c["dw"])
        assert torch.equal(G.conv3d_input(x.shape, w, dy, stride=s, padding=p).double(), c["dx"])
        er.expect32(c["dw"], d3.GSCALE), er.expect32(c["dx"], d3.GSCALE), er.expect16(c["y"], torch.bfloat16)
        assert float((c["y"] + c["b"].view(1, -1, 1, 1, 1)).abs().max()) < er.LIMIT


@pytest.mark.parametrize("case", d3.HEAD_CASES, ids=d3.head_id)
def test_head_cases_are_exact_in_fp32_in_any_order(case):
    Cin, k, vol = case
    p = d3.HEAD_PAD[k]
    for vset in ("S", "P"):
        r = d3.head_build(case, vset)
        x, w, dl = r["x"], r["w"], r["dy"]
        assert torch.equal(F.conv3d(x, w, None, padding=p).double(), r["y"])
        assert torch.equal(_permuted_channel_sum(x, w, 1, p).double(), r["y"])
        assert torch.equal(G.conv3d_weight(x, w.shape, dl, padding=p).double(), r["dw"])
        assert torch.equal(G.conv3d_input(x.shape, w, dl, padding=p).double(), r["dx"])
        er.expect32(r["dw"] * d3.GSCALE + 2.0), er.expect32(r["db"] * d3.GSCALE - 3.0), er.expect16(r["dx"], torch.bfloat16)


@pytest.mark.parametrize("case", d3.ENGINE_CASES, ids=d3.engine_id)
def test_engine_cases_are_exact_in_fp32_in_any_order(case):
    Cin, Cout, s, vol = case
    for vset in ("S", "P"):
        r = d3.engine_build(case, vset)
        x, w, dy = r["x"], r["w"], r["dy"]
        assert torch.equal(F.conv3d(x, w, None, stride=s, padding=1).double(), r["y"])
        assert torch.equal(_permuted_channel_sum(x, w, s, 1).double(), r["y"])
        assert torch.equal(G.conv3d_weight(x, w.shape, dy, stride=s, padding=1).double(), r["dw"])
        assert torch.equal(G.conv3d_input(x.shape, w, dy, stride=s, padding=1).double(), r["dx"])
        er.expect32(r["dw"], d3.GSCALE)


def _differs(a, b):
    return er.mismatches(a.float(), b.float()).shape[0] > 0


@pytest.mark.parametrize("case", d3.IMG_CASES, ids=d3.img_id)
def test_wrong_first_layers_are_wrong_on_the_cases(case):
    """assert_exact sees each mutant on every case at which it is a different function.  Not different, by construction: k 1 has one tap,
    no pad and stride 1 (every geometric mutant is the right function there: the k 4 cases catch them); at a 1 x 1 x 1 output stride 1
    along depth reads the same slices for the one output slice; `depth pad in front only` where no tap reaches the far pad (depth 5 at
    stride 2: the even depths catch it); an output of fewer than three voxels on an axis has no interior (`bias gradient without the
    border` is zero there, a wrong value)."""
    Cin, Cout, k, N, vol = case
    s, p = d3.GEOM[k]
    c = d3.img_build(case, "S")
    x, w, b, dy = c["x"].double(), c["w"].double(), c["b"].double(), c["dy"].double()
    right = d3.fwd_right(x, w, b, k, s, p)
    for name, fn in d3.FWD_MUTANTS.items():
        same_function = (k == 1 and name != "bias dropped") or (name == "depth stride 1" and d3.img_out(case)[0] == 1) or \
                        (name == "depth pad in front only" and not d3.far_pad_reached(vol[0], k, s, p))
        assert _differs(fn(x, w, b, k, s, p), right) != same_function, name
    assert _differs(d3.db_without_border(dy), d3.db_right(dy))
    for name, fn in d3.DGRAD_MUTANTS.items():
        assert _differs(fn(dy, w, x.shape, k, s, p), d3.dgrad_right(dy, w, x.shape, k, s, p)) == (k == 4), name


@pytest.mark.parametrize("case", d3.ENGINE_CASES, ids=d3.engine_id)
def test_wrong_middle_convs_are_wrong_on_the_cases(case):
    """the same mutants on the generic-engine cases (k 4 / pad 1, stride 2 and 1).  `classes exchanged` and `depth stride 1` are the right
    function at stride 1, `depth pad in front only` at depth 7 / stride 2 (no tap reaches the far pad; depth 4 catches it)."""
    Cin, Cout, s, vol = case
    r = d3.engine_build(case, "S")
    x, w, b, dy = r["x"].double(), r["w"].double(), r["b"].double(), r["dy"].double()
    right = d3.fwd_right(x, w, b, 4, s, 1)
    for name, fn in d3.FWD_MUTANTS.items():
        same_function = (name == "depth stride 1" and s == 1) or \
                        (name == "depth pad in front only" and not d3.far_pad_reached(vol[0], 4, s, 1))
        assert _differs(fn(x, w, b, 4, s, 1), right) != same_function, name
    assert _differs(d3.dgrad_depth_taps_unflipped(dy, w, x.shape, 4, s, 1), d3.dgrad_right(dy, w, x.shape, 4, s, 1))
    assert _differs(d3.dgrad_depth_classes_exchanged(dy, w, x.shape, 4, s, 1), d3.dgrad_right(dy, w, x.shape, 4, s, 1)) == (s == 2)


# ================================================================================================ geometry builders, pack order
def _run_geom(g, x, pack):
    """a GsConvGeom as gs_conv_igemm reads it, in torch fp64: x [N*Din, IH, IW, Cin], pack [slot][Cout][Cin] -> y [N*Dout, OH, OW, Cout]
    (only the logical output grid is written; the rest stays NaN)"""
    y = torch.full((g.N * g.Dout, g.OH, g.OW, g.Cout), float("nan"), dtype=torch.float64)
    for n in range(g.N):
        for d in range(g.Dg):
            for oy in range(g.OHg):
                for ox in range(g.OWg):
                    acc = torch.zeros(g.Cout, dtype=torch.float64)
                    for t in range(g.ntaps):
                        iz, iy, ix = d * g.isz + g.tap_dz[t], oy * g.isy + g.tap_dy[t], ox * g.isx + g.tap_dx[t]
                        if 0 <= iz < g.Din and 0 <= iy < g.IH and 0 <= ix < g.IW:
                            acc += pack[g.tap_w[t]] @ x[n * g.Din + iz, iy, ix]
                    y[n * g.Dout + d * g.osz + g.ooz, oy * g.osy + g.ooy, ox * g.osx + g.oox] = acc
    return y


@pytest.mark.parametrize("vol", [(4, 6, 5), (5, 3, 4)])
@pytest.mark.parametrize("s", [2, 1])
def test_geometry_builders_equal_conv3d(vol, s):
    from semantic_segmentation_amd import ops
    N, Cin, Cout, (D, H, W) = 2, 8, 3, vol
    gen = torch.Generator().manual_seed(4)
    x = torch.randn((N, Cin, D, H, W), generator=gen, dtype=torch.float64)
    w = torch.randn((Cout, Cin, 4, 4, 4), generator=gen, dtype=torch.float64)
    y = F.conv3d(x, w, None, stride=s, padding=1)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    g = ops.geom_conv3d(N, D, H, W, Cin, Cout, 4, s, 1)
    assert g.ntaps == 64 and (g.Dout, g.OH, g.OW) == tuple(y.shape[2:])
    got = _run_geom(g, d3.slices(x), d3.pack_slots(w, False))
    assert float((got - d3.slices(y)).abs().max()) < 1e-12
    dx = G.conv3d_input(x.shape, w, dy, stride=s, padding=1)
    wd = d3.pack_slots(w, True)
    if s == 1:
        got = _run_geom(ops.geom_conv3d_dgrad_s1(N, D, H, W, Cin, Cout, 4, 1), d3.slices(dy), wd)
    else:
        got = torch.full((N * D, H, W, Cin), float("nan"), dtype=torch.float64)
        for cls in range(8):
            gc = ops.geom_conv3d_s2_dgrad_class(N, D, H, W, Cin, Cout, 4, 1, cls >> 2, (cls >> 1) & 1, cls & 1)
            assert gc.ntaps == 8
            part = _run_geom(gc, d3.slices(dy), wd)
            assert not bool((~torch.isnan(part) & ~torch.isnan(got)).any()), "the classes write disjoint voxels"
            got = torch.where(torch.isnan(part), got, part)
    assert not bool(torch.isnan(got).any()) and float((got - d3.slices(dx)).abs().max()) < 1e-12


def test_pack_views_give_the_slot_order():
    """pack_weight is written for [Cout][Cin][kh][kw] and packs slot kh * KW + kw: the [16][4] and [8][8] views of a [4][4][4] kernel
    both give slot (kz*4 + ky)*4 + kx, the order of ops.geom_conv3d's taps"""
    from semantic_segmentation_amd import ops
    w = torch.arange(3 * 5 * 64, dtype=torch.float32).reshape(3, 5, 4, 4, 4)
    want = d3.pack_slots(w, False)
    for kh, kw in ((16, 4), (8, 8)):
        v = w.view(3, 5, kh, kw)
        assert torch.equal(v.permute(2, 3, 0, 1).reshape(kh * kw, 3, 5), want)
    assert torch.equal(ops.conv3d_weight_view(w), w.view(3, 5, 16, 4))
    assert want[(2 * 4 + 1) * 4 + 3, 1, 2] == w[1, 2, 2, 1, 3]
    g = ops.geom_conv3d(1, 4, 4, 4, 8, 8, 4, 2, 1)
    assert [(g.tap_dz[t], g.tap_dy[t], g.tap_dx[t]) for t in (0, 1, 4, 16, 63)] == [(-1, -1, -1), (-1, -1, 0), (-1, 0, -1), (0, -1, -1), (2, 2, 2)]


# ================================================================================================ the statement
def assert_1e9(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    for k in ref:
        assert float((got[k] - ref[k]).norm()) <= 1e-9 * float(ref[k].norm()), k


@pytest.mark.parametrize("cid", sorted(d3.NET_CASES))
def test_statement_equals_autograd(cid):
    kind, cin, ndf, nl, norm, N, vol, train, dtn, need_dx = d3.NET_CASES[cid]
    sd, x = d3.net_case(cid)
    net = d3.torch_module(kind, cin, ndf, nl, norm)
    net.load_state_dict(sd, strict=True)                            # the key set
    net.double().train(train)
    xx = x.double().requires_grad_(True)
    out = net.forward(xx)
    dl = ir.dlogits_of(out.detach(), d3.NET_SEED)
    (out * dl).sum().backward()
    state, logits = d3.forward_state(sd, x, train)
    assert logits.shape == out.shape and ir.rel_err(logits, out.detach()) <= 1e-9
    res = d3.replay(state, dl, True)
    got = d3.flat(res[:2])
    ref = {k: p.grad for k, p in net.named_parameters()}
    ref["dx"] = xx.grad
    assert set(res[2]) == ({k for k in sd if k.endswith(".bias") and k[:-5] + ".weight" in sd and sd[k[:-5] + ".weight"].dim() == 5}
                           - {state["recs"][0]["name"] + ".bias", state["recs"][-1]["name"] + ".bias"} if norm == "instance" else set())
    for k, sc in res[2].items():                                    # the bias in front of the norm: zero up to rounding on both sides
        assert float(got.pop(k).abs().max()) <= 1e-9 * sc and float(ref.pop(k).abs().max()) <= 1e-9 * sc
    assert_1e9(got, ref)
    assert d3.replay(state, dl, False)[1] is None


def test_no_activation_sign_is_undecided_at_the_seed():
    """d_U = 0 in every bound of tests/test_disc3d_networks_gpu.py (on the statement's own forward with the engine's stores)"""
    for cid, c in d3.NET_CASES.items():
        sd, x = d3.net_case(cid)
        assert d3.undecided(d3.forward_state(sd, x, c[7], store=ir.TORCH_DT[c[8]])[0])[1] == 0, cid


@pytest.mark.parametrize("i", range(len(FIXTURES["pix2pix3d_disc"])))
def test_statement_equals_the_reference_fixture(i, golden_dir):
    f = FIXTURES["pix2pix3d_disc"][i]
    g = dict(np.load(os.path.join(golden_dir, "pix2pix3d_disc.npz")))
    t = f["tag"] + "/"
    sd, x = fixture_state_dict(f), fixture_input(f)
    assert np.array_equal(g[t + "input"], x.numpy()) and g[t + "input"].dtype == np.float32
    assert {k[len(t + "wsum/"):] for k in g if k.startswith(t + "wsum/")} == set(sd)          # the reference's key set (strict=True there)
    for k, v in sd.items():
        assert np.array_equal(g[t + "wsum/" + k], tensor_checksum(v)), k
    state, logits = d3.forward_state(sd, x, True)
    assert ir.rel_err(logits, torch.from_numpy(g[t + "logits"])) < 1e-9
    assert ir.rel_err(d3.forward_state(perturbed_running(sd, f["seed"] + 3), x, False)[1], torch.from_numpy(g[t + "logits_eval"])) < 1e-9
    dense = fixture_dense(logits.shape, f)
    assert np.array_equal(g[t + "dense"], dense.numpy())
    res = d3.replay(state, dense, True)
    got = d3.flat(res[:2])
    keys = {k[len(t + "gsum/"):] for k in g if k.startswith(t + "gsum/")}
    assert keys == set(got), keys ^ set(got)
    for k in keys:
        s_got, s_ref = grad_summary(got[k]), g[t + "gsum/" + k]
        if k in res[2]:                          # in front of the norm: zero up to rounding on both sides
            assert np.abs(s_got).max() <= 1e-9 * res[2][k] and np.abs(s_ref).max() <= 1e-9 * res[2][k], k
        else:
            assert np.linalg.norm(s_got - s_ref) <= 1e-9 * np.linalg.norm(s_ref), k


def _fixture_replays(f, dt):
    sd, x = fixture_state_dict(f), fixture_input(f)
    st64, logits = d3.forward_state(sd, x, True)
    dense = fixture_dense(logits.shape, f)
    res = d3.replay(st64, dense, True)
    st16 = d3.forward_state(sd, x, True, store=dt)[0]
    return sd, x, dense, d3.flat(res[:2]), d3.flat(d3.replay(st16, dense, True, dt)[:2]), st16, set(res[2])


@pytest.mark.parametrize("i", range(len(FIXTURES["pix2pix3d_disc"])))
def test_summary_bound_passes_a_right_implementation_and_tells_wrong_ones(i, golden_dir):
    """disc3d_reference.summary_failures, the bound tests/test_disc3d_networks_gpu.py holds the engine's gradient summaries to against the
    STORED ones: the statement with the engine's 16-bit stores passes on every tensor, and so do right implementations whose conv
    weights are perturbed by 3e-7 relative (a few fp32 roundoffs: another accumulation order stands in) -- their plain summary error
    |summary - stored| / |stored| is printed beside the 16-bit statement's and runs from far below to several times it, which is why the
    bound is taken per component from the full tensor's error and not as 4 times that one figure.  Each backward mutant that is a
    different function on the part misses the bound on at least one tensor."""
    f = FIXTURES["pix2pix3d_disc"][i]
    g = dict(np.load(os.path.join(golden_dir, "pix2pix3d_disc.npz")))
    t, dt = f["tag"] + "/", torch.float16
    sd, x, dense, r64, r16, st16, cancelled = _fixture_replays(f, dt)
    keys = sorted(set(r64) - cancelled)
    e16 = {k: ir.rel_err(r16[k], r64[k]) for k in keys}

    def failures(got):
        return {k: d3.summary_failures(grad_summary(got[k]), g[t + "gsum/" + k], r64[k].numel(), e16[k]) for k in keys}
    assert not any(bad for bad, _ in failures(r16).values())
    for seed in range(3):
        gen = torch.Generator().manual_seed(seed)
        sdp = {k: v * (1 + 3e-7 * torch.randn(v.shape, generator=gen)) if v.dim() == 5 else v for k, v in sd.items()}
        rv = d3.flat(d3.replay(d3.forward_state(sdp, x, True, store=dt)[0], dense, True, dt)[:2])
        res = failures(rv)
        for k in keys:
            want = g[t + "gsum/" + k]
            plain = np.linalg.norm(grad_summary(rv[k]) - want) / max(np.linalg.norm(grad_summary(r16[k]) - want), 1e-300)
            print(f"{t}{k} seed {seed}: plain summary error {plain:.3g} x the 16-bit statement's; shares of the bound {res[k][1]}")
        assert not any(bad for bad, _ in res.values()), {k: v for k, v in res.items() if v[0]}
    for mutant in d3.BWD_NET_MUTANTS:
        same_function = (f["kind"] == "pixel" and mutant.startswith("dgrad")) or \
                        (mutant in ("bn_count_without_d", "drop_c2") and f["norm"] == "instance")
        res = failures(d3.flat(d3.replay(st16, dense, True, dt, mutant=mutant)[:2]))
        print(f"{t}{mutant}: misses {[k for k, v in res.items() if v[0]][:4]}")
        # through the summaries alone `drop_c2` does not show on the BatchNorm PatchGAN part, whose dense-gradient e16 is 3e-2 (bound
        # 1.2e-1): the pixel part catches it, and so does the full-tensor bound on this part (test_network_bounds_tell_... above)
        invisible = same_function or (t == "d2_bn/" and mutant == "drop_c2")
        assert any(bad for bad, _ in res.values()) != invisible, (t, mutant)


# ================================================================================================ the public surface without a device
def test_threed_surface_key_sets_and_refusals_by_name():
    import argparse
    import functools
    import torch.nn as nn
    from semantic_segmentation_amd.models_pix2pix import create_model, networks
    assert networks.get_norm_layer("batch", threed=True).func is nn.BatchNorm3d and networks.get_norm_layer("batch").func is nn.BatchNorm2d
    assert networks.get_norm_layer("instance", threed=True).func is nn.InstanceNorm3d
    d = networks.define_D(2, 64, "basic", norm="batch", threed=True)
    assert isinstance(d, networks.NLayerDiscriminator) and d.threed and d.engine.net is d
    shapes = {k: tuple(v.shape) for k, v in d.state_dict().items()}
    assert shapes["model.0.weight"] == (64, 2, 4, 4, 4) and shapes["model.8.weight"] == (512, 256, 4, 4, 4)
    assert shapes["model.11.weight"] == (1, 512, 4, 4, 4) and shapes["model.11.bias"] == (1,) and "model.2.bias" not in shapes
    assert isinstance(d.model[3], nn.BatchNorm3d) and isinstance(d.model[2], nn.Conv3d)
    for kind, cin, ndf, nl, norm in (("patch", 2, 64, 3, "batch"), ("patch", 2, 16, 2, "instance"), ("pixel", 2, 64, None, "batch"),
                                     ("pixel", 4, 16, None, "instance")):
        nlayer = networks.get_norm_layer(norm, threed=True)
        net = networks.NLayerDiscriminator(cin, ndf, nl, nlayer) if kind == "patch" else networks.PixelDiscriminator(cin, ndf, nlayer)
        ref = d3.torch_module(kind, cin, ndf, nl, norm)
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        from golden_util_disc3d import state_dict_of
        sd = state_dict_of(kind, 1, cin, ndf, nl, norm)
        net.load_state_dict(sd, strict=True)
        assert set(net.engine.param_names()) == {k for k, v in sd.items() if v.is_floating_point() and "running" not in k}
        assert [i for i, _, _ in net.engine.layout()] == d3.net_layout(sd)[1]
    # the 2-D surface has not moved
    d2 = networks.define_D(2, 64, "basic")
    assert not d2.threed and isinstance(d2.model[0], nn.Conv2d) and type(d2.engine).__name__ == "DiscriminatorEngine"
    # refused by name before the engine asks for a device (a CPU tensor otherwise fails with RuntimeError)
    with pytest.raises(NotImplementedError, match="up to 16"):
        networks.define_D(17, 64, "basic", threed=True)(torch.zeros(1, 17, 24, 24, 24))
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        networks.define_D(2, 20, "basic", threed=True)(torch.zeros(1, 2, 24, 24, 24))
    with pytest.raises(NotImplementedError, match="at most 128"):
        networks.define_D(2, 136, "pixel", threed=True)(torch.zeros(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="volume"):
        d(torch.zeros(1, 2, 32, 32))
    with pytest.raises(ValueError, match="image batch"):
        d2(torch.zeros(1, 2, 24, 32, 32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        d(torch.zeros(1, 2, 24, 24, 24))
    with pytest.raises(NotImplementedError, match="affine"):
        networks.NLayerDiscriminator(2, 16, 2, functools.partial(nn.InstanceNorm3d, affine=True, track_running_stats=False))
    with pytest.raises(NotImplementedError):
        create_model(argparse.Namespace(model="pix2pix3d"))


NEW_SYMBOLS = ("gs_conv3d_img_fwd", "gs_conv3d_img_wgrad_ws_floats", "gs_conv3d_img_wgrad", "gs_conv3d_img_dgrad", "gs_conv3d_head_fwd",
               "gs_conv3d_head_bwd_ws_floats", "gs_conv3d_head_bwd")


def test_library_exports_the_new_entry_points():
    """declared in include/gsseg.h with the reference lines they replace, bound in _lib.PROTOTYPES, exported by the built library; header,
    binding and library agree on the ABI version; the workspace queries answer without a device"""
    import re
    from semantic_segmentation_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gsseg.h")).read()
    assert "GenSeg-3D/models/networks.py:829" in hdr and "GenSeg-3D/models/networks.py:850" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in gsseg.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+GS_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == lib.gs_abi_version()
    # k4: 2 channels per grid.y chunk, one slab per block, at most 256 blocks; k1: depth folded into the rows, four voxel parts
    assert lib.gs_conv3d_img_wgrad_ws_floats(1, 1, 1, 1, 2, 64, 4) == 1 * 1 * 64 * 2 * 64
    assert lib.gs_conv3d_img_wgrad_ws_floats(4, 32, 32, 32, 2, 64, 4) == 256 * 64 * 2 * 64
    assert lib.gs_conv3d_img_wgrad_ws_floats(1, 3, 4, 5, 16, 8, 1) == 3 * 4 * 8 * 16
    assert lib.gs_conv3d_img_wgrad_ws_floats(1, 3, 4, 5, 16, 8, 3) == 0
    assert lib.gs_conv3d_head_bwd_ws_floats(2, 3, 4, 8, 512, 4) == 3 * (512 * 64 + 1)
    assert lib.gs_conv3d_head_bwd_ws_floats(4, 64, 64, 64, 128, 1) == 256 * 129


# ================================================================================================ the GPU bounds and the mutants
def logits_bound(ref64, l16):
    return 4 * max(ir.rel_err(l16, ref64), pr.FLOOR32)


@pytest.mark.parametrize("cid", sorted(d3.NET_CASES))
def test_network_bounds_tell_the_wrong_implementations(cid):
    """On the GPU tests' seeds and shapes: the right forward with 16-bit stores passes the logits bound (it IS e16) and its replay passes
    compare(); each wrong one does not.  Invisible by construction, and where it is caught instead:
      * PixelDiscriminator (k 1, stride 1, no pad): every tap / pad / stride / class mutant is the right function (the PatchGAN cases);
      * `depth_pad_front_only` needs a first layer whose last tap reaches the far pad: every PatchGAN case here has an even depth;
      * `in_stats_per_slice` under BatchNorm3d, `bn_count_without_d` and `drop_c2` under InstanceNorm3d or in eval mode (running
        statistics: c1 = c2 = 0): the other norm's / the train cases;
      * `dgrad_depth_classes` where no stride-2 layer's data gradient is asked for (d1_bn_1layer has only its first layer at stride
        2: visible through dx alone, which that case asks for);
      * without dx (d6_in_nodx) the first layer's data gradient is not formed: the mutants still show in the middle layers."""
    kind, cin, ndf, nl, norm, N, vol, train, dtn, need_dx = d3.NET_CASES[cid]
    dt = ir.TORCH_DT[dtn]
    sd, x = d3.net_case(cid)
    ref64 = d3.forward_state(sd, x, train)[1]
    state16, l16 = d3.forward_state(sd, x, train, store=dt)
    bound = logits_bound(ref64, l16)
    for mutant in d3.FWD_NET_MUTANTS:
        same_function = (kind == "pixel" and mutant != "in_stats_per_slice") or (mutant == "in_stats_per_slice" and norm == "batch")
        err = ir.rel_err(d3.forward_state(sd, x, train, store=dt, mutant=mutant)[1], ref64)
        print(f"{cid} {mutant}: err {err:.3g} bound {bound:.3g}")
        assert (err > bound) != same_function, (cid, mutant, err, bound)
    dl = ir.dlogits_of(ref64, d3.NET_SEED)
    rp = d3.replays(state16, dl, need_dx, dt)
    _, bad = d3.hold(rp[1], rp, dt)
    assert not bad
    for mutant in d3.BWD_NET_MUTANTS:
        same_function = (kind == "pixel" and mutant.startswith("dgrad")) or \
                        (mutant in ("bn_count_without_d", "drop_c2") and (norm == "instance" or not train))
        got = d3.flat(d3.replay(state16, dl, need_dx, dt, mutant=mutant)[:2])
        rep, bad = d3.hold(got, rp, dt)
        print(f"{cid} {mutant}: fails {sorted(bad)[:4]}")
        assert bool(bad) != same_function, (cid, mutant, bad)
