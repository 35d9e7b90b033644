"""GPU (-m gpu): ``batch["view_counts"]`` through VolumetricTriangulationNet and AlgebraicTriangulationNet.  The fixture, shapes and helpers are those of
tests/test_gpu_view_mask_models.py (B = 3, 128^2, V = 32; masks 1111 / 1011 / 0101, i.e. counts 4, 3, 2 after ``ragged_batch``).

  11. the fp32 ragged forward against the REFERENCE run per sample on its own views (tests/golden/view_mask_small.npz) and its fp64 truth, gated as
      tests/test_gpu_cascade.py gates: err <= max(2 x the reference's own fp32 error, floor); the bf16 deviation and the distance to the padded masked
      forward are recorded, not gated (9 and 12 images may select different backbone kernels);
  12. counts 4, 4, 4: every returned tensor equals the plain (3, 4) forward's, reshaped, bit for bit, fp32 and bf16, graph on and off;
  13. other counts on a captured plan equal a fresh model's result; plain forwards before and after are unchanged;
  14. ``keypoint_stats`` with ``view_counts`` returns B rows and leaves the joints' bits alone;
  15. the four plan-level C entries through ctypes equal the Python host bit for bit, fp32 and bf16; their refusals return the documented codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from oracle import truth as T
from test_gpu_cascade import FLOOR_2D, FLOOR_JOINTS, _gate
from test_gpu_view_mask_models import _batch, _net, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, NV = 3, 4


def _ragged(inp, mask, P=None):
    from mvn.datasets.utils import ragged_batch
    images, Pr, rb = ragged_batch(inp["images"], P, _batch(inp, np.asarray(mask)))
    return (images.to(DEV), rb) if P is None else (images.to(DEV), Pr.to(DEV), rb)


def _regroup(inp, counts):
    """The fixture's 12 images dealt out anew: the first sum(counts) images of the padded batch, ``counts[b]`` of them to sample b."""
    from mvn.utils.multiview import Camera
    n = int(sum(counts))
    flat = [(b, v) for b in range(B) for v in range(NV)][:n]
    cams = [Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _, v in flat]
    images = torch.stack([inp["images"][b, v] for b, v in flat]).to(DEV)
    return images, {"cameras": cams, "pred_keypoints_3d": inp["pred_keypoints_3d"][:len(counts)], "view_counts": list(counts)}


# ---- 11. against the reference on each sample's own views --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["vol_softmax", "vol_conf_norm"])
def test_ragged_fp32_forward_vs_reference_on_each_samples_views(golden_dir, case):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    masks = g["masks"]
    images, rb = _ragged(inp, masks)
    assert rb["view_counts"] == [4, 3, 2] and images.shape[0] == 9
    net = _net(case, cfgs, sds, torch.float32, True)
    out = net(images, None, rb)
    torch.cuda.synchronize()
    tag = "view_counts %s/" % case
    h, w = out[1].shape[2:]
    assert tuple(out[0].shape) == (B, 17, 3) and tuple(out[1].shape) == (9, 32, h, w) and tuple(out[2].shape) == (B, 17, 32, 32, 32)
    assert len(out[4]) == B and tuple(out[5].shape) == (B, 32, 32, 32, 3) and tuple(out[6].shape) == (B, 3)
    bad = [_gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(out[0].cpu().numpy(), g["truth/" + case + "/kp"]), float(g["ref32_err/" + case + "/kp"]),
                 FLOOR_JOINTS)]
    assert not [b for b in bad if b], [b for b in bad if b]
    padded = net(inp["images"].to(DEV), None, _batch(inp, masks))
    torch.cuda.synchronize()
    on = torch.from_numpy(masks.astype(bool)).to(DEV)
    if case == "vol_conf_norm":
        conf = out[3]
        assert tuple(conf.shape) == (9, 32)
        sums = torch.stack([conf[lo:hi].sum(0) for lo, hi in ((0, 4), (4, 7), (7, 9))])
        assert torch.allclose(sums, torch.ones_like(sums), atol=1e-5)          # normalised over each sample's views
        record(tag + "vol_confidences fp32 vs fp64 truth, recorded",
               {"err_ours": T.max_rel(conf.cpu().numpy(), g["truth/vol_conf_norm/conf"][masks.astype(bool)]), "ref32_err": float(g["ref32_err/vol_conf_norm/conf"])})
        record(tag + "vol_confidences: max |ragged - padded masked|, recorded", float((conf - padded[3][on]).abs().max()))
    else:
        assert out[3] is None
    record(tag + "joints: max |ragged - padded masked| (mm), recorded", float((out[0] - padded[0]).abs().max()))
    record(tag + "features: max |ragged - padded masked|, recorded", float((out[1] - padded[1][on]).abs().max()))
    net16 = _net(case, cfgs, sds, torch.bfloat16, True)
    kp16 = net16(images, None, rb)[0].cpu().numpy()
    record(tag + "bf16 joints deviation from the fp64 truth (max rel, 1 mm floor), recorded", T.joints_rel(kp16, g["truth/" + case + "/kp"]))
    assert np.isfinite(kp16).all()


# ---- 12. equal counts == the plain forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ["vol_softmax", "vol_conf_norm"])
def test_equal_counts_equal_the_plain_forward(golden_dir, case, dtype, graph):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    net = _net(case, cfgs, sds, dtype, graph)
    plain = net(inp["images"].to(DEV), None, _batch(inp))
    images, rb = _ragged(inp, np.ones((B, NV), dtype=np.uint8))
    assert rb["view_counts"] == [4, 4, 4]
    for rep in ("first", "replay"):
        out = net(images, None, rb)
        torch.cuda.synchronize()
        what = "%s %s %s %s" % (case, dtype, "graph" if graph else "eager", rep)
        for i, name in ((0, "keypoints_3d"), (2, "volumes"), (5, "coord_volumes"), (6, "base_points")):
            assert torch.equal(out[i], plain[i]), "%s %s: max |d| %.3e" % (what, name, float((out[i].double() - plain[i].double()).abs().max()))
        assert torch.equal(out[1], plain[1].reshape(out[1].shape)), what + " features"
        if case == "vol_conf_norm":
            assert torch.equal(out[3], plain[3].reshape(out[3].shape)), what + " vol_confidences"
        else:
            assert out[3] is None and plain[3] is None
        assert all(np.array_equal(a.position, b.position) and np.array_equal(a.sides, b.sides) for a, b in zip(out[4], plain[4]))
    assert len(net._plans) == 2          # its own plan, beside the plain one


# ---- 13. other counts on a captured plan -------------------------------------------------------------------------------------------------------------------
def test_other_counts_on_a_captured_plan(golden_dir):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images1, rb1 = _regroup(inp, [4, 3, 2])
    images2, rb2 = _regroup(inp, [2, 3, 4])
    assert torch.equal(images1, images2)
    net = _net("vol_softmax", cfgs, sds, torch.float32, True)
    plain_in = inp["images"].to(DEV)
    before = net(plain_in, None, _batch(inp))
    first = net(images1, None, rb1)          # records and captures the ragged plan
    second = net(images2, None, rb2)         # replays it with other counts
    after = net(plain_in, None, _batch(inp))
    torch.cuda.synchronize()
    assert len(net._plans) == 2
    want2 = _net("vol_softmax", cfgs, sds, torch.float32, True)(images2, None, rb2)
    want1 = _net("vol_softmax", cfgs, sds, torch.float32, True)(images1, None, rb1)
    torch.cuda.synchronize()
    assert torch.equal(second[0], want2[0]) and torch.equal(first[0], want1[0]) and torch.equal(second[2], want2[2])
    assert torch.isfinite(second[0]).all() and not torch.equal(second[0], first[0])
    for i in (0, 1, 2, 5, 6):
        assert torch.equal(after[i], before[i]), "plain forwards around the ragged ones differ in output %d" % i


# ---- 14. keypoint_stats ------------------------------------------------------------------------------------------------------------------------------------
def test_keypoint_stats_with_view_counts(golden_dir):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images, rb = _ragged(inp, g["masks"])
    net = _net("vol_softmax", cfgs, sds, torch.float32, True)
    kp = net(images, None, rb)[0]
    assert net.last_keypoint_stats is None
    net.keypoint_stats = True
    kp_s = net(images, None, rb)[0]
    torch.cuda.synchronize()
    st = net.last_keypoint_stats
    assert st is not None and tuple(st.peak.shape) == (B, 17) and tuple(st.covariance.shape) == (B, 17, 3, 3) and torch.isfinite(st.covariance).all()
    assert torch.equal(kp_s, kp)


# ---- the algebraic model: 11, 12 and 13 -----------------------------------------------------------------------------------------------------------------------
def test_ragged_alg_fp32_forward_vs_reference_on_each_samples_views(golden_dir):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    masks = g["masks"]
    on = masks.astype(bool)
    images, Pr, rb = _ragged(inp, masks, P)
    net = _net("alg", cfgs, sds, torch.float32, True)
    kp3, kp2, hm, conf = net(images, Pr, rb)
    torch.cuda.synchronize()
    assert tuple(kp3.shape) == (B, 17, 3) and tuple(kp2.shape) == (9, 17, 2) and tuple(conf.shape) == (9, 17) and tuple(hm.shape[:2]) == (9, 17)
    err = lambda name: float(g["ref32_err/alg/" + name])
    tru = lambda name: g["truth/alg/" + name]
    tag = "view_counts alg/"
    bad = [_gate(tag + "keypoints_2d fp32 (max rel, 1 px floor)", T.joints_rel(kp2.cpu().numpy(), tru("kp2")[on]), err("kp2"), FLOOR_2D),
           _gate(tag + "confidences fp32", T.max_rel(conf.cpu().numpy(), tru("conf")[on]), err("conf"), FLOOR_2D),
           _gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(kp3.cpu().numpy(), tru("kp3")), err("kp3"), FLOOR_JOINTS)]
    assert not [b for b in bad if b], [b for b in bad if b]
    padded = net(inp["images"].to(DEV), P.to(DEV), _batch(inp, masks))
    torch.cuda.synchronize()
    ond = torch.from_numpy(on).to(DEV)
    record(tag + "joints: max |ragged - padded masked| (mm), recorded", float((kp3 - padded[0]).abs().max()))
    record(tag + "keypoints_2d: max |ragged - padded masked| (px), recorded", float((kp2 - padded[1][ond]).abs().max()))
    kp16 = _net("alg", cfgs, sds, torch.bfloat16, True)(images, Pr, rb)[0].cpu().numpy()
    record(tag + "bf16 joints deviation from the fp64 truth (max rel, 1 mm floor), recorded", T.joints_rel(kp16, tru("kp3")))
    assert np.isfinite(kp16).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_alg_equal_counts_equal_the_plain_forward_and_other_counts_reuse_the_plan(golden_dir, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    net = _net("alg", cfgs, sds, dtype, True)
    before = net(inp["images"].to(DEV), P.to(DEV), _batch(inp))
    images, Pr, rb = _ragged(inp, np.ones((B, NV), dtype=np.uint8), P)
    out = net(images, Pr, rb)
    torch.cuda.synchronize()
    assert torch.equal(out[0], before[0])
    for i, name in ((1, "keypoints_2d"), (2, "heatmaps"), (3, "alg_confidences")):
        assert torch.equal(out[i], before[i].reshape(out[i].shape)), "%s %s" % (dtype, name)
    assert len(net._plans) == 2
    # counts 5, 3, 4 and 3, 4, 5 of the same 12 images: one more plan (NVcap 8), shared by both; a fresh model gives the same
    a = net(images, Pr, dict(rb, view_counts=[5, 3, 4]))
    b = net(images, Pr, dict(rb, view_counts=[3, 4, 5]))
    after = net(inp["images"].to(DEV), P.to(DEV), _batch(inp))
    torch.cuda.synchronize()
    assert len(net._plans) == 3
    want = _net("alg", cfgs, sds, dtype, True)(images, Pr, dict(rb, view_counts=[3, 4, 5]))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(b, want)) and not torch.equal(a[0], b[0]) and torch.isfinite(b[0]).all()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])          # per-view outputs do not depend on the grouping
    assert all(torch.equal(x, y) for x, y in zip(after, before))


# ---- 15. the C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def _named(sd):
    keep, arr = [], (H.NamedTensor * len(sd))()
    for i, (k, v) in enumerate(sd.items()):
        t = v.detach().float().contiguous()
        keep.append(t)
        arr[i].name, arr[i].data, arr[i].ndim = k.encode(), t.data_ptr(), max(1, t.dim())
        for j, n in enumerate(t.shape if t.dim() else (1,)):
            arr[i].shape[j] = n
    return keep, arr


def _vol_config(cfg, dtype, nb, cap):
    m = cfg.model
    pc = H.VolPlanConfig()
    pc.dtype = H.LT_F32 if dtype == torch.float32 else H.LT_BF16
    pc.num_layers, pc.style_caffe, pc.num_joints = m.backbone.num_layers, 0, 17
    pc.B, pc.NV, pc.H, pc.W = nb, cap, 128, 128
    pc.volume_size, pc.cuboid_side, pc.volume_multiplier = m.volume_size, m.cuboid_side, m.volume_multiplier
    pc.volume_softmax, pc.aggregation, pc.transfer_cmu_to_human36m, pc.use_graph = int(bool(m.volume_softmax)), H.AGG[m.volume_aggregation_method], 0, 1
    return pc


def _alg_config(cfg, dtype, nb, cap):
    m = cfg.model
    pc = H.AlgPlanConfig()
    pc.model, pc.dtype = H.LT_MODEL_ALG, H.LT_F32 if dtype == torch.float32 else H.LT_BF16
    pc.num_layers, pc.style_caffe, pc.num_joints = m.backbone.num_layers, int(m.backbone.get("style", "simple") == "caffe"), m.backbone.num_joints
    pc.B, pc.NV, pc.H, pc.W = nb, cap, 128, 128
    pc.use_confidences = int(bool(m.get("use_confidences", False)))
    pc.heatmap_softmax, pc.heatmap_multiplier = int(bool(m.get("heatmap_softmax", True))), float(m.get("heatmap_multiplier", 1.0))
    pc.direct_optimization, pc.reprojection_error_epsilon, pc.use_graph = 1, 15.0, 1
    return pc


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _vol_forward(plan, entry, images, cams, counts, base, V=32):
    """lt_plan_forward_vol_ragged (counts) or lt_plan_forward_vol (None) -> (rc, keypoints_3d, volumes, features, vol_confidences)."""
    n, nb = images.shape[0] if counts is not None else images.shape[0] * images.shape[1], len(base)
    K = np.ascontiguousarray(np.stack([c.K for c in cams]), dtype=np.float64)
    R = np.ascontiguousarray(np.stack([c.R for c in cams]), dtype=np.float64)
    t = np.ascontiguousarray(np.stack([np.asarray(c.t).reshape(3) for c in cams]), dtype=np.float64)
    bp = np.ascontiguousarray(np.asarray(base, dtype=np.float64)[:, 6, :3])
    kp, vols = torch.full((nb, 17, 3), float("nan"), device=DEV), torch.empty(nb, 17, V, V, V, device=DEV)
    feats, conf = torch.empty(n, 32, 32, 32, device=DEV), torch.empty(n, 32, device=DEV)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = torch.cuda.current_stream().cuda_stream
    if counts is None:
        rc = H.lib().lt_plan_forward_vol(plan, images.data_ptr(), dp(K), dp(R), dp(t), dp(bp), None, kp.data_ptr(), vols.data_ptr(), None, None, None, st)
    else:
        keep, pc = _i32(counts)
        rc = getattr(H.lib(), entry)(plan, images.data_ptr(), dp(K), dp(R), dp(t), pc, dp(bp), None, kp.data_ptr(), vols.data_ptr(), feats.data_ptr(), None, None, st)
    torch.cuda.synchronize()
    return rc, kp, vols, feats


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_ragged_vol_plan_equals_the_python_host(golden_dir, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    images, rb1 = _regroup(inp, [4, 3, 2])
    _, rb2 = _regroup(inp, [2, 3, 4])
    images = images.contiguous()
    for case in ("vol_softmax", "vol_conf_norm"):
        net = _net(case, cfgs, sds, dtype, True)
        want1, want2 = net(images, None, rb1), net(images, None, rb2)
        torch.cuda.synchronize()
        keep, arr = _named(sds[case])
        pc = _vol_config(cfgs[case], dtype, 3, 4)
        plan = C.c_void_p()
        H.check(lib.lt_plan_create_vol_ragged(C.byref(pc), 9, arr, len(sds[case]), C.byref(plan)), "lt_plan_create_vol_ragged")
        try:
            for rnd in range(2):          # the capturing forward and a replay
                rc, kp, vols, feats = _vol_forward(plan, "lt_plan_forward_vol_ragged", images, rb1["cameras"], [4, 3, 2], rb1["pred_keypoints_3d"])
                assert rc == 0, err()
                assert torch.equal(kp, want1[0]) and torch.equal(vols, want1[2]) and torch.equal(feats, want1[1]), (case, dtype, rnd, float((kp - want1[0]).abs().max()))
            rc, kp, vols, _ = _vol_forward(plan, "lt_plan_forward_vol_ragged", images, rb2["cameras"], [2, 3, 4], rb2["pred_keypoints_3d"])
            assert rc == 0 and torch.equal(kp, want2[0]) and torch.equal(vols, want2[2]), (case, dtype, "other counts")
            # refusals, all LT_ERR_INVALID: counts that do not sum to T, a count of 0, one above NVcap; the plain forward; a view mask
            for bad, msg in (([4, 3, 3], "sums to 10"), ([5, 4, 0], "sample 0 has 5 views"), ([4, 0, 5], "sample 1 has 0 views")):
                assert _vol_forward(plan, "lt_plan_forward_vol_ragged", images, rb1["cameras"], bad, rb1["pred_keypoints_3d"])[0] == -1 and msg in err(), (bad, err())
            assert _vol_forward(plan, None, images, rb1["cameras"], None, rb1["pred_keypoints_3d"])[0] == -1 and "lt_plan_forward_vol_ragged" in err()
            m = np.ones(12, dtype=np.uint8)
            assert lib.lt_plan_set_view_mask(plan, m.ctypes.data_as(C.c_void_p)) == -1 and "ragged" in err()
            rc, kp, _, _ = _vol_forward(plan, "lt_plan_forward_vol_ragged", images, rb1["cameras"], [4, 3, 2], rb1["pred_keypoints_3d"])
            assert rc == 0 and torch.equal(kp, want1[0])          # the refusals left the plan usable
        finally:
            lib.lt_plan_destroy(plan)
        del keep, arr
    # the ragged forward on a plain plan
    from test_gpu_view_mask_models import VolCPlan
    cp = VolCPlan(cfgs["vol_softmax"], sds["vol_softmax"], dtype)
    try:
        assert _vol_forward(cp.plan, "lt_plan_forward_vol_ragged", images, rb1["cameras"], [4, 3, 2], rb1["pred_keypoints_3d"])[0] == -1 and "lt_plan_forward_vol" in err()
    finally:
        cp.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_ragged_alg_plan_equals_the_python_host(golden_dir, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    images, Pr, rb = _ragged(inp, g["masks"], P)
    images, Pr = images.contiguous(), Pr.float().contiguous()
    net = _net("alg", cfgs, sds, dtype, True)
    want = net(images, Pr, rb)
    want2 = net(images, Pr, dict(rb, view_counts=[2, 3, 4]))
    torch.cuda.synchronize()
    h, w = want[2].shape[2:]
    keep, arr = _named(sds["alg"])
    pc = _alg_config(cfgs["alg"], dtype, 3, 4)
    plan = C.c_void_p()
    H.check(lib.lt_plan_create_alg_ragged(C.byref(pc), 9, arr, len(sds["alg"]), C.byref(plan)), "lt_plan_create_alg_ragged")
    st = torch.cuda.current_stream().cuda_stream

    def forward(counts, entry="lt_plan_forward_alg_ragged"):
        o = [torch.full((3, 17, 3), float("nan"), device=DEV), torch.full((9, 17, 2), float("nan"), device=DEV), torch.full((9, 17, h, w), float("nan"), device=DEV),
             torch.full((9, 17), float("nan"), device=DEV)]
        if counts is None:
            rc = lib.lt_plan_forward_alg(plan, images.data_ptr(), Pr.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), st)
        else:
            k, pcnt = _i32(counts)
            rc = lib.lt_plan_forward_alg_ragged(plan, images.data_ptr(), Pr.data_ptr(), pcnt, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), st)
        torch.cuda.synchronize()
        return rc, o
    try:
        for rnd in range(2):
            rc, o = forward([4, 3, 2])
            assert rc == 0, err()
            for name, a, b in zip(("keypoints_3d", "keypoints_2d", "heatmaps", "alg_confidences"), o, want):
                assert torch.equal(a, b), "%s forward %d %s: max |d| %.3e" % (dtype, rnd, name, float((a - b).abs().max()))
        rc, o = forward([2, 3, 4])
        assert rc == 0 and all(torch.equal(a, b) for a, b in zip(o, want2))
        for bad, msg in (([4, 4, 2], "sums to 10"), ([4, 4, 1], "sample 2 has 1 view,"), ([5, 2, 2], "sample 0 has 5 views")):
            assert forward(bad)[0] == -1 and msg in err(), (bad, err())
        assert forward(None)[0] == -1 and "lt_plan_forward_alg_ragged" in err()
        m = np.ones(12, dtype=np.uint8)
        assert lib.lt_plan_set_view_mask(plan, m.ctypes.data_as(C.c_void_p)) == -1 and "ragged" in err()
        assert lib.lt_plan_set_alg_keypoint_stats(plan, 1, 1, 1, 1, 1) == -2 and "ragged" in err()
        assert forward([4, 3, 2])[0] == 0
    finally:
        lib.lt_plan_destroy(plan)
    del keep, arr
    from test_gpu_plan_abi_alg import AlgCPlan
    cp = AlgCPlan(H.LT_MODEL_ALG, cfgs["alg"], sds["alg"], 3, 4, 128, dtype)
    try:
        k, pcnt = _i32([4, 3, 2])
        assert lib.lt_plan_forward_alg_ragged(cp.plan, images.data_ptr(), Pr.data_ptr(), pcnt, 1, None, None, None, st) == -1 and "lt_plan_forward_alg" in err()
    finally:
        cp.close()
