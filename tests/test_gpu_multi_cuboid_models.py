"""GPU (-m gpu): several cuboids per frame -- VolumetricTriangulationNet.forward with ``batch["cuboid_frame"]`` and the C plan host
(lt_plan_create_vol_multi / lt_plan_forward_vol_multi).

  1. the identity assignment (P = F, cuboid p on frame p) against the plain forward: all seven outputs ``torch.equal``, fp32 and bf16, graph and eager, the
     small networks and BASELINE config 2's; a replay, and another assignment of the same (F, P) on the captured plan against the plain forward on the
     frames repeated per cuboid (what a user does today);
  2. against the REFERENCE on the repeated frames (tests/golden/multi_cuboid_small.npz, tools/make_golden_multi_cuboid.py) and its fp64 truth, at the gate
     of tests/test_gpu_cascade.py::_gate -- err <= max(2 x the reference's own fp32 error, floor) -- with the floors of tests/test_gpu_truth.py; the bf16
     forward is recorded, not gated;
  3. composition with ``keypoint_stats`` and ``batch["view_mask"]``;
  4. the C ABI through ctypes alone, bit-identical to the Python host, and the cross-plan refusals;
  5. a second forward never waits for the GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from oracle import spec, synth
from oracle import truth as T
from test_multi_cuboid_cpu import F, FRAME_OF, HW, J, NV, P, V, cameras, multi_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = {"kp": 1e-4, "feat_sub": 2e-6, "vol_sub": 1e-5}          # tests/test_gpu_truth.py: FLOOR
NAMES = ("keypoints_3d", "features", "volumes", "vol_confidences", "cuboids", "coord_volumes", "base_points")


@functools.lru_cache(maxsize=4)
def _state_dict(nl, seed):
    return synth.make_state_dict(spec.vol_net_spec(nl, J, False), seed=seed, basic_block=(nl < 50))


def _model(nl, vol_size, kind, dtype, graph, seed=72, method="softmax"):
    from mvn.models.triangulation import VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(nl, vol_size, method, 1.0, kind), device=DEV)
    vol.load_state_dict(_state_dict(nl, int(seed)) if method == "softmax" else
                        synth.make_state_dict(spec.vol_net_spec(nl, J, True), seed=int(seed), basic_block=(nl < 50)), strict=True)
    vol.eval()
    vol.compute_dtype, vol.use_graph = dtype, graph
    return vol


def _joints(n, seed):
    """(n, J, 3) joints whose base points (mpii joint 6, coco mean of 11 and 12) are distinct and a few hundred mm from the origin."""
    return np.random.RandomState(seed).randn(n, J, 3) * 150.0


def _assert_same(got, want, what, rows=None):
    """All seven outputs; rows: the cuboids of ``got`` to compare with ``want``'s (per-cuboid outputs only)."""
    assert len(got) == 7
    for i, (name, x, y) in enumerate(zip(NAMES, got, want)):
        if name == "cuboids":
            assert len(x) == len(y), (what, name)
            for cx, cy in zip(x, y):
                assert np.array_equal(np.asarray(cx.position), np.asarray(cy.position)) and np.array_equal(np.asarray(cx.sides), np.asarray(cy.sides)), (what, name)
            continue
        if y is None:
            assert x is None, (what, name)
            continue
        assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert torch.isfinite(y).all(), (what, name, "the plain forward's own output is not finite")
        assert torch.equal(x, y), "%s %s: max |d| %.3e" % (what, name, float((x.double() - y.double()).abs().max()))


# ---- 1. bit identity with the plain forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ["small", "c2"])
def test_identity_assignment_equals_the_plain_forward_bit_for_bit(shape, dtype, graph):
    nl, hw, vs, nv = (18, 128, 32, 4) if shape == "small" else (152, 384, 64, 4)          # c2: BASELINE config 2's networks and shape
    vol = _model(nl, vs, "mpii", dtype, graph)
    inp = synth.make_inputs(2, nv, hw, seed=13)
    images = inp["images"].to(DEV)
    cams = cameras(inp, 2)
    kp = _joints(2, 5)
    what = "%s %s %s" % (shape, dtype, "graph" if graph else "eager")
    plain = vol(images, None, {"cameras": cams, "pred_keypoints_3d": kp})
    multi = vol(images, None, {"cameras": cams, "pred_keypoints_3d": kp, "cuboid_frame": [0, 1]})
    torch.cuda.synchronize()
    _assert_same(multi, plain, what)
    again = vol(images, None, {"cameras": cams, "pred_keypoints_3d": kp, "cuboid_frame": np.array([0, 1])})          # a replay
    torch.cuda.synchronize()
    _assert_same(again, plain, what + " (second call)")
    # another assignment of the same (F, P) on the captured plan: both cuboids on frame 1, in the other order of base points
    n_plans = len(vol._plans) if hasattr(vol, "_plans") else None
    swapped = vol(images, None, {"cameras": cams, "pred_keypoints_3d": kp[::-1].copy(), "cuboid_frame": torch.tensor([1, 1])})
    rep = vol(images[[1, 1]], None, {"cameras": cams, "pred_keypoints_3d": kp[::-1].copy()})          # what a user does today: the frame repeated
    torch.cuda.synchronize()
    if n_plans is not None:
        assert len(vol._plans) == n_plans, "a new assignment of the same (F, P) built a new plan"
    for i in (0, 2, 5, 6):
        assert torch.equal(swapped[i], rep[i]), "%s (both cuboids on frame 1) %s: max |d| %.3e" % (what, NAMES[i], float((swapped[i].double() - rep[i].double()).abs().max()))
    assert torch.equal(swapped[1], plain[1]), what + ": the features are per frame"
    assert not torch.equal(swapped[0], plain[0])


# ---- 2. against the reference on the repeated frames and its fp64 truth ------------------------------------------------------------------------------------
def _gate(name, ours, ref32, floor):
    eff = max(2.0 * ref32, floor)
    record(name + " vs fp64 truth", {"err_ours": ours, "ref32_err": ref32, "ratio": ours / max(ref32, 1e-300), "gate": eff})
    print("%s: err %.3e, reference's own %.3e, gate %.3e" % (name, ours, ref32, eff))
    return None if ours <= eff else "%s: err %.3e > max(2 x reference's %.3e, floor %.1e)" % (name, ours, ref32, floor)


def _sub(t, s):
    sl = (slice(None), slice(None)) + tuple(slice(None, None, s) for _ in range(t.dim() - 2))
    return t[sl].contiguous().numpy()


@pytest.mark.parametrize("kind,prefix", [("mpii", ""), ("coco", "coco/")])
def test_multi_cuboid_fp32_vs_reference_and_truth(golden_dir, kind, prefix):
    g = np.load(os.path.join(golden_dir, "multi_cuboid_small.npz"))
    k = lambda name: g[prefix + name]
    vcfg, vsd, inp, kp_in = multi_setup(kind, k("seeds"))
    vol = _model(18, V, kind, torch.float32, True, seed=k("seeds")[0])
    assert np.allclose(synth.state_dict_checksum({n: t.cpu() for n, t in vol.state_dict().items()}), k("vol_sd_digest"), rtol=1e-12)
    assert np.allclose(T.images_digest(inp["images"]), k("images_digest"), rtol=1e-12)
    images = inp["images"].to(DEV)
    batch = {"cameras": cameras(inp, F), "pred_keypoints_3d": kp_in, "cuboid_frame": k("frame_of")}
    kp, feats, vols, conf, cuboids, coords, base = vol(images, None, batch)
    torch.cuda.synchronize()
    assert kp.shape == (P, J, 3) and feats.shape == (F, NV, 32, HW // 4, HW // 4) and vols.shape == (P, J, V, V, V) and conf is None
    assert len(cuboids) == P and coords.shape == (P, V, V, V, 3) and base.shape == (P, 3)
    err = lambda name: float(k("ref32_err/" + name))
    tag = "multi-cuboid %s/" % kind
    s = int(k("stride"))
    bad = [_gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(kp.cpu().numpy(), k("truth/kp")), err("kp"), FLOOR["kp"]),
           _gate(tag + "features fp32", T.max_rel(_sub(feats.cpu().reshape(F * NV, 32, HW // 4, HW // 4), s), k("truth/feat_sub")), err("feat_sub"), FLOOR["feat_sub"]),
           _gate(tag + "volumes (softmaxed) fp32", T.max_rel(_sub(vols.cpu(), s), k("truth/vol_sub")), err("vol_sub"), FLOOR["vol_sub"])]
    dcv = float(np.abs(coords.cpu().numpy()[:, ::s, ::s, ::s].astype(np.float64) - k("cv_sub")).max())
    lim = 2e-7 * float(np.abs(k("cv_sub")).max())          # the coordinates' gate of the golden tests (tests/test_gpu_plan_abi.py: 2e-7)
    record(tag + "coord_volumes vs the reference's: max |d| mm", {"err_ours": dcv, "gate": lim})
    print("%scoord_volumes: max |d| %.3e mm, gate %.3e" % (tag, dcv, lim))
    if dcv > lim:
        bad.append("%scoord_volumes: max |d| %.3e mm > 2e-7 x max|ref| = %.3e" % (tag, dcv, lim))
    assert np.array_equal(base.cpu().numpy(), k("base_points")), "base_points: fp32(base), as the reference returns them"
    assert np.array_equal(np.stack([c.position for c in cuboids]), k("cuboid_pos"))
    assert not [b for b in bad if b], [b for b in bad if b]
    # bf16: deviations recorded, not gated (no measured value exists yet)
    vol.compute_dtype = torch.bfloat16
    kp16, f16, v16 = vol(images, None, batch)[:3]
    torch.cuda.synchronize()
    record(tag + "bf16 deviation from the fp64 truth",
           {"joints (max rel, 1 mm floor)": T.joints_rel(kp16.cpu().numpy(), k("truth/kp")),
            "features": T.max_rel(_sub(f16.cpu().reshape(F * NV, 32, HW // 4, HW // 4), s), k("truth/feat_sub")),
            "volumes": T.max_rel(_sub(v16.cpu(), s), k("truth/vol_sub"))})
    assert torch.isfinite(kp16).all()


# ---- 3. composition ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_keypoint_stats_compose(dtype):
    vol = _model(18, 32, "mpii", dtype, True)
    inp = synth.make_inputs(2, 4, 128, seed=13)
    images, cams = inp["images"].to(DEV), cameras(inp, 2)
    kp2, kp5 = _joints(2, 5), _joints(P, 6)
    ident = {"cameras": cams, "pred_keypoints_3d": kp2, "cuboid_frame": [0, 1]}
    five = {"cameras": cams, "pred_keypoints_3d": kp5, "cuboid_frame": list(FRAME_OF)}
    no_stats = [vol(images, None, b) for b in (ident, five)]
    assert vol.last_keypoint_stats is None
    vol.keypoint_stats = True
    plain = vol(images, None, {"cameras": cams, "pred_keypoints_3d": kp2})
    st_plain = vol.last_keypoint_stats
    for b, want, rows in ((ident, no_stats[0], 2), (five, no_stats[1], P)):
        out = vol(images, None, b)
        st = vol.last_keypoint_stats
        torch.cuda.synchronize()
        _assert_same(out, want, "keypoint_stats %s %d cuboids" % (dtype, rows))          # the joints and volumes (and everything else) keep their bits
        assert st.peak.shape == (rows, J) and st.covariance.shape == (rows, J, 3, 3) and all(bool(torch.isfinite(t.float()).all()) for t in st)
        if rows == 2:          # the identity case: the rows of the plain forward
            for name, x, y in zip(("peak", "peak_index", "mass", "covariance"), st, st_plain):
                assert torch.equal(x, y), name


@pytest.mark.parametrize("dtype,method", [(torch.float32, "softmax"), (torch.bfloat16, "softmax"), (torch.float32, "conf_norm")], ids=["f32", "bf16", "f32-conf_norm"])
def test_view_mask_composes(dtype, method):
    """mask (F, NV): frame 0 all ones, frame 1 without view 2.  The cuboids of frame 0 keep the unmasked forward's bits; those of frame 1 equal the plain
    masked forward on the repeated frames."""
    vol = _model(18, 32, "mpii", dtype, True, method=method)
    inp = synth.make_inputs(2, 4, 128, seed=13)
    images, cams = inp["images"].to(DEV), cameras(inp, 2)
    kp5 = _joints(P, 6)
    fo = list(FRAME_OF)
    mask = np.array([[1, 1, 1, 1], [1, 1, 0, 1]], dtype=np.uint8)
    five = {"cameras": cams, "pred_keypoints_3d": kp5, "cuboid_frame": fo}
    unmasked = vol(images, None, five)
    masked = vol(images, None, dict(five, view_mask=mask))
    rep = vol(images[fo], None, {"cameras": cameras(inp, P), "pred_keypoints_3d": kp5, "view_mask": mask[fo]})          # the plain masked forward, frames repeated
    torch.cuda.synchronize()
    on0 = torch.tensor([f == 0 for f in fo], device=DEV)
    for i in (0, 2):
        assert torch.equal(masked[i][on0], unmasked[i][on0]), NAMES[i] + ": a frame whose mask is all ones keeps the unmasked bits"
        assert torch.equal(masked[i], rep[i]), NAMES[i] + ": the plain masked forward on the repeated frames"
        assert not torch.equal(masked[i][~on0], unmasked[i][~on0])
    assert torch.equal(masked[5], unmasked[5]) and torch.equal(masked[6], unmasked[6])
    if method == "conf_norm":
        assert masked[3].shape == (F, NV, 32) and torch.equal(masked[3][0], unmasked[3][0]) and bool((masked[3][1, 2] == 0).all())
        assert torch.equal(masked[3][1], rep[3][1])


def test_copy_outputs_false_and_op_frame_index():
    """copy_outputs = False hands out the plan's buffers with the same bits; op.unproject_heatmaps(frame_index=) equals itself on the gathered inputs."""
    from mvn.utils import op
    vol = _model(18, 32, "mpii", torch.float32, True)
    inp = synth.make_inputs(2, 4, 128, seed=13)
    images, cams = inp["images"].to(DEV), cameras(inp, 2)
    five = {"cameras": cams, "pred_keypoints_3d": _joints(P, 6), "cuboid_frame": list(FRAME_OF)}
    want = vol(images, None, five)
    vol.copy_outputs = False
    got = vol(images, None, five)
    torch.cuda.synchronize()
    for i in (0, 1, 2, 5, 6):
        assert torch.equal(got[i], want[i]), NAMES[i]
    g = torch.Generator().manual_seed(3)
    hm = torch.randn(2, 3, 4, 8, 8, generator=g).to(DEV)
    proj = torch.randn(2, 3, 3, 4, generator=g).to(DEV)
    cv = (torch.randn(P, 4, 4, 16, 3, generator=g) * 500).to(DEV)
    conf = (torch.rand(2, 3, 4, generator=g) + 0.1).to(DEV)
    idx = torch.tensor(FRAME_OF, device=DEV)
    mask = torch.tensor([[1, 0, 1], [1, 1, 1]], dtype=torch.uint8)
    for fi in (list(FRAME_OF), np.array(FRAME_OF), idx):
        a = op.unproject_heatmaps(hm, proj, cv, "conf_norm", conf, frame_index=fi)
        assert a.shape == (P, 4, 4, 4, 16) and torch.equal(a, op.unproject_heatmaps(hm[idx], proj[idx], cv, "conf_norm", conf[idx]))
    a = op.unproject_heatmaps(hm, proj, cv, "softmax", view_mask=mask, frame_index=list(FRAME_OF))
    assert torch.equal(a, op.unproject_heatmaps(hm[idx], proj[idx], cv, "softmax", view_mask=mask[list(FRAME_OF)]))
    with pytest.raises(ValueError):
        op.unproject_heatmaps(hm, proj, cv, "sum", frame_index=[0, 1, 2, 0, 1])
    with pytest.raises(ValueError):
        op.unproject_heatmaps(hm, proj, cv, "sum", frame_index=[0, 1])


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------------------------------
class MultiCPlan:
    """lt_plan_create_vol_multi / lt_plan_forward_vol_multi through ctypes: what a host in any language does."""

    def __init__(self, vcfg, vsd, nf, ncub, nv, hw, dtype, use_graph=True):
        m = vcfg.model
        pc = H.VolPlanConfig()
        pc.dtype = H.LT_F32 if dtype == torch.float32 else H.LT_BF16
        pc.num_layers, pc.style_caffe, pc.num_joints = m.backbone.num_layers, 0, m.backbone.num_joints
        pc.B, pc.NV, pc.H, pc.W = nf, nv, hw, hw
        pc.volume_size, pc.cuboid_side, pc.volume_multiplier = m.volume_size, m.cuboid_side, m.volume_multiplier
        pc.volume_softmax, pc.aggregation, pc.transfer_cmu_to_human36m, pc.use_graph = int(bool(m.volume_softmax)), H.AGG[m.volume_aggregation_method], 0, int(use_graph)
        self.kind, self.ncub = m.kind, ncub
        keep = []
        arr = (H.NamedTensor * len(vsd))()
        for i, (key, val) in enumerate(vsd.items()):
            t = val.detach().float().contiguous()
            keep.append(t)
            arr[i].name, arr[i].data, arr[i].ndim = key.encode(), t.data_ptr(), max(1, t.dim())
            for j, n in enumerate(t.shape if t.dim() else (1,)):
                arr[i].shape[j] = n
        self.plan = C.c_void_p()
        H.check(H.lib().lt_plan_create_vol_multi(C.byref(pc), ncub, arr, len(vsd), C.byref(self.plan)), "lt_plan_create_vol_multi")
        del keep, arr
        self.pc = pc
        self.info = H.PlanInfo()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(self.info)), "lt_plan_info")

    def forward(self, images, inp, frame_of, kp3d, optional=True, stream="current"):
        pc, n = self.pc, self.ncub
        nf, nv, vs, nj = pc.B, pc.NV, pc.volume_size, pc.num_joints
        h, w = self.info.heatmap_h, self.info.heatmap_w
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        o = {"kp": nan(n, nj, 3), "vols": nan(n, nj, vs, vs, vs), "feats": nan(nf, nv, 32, h, w), "coords": nan(n, vs, vs, vs, 3)}
        K = np.ascontiguousarray(np.broadcast_to(inp["K"][None], (nf, nv, 3, 3)), dtype=np.float64)
        R = np.ascontiguousarray(np.broadcast_to(inp["R"][None], (nf, nv, 3, 3)), dtype=np.float64)
        t = np.ascontiguousarray(np.broadcast_to(inp["t"].reshape(nv, 3)[None], (nf, nv, 3)), dtype=np.float64)
        k3 = np.asarray(kp3d, dtype=np.float64)
        base = np.ascontiguousarray((k3[:, 11, :3] + k3[:, 12, :3]) / 2 if self.kind == "coco" else k3[:, 6, :3])
        fo = np.ascontiguousarray(frame_of, dtype=np.int32)
        dp = lambda x: x.ctypes.data_as(C.c_void_p)
        p = lambda name: o[name].data_ptr() if optional else None
        st = torch.cuda.current_stream().cuda_stream if stream == "current" else None
        rc = H.lib().lt_plan_forward_vol_multi(self.plan, images.data_ptr(), dp(K), dp(R), dp(t), dp(fo), dp(base), None, o["kp"].data_ptr(), p("vols"), p("feats"),
                                               p("coords"), None, st)
        if rc != 0:
            return rc
        torch.cuda.synchronize()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(self.info)), "lt_plan_info")
        return o

    def close(self):
        if self.plan:
            H.lib().lt_plan_destroy(self.plan)
            self.plan = None


@pytest.mark.parametrize("kind,prefix", [("mpii", ""), ("coco", "coco/")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_multi_plan_abi_equals_the_python_host_bit_for_bit(golden_dir, dtype, kind, prefix):
    g = np.load(os.path.join(golden_dir, "multi_cuboid_small.npz"))
    seeds = g[prefix + "seeds"]
    vcfg, vsd, inp, kp_in = multi_setup(kind, seeds)
    vol = _model(18, V, kind, dtype, True, seed=seeds[0])
    images = inp["images"].to(DEV).contiguous()
    fo = list(FRAME_OF)
    mask = np.array([[1, 0, 1, 1], [1, 1, 1, 1]], dtype=np.uint8)
    batch = {"cameras": cameras(inp, F), "pred_keypoints_3d": kp_in, "cuboid_frame": fo}
    kp, feats, vols, _, _, coords, _ = vol(images, None, batch)
    fo2 = [1, 0, 0, 0, 1]
    kp_b = vol(images, None, dict(batch, cuboid_frame=fo2))[0]
    vol.keypoint_stats = True
    kp_m, _, vols_m = vol(images, None, dict(batch, view_mask=mask))[:3]
    st_m = vol.last_keypoint_stats
    torch.cuda.synchronize()
    lib = H.lib()
    cp = MultiCPlan(vcfg, vsd, F, P, NV, HW, dtype)
    try:
        assert cp.info.heatmap_h == HW // 4 and cp.info.launches > 50 and cp.info.graph_captured == 0
        for rnd in range(2):          # the capturing forward and a replay
            o = cp.forward(images, inp, fo, kp_in)
            for name, ours, want in (("keypoints_3d", o["kp"], kp), ("volumes", o["vols"], vols), ("features", o["feats"], feats), ("coord_volumes", o["coords"], coords)):
                assert torch.isfinite(want).all(), name
                assert torch.equal(ours, want), "%s %s forward %d %s: max |d| %.3e" % (kind, dtype, rnd, name, float((ours - want).abs().max()))
        assert cp.info.graph_captured == 1
        # another assignment on the captured plan; the optional outputs may be NULL, and stream NULL runs on the plan's own stream
        o2 = cp.forward(images, inp, fo2, kp_in, optional=False, stream=None)
        assert torch.equal(o2["kp"], kp_b) and torch.isnan(o2["vols"]).all()
        # a bad index: LT_ERR_INVALID before any device call, the message names the entry
        assert cp.forward(images, inp, [0, 1, 2, 0, 1], kp_in) == -1 and "cuboid_frame[2] = 2" in lib.lt_last_error().decode()
        assert cp.forward(images, inp, [0, 1, 1, -1, 1], kp_in) == -1 and "cuboid_frame[3] = -1" in lib.lt_last_error().decode()
        # lt_plan_forward_vol refuses a multi plan
        one = torch.zeros(1, device=DEV)
        assert lib.lt_plan_forward_vol(cp.plan, one.data_ptr(), 1, 1, 1, 1, None, one.data_ptr(), None, None, None, None, None) == -1
        assert "lt_plan_forward_vol_multi" in lib.lt_last_error().decode()
        # lt_plan_set_view_mask comes before the first forward, as on every plan
        assert lib.lt_plan_set_view_mask(cp.plan, mask.ctypes.data_as(C.c_void_p)) == -1
    finally:
        cp.close()
    # a masked multi plan with the per-joint statistics
    cm = MultiCPlan(vcfg, vsd, F, P, NV, HW, dtype)
    try:
        H.check(lib.lt_plan_set_view_mask(cm.plan, mask.ctypes.data_as(C.c_void_p)), "lt_plan_set_view_mask")
        rec = torch.full((P, J, 8), float("nan"), device=DEV)
        idx = torch.full((P, J), -1, dtype=torch.int32, device=DEV)
        H.check(lib.lt_plan_set_keypoint_stats(cm.plan, rec.data_ptr(), idx.data_ptr()), "lt_plan_set_keypoint_stats")
        o = cm.forward(images, inp, fo, kp_in)
        assert torch.equal(o["kp"], kp_m) and torch.equal(o["vols"], vols_m)
        assert torch.equal(rec[..., 0], st_m.peak) and torch.equal(idx, st_m.peak_index) and torch.equal(rec[..., 1], st_m.mass)
    finally:
        cm.close()


def test_multi_forward_refuses_other_plans():
    from test_gpu_plan_abi import CPlan
    p = CPlan("small_max", torch.float32)
    try:
        one = torch.zeros(1, device=DEV)
        rc = H.lib().lt_plan_forward_vol_multi(p.plan, one.data_ptr(), 1, 1, 1, 1, 1, None, one.data_ptr(), None, None, None, None, None)
        assert rc == -1 and "lt_plan_forward_vol" in H.lib().lt_last_error().decode()
    finally:
        p.close()


# ---- 5. no host wait -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_second_multi_cuboid_forward_never_waits_for_the_gpu(monkeypatch, dtype):
    vol = _model(18, 32, "mpii", dtype, True)
    inp = synth.make_inputs(2, 4, 128, seed=13)
    images = inp["images"].to(DEV)
    batch = {"cameras": cameras(inp, 2), "pred_keypoints_3d": _joints(P, 6), "cuboid_frame": np.array(FRAME_OF)}
    first = vol(images, None, batch)          # warm-up: records and captures the plan (that synchronises, once per shape)
    torch.cuda.synchronize()

    def refuse(name, orig=None, only_cuda=False):
        def f(self, *a, **kw):
            if only_cuda and not self.is_cuda:
                return orig(self, *a, **kw)
            raise AssertionError("the multi-cuboid forward waited for the GPU: %s" % name)
        return f

    def no_device_sync(*a, **kw):
        raise AssertionError("the multi-cuboid forward waited for the GPU: torch.cuda.synchronize")
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", no_device_sync)
        mp.setattr(torch.cuda.Stream, "synchronize", refuse("Stream.synchronize"))
        mp.setattr(torch.cuda.Event, "synchronize", refuse("Event.synchronize"))
        for name in ("cpu", "numpy", "item", "tolist"):
            mp.setattr(torch.Tensor, name, refuse("Tensor." + name, getattr(torch.Tensor, name), only_cuda=True))
        second = vol(images, None, batch)          # fewer forwards than GEO_RING: the ring has not wrapped
    torch.cuda.synchronize()
    _assert_same(second, first, "second forward")
