"""GPU (-m gpu): the cascade -- AlgebraicTriangulationNet's pelvis -> VolumetricTriangulationNet's cuboid on the device (lt_cuboid_from_keypoints,
CascadeTriangulationNet, lt_plan_create_cascade / lt_plan_forward_cascade).

  1. the seam kernel against its numpy statement (mvn.utils.volumetric.cuboid_from_keypoints), bit for bit;
  2. the cascade against the two-call route it replaces (run ``alg``, copy its joints to the host, run ``vol`` with them as ``pred_keypoints_3d``): the
     yardstick is the behaviour of the two existing models, and every output is ``torch.equal``;
  3. against the REFERENCE's two-stage route (tests/golden/cascade_small.npz, tools/make_golden_cascade.py) and its fp64 truth, at the gates of
     tests/test_gpu_truth.py: err <= max(2 x the reference's own fp32 error, floor);
  4. a second forward never waits for the GPU;
  5. the C ABI through ctypes alone, bit-identical to the Python host."""
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
from test_cascade_cpu import B, HW, J, NV, V, cameras, cascade_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR_2D, FLOOR_JOINTS = 1e-5, 1e-4          # tests/test_gpu_truth.py: FLOOR["kp2"] = FLOOR["conf"], FLOOR["kp"]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mpii", "coco"])
@pytest.mark.parametrize("nb", [1, 5, 64])
def test_cuboid_kernel_equals_numpy_bit_for_bit(kind, nb):
    from mvn.utils import volumetric
    rs = np.random.RandomState(7 * nb + (kind == "coco"))
    nj = 17 if nb != 5 else (13 if kind == "coco" else 7)          # the smallest J of the kind too
    kp = (rs.randn(nb, nj, 3) * 10.0 ** rs.randint(-1, 6, size=(nb, nj, 1))).astype(np.float32)
    kp[0, 6] = [1.0e5, -1.0e5, 99999.9921875]
    if nj > 12:
        kp[0, 11], kp[0, 12] = [16777216.0, -3.0, 1.0e5], [1.0, -2.5e-7, -99999.9921875]
    side = 2500.0 if nb != 5 else 1234.567
    d = torch.from_numpy(kp).to(DEV)
    out = torch.full((2, nb + 1, 3), float("nan"), device=DEV)          # one guard row behind each output
    H.check(H.lib().lt_cuboid_from_keypoints(d.data_ptr(), nb, nj, H.KIND[kind], side, out[0].data_ptr(), out[1].data_ptr(), torch.cuda.current_stream().cuda_stream),
            "lt_cuboid_from_keypoints")
    torch.cuda.synchronize()
    pos, center = volumetric.cuboid_from_keypoints(kp, kind, side)
    o = out.cpu().numpy()
    assert o[0, :nb].tobytes() == pos.tobytes(), np.abs(o[0, :nb] - pos).max()
    assert o[1, :nb].tobytes() == center.tobytes(), np.abs(o[1, :nb] - center).max()
    assert np.isnan(o[:, nb]).all()


# ---- the models ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _state_dicts(nl, alg_seed, vol_seed):
    return (synth.make_state_dict(spec.alg_net_spec(nl, J, True), seed=alg_seed, basic_block=(nl < 50)),
            synth.make_state_dict(spec.vol_net_spec(nl, J, False), seed=vol_seed, basic_block=(nl < 50)))


def _models(nl, vol_size, kind, dtype, graph, seeds=(61, 62)):
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet, VolumetricTriangulationNet
    acfg = synth.alg_config(nl, True, J)
    acfg.model.heatmap_multiplier = 1.0          # the seam is ill posed at 100 with synthetic weights (tools/make_golden_cascade.py)
    vcfg = synth.vol_config(nl, vol_size, "softmax", 1.0, kind)
    asd, vsd = _state_dicts(nl, int(seeds[0]), int(seeds[1]))
    alg = AlgebraicTriangulationNet(acfg, device=DEV)
    alg.load_state_dict(asd, strict=True)
    vol = VolumetricTriangulationNet(vcfg, device=DEV)
    vol.load_state_dict(vsd, strict=True)
    for m in (alg, vol):
        m.eval()
        m.compute_dtype = dtype
        m.use_graph = graph
    return alg, vol, CascadeTriangulationNet(alg, vol).eval()


def _inputs(nb, nv, hw, seed):
    inp = synth.make_inputs(nb, nv, hw, seed=seed)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(nb, 1, 1, 1)
    return inp, inp["images"].to(DEV), P.to(DEV)


def _two_call_route(alg, vol, images, P, cams):
    """What a user does today: the algebraic model, its joints to the host (a device synchronisation), the volumetric model on them."""
    a = alg(images, P, {"cameras": cams})
    pred = a[0].cpu().numpy()
    v = vol(images, None, {"cameras": cams, "pred_keypoints_3d": pred})
    return v, a


def _assert_same(casc, two, what):
    (cv, ca), (tv, ta) = casc, two
    assert len(cv) == 7 and len(ca) == 4
    names_v = ("keypoints_3d", "features", "volumes", "vol_confidences", "cuboids", "coord_volumes", "base_points")
    names_a = ("alg keypoints_3d", "alg keypoints_2d", "alg heatmaps", "alg confidences")
    for name, x, y in list(zip(names_v, cv, tv)) + list(zip(names_a, ca, ta)):
        if name == "cuboids":
            assert len(x) == len(y)
            for cx, cy in zip(x, y):
                assert np.array_equal(np.asarray(cx.position), np.asarray(cy.position)) and np.asarray(cx.position).dtype == np.asarray(cy.position).dtype, (what, name)
                assert np.array_equal(np.asarray(cx.sides), np.asarray(cy.sides)), (what, name)
            assert np.array_equal(np.asarray(x[0].position), np.asarray(y[0].position))          # indexable as the list is
            continue
        if y is None:
            assert x is None, (what, name)
            continue
        assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert torch.isfinite(y).all(), (what, name, "the two-call route's own output is not finite")
        assert torch.equal(x, y), "%s %s: max |d| %.3e" % (what, name, float((x.double() - y.double()).abs().max()))


# ---- 2. bit identity with the two-call route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mpii", "coco"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ["small", "c2"])
def test_cascade_equals_the_two_call_route_bit_for_bit(shape, dtype, graph, kind):
    nl, hw, vs, nv = (18, 128, 32, 4) if shape == "small" else (152, 384, 64, 4)          # c2: BASELINE config 2's networks and shape
    alg, vol, casc = _models(nl, vs, kind, dtype, graph)
    inp, images, P = _inputs(2, nv, hw, seed=13)
    cams = cameras(inp, 2)
    what = "%s %s %s %s" % (shape, dtype, "graph" if graph else "eager", kind)
    two = _two_call_route(alg, vol, images, P, cams)
    # pred_keypoints_3d / keypoints_3d in the batch are ignored: poison them
    casc_out = casc(images, P, {"cameras": cams, "pred_keypoints_3d": np.full((2, J, 3), np.nan), "keypoints_3d": np.full((2, J, 3), np.nan)})
    torch.cuda.synchronize()
    _assert_same(casc_out, two, what)
    # the pelvis the cuboid is centred on IS the algebraic stage's
    a3 = casc_out[1][0]
    want = (a3[:, 11] + a3[:, 12]) / 2 if kind == "coco" else a3[:, 6]
    assert torch.equal(casc_out[0][6], want)
    # again (a replay of both plans), and with only `cameras` in the batch
    again = casc(images, P, {"cameras": cams})
    torch.cuda.synchronize()
    _assert_same(again, two, what + " (second call)")


def test_cascade_sub_batches_equal_the_two_call_route():
    alg, vol, casc = _models(18, 32, "mpii", torch.float32, True)
    vol.max_samples_per_launch = lambda *a: 1          # the walk VolumetricTriangulationNet.forward does above its per-launch limit
    inp, images, P = _inputs(3, 4, 128, seed=14)
    cams = cameras(inp, 3)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        two = _two_call_route(alg, vol, images, P, cams)
    out = casc(images, P, {"cameras": cams})
    torch.cuda.synchronize()
    _assert_same(out, two, "sub-batches")


def test_cascade_refuses_training_mode():
    alg, vol, casc = _models(18, 32, "mpii", torch.float32, True)
    inp, images, P = _inputs(1, 2, 128, seed=3)
    casc.train()
    with pytest.raises(NotImplementedError):
        casc(images, P, {"cameras": cameras(inp, 1)})


# ---- 3. against the reference's two-stage route and its fp64 truth -----------------------------------------------------------------------------------------
def _gate(name, ours, ref32, floor):
    eff = max(2.0 * ref32, floor)
    record(name + " vs fp64 truth", {"err_ours": ours, "ref32_err": ref32, "ratio": ours / max(ref32, 1e-300), "gate": eff})
    print("%s: err %.3e, reference's own %.3e, gate %.3e" % (name, ours, ref32, eff))
    return None if ours <= eff else "%s: err %.3e > max(2 x reference's %.3e, floor %.1e)" % (name, ours, ref32, floor)


@pytest.mark.parametrize("kind,prefix", [("mpii", ""), ("coco", "coco/")])
def test_cascade_fp32_vs_reference_route_and_truth(golden_dir, kind, prefix):
    g = np.load(os.path.join(golden_dir, "cascade_small.npz"))
    k = lambda name: g[prefix + name]
    seeds = k("seeds")
    alg, vol, casc = _models(18, V, kind, torch.float32, True, seeds=(seeds[0], seeds[1]))
    inp, images, P = _inputs(B, NV, HW, seed=int(seeds[2]))
    assert np.allclose(synth.state_dict_checksum({n: t.cpu() for n, t in alg.state_dict().items()}), k("alg_sd_digest"), rtol=1e-12)
    assert np.allclose(T.images_digest(inp["images"]), k("images_digest"), rtol=1e-12)
    (kp, feats, vols, conf, cuboids, coords, base), (a3, a2, ahm, aconf) = casc(images, P, {"cameras": cameras(inp, B)})
    torch.cuda.synchronize()
    err = lambda name: float(k("ref32_err/" + name))
    tag = "cascade %s/" % kind
    bad = [_gate(tag + "alg keypoints_2d fp32 (max rel, 1 px floor)", T.joints_rel(a2.cpu().numpy(), k("truth/alg_kp2")), err("alg_kp2"), FLOOR_2D),
           _gate(tag + "alg confidences fp32", T.max_rel(aconf.cpu().numpy(), k("truth/alg_conf")), err("alg_conf"), FLOOR_2D),
           _gate(tag + "pelvis fp32 (max rel, 1 mm floor)", T.joints_rel(base.cpu().numpy(), k("truth/base_points")), err("base_points"), FLOOR_JOINTS),
           _gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(kp.cpu().numpy(), k("truth/kp")), err("kp"), FLOOR_JOINTS)]
    s = int(k("stride"))
    dp = float(np.abs(base.cpu().numpy().astype(np.float64) - k("base_points")).max())
    dcv = float(np.abs(coords.cpu().numpy()[:, ::s, ::s, ::s].astype(np.float64) - k("cv_sub")).max())
    lim = 1e-7 * float(np.abs(k("cv_sub")).max()) + dp
    record(tag + "coord_volumes vs the reference's: max |d| mm", {"err_ours": dcv, "gate": lim, "pelvis_difference_mm": dp})
    print("%scoord_volumes: max |d| %.3e mm, gate %.3e (pelvis difference %.3e mm)" % (tag, dcv, lim, dp))
    if dcv > lim:
        bad.append("%scoord_volumes: max |d| %.3e mm > 1e-7 x max|ref| + the pelvis difference = %.3e" % (tag, dcv, lim))
    record(tag + "alg keypoints_3d fp32 vs fp64 truth (max rel, 1 mm floor), recorded", {"err_ours": T.joints_rel(a3.cpu().numpy(), k("truth/alg_kp3")), "ref32_err": err("alg_kp3")})
    assert np.array_equal(np.stack([c.position for c in cuboids]), base.cpu().numpy().astype(np.float64) - float(vol.cuboid_side) / 2)
    assert not [b for b in bad if b], [b for b in bad if b]
    # bf16: deviations recorded, not gated (no measured value exists yet)
    alg.compute_dtype = vol.compute_dtype = torch.bfloat16
    (kp16, _, _, _, _, _, base16), (a316, a216, _, aconf16) = casc(images, P, {"cameras": cameras(inp, B)})
    torch.cuda.synchronize()
    record(tag + "bf16 deviation from the fp64 truth",
           {"alg keypoints_2d (max rel, 1 px floor)": T.joints_rel(a216.cpu().numpy(), k("truth/alg_kp2")),
            "alg confidences": T.max_rel(aconf16.cpu().numpy(), k("truth/alg_conf")),
            "pelvis (max rel, 1 mm floor)": T.joints_rel(base16.cpu().numpy(), k("truth/base_points")),
            "joints (max rel, 1 mm floor)": T.joints_rel(kp16.cpu().numpy(), k("truth/kp"))})
    assert torch.isfinite(kp16).all()


# ---- 4. no host wait -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_second_cascade_forward_never_waits_for_the_gpu(monkeypatch, dtype):
    alg, vol, casc = _models(18, 32, "mpii", dtype, True)
    inp, images, P = _inputs(2, 4, 128, seed=13)
    batch = {"cameras": cameras(inp, 2)}
    first = casc(images, P, batch)          # warm-up: records and captures both plans (that synchronises, once per shape)
    torch.cuda.synchronize()

    def refuse(name, orig=None, only_cuda=False):
        def f(self, *a, **kw):
            if only_cuda and not self.is_cuda:
                return orig(self, *a, **kw)
            raise AssertionError("the cascade forward waited for the GPU: %s" % name)
        return f

    def no_device_sync(*a, **kw):
        raise AssertionError("the cascade forward waited for the GPU: torch.cuda.synchronize")
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", no_device_sync)
        mp.setattr(torch.cuda.Stream, "synchronize", refuse("Stream.synchronize"))
        mp.setattr(torch.cuda.Event, "synchronize", refuse("Event.synchronize"))
        for name in ("cpu", "numpy", "item", "tolist"):
            mp.setattr(torch.Tensor, name, refuse("Tensor." + name, getattr(torch.Tensor, name), only_cuda=True))
        second = casc(images, P, batch)          # fewer forwards than GEO_RING: the ring has not wrapped
    torch.cuda.synchronize()
    _assert_same(second, first, "second forward")


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------------------------------
class CascadeCPlan:
    """lt_plan_create_cascade / lt_plan_forward_cascade through ctypes: what a host in any language does."""

    def __init__(self, acfg, asd, vcfg, vsd, nb, nv, hw, dtype, use_graph=True):
        pc = H.CascadePlanConfig()
        code = H.LT_F32 if dtype == torch.float32 else H.LT_BF16
        a, v, am, vm = pc.alg, pc.vol, acfg.model, vcfg.model
        a.model, a.dtype, a.num_layers, a.style_caffe, a.num_joints = H.LT_MODEL_ALG, code, am.backbone.num_layers, 0, am.backbone.num_joints
        a.B, a.NV, a.H, a.W = nb, nv, hw, hw
        a.use_confidences, a.heatmap_softmax, a.heatmap_multiplier, a.use_graph = int(bool(am.use_confidences)), int(bool(am.heatmap_softmax)), float(am.heatmap_multiplier), int(use_graph)
        v.dtype, v.num_layers, v.style_caffe, v.num_joints = code, vm.backbone.num_layers, 0, vm.backbone.num_joints
        v.B, v.NV, v.H, v.W = nb, nv, hw, hw
        v.volume_size, v.cuboid_side, v.volume_multiplier = vm.volume_size, vm.cuboid_side, vm.volume_multiplier
        v.volume_softmax, v.aggregation, v.transfer_cmu_to_human36m, v.use_graph = int(bool(vm.volume_softmax)), H.AGG[vm.volume_aggregation_method], 0, int(use_graph)
        pc.kind = H.KIND[vm.kind]
        keep = []

        def named(sd):
            arr = (H.NamedTensor * len(sd))()
            for i, (key, val) in enumerate(sd.items()):
                t = val.detach().float().contiguous()
                keep.append(t)
                arr[i].name, arr[i].data, arr[i].ndim = key.encode(), t.data_ptr(), max(1, t.dim())
                for j, n in enumerate(t.shape if t.dim() else (1,)):
                    arr[i].shape[j] = n
            return arr
        aw, vw = named(asd), named(vsd)
        self.plan = C.c_void_p()
        H.check(H.lib().lt_plan_create_cascade(C.byref(pc), aw, len(asd), vw, len(vsd), C.byref(self.plan)), "lt_plan_create_cascade")
        del keep, aw, vw
        self.pc = pc
        self.info = H.PlanInfo()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(self.info)), "lt_plan_info")

    def forward(self, images, K, R, t, optional=True, stream="current"):
        a, v = self.pc.alg, self.pc.vol
        nb, nv, vs, nj = v.B, v.NV, v.volume_size, v.num_joints
        h, w = self.info.heatmap_h, self.info.heatmap_w
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        o = {"kp": nan(nb, nj, 3), "alg_kp3": nan(nb, a.num_joints, 3), "base": nan(nb, 3), "vols": nan(nb, nj, vs, vs, vs), "feats": nan(nb, nv, 32, h, w),
             "coords": nan(nb, vs, vs, vs, 3)}
        K = np.ascontiguousarray(np.broadcast_to(K[None], (nb, nv, 3, 3)), dtype=np.float64)
        R = np.ascontiguousarray(np.broadcast_to(R[None], (nb, nv, 3, 3)), dtype=np.float64)
        t = np.ascontiguousarray(np.broadcast_to(t.reshape(nv, 3)[None], (nb, nv, 3)), dtype=np.float64)
        dp = lambda x: x.ctypes.data_as(C.c_void_p)
        p = lambda name: o[name].data_ptr() if optional else None
        st = torch.cuda.current_stream().cuda_stream if stream == "current" else None
        H.check(H.lib().lt_plan_forward_cascade(self.plan, images.data_ptr(), dp(K), dp(R), dp(t), None, o["kp"].data_ptr(), p("alg_kp3"), p("base"), p("vols"), p("feats"),
                                                p("coords"), None, st), "lt_plan_forward_cascade")
        torch.cuda.synchronize()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(self.info)), "lt_plan_info")
        return o

    def close(self):
        if self.plan:
            H.lib().lt_plan_destroy(self.plan)
            self.plan = None


@pytest.mark.parametrize("kind,prefix", [("mpii", ""), ("coco", "coco/")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cascade_plan_abi_equals_the_python_host_bit_for_bit(golden_dir, dtype, kind, prefix):
    g = np.load(os.path.join(golden_dir, "cascade_small.npz"))
    seeds = g[prefix + "seeds"]
    acfg, asd, vcfg, vsd, inp, P = cascade_setup(kind, seeds)
    alg, vol, casc = _models(18, V, kind, dtype, True, seeds=(seeds[0], seeds[1]))
    images = inp["images"].to(DEV).contiguous()
    (kp, feats, vols, _, _, coords, base), (a3, _, _, _) = casc(images, P.to(DEV), {"cameras": cameras(inp, B)})
    torch.cuda.synchronize()
    cp = CascadeCPlan(acfg, asd, vcfg, vsd, B, NV, HW, dtype)
    try:
        lib = H.lib()
        info0 = cp.info
        assert info0.heatmap_h == HW // 4 and info0.heatmap_w == HW // 4 and info0.launches > 50 and info0.flops > 0 and info0.graph_captured == 0
        for rnd in range(2):          # the capturing forward and a replay
            o = cp.forward(images, inp["K"], inp["R"], inp["t"])
            for name, ours, want in (("keypoints_3d", o["kp"], kp), ("alg_keypoints_3d", o["alg_kp3"], a3), ("base_points", o["base"], base), ("volumes", o["vols"], vols),
                                     ("features", o["feats"], feats), ("coord_volumes", o["coords"], coords)):
                assert torch.isfinite(want).all(), name
                assert torch.equal(ours, want), "%s %s forward %d %s: max |d| %.3e" % (kind, dtype, rnd, name, float((ours - want).abs().max()))
        assert cp.info.graph_captured == 1
        # the optional outputs may be NULL, and stream NULL runs on the plan's own stream
        o2 = cp.forward(images, inp["K"], inp["R"], inp["t"], optional=False, stream=None)
        assert torch.equal(o2["kp"], kp) and torch.isnan(o2["base"]).all()
        # other cameras: the result moves (the graph holds no stale geometry)
        K2, R2, t2 = synth.ring_cameras(NV, HW, radius=3500.0, height=1400.0)
        o3 = cp.forward(images, K2, R2, t2)
        assert torch.isfinite(o3["kp"]).all() and not torch.equal(o3["kp"], kp) and not torch.equal(o3["alg_kp3"], a3)
        want = (o3["alg_kp3"][:, 11] + o3["alg_kp3"][:, 12]) / 2 if kind == "coco" else o3["alg_kp3"][:, 6]
        assert torch.equal(o3["base"], want)
        # the single-stage forwards refuse a cascade plan, and the cascade forward a single-stage plan's arguments stay unread
        one = torch.zeros(1, device=DEV)
        assert lib.lt_plan_forward_vol(cp.plan, one.data_ptr(), 1, 1, 1, 1, None, one.data_ptr(), None, None, None, None, None) == -1
        assert "cascade" in lib.lt_last_error().decode() and "lt_plan_forward_cascade" in lib.lt_last_error().decode()
        assert lib.lt_plan_forward_alg(cp.plan, one.data_ptr(), one.data_ptr(), one.data_ptr(), None, None, None, None) == -1
        assert "cascade" in lib.lt_last_error().decode()
    finally:
        cp.close()


def test_cascade_forward_refuses_single_stage_plans():
    from test_gpu_plan_abi import CPlan
    p = CPlan("small_max", torch.float32)
    try:
        one = torch.zeros(1, device=DEV)
        rc = H.lib().lt_plan_forward_cascade(p.plan, one.data_ptr(), 1, 1, 1, None, one.data_ptr(), None, None, None, None, None, None, None)
        assert rc == -1 and "lt_plan_forward_vol" in H.lib().lt_last_error().decode()
    finally:
        p.close()
