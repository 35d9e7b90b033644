"""GPU (-m gpu): the plan-level C ABI of the algebraic and RANSAC models (include/lt_hip.h: lt_plan_create_alg / lt_plan_forward_alg) and the algebraic tail
kernel (lt_alg_tail_fwd), driven through ctypes: the state dict goes in as names + host fp32 arrays, images and projection matrices as device pointers, and torch
owns device memory only.

Gates: against the reference's golden outputs at the gates tests/test_gpu_models.py and tests/test_gpu_ransac.py hold the Python models to; against the Python
host (AlgebraicTriangulationNet, RANSACTriangulationNet, VolumetricTriangulationNet) bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import check, record, rel_err
from oracle import spec, synth
from test_gpu_plan_abi import CPlan
from test_oracle_golden import build_vol_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sub(t, s):
    sl = (slice(None), slice(None)) + tuple(slice(None, None, s) for _ in range(t.dim() - 2))
    return t[sl]


def _proj(inp, B):          # K [R | t] at image resolution, (B, NV, 3, 4) fp32: the reference's proj_matricies_batch
    return torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(B, 1, 1, 1)


# tag -> the model, its configuration, state dict and inputs (those of tests/test_gpu_models.py and tests/test_gpu_ransac.py)
def _case(tag):
    if tag == "alg_c1":
        cfg = synth.alg_config(50, True)
        sd = synth.make_state_dict(spec.alg_net_spec(50, 17, True), seed=50)
        inp = synth.make_inputs(2, 4, 256, seed=1)
        return H.LT_MODEL_ALG, cfg, sd, inp, _proj(inp, 2)
    if tag == "alg_relu_noconf":
        cfg = synth.alg_config(18, False)
        cfg.model.heatmap_softmax = False
        cfg.model.heatmap_multiplier = 1.0
        cfg.model["heatmap_softmax"] = False
        cfg.model["heatmap_multiplier"] = 1.0
        sd = synth.make_state_dict(spec.alg_net_spec(18, 17, False), seed=51, basic_block=True)
        inp = synth.make_inputs(2, 3, 128, seed=9)
        return H.LT_MODEL_ALG, cfg, sd, inp, _proj(inp, 2)
    assert tag == "ransac_net"
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "experiments_human36m.json")) as f:
        y = json.load(f)["eval/human36m_ransac.yaml"]
    cfg = synth.AttrDict({"model": y["model"]})
    cfg.model.backbone.update({"name": "resnet18", "num_layers": 18, "init_weights": False, "checkpoint": ""})
    cfg.model.direct_optimization = True
    sd = synth.make_state_dict(spec.alg_net_spec(18, 17, False), seed=61, basic_block=True)
    inp = synth.make_inputs(2, 4, 128, seed=13)
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ransac_net.npz"))
    return H.LT_MODEL_RANSAC, cfg, sd, inp, torch.from_numpy(g["P"]).float()


class AlgCPlan:
    """lt_plan_create_alg / lt_plan_forward_alg through ctypes: what a host in any language does."""

    def __init__(self, model, cfg, sd, B, NV, Hh, dtype, use_graph=True):
        m = cfg.model
        pc = H.AlgPlanConfig()
        pc.model, pc.dtype = model, H.LT_F32 if dtype == torch.float32 else H.LT_BF16
        pc.num_layers, pc.style_caffe, pc.num_joints = m.backbone.num_layers, int(m.backbone.get("style", "simple") == "caffe"), m.backbone.num_joints
        pc.B, pc.NV, pc.H, pc.W = B, NV, Hh, Hh
        pc.use_confidences = int(bool(m.get("use_confidences", False))) if model == H.LT_MODEL_ALG else 0
        pc.heatmap_softmax, pc.heatmap_multiplier = int(bool(m.get("heatmap_softmax", True))), float(m.get("heatmap_multiplier", 1.0))
        pc.direct_optimization, pc.reprojection_error_epsilon = int(bool(m.get("direct_optimization", True))), 15.0
        pc.use_graph = int(use_graph)
        keep = []
        arr = (H.NamedTensor * len(sd))()
        for i, (k, v) in enumerate(sd.items()):
            t = v.detach().float().contiguous()
            keep.append(t)
            arr[i].name, arr[i].data, arr[i].ndim = k.encode(), t.data_ptr(), max(1, t.dim())
            for j, n in enumerate(t.shape if t.dim() else (1,)):
                arr[i].shape[j] = n
        self.plan = C.c_void_p()
        H.check(H.lib().lt_plan_create_alg(C.byref(pc), arr, len(sd), C.byref(self.plan)), "lt_plan_create_alg")
        del keep, arr
        self.pc, self.model = pc, model
        self.info = H.PlanInfo()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(self.info)), "lt_plan_info")

    def forward(self, images, proj, stream="current"):
        pc = self.pc
        B, NV, J, h, w = pc.B, pc.NV, pc.num_joints, self.info.heatmap_h, self.info.heatmap_w
        ransac = self.model == H.LT_MODEL_RANSAC
        o = {"kp3d": torch.full((B, J, 3), float("nan"), device=DEV),
             "kp2d": torch.full((B, NV, J, 2), -7, dtype=torch.int64, device=DEV) if ransac else torch.full((B, NV, J, 2), float("nan"), device=DEV),
             "hm": torch.full((B, NV, J, h, w), float("nan"), device=DEV), "conf": torch.full((B, NV, J), float("nan"), device=DEV)}
        images = images.to(DEV).contiguous()
        proj = proj.to(DEV, torch.float32).contiguous()
        st = torch.cuda.current_stream().cuda_stream if stream == "current" else None
        H.check(H.lib().lt_plan_forward_alg(self.plan, images.data_ptr(), proj.data_ptr(), o["kp3d"].data_ptr(), o["kp2d"].data_ptr(), o["hm"].data_ptr(),
                                            o["conf"].data_ptr(), st), "lt_plan_forward_alg")
        torch.cuda.synchronize()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(self.info)), "lt_plan_info")
        return o

    def close(self):
        if self.plan:
            H.lib().lt_plan_destroy(self.plan)
            self.plan = None


def _cplan(tag, dtype, use_graph=True):
    model, cfg, sd, inp, P = _case(tag)
    B, NV, _, Hh, _ = inp["images"].shape
    return AlgCPlan(model, cfg, sd, B, NV, Hh, dtype, use_graph), inp, P


def _python_model(tag, dtype):
    from mvn.models.triangulation import AlgebraicTriangulationNet, RANSACTriangulationNet
    model, cfg, sd, inp, P = _case(tag)
    m = (AlgebraicTriangulationNet if model == H.LT_MODEL_ALG else RANSACTriangulationNet)(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    m.compute_dtype = dtype
    return m, inp, P


# ---- 1. ALG plans against the reference's goldens ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["alg_c1", "alg_relu_noconf"])
def test_alg_plan_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "%s.npz" % tag))
    P, inp, proj = _cplan(tag, torch.float32)
    try:
        o = P.forward(inp["images"], proj)
        B, NV, J, h, w = o["hm"].shape
        s = 4 if tag == "alg_c1" else 2
        check("plan-alg %s/keypoints_2d" % tag, o["kp2d"].cpu(), g["kp2"], 1e-4)
        check("plan-alg %s/confidences" % tag, o["conf"].cpu(), g["conf"], 1e-4 if tag == "alg_c1" else 1e-6)
        check("plan-alg %s/heatmaps" % tag, _sub(o["hm"].cpu().reshape(B * NV, J, h, w), s), g["hm_sub"], 2e-3)
        # random weights: the views' 2D keypoints disagree, the DLT systems are ill conditioned (tests/test_gpu_models.py) -- recorded, not gated
        record("plan-alg %s/keypoints_3d end-to-end deviation (ill-conditioned)" % tag, rel_err(o["kp3d"].cpu(), g["kp3"]))
        assert torch.isfinite(o["kp3d"]).all()
        i = P.info
        assert i.n_pwchain == 0 and i.n_conv_skip == 0 and not i.logits and i.n_stem_pool == 0          # no V2V; fp32 plans record no bf16-only fusion
    finally:
        P.close()


# ---- 2. the tail kernel on the well-conditioned rendered heatmaps ----------------------------------------------------------------------------------------------
def test_alg_tail_kernel_on_rendered_heatmaps_vs_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "pipe2d.npz"))
    hm = torch.from_numpy(g["hm"]).float().to(DEV).contiguous()
    B, NV, J, h, w = hm.shape
    lib, st = H.lib(), torch.cuda.current_stream().cuda_stream
    kp_hm = torch.empty(B * NV, J, 2, device=DEV)
    H.check(lib.lt_softargmax2d_fwd(hm.data_ptr(), 100.0, 1, kp_hm.data_ptr(), None, B * NV * J, h, w, st), "lt_softargmax2d_fwd")
    conf_raw = torch.from_numpy(g["conf"]).float().to(DEV).contiguous()
    proj = torch.from_numpy(g["P"]).float().to(DEV).contiguous()
    kp2d, conf, kp3d = torch.empty(B, NV, J, 2, device=DEV), torch.empty(B, NV, J, device=DEV), torch.empty(B, J, 3, device=DEV)
    H.check(lib.lt_alg_tail_fwd(kp_hm.data_ptr(), conf_raw.data_ptr(), J, proj.data_ptr(), 256 / w, 256 / h, kp2d.data_ptr(), conf.data_ptr(), kp3d.data_ptr(),
                                B, NV, J, st), "lt_alg_tail_fwd")
    torch.cuda.synchronize()
    check("tail pipe2d/keypoints_2d (image px)", kp2d.cpu(), g["kp2d"], 1e-5)
    rel = np.abs(kp3d.cpu().numpy() - g["kp3d"]) / np.maximum(np.abs(g["kp3d"]), 1.0)
    record("tail pipe2d/keypoints_3d end to end: max rel (1 mm floor)", float(rel.max()))
    assert rel.max() <= 1e-3, rel.max()


# ---- 3. the tail kernel against the Python host's torch glue, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("NV", [2, 3, 4, 8])
@pytest.mark.parametrize("with_conf", [True, False])
def test_alg_tail_kernel_equals_the_torch_glue_bit_for_bit(NV, with_conf):
    from mvn.utils import multiview
    B, J, Hh, W, h, w = 3, 17, 257, 300, 64, 72
    gen = torch.Generator().manual_seed(100 * NV + with_conf)
    kp_hm = (torch.rand(B * NV, J, 2, generator=gen) * torch.tensor([w - 1.0, h - 1.0])).to(DEV).contiguous()
    ld = J + 3          # a padded row stride of the raw confidences
    raw_pad = torch.rand(B * NV, ld, generator=gen).mul(0.98).add(0.01).to(DEV).contiguous()
    K, R, t = synth.ring_cameras(NV, 256)
    proj = torch.from_numpy(K @ np.concatenate([R, t], -1)).float()[None].repeat(B, 1, 1, 1).to(DEV).contiguous()
    # the glue AlgebraicTriangulationNet ran before lt_alg_tail_fwd (reference :173-193)
    conf = raw_pad[:, :J].contiguous().reshape(B, NV, J) if with_conf else torch.ones(B, NV, J, dtype=torch.float32, device=DEV)
    conf = conf / conf.sum(dim=1, keepdim=True) + 1e-5
    scale = torch.tensor([W / w, Hh / h], dtype=torch.float32, device=DEV)
    kp2d = kp_hm.reshape(B, NV, J, 2) * scale
    kp3d = multiview.triangulate_batch_of_points(proj, kp2d, confidences_batch=conf)
    k2, cf, k3 = torch.empty_like(kp2d), torch.empty_like(conf), torch.empty_like(kp3d)
    H.check(H.lib().lt_alg_tail_fwd(kp_hm.data_ptr(), raw_pad.data_ptr() if with_conf else None, ld, proj.data_ptr(), W / w, Hh / h, k2.data_ptr(), cf.data_ptr(),
                                    k3.data_ptr(), B, NV, J, torch.cuda.current_stream().cuda_stream), "lt_alg_tail_fwd")
    torch.cuda.synchronize()
    for name, a, b in (("keypoints_2d", k2, kp2d), ("confidences", cf, conf), ("keypoints_3d", k3, kp3d)):
        assert torch.equal(a, b), "NV %d conf %s %s: max |d| %.3e" % (NV, with_conf, name, float((a - b).abs().max()))
    # the optional outputs may be NULL
    k3b = torch.empty_like(kp3d)
    H.check(H.lib().lt_alg_tail_fwd(kp_hm.data_ptr(), raw_pad.data_ptr() if with_conf else None, ld, proj.data_ptr(), W / w, Hh / h, None, None, k3b.data_ptr(),
                                    B, NV, J, torch.cuda.current_stream().cuda_stream), "lt_alg_tail_fwd")
    torch.cuda.synchronize()
    assert torch.equal(k3b, kp3d)


# ---- 4. the RANSAC plan against the reference's golden ------------------------------------------------------------------------------------------------------
def test_ransac_plan_vs_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "ransac_net.npz"))
    P, inp, proj = _cplan("ransac_net", torch.float32)
    try:
        o = P.forward(inp["images"], proj)
        kp3, kp2, hm, conf = o["kp3d"], o["kp2d"], o["hm"], o["conf"]
        assert kp3.dtype == torch.float32 and kp3.shape == (2, 17, 3)
        assert kp2.dtype == torch.int64 and kp2.shape == (2, 4, 17, 2)
        assert hm.dtype == torch.float32 and hm.shape == (2, 4, 17, 32, 32)
        assert conf.dtype == torch.float32 and conf.shape == (2, 4, 17) and not conf.any()
        tol = 2e-3
        check("plan-ransac/raw heatmaps", hm.cpu().reshape(8, 17, 32, 32)[:, :, ::2, ::2], g["hm_sub"], tol)
        sure = g["margin"] > 2 * tol * float(g["hm_absmax"])          # an argmax can only move where the reference's top-2 gap is within twice the tolerance
        record("plan-ransac/keypoints_2d entries excluded (top-2 margin <= 2 tol max|hm|)", int((~sure).sum()))
        k2 = kp2.cpu().numpy()
        assert np.array_equal(k2[sure], g["kp2"][sure]), np.argwhere((k2 != g["kp2"]).any(-1) & sure)
        record("plan-ransac/keypoints_3d end-to-end deviation (random init: views disagree)", rel_err(kp3.cpu(), g["kp3"]))
        assert torch.isfinite(kp3).all()
    finally:
        P.close()


# ---- 5. bit for bit against the Python host ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["alg_c1", "alg_relu_noconf", "ransac_net"])
def test_alg_plan_equals_the_python_hosts_model_bit_for_bit(tag, dtype):
    P, inp, proj = _cplan(tag, dtype)
    try:
        o = P.forward(inp["images"], proj)
        m, _, _ = _python_model(tag, dtype)
        with torch.no_grad():
            kp3, kp2, hm, conf = m(inp["images"].to(DEV), proj.to(DEV), {})
        torch.cuda.synchronize()
        for name, a, b in (("keypoints_3d", o["kp3d"], kp3), ("keypoints_2d", o["kp2d"], kp2), ("heatmaps", o["hm"], hm), ("confidences", o["conf"], conf)):
            assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
            assert torch.equal(a, b), "%s %s: C plan != Python model (max |d| %.3e)" % (tag, name, float((a.double() - b.double()).abs().max()))
        # the same launches: the C plan adds its image layout pass in fp32 (the Python host launches it outside its plan) and its tail kernel
        # (ALG: lt_alg_tail_fwd; RANSAC: lt_triangulate_ransac, which the Python host launches after its plan)
        npy = len(list(m._plans.values())[0]["plan"].ops)
        record("plan-alg %s %s: launches of the C plan | of the Python plan" % (tag, "fp32" if dtype == torch.float32 else "bf16"), [P.info.launches, npy])
        assert P.info.launches == npy + (1 if dtype == torch.float32 else 0) + 1
    finally:
        P.close()


# ---- 6. graph against eager, replay against the first call, the plan's own stream ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["alg_relu_noconf", "ransac_net"])
def test_alg_plan_graph_equals_eager(tag):
    Pg, inp, proj = _cplan(tag, torch.float32, use_graph=True)
    Pe, _, _ = _cplan(tag, torch.float32, use_graph=False)
    try:
        a = Pg.forward(inp["images"], proj)
        assert Pg.info.graph_captured == 1
        b = Pg.forward(inp["images"], proj)          # replays the captured graph
        c = Pg.forward(inp["images"], proj, stream=None)          # stream NULL: the plan's own stream, ordered by events
        e = Pe.forward(inp["images"], proj)
        e2 = Pe.forward(inp["images"], proj)
        assert Pe.info.graph_captured == 0
        for k in a:
            for other in (b, c, e, e2):
                assert torch.equal(a[k], other[k]), (tag, k)
    finally:
        Pg.close()
        Pe.close()


# ---- 7. the two-stage Human3.6M pipeline from C ------------------------------------------------------------------------------------------------------------
def _vol_forward(P, base):
    """lt_plan_forward_vol of a CPlan (tests/test_gpu_plan_abi.py) with the caller's base points (B, 3) fp64."""
    inp, pc, lib = P.inp, P.pc, H.lib()
    B, NV, V, J = pc.B, pc.NV, pc.volume_size, pc.num_joints
    K = np.ascontiguousarray(np.broadcast_to(inp["K"][None], (B, NV, 3, 3)), dtype=np.float64)
    R = np.ascontiguousarray(np.broadcast_to(inp["R"][None], (B, NV, 3, 3)), dtype=np.float64)
    t = np.ascontiguousarray(np.broadcast_to(inp["t"].reshape(NV, 3)[None], (B, NV, 3)), dtype=np.float64)
    base = np.ascontiguousarray(base, dtype=np.float64)
    images = inp["images"].to(DEV).contiguous()
    kp, vols = torch.empty(B, J, 3, device=DEV), torch.empty(B, J, V, V, V, device=DEV)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    H.check(lib.lt_plan_forward_vol(P.plan, images.data_ptr(), dp(K), dp(R), dp(t), dp(base), None, kp.data_ptr(), vols.data_ptr(), None, None, None,
                                    torch.cuda.current_stream().cuda_stream), "lt_plan_forward_vol")
    torch.cuda.synchronize()
    return kp, vols


@pytest.mark.parametrize("tag,dtype", [("small_softmax", torch.float32), ("c2_b4", torch.bfloat16)])
def test_two_stage_pipeline_from_c_equals_the_python_models(tag, dtype):
    from mvn.models.triangulation import AlgebraicTriangulationNet, VolumetricTriangulationNet
    from mvn.utils.multiview import Camera
    cfg, sd, inp, c = build_vol_case(tag)
    assert c["kind"] == "mpii"
    nl, B, NV, Hh = c["nl"], c["B"], c["NV"], c["H"]
    acfg = synth.alg_config(nl, True)
    asd = synth.make_state_dict(spec.alg_net_spec(nl, 17, True), seed=300 + nl, basic_block=nl < 50)
    proj = _proj(inp, B)
    A = AlgCPlan(H.LT_MODEL_ALG, acfg, asd, B, NV, Hh, dtype)
    Vp = CPlan(tag, dtype)
    try:
        # C: algebraic plan -> pelvis (joint 6, kind 'mpii') -> volumetric plan
        kp_alg = A.forward(inp["images"], proj)["kp3d"]
        assert torch.isfinite(kp_alg).all()
        kp, vols = _vol_forward(Vp, kp_alg[:, 6].double().cpu().numpy())
        # Python: the same two stages, the second reading batch["pred_keypoints_3d"]
        am = AlgebraicTriangulationNet(acfg, device=DEV)
        am.load_state_dict(asd, strict=True)
        am.eval()
        am.compute_dtype = dtype
        vm = VolumetricTriangulationNet(cfg, device=DEV)
        vm.load_state_dict(sd, strict=True)
        vm.eval()
        vm.compute_dtype = dtype
        with torch.no_grad():
            kp3_py = am(inp["images"].to(DEV), proj.to(DEV), {})[0]
            cams = [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(B)] for v in range(NV)]
            kp_py, _, vols_py = vm(inp["images"].to(DEV), None, {"cameras": cams, "pred_keypoints_3d": kp3_py.cpu().numpy()})[:3]
        torch.cuda.synchronize()
        assert torch.equal(kp_alg, kp3_py), "%s: stage 1 (max |d| %.3e)" % (tag, float((kp_alg - kp3_py).abs().max()))
        assert torch.equal(kp, kp_py), "%s: stage 2 joints (max |d| %.3e)" % (tag, float((kp - kp_py).abs().max()))
        assert torch.equal(vols, vols_py), "%s: stage 2 volumes" % tag
        record("plan-alg two-stage %s: pelvis from the algebraic plan (mm) | joints" % tag, [kp_alg[:, 6].cpu().tolist(), float(kp.abs().max())])
    finally:
        A.close()
        Vp.close()


# ---- 8. wrong plan kind -------------------------------------------------------------------------------------------------------------------------------
def test_wrong_plan_kind_is_refused():
    lib = H.lib()
    P, inp, proj = _cplan("alg_relu_noconf", torch.float32)
    Vp = CPlan("small_max", torch.float32)
    try:
        x = torch.zeros(1, device=DEV)
        h = np.zeros(64)
        dp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = lib.lt_plan_forward_vol(P.plan, x.data_ptr(), dp(h), dp(h), dp(h), dp(h), None, x.data_ptr(), None, None, None, None, None)
        assert rc == -1 and b"lt_plan_forward_alg" in lib.lt_last_error(), (rc, lib.lt_last_error())
        rc = lib.lt_plan_forward_alg(Vp.plan, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, None, None)
        assert rc == -1 and b"lt_plan_forward_vol" in lib.lt_last_error(), (rc, lib.lt_last_error())
        torch.cuda.synchronize()
        o = P.forward(inp["images"], proj)          # the refused call left the plan usable
        assert torch.isfinite(o["kp3d"]).all()
    finally:
        P.close()
        Vp.close()
