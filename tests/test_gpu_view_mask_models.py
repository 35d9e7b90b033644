"""GPU (-m gpu): ``batch["view_mask"]`` through VolumetricTriangulationNet, AlgebraicTriangulationNet and CascadeTriangulationNet, and
lt_plan_set_view_mask through ctypes.

  5. the fp32 masked forward of the full batch against the REFERENCE run per sample on its valid views alone (tests/golden/view_mask_small.npz,
     tools/make_golden_view_mask.py) and its fp64 truth, gated as tests/test_gpu_cascade.py gates: err <= max(2 x the reference's own fp32 error, floor);
  6. an all-ones mask equals no mask, every returned tensor, fp32 and bf16, graph on and off;
  7. the images of masked views do not matter (zeros or NaN: the same joints, bit for bit);
  8. a new mask on a captured masked plan gives what a fresh model gives; unmasked forwards before and after are identical;
  9. the C ABI: lt_plan_set_view_mask + the forward equals the Python host bit for bit; its refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from oracle import truth as T
from test_gpu_cascade import FLOOR_2D, FLOOR_JOINTS, CascadeCPlan, _gate
from test_gpu_plan_abi_alg import AlgCPlan
from test_view_mask_cpu import cameras, vm_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, NV, HW, V, J = 3, 4, 128, 32, 17
CASES = ("vol_softmax", "vol_conf_norm", "alg", "cascade")


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "view_mask_small.npz"))


_SETUP = {}


def _setup(golden_dir):
    if "s" not in _SETUP:
        g = _fixture(golden_dir)
        _SETUP["s"] = (g,) + tuple(vm_setup(g["seeds"]))
    return _SETUP["s"]


def _net(case, cfgs, sds, dtype, graph):
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet, VolumetricTriangulationNet
    import copy

    def one(name):
        cls = AlgebraicTriangulationNet if name == "alg" else VolumetricTriangulationNet
        m = cls(copy.deepcopy(cfgs[name]), device=DEV)
        m.load_state_dict(sds[name], strict=True)
        m.eval()
        m.compute_dtype, m.use_graph = dtype, graph
        return m
    if case == "cascade":
        return CascadeTriangulationNet(one("alg"), one("vol_softmax")).eval()
    return one(case)


def _batch(inp, mask=None, nb=B):
    b = {"cameras": cameras(inp, nb), "pred_keypoints_3d": inp["pred_keypoints_3d"][:nb]}
    if mask is not None:
        b["view_mask"] = mask
    return b


def _flat(out):
    """Every returned tensor of a forward, named (the cascade returns (vol 7-tuple, alg 4-tuple))."""
    if len(out) == 2:
        return [("vol/" + n, t) for n, t in _flat(out[0])] + [("alg/" + n, t) for n, t in _flat(out[1])]
    names = ("keypoints_3d", "features", "volumes", "vol_confidences", "cuboids", "coord_volumes", "base_points") if len(out) == 7 else \
        ("keypoints_3d", "keypoints_2d", "heatmaps", "alg_confidences")
    return [(n, t) for n, t in zip(names, out) if torch.is_tensor(t)]


def _same(a, b, what):
    fa, fb = _flat(a), _flat(b)
    assert [n for n, _ in fa] == [n for n, _ in fb], what
    for (n, x), (_, y) in zip(fa, fb):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, n)
        assert torch.equal(x, y), "%s %s: max |d| %.3e" % (what, n, float((x.double() - y.double()).abs().max()))


def _joints(case, out):
    return out[0][0] if case == "cascade" else out[0]


# ---- 5. against the reference on the valid views ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_masked_fp32_forward_vs_reference_on_the_valid_views(golden_dir, case):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    masks = g["masks"]
    on = masks.astype(bool)
    net = _net(case, cfgs, sds, torch.float32, True)
    images = inp["images"].to(DEV)
    out = net(images, P.to(DEV), _batch(inp, masks))
    torch.cuda.synchronize()
    err = lambda name: float(g["ref32_err/" + name])
    tru = lambda name: g["truth/" + name]
    tag = "view_mask %s/" % case
    bad = []
    if case.startswith("vol"):
        bad.append(_gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(out[0].cpu().numpy(), tru(case + "/kp")), err(case + "/kp"), FLOOR_JOINTS))
        if case == "vol_conf_norm":
            conf = out[3].cpu().numpy()
            assert np.count_nonzero(conf[~on]) == 0          # masked entries are 0, the valid ones sum to 1 over the views
            assert np.allclose(conf.sum(axis=1), 1.0, atol=1e-5)
            record(tag + "vol_confidences of the valid views fp32 vs fp64 truth, recorded",
                   {"err_ours": T.max_rel(conf[on], tru("vol_conf_norm/conf")[on]), "ref32_err": err("vol_conf_norm/conf")})
    else:
        a = out[1] if case == "cascade" else out
        pre = "alg/"
        bad.append(_gate(tag + "alg keypoints_2d of the valid views fp32 (max rel, 1 px floor)", T.joints_rel(a[1].cpu().numpy()[on], tru(pre + "kp2")[on]), err(pre + "kp2"),
                         FLOOR_2D))
        bad.append(_gate(tag + "alg confidences of the valid views fp32", T.max_rel(a[3].cpu().numpy()[on], tru(pre + "conf")[on]), err(pre + "conf"), FLOOR_2D))
        assert np.count_nonzero(a[3].cpu().numpy()[~on]) == 0          # masked confidences are exactly 0
        if case == "alg":
            bad.append(_gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(a[0].cpu().numpy(), tru("alg/kp3")), err("alg/kp3"), FLOOR_JOINTS))
        else:
            v = out[0]
            bad.append(_gate(tag + "pelvis fp32 (max rel, 1 mm floor)", T.joints_rel(v[6].cpu().numpy(), tru("cascade/base_points")), err("cascade/base_points"), FLOOR_JOINTS))
            bad.append(_gate(tag + "joints fp32 (max rel, 1 mm floor)", T.joints_rel(v[0].cpu().numpy(), tru("cascade/kp")), err("cascade/kp"), FLOOR_JOINTS))
            record(tag + "alg keypoints_3d fp32 vs fp64 truth (max rel, 1 mm floor), recorded",
                   {"err_ours": T.joints_rel(a[0].cpu().numpy(), tru("cascade/alg_kp3")), "ref32_err": err("cascade/alg_kp3")})
    assert not [b for b in bad if b], [b for b in bad if b]
    # bf16: deviations recorded, not gated (no measured value exists yet)
    net16 = _net(case, cfgs, sds, torch.bfloat16, True)
    out16 = net16(images, P.to(DEV), _batch(inp, masks))
    torch.cuda.synchronize()
    kp16 = _joints(case, out16).cpu().numpy()
    key = {"vol_softmax": "vol_softmax/kp", "vol_conf_norm": "vol_conf_norm/kp", "alg": "alg/kp3", "cascade": "cascade/kp"}[case]
    record(tag + "bf16 joints deviation from the fp64 truth (max rel, 1 mm floor), recorded", T.joints_rel(kp16, tru(key)))
    assert np.isfinite(kp16).all()


# ---- 6. all-ones mask == no mask ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_all_ones_mask_equals_no_mask(golden_dir, case, dtype, graph):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    net = _net(case, cfgs, sds, dtype, graph)
    images, Pd = inp["images"].to(DEV), P.to(DEV)
    plain = net(images, Pd, _batch(inp))
    ones = net(images, Pd, _batch(inp, torch.ones(B, NV, dtype=torch.bool)))
    again = net(images, Pd, _batch(inp, np.ones((B, NV), dtype=np.uint8)))          # the masked plan's replay
    torch.cuda.synchronize()
    what = "%s %s %s" % (case, dtype, "graph" if graph else "eager")
    _same(ones, plain, what)
    _same(again, plain, what + " (replay)")
    vol = net.vol if case == "cascade" else net
    assert len(vol._plans) == 2 if case != "cascade" else (len(net.vol._plans) == 2 and len(net.alg._plans) == 2)          # its own plan, beside the unmasked one


# ---- 7. masked images do not matter -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ["vol_softmax", "cascade"])
def test_images_of_masked_views_do_not_matter(golden_dir, case, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    net = _net(case, cfgs, sds, dtype, True)
    mask = np.tile(np.array([[1, 0, 1, 1]], dtype=np.uint8), (B, 1))
    zeros, nans = inp["images"].clone(), inp["images"].clone()
    zeros[:, 1], nans[:, 1] = 0.0, float("nan")
    a = _joints(case, net(zeros.to(DEV), P.to(DEV), _batch(inp, mask)))
    b = _joints(case, net(nans.to(DEV), P.to(DEV), _batch(inp, mask)))
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b), "%s %s: the joints depend on a masked view's image" % (case, dtype)


# ---- 8. replay --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["vol_softmax", "alg", "cascade"])
def test_a_new_mask_on_a_captured_plan(golden_dir, case):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images, Pd = inp["images"].to(DEV), P.to(DEV)
    m1, m2 = g["masks"], np.array([[0, 1, 1, 0], [1, 1, 1, 1], [1, 1, 0, 1]], dtype=np.uint8)
    net = _net(case, cfgs, sds, torch.float32, True)
    before = net(images, Pd, _batch(inp))
    first = net(images, Pd, _batch(inp, m1))          # records and captures the masked plan
    second = net(images, Pd, _batch(inp, m2))         # replays it with another mask
    after = net(images, Pd, _batch(inp))
    torch.cuda.synchronize()
    fresh = _net(case, cfgs, sds, torch.float32, True)
    want2 = fresh(images, Pd, _batch(inp, m2))
    fresh1 = _net(case, cfgs, sds, torch.float32, True)
    want1 = fresh1(images, Pd, _batch(inp, m1))
    torch.cuda.synchronize()
    assert torch.equal(_joints(case, second), _joints(case, want2)) and torch.equal(_joints(case, first), _joints(case, want1))
    assert not torch.equal(_joints(case, second), _joints(case, first))
    _same(after, before, case + ": unmasked forwards around the masked ones")


# ---- 9. the C ABI ---------------------------------------------------------------------------------------------------------------------------------------
def _u8(mask):
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    return m, m.ctypes.data_as(C.c_void_p)


class VolCPlan:
    """lt_plan_create_vol / lt_plan_forward_vol through ctypes for a given configuration and state dict."""

    def __init__(self, cfg, sd, dtype):
        m = cfg.model
        pc = H.VolPlanConfig()
        pc.dtype = H.LT_F32 if dtype == torch.float32 else H.LT_BF16
        pc.num_layers, pc.style_caffe, pc.num_joints = m.backbone.num_layers, 0, J
        pc.B, pc.NV, pc.H, pc.W = B, NV, HW, HW
        pc.volume_size, pc.cuboid_side, pc.volume_multiplier = m.volume_size, m.cuboid_side, m.volume_multiplier
        pc.volume_softmax, pc.aggregation, pc.transfer_cmu_to_human36m, pc.use_graph = int(bool(m.volume_softmax)), H.AGG[m.volume_aggregation_method], 0, 1
        keep, arr = [], (H.NamedTensor * len(sd))()
        for i, (k, v) in enumerate(sd.items()):
            t = v.detach().float().contiguous()
            keep.append(t)
            arr[i].name, arr[i].data, arr[i].ndim = k.encode(), t.data_ptr(), max(1, t.dim())
            for j, n in enumerate(t.shape if t.dim() else (1,)):
                arr[i].shape[j] = n
        self.plan = C.c_void_p()
        H.check(H.lib().lt_plan_create_vol(C.byref(pc), arr, len(sd), C.byref(self.plan)), "lt_plan_create_vol")
        del keep, arr

    def forward(self, images, inp):
        K = np.ascontiguousarray(np.broadcast_to(inp["K"][None], (B, NV, 3, 3)), dtype=np.float64)
        R = np.ascontiguousarray(np.broadcast_to(inp["R"][None], (B, NV, 3, 3)), dtype=np.float64)
        t = np.ascontiguousarray(np.broadcast_to(inp["t"].reshape(NV, 3)[None], (B, NV, 3)), dtype=np.float64)
        base = np.ascontiguousarray(np.asarray(inp["pred_keypoints_3d"], dtype=np.float64)[:, 6, :3])
        kp, vols = torch.full((B, J, 3), float("nan"), device=DEV), torch.empty(B, J, V, V, V, device=DEV)
        dp = lambda a: a.ctypes.data_as(C.c_void_p)
        H.check(H.lib().lt_plan_forward_vol(self.plan, images.data_ptr(), dp(K), dp(R), dp(t), dp(base), None, kp.data_ptr(), vols.data_ptr(), None, None, None,
                                            torch.cuda.current_stream().cuda_stream), "lt_plan_forward_vol")
        torch.cuda.synchronize()
        return kp, vols

    def close(self):
        if self.plan:
            H.lib().lt_plan_destroy(self.plan)
            self.plan = None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_vol_plan_with_a_mask_equals_the_python_host(golden_dir, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images = inp["images"].to(DEV).contiguous()
    lib = H.lib()
    for case in ("vol_softmax", "vol_conf_norm"):
        net = _net(case, cfgs, sds, dtype, True)
        m2 = np.array([[0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 1]], dtype=np.uint8)
        want1, want2 = net(images, None, _batch(inp, g["masks"])), net(images, None, _batch(inp, m2))
        cp = VolCPlan(cfgs[case], sds[case], dtype)
        try:
            keep, ptr = _u8(g["masks"])
            H.check(lib.lt_plan_set_view_mask(cp.plan, ptr), "lt_plan_set_view_mask")
            for rnd in range(2):          # the capturing forward and a replay: the mask persists
                kp, vols = cp.forward(images, inp)
                assert torch.equal(kp, want1[0]) and torch.equal(vols, want1[2]), (case, dtype, rnd, float((kp - want1[0]).abs().max()))
            keep2, ptr2 = _u8(m2)
            H.check(lib.lt_plan_set_view_mask(cp.plan, ptr2), "lt_plan_set_view_mask")
            kp, vols = cp.forward(images, inp)
            assert torch.equal(kp, want2[0]) and torch.equal(vols, want2[2]), (case, dtype, "second mask")
            # a sample without a valid view is refused, the message names it; the plan keeps its mask
            bad, pbad = _u8(np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]]))
            assert lib.lt_plan_set_view_mask(cp.plan, pbad) == -1 and "sample 1 has 0 valid views" in lib.lt_last_error().decode()
            assert torch.equal(cp.forward(images, inp)[0], want2[0])
            H.check(lib.lt_plan_set_view_mask(cp.plan, None), "lt_plan_set_view_mask")          # NULL: all valid
            plain = net(images, None, _batch(inp))
            assert torch.equal(cp.forward(images, inp)[0], plain[0])
        finally:
            cp.close()


def test_c_abi_first_mask_after_a_forward_is_refused(golden_dir):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images = inp["images"].to(DEV).contiguous()
    cp = VolCPlan(cfgs["vol_softmax"], sds["vol_softmax"], torch.float32)
    try:
        cp.forward(images, inp)
        keep, ptr = _u8(g["masks"])
        assert H.lib().lt_plan_set_view_mask(cp.plan, ptr) == -1 and "before the plan's first forward" in H.lib().lt_last_error().decode()
    finally:
        cp.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_alg_plan_with_a_mask_equals_the_python_host(golden_dir, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images = inp["images"].to(DEV).contiguous()
    net = _net("alg", cfgs, sds, dtype, True)
    want = net(images, P.to(DEV), _batch(inp, g["masks"]))
    on = torch.from_numpy(g["masks"].astype(bool)).to(DEV)
    lib = H.lib()
    cp = AlgCPlan(H.LT_MODEL_ALG, cfgs["alg"], sds["alg"], B, NV, HW, dtype)
    try:
        bad, pbad = _u8(np.array([[1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 1, 0]]))
        assert lib.lt_plan_set_view_mask(cp.plan, pbad) == -1 and "sample 2 has 1 valid view," in lib.lt_last_error().decode()
        keep, ptr = _u8(g["masks"])
        H.check(lib.lt_plan_set_view_mask(cp.plan, ptr), "lt_plan_set_view_mask")
        for rnd in range(2):
            o = cp.forward(images, P)
            assert torch.equal(o["kp3d"], want[0]) and torch.equal(o["conf"], want[3]) and torch.equal(o["kp2d"][on], want[1][on]), (dtype, rnd)
            assert torch.count_nonzero(o["conf"][~on]) == 0
    finally:
        cp.close()
    rp = AlgCPlan(H.LT_MODEL_RANSAC, cfgs["alg"], sds["alg"], B, NV, HW, torch.float32)
    try:
        keep, ptr = _u8(g["masks"])
        assert lib.lt_plan_set_view_mask(rp.plan, ptr) == -2 and "RANSAC" in lib.lt_last_error().decode()
    finally:
        rp.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_cascade_plan_with_a_mask_equals_the_python_host(golden_dir, dtype):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    images = inp["images"].to(DEV).contiguous()
    net = _net("cascade", cfgs, sds, dtype, True)
    (kp, feats, vols, _, _, coords, base), (a3, _, _, _) = net(images, P.to(DEV), _batch(inp, g["masks"]))
    torch.cuda.synchronize()
    cp = CascadeCPlan(cfgs["alg"], sds["alg"], cfgs["vol_softmax"], sds["vol_softmax"], B, NV, HW, dtype)
    try:
        bad, pbad = _u8(np.array([[1, 1, 1, 1], [0, 1, 0, 0], [1, 1, 1, 1]]))
        assert H.lib().lt_plan_set_view_mask(cp.plan, pbad) == -1 and "sample 1 has 1 valid view," in H.lib().lt_last_error().decode()
        keep, ptr = _u8(g["masks"])
        H.check(H.lib().lt_plan_set_view_mask(cp.plan, ptr), "lt_plan_set_view_mask")
        for rnd in range(2):
            o = cp.forward(images, inp["K"], inp["R"], inp["t"])
            for name, ours, want in (("keypoints_3d", o["kp"], kp), ("alg_keypoints_3d", o["alg_kp3"], a3), ("base_points", o["base"], base), ("volumes", o["vols"], vols),
                                     ("coord_volumes", o["coords"], coords)):
                assert torch.equal(ours, want), "%s forward %d %s: max |d| %.3e" % (dtype, rnd, name, float((ours - want).abs().max()))
    finally:
        cp.close()
