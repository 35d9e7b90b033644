"""CPU: the cascade (algebraic pelvis -> volumetric cuboid on the device) without a GPU.

  * ``mvn.utils.volumetric.cuboid_from_keypoints`` -- the CPU statement of lt_cuboid_from_keypoints -- equals, bit for bit, what
    ``VolumetricTriangulationNet._host_geometry`` writes into the pos / center ranges of a plan's geometry block;
  * the new symbols are exported with the declared signatures and every configuration error is LT_ERR_INVALID before any device call, with a
    message that names the field;
  * tests/golden/cascade_small.npz (tools/make_golden_cascade.py: the REFERENCE's two-stage route) was made from the weights and images ``synth``
    makes today, and the oracle's two stages chained in fp32 reproduce its reference outputs at the tolerances tests/test_oracle_golden.py uses for
    the single stages."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import spec, synth
from oracle import vol_oracle as O

ERR_INVALID = -1          # LT_ERR_INVALID
NL, J, B, NV, HW, V = 18, 17, 2, 4, 128, 32          # tools/make_golden_cascade.py


def cascade_setup(kind, seeds):
    """tools/make_golden_cascade.py:setup -- (alg config, alg state dict, vol config, vol state dict, inputs, fp32 image-resolution projections)."""
    alg_seed, vol_seed, input_seed = (int(s) for s in seeds)
    acfg = synth.alg_config(NL, True, J)
    acfg.model.heatmap_multiplier = 1.0
    vcfg = synth.vol_config(NL, V, "softmax", 1.0, kind)
    asd = synth.make_state_dict(spec.alg_net_spec(NL, J, True), seed=alg_seed, basic_block=True)
    vsd = synth.make_state_dict(spec.vol_net_spec(NL, J, False), seed=vol_seed, basic_block=True)
    inp = synth.make_inputs(B, NV, HW, seed=input_seed)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(B, 1, 1, 1)
    return acfg, asd, vcfg, vsd, inp, P


def cameras(inp, nb):
    from mvn.utils.multiview import Camera
    return [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(nb)] for v in range(inp["K"].shape[0])]


# ---- 1. the numpy statement against the host route's geometry block ------------------------------------------------------------------------------
def _random_joints(nb, seed):
    """fp32 joints with small, large (1e5 mm), negative and exactly representable values, and pairs whose fp32 sum rounds."""
    rs = np.random.RandomState(seed)
    kp = (rs.randn(nb, J, 3) * 10.0 ** rs.randint(-1, 6, size=(nb, J, 1))).astype(np.float32)
    kp[0, 6] = [1.0e5, -1.0e5, 99999.9921875]
    kp[0, 11], kp[0, 12] = [16777216.0, -3.0, 1.0e5], [1.0, -2.5e-7, -99999.9921875]
    if nb > 1:
        kp[1, 6] = [-0.0, 1249.99993896484375, -1250.00006103515625]
        kp[1, 11], kp[1, 12] = [0.1, 0.2, 0.3], [0.7, 1e-3, -0.3]
    return kp


@pytest.mark.parametrize("kind", ["mpii", "coco"])
@pytest.mark.parametrize("nb,side", [(1, 2500.0), (5, 2500.0), (3, 1234.567)])
def test_cuboid_from_keypoints_equals_host_geometry_bit_for_bit(kind, nb, side):
    from lt_staging import PinnedRing
    from mvn.models.triangulation import VolumetricTriangulationNet
    from mvn.utils import volumetric
    cfg = synth.vol_config(18, 32, "softmax", kind=kind, cuboid_side=side)
    m = VolumetricTriangulationNet(cfg, device="cpu")
    m.eval()
    nv, h = 2, 16
    inp = synth.make_inputs(nb, nv, 64, seed=3)
    kp = _random_joints(nb, 17 * nb + (kind == "coco"))
    n_geo = nb * nv * 12 + nb * 15
    o_pos, o_cen, o_rot = nb * nv * 12, nb * nv * 12 + 3 * nb, nb * nv * 12 + 6 * nb
    def nan_ring():
        ring = PinnedRing(n_geo, torch.float32, 2, pin=False)
        for blk in ring.blocks:
            blk.fill_(float("nan"))
        return ring
    P = {"hw": (h, h), "offs": (o_pos, o_cen, o_rot), "geo_ring": nan_ring()}
    position, base, sides = m._host_geometry({"cameras": cameras(inp, nb), "pred_keypoints_3d": kp}, nb, (64, 64), P)
    gh = P["geo_host"].numpy()
    pos, center = volumetric.cuboid_from_keypoints(kp, kind, side)
    assert pos.dtype == np.float32 and center.dtype == np.float32 and pos.shape == (nb, 3) and center.shape == (nb, 3)
    assert pos.tobytes() == gh[o_pos:o_cen].tobytes()
    assert center.tobytes() == gh[o_cen:o_rot].tobytes()
    # and the camera half alone fills what the cuboid half does not
    P2 = dict(P, geo_ring=nan_ring())
    g2 = m._host_cameras({"cameras": cameras(inp, nb)}, nb, (64, 64), P2).numpy()
    assert np.isnan(g2[o_pos:o_rot]).all()
    assert g2[:o_pos].tobytes() == gh[:o_pos].tobytes() and g2[o_rot:].tobytes() == gh[o_rot:].tobytes()


def test_cuboid_from_keypoints_refuses_too_few_joints():
    from mvn.utils import volumetric
    with pytest.raises(ValueError):
        volumetric.cuboid_from_keypoints(np.zeros((1, 6, 3), np.float32), "mpii", 2500.0)
    with pytest.raises(ValueError):
        volumetric.cuboid_from_keypoints(np.zeros((1, 12, 3), np.float32), "coco", 2500.0)
    volumetric.cuboid_from_keypoints(np.zeros((1, 7, 3), np.float32), "mpii", 2500.0)


# ---- 2. the C ABI without a GPU -------------------------------------------------------------------------------------------------------------------
def test_cascade_symbols_are_exported_with_the_declared_signatures():
    lib = C.CDLL(H.LIB_PATH)
    for name in ("lt_cuboid_from_keypoints", "lt_plan_create_cascade", "lt_plan_forward_cascade"):
        assert hasattr(lib, name), name
        assert name in H.SIGNATURES, name
    vp, i32 = C.c_void_p, C.c_int32
    assert H.SIGNATURES["lt_cuboid_from_keypoints"] == (C.c_int, [vp, i32, i32, i32, C.c_double, vp, vp, vp])
    res, args = H.SIGNATURES["lt_plan_create_cascade"]
    assert res is C.c_int and len(args) == 6 and args[0] is C.POINTER(H.CascadePlanConfig)
    assert H.SIGNATURES["lt_plan_forward_cascade"] == (C.c_int, [vp] * 14)
    assert [f[0] for f in H.CascadePlanConfig._fields_] == ["alg", "vol", "kind"]
    assert H.CascadePlanConfig.alg.size == C.sizeof(H.AlgPlanConfig) and H.CascadePlanConfig.vol.size == C.sizeof(H.VolPlanConfig)
    assert (H.LT_KIND_MPII, H.LT_KIND_COCO) == (0, 1) and H.KIND == {"mpii": 0, "coco": 1}
    assert H.lib().lt_abi_version() == 1


def test_cuboid_kernel_argument_checks():
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    assert lib.lt_cuboid_from_keypoints(None, 1, 17, 0, 2500.0, 1, 1, None) == ERR_INVALID and "null" in err()
    assert lib.lt_cuboid_from_keypoints(1, 1, 17, 0, 2500.0, None, 1, None) == ERR_INVALID and "null" in err()
    assert lib.lt_cuboid_from_keypoints(1, 1, 17, 0, 2500.0, 1, None, None) == ERR_INVALID and "null" in err()
    assert lib.lt_cuboid_from_keypoints(1, 0, 17, 0, 2500.0, 1, 1, None) == ERR_INVALID and "B 0" in err()
    assert lib.lt_cuboid_from_keypoints(1, 1, 6, H.LT_KIND_MPII, 2500.0, 1, 1, None) == ERR_INVALID and "J 6" in err()
    assert lib.lt_cuboid_from_keypoints(1, 1, 12, H.LT_KIND_COCO, 2500.0, 1, 1, None) == ERR_INVALID and "J 12" in err()
    assert lib.lt_cuboid_from_keypoints(1, 1, 17, 2, 2500.0, 1, 1, None) == ERR_INVALID and "kind 2" in err()


def _cfg(**kw):
    c = H.CascadePlanConfig()
    a, v = c.alg, c.vol
    a.model, a.dtype, a.num_layers, a.style_caffe, a.num_joints = H.LT_MODEL_ALG, H.LT_F32, 18, 0, 17
    a.B, a.NV, a.H, a.W = 2, 4, 128, 128
    a.use_confidences, a.heatmap_softmax, a.heatmap_multiplier, a.use_graph = 1, 1, 1.0, 1
    v.dtype, v.num_layers, v.style_caffe, v.num_joints = H.LT_F32, 18, 0, 17
    v.B, v.NV, v.H, v.W = 2, 4, 128, 128
    v.volume_size, v.cuboid_side, v.volume_multiplier, v.volume_softmax, v.aggregation, v.use_graph = 32, 2500.0, 1.0, 1, H.AGG["softmax"], 1
    c.kind = H.LT_KIND_MPII
    for k, val in kw.items():
        obj, _, field = k.rpartition("__")
        setattr(getattr(c, obj) if obj else c, field, val)
    return c


def _weights(names=("backbone.conv1.weight",)):
    arr = (H.NamedTensor * len(names))()
    keep = (C.c_float * 1)()
    for i, n in enumerate(names):
        arr[i].name, arr[i].data, arr[i].ndim, arr[i].shape[0] = n.encode(), C.cast(keep, C.c_void_p), 1, 1
    return arr, keep


def _create(cfg, alg_names=("backbone.conv1.weight",)):
    aw, k1 = _weights(alg_names)
    vw, k2 = _weights()
    plan = C.c_void_p()
    rc = H.lib().lt_plan_create_cascade(C.byref(cfg), aw, len(alg_names), vw, 1, C.byref(plan))
    assert not plan.value
    return rc, H.lib().lt_last_error().decode()


def test_cascade_plan_null_arguments():
    lib = H.lib()
    aw, k1 = _weights()
    plan = C.c_void_p()
    cfg = _cfg()
    for args in ((None, aw, 1, aw, 1, C.byref(plan)), (C.byref(cfg), None, 1, aw, 1, C.byref(plan)), (C.byref(cfg), aw, 1, None, 1, C.byref(plan)),
                 (C.byref(cfg), aw, 0, aw, 1, C.byref(plan)), (C.byref(cfg), aw, 1, aw, 0, C.byref(plan)), (C.byref(cfg), aw, 1, aw, 1, None)):
        assert lib.lt_plan_create_cascade(*args) == ERR_INVALID and "null" in lib.lt_last_error().decode()
    assert lib.lt_plan_forward_cascade(None, 1, 1, 1, 1, None, 1, None, None, None, None, None, None, None) == ERR_INVALID and "null" in lib.lt_last_error().decode()


@pytest.mark.parametrize("field,value,needle", [
    ("alg__model", H.LT_MODEL_RANSAC, "alg.model 2"), ("alg__model", 0, "model 0"),
    ("vol__B", 3, "vol.B 3"), ("vol__NV", 2, "vol.NV 2"), ("vol__H", 256, "vol.H 256"), ("vol__W", 64, "vol.W 64"),
    ("kind", 2, "kind 2"), ("kind", -1, "kind -1"),
    ("alg__num_joints", 6, "alg.num_joints 6"),
    ("alg__dtype", 7, "dtype 7"), ("vol__dtype", H.LT_FP8, "dtype 2"), ("vol__aggregation", 9, "aggregation 9"), ("alg__NV", 1, "NV 1"),
])
def test_cascade_plan_config_validation(field, value, needle):
    rc, msg = _create(_cfg(**{field: value}))
    assert rc == ERR_INVALID and needle in msg and "lt_plan_create_cascade" in msg, (rc, msg)


def test_cascade_plan_coco_needs_thirteen_joints():
    rc, msg = _create(_cfg(kind=H.LT_KIND_COCO, alg__num_joints=12))
    assert rc == ERR_INVALID and "alg.num_joints 12" in msg and "coco" in msg, msg


def test_cascade_plan_names_the_missing_head_key():
    rc, msg = _create(_cfg())
    assert rc == ERR_INVALID and "backbone.final_layer.weight" in msg and "lt_plan_create_cascade" in msg, msg
    rc, msg = _create(_cfg(), ("backbone.final_layer.weight", "backbone.final_layer.bias"))
    assert rc == ERR_INVALID and "backbone.alg_confidences.head.4.weight" in msg, msg


def test_cascade_module_is_inference_only_and_keeps_both_state_dicts():
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet, VolumetricTriangulationNet
    alg = AlgebraicTriangulationNet(synth.alg_config(18, True), device="cpu")
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu")
    m = CascadeTriangulationNet(alg, vol)
    assert m.alg is alg and m.vol is vol
    keys = list(m.state_dict().keys())
    assert keys == ["alg." + k for k in alg.state_dict()] + ["vol." + k for k in vol.state_dict()]
    with pytest.raises(TypeError):
        CascadeTriangulationNet(vol, alg)
    with pytest.raises(ValueError):
        CascadeTriangulationNet(AlgebraicTriangulationNet(synth.alg_config(18, True, num_joints=12), device="cpu"),
                                VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax", kind="coco"), device="cpu"))
    with pytest.raises(RuntimeError):          # no CPU path
        m.eval()(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 3, 4), {})


# ---- 3. the fixture ---------------------------------------------------------------------------------------------------------------------------------
def _close(a, b, tol, what=""):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    e = float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))
    assert e <= tol, "%s: max|d|/max|ref| = %.3e > %.1e" % (what, e, tol)


def _sub(t, s):
    sl = (slice(None), slice(None)) + tuple(slice(None, None, s) for _ in range(t.dim() - 2))
    return t[sl]


@pytest.mark.parametrize("kind,prefix", [("mpii", ""), ("coco", "coco/")])
def test_cascade_fixture_matches_synth_and_the_chained_oracle(golden_dir, kind, prefix):
    path = os.path.join(golden_dir, "cascade_small.npz")
    assert os.path.getsize(path) < (1 << 20)
    g = np.load(path)
    k = lambda name: g[prefix + name]
    acfg, asd, vcfg, vsd, inp, P = cascade_setup(kind, k("seeds"))
    assert np.allclose(synth.state_dict_checksum(asd), k("alg_sd_digest"), rtol=1e-12), "weight generator drift"
    assert np.allclose(synth.state_dict_checksum(vsd), k("vol_sd_digest"), rtol=1e-12), "weight generator drift"
    assert np.allclose([float(inp["images"].double().sum()), float((inp["images"].double() ** 2).sum())], k("images_digest"), rtol=1e-12)
    # what the generator asserted: the seam is well posed, the reference's own noise sits below a quarter of the 1e-4 joint gate
    side = float(vcfg.model.cuboid_side)
    assert np.linalg.norm(k("truth/base_points") - k("look_at"), axis=1).max() <= side / 4
    assert float(k("ref32_err/kp")) <= 0.25e-4
    assert np.array_equal(k("cuboid_pos"), k("base_points").astype(np.float64) - side / 2) and np.array_equal(k("cuboid_sides"), np.full((B, 3), side))
    # the oracle's two stages chained in fp32, the joints handed over as the fp32 array a results file holds
    a = O.algebraic_forward(asd, acfg, inp["images"], inp["K"], inp["R"], inp["t"])
    _close(a["keypoints_2d"], k("alg_kp2"), 1e-4, "alg keypoints_2d")
    _close(a["alg_confidences"], k("alg_conf"), 1e-4, "alg confidences")
    _close(a["keypoints_3d"], k("alg_kp3"), 1e-3, "alg keypoints_3d")
    # stage 2 on the REFERENCE's pelvis (the fixture's joints): isolates the stage, as the single-stage fixtures do
    o = O.volumetric_forward(vsd, vcfg, inp["images"], inp["K"], inp["R"], inp["t"], k("alg_kp3"))
    s = int(k("stride"))
    _close(o["base_points"], k("base_points"), 1e-7, "base_points")
    _close(o["coord_volumes"][:, ::s, ::s, ::s], k("cv_sub"), 1e-7, "coord_volumes")
    _close(_sub(o["features"].reshape(-1, *o["features"].shape[2:]), s), k("feat_sub"), 2e-5, "features")
    _close(_sub(o["volumes"], s), k("vol_sub"), 1e-3, "volumes")
    rel = np.abs(o["keypoints_3d"].numpy() - k("kp")) / np.maximum(np.abs(k("kp")), 1.0)
    assert rel.max() <= 1e-4, "joints: max rel %.3e" % rel.max()
    # and end to end: the oracle's own fp32 pelvis moves the cuboid by the two pelvises' difference, and the joints with it
    o2 = O.volumetric_forward(vsd, vcfg, inp["images"], inp["K"], inp["R"], inp["t"], a["keypoints_3d"].numpy())
    dp = float(np.abs(o2["base_points"].numpy() - k("base_points")).max())
    assert float(np.abs(o2["coord_volumes"][:, ::s, ::s, ::s].numpy() - k("cv_sub")).max()) <= 1e-7 * float(np.abs(k("cv_sub")).max()) + dp
    rel = np.abs(o2["keypoints_3d"].numpy() - k("kp")) / np.maximum(np.abs(k("kp")), 1.0)
    assert rel.max() <= 1e-4, "chained joints: max rel %.3e (pelvis difference %.3e mm)" % (rel.max(), dp)
