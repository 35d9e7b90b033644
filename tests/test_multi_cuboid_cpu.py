"""CPU: several cuboids per frame (``batch["cuboid_frame"]``, lt_unproject_indexed_fwd, lt_plan_create_vol_multi) without a GPU.

  * a dry-run plan for F = 2 frames and P = 5 cuboids records the backbone at F * NV images and the gather, V2V and the tail at P, its geometry block
    is ``proj F*NV*12 | pos P*3 | center P*3 | rot P*9 | frame_of P int32 | [mask F*NV bytes]``, and the same call without cuboids records what it did;
  * the hosts refuse a bad assignment before any launch, and what there is no kernel for (training, the cascade, a gradient);
  * the new symbols are exported with the declared signatures, the header still compiles as C, and every configuration error of the C multi plan is
    LT_ERR_INVALID before any device call;
  * tests/golden/multi_cuboid_small.npz (tools/make_golden_multi_cuboid.py: the REFERENCE on the frames repeated per cuboid) was made from the weights,
    images and joints this file rebuilds."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import spec, synth
from oracle import truth as T

ERR_INVALID = -1          # LT_ERR_INVALID
NL, J, NV, HW, V = 18, 17, 4, 128, 32          # tools/make_golden_multi_cuboid.py
F, FRAME_OF = 2, (0, 1, 1, 0, 1)
P = len(FRAME_OF)


def base_points(seed, side):
    """tools/make_golden_multi_cuboid.py:base_points"""
    rs = np.random.RandomState(seed + 101)
    d = rs.randn(P, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (side / 5) * rs.uniform(0.3, 1.0, size=(P, 1))


def keypoints_for(base, kind, seed):
    """tools/make_golden_multi_cuboid.py:keypoints_for"""
    rs = np.random.RandomState(seed + 202)
    kp = rs.randn(P, J, 3) * 100.0
    if kind == "coco":
        off = rs.randn(P, 3) * 50.0
        kp[:, 11], kp[:, 12] = base + off, base - off
    else:
        kp[:, 6] = base
    return kp


def multi_setup(kind, seeds):
    """tools/make_golden_multi_cuboid.py:setup -- (vol config, vol state dict, inputs of the F frames, (P, J, 3) joints)."""
    vol_seed, input_seed = (int(s) for s in seeds)
    vcfg = synth.vol_config(NL, V, "softmax", 1.0, kind)
    vsd = synth.make_state_dict(spec.vol_net_spec(NL, J, False), seed=vol_seed, basic_block=True)
    inp = synth.make_inputs(F, NV, HW, seed=input_seed)
    return vcfg, vsd, inp, keypoints_for(base_points(input_seed, float(vcfg.model.cuboid_side)), kind, input_seed)


def cameras(inp, nb):
    from mvn.utils.multiview import Camera
    return [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(nb)] for v in range(inp["K"].shape[0])]


def _vol(kind="mpii"):
    from mvn.models.triangulation import VolumetricTriangulationNet
    return VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax", 1.0, kind), device="cpu").eval()


def _launches(plan):
    return [(meta["kind"], meta["label"]) for _, meta in plan.ops]


def _batch_of(meta):
    """The leading (sample) dimension an op was recorded at: its convolution spec's N, or its output / volume tensor's."""
    info = meta.get("info") or {}
    if "spec" in info:
        return info["spec"].N
    for k in ("y", "vol", "kp"):
        if k in info and info[k] is not None:
            return info[k].shape[0]
    return None


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_dry_run_plan_records_the_backbone_per_frame_and_the_rest_per_cuboid(dt):
    vol = _vol()
    vol.compute_dtype = dt
    assert vol._plan_key(F, NV, 64, 64, "cpu") == vol._plan_key(F, NV, 64, 64, "cpu", False, False, None)          # a forward without the key keeps its plan
    assert vol._plan_key(F, NV, 64, 64, "cpu", cuboids=P) != vol._plan_key(F, NV, 64, 64, "cpu")
    assert vol._plan_key(F, NV, 64, 64, "cpu", cuboids=P) != vol._plan_key(F, NV, 64, 64, "cpu", cuboids=P + 1)
    assert vol._plan_key(F, NV, 64, 64, "cpu", cuboids=F) != vol._plan_key(F, NV, 64, 64, "cpu")          # P == F is still a multi plan
    plain = vol._build_plan(F, NV, 64, 64, "cpu", dry_run=True)
    before = _launches(plain["plan"])
    multi = vol._build_plan(F, NV, 64, 64, "cpu", dry_run=True, cuboids=P)
    again = vol._build_plan(F, NV, 64, 64, "cpu", dry_run=True)
    assert _launches(plain["plan"]) == before == _launches(again["plan"])          # the same call without cuboids: the launch list it yields today
    assert plain["cuboids"] is None and multi["cuboids"] == P and multi["frames"] == F
    ops, pops = multi["plan"].ops, plain["plan"].ops
    kinds = [m["kind"] for _, m in ops]
    u = kinds.index("unproject")
    assert [m["kind"] for _, m in pops].index("unproject") == u
    assert _launches(multi["plan"])[:u] == before[:u]          # the backbone and process_features: the plain plan's launches ...
    sized = [_batch_of(m) for _, m in ops[:u]]
    assert sized and all(n in (None, F * NV) for n in sized) and sized.count(F * NV) >= 10, sized          # ... at F * NV images
    info = ops[u][1]["info"]
    assert info["entry"] == "lt_unproject_grid_indexed_fwd" and pops[u][1]["info"]["entry"] == "lt_unproject_grid_fwd"
    assert (info["frames"], info["cuboids"]) == (F, P)
    assert tuple(info["feats"].shape[:1]) == (F * NV,) and tuple(info["vol"].shape) == (P, 32, 32, 32, 32) and tuple(info["coords"].shape) == (P, 32, 32, 32, 3)
    tail = [_batch_of(m) for _, m in ops[u + 1:] if m["kind"] not in ("features_out",)]
    assert tail and all(n in (None, P) for n in tail) and tail.count(P) >= 10, tail          # V2V and the soft-argmax at P
    sa = ops[-1][1]["info"]
    assert tuple(sa["kp"].shape) == (P, J, 3) and tuple(sa["probs"].shape) == (P, J, 32, 32, 32)
    fo = [m for _, m in ops if m["kind"] == "features_out"]
    assert len(fo) == 1 and tuple(fo[0]["info"]["feats"].shape[:1]) == (F * NV,)
    # the stats flavour composes: same launches, P rows
    st = vol._build_plan(F, NV, 64, 64, "cpu", dry_run=True, cuboids=P, stats=True)
    assert _launches(st["plan"]) == _launches(multi["plan"]) and tuple(st["kstats"].shape) == (P, J, 8) and tuple(st["kindex"].shape) == (P, J)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_geometry_block_layout(masked):
    """proj F*NV*12 | pos P*3 | center P*3 | rot P*9 | frame_of P int32 | [mask F*NV bytes]; the floats are those of the plain plans."""
    from mvn.utils import volumetric
    vol = _vol()
    nv = 3
    inp = synth.make_inputs(F, nv, 64, seed=4)
    rs = np.random.RandomState(5)
    kp = rs.randn(P, J, 3) * 100.0
    fo = np.array(FRAME_OF, dtype=np.int32)
    m = np.array([[1, 0, 1], [0, 1, 1]], dtype=np.uint8)
    batch = {"cameras": cameras(inp, F), "pred_keypoints_3d": kp, "cuboid_frame": fo}
    if masked:
        batch["view_mask"] = m
    multi = vol._build_plan(F, nv, 64, 64, "cpu", dry_run=True, cuboids=P, masked=masked)
    n_f = F * nv * 12 + P * 15 + P
    assert multi["geo"].numel() == n_f + ((F * nv + 3) // 4 if masked else 0)
    assert multi["offs"] == (F * nv * 12, F * nv * 12 + 3 * P, F * nv * 12 + 6 * P) and multi["o_fof"] == F * nv * 12 + 15 * P and multi["o_mask"] == n_f
    position, base, sides = vol._host_geometry(batch, F, (64, 64), multi)
    gh = multi["geo_host"]
    plain = vol._build_plan(F, nv, 64, 64, "cpu", dry_run=True)
    vol._host_geometry({"cameras": cameras(inp, F), "pred_keypoints_3d": kp[:F]}, F, (64, 64), plain)
    o_pos, o_cen, o_rot = multi["offs"]
    assert torch.equal(gh[:o_pos], plain["geo_host"][:F * nv * 12])          # the projections: per frame
    pos, center = volumetric.cuboid_from_keypoints(kp.astype(np.float32), "mpii", 2500.0)
    assert position.shape == (P, 3) and base.shape == (P, 3)
    assert gh[o_cen:o_rot].numpy().tobytes() == kp[:, 6].astype(np.float32).tobytes()
    assert gh[o_pos:o_cen].numpy().tobytes() == (kp[:, 6] - 1250.0).astype(np.float32).tobytes()
    assert torch.equal(gh[o_rot:o_rot + 9 * P].reshape(P, 9), torch.eye(3).reshape(1, 9).repeat(P, 1))
    assert gh.view(torch.int32)[multi["o_fof"]:multi["o_fof"] + P].tolist() == list(FRAME_OF)
    if masked:
        assert gh.view(torch.uint8)[4 * n_f:4 * n_f + F * nv].tolist() == m.reshape(-1).tolist()


# ---- 2. the hosts' refusals ----------------------------------------------------------------------------------------------------------------------------
def test_frame_index_host_checks():
    from mvn.utils import op
    a = op.frame_index_host([1, 0, 1], 2)
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] and a.tolist() == [1, 0, 1]
    assert op.frame_index_host(torch.tensor([0, 0]), 1).tolist() == [0, 0]
    assert op.frame_index_host(np.array([2, 0], dtype=np.uint8), 3).tolist() == [2, 0]
    for bad, needle in (([0, 2], r"\[1\] = 2"), ([-1], r"\[0\] = -1"), ([], "at least one"), ([[0, 1]], "flat")):
        with pytest.raises(ValueError, match=needle):
            op.frame_index_host(bad, 2)
    with pytest.raises(TypeError):
        op.frame_index_host([0.0, 1.0], 2)


def test_models_refuse_bad_assignments_before_any_launch():
    """CPU images: the checks come first (a good assignment then reaches the 'must live on the GPU' error, nothing else)."""
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet
    vol = _vol()
    inp = synth.make_inputs(F, NV, 64, seed=1)
    kp = np.random.RandomState(2).randn(P, J, 3) * 100.0
    batch = lambda cf, k=kp: {"cameras": cameras(inp, F), "pred_keypoints_3d": k, "cuboid_frame": cf}
    images = inp["images"]
    with pytest.raises(ValueError, match="outside"):
        vol(images, None, batch([0, 1, 2, 0, 1]))
    with pytest.raises(ValueError, match="outside"):
        vol(images, None, batch([0, -1, 1, 0, 1]))
    with pytest.raises(ValueError, match="5 cuboids.*4 entries"):
        vol(images, None, batch(list(FRAME_OF), kp[:4]))
    with pytest.raises(ValueError, match="at least one"):
        vol(images, None, batch([], kp[:0]))
    with pytest.raises(RuntimeError, match="GPU"):
        vol(images, None, batch(list(FRAME_OF)))
    with pytest.raises(RuntimeError, match="GPU"):
        vol(images, None, batch(torch.tensor([1, 1, 1, 1, 1])))          # any order; a frame may have no cuboid
    vol.max_samples_per_launch = lambda *a: 4
    with pytest.raises(ValueError, match="one plan"):
        vol(images, None, batch(list(FRAME_OF)))
    del vol.max_samples_per_launch
    vol.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        vol(images, None, batch(list(FRAME_OF)))
    vol.eval()
    alg = AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu").eval()
    casc = CascadeTriangulationNet(alg, vol).eval()
    with pytest.raises(NotImplementedError, match="ONE pelvis per frame"):
        casc(images, torch.zeros(F, NV, 3, 4), batch(list(FRAME_OF)))


def test_unproject_heatmaps_frame_index_is_inference_only():
    from mvn.utils import op
    hm = torch.randn(2, 3, 4, 8, 8, requires_grad=True)
    args = (torch.zeros(2, 3, 3, 4), torch.zeros(5, 4, 4, 16, 3))
    with pytest.raises(NotImplementedError, match="frame_index"):
        op.unproject_heatmaps(hm, *args, "sum", frame_index=list(FRAME_OF))
    conf = torch.rand(2, 3, 4, requires_grad=True)
    with pytest.raises(NotImplementedError, match="frame_index"):
        op.unproject_heatmaps(hm.detach(), *args, "conf", vol_confidences=conf, frame_index=list(FRAME_OF))
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):          # no gradient asked: it gets as far as the device check
        op.unproject_heatmaps(hm, *args, "sum", frame_index=list(FRAME_OF))


# ---- 3. the C ABI without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_with_the_declared_signatures():
    lib = C.CDLL(H.LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    for name in ("lt_unproject_indexed_fwd", "lt_unproject_grid_indexed_fwd", "lt_plan_create_vol_multi", "lt_plan_forward_vol_multi"):
        assert hasattr(lib, name) and name in H.SIGNATURES, name
    assert H.SIGNATURES["lt_unproject_indexed_fwd"] == (C.c_int, [i32] + [vp] * 7 + [i32] * 10 + [vp])
    assert H.SIGNATURES["lt_unproject_grid_indexed_fwd"] == (C.c_int, [i32] + [vp] * 5 + [f32, i32] + [vp] * 5 + [i32] * 8 + [vp])
    res, args = H.SIGNATURES["lt_plan_create_vol_multi"]
    assert res is C.c_int and args[0] is C.POINTER(H.VolPlanConfig) and args[1] is i32 and len(args) == 5
    assert H.SIGNATURES["lt_plan_forward_vol_multi"] == (C.c_int, [vp] * 14)
    assert [f[0] for f in H.VolPlanConfig._fields_][4:8] == ["B", "NV", "H", "W"] and C.sizeof(H.VolPlanConfig) == 72          # the config keeps its layout
    assert H.lib().lt_abi_version() == 1


def test_public_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    assert os.path.exists(cc), "no C compiler found (the build needs hipcc's clang at least)"
    src = tmp_path / "includer.c"
    src.write_text('#include "lt_hip.h"\n'
                   'int (*create)(const lt_vol_plan_config*, int32_t, const lt_named_tensor*, int32_t, lt_plan**) = lt_plan_create_vol_multi;\n'
                   'int (*fwd)(lt_plan*, const float*, const double*, const double*, const double*, const int32_t*, const double*, const double*, float*, float*, float*, '
                   'float*, float*, void*) = lt_plan_forward_vol_multi;\n'
                   'int (*gather)(int32_t, const void*, const float*, const float*, const float*, const uint8_t*, const int32_t*, void*, int32_t, int32_t, int32_t, int32_t, '
                   'int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, void*) = lt_unproject_indexed_fwd;\n'
                   'int main(void) { return 0; }\n')
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _cfg(**kw):
    v = H.VolPlanConfig()
    v.dtype, v.num_layers, v.style_caffe, v.num_joints = H.LT_F32, 18, 0, 17
    v.B, v.NV, v.H, v.W = F, NV, 128, 128
    v.volume_size, v.cuboid_side, v.volume_multiplier, v.volume_softmax, v.aggregation, v.use_graph = 32, 2500.0, 1.0, 1, H.AGG["softmax"], 1
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def _weights():
    arr = (H.NamedTensor * 1)()
    keep = (C.c_float * 1)()
    arr[0].name, arr[0].data, arr[0].ndim, arr[0].shape[0] = b"backbone.conv1.weight", C.cast(keep, C.c_void_p), 1, 1
    return arr, keep


def _create(cfg, n_cuboids):
    w, keep = _weights()
    plan = C.c_void_p()
    rc = H.lib().lt_plan_create_vol_multi(C.byref(cfg), n_cuboids, w, 1, C.byref(plan))
    assert not plan.value
    return rc, H.lib().lt_last_error().decode()


@pytest.mark.parametrize("field,value,cuboids,needle", [
    (None, None, 0, "P 0"), (None, None, -3, "P -3"), ("dtype", 7, P, "dtype 7"), ("dtype", H.LT_FP8, P, "dtype 2"), ("B", 0, P, "bad shape"),
    ("NV", 0, P, "bad shape"), ("H", 16, P, "bad shape"), ("volume_size", 1, P, "bad shape"), ("num_joints", 0, P, "bad shape"), ("aggregation", 9, P, "aggregation 9"),
])
def test_multi_plan_config_validation(field, value, cuboids, needle):
    rc, msg = _create(_cfg(**({field: value} if field else {})), cuboids)
    assert rc == ERR_INVALID and needle in msg and "lt_plan_create_vol_multi" in msg, (rc, msg)


def test_multi_plan_null_arguments():
    lib = H.lib()
    w, keep = _weights()
    plan = C.c_void_p()
    cfg = _cfg()
    for args in ((None, P, w, 1, C.byref(plan)), (C.byref(cfg), P, None, 1, C.byref(plan)), (C.byref(cfg), P, w, 0, C.byref(plan)), (C.byref(cfg), P, w, 1, None)):
        assert lib.lt_plan_create_vol_multi(*args) == ERR_INVALID and "null" in lib.lt_last_error().decode()
    assert lib.lt_plan_forward_vol_multi(None, 1, 1, 1, 1, 1, 1, None, 1, None, None, None, None, None) == ERR_INVALID and "null" in lib.lt_last_error().decode()
    # the gather's own checks come before any launch too
    assert lib.lt_unproject_indexed_fwd(H.LT_F32, 1, 1, 1, None, None, None, 1, 2, 5, 3, 4, 8, 8, 4, 4, 16, 0, None) == ERR_INVALID and "frame_of" in lib.lt_last_error().decode()
    assert lib.lt_unproject_indexed_fwd(H.LT_F32, 1, 1, 1, None, None, 1, 1, 0, 5, 3, 4, 8, 8, 4, 4, 16, 0, None) == ERR_INVALID and "F 0" in lib.lt_last_error().decode()
    assert lib.lt_unproject_grid_indexed_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, None, 1, 1, 2, 0, 3, 4, 8, 8, 16, 0, None) == ERR_INVALID
    assert "P 0" in lib.lt_last_error().decode()


# ---- 4. the fixture ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,prefix", [("mpii", ""), ("coco", "coco/")])
def test_fixture_matches_what_this_file_rebuilds(golden_dir, kind, prefix):
    path = os.path.join(golden_dir, "multi_cuboid_small.npz")
    assert os.path.getsize(path) < T.MAX_BYTES
    g = np.load(path, allow_pickle=False)
    k = lambda name: g[prefix + name]
    vcfg, vsd, inp, kp = multi_setup(kind, k("seeds"))
    assert np.allclose(synth.state_dict_checksum(vsd), k("vol_sd_digest"), rtol=1e-12)
    assert np.allclose(T.images_digest(inp["images"]), k("images_digest"), rtol=1e-12)
    assert np.array_equal(kp, k("pred_keypoints_3d")) and k("frame_of").tolist() == list(FRAME_OF)
    from oracle import vol_oracle as O
    base = O.base_points_from_batch(kp, kind)
    assert np.array_equal(base, k("truth/base_points")) and np.array_equal(k("cuboid_pos"), base - 1250.0)
    assert float(np.linalg.norm(base, axis=1).max()) <= 2500.0 / 4          # within cuboid_side / 4 of the point the ring cameras look at
    assert min(np.linalg.norm(base[i] - base[j]) for i in range(P) for j in range(i)) > 1.0          # distinct
    assert float(k("ref32_err/kp")) <= 0.25e-4 and T.joints_rel(k("kp"), k("truth/kp")) == float(k("ref32_err/kp"))
    s = int(k("stride"))
    assert k("kp").shape == (P, J, 3) and k("vol_sub").shape == (P, J, V // s, V // s, V // s) and k("feat_sub").shape == (F * NV, 32, HW // 4 // s, HW // 4 // s)
    assert k("cv_sub").shape == (P, V // s, V // s, V // s, 3)
