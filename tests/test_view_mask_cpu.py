"""CPU: per-sample view masks.  The oracle reproduces tests/golden/view_mask_small.npz on the valid views of each sample (the mask's meaning: sample b is
what the reference gives on its valid views alone); every validation error of the functional ops, the models and the C entry points fires without a GPU; a
masked plan has its own cache key, the same number of launches, and leaves the unmasked plan's recorded launches as they are."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import spec, synth
from oracle import truth as T
from oracle import vol_oracle as O

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
F64 = torch.float64


def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "view_mask_small.npz"))


NL, J, B, NV, HW, V = 18, 17, 3, 4, 128, 32          # tools/make_golden_view_mask.py


def vm_setup(seeds):
    """tools/make_golden_view_mask.py:setup -- configs and state dicts of the cases, the inputs and the fp32 image-resolution projections, from the seeds
    the fixture stores."""
    alg_seed, vol_seed, conf_seed, input_seed = [int(s) for s in seeds]
    acfg = synth.alg_config(NL, True, J)
    acfg.model.heatmap_multiplier = 1.0
    cfgs = {"alg": acfg, "vol_softmax": synth.vol_config(NL, V, "softmax", 1.0, "mpii"), "vol_conf_norm": synth.vol_config(NL, V, "conf_norm", 1.0, "mpii")}
    sds = {"alg": synth.make_state_dict(spec.alg_net_spec(NL, J, True), seed=alg_seed, basic_block=True),
           "vol_softmax": synth.make_state_dict(spec.vol_net_spec(NL, J, False), seed=vol_seed, basic_block=True),
           "vol_conf_norm": synth.make_state_dict(spec.vol_net_spec(NL, J, True), seed=conf_seed, basic_block=True)}
    inp = synth.make_inputs(B, NV, HW, seed=input_seed)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(B, 1, 1, 1)
    return cfgs, sds, inp, P


def cameras(inp, nb):
    from mvn.utils.multiview import Camera
    return [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(nb)] for v in range(inp["K"].shape[0])]


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_data_only_and_small(golden_dir):
    path = os.path.join(golden_dir, "view_mask_small.npz")
    assert os.path.getsize(path) < T.MAX_BYTES
    g = np.load(path, allow_pickle=False)
    assert g["masks"].tolist() == [[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 1]]
    for k in ("vol_softmax/kp", "vol_conf_norm/kp", "alg/kp3", "cascade/kp"):
        assert g[k].shape == (3, 17, 3) and g["truth/" + k].dtype == np.float64 and float(g["ref32_err/" + k]) >= 0
    assert float(g["ref32_err/vol_softmax/kp"]) <= 0.25e-4 and float(g["ref32_err/vol_conf_norm/kp"]) <= 0.25e-4 and float(g["ref32_err/cascade/kp"]) <= 0.25e-4
    on = g["masks"].astype(bool)
    assert np.isnan(g["alg/kp2"][~on]).all() and np.isfinite(g["alg/kp2"][on]).all() and np.isnan(g["alg/conf"][~on]).all()


def _close(a, b, tol, what):
    """max|a - b| / max|b| <= tol, as tests/test_oracle_golden.py:_close."""
    e = T.max_rel(a.numpy() if torch.is_tensor(a) else a, b)
    assert e <= tol, "%s: max|d|/max|ref| = %.3e > %.1e" % (what, e, tol)


def _joints_close(a, b, what):
    rel = T.joints_rel(a.numpy() if torch.is_tensor(a) else a, b)
    assert rel <= 1e-4, "%s: joints max rel %.3e" % (what, rel)


def test_oracle_reproduces_the_fixture_on_the_valid_views(golden_dir):
    """The fp32 oracle, run per sample on its valid views alone, against the reference's stored fp32 outputs of all four cases, at the tolerances of
    tests/test_oracle_golden.py (2D keypoints and confidences 1e-4, algebraic joints 1e-3, volumes 1e-3, volumetric joints 1e-4 of the 1 mm floored magnitude);
    the second stage of the two-stage route on the REFERENCE's pelvis, as tests/test_cascade_cpu.py isolates it.  The weights and images the GPU tests
    rebuild from the stored seeds are pinned by their digests."""
    g = fixture(golden_dir)
    cfgs, sds, inp, P = vm_setup(g["seeds"])
    for name, key in (("alg", "alg_sd_digest"), ("vol_softmax", "vol_sd_digest"), ("vol_conf_norm", "conf_sd_digest")):
        assert np.allclose(synth.state_dict_checksum(sds[name]), g[key], rtol=1e-12), "weight generator drift: " + name
    assert np.allclose(T.images_digest(inp["images"]), g["images_digest"], rtol=1e-12)
    s = int(g["stride"])
    for b in range(3):
        idx = np.nonzero(g["masks"][b])[0]
        what = "sample %d (views %s) " % (b, idx.tolist())
        img = inp["images"][b:b + 1, idx].contiguous()
        K, R, t = inp["K"][idx], inp["R"][idx], inp["t"][idx]
        pred = inp["pred_keypoints_3d"][b:b + 1]
        a = O.algebraic_forward(sds["alg"], cfgs["alg"], img, K, R, t)
        _close(a["keypoints_2d"][0], g["alg/kp2"][b][idx], 1e-4, what + "alg keypoints_2d")
        _close(a["alg_confidences"][0], g["alg/conf"][b][idx], 1e-4, what + "alg confidences")
        _close(a["keypoints_3d"][0], g["alg/kp3"][b], 1e-3, what + "alg keypoints_3d")
        v = O.volumetric_forward(sds["vol_softmax"], cfgs["vol_softmax"], img, K, R, t, pred)
        _joints_close(v["keypoints_3d"][0], g["vol_softmax/kp"][b], what + "vol softmax")
        _close(v["volumes"][0][:, ::s, ::s, ::s], g["vol_softmax/vol_sub"][b], 1e-3, what + "vol softmax volumes")
        c = O.volumetric_forward(sds["vol_conf_norm"], cfgs["vol_conf_norm"], img, K, R, t, pred)
        _joints_close(c["keypoints_3d"][0], g["vol_conf_norm/kp"][b], what + "vol conf_norm")
        _close(c["vol_confidences"][0], g["vol_conf_norm/conf"][b][idx], 1e-4, what + "vol conf_norm confidences")
        assert abs(float(g["vol_conf_norm/conf"][b][idx].sum(axis=0).mean()) - 1.0) < 1e-5          # normalised over the VALID views
        # the two-stage route: its first stage is the algebraic case, its second runs on the reference's fp32 pelvis
        assert np.array_equal(g["cascade/alg_kp3"][b], g["alg/kp3"][b])
        o = O.volumetric_forward(sds["vol_softmax"], cfgs["vol_softmax"], img, K, R, t, g["cascade/alg_kp3"][b:b + 1])
        _close(o["base_points"][0], g["cascade/base_points"][b], 1e-7, what + "cascade base_points")
        _joints_close(o["keypoints_3d"][0], g["cascade/kp"][b], what + "cascade")


def test_public_header_compiles_as_c(tmp_path):
    """include/lt_hip.h is the drop-in boundary for hosts in C: a one-line includer must pass a C11 syntax check, and every prototype must be at file scope
    (what the name scan of tests/test_host_logic.py cannot see)."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    assert os.path.exists(cc), "no C compiler found (the build needs hipcc's clang at least)"
    src = tmp_path / "includer.c"
    src.write_text('#include "lt_hip.h"\nint (*probe)(lt_plan*, const uint8_t*) = lt_plan_set_view_mask;\nint main(void) { lt_cascade_plan_config c; c.kind = LT_KIND_MPII; '
                   'return c.kind; }\n')
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- validation without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_view_mask_host_checks():
    from mvn.utils import op
    m = op.view_mask_host(torch.tensor([[True, False], [True, True]]), 2, 2)
    assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and m.tolist() == [[1, 0], [1, 1]]
    assert op.view_mask_host(np.array([[7, 0], [0, 255]], dtype=np.uint8), 2, 2).tolist() == [[1, 0], [0, 1]]
    with pytest.raises(ValueError, match=r"\(2, 2\).*\(2, 3\)"):
        op.view_mask_host(np.ones((2, 3), dtype=bool), 2, 2)
    with pytest.raises(ValueError, match="sample 1 has 0 valid views, at least 1"):
        op.view_mask_host(np.array([[1, 0], [0, 0]]), 2, 2, min_valid=1)
    with pytest.raises(ValueError, match="sample 0 has 1 valid view, at least 2"):
        op.view_mask_host(np.array([[1, 0], [1, 1]]), 2, 2, min_valid=2)
    with pytest.raises(TypeError):
        op.view_mask_host(np.ones((2, 2), dtype=np.float32), 2, 2)


def _models():
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet, VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    alg = AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu").eval()
    return vol, alg, CascadeTriangulationNet(alg, vol).eval()


def test_models_refuse_bad_masks_before_any_launch():
    """CPU images: the mask checks come first (a good mask then reaches the 'must live on the GPU' error, nothing else)."""
    vol, alg, casc = _models()
    inp = synth.make_inputs(2, 4, 64, seed=1)
    images, P = inp["images"], torch.zeros(2, 4, 3, 4)
    batch = lambda m: {"cameras": cameras(inp, 2), "pred_keypoints_3d": inp["pred_keypoints_3d"], "view_mask": m}
    for net in (vol, alg, casc):
        with pytest.raises(ValueError, match=r"\(B, NV\) = \(2, 4\)"):
            net(images, P, batch(np.ones((2, 3), dtype=bool)))
        with pytest.raises(ValueError, match=r"\(B, NV\) = \(2, 4\)"):
            net(images, P, batch(np.ones((4,), dtype=bool)))
    with pytest.raises(ValueError, match="sample 1 has 0 valid views"):
        vol(images, P, batch(np.array([[1, 1, 1, 1], [0, 0, 0, 0]])))
    for net in (alg, casc):
        with pytest.raises(ValueError, match="sample 1 has 1 valid view, at least 2"):
            net(images, P, batch(torch.tensor([[1, 1, 1, 1], [0, 0, 1, 0]], dtype=torch.uint8)))
    for net in (vol, alg, casc):          # a good mask passes the checks
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            net(images, P, batch(np.array([[1, 0, 1, 1], [0, 1, 0, 1]], dtype=bool)))
    one_view = np.array([[1, 0, 0, 0], [0, 0, 0, 1]], dtype=bool)          # enough for the volumetric model
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        vol(images, P, batch(one_view))
    for net in (vol, alg, casc):          # training mode
        net.train()
        with pytest.raises(NotImplementedError):
            net(images, P, batch(np.ones((2, 4), dtype=bool)))
        net.eval()


def test_ransac_refuses_a_mask():
    from mvn.models.triangulation import RANSACTriangulationNet
    cfg = synth.alg_config(18, False, 17)
    cfg.model.direct_optimization = True
    net = RANSACTriangulationNet(cfg, device="cpu").eval()
    inp = synth.make_inputs(1, 4, 64, seed=1)
    with pytest.raises(NotImplementedError, match="view_mask"):
        net(inp["images"], torch.zeros(1, 4, 3, 4), {"cameras": cameras(inp, 1), "view_mask": np.ones((1, 4), dtype=bool)})


def test_c_entry_points_check_their_arguments():
    lib = H.lib()
    for name in ("lt_unproject_masked_fwd", "lt_unproject_grid_masked_fwd", "lt_alg_tail_masked_fwd", "lt_plan_set_view_mask"):
        assert hasattr(C.CDLL(H.LIB_PATH), name) and name in H.SIGNATURES, name
    err = lambda: lib.lt_last_error().decode()
    # a null view_mask is LT_ERR_INVALID, with every other pointer given
    assert lib.lt_unproject_masked_fwd(H.LT_F32, 1, 1, 1, None, None, 1, 1, 4, 32, 8, 8, 4, 4, 16, H.AGG["sum"], None) == ERR_INVALID and "null view_mask" in err()
    assert lib.lt_unproject_grid_masked_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, None, 1, 1, 4, 32, 8, 8, 16, H.AGG["sum"], None) == ERR_INVALID
    assert "null view_mask" in err()
    assert lib.lt_alg_tail_masked_fwd(1, None, 17, 1, 1.0, 1.0, None, None, None, 1, 2, 4, 17, None) == ERR_INVALID and "null view_mask" in err()
    # the checks of the unmasked entries hold
    assert lib.lt_unproject_masked_fwd(H.LT_F32, None, 1, 1, None, 1, 1, 1, 4, 32, 8, 8, 4, 4, 16, H.AGG["sum"], None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_masked_fwd(7, 1, 1, 1, None, 1, 1, 1, 4, 32, 8, 8, 4, 4, 16, H.AGG["sum"], None) == ERR_INVALID and "dtype 7" in err()
    assert lib.lt_unproject_masked_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 1, 4, 32, 8, 8, 4, 4, 16, H.AGG["conf_norm"], None) == ERR_INVALID and "confidences" in err()
    assert lib.lt_unproject_masked_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 1, 0, 32, 8, 8, 4, 4, 16, H.AGG["sum"], None) == ERR_INVALID and "bad shape" in err()
    assert lib.lt_unproject_grid_masked_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, None, None, 1, 1, 1, 4, 32, 8, 8, 16, H.AGG["sum"], None) == ERR_INVALID
    assert lib.lt_alg_tail_masked_fwd(1, None, 17, 1, 1.0, 1.0, 1, None, None, 1, 2, 1, 17, None) == ERR_INVALID and "NV 1" in err()
    assert lib.lt_alg_tail_masked_fwd(1, 1, 16, 1, 1.0, 1.0, 1, None, None, 1, 2, 4, 17, None) == ERR_INVALID and "ld_conf 16" in err()
    assert lib.lt_plan_set_view_mask(None, None) == ERR_INVALID and "null plan" in err()
    m = (C.c_uint8 * 8)(*([1] * 8))
    assert lib.lt_plan_set_view_mask(None, C.cast(m, C.c_void_p)) == ERR_INVALID


# ---- plans --------------------------------------------------------------------------------------------------------------------------------------------
def _launches(plan):
    return [(meta["kind"], meta["label"]) for _, meta in plan.ops]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_masked_plan_has_its_own_key_and_the_same_launches(dt):
    from mvn.models.triangulation import AlgebraicTriangulationNet, VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    vol.compute_dtype = dt
    assert vol._plan_key(2, 4, 64, 64, "cpu", False) != vol._plan_key(2, 4, 64, 64, "cpu", True)
    assert vol._plan_key(2, 4, 64, 64, "cpu") == vol._plan_key(2, 4, 64, 64, "cpu", False)
    plain = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True)
    before = _launches(plain["plan"])
    masked = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True, masked=True)
    assert _launches(plain["plan"]) == before          # building the masked plan leaves the unmasked plan's recorded launches alone
    assert len(masked["plan"].ops) == len(plain["plan"].ops) and _launches(masked["plan"]) == before
    assert masked["masked"] and not plain["masked"]
    un = [meta for _, meta in masked["plan"].ops if meta["kind"] == "unproject"]
    assert len(un) == 1 and un[0]["info"]["masked"] and not [meta for _, meta in plain["plan"].ops if meta["kind"] == "unproject"][0]["info"]["masked"]
    # the mask rides behind the floats of the geometry block: B * NV bytes in whole words, nothing else moves
    n = 2 * 4 * 12 + 2 * 15
    assert plain["geo"].numel() == n and masked["geo"].numel() == n + 2 and masked["o_mask"] == n and masked["offs"] == plain["offs"]
    alg = AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu").eval()
    alg.compute_dtype = dt
    assert alg._plan_key(2, 4, 64, 64, "cpu", False) != alg._plan_key(2, 4, 64, 64, "cpu", True)
    pa, ma = alg._build_plan(2, 4, 64, 64, "cpu", dry_run=True), alg._build_plan(2, 4, 64, 64, "cpu", dry_run=True, masked=True)
    assert _launches(pa["plan"]) == _launches(ma["plan"]) and tuple(ma["mask"].shape) == (8,) and ma["mask"].dtype == torch.uint8 and "mask" not in pa


def test_mask_is_written_into_the_geometry_block():
    """_host_cameras puts the mask bytes behind the rotations of the pinned slot; the floats in front are those of the unmasked plan."""
    from mvn.models.triangulation import VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    inp = synth.make_inputs(2, 3, 64, seed=4)
    batch = {"cameras": cameras(inp, 2), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    plain = vol._build_plan(2, 3, 64, 64, "cpu", dry_run=True)
    masked = vol._build_plan(2, 3, 64, 64, "cpu", dry_run=True, masked=True)
    vol._host_geometry(batch, 2, (64, 64), plain)
    m = np.array([[1, 0, 1], [0, 1, 1]], dtype=np.uint8)
    vol._host_geometry(dict(batch, view_mask=m), 2, (64, 64), masked)
    n = plain["geo_host"].numel()
    assert torch.equal(masked["geo_host"][:n], plain["geo_host"])
    assert masked["geo_host"].view(torch.uint8)[4 * n:4 * n + 6].tolist() == m.reshape(-1).tolist()
