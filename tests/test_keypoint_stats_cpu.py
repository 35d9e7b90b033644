"""CPU: per-joint statistics of the volumetric joints' 3D heatmaps.  The numpy fp64 statement (mvn.utils.volumetric.keypoint_stats) against a brute-force
loop over the voxels; the recorded launch lists of plans with and without ``keypoint_stats``; the refusals of the C entry points that fire before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import synth

ERR_INVALID, ERR_UNSUPPORTED = -1, -2


def _brute(x, coords, kp, softmax, mass32=None):
    """One (b, j) at a time, one voxel at a time, in Python floats (fp64): the definitions of include/lt_hip.h, written as loops."""
    B, J, n = x.shape
    peak, idx, mass, cov = np.zeros((B, J)), np.zeros((B, J), dtype=np.int64), np.zeros((B, J)), np.zeros((B, J, 3, 3))
    for b in range(B):
        for j in range(J):
            xs = [float(v) for v in x[b, j]]
            best = 0
            for i in range(1, n):
                if xs[i] > xs[best]:          # strict: the smallest index of equal maxima
                    best = i
            if softmax:
                e = [np.exp(v - xs[best]) for v in xs]
                s = sum(e)
                p = [v / s for v in e]
                m = 1.0
                centre = [float(v) for v in kp[b, j]]
            else:
                w = [max(v, 0.0) for v in xs]
                m = sum(w)
                m32 = np.float32(m) if mass32 is None else np.float32(mass32[b, j])
                p = [v / m if m > 0 else 0.0 for v in w]
                centre = [float(np.float32(v) / m32) if m > 0 else 0.0 for v in kp[b, j]]
            peak[b, j], idx[b, j], mass[b, j] = p[best], best, m
            for i in range(n):
                d = [float(coords[b, i, r]) - centre[r] for r in range(3)]
                for r in range(3):
                    for s_ in range(3):
                        cov[b, j, r, s_] += p[i] * d[r] * d[s_]
    return peak, idx, mass, cov


def _rotated_grid(B, V, rng):
    """(B, V^3, 3) fp32 voxel centres of a 2500 mm cuboid at a non-zero base point, rotated about the vertical through the base like the model's cuboids."""
    from mvn.utils import volumetric
    ax = np.linspace(-1250.0, 1250.0, V)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    out = np.empty((B, V ** 3, 3), dtype=np.float32)
    for b in range(B):
        R = volumetric.get_rotation_matrix([0, 0, 1], 0.7 + 1.3 * b)
        out[b] = (g @ R.T + np.array([130.0 + 100.0 * b, -220.0, 310.0])).astype(np.float32)
    return out


@pytest.mark.parametrize("softmax", [True, False], ids=["softmax", "relu"])
def test_numpy_statement_agrees_with_a_per_voxel_loop(softmax):
    from mvn.utils import volumetric
    rng = np.random.default_rng(5)
    B, J, V = 2, 3, 5
    coords = _rotated_grid(B, V, rng)
    x = (rng.standard_normal((B, J, V ** 3)) * (3.0 if softmax else 0.05)).astype(np.float32)
    x[0, 1, 17] = x[0, 1, 90] = x[0, 1].max() + 1.0          # two equal maxima: the lower index is the peak
    if not softmax:
        x[1, 2] = -np.abs(x[1, 2])                            # no mass at all
    p = np.exp(x.astype(np.float64) - x.max(2, keepdims=True)); p /= p.sum(2, keepdims=True)
    w = p if softmax else np.maximum(x.astype(np.float64), 0.0)
    kp = np.einsum("bjn,bnc->bjc", w, coords.astype(np.float64)).astype(np.float32)          # what the soft-argmax returns: fp32, ReLU not normalised
    st = volumetric.keypoint_stats(x.reshape(B, J, V, V, V), coords.reshape(B, V, V, V, 3), kp, softmax=softmax)
    peak, idx, mass, cov = _brute(x, coords, kp, softmax)
    assert np.array_equal(st.peak_index, idx) and st.peak_index[0, 1] == 17
    assert np.allclose(st.peak, peak, rtol=1e-12, atol=0) and np.allclose(st.mass, mass, rtol=1e-12, atol=0)
    tr = np.trace(cov, axis1=2, axis2=3)
    assert float(np.abs(st.covariance - cov).max() / tr.max()) < 1e-12
    assert np.array_equal(st.covariance, np.swapaxes(st.covariance, 2, 3))          # symmetric, exactly
    ev = np.linalg.eigvalsh(st.covariance)
    assert (ev >= -1e-9 * np.maximum(tr, 1.0)[..., None]).all()                      # positive semi-definite
    if softmax:
        assert np.array_equal(st.mass, np.ones((B, J)))
    else:
        assert st.mass[1, 2] == 0 and st.peak[1, 2] == 0 and not st.covariance[1, 2].any()
    # the same numbers from the returned volumes instead of the logits
    sp = volumetric.keypoint_stats(w, coords, kp, softmax=softmax, from_probs=True)
    some = mass > 0          # relu(x) of a volume without a positive logit is all zeros: its peak voxel is only known from x
    assert np.array_equal(sp.peak_index[some], idx[some])
    assert np.allclose(sp.peak, peak, rtol=1e-12) and float(np.abs(sp.covariance - cov).max() / tr.max()) < 1e-12


def test_numpy_statement_on_a_one_voxel_volume():
    from mvn.utils import volumetric
    coords = np.array([[[1e5, -2e5, 5e4]]], dtype=np.float32)          # (1, 1, 3)
    x = np.array([[[0.3], [-4.0]]], dtype=np.float32)                   # (1, 2, 1)
    kp = np.repeat(coords, 2, axis=1)
    st = volumetric.keypoint_stats(x, coords, kp, softmax=True)
    assert np.array_equal(st.peak, np.ones((1, 2))) and not st.peak_index.any() and not st.covariance.any()
    with pytest.raises(ValueError, match="voxels"):
        volumetric.keypoint_stats(x, np.zeros((1, 2, 3), dtype=np.float32), kp)


def test_moments_about_the_joint_survive_world_coordinates():
    """The case a raw-moment formulation loses: a cuboid at (1e5, -2e5, 5e4) mm.  The statement's covariance does not depend on where the cuboid is."""
    from mvn.utils import volumetric
    rng = np.random.default_rng(9)
    near = _rotated_grid(1, 4, rng).astype(np.float64)
    shift = np.array([1e5, -2e5, 5e4])
    x = (rng.standard_normal((1, 2, 64)) * 3.0).astype(np.float32)
    p = np.exp(x.astype(np.float64) - x.max(2, keepdims=True)); p /= p.sum(2, keepdims=True)
    covs = []
    for c in (near, near + shift):
        kp = np.einsum("bjn,bnc->bjc", p, c)
        covs.append(volumetric.keypoint_stats(x, c, kp.astype(np.float64), softmax=True).covariance)
    # keypoints are rounded to fp32 inside the statement (they are the RETURNED joints): 2e5 mm has an ulp of 0.016 mm, against a spread of ~ 1000 mm
    assert float(np.abs(covs[0] - covs[1]).max() / np.trace(covs[0], axis1=2, axis2=3).max()) < 1e-4


def test_records_to_keypoint_stats():
    from mvn.utils import op
    rec = torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(2, 3, 8)
    idx = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    st = op.keypoint_stats_from_records(rec, idx)
    assert isinstance(st, op.KeypointStats) and st._fields == ("peak", "peak_index", "mass", "covariance")
    assert torch.equal(st.peak, rec[..., 0]) and torch.equal(st.mass, rec[..., 1]) and st.peak_index is idx
    assert st.covariance.shape == (2, 3, 3, 3) and torch.equal(st.covariance, st.covariance.transpose(2, 3))
    assert st.covariance[1, 2].tolist() == [[42.0, 43.0, 44.0], [43.0, 45.0, 46.0], [44.0, 46.0, 47.0]]


# ---- plans --------------------------------------------------------------------------------------------------------------------------------------------
def _kinds(plan):
    return [meta["kind"] for _, meta in plan.ops]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_flagged_plan_has_its_own_key_and_the_same_launches(dt):
    from mvn.models.triangulation import VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    vol.compute_dtype = dt
    assert vol.keypoint_stats is False and vol.last_keypoint_stats is None
    never = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True)          # the call of a host that has never heard of the flag
    off = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True, stats=False)
    on = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True, stats=True)
    both = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True, masked=True, stats=True)
    for P in (off, on, both):
        assert _kinds(P["plan"]) == _kinds(never["plan"]) and len(P["plan"].ops) == len(never["plan"].ops)
        assert P["plan"].nhead == never["plan"].nhead and P["plan"].npre == never["plan"].npre
    last = lambda P: P["plan"].ops[-1][1]
    assert last(never)["kind"] == last(on)["kind"] == "softargmax3d"
    assert "entry" not in last(never)["info"] and "entry" not in last(off)["info"] and sorted(last(off)["info"]) == sorted(last(never)["info"])
    assert last(off)["bytes"] == last(never)["bytes"]
    for P in (on, both):
        info = last(P)["info"]
        assert info["entry"] == "lt_softargmax3d_stats_fwd"
        assert tuple(info["stats"].shape) == (2, 17, 8) and info["stats"].dtype == torch.float32
        assert tuple(info["peak_index"].shape) == (2, 17) and info["peak_index"].dtype == torch.int32
        assert P["kstats"] is info["stats"] and P["kindex"] is info["peak_index"]
    assert off["kstats"] is None and never["kindex"] is None
    # the flagged tail additionally reads the coordinates once per sample
    assert last(on)["bytes"] == last(never)["bytes"] + 2 * 32 ** 3 * 12
    # the key
    k = lambda **kw: vol._plan_key(2, 4, 64, 64, "cpu", **kw)
    assert k() == k(masked=False, stats=False) and k(stats=True) != k() and k(masked=True, stats=True) != k(masked=True) and k(masked=True, stats=True) != k(stats=True)


def test_c_entry_points_check_their_arguments():
    lib = H.lib()
    for name in ("lt_softargmax3d_stats_workspace", "lt_softargmax3d_stats_fwd", "lt_plan_set_keypoint_stats"):
        assert hasattr(C.CDLL(H.LIB_PATH), name) and name in H.SIGNATURES, name
    err = lambda: lib.lt_last_error().decode()
    # arguments: logits, coords, mult, softmax, channels_last, ld, kp, probs, stats, peak_index, B, J, nvox, workspace, stream
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 0, 5, 1, None, None, 1, 2, 5, 343, 1, None) == ERR_INVALID and "stats" in err()
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 0, 5, 1, None, 1, None, 2, 5, 343, 1, None) == ERR_INVALID and "peak_index" in err()
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 0, 5, None, None, 1, 1, 2, 5, 343, 1, None) == ERR_INVALID and "lt_softargmax3d_stats_fwd" in err()
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 1, 33, 1, None, 1, 1, 2, 33, 343, 1, None) == ERR_UNSUPPORTED and "J=33" in err()
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 1, 8, 1, None, 1, 1, 2, 5, 343, 1, None) == ERR_UNSUPPORTED and "ld == J" in err()
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 1, 4, 1, None, 1, 1, 2, 5, 343, 1, None) == ERR_INVALID
    assert lib.lt_softargmax3d_stats_fwd(1, 1, 1.0, 1, 0, 5, 1, None, 1, 1, 1, 5, 1 << 31, 1, None) == ERR_UNSUPPORTED and "int32" in err()
    # the workspace: the plain call's, then one 8-float record per (b, j, 2048-voxel chunk)
    plain = lib.lt_softargmax3d_workspace(2, 17, 64 ** 3)
    assert lib.lt_softargmax3d_stats_workspace(2, 17, 64 ** 3) == plain + 2 * 17 * 128 * 8 * 4
    assert lib.lt_softargmax3d_stats_workspace(1, 1, 1) == lib.lt_softargmax3d_workspace(1, 1, 1) + 8 * 4
    assert lib.lt_plan_set_keypoint_stats(None, None, None) == ERR_INVALID and "null plan" in err()


def _interpret_keypoint_stats(plan):
    """The branch of the plan interpreter (tests/emul.py:run_plan_on_cpu) for a tail recorded as lt_softargmax3d_stats_fwd: the interpreter has evaluated the op
    by its kind (joints and probabilities); this fills the two buffers the flagged entry point adds, by the numpy statement of the definitions."""
    from mvn.utils import volumetric
    _, meta = plan.ops[-1]
    info = meta["info"]
    assert meta["kind"] == "softargmax3d" and info["entry"] == "lt_softargmax3d_stats_fwd"
    x = (info["logits"].t.float().permute(0, 4, 1, 2, 3) * torch.tensor(info["mult"], dtype=torch.float32)).numpy()
    st = volumetric.keypoint_stats(x, info["coords"].numpy(), info["kp"].numpy(), softmax=bool(info["softmax"]))
    c = st.covariance
    rec = np.stack([st.peak, st.mass, c[..., 0, 0], c[..., 0, 1], c[..., 0, 2], c[..., 1, 1], c[..., 1, 2], c[..., 2, 2]], axis=-1)
    info["stats"].copy_(torch.from_numpy(rec).float())
    info["peak_index"].copy_(torch.from_numpy(st.peak_index).int())


def test_interpreted_flagged_plan_gives_the_statistics_of_the_oracle_heatmaps():
    """A flagged dry-run plan through the interpreter: joints and probabilities as without the flag, the statistics those of the oracle's volumes."""
    from emul import run_plan_on_cpu
    from mvn.models.triangulation import VolumetricTriangulationNet
    from mvn.utils import op, volumetric
    from oracle import spec
    from oracle import vol_oracle as O
    from test_view_mask_cpu import cameras
    nb, nv, hw, V = 1, 2, 64, 32
    cfg = synth.vol_config(18, V, "softmax")
    sd = synth.make_state_dict(spec.vol_net_spec(18, 17, False), seed=31, sharpen=True, basic_block=True)
    inp = synth.make_inputs(nb, nv, hw, seed=31)
    m = VolumetricTriangulationNet(cfg, device="cpu")
    m.load_state_dict(sd, strict=True)
    m.eval()
    P = m._build_plan(nb, nv, hw, hw, "cpu", dry_run=True, stats=True)
    m._host_geometry({"cameras": cameras(inp, nb), "pred_keypoints_3d": inp["pred_keypoints_3d"]}, nb, (hw, hw), P)
    P["geo"].copy_(P["geo_host"])
    P["x_in"].t.zero_()
    P["x_in"].t[:, 0, :, :, :3] = inp["images"].reshape(nb * nv, 3, hw, hw).permute(0, 2, 3, 1)
    run_plan_on_cpu(P["plan"])
    _interpret_keypoint_stats(P["plan"])
    st = op.keypoint_stats_from_records(P["kstats"], P["kindex"])
    o = O.volumetric_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"], inp["pred_keypoints_3d"])
    want = volumetric.keypoint_stats(o["volumes"].numpy(), o["coord_volumes"].numpy(), o["keypoints_3d"].numpy(), softmax=True, from_probs=True)
    # a WIRING check like tests/test_plan_cpu.py's (sharpened heatmaps: 1e-3 on the probabilities there), not the parity gate
    assert float(np.abs(st.peak.numpy() - want.peak).max() / want.peak.max()) < 1e-3
    tr = np.trace(want.covariance, axis1=2, axis2=3)
    assert float((np.abs(st.covariance.numpy() - want.covariance).max(axis=(2, 3)) / tr).max()) < 1e-2
    assert (st.peak_index.numpy() == want.peak_index).mean() > 0.9 and bool((st.mass == 1).all())
