"""CPU: per-joint statistics of the algebraic joints.  The numpy fp64 statement (mvn.utils.multiview.heatmap_stats_2d, triangulation_jacobian,
triangulation_stats): its Jacobian against central differences, the algebra of the propagated covariance, masking, the 2D heatmap statistics on maps with
known answers; the recorded launch lists of plans with and without ``keypoint_stats``; the refusals of the C entry points that fire before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import synth

ERR_INVALID, ERR_UNSUPPORTED = -1, -2


def rig(nv, B=2, J=3, seed=0, noise=2.0):
    """nv ring cameras (well-separated centres) looking at points within 300 mm of the origin: proj (B,nv,3,4), noisy 2D points (B,nv,J,2), confidences
    (B,nv,J) in (0.2, 1.2), 2D covariances (B,nv,J,2,2) (random, positive definite, px^2)."""
    rng = np.random.default_rng(seed)
    K, R, t = synth.ring_cameras(nv, 256)
    P = np.tile((K @ np.concatenate([R, t], -1))[None], (B, 1, 1, 1))
    X = rng.standard_normal((B, J, 3))
    X = X / np.linalg.norm(X, axis=-1, keepdims=True) * 300.0 * rng.random((B, J, 1))
    hh = np.einsum("bvik,bjk->bvji", P, np.concatenate([X, np.ones((B, J, 1))], -1))
    pts = hh[..., :2] / hh[..., 2:3] + rng.standard_normal((B, nv, J, 2)) * noise
    conf = rng.random((B, nv, J)) + 0.2
    L = rng.standard_normal((B, nv, J, 2, 2))
    cov = L @ np.swapaxes(L, -1, -2) + 0.5 * np.eye(2)
    return P, pts, conf, cov


@pytest.mark.parametrize("nv", [2, 4, 10])
def test_jacobian_of_the_statement_against_central_differences(nv):
    """Step 1e-3 px: truncation O(step^2), round-off about 1e-16 |X| / step = 1e-10; the gate is 1e-6 of the Jacobian's largest entry."""
    from mvn.utils import multiview
    P, pts, conf, _ = rig(nv, seed=nv)
    B, _, J = conf.shape
    X, jac = multiview.triangulation_jacobian(P, pts, conf)
    assert X.shape == (B, J, 3) and jac.shape == (B, nv, J, 3, 2) and np.isfinite(jac).all()
    step = 1e-3
    num = np.zeros_like(jac)
    for v in range(nv):
        for r in range(2):
            hi, lo = pts.copy(), pts.copy()
            hi[:, v, :, r] += step
            lo[:, v, :, r] -= step
            num[:, v, :, :, r] = (multiview.triangulation_jacobian(P, hi, conf)[0] - multiview.triangulation_jacobian(P, lo, conf)[0]) / (2 * step)
    err = float(np.abs(jac - num).max() / np.abs(jac).max())
    print("jacobian vs central differences, %d views: %.3e of the largest entry" % (nv, err))
    assert err <= 1e-6, err
    # the statement's joint is the host DLT's (unit confidences)
    X1 = multiview.triangulation_jacobian(P, pts)[0]
    want = multiview.triangulate_point_from_multiple_views_linear(P[0], pts[0, :, 1])
    assert np.allclose(X1[0, 1], want, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("nv", [2, 4, 10])
def test_covariance_is_the_jacobian_sandwich_symmetric_and_psd(nv):
    from mvn.utils import multiview
    P, pts, conf, cov2 = rig(nv, seed=10 + nv)
    X, jac = multiview.triangulation_jacobian(P, pts, conf)
    err, cov = multiview.triangulation_stats(P, pts, conf, cov2, X)
    want = np.zeros_like(cov)
    for v in range(nv):
        want += jac[:, v] @ cov2[:, v] @ np.swapaxes(jac[:, v], -1, -2)
    tr = np.trace(cov, axis1=2, axis2=3)
    assert (tr > 0).all() and float((np.abs(cov - want).max(axis=(2, 3)) / tr).max()) < 1e-12
    assert float((np.abs(cov - np.swapaxes(cov, 2, 3)).max(axis=(2, 3)) / tr).max()) < 1e-14
    assert (np.linalg.eigvalsh((cov + np.swapaxes(cov, 2, 3)) / 2) >= -1e-12 * tr[..., None]).all()
    # the packed {xx, xy, yy} form of the 2D covariances is the same input
    packed = np.stack([cov2[..., 0, 0], cov2[..., 0, 1], cov2[..., 1, 1]], -1)
    err2, cov_p = multiview.triangulation_stats(P, pts, conf, packed, X)
    assert np.array_equal(cov_p, cov) and np.array_equal(err2, err)
    # the reprojection error, written out for one (b, v, j); X is read as the fp32 joint a model returns
    b, v, j = 1, nv - 1, 2
    h = P[b, v] @ np.append(X[b, j].astype(np.float32).astype(np.float64), 1.0)
    assert np.isclose(err[b, v, j], np.linalg.norm(h[:2] / h[2] - pts[b, v, j]), rtol=1e-12)
    assert err.shape == (2, nv, 3) and (err > 0).all() and np.isfinite(err).all()


def test_masked_views_are_never_read():
    from mvn.utils import multiview
    P, pts, conf, cov2 = rig(4, seed=3)
    mask = np.array([[1, 0, 1, 1], [1, 1, 0, 1]], dtype=np.uint8)
    Pn, pn, cn, sn = P.copy(), pts.copy(), conf.copy(), cov2.copy()
    for b, v in ((0, 1), (1, 2)):
        Pn[b, v] = pn[b, v] = cn[b, v] = sn[b, v] = np.nan
    X, jac = multiview.triangulation_jacobian(Pn, pn, cn, mask)
    err, cov = multiview.triangulation_stats(Pn, pn, cn, sn, X, mask)
    assert np.isfinite(X).all() and np.isfinite(cov).all() and not jac[0, 1].any() and not jac[1, 2].any()
    for b in range(2):          # each sample is the statement on its valid views alone
        keep = np.flatnonzero(mask[b])
        Xb, jb = multiview.triangulation_jacobian(P[b:b + 1, keep], pts[b:b + 1, keep], conf[b:b + 1, keep])
        eb, cb = multiview.triangulation_stats(P[b:b + 1, keep], pts[b:b + 1, keep], conf[b:b + 1, keep], cov2[b:b + 1, keep], Xb)
        assert np.array_equal(X[b], Xb[0]) and np.array_equal(jac[b, keep], jb[0]) and np.array_equal(cov[b], cb[0])
        assert np.array_equal(err[b, keep], eb[0]) and np.isnan(err[b, np.flatnonzero(mask[b] == 0)[0]]).all()
    # one valid view: no joint, no covariance
    X1, _ = multiview.triangulation_jacobian(P, pts, conf, np.array([[1, 0, 0, 0], [1, 1, 1, 1]]))
    e1, c1 = multiview.triangulation_stats(P, pts, conf, cov2, X, np.array([[1, 0, 0, 0], [1, 1, 1, 1]]))
    assert np.isnan(X1[0]).all() and np.isnan(c1[0]).all() and np.isfinite(c1[1]).all() and np.isfinite(X1[1]).all()


def test_heatmap_stats_2d_known_answers():
    from mvn.utils import multiview
    h, w = 7, 9
    # one-hot (a softmax over logits 0 / 1000): peak 1, covariance 0
    hot = np.zeros((1, h, w), dtype=np.float32)
    hot[0, 4, 6] = 1000.0
    peak, idx, mass, cov = multiview.heatmap_stats_2d(hot, 1.0, True)
    assert peak[0] == 1.0 and idx[0] == 4 * w + 6 and mass[0] == 1.0 and not cov.any()
    # ReLU one-hot: the same, with the mass of the one value
    peak, idx, mass, cov = multiview.heatmap_stats_2d(hot, 0.5, False)
    assert peak[0] == 1.0 and idx[0] == 4 * w + 6 and mass[0] == 500.0 and not cov.any()
    # a tie goes to the lower index
    tie = np.zeros((1, h, w), dtype=np.float32)
    tie[0, 5, 2] = tie[0, 1, 3] = tie[0, 1, 8] = 2.0
    for sm in (True, False):
        assert multiview.heatmap_stats_2d(tie, 3.0, sm)[1][0] == 1 * w + 3
    # ReLU without mass: zeros
    peak, idx, mass, cov = multiview.heatmap_stats_2d(-np.abs(np.random.default_rng(0).standard_normal((2, h, w))).astype(np.float32) - 0.1, 1.0, False)
    assert not peak.any() and not mass.any() and not cov.any()
    # a separable Gaussian well inside a large map: its variances, no correlation; lead dimensions are kept
    H2, W2, sx, sy, mx, my = 48, 64, 3.0, 2.0, 30.0, 20.0
    yy, xx = np.mgrid[:H2, :W2].astype(np.float64)
    logit = (-(xx - mx) ** 2 / (2 * sx ** 2) - (yy - my) ** 2 / (2 * sy ** 2)).astype(np.float32)
    peak, idx, mass, cov = multiview.heatmap_stats_2d(np.tile(logit, (2, 3, 1, 1)), 1.0, True)
    assert cov.shape == (2, 3, 2, 2) and peak.shape == idx.shape == mass.shape == (2, 3)
    assert abs(cov[1, 2, 0, 0] - sx ** 2) < 1e-3 and abs(cov[1, 2, 1, 1] - sy ** 2) < 1e-3 and abs(cov[1, 2, 0, 1]) < 1e-6 and cov[0, 0, 0, 1] == cov[0, 0, 1, 0]
    assert idx[0, 0] == 20 * W2 + 30 and abs(peak[0, 0] - 1.0 / (2 * np.pi * sx * sy)) < 1e-4
    # in ReLU mode the same numbers from the exponentiated map, whose mass is the Gaussian's integral
    peak_r, idx_r, mass_r, cov_r = multiview.heatmap_stats_2d(np.exp(logit)[None], 1.0, False)
    assert abs(mass_r[0] - 2 * np.pi * sx * sy) < 1e-3 and np.allclose(cov_r[0], cov[0, 0], atol=1e-4) and idx_r[0] == idx[0, 0]
    # the moments are about the coordinates that are handed in
    c0 = np.array([[31.0, 20.0]], dtype=np.float32)
    assert abs(multiview.heatmap_stats_2d(logit[None], 1.0, True, coords=c0)[3][0, 0, 0] - (sx ** 2 + 1.0)) < 1e-3


def test_records_to_alg_keypoint_stats():
    from mvn.utils import op, volumetric
    assert op.AlgKeypointStats is volumetric.AlgKeypointStats
    assert op.AlgKeypointStats._fields == ("peak", "peak_index", "mass", "covariance_2d", "reprojection_error", "covariance")
    rec = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    idx = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)
    c2 = torch.arange(2 * 3 * 4 * 3, dtype=torch.float32).reshape(2, 3, 4, 3)
    err = torch.rand(2, 3, 4)
    c3 = torch.arange(2 * 4 * 6, dtype=torch.float32).reshape(2, 4, 6)
    st = op.alg_keypoint_stats_from_records(rec, idx, c2, err, c3)
    assert isinstance(st, op.AlgKeypointStats) and torch.equal(st.peak, rec[..., 0]) and torch.equal(st.mass, rec[..., 1]) and st.peak_index is idx
    assert st.reprojection_error is err and st.covariance_2d.shape == (2, 3, 4, 2, 2) and st.covariance.shape == (2, 4, 3, 3)
    assert st.covariance_2d[1, 2, 3].tolist() == [[69.0, 70.0], [70.0, 71.0]]
    assert st.covariance[1, 3].tolist() == [[42.0, 43.0, 44.0], [43.0, 45.0, 46.0], [44.0, 46.0, 47.0]]
    p, i, m, c = op.heatmap_stats_from_records(rec, idx)
    assert c[1, 2, 3].tolist() == [[117.0, 118.0], [118.0, 119.0]] and torch.equal(p, st.peak) and torch.equal(m, st.mass) and i is idx


# ---- plans --------------------------------------------------------------------------------------------------------------------------------------------
def test_flagged_plan_has_its_own_key_and_the_same_launches():
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet
    alg = AlgebraicTriangulationNet(synth.alg_config(18), device="cpu").eval()
    assert alg.keypoint_stats is False and alg.last_keypoint_stats is None
    never = alg._build_plan(2, 4, 64, 64, "cpu", dry_run=True)          # the call of a host that has never heard of the flag
    off = alg._build_plan(2, 4, 64, 64, "cpu", dry_run=True, stats=False)
    on = alg._build_plan(2, 4, 64, 64, "cpu", dry_run=True, stats=True)
    both = alg._build_plan(2, 4, 64, 64, "cpu", dry_run=True, masked=True, stats=True)
    kinds = lambda P: [meta["kind"] for _, meta in P["plan"].ops]
    for P in (off, on, both):
        assert kinds(P) == kinds(never) and P["plan"].npre == never["plan"].npre
    last = lambda P: P["plan"].ops[-1][1]
    assert "entry" not in last(never)["info"] and "entry" not in last(off)["info"] and off["kstats"] is None and never["kindex"] is None
    J = alg.backbone.final_layer.out_channels
    for P in (on, both):
        info = last(P)["info"]
        assert info["entry"] == "lt_softargmax2d_stats_fwd" and P["kstats"] is info["stats"] and P["kindex"] is info["peak_index"]
        assert tuple(info["stats"].shape) == (8, J, 5) and info["stats"].dtype == torch.float32
        assert tuple(info["peak_index"].shape) == (8, J) and info["peak_index"].dtype == torch.int32
    assert "mask" in both and "mask" not in on
    k = lambda **kw: alg._plan_key(2, 4, 64, 64, "cpu", **kw)
    assert k() == k(masked=False, stats=False) and len(k()) == 10          # the unflagged key is the tuple it was before the flag existed
    assert k(stats=True) != k() and k(masked=True, stats=True) != k(masked=True) and k(masked=True, stats=True) != k(stats=True)


def test_c_entry_points_check_their_arguments():
    lib = H.lib()
    for name in ("lt_softargmax2d_stats_fwd", "lt_alg_tail_stats_fwd", "lt_plan_set_alg_keypoint_stats", "lt_triangulate_dlt_stats"):
        assert hasattr(C.CDLL(H.LIB_PATH), name) and name in H.SIGNATURES, name
    err = lambda: lib.lt_last_error().decode()
    # heatmaps, mult, softmax, coords, probs, stats, peak_index, NJ, h, w, stream
    sa = lib.lt_softargmax2d_stats_fwd
    assert sa(1, 1.0, 1, 1, None, None, 1, 2, 8, 8, None) == ERR_INVALID and "stats" in err() and "lt_softargmax2d_stats_fwd" in err()
    assert sa(1, 1.0, 1, 1, None, 1, None, 2, 8, 8, None) == ERR_INVALID and "peak_index" in err()
    assert sa(None, 1.0, 1, 1, None, 1, 1, 2, 8, 8, None) == ERR_INVALID and "heatmaps" in err()
    assert sa(1, 1.0, 1, None, None, 1, 1, 2, 8, 8, None) == ERR_INVALID and "coords" in err()
    for nj, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, -1)):
        assert sa(1, 1.0, 1, 1, None, 1, 1, nj, h, w, None) == ERR_INVALID and "shape" in err()
    assert sa(1, 1.0, 1, 1, None, 1, 1, 2, 1 << 16, 1 << 15, None) == ERR_UNSUPPORTED and "int32" in err()
    # keypoints_hm, conf_raw, ld_conf, proj, scale_x, scale_y, view_mask, stats2d, keypoints_2d, confidences, keypoints_3d, cov2d_img, reproj_err, cov3d, B, NV, J, stream
    tail = lambda stats2d=1, cov2d=1, reproj=1, cov3d=1, nv=4, kp3d=1: lib.lt_alg_tail_stats_fwd(1, None, 17, 1, 4.0, 4.0, None, stats2d, None, None, kp3d, cov2d, reproj,
                                                                                                  cov3d, 2, nv, 17, None)
    assert tail(stats2d=None) == ERR_INVALID and "stats2d" in err() and "lt_alg_tail_stats_fwd" in err()
    assert tail(cov2d=None) == ERR_INVALID and "cov2d_img" in err()
    assert tail(reproj=None) == ERR_INVALID and "reproj_err" in err()
    assert tail(cov3d=None) == ERR_INVALID and "cov3d" in err()
    assert tail(nv=1) == ERR_INVALID and "NV 1" in err()          # as lt_alg_tail_fwd
    assert lib.lt_alg_tail_fwd(1, None, 17, 1, 4.0, 4.0, None, None, 1, 2, 1, 17, None) == ERR_INVALID and "NV 1" in err()
    assert tail(kp3d=None) == ERR_INVALID
    assert lib.lt_alg_tail_stats_fwd(1, 1, 16, 1, 4.0, 4.0, None, 1, None, None, 1, 1, 1, 1, 2, 4, 17, None) == ERR_INVALID and "ld_conf" in err()
    # proj, points, conf, cov2d, view_mask, out, reproj_err, cov3d, B, NV, J, stream
    dlt = lib.lt_triangulate_dlt_stats
    assert dlt(1, 1, None, None, None, 1, 1, 1, 2, 4, 17, None) == ERR_INVALID and "cov2d" in err()
    assert dlt(1, 1, None, 1, None, 1, None, 1, 2, 4, 17, None) == ERR_INVALID and "reproj_err" in err()
    assert dlt(1, 1, None, 1, None, 1, 1, None, 2, 4, 17, None) == ERR_INVALID and "cov3d" in err()
    assert dlt(1, 1, None, 1, None, 1, 1, 1, 2, 1, 17, None) == ERR_INVALID and "NV 1" in err()
    assert lib.lt_plan_set_alg_keypoint_stats(None, None, None, None, None, None) == ERR_INVALID and "null plan" in err()
    assert lib.lt_plan_set_alg_keypoint_stats(None, 1, 1, 1, 1, 1) == ERR_INVALID and "null plan" in err()
