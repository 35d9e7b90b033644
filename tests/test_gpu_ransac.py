"""RANSACTriangulationNet on the GPU: lt_heatmap_argmax_nchw_f32 against torch.max on the CPU, lt_triangulate_ransac against the
reference's triangulate_ransac (tests/golden/ransac_ops.npz: replayed random draws and the exhaustive pair schedule), and the whole
model against the reference model (tests/golden/ransac_net.npz).  Fixtures: tools/make_golden_ransac.py."""
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import check, record, rel_err
from oracle import spec, synth
from ransac_ref import huber_cost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(nv, d) for nv in (2, 3, 4, 8) for d in (0, 1)]


def _argmax_case(N, J, h, w, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, h, w, ld, generator=g)
    x = torch.round(x * 4) / 4                     # plenty of exact ties
    for n in range(N):                             # planted ties at the maximum, planted NaNs (two in one map: the first wins)
        j = n % J
        for p in (h * w - 1, 5):
            x[n, p // w, p % w, j] = 100.0
        if n % 3 == 0:
            for p in (h * w // 2, 7):
                x[n, p // w, p % w, (n + 1) % J] = float("nan")
    xd = x.to(DEV)
    y = torch.empty(N, J, h, w, device=DEV)
    idx = torch.empty(N, J, dtype=torch.int64, device=DEV)
    kp = torch.empty(N, J, 2, dtype=torch.int64, device=DEV)
    Hi, Wi = 4 * h, 4 * w + 3                       # a non-integer ratio on x
    H.check(H.lib().lt_heatmap_argmax_nchw_f32(xd.data_ptr(), ld, y.data_ptr(), idx.data_ptr(), kp.data_ptr(), N, J, h, w, Hi, Wi,
                                               H.cur_stream()), "lt_heatmap_argmax_nchw_f32")
    y2 = torch.empty_like(y)
    H.check(H.lib().lt_nhwc_to_nchw_f32(H.LT_F32, xd.data_ptr(), y2.data_ptr(), N, J, h * w, ld, H.cur_stream()), "lt_nhwc_to_nchw_f32")
    torch.cuda.synchronize()
    ref_hm = x[..., :J].permute(0, 3, 1, 2).contiguous()
    _, ref_idx = torch.max(ref_hm.view(N, J, -1), -1)
    kx = ref_idx % w
    ky = ref_idx // w
    ref_kp = torch.zeros(N, J, 2, dtype=torch.int64)      # reference triangulation.py:49-51
    ref_kp[..., 0] = kx * (Wi / w)
    ref_kp[..., 1] = ky * (Hi / h)
    assert torch.equal(y.cpu().view(torch.int32), y2.cpu().view(torch.int32))
    assert torch.equal(y.cpu().view(torch.int32), ref_hm.view(torch.int32))
    assert torch.equal(idx.cpu(), ref_idx), (idx.cpu() != ref_idx).sum()
    assert torch.equal(kp.cpu(), ref_kp)


@pytest.mark.parametrize("N,J,h,w,ld", [(8, 17, 96, 96, 17), (6, 17, 32, 32, 17), (5, 13, 96, 96, 13), (4, 13, 32, 32, 16), (3, 21, 31, 29, 21)])
def test_heatmap_argmax_matches_torch_max(N, J, h, w, ld):
    _argmax_case(N, J, h, w, ld, seed=N * 1000 + J * 10 + h)


def _ransac(g, tag, mode, direct):
    P = torch.from_numpy(g[tag + "_P"]).to(DEV)
    pts = torch.from_numpy(g[tag + "_pts"]).to(DEV)
    pairs = torch.from_numpy(g["%s_%s_draws" % (tag, mode)]) if mode == "replay" else None
    from mvn.utils import multiview
    kp, inl = multiview.triangulate_ransac_batch(P, pts, pairs, 15, direct, return_inliers=True)
    return kp.cpu().double().numpy(), inl.cpu().numpy()


def _check_ransac(name, P, pts, kp_pre, kp, inl, pre, post, ref_inl, cost, well, direct, skip=None):
    B, J = kp.shape[:2]
    ok = np.ones((B, J), bool) if skip is None else ~skip
    assert np.array_equal(inl[ok], ref_inl[ok].astype(bool)), "%s: inlier sets differ at %s" % (name, np.argwhere((inl != ref_inl.astype(bool)).any(-1) & ok))
    check(name + "/pre-refinement points", kp_pre[ok], pre[ok], 1e-6)
    if not direct:
        check(name + "/points", kp[ok], post[ok], 1e-6)
        return
    wp = ok & well
    check(name + "/refined points (well posed: %d of %d)" % (wp.sum(), ok.sum()), kp[wp], post[wp], 1e-4)
    # Huber cost at the fp32 point we return vs scipy's final cost.  Gated on the well-posed problems.  The others are recorded: on a
    # 2-view inlier set whose residuals are all in Huber's linear regime (a sum of distances, r_v > 100 px on the outlier pairs of
    # these fixtures) the objective is multimodal -- minima near a camera centre, in a valley towards a vanishing point -- and the
    # basin scipy's trust region reaches from the DLT point is not always the one this kernel reaches.
    worst, above = -np.inf, []
    for b in range(B):
        for j in range(J):
            if not ok[b, j]:
                continue
            ours = huber_cost(P[b], pts[b, :, j], kp[b, j], inl[b, j])
            if ours > cost[b, j] * (1 + 1e-6) + 1e-9:
                assert not well[b, j], (name, b, j, ours, cost[b, j])
                above.append([int(b), int(j), float(ours), float(cost[b, j])])
            elif well[b, j]:
                worst = max(worst, (ours - cost[b, j]) / max(cost[b, j], 1e-30))
    record(name + "/Huber cost (ours - scipy) / scipy, max over well-posed", worst)
    record(name + "/Huber cost above scipy's (not well posed): [b, j, ours, scipy]", above)


@pytest.mark.parametrize("nv,direct", CASES)
@pytest.mark.parametrize("mode", ["replay", "exh"])
def test_ransac_kernel_vs_reference(golden_dir, nv, direct, mode):
    """mode replay: the reference's own random draws replayed through the pair schedule; mode exh: the default exhaustive schedule
    (pairs = NULL) against the reference run with every pair in lexicographic order."""
    g = np.load(os.path.join(golden_dir, "ransac_ops.npz"))
    tag = "nv%d_d%d" % (nv, direct)
    kp_pre, _ = _ransac(g, tag, mode, False)
    kp, inl = _ransac(g, tag, mode, bool(direct))
    r = lambda k: g["%s_%s_%s" % (tag, mode, k)]  # noqa: E731
    _check_ransac("ransac/%s/%s" % (tag, mode), g[tag + "_P"], g[tag + "_pts"], kp_pre, kp, inl, r("pre"), r("post"), r("inl"),
                  r("cost"), r("well"), direct)


@pytest.mark.parametrize("nv", [2, 3, 8])
def test_ransac_with_every_view_an_inlier_equals_the_dlt_kernel_bit_for_bit(nv):
    """Both kernels solve through the one routine of csrc/dlt.h: with eps = 1e30 every view is an inlier of every hypothesis, the final
    DLT of lt_triangulate_ransac (no refinement) is over all views with weight 1, and lt_triangulate_dlt on the same points as fp32
    without confidences is the same system -- the same bits."""
    from mvn.utils import multiview
    B, J = 3, 5
    K, R, t = synth.ring_cameras(nv, 384)
    P = torch.from_numpy((K @ np.concatenate([R, t], -1)).astype(np.float32))[None].repeat(B, 1, 1, 1).to(DEV)
    pts = torch.from_numpy(np.random.RandomState(29).randint(0, 384, (B, nv, J, 2)).astype(np.int64)).to(DEV)
    kp, inl = multiview.triangulate_ransac_batch(P, pts, None, 1e30, False, return_inliers=True)
    assert inl.all()
    ref = multiview.triangulate_batch_of_points(P, pts.float())
    assert torch.isfinite(ref).all()
    assert torch.equal(kp, ref)


def _net(direct=True):
    from mvn.models.triangulation import RANSACTriangulationNet
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "experiments_human36m.json")) as f:
        y = json.load(f)["eval/human36m_ransac.yaml"]
    cfg = synth.AttrDict({"model": y["model"]})
    cfg.model.backbone.update({"name": "resnet18", "num_layers": 18, "init_weights": False, "checkpoint": ""})
    cfg.model.direct_optimization = direct
    m = RANSACTriangulationNet(cfg, device=DEV)
    m.load_state_dict(synth.make_state_dict(spec.alg_net_spec(18, 17, False), seed=61, basic_block=True), strict=True)
    return m.eval()


def test_ransac_net_vs_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "ransac_net.npz"))
    m = _net()
    inp = synth.make_inputs(2, 4, 128, seed=13)
    P = torch.from_numpy(g["P"])
    with torch.no_grad():
        kp3, kp2, hm, conf = m(inp["images"].to(DEV), P.to(DEV), {})
        out2 = m(inp["images"].to(DEV), P.to(DEV), {})
    assert kp3.dtype == torch.float32 and kp3.shape == (2, 17, 3)
    assert kp2.dtype == torch.int64 and kp2.shape == (2, 4, 17, 2)
    assert hm.dtype == torch.float32 and hm.shape == (2, 4, 17, 32, 32)
    assert conf.dtype == torch.float32 and conf.shape == (2, 4, 17) and not conf.any()
    for a, b in zip((kp3, kp2, hm, conf), out2):
        assert torch.equal(a, b)                          # two forwards: bitwise identical
    tol = 2e-3                                            # what the algebraic model's heatmaps are held to
    check("ransac-net/raw heatmaps", hm.cpu().reshape(8, 17, 32, 32)[:, :, ::2, ::2], g["hm_sub"], tol)
    # an argmax can only move where the reference's top-1 / top-2 gap is within twice the heatmap tolerance
    sure = g["margin"] > 2 * tol * float(g["hm_absmax"])
    record("ransac-net/keypoints_2d entries excluded (top-2 margin <= 2 tol max|hm|)", int((~sure).sum()))
    k2 = kp2.cpu().numpy()
    assert np.array_equal(k2[sure], g["kp2"][sure]), np.argwhere((k2 != g["kp2"]).any(-1) & sure)
    # the batched RANSAC on the reference's 2D keypoints with its logged draws reproduces the reference's 3D keypoints
    from mvn.utils import multiview
    kpd = torch.from_numpy(g["kp2"]).to(DEV)
    kr, inl = multiview.triangulate_ransac_batch(P.to(DEV), kpd, torch.from_numpy(g["pairs"]), 15, True, return_inliers=True)
    kr_pre = multiview.triangulate_ransac_batch(P.to(DEV), kpd, torch.from_numpy(g["pairs"]), 15, False)
    kr, kr_pre, inl = kr.cpu().double().numpy(), kr_pre.cpu().double().numpy(), inl.cpu().numpy()
    skip = g["eps_margin"] < 1e-6
    record("ransac-net/problems with an error within 1e-6 of eps (not gated)", int(skip.sum()))
    _check_ransac("ransac-net/replayed draws", g["P"], g["kp2"], kr_pre, kr, inl, g["replay_pre"], g["replay_post"], g["replay_inl"],
                  g["replay_cost"], g["replay_well"], True, skip=skip)
    record("ransac-net/keypoints_3d end-to-end deviation (random init: views disagree)", rel_err(kp3.cpu(), g["kp3"]))
    assert torch.isfinite(kp3).all()


def test_ransac_net_single_point_method_and_train_mode(golden_dir):
    g = np.load(os.path.join(golden_dir, "ransac_ops.npz"))
    m = _net()
    P, pts = g["nv4_d1_P"][0], g["nv4_d1_pts"][0, :, 3]
    X, inl = m.triangulate_ransac(P, pts, n_iters=10, reprojection_error_epsilon=15, direct_optimization=True)
    assert X.shape == (3,) and list(inl) == list(np.nonzero(g["nv4_d1_exh_inl"][0, 3])[0])
    assert huber_cost(P, pts, X, g["nv4_d1_exh_inl"][0, 3]) <= g["nv4_d1_exh_cost"][0, 3] * (1 + 1e-6) + 1e-9
    m.train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 2, 3, 64, 64, device=DEV), torch.zeros(1, 2, 3, 4, device=DEV), {})
