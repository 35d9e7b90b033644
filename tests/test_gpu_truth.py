"""GPU (-m gpu): the fp32 kernel mode against fp64 GROUND TRUTH (tests/golden/truth_*.npz, oracle/truth.py), not against the reference's fp32
outputs, which carry rounding errors of their own (stored beside the truth as ref32_err/<key>, measured when the files were generated).

One rule for every quantity q, no per-fixture constants:  err_ours(q) <= max(2 * ref32_err(q), floor(q)) -- at least comparably accurate to the
reference, both measured against the exact answer -- and, where the suite already holds q to the reference, also <= that tolerance.

The DLT kernels are held to an exact SVD on problem families built here (well posed, narrow baseline, inconsistent views, far points, confidences
down to 1e-5), with a bound derived from what fp32 rounding of the rows can explain."""
import math
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import check, record
from oracle import spec, synth
from oracle import truth as T
from oracle import vol_oracle as O
from test_gpu_models import BF16_GATES, DEV, _run_vol, _sub
from test_oracle_golden import VOL_CASES, build_vol_case

pytestmark = pytest.mark.gpu

# floors: joints at the north star's 1e-4; conv outputs (features, heatmaps, V2V logits) and the unprojected volume at 2e-6;
# softmaxed / sigmoid outputs (volumes, heatmaps after the 2D softmax, confidences, 2D keypoints) at 1e-5
FLOOR = {"kp": 1e-4, "kp_norm": 1e-4, "feat_sub": 2e-6, "unproj_sub": 2e-6, "logits_sub": 2e-6, "vol_sub": 1e-5, "vol_conf": 1e-5,
         "feat_s2": 2e-6, "hm": 2e-6, "algc": 1e-5, "volc": 1e-5, "kp2": 1e-5, "conf": 1e-5, "hm_sub": 1e-5}
# what tests/test_gpu_models.py already asserts against the reference: the truth gates are never looser
TODAY = {"feat_sub": 2e-5, "logits_sub": 2e-5, "vol_sub": 1e-4, "vol_conf": 1e-4, "feat_s2": 1e-4, "hm": 1e-4, "algc": 1e-4, "volc": 1e-4,
         "kp2": 1e-4}


def _truth(golden_dir, name):
    return np.load(os.path.join(golden_dir, "truth_%s.npz" % name))


def gate(name, floor_key, ours, ref32, today_key=None):
    eff = max(2.0 * ref32, FLOOR[floor_key])
    today = TODAY.get(today_key or floor_key)
    record(name + " vs fp64 truth", {"err_ours": ours, "ref32_err": ref32, "ratio": ours / max(ref32, 1e-300), "gate": eff, "today_vs_reference": today})
    assert ours <= eff, "%s: err %.3e > max(2 x reference's %.3e, floor %.1e)" % (name, ours, ref32, FLOOR[floor_key])
    if today is not None:
        assert ours <= today, "%s: err %.3e > the suite's tolerance against the reference %.1e" % (name, ours, today)


# ---- volumetric fixtures ------------------------------------------------------------------------------------------------------------------
def _unprojected(m):
    """The plan's unprojected volume (B, 32, V, V, V).  V2V hands that buffer back to the pool after its first layer, so the recorded
    unprojection launch is replayed once more on the plan's (kept) features and geometry."""
    P = list(m._plans.values())[0]
    ops = [fn for fn, meta in P["plan"].ops if meta["label"] == "unproject"]
    assert len(ops) == 1
    ops[0](H.cur_stream())
    torch.cuda.synchronize()
    return P["vol"].t.permute(0, 4, 1, 2, 3).float().cpu()


@pytest.mark.parametrize("tag", list(VOL_CASES))
def test_volumetric_fp32_vs_truth(golden_dir, tag):
    t = _truth(golden_dir, tag)
    cfg, sd, inp, c = build_vol_case(tag)
    assert np.allclose(synth.state_dict_checksum(sd), t["sd_digest"], rtol=1e-12)
    assert np.allclose(T.images_digest(inp["images"]), t["images_digest"], rtol=1e-12)
    m, (kp, feats, vols, conf, _, _, _), _, c, _ = _run_vol(tag, torch.float32)
    s = int(t["stride"])
    B, NV = c["B"], c["NV"]
    err = lambda k: float(t["ref32_err/" + k])
    P = list(m._plans.values())[0]
    logits = P["logits"].t.permute(0, 4, 1, 2, 3).float().cpu()
    kp = kp.cpu().double().numpy()
    if c["volume_softmax"]:
        gate(tag + "/joints fp32 (max rel, 1 mm floor)", "kp", T.joints_rel(kp, t["kp"]), err("kp"))
    else:   # ReLU volumes: unnormalised sums whose components cancel to different degrees -- element-wise and norm-wise
        gate(tag + "/joints fp32 (element-wise max rel, 1 mm floor)", "kp", T.joints_rel(kp, t["kp"]), err("kp"))
        gate(tag + "/joints fp32 (norm-wise)", "kp_norm", T.joints_norm_rel(kp, t["kp"]), err("kp_norm"))
    gate(tag + "/features fp32", "feat_sub", T.max_rel(_sub(feats.cpu().reshape(B * NV, *feats.shape[2:]), s).numpy(), t["feat_sub"]), err("feat_sub"))
    gate(tag + "/v2v logits fp32", "logits_sub", T.max_rel(_sub(logits, s).numpy(), t["logits_sub"]), err("logits_sub"))
    gate(tag + "/volumes (softmaxed) fp32", "vol_sub", T.max_rel(_sub(vols.cpu(), s).numpy(), t["vol_sub"]), err("vol_sub"))
    if conf is not None:
        gate(tag + "/vol_confidences fp32", "vol_conf", T.max_rel(conf.cpu().numpy(), t["vol_conf"]), err("vol_conf"))
    gate(tag + "/unprojected volume fp32", "unproj_sub", T.max_rel(_sub(_unprojected(m), s).numpy(), t["unproj_sub"]), err("unproj_sub"))
    del m
    if tag in BF16_GATES:           # bf16 throughput mode: its deviation from the truth, recorded (its gates stay in test_gpu_models.py)
        m, (kp16, f16, v16, _, _, _, _), _, _, _ = _run_vol(tag, torch.bfloat16)
        d = kp16.cpu().double().numpy() - t["kp"]
        lg16 = list(m._plans.values())[0]["logits"].t.permute(0, 4, 1, 2, 3).float().cpu()
        record(tag + "/bf16 vs fp64 truth", {
            "joints MPJPE mm": float(np.sqrt((d ** 2).sum(-1)).mean()), "joints max abs mm": float(np.abs(d).max()),
            "joints max rel (1 mm floor)": T.joints_rel(kp16.cpu().numpy(), t["kp"]),
            "features": T.max_rel(_sub(f16.cpu().reshape(B * NV, *f16.shape[2:]), s).numpy(), t["feat_sub"]),
            "logits": T.max_rel(_sub(lg16, s).numpy(), t["logits_sub"]), "volumes": T.max_rel(_sub(v16.cpu(), s).numpy(), t["vol_sub"])})
        del m
    torch.cuda.empty_cache()


# ---- backbones (nets.npz) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,hw,conf", list(T.NETS))
def test_pose_resnet_fp32_vs_truth(golden_dir, nl, hw, conf):
    from mvn.models import pose_resnet
    t = _truth(golden_dir, "nets")
    gen = torch.Generator().manual_seed(9)
    torch.randn(1, 32, 32, 32, 32, generator=gen)      # oracle/make_golden.py gen_nets' draw order
    for n2, h2, _ in T.NETS:
        x = torch.randn(2, 3, h2, h2, generator=gen)
        if n2 == nl:
            break
    assert np.allclose(T.images_digest(x), t["rn%d_images_digest" % nl], rtol=1e-12)
    cfg = synth.AttrDict(num_layers=nl, style="simple", num_joints=17, alg_confidences=conf, vol_confidences=conf, init_weights=False, checkpoint="")
    m = pose_resnet.get_pose_net(cfg, device=DEV)
    sd = synth.make_state_dict(spec.pose_resnet_spec(nl, 17, conf, conf, ""), seed=nl, basic_block=(nl < 50))
    assert np.allclose(synth.state_dict_checksum(sd), t["rn%d_sd_digest" % nl], rtol=1e-12)
    m.load_state_dict(sd, strict=True)
    m.eval()
    hm, ft, ac, vc = m(x.to(DEV))
    k = lambda q: "rn%d_%s" % (nl, q)
    gate("resnet%d/features fp32" % nl, "feat_s2", T.max_rel(_sub(ft.cpu(), 2).numpy(), t[k("feat_s2")]), float(t["ref32_err/" + k("feat_s2")]))
    gate("resnet%d/heatmaps fp32" % nl, "hm", T.max_rel(hm.cpu().numpy(), t[k("hm")]), float(t["ref32_err/" + k("hm")]))
    if conf:
        gate("resnet%d/alg_confidences fp32" % nl, "algc", T.max_rel(ac.cpu().numpy(), t[k("algc")]), float(t["ref32_err/" + k("algc")]))
        gate("resnet%d/vol_confidences fp32" % nl, "volc", T.max_rel(vc.cpu().numpy(), t[k("volc")]), float(t["ref32_err/" + k("volc")]))


# ---- DLT: exact SVD and the rounding bound ----------------------------------------------------------------------------------------------
def dlt_rows64(P, pts, conf):
    """A (B, J, 2 NV, 4) in fp64 from the fp32 inputs, the reference's rows c (x P[2,:] - P[r,:]) (multiview.py:159-161)."""
    P, p = P.astype(np.float64), pts.astype(np.float64)
    A = P[:, :, None, 2:3, :] * p[..., :, None] - P[:, :, None, :2, :]
    if conf is not None:
        A = A * conf.astype(np.float64)[..., None, None]
    return A.transpose(0, 2, 1, 3, 4).reshape(A.shape[0], A.shape[2], -1, 4)


def _svd_point(A):
    _, sv, vh = np.linalg.svd(A)
    v = vh[..., 3, :]
    return v[..., :3] / v[..., 3:4], sv


def dlt_truth(P, pts, conf, draws=8, seed=0):
    """(X, s, sigma): the exact DLT point (fp64 SVD of the fp64 rows), s = the largest displacement of it over ``draws`` perturbations of
    every entry of A by an independent relative +-2^-24 (what fp32 rounding of the rows can explain), and A's singular values."""
    A = dlt_rows64(P, pts, conf)
    X, sv = _svd_point(A)
    rs = np.random.RandomState(seed)
    s = np.zeros(X.shape[:2])
    for _ in range(draws):
        X2, _ = _svd_point(A * (1.0 + rs.choice([-1.0, 1.0], A.shape) * 2.0 ** -24))
        s = np.maximum(s, np.linalg.norm(X2 - X, axis=-1))
    return X, s, sv


def dlt_gate(name, ours, X, s, sv):
    """Per point:  |ours - truth| <= 4 s + 1e-6 max(|truth|, 1 mm).  Records the worst err / s and err / bound."""
    err = np.linalg.norm(np.asarray(ours, np.float64) - X, axis=-1)
    bound = 4.0 * s + 1e-6 * np.maximum(np.linalg.norm(X, axis=-1), 1.0)
    worst = int(np.argmax(err / bound))
    record(name + " vs exact SVD", {"worst err/s": float((err / np.maximum(s, 1e-300)).max()), "worst err/bound": float((err / bound).max()),
                                     "kappa max": float((sv[..., 0] / sv[..., 3]).max()), "sigma3/sigma4 min": float((sv[..., 2] / sv[..., 3]).min()),
                                     "|X| max": float(np.linalg.norm(X, axis=-1).max())})
    assert (err <= bound).all(), "%s: %d of %d points outside 4 s + 1e-6 |X|; worst err %.3e, s %.3e, |X| %.3e, kappa %.2e" % (
        name, int((err > bound).sum()), err.size, err.flat[worst], s.flat[worst], np.linalg.norm(X, axis=-1).flat[worst],
        (sv[..., 0] / sv[..., 3]).flat[worst])


def _look_at(C, image_size):
    """P = K [R | t] of a synth.ring_cameras-style camera at C looking at the origin."""
    C = np.asarray(C, np.float64)
    fwd = -C / np.linalg.norm(C)
    right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    f = 1.2 * image_size
    K = np.array([[f, 0.0, image_size / 2.0], [0.0, f, image_size / 2.0], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, (-R @ C).reshape(3, 1)], 1)


def _project(P, X):
    p = np.einsum("vik,bjk->bvji", P, np.concatenate([X, np.ones(X.shape[:-1] + (1,))], -1))
    return p[..., :2] / p[..., 2:3]


DLT_FAMILIES = (["well_nv%d_px%g" % (nv, n) for nv in (2, 3, 4, 8, 16) for n in (0, 0.5, 5)]
                + ["narrow_baseline_1deg", "inconsistent_views", "far_points", "conf_1e-5_to_1", "conf_one_view_1e-5", "conf_all_equal"])


def dlt_family(name, B=16, J=16):
    """(P (B,NV,3,4), points (B,NV,J,2), confidences (B,NV,J)) fp32 -- B x J = 256 DLT problems; 384^2 images, skeletons of +-300 mm at the
    origin seen from a 4 m ring (synth.ring_cameras) unless the family says otherwise."""
    rs = np.random.RandomState(sum(map(ord, name)))
    NV, noise, Ps = 4, 0.5, None
    X = rs.randn(B, J, 3) * 300.0
    if name.startswith("well"):
        nv, px = name.split("_")[1:]
        NV, noise = int(nv[2:]), float(px[2:])
    elif name == "narrow_baseline_1deg":          # two cameras 1 degree apart on the ring
        NV, Ps = 2, np.stack([_look_at([4000.0 * math.cos(a), 4000.0 * math.sin(a), 1000.0], 384) for a in (0.0, math.radians(1.0))])
    elif name == "far_points":                     # |X| from 1e4 to 1e5 mm, log-uniform
        d = rs.randn(B, J, 3)
        X = d / np.linalg.norm(d, axis=-1, keepdims=True) * np.exp(rs.uniform(math.log(1e4), math.log(1e5), (B, J, 1)))
    if Ps is None:
        K, R, t = synth.ring_cameras(NV, 384)
        Ps = K @ np.concatenate([R, t], -1)
    if name == "inconsistent_views":               # every view sees a different point, as at random init: sigma3 / sigma4 ~ 1.0-1.3
        pts = np.concatenate([_project(Ps[v:v + 1], rs.randn(B, J, 3) * 300.0) for v in range(NV)], 1)
    else:
        pts = _project(Ps, X) + rs.randn(B, NV, J, 2) * noise
    if name == "conf_1e-5_to_1":
        conf = np.exp(rs.uniform(math.log(1e-5), 0.0, (B, NV, J)))
    elif name == "conf_one_view_1e-5":
        conf = np.ones((B, NV, J)); conf[:, 0] = 1e-5
    elif name == "conf_all_equal":
        conf = np.full((B, NV, J), 1.0 / NV + 1e-5)
    else:
        conf = rs.uniform(0.2, 1.2, (B, NV, J))
    return (np.ascontiguousarray(np.broadcast_to(Ps, (B,) + Ps.shape)).astype(np.float32), pts.astype(np.float32), conf.astype(np.float32))


@pytest.mark.parametrize("fam", DLT_FAMILIES)
def test_dlt_kernels_vs_exact_svd(fam):
    """lt_triangulate_dlt and lt_alg_tail_fwd (fed the equivalent heatmap keypoints and scale) against the fp64 SVD, at the bound above;
    lt_triangulate_dlt_bwd against fp64 autograd through the oracle's triangulate_batch_of_points at the suite's 2e-3 -- except where
    sigma3 / sigma4 < 1.01, whose gradient carries 1 / (lambda3 - lambda4) (recorded there)."""
    from mvn.utils import multiview
    P, pts, conf = dlt_family(fam)
    B, NV, J = pts.shape[:3]
    X, s, sv = dlt_truth(P, pts, conf)
    Pd, ptd, cd = (torch.from_numpy(a).to(DEV) for a in (P, pts, conf))
    dlt_gate("dlt/%s lt_triangulate_dlt" % fam, multiview.triangulate_batch_of_points(Pd, ptd, cd).cpu().numpy(), X, s, sv)
    # algebraic tail: heatmap keypoints x 4 (exact) are the same pixels; its confidences are raw / sum over views + 1e-5
    kp_hm = (ptd / 4.0).contiguous()
    kp2d, c_out, kp3 = torch.empty_like(ptd), torch.empty_like(cd), torch.empty(B, J, 3, device=DEV)
    H.check(H.lib().lt_alg_tail_fwd(kp_hm.data_ptr(), cd.data_ptr(), J, Pd.data_ptr(), 4.0, 4.0, kp2d.data_ptr(), c_out.data_ptr(), kp3.data_ptr(),
                                    B, NV, J, H.cur_stream()), "lt_alg_tail_fwd")
    assert torch.equal(kp2d, ptd)
    Xa, sa, sva = dlt_truth(P, kp2d.cpu().numpy(), c_out.cpu().numpy())
    dlt_gate("dlt/%s lt_alg_tail_fwd" % fam, kp3.cpu().numpy(), Xa, sa, sva)
    # backward
    GX = torch.from_numpy(np.random.RandomState(5).randn(B, J, 3)).float()
    p64 = torch.from_numpy(pts).double().requires_grad_(True)
    c64 = torch.from_numpy(conf).double().requires_grad_(True)
    (O.triangulate_batch_of_points(torch.from_numpy(P), p64, c64, dtype=torch.float64) * GX.double()).sum().backward()
    pg, cg = ptd.clone().requires_grad_(True), cd.clone().requires_grad_(True)
    (multiview.triangulate_batch_of_points(Pd, pg, cg) * GX.to(DEV)).sum().backward()
    ok = torch.from_numpy(sv[..., 2] / sv[..., 3] >= 1.01)                 # (B, J)
    gp, gc = pg.grad.cpu().double(), cg.grad.cpu().double()
    okp, okc = ok[:, None, :, None].expand_as(gp), ok[:, None, :].expand_as(gc)
    if (~ok).any():
        record("dlt/%s backward where sigma3/sigma4 < 1.01 (%d points, recorded)" % (fam, int((~ok).sum())), {
            "d/d points": float((gp - p64.grad)[~okp].abs().max() / p64.grad[~okp].abs().max()),
            "d/d confidences": float((gc - c64.grad)[~okc].abs().max() / c64.grad[~okc].abs().max())})
    if ok.any():
        check("dlt/%s backward d/d points" % fam, torch.where(okp, gp, 0.0), torch.where(okp, p64.grad, 0.0), 2e-3)
        check("dlt/%s backward d/d confidences" % fam, torch.where(okc, gc, 0.0), torch.where(okc, c64.grad, 0.0), 2e-3)


# ---- algebraic fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.ALG_CASES))
def test_algebraic_fp32_vs_truth(golden_dir, name):
    from mvn.models.triangulation import AlgebraicTriangulationNet
    from mvn.utils import multiview
    t = _truth(golden_dir, name)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg, sd, inp, P = T.alg_setup(name)
    assert np.allclose(synth.state_dict_checksum(sd), t["sd_digest"], rtol=1e-12)
    m = AlgebraicTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    kp3, kp2, hm, conf = m(inp["images"].to(DEV), P.to(DEV), {})
    B, NV, J, h, w = hm.shape
    s = 4 if name == "alg_c1" else 2
    err = lambda k: float(t["ref32_err/" + k])
    gate(name + "/keypoints_2d fp32 (max rel, 1 px floor)", "kp2", T.joints_rel(kp2.cpu().numpy(), t["kp2"]), err("kp2"))
    gate(name + "/confidences fp32", "conf", T.max_rel(conf.cpu().numpy(), t["conf"]), err("conf"))
    gate(name + "/heatmaps fp32", "hm_sub", T.max_rel(_sub(hm.cpu().reshape(B * NV, J, h, w), s).numpy(), t["hm_sub"]), err("hm_sub"))
    record(name + "/keypoints_3d end to end vs fp64 truth (ill-conditioned at random init), recorded",
           {"err_ours": T.joints_rel(kp3.cpu().numpy(), t["kp3"]), "ref32_err": err("kp3")})
    # the DLT kernel on the reference's 2D keypoints and confidences: the exact-SVD bound (the truth file's kp3_of_ref2d is that exact SVD)
    X, sdisp, sv = dlt_truth(P.numpy(), g["kp2"], g["conf"])
    assert np.allclose(X, t["kp3_of_ref2d"], rtol=1e-6, atol=1e-6)
    k3 = multiview.triangulate_batch_of_points(P.to(DEV), torch.from_numpy(g["kp2"]).to(DEV), torch.from_numpy(g["conf"]).to(DEV))
    dlt_gate(name + "/lt_triangulate_dlt on the reference's 2D keypoints", k3.cpu().numpy(), X, sdisp, sv)
    record(name + "/reference's fp32 torch.svd vs the exact DLT of its own 2D keypoints (max rel, 1 mm floor)", err("kp3_of_ref2d"))
