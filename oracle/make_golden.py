"""TEST INFRASTRUCTURE (see oracle/__init__.py).

Generates tests/golden/*.npz by RUNNING THE REFERENCE ITSELF (/root/reference, CPU, fp32) on the
deterministic synthetic weights/inputs of oracle/synth.py, and asserts on the way that the oracle
restatement (oracle/vol_oracle.py) reproduces every reference output.  Run in the build container:

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden

The fixtures hold REFERENCE outputs (not oracle outputs); big tensors are stored as strided
sub-samples (the stride is stored too).  Inputs/weights are regenerated from seeds at test time.

    python -m oracle.make_golden truth [vol_<tag> | alg_c1 | alg_relu_noconf | nets ...]

writes the fp64 ground truth beside those fixtures (tests/golden/truth_*.npz, oracle/truth.py); it reads
only tests/golden and the oracle, and leaves the fp32 fixtures alone.
"""
import json
import os
import sys
import time
import zipfile

import numpy as np
import torch

from . import ref_loader, spec, synth
from . import truth as T
from . import vol_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def _maxrel(a, b):
    a = a.double(); b = b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _check(name, ours, ref, tol):
    e = _maxrel(torch.as_tensor(ours), torch.as_tensor(ref))
    print("  oracle-vs-reference %-28s max|d|/max|ref| = %.3e (tol %.1e)" % (name, e, tol))
    assert e <= tol, (name, e)
    return e


def _cameras(mvn, K, R, t, B):
    """batch['cameras']: list[NV] of list[B] of reference Camera objects (datasets/utils.py:26)."""
    Cam = mvn.utils.multiview.Camera
    return [[Cam(R[v], t[v], K[v]) for _ in range(B)] for v in range(K.shape[0])]


def sub(t, stride):
    """Strided sub-sample over the trailing spatial dims of a (N, C, spatial...) tensor."""
    sl = (slice(None), slice(None)) + tuple(slice(None, None, stride) for _ in range(t.dim() - 2))
    return t[sl].contiguous().numpy()


def gen_ops(mvn):
    op, mv, vol = mvn.utils.op, mvn.utils.multiview, mvn.utils.volumetric
    out = {}
    g = torch.Generator().manual_seed(5)
    # --- unprojection: non-square heatmaps (exercises the h/w swap), camera 0 inside the cube
    B, NV, h, w, V = 2, 3, 12, 20, 7
    K, R, t = synth.ring_cameras(NV, 64, inside=True)
    P = torch.from_numpy(O.resized_projection(K, R, t, (64, 64), (h, w))).float()
    P = P[None].repeat(B, 1, 1, 1).contiguous()
    P[1, 1] *= 1.01
    base = np.array([[30.0, -20.0, 10.0], [-100.0, 50.0, 80.0]])
    cv = torch.stack([O.coord_volume(base[b], 2500.0, V, theta=0.3 * b) for b in range(B)])
    for C in (32, 8, 5):
        hm = torch.randn(B, NV, C, h, w, generator=g)
        conf = torch.rand(B, NV, C, generator=g)
        out["unproj_hm_C%d" % C] = hm.numpy()
        out["unproj_cin_C%d" % C] = conf.numpy()
        for method in ("sum", "max", "softmax", "conf"):
            ref = op.unproject_heatmaps(hm, P, cv, method, conf)
            _check("unproject/%s/C%d" % (method, C), O.unproject_heatmaps(hm, P, cv, method, conf), ref, 2e-6)
            out["unproj_%s_C%d" % (method, C)] = ref.numpy()
    out["unproj_P"] = P.numpy(); out["unproj_cv"] = cv.numpy()
    try:
        op.unproject_heatmaps(hm, P, cv, "bogus")
        raise AssertionError("expected ValueError")
    except ValueError as e:
        out["unproj_bad_method_msg"] = np.array(str(e))
    # --- 3D soft-argmax
    vols = torch.randn(2, 5, 6, 7, 8, generator=g) * 3
    cvs = torch.randn(2, 6, 7, 8, 3, generator=g) * 100
    for sm in (True, False):
        rc, rv = op.integrate_tensor_3d_with_coordinates(vols, cvs, softmax=sm)
        oc, ov = O.integrate_tensor_3d_with_coordinates(vols, cvs, softmax=sm)
        _check("integrate3d/softmax=%s" % sm, oc, rc, 2e-6); _check("integrate3d vols", ov, rv, 2e-6)
        out["int3d_coords_%d" % sm] = rc.numpy(); out["int3d_vols_%d" % sm] = rv.numpy()
    out["int3d_in"] = vols.numpy(); out["int3d_cv"] = cvs.numpy()
    # --- 2D soft-argmax
    hm2 = torch.randn(3, 4, 9, 11, generator=g) * 4
    for sm in (True, False):
        rc, rh = op.integrate_tensor_2d(hm2, softmax=sm)
        oc, oh = O.integrate_tensor_2d(hm2, softmax=sm)
        _check("integrate2d/softmax=%s" % sm, oc, rc, 2e-6); _check("integrate2d hm", oh, rh, 2e-6)
        out["int2d_coords_%d" % sm] = rc.numpy(); out["int2d_hm_%d" % sm] = rh.numpy()
    out["int2d_in"] = hm2.numpy()
    # --- DLT: project a known point, triangulate back (SURVEY.md section 4 known-answer)
    K4, R4, t4 = synth.ring_cameras(4, 256)
    P4 = torch.from_numpy(K4 @ np.concatenate([R4, t4], -1)).float()
    X = torch.tensor([[100.0, -50.0, 300.0], [-400.0, 20.0, -100.0], [0.0, 0.0, 0.0]])
    pts = torch.stack([mv.project_3d_points_to_image_plane_without_distortion(P4[v], X) for v in range(4)])  # (NV,J,2)
    pts = pts[None].repeat(2, 1, 1, 1).contiguous()
    pts[1] += torch.randn(pts[1].shape, generator=g) * 2.0
    conf = torch.rand(2, 4, 3, generator=g) + 0.1
    Pb = P4[None].repeat(2, 1, 1, 1).contiguous()
    rt = mv.triangulate_batch_of_points(Pb, pts, conf)
    _check("triangulate", O.triangulate_batch_of_points(Pb, pts, conf), rt, 1e-5)
    assert float((rt[0] - X).abs().max()) < 1e-2, rt[0]
    rt_nc = mv.triangulate_batch_of_points(Pb, pts)
    out.update(dlt_P=Pb.numpy(), dlt_pts=pts.numpy(), dlt_conf=conf.numpy(), dlt_out=rt.numpy(),
               dlt_out_noconf=rt_nc.numpy(), dlt_X=X.numpy())
    # --- geometry helpers
    for i, (axis, th) in enumerate([((0, 0, 1), 0.0), ((0, 0, 1), 1.234), ((0, 1, 0), -2.5), ((1, 2, 3), 0.7)]):
        rr = vol.get_rotation_matrix(axis, th)
        assert np.abs(rr - O.rotation_matrix(axis, th)).max() < 1e-15
        out["rot_%d" % i] = rr; out["rot_%d_arg" % i] = np.array(list(axis) + [th], dtype=np.float64)
    cam = mv.Camera(R4[1], t4[1], K4[1])
    cam.update_after_crop((10, 20, 200, 220))
    cam.update_after_resize((200, 190), (96, 96))
    out["cam_K_after"] = cam.K.copy(); out["cam_P_after"] = cam.projection.copy()
    out["cam_in"] = np.concatenate([R4[1].ravel(), t4[1].ravel(), K4[1].ravel()])
    Kc = K4[1].copy(); Kc[0, 2] -= 10; Kc[1, 2] -= 20
    assert np.abs(O.resized_projection(Kc, R4[1], t4[1], (200, 190), (96, 96)) - cam.projection).max() < 1e-9
    cvr = O.coord_volume(base[0], 2500.0, 8, theta=0.9)
    # reference coord-volume arithmetic, triangulation.py:306-333, executed verbatim on its pieces
    pos = base[0] - 2500.0 / 2
    xxx, yyy, zzz = torch.meshgrid(torch.arange(8), torch.arange(8), torch.arange(8))
    grid = torch.stack([xxx, yyy, zzz], dim=-1).type(torch.float).reshape((-1, 3))
    gc = torch.zeros_like(grid)
    for i in range(3):
        gc[:, i] = pos[i] + (2500.0 / (8 - 1)) * grid[:, i]
    center = torch.from_numpy(base[0]).type(torch.float)
    ref_cv = vol.rotate_coord_volume(gc.reshape(8, 8, 8, 3) - center, 0.9, [0, 0, 1]) + center
    _check("coord_volume(theta=0.9)", cvr, ref_cv, 1e-7)
    out["cv_ref"] = ref_cv.numpy(); out["cv_base"] = base[0]
    np.savez_compressed(os.path.join(GOLD, "ops.npz"), **out)


def gen_nets(mvn):
    out = {}
    g = torch.Generator().manual_seed(9)
    # --- V2V on a 32^3 volume
    sp = spec.v2v_spec(32, 17, "")
    ref = mvn.models.v2v.V2VModel(32, 17)
    rsd = ref.state_dict()
    assert list(rsd.keys()) == list(sp.keys()), "v2v key order"
    assert all(tuple(rsd[k].shape) == sp[k][0] for k in sp)
    sd = synth.make_state_dict(sp, seed=3)
    ref.load_state_dict(sd, strict=True); ref.eval()
    x = torch.randn(1, 32, 32, 32, 32, generator=g)
    with torch.no_grad():
        y = ref(x)
    _check("v2v 32^3", O.v2v(sd, x, prefix=""), y, 2e-5)
    out["v2v_out_s3"] = sub(y, 3); out["v2v_out_absmean"] = y.abs().mean(dim=(2, 3, 4)).numpy()
    out["v2v_sd_digest"] = np.array(synth.state_dict_checksum(sd))
    print("  v2v logits std %.4f" % float(y.std()))
    assert 1e-3 < float(y.std()) < 1.0
    # --- pose resnets
    for nl, hw, algc, volc in ((152, 128, False, False), (50, 128, True, True), (18, 64, False, False)):
        sp = spec.pose_resnet_spec(nl, 17, algc, volc, "")
        cfg = synth.AttrDict(num_layers=nl, style="simple", num_joints=17, alg_confidences=algc,
                             vol_confidences=volc, init_weights=False, checkpoint="")
        ref = mvn.models.pose_resnet.get_pose_net(cfg, device="cpu")
        rsd = ref.state_dict()
        assert list(rsd.keys()) == list(sp.keys()), "resnet%d key order" % nl
        assert all(tuple(rsd[k].shape) == sp[k][0] for k in sp)
        sd = synth.make_state_dict(sp, seed=nl, basic_block=(nl < 50))
        ref.load_state_dict(sd, strict=True); ref.eval()
        x = torch.randn(2, 3, hw, hw, generator=g)
        with torch.no_grad():
            hm, ft, ac, vc = ref(x)
        ohm, oft, oac, ovc = O.pose_resnet(sd, x, nl, prefix="")
        _check("resnet%d features" % nl, oft, ft, 2e-5); _check("resnet%d heatmaps" % nl, ohm, hm, 2e-5)
        print("  resnet%d features absmean %.4f max %.3f" % (nl, float(ft.abs().mean()), float(ft.abs().max())))
        out["rn%d_feat_s2" % nl] = sub(ft, 2); out["rn%d_hm" % nl] = hm.numpy()
        out["rn%d_sd_digest" % nl] = np.array(synth.state_dict_checksum(sd))
        if algc:
            _check("resnet%d alg conf" % nl, oac, ac, 2e-5); _check("resnet%d vol conf" % nl, ovc, vc, 2e-5)
            out["rn%d_algc" % nl] = ac.numpy(); out["rn%d_volc" % nl] = vc.numpy()
    np.savez_compressed(os.path.join(GOLD, "nets.npz"), **out)


def gen_caffe(mvn):
    """style == 'caffe' (pose_resnet.py:322-324, Bottleneck_CAFFE :98-137): at a bottleneck depth (50) and at a basic-block
    depth (18), where the reference still swaps in the expansion-4 caffe bottleneck."""
    out = {}
    g = torch.Generator().manual_seed(31)
    for nl, hw in ((50, 128), (18, 64)):
        sp = spec.pose_resnet_spec(nl, 17, False, False, "", caffe=True)
        cfg = synth.AttrDict(num_layers=nl, style="caffe", num_joints=17, alg_confidences=False, vol_confidences=False,
                             init_weights=False, checkpoint="")
        ref = mvn.models.pose_resnet.get_pose_net(cfg, device="cpu")
        rsd = ref.state_dict()
        assert list(rsd.keys()) == list(sp.keys()), "caffe resnet%d key order" % nl
        assert all(tuple(rsd[k].shape) == sp[k][0] for k in sp)
        sd = synth.make_state_dict(sp, seed=700 + nl)
        ref.load_state_dict(sd, strict=True); ref.eval()
        x = torch.randn(2, 3, hw, hw, generator=g)
        with torch.no_grad():
            hm, ft, _, _ = ref(x)
        ohm, oft, _, _ = O.pose_resnet(sd, x, nl, prefix="", caffe=True)
        _check("caffe resnet%d features" % nl, oft, ft, 2e-5); _check("caffe resnet%d heatmaps" % nl, ohm, hm, 2e-5)
        # the two styles really differ on the same weights (otherwise this fixture would pin nothing)
        _, sft, _, _ = O.pose_resnet(sd, x, nl if nl >= 50 else 50, prefix="", caffe=False) if nl >= 50 else (None, None, None, None)
        if sft is not None:
            assert _maxrel(sft, ft) > 1e-2
        out["rn%d_feat_s2" % nl] = sub(ft, 2); out["rn%d_hm" % nl] = hm.numpy()
        out["rn%d_sd_digest" % nl] = np.array(synth.state_dict_checksum(sd))
        out["rn%d_nkeys" % nl] = np.array(len(sp))
    np.savez_compressed(os.path.join(GOLD, "nets_caffe.npz"), **out)


def gen_pipe2d(mvn):
    """Well-conditioned algebraic tail (triangulation.py:164-191): heatmaps RENDERED from a projected skeleton (Gaussian blobs
    at the projections of known 3D joints + noise), through op.integrate_tensor_2d (x100, softmax), the heatmap->image scaling
    and multiview.triangulate_batch_of_points.  Unlike random-weight heatmaps the four views agree on a 3D point, so the
    DLT is well conditioned and the END-TO-END 3D output can be gated."""
    op, mv = mvn.utils.op, mvn.utils.multiview
    g = torch.Generator().manual_seed(77)
    B, NV, J, H, h = 2, 4, 17, 256, 64
    K, R, t = synth.ring_cameras(NV, H)
    P = torch.from_numpy(K @ np.concatenate([R, t], -1)).float()                      # image-resolution projections
    X = (torch.rand(B, J, 3, generator=g) - 0.5) * torch.tensor([800.0, 800.0, 1600.0])  # a "skeleton" inside the capture volume
    hm = torch.zeros(B, NV, J, h, h)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing="ij")
    for b in range(B):
        for v in range(NV):
            uv = mv.project_3d_points_to_image_plane_without_distortion(P[v], X[b]) * (h / H)   # heatmap pixels
            for j in range(J):
                hm[b, v, j] = 0.12 * torch.exp(-((xx - uv[j, 0]) ** 2 + (yy - uv[j, 1]) ** 2) / (2 * 1.5 ** 2))
    hm = hm + 0.002 * torch.randn(hm.shape, generator=g)
    conf = torch.rand(B, NV, J, generator=g) + 0.2
    kp2d, hm_sm = op.integrate_tensor_2d(hm.reshape(B * NV, J, h, h) * 100.0, True)
    kp2d = kp2d.reshape(B, NV, J, 2)
    cn = conf / conf.sum(dim=1, keepdim=True) + 1e-5
    kp2d_img = torch.stack([kp2d[..., 0] * (H / h), kp2d[..., 1] * (H / h)], dim=-1)
    Pb = P[None].repeat(B, 1, 1, 1).contiguous()
    kp3d = mv.triangulate_batch_of_points(Pb, kp2d_img, cn)
    err = float((kp3d - X).norm(dim=-1).max())
    print("  rendered-heatmap pipeline: triangulated vs true joints max %.2f mm" % err)
    assert err < 30.0, err       # soft-argmax of a blob on a 64-pixel grid: a few mm, i.e. the views AGREE
    o2, _ = O.integrate_tensor_2d(hm.reshape(B * NV, J, h, h) * 100.0, True)
    _check("pipe2d kp2d", o2.reshape(B, NV, J, 2), kp2d, 2e-6)
    _check("pipe2d kp3d", O.triangulate_batch_of_points(Pb, kp2d_img, cn), kp3d, 1e-5)
    np.savez_compressed(os.path.join(GOLD, "pipe2d.npz"), hm=hm.numpy(),
                        conf=conf.numpy(), P=Pb.numpy(), kp2d=kp2d_img.numpy(), kp3d=kp3d.numpy(), X=X.numpy(),
                        hm_sm_sub=sub(hm_sm, 4))


def gen_grad(mvn):
    """Gradient fixtures for the non-convolution backward kernels: torch.autograd THROUGH THE REFERENCE'S OWN
    op.unproject_heatmaps / op.integrate_tensor_3d_with_coordinates / loss.KeypointsMAELoss / loss.VolumetricCELoss on CPU.
      (1) the small op fixtures of gen_ops (non-square maps, a camera inside the cube, rotated grids; C = 8), every aggregation;
      (2) the small_softmax whole-pipeline case: d loss / d features through the unprojection for a random upstream gradient, and
          d (MAE + 0.01 CE) / d logits through the 3D soft-argmax (train.py:217-230)."""
    import mvn.models.loss as L
    op = mvn.utils.op
    ops = np.load(os.path.join(GOLD, "ops.npz"))
    out = {}
    g = torch.Generator().manual_seed(41)
    P, cv = torch.from_numpy(ops["unproj_P"]), torch.from_numpy(ops["unproj_cv"])
    hm0 = torch.from_numpy(ops["unproj_hm_C8"]); conf0 = torch.from_numpy(ops["unproj_cin_C8"])
    G = torch.randn(2, 8, 7, 7, 7, generator=g)
    out["u_G"] = G.numpy()
    for method in ("sum", "max", "softmax", "conf"):
        hm = hm0.clone().requires_grad_(True); conf = conf0.clone().requires_grad_(True)
        vol = op.unproject_heatmaps(hm, P, cv, method, conf)
        (vol * G).sum().backward()
        out["u_ghm_" + method] = hm.grad.numpy()
        if method == "conf":
            out["u_gconf"] = conf.grad.numpy()
        print("  unproject/%s: |grad| max %.3e" % (method, float(hm.grad.abs().max())))
    # 3D soft-argmax + losses on the int3d fixture
    vols0, cvs = torch.from_numpy(ops["int3d_in"]), torch.from_numpy(ops["int3d_cv"])
    Gk = torch.randn(2, 5, 3, generator=g); Gp = torch.randn(2, 5, 6, 7, 8, generator=g) * 0.1
    gt = torch.randn(2, 5, 3, generator=g) * 60; val = (torch.rand(2, 5, 1, generator=g) > 0.25).float()
    out.update(s_Gk=Gk.numpy(), s_Gp=Gp.numpy(), s_gt=gt.numpy(), s_val=val.numpy())
    for sm in (True, False):
        v = vols0.clone().requires_grad_(True)
        c, pv = op.integrate_tensor_3d_with_coordinates(v, cvs, softmax=sm)
        ((c * Gk).sum() + (pv * Gp).sum()).backward()
        out["s_glogits_dense_%d" % sm] = v.grad.numpy()
    v = vols0.clone().requires_grad_(True)
    c, pv = op.integrate_tensor_3d_with_coordinates(v, cvs, softmax=True)
    mae = L.KeypointsMAELoss()(c * 0.1, gt * 0.1, val)
    ce = L.VolumetricCELoss()(cvs, pv, gt, val)
    (mae + 0.01 * ce).backward()
    out.update(s_mae=np.array(float(mae)), s_ce=np.array(float(ce)), s_glogits_loss=v.grad.numpy())
    for name, cls in (("mse", L.KeypointsMSELoss), ("mse_smooth", L.KeypointsMSESmoothLoss), ("l2", L.KeypointsL2Loss)):
        out["s_" + name] = np.array(float(cls()(c.detach() * 0.1, gt * 0.1, val)))
    # whole-pipeline shapes: the small_softmax case (2 samples, 3 views, camera 0 inside the cube, rotated cuboids)
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), ""))
    c = dict(nl=18, B=2, NV=3, H=128, V=32, seed=2)
    cfg = synth.vol_config(c["nl"], c["V"], "softmax", 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(c["nl"], 17, False), seed=c["seed"], sharpen=True, basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=True)
    gs = np.load(os.path.join(GOLD, "vol_small_softmax.npz"))
    o = O.volumetric_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"], inp["pred_keypoints_3d"], thetas=gs["thetas"], stages=True)
    f = o["features"].clone().requires_grad_(True)
    GV = torch.randn(o["unprojected"].shape, generator=g)
    vol = op.unproject_heatmaps(f, o["proj"], o["coord_volumes"], "softmax")
    _check("grad fixture: unprojected volume", vol.detach(), o["unprojected"], 2e-6)
    (vol * GV).sum().backward()
    out["p_gfeat"] = f.grad.numpy(); out["p_GV_seed"] = np.array(41)
    lg = o["logits"].clone().requires_grad_(True)
    kp, pv = op.integrate_tensor_3d_with_coordinates(lg * 1.0, o["coord_volumes"], softmax=True)
    gt3 = kp.detach() + torch.randn(kp.shape, generator=g) * 30; val3 = torch.ones(2, 17, 1); val3[1, 3] = 0
    mae = L.KeypointsMAELoss()(kp * 0.1, gt3 * 0.1, val3)
    ce = L.VolumetricCELoss()(o["coord_volumes"], pv, gt3, val3)
    (mae + 0.01 * ce).backward()
    out.update(p_gt=gt3.numpy(), p_val=val3.numpy(), p_mae=np.array(float(mae)), p_ce=np.array(float(ce)), p_glogits_s2=sub(lg.grad, 2),
               p_glogits_absmax=np.array(float(lg.grad.abs().max())))
    print("  pipeline: mae %.4f ce %.4f |glogits| max %.3e |gfeat| max %.3e" % (float(mae), float(ce), float(lg.grad.abs().max()), float(f.grad.abs().max())))
    np.savez_compressed(os.path.join(GOLD, "grads.npz"), **out)


def gen_data(mvn):
    """Dataset/eval adjacency of the hot path: the reference's collate_fn / prepare_batch
    (datasets/utils.py:6-65) and Human36MMultiViewDataset.evaluate (human36m.py:190-273) on synthetic items / labels."""
    import types
    import mvn.datasets.utils as du
    import mvn.datasets.human36m as h36
    rs = np.random.RandomState(12)
    NVt, B, H, J = 5, 3, 16, 17
    K, R, t = synth.ring_cameras(NVt, H)
    Cam = mvn.utils.multiview.Camera
    items = []
    for b in range(B):
        items.append({"images": [rs.randn(H, H, 3) for _ in range(NVt)], "detections": [rs.rand(5) for _ in range(NVt)],
                      "cameras": [Cam(R[v], t[v], K[v]) for v in range(NVt)], "keypoints_3d": np.concatenate([rs.randn(J, 3) * 100, np.ones((J, 1))], 1),
                      "indexes": b, "pred_keypoints_3d": rs.randn(J, 3) * 100})
    items.insert(1, None)
    batch = du.make_collate_fn(randomize_n_views=False)(items)
    np.random.seed(4)
    batch_r = du.make_collate_fn(randomize_n_views=True, min_n_views=2, max_n_views=4)(items)
    im, kp, val, P = du.prepare_batch(batch, "cpu", None)
    out = {"items_seed": np.array(12), "images": im.numpy(), "kp": kp.numpy(), "val": val.numpy(), "P": P.numpy(),
           "rand_images_shape": np.array(batch_r["images"].shape), "rand_images_sum": np.array(float(batch_r["images"].sum())),
           "pred_kp": batch["pred_keypoints_3d"]}
    # evaluate: a fake label table with 4 actions x 2 trials, 3 subjects
    N = 40
    action_names = ["Walking-1", "Walking-2", "Eating-1", "Eating-2"]
    subject_names = ["S1", "S5", "S9"]
    table = {"keypoints": rs.randn(N, J, 3) * 300, "action_idx": rs.randint(0, 4, size=N), "subject_idx": rs.randint(0, 3, size=N)}
    fake = types.SimpleNamespace(labels={"table": table, "action_names": action_names, "subject_names": subject_names}, num_keypoints=J, kind="mpii")
    fake.evaluate_using_per_pose_error = types.MethodType(h36.Human36MMultiViewDataset.evaluate_using_per_pose_error, fake)
    pred = table["keypoints"] + rs.randn(N, J, 3) * 20
    res = {}
    for name, kw in (("plain", {}), ("cmu", {"transfer_cmu_to_human36m": True}), ("h36", {"transfer_human36m_to_human36m": True})):
        scalar, full = h36.Human36MMultiViewDataset.evaluate(fake, pred, **kw)
        res[name] = {"scalar": float(scalar), "full": {k: {s: {a: float(v) for a, v in d.items()} for s, d in sd.items()} for k, sd in full.items()}}
    try:
        h36.Human36MMultiViewDataset.evaluate(fake, pred[:, :5])
        raise AssertionError("expected ValueError")
    except ValueError as e:
        res["bad_shape_msg"] = str(e)
    out.update(ev_kp=table["keypoints"], ev_action=table["action_idx"], ev_subject=table["subject_idx"], ev_pred=pred, ev_json=np.array(json.dumps(res)))
    np.savez_compressed(os.path.join(GOLD, "data_eval.npz"), **out)


def _train_sub(t, n=129):
    """Strided sample of a parameter-shaped tensor (<= n values) -- the fixtures stay small; the norms cover the rest."""
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // n)][:n].numpy().copy()


def gen_train(mvn, method="softmax", fname="train_step.npz", freeze_backbone_bn=False, nl=18, kind="mpii", cmu=False):
    """One full training step of the reference's VolumetricTriangulationNet on CPU (train.py:148-243): model.train() (BatchNorm on batch
    statistics, running statistics updated, random cuboid rotation), criterion MAE on keypoints * scale_keypoints_3d + 0.01 *
    VolumetricCELoss, total_loss.backward(), torch.optim.Adam with the three learning-rate groups of train.py:430-437, opt.step().
    Stored: losses, predictions, per-parameter gradient norms + strided samples, the BatchNorm running statistics and the parameters
    after the step (samples).

    Training-mode BatchNorm over few samples makes the step ILL-CONDITIONED (the V2V bottleneck normalises 2 x 2^3 = 16 values per
    channel at V = 64; at V = 32 it would be 2, where a 1e-6 relative change of the images moves the reference's own gradients by
    6 % median).  So the reference is run three times -- 8 threads, 1 thread (another fp32 summation order), and with the images
    scaled by (1 + 1e-6) -- and the fixture stores, per parameter, how far the reference's gradient moves between them
    (``noise/<name>``): the test gates ours against the reference within that measured self-noise.

    method = "conf_norm" (fixture train_step_conf_norm.npz): the same step with volume_aggregation_method conf_norm -- the backbone's
    vol_confidences head (GlobalAveragePoolingHead, pose_resnet.py:140-174) is then part of the graph, its sigmoid output weights the
    views (op.py:150-151) after normalisation over them (triangulation.py:268-269), and the returned confidences are stored too."""
    import mvn.models.loss as L
    torch.set_num_threads(8)          # the fixture's fp32 summation order (the 1-thread run below measures what another order changes)
    c = dict(nl=nl, B=2, NV=3, H=128, V=64, seed=12)          # nl = 50: BOTTLENECK blocks (1x1 reduce / 3x3 / 1x1 expand, strided downsample convolutions -- ResNet-152's)
    cfg = synth.vol_config(c["nl"], c["V"], method, 1.0, kind)          # kind "coco": the cuboid is centred between the hips (triangulation.py:282-288)
    if cmu:                                                              # ... and the CMU -> Human3.6M axis permutation of the grid (triangulation.py:336-339)
        cfg.model.transfer_cmu_to_human36m = True
    sp = spec.vol_net_spec(c["nl"], 17, method.startswith("conf"))
    sd = synth.make_state_dict(sp, seed=c["seed"], sharpen=60.0, basic_block=nl < 50)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    lr, pf_lr, vn_lr = 1e-4, 1e-3, 1e-3          # experiments/human36m/train/human36m_vol_softmax.yaml
    g = torch.Generator().manual_seed(43)
    dgt = torch.randn(c["B"], 17, 3, generator=g) * 40
    val = torch.ones(c["B"], 17, 1); val[1, 5] = 0

    def step(eps=0.0, gt=None):
        ref = mvn.models.triangulation.VolumetricTriangulationNet(cfg, device="cpu")
        ref.load_state_dict(sd, strict=True)
        ref.train()
        if freeze_backbone_bn:          # fine-tuning with frozen backbone statistics: the backbone's BatchNorm modules in eval(), everything still trainable
            for mod in ref.backbone.modules():
                if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                    mod.eval()
        opt = torch.optim.Adam([{"params": ref.backbone.parameters()}, {"params": ref.process_features.parameters(), "lr": pf_lr},
                                {"params": ref.volume_net.parameters(), "lr": vn_lr}], lr=lr)
        batch = {"cameras": _cameras(mvn, inp["K"], inp["R"], inp["t"], c["B"]), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
        np.random.seed(c["seed"] + 100)
        kp, feats, vols, vconf, cuboids, cvs, bps = ref(inp["images"] * (1.0 + eps), torch.zeros(c["B"], c["NV"], 3, 4), batch)
        if gt is None:
            gt = kp.detach() + dgt
        mae = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val)
        ce = L.VolumetricCELoss()(cvs, vols, gt, val)
        opt.zero_grad()
        (mae + 0.01 * ce).backward()
        return ref, opt, dict(kp=kp.detach(), feats=feats.detach(), vols=vols.detach(), gt=gt, mae=float(mae), ce=float(ce),
                              vconf=None if vconf is None else vconf.detach())

    np.random.seed(c["seed"] + 100)
    thetas = np.random.uniform(0.0, 2 * np.pi, size=c["B"])
    t0 = time.time()
    ref, opt, r = step()
    nthr = 8
    torch.set_num_threads(1)
    ref1, _, r1 = step(gt=r["gt"])
    torch.set_num_threads(nthr)
    refp, _, rp = step(eps=1e-6, gt=r["gt"])
    kp = r["kp"]
    kp_noise = max(float(((o["kp"] - kp).abs() / kp.abs().clamp(min=1.0)).max()) for o in (r1, rp))
    out = {"kp": kp.numpy(), "gt": r["gt"].numpy(), "val": val.numpy(), "mae": np.array(r["mae"]), "ce": np.array(r["ce"]),
           "thetas": thetas, "lrs": np.array([lr, pf_lr, vn_lr]), "vol_sub": sub(r["vols"], 4), "kp_noise": np.array(kp_noise),
           "loss_noise": np.array(max(abs(o["mae"] - r["mae"]) / r["mae"] for o in (r1, rp))),
           "feat_sub": sub(r["feats"].reshape(c["B"] * c["NV"], *r["feats"].shape[2:]), 2)}
    if r["vconf"] is not None:
        out["vconf"] = r["vconf"].numpy()
        out["vconf_noise"] = np.array(max(float((o["vconf"] - r["vconf"]).abs().max()) for o in (r1, rp)))
    names, no_grad, noises = [], [], []
    g1, gp = dict(ref1.named_parameters()), dict(refp.named_parameters())
    for n, p in ref.named_parameters():
        if p.grad is None:
            no_grad.append(n)
            continue
        names.append(n)
        gmax = float(p.grad.abs().max())
        out["g/" + n] = _train_sub(p.grad)
        out["gn/" + n] = np.array([float(p.grad.double().norm()), gmax, float(p.grad.double().sum())])
        noise = max(float((o[n].grad - p.grad).abs().max()) for o in (g1, gp)) / max(gmax, 1e-30)
        out["noise/" + n] = np.array(noise)
        noises.append(noise)
    opt.step()
    for n, p in ref.named_parameters():
        if n in names:
            out["p1/" + n] = _train_sub(p)
    for n, b_ in ref.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            out["rs/" + n] = _train_sub(b_)
    out["names"] = np.array(names); out["no_grad"] = np.array(no_grad)
    gn = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters() if p.grad is not None)))
    out["grad_norm"] = np.array(gn)
    noises = np.sort(np.array(noises))
    print("  train step x3: %.1fs; mae %.4f ce %.4f; %d parameters with gradients (%d without), global grad norm %.4e" % (
        time.time() - t0, r["mae"], r["ce"], len(names), len(no_grad), gn))
    print("  reference self-noise (threads / 1e-6 perturbation): kp %.2e; gradients median %.2e, 90%% %.2e, max %.2e" % (
        kp_noise, noises[len(noises) // 2], noises[int(len(noises) * 0.9)], noises[-1]))
    np.savez_compressed(os.path.join(GOLD, fname), **out)


def gen_train_alg(mvn, use_conf=True, fname="train_step_alg.npz"):
    """One full training step of the reference's AlgebraicTriangulationNet on CPU (train.py:148-243 with model_type "alg"): model.train(), criterion
    MSESmooth(threshold 400) on keypoints * scale_keypoints_3d (experiments/human36m/train/human36m_alg.yaml:9-19), total_loss.backward() through
    triangulate_batch_of_points (torch.svd, multiview.py:163), the 2D soft-argmax, the alg_confidences head and the backbone, torch.optim.Adam.
    ``heatmap_multiplier`` is 1 here (the yaml's 100 turns the soft-argmax of random-init heatmaps into a near-argmax whose DLT is ill-conditioned:
    the reference's own gradients then move by orders of magnitude between two thread counts); the self-noise of the reference (8 threads / 1 thread /
    images x (1 + 1e-6)) is stored per parameter like in gen_train."""
    import mvn.models.loss as L
    torch.set_num_threads(8)
    c = dict(nl=18, B=2, NV=3, H=128, seed=21)
    cfg = synth.alg_config(c["nl"], use_conf)          # use_conf False: experiments/human36m/train/human36m_alg_no_conf.yaml (uniform view weights, no head)
    cfg.model.heatmap_multiplier = 1.0
    sp = spec.alg_net_spec(c["nl"], 17, use_conf)
    sd = synth.make_state_dict(sp, seed=c["seed"], basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(c["B"], 1, 1, 1)
    lr = 1e-5
    g = torch.Generator().manual_seed(44)
    dgt = torch.randn(c["B"], 17, 3, generator=g) * 40
    val = torch.ones(c["B"], 17, 1); val[0, 3] = 0

    def step(eps=0.0, gt=None, dt=torch.float32):
        ref = mvn.models.triangulation.AlgebraicTriangulationNet(cfg, device="cpu")
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.to(dt)
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, ref.parameters()), lr=lr)
        kp3, kp2, hm, conf = ref((inp["images"] * (1.0 + eps)).to(dt), P.to(dt), {})
        if gt is None:
            gt = kp3.detach() + dgt
        loss = L.KeypointsMSESmoothLoss(400)(kp3 * 0.1, gt.to(kp3.dtype) * 0.1, val.to(kp3.dtype))
        opt.zero_grad()
        loss.backward()
        return ref, opt, dict(kp3=kp3.detach(), kp2=kp2.detach(), hm=hm.detach(), conf=conf.detach(), gt=gt, loss=float(loss))

    t0 = time.time()
    ref, opt, r = step()
    torch.set_num_threads(1)
    ref1, _, r1 = step(gt=r["gt"])
    torch.set_num_threads(8)
    refp, _, rp = step(eps=1e-6, gt=r["gt"])
    kp = r["kp3"]
    kp_noise = max(float(((o["kp3"] - kp).abs() / kp.abs().clamp(min=1.0)).max()) for o in (r1, rp))
    out = {"kp3": kp.numpy(), "kp2": r["kp2"].numpy(), "conf": r["conf"].numpy(), "gt": r["gt"].numpy(), "val": val.numpy(), "loss": np.array(r["loss"]),
           "P": P.numpy(), "lr": np.array(lr), "kp_noise": np.array(kp_noise), "loss_noise": np.array(max(abs(o["loss"] - r["loss"]) / r["loss"] for o in (r1, rp))),
           "hm_sub": sub(r["hm"].reshape(c["B"] * c["NV"], *r["hm"].shape[2:]), 2)}
    # how exact is the reference's OWN gradient through torch.svd in fp32?  The tail (DLT + loss) on the stored 2D keypoints / confidences, once in
    # fp32 (what the step above did) and once in fp64: every parameter gradient of the step inherits this relative error, and no thread count shows it
    def tail_grads(dt):
        p2 = r["kp2"].to(dt).clone().requires_grad_(True)
        cf = r["conf"].to(dt).clone().requires_grad_(True)
        x3 = mvn.utils.multiview.triangulate_batch_of_points(P.to(dt), p2, confidences_batch=cf)
        L.KeypointsMSESmoothLoss(400)(x3.to(dt) * 0.1, r["gt"].to(dt) * 0.1, val.to(dt)).backward()
        return p2.grad.double(), cf.grad.double()
    # ... and the WHOLE step with the reference's modules in fp64 (same code, .double()): the exact gradients the fp32 step approximates
    ref64, _, r64 = step(gt=r["gt"], dt=torch.float64)
    g64 = dict(ref64.named_parameters())
    (p32, c32), (p64, c64) = tail_grads(torch.float32), tail_grads(torch.float64)
    svd32 = max(float((p32 - p64).abs().max() / p64.abs().max()), float((c32 - c64).abs().max() / c64.abs().max()))
    out["svd32_rel"] = np.array(svd32)
    names, no_grad, noises = [], [], []
    g1, gp = dict(ref1.named_parameters()), dict(refp.named_parameters())
    for n, p in ref.named_parameters():
        if p.grad is None:
            no_grad.append(n)
            continue
        names.append(n)
        gmax = float(p.grad.abs().max())
        out["g/" + n] = _train_sub(p.grad)
        out["gn/" + n] = np.array([float(p.grad.double().norm()), gmax, float(p.grad.double().sum())])
        noise = max(float((o[n].grad - p.grad).abs().max()) for o in (g1, gp)) / max(gmax, 1e-30)
        out["noise/" + n] = np.array(noise)
        noises.append(noise)
        out["g64/" + n] = _train_sub(g64[n].grad)
        out["gn64/" + n] = np.array([float(g64[n].grad.norm()), float(g64[n].grad.abs().max())])
    opt.step()
    for n, p in ref.named_parameters():
        if n in names:
            out["p1/" + n] = _train_sub(p)
    for n, b_ in ref.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            out["rs/" + n] = _train_sub(b_)
    out["names"] = np.array(names); out["no_grad"] = np.array(no_grad)
    gn = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters() if p.grad is not None)))
    out["grad_norm"] = np.array(gn)
    out["grad_norm64"] = np.array(float(torch.sqrt(sum(p.grad.pow(2).sum() for p in ref64.parameters() if p.grad is not None))))
    dev32 = sorted(float((p.grad.double() - g64[n].grad).abs().max() / max(float(g64[n].grad.abs().max()), 1e-30)) for n, p in ref.named_parameters() if out["noise/" + n] <= 0.05)
    print("  the reference's fp32 step against its fp64 step, per-parameter max|d|/max|g|: median %.2e, max %.2e" % (dev32[len(dev32) // 2], dev32[-1]))
    noises = np.sort(np.array(noises))
    print("  the reference's fp32 torch.svd backward against fp64 on the same tail inputs: %.2e (relative)" % svd32)
    print("  alg train step x3: %.1fs; loss %.4f; %d parameters with gradients (%d without), global grad norm %.4e" % (time.time() - t0, r["loss"], len(names), len(no_grad), gn))
    print("  reference self-noise: kp %.2e; gradients median %.2e, 90%% %.2e, max %.2e" % (kp_noise, noises[len(noises) // 2], noises[int(len(noises) * 0.9)], noises[-1]))
    np.savez_compressed(os.path.join(GOLD, fname), **out)


def run_vol_case(mvn, tag, num_layers, B, NV, H, V, method="softmax", multiplier=1.0, sharpen=False,
                 inside=False, rotate=False, kind="mpii", seed=0, stride=4, cmu=False, volume_softmax=True, order_noise=False):
    cfg = synth.vol_config(num_layers, V, method, multiplier, kind, volume_softmax=volume_softmax)
    if cmu:
        cfg.model.transfer_cmu_to_human36m = True
    sp = spec.vol_net_spec(num_layers, 17, method.startswith("conf"))
    sd = synth.make_state_dict(sp, seed=seed, sharpen=sharpen, basic_block=(num_layers < 50))
    inp = synth.make_inputs(B, NV, H, seed=seed, inside=inside)
    ref = mvn.models.triangulation.VolumetricTriangulationNet(cfg, device="cpu")
    rsd = ref.state_dict()
    assert list(rsd.keys()) == list(sp.keys()), "vol key order"
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    thetas = None
    if rotate:  # random theta of triangulation.py:318-319 without putting BN into train mode
        ref.training = True
        np.random.seed(seed + 100)
        thetas = np.random.uniform(0.0, 2 * np.pi, size=B)
        np.random.seed(seed + 100)
    batch = {"cameras": _cameras(mvn, inp["K"], inp["R"], inp["t"], B), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    t0 = time.time()
    with torch.no_grad():
        kp, feats, vols, volc, cuboids, cvs, bps = ref(inp["images"], torch.zeros(B, NV, 3, 4), batch)
    dt = time.time() - t0
    o = O.volumetric_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"], inp["pred_keypoints_3d"],
                             thetas=thetas, stages=True)
    print(" case %s: reference forward %.2fs; logits std %.3f, max prob %.2e, kp spread %.1f mm" % (
        tag, dt, float(o["logits"].std() * multiplier), float(vols.max()), float(kp.std(dim=1).mean())))
    _check(tag + " coord_volumes", o["coord_volumes"], cvs, 1e-7)
    _check(tag + " features", o["features"], feats, 2e-5)
    _check(tag + " volumes", o["volumes"], vols, 1e-3)
    _check(tag + " base_points", o["base_points"], bps, 1e-7)
    d = (o["keypoints_3d"] - kp).abs() / kp.abs().clamp(min=1.0)
    print("  oracle-vs-reference %-28s max rel (|ref| floor 1mm) = %.3e" % (tag + " keypoints_3d", float(d.max())))
    assert float(d.max()) < 1e-4
    # the EXACT soft-argmax (fp64) of the reference's own logits: torch's fp32 softmax / einsum over V^3 voxels carry a reduction
    # error of their own (2.9e-4 relative at 128^3: the fp32 probabilities sum to 1 +- 2.9e-4), which a more accurate kernel
    # cannot -- and should not -- reproduce; the fixture stores both so that tests can gate against the exact value
    lg64 = (o["logits"].double() * multiplier).reshape(B, 17, -1)
    p64 = torch.softmax(lg64, dim=2) if volume_softmax else torch.relu(lg64)          # (volume_softmax: false -- ReLU volumes, no normalisation, op.py:91-93)
    kp64 = torch.einsum("bjn,bnc->bjc", p64, cvs.double().reshape(B, -1, 3))
    self_rel = float(((kp.double() - kp64).abs() / kp64.abs().clamp(min=1.0)).max())
    print("  reference fp32 soft-argmax vs the fp64 soft-argmax of its own logits: max rel %.3e" % self_rel)
    res = {
        "kp": kp.numpy(), "kp_fp64": kp64.numpy(), "ref_self_rel": np.array(self_rel), "base_points": bps.numpy(), "proj": o["proj"].numpy(),
        "feat_sub": sub(feats.reshape(B * NV, *feats.shape[2:]), stride), "vol_sub": sub(vols, stride),
        "unproj_sub": sub(o["unprojected"], stride), "logits_sub": sub(o["logits"], stride),
        "cv_sub": cvs[:, ::stride, ::stride, ::stride].contiguous().numpy(), "stride": np.array(stride),
        "sd_digest": np.array(synth.state_dict_checksum(sd)),
        "images_digest": np.array([float(inp["images"].double().sum()), float((inp["images"].double() ** 2).sum())]),
        "cuboid_pos": np.stack([c.position for c in cuboids]), "cuboid_sides": np.stack([c.sides for c in cuboids]),
    }
    if thetas is not None:
        res["thetas"] = thetas
    if volc is not None:
        res["vol_conf"] = volc.numpy()
    if order_noise:
        # the same forward on ONE thread (oneDNN / ATen split their fp32 reductions by thread count): the exact soft-argmax of ITS logits against kp64 above --
        # the fp32 noise of the reference's layers as the soft-argmax amplifies it, in the units of the joint gate
        assert not rotate
        nthr = torch.get_num_threads()
        torch.set_num_threads(1)
        cap = {}
        hk = ref.volume_net.register_forward_hook(lambda m, i, out: cap.__setitem__("logits", out.detach()))
        with torch.no_grad():
            kp1 = ref(inp["images"], torch.zeros(B, NV, 3, 4), batch)[0]
        hk.remove()
        torch.set_num_threads(nthr)
        lg1 = (cap["logits"].double() * multiplier).reshape(B, 17, -1)
        kp64_1 = torch.einsum("bjn,bnc->bjc", torch.softmax(lg1, dim=2), cvs.double().reshape(B, -1, 3))
        order_rel = float(((kp64_1 - kp64).abs() / kp64.abs().clamp(min=1.0)).max())
        print("  reference on 1 thread vs %d threads: exact soft-argmax of the logits differs by max rel %.3e; joints %.3e" % (
            nthr, order_rel, float(((kp1.double() - kp.double()).abs() / kp.double().abs().clamp(min=1.0)).max())))
        res["ref_order_rel"] = np.array(order_rel)
    np.savez_compressed(os.path.join(GOLD, "vol_%s.npz" % tag), **res)
    return float(o["logits"].std())


def gen_alg(mvn):
    cfg = synth.alg_config(50, True)
    sp = spec.alg_net_spec(50, 17, True)
    sd = synth.make_state_dict(sp, seed=50)
    inp = synth.make_inputs(2, 4, 256, seed=1)
    ref = mvn.models.triangulation.AlgebraicTriangulationNet(cfg, device="cpu")
    assert list(ref.state_dict().keys()) == list(sp.keys())
    ref.load_state_dict(sd, strict=True); ref.eval()
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(2, 1, 1, 1)
    with torch.no_grad():
        kp3, kp2, hm, conf = ref(inp["images"], P, {})
    o = O.algebraic_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"])
    _check("alg keypoints_2d", o["keypoints_2d"], kp2, 1e-4)
    _check("alg confidences", o["alg_confidences"], conf, 1e-4)
    _check("alg keypoints_3d", o["keypoints_3d"], kp3, 1e-3)
    np.savez_compressed(os.path.join(GOLD, "alg_c1.npz"), kp3=kp3.numpy(), kp2=kp2.numpy(), conf=conf.numpy(),
                        hm_sub=sub(hm.reshape(8, 17, 64, 64), 4), sd_digest=np.array(synth.state_dict_checksum(sd)))


def gen_alg2(mvn):
    """AlgebraicTriangulationNet with the two switches alg_c1 does not flip: use_confidences false (all-ones weights, triangulation.py:137-143) and
    heatmap_softmax false (ReLU heatmaps normalised by their mass, op.py:11-18); ResNet-18, 2 x 3 views of 128^2."""
    cfg = synth.alg_config(18, False)
    cfg.model.heatmap_softmax = False
    cfg.model.heatmap_multiplier = 1.0
    sp = spec.alg_net_spec(18, 17, False)
    sd = synth.make_state_dict(sp, seed=51, basic_block=True)
    inp = synth.make_inputs(2, 3, 128, seed=9)
    ref = mvn.models.triangulation.AlgebraicTriangulationNet(cfg, device="cpu")
    assert list(ref.state_dict().keys()) == list(sp.keys())
    ref.load_state_dict(sd, strict=True); ref.eval()
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(2, 1, 1, 1)
    with torch.no_grad():
        kp3, kp2, hm, conf = ref(inp["images"], P, {})
    o = O.algebraic_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"])
    _check("alg2 keypoints_2d", o["keypoints_2d"], kp2, 1e-4)
    _check("alg2 confidences", o["alg_confidences"], conf, 1e-6)
    np.savez_compressed(os.path.join(GOLD, "alg_relu_noconf.npz"), kp3=kp3.numpy(), kp2=kp2.numpy(), conf=conf.numpy(),
                        hm_sub=sub(hm.reshape(6, 17, 32, 32), 2), sd_digest=np.array(synth.state_dict_checksum(sd)))


def gen_experiments():
    """The reference's human36m experiment files (train and eval), each as its parsed YAML mapping, keyed by '<train|eval>/<file name>': the
    config surface tests/test_host_logic.py builds the models from (it writes them back out as YAML and reads them with mvn.utils.cfg)."""
    import glob
    import yaml
    root = os.path.join(ref_loader.REFERENCE_ROOT, "experiments", "human36m")
    out = {}
    for f in sorted(glob.glob(os.path.join(root, "*", "*.yaml"))):
        with open(f) as fin:
            out[os.path.relpath(f, root)] = yaml.safe_load(fin)
    with open(os.path.join(GOLD, "experiments_human36m.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def gen_pose_net_loading(mvn):
    """The REFERENCE's get_pose_net (pose_resnet.py:321-377) on the fake checkpoints of tests/test_pose_net_loading.py (the same helper builds them)
    under the same RNG state: per case, the digest of every tensor of the state dict it returns."""
    import tempfile
    sys.path.insert(0, os.path.dirname(GOLD))
    from test_pose_net_loading import CASES, _cfg, _fake_checkpoint, case_id
    nl, J = 18, 17
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for wrap, prefix, joints_ckpt in CASES:
            path = os.path.join(d, "ckpt.pth")
            _fake_checkpoint(path, nl, joints_ckpt, wrap, prefix)
            torch.manual_seed(1234)
            sd = mvn.models.pose_resnet.get_pose_net(_cfg(nl, ckpt=path, init=True, joints=J), device="cpu").state_dict()
            out[case_id(wrap, prefix, joints_ckpt)] = {k: synth.tensor_digest(v) for k, v in sd.items()}
    with open(os.path.join(GOLD, "pose_net_loading.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def _write_truth(name, fixture, truth, tols, norm_wise_joints=False, factor=1):
    """truth_<name>.npz: ``truth`` plus ref32_err/<key> (the fp32 fixture's value against the truth) for every quantity both hold.
    Asserts first that the truth is within the oracle-vs-reference tolerance of the fixture (``tols``: key -> tol), so that a broken
    fp64 path is never committed, and that it is not larger than the fixture.  ``factor``: the truth's strided sub-samples (keys *_sub) keep
    every factor-th point of the fixture's (T.STRIDE_FACTOR for the volumetric fixtures); the reference's error is measured at those points."""
    g = np.load(os.path.join(GOLD, fixture))
    for k in ("sd_digest", "images_digest"):
        if k in g.files:
            assert np.allclose(truth[k], g[k], rtol=1e-12), (name, k, truth[k], g[k])
    if "stride" in g.files:
        assert int(truth["stride"]) == factor * int(g["stride"]), (name, truth["stride"], g["stride"])
    out = dict(truth)
    for k, v in truth.items():
        if k.endswith("digest") or k == "stride":
            continue
        ref = g[T.REF_KEY.get(k, k)]
        e = T.err_of(k, T.coarser(ref, factor) if k.endswith("_sub") else ref, v)
        out["ref32_err/" + k] = np.array(e)
        print("  %-16s %-20s reference fp32 vs fp64 truth %.3e%s" % (name, k, e, " (max rel, 1 mm floor)" if k in T.JOINT_KEYS else ""))
        if k in tols:
            assert e <= tols[k], (name, k, e, tols[k])
    if norm_wise_joints:
        e = T.joints_norm_rel(g["kp"], truth["kp"])
        out["ref32_err/kp_norm"] = np.array(e)
        print("  %-16s %-20s reference fp32 vs fp64 truth %.3e (norm-wise)" % (name, "kp", e))
    path = os.path.join(GOLD, "truth_%s.npz" % name)
    # an .npz (np.load reads it) compressed with LZMA rather than np.savez_compressed's deflate: the truth holds the fixture's arrays plus its
    # own error figures and digests, and must not outgrow the fixture (alg_relu_noconf: 53.7 kB deflated against the fixture's 50.9 kB)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as z:
        for k, v in out.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    # no larger than the fixture -- except below 8 kB: alg_c1.npz is 3.5 kB, less than its truth's two fp64 joint arrays and their zip headers
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(GOLD, fixture)), 8192), (path, os.path.getsize(path))
    assert os.path.getsize(path) < T.MAX_BYTES, (path, os.path.getsize(path))


def gen_truth(which=None):
    """fp64 ground truth beside the fp32 fixtures (oracle/truth.py): every vol_*.npz, alg_c1 and alg_relu_noconf, the nets.npz backbones.
    Self-check tolerances are run_vol_case's / gen_nets' / gen_alg's oracle-vs-reference ones; joints 1e-3 (the reference itself is 1.9e-4
    from the truth on c2_b8_sharp).  The end-to-end algebraic 3D joints are not checked: at random init those DLT systems are so ill
    conditioned that a 5e-5 change of the 2D keypoints moves them by 1.3e-2 (tests/test_gpu_models.py); kp3_of_ref2d is."""
    names = which or (["vol_" + t for t in T.vol_cases()] + list(T.ALG_CASES) + ["nets"])
    for name in names:
        t0 = time.time()
        if name.startswith("vol_"):
            tag = name[4:]
            g = np.load(os.path.join(GOLD, name + ".npz"))
            tr = T.vol_truth(tag, T.STRIDE_FACTOR * int(g["stride"]))
            relu = not T.vol_cases_cfg(tag)["volume_softmax"]
            tols = {"feat_sub": 2e-5, "vol_conf": 2e-5, "unproj_sub": 1e-3, "logits_sub": 1e-3, "vol_sub": 1e-3}     # features / volumes as in run_vol_case
            if not relu:
                tols["kp"] = 1e-3
            _write_truth(tag, name + ".npz", tr, tols, norm_wise_joints=relu, factor=T.STRIDE_FACTOR)
            if relu:
                assert float(T.joints_norm_rel(g["kp"], tr["kp"])) <= 1e-3
        elif name == "nets":
            _write_truth("nets", "nets.npz", T.nets_truth(), {k: 2e-5 for k in ("rn152_feat_s2", "rn152_hm", "rn50_feat_s2", "rn50_hm",
                                                                                "rn50_algc", "rn50_volc", "rn18_feat_s2", "rn18_hm")})
        else:
            g = np.load(os.path.join(GOLD, name + ".npz"))
            tr = T.alg_truth(name, g)
            # gen_alg's oracle-vs-reference measure for the 3D joints, max|d| / max|ref| (element-wise with the 1 mm floor, the reference's fp32
            # SVD is 3.8e-3 from the exact DLT of its own inputs on alg_relu_noconf)
            assert T.max_rel(g["kp3"], tr["kp3_of_ref2d"]) <= 1e-3, name
            _write_truth(name, name + ".npz", tr, {"kp2": 1e-4, "conf": 1e-4})
        print("  truth_%s: %.1f s" % (name[4:] if name.startswith("vol_") else name, time.time() - t0))


def main():
    torch.manual_seed(0)
    os.makedirs(GOLD, exist_ok=True)
    if sys.argv[1:2] == ["truth"]:         # reads only tests/golden and the oracle, not the reference
        print("[truth]"); gen_truth(sys.argv[2:] or None)
        return
    mvn = ref_loader.load()
    which = sys.argv[1:] or ["ops", "nets", "vol", "vol2", "vol3", "vol4", "alg", "alg2", "caffe", "pipe2d", "data", "grad", "train", "train_conf", "train_alg", "train_frozen", "train_sum", "train_max", "train_r50", "train_alg_noconf", "train_cmu", "experiments", "pose_net_loading"]
    if "experiments" in which:
        print("[experiments]"); gen_experiments()
    if "pose_net_loading" in which:
        print("[pose_net_loading]"); gen_pose_net_loading(mvn)
    if "ops" in which:
        print("[ops]"); gen_ops(mvn)
    if "nets" in which:
        print("[nets]"); gen_nets(mvn)
    if "vol" in which:
        print("[vol]")
        # small whole-pipeline cases (fast on CPU, exercise every branch)
        run_vol_case(mvn, "small_softmax", 18, 2, 3, 128, 32, "softmax", sharpen=True, inside=True, rotate=True, seed=2, stride=2)
        run_vol_case(mvn, "small_sum_coco", 18, 1, 2, 128, 32, "sum", multiplier=100.0, sharpen=False, kind="coco", rotate=True, seed=3, stride=2, cmu=True)
        # (multiplier 100 instead of the x250 sharpening: with it the reference deviates from ITSELF by 8.9e-5 between 1 and 8 threads)
        run_vol_case(mvn, "small_conf", 50, 2, 4, 128, 32, "conf_norm", multiplier=100.0, sharpen=False, seed=4, stride=2)
        run_vol_case(mvn, "small_max", 18, 1, 3, 128, 32, "max", sharpen=True, seed=5, stride=2)
        # BASELINE config 2 shape, B=1: default and sharpened weights
        run_vol_case(mvn, "c2_default", 152, 1, 4, 384, 64, "softmax", sharpen=False, seed=0, stride=4)
        std = run_vol_case(mvn, "c2_sharp", 152, 1, 4, 384, 64, "softmax", sharpen=True, seed=0, stride=4)
        print("  (calibration) sharpened logit std = %.3f with SHARPEN_GAIN=%.1f" % (std, synth.SHARPEN_GAIN))
    if "vol3" in which:
        print("[vol3]")
        # round 3: the two switches no other case flips -- volume_softmax: false (ReLU volumes, unnormalised integration, op.py:84-96) with the plain
        # `conf` aggregation (sigmoid confidences as they are, op.py:150-151)
        run_vol_case(mvn, "small_relu_conf", 18, 2, 3, 128, 32, "conf", sharpen=False, seed=7, stride=2, volume_softmax=False)
    if "vol2" in which:
        print("[vol2]")
        # BASELINE config 2 shape at B = 4 (four different samples; batch kernels and XCD pinning see a real batch)
        run_vol_case(mvn, "c2_b4", 152, 4, 4, 384, 64, "softmax", sharpen=True, seed=6, stride=4)
        # BASELINE config 4: 8 views, 128^3 voxels (Panoptic-shaped), ResNet-152, 384^2
        # gain 157 instead of 250: SURVEY section 7 defines "sharpened" by logit std ~5; at 8 views / 128^3 the x250 gain gives std 7.95
        # and max prob 0.22 -- towards the near-argmax regime the survey says not to gate on (logit noise of 1e-6 of max then moves
        # the joints by > 1e-4; the reference's own 2-vs-8-thread deviation was 3e-5 there)
        run_vol_case(mvn, "c4_sharp", 152, 1, 8, 384, 128, "softmax", sharpen=157.0, seed=8, stride=8)
    if "vol4" in which:
        print("[vol4]")
        # round 6: the benchmark shape at B = 8 (32 images): the smallest batch at which the bf16 plan records the kernels the timed forward is made of --
        # conv2d_halo_kernel (from 20 images), the layer3 seam kernel, bneck_ds, cat2 (forced on in its test) -- so that they run under a REFERENCE golden
        # with a joint gate in mm (tests/test_gpu_models.py::test_volumetric_forward_bf16_deviation); stride 8 keeps the fixture at ~2.5 MB
        # gain 150, not the x250 of c2_sharp: with this seed's weights x250 puts the soft-argmax into the near-argmax regime SURVEY section 7 says not to gate
        # on (largest probability 0.07-0.24 per sample against c2_sharp's 7e-3; the REFERENCE then deviates from itself by 1.2e-4 between 1 and 8 threads --
        # measured -- i.e. by more than the 1e-4 gate); x150: largest probability 2.7e-2.  x100 is no easier: the distribution broadens, the joints collapse towards
        # the cube centre (spread 20 mm) and the reference's own fp32 reduction error reaches 1.0e-4 of the 1 mm floor.
        # order_noise: the fixture also stores how far the REFERENCE's joints move when only the order of its fp32 sums changes (1 thread vs 8: 3.0e-5 here, in
        # the units of the gate) -- the reference's output is defined up to that, and 408 coordinates with a 1 mm floor make this the tightest fixture of the set
        run_vol_case(mvn, "c2_b8_sharp", 152, 8, 4, 384, 64, "softmax", sharpen=150.0, seed=11, stride=8, order_noise=True)
    if "train" in which:
        print("[train]"); gen_train(mvn)
    if "train_frozen" in which:
        print("[train_frozen]"); gen_train(mvn, "softmax", "train_step_frozen_bn.npz", freeze_backbone_bn=True)
    if "train_alg" in which:
        print("[train_alg]"); gen_train_alg(mvn)
    if "train_alg_noconf" in which:
        print("[train_alg_noconf]"); gen_train_alg(mvn, False, "train_step_alg_noconf.npz")
    if "train_conf" in which:
        print("[train_conf]"); gen_train(mvn, "conf_norm", "train_step_conf_norm.npz")
    if "train_r50" in which:
        print("[train_r50]"); gen_train(mvn, "softmax", "train_step_r50.npz", nl=50)
    if "train_cmu" in which:
        print("[train_cmu]"); gen_train(mvn, "softmax", "train_step_cmu.npz", kind="coco", cmu=True)
    if "train_sum" in which:          # the two aggregation methods without learned view weights: mean over the views / per-voxel maximum (op.py:143-148)
        print("[train_sum]"); gen_train(mvn, "sum", "train_step_sum.npz")
    if "train_max" in which:
        print("[train_max]"); gen_train(mvn, "max", "train_step_max.npz")
    if "alg" in which:
        print("[alg]"); gen_alg(mvn)
    if "alg2" in which:
        print("[alg2]"); gen_alg2(mvn)
    if "caffe" in which:
        print("[caffe]"); gen_caffe(mvn)
    if "pipe2d" in which:
        print("[pipe2d]"); gen_pipe2d(mvn)
    if "data" in which:
        print("[data]"); gen_data(mvn)
    if "grad" in which:
        print("[grad]"); gen_grad(mvn)
    digest = {k: [list(v[0]), v[1]] for k, v in spec.vol_net_spec(152, 17).items()}
    with open(os.path.join(GOLD, "spec_digest.json"), "w") as f:
        json.dump({"n_keys": len(digest), "n_params": int(sum(int(np.prod(v[0])) for v in digest.values())),
                   "first": list(digest)[:3], "last": list(digest)[-3:]}, f)
    print("golden fixtures written to", GOLD)


if __name__ == "__main__":
    main()
