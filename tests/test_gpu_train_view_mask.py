"""GPU (-m gpu): training with per-sample view masks (``masked_training``) -- lt_unproject_grid_masked_fwd / lt_unproject_masked_bwd inside the recorded
step of VolumetricTriangulationNet, and the masked tail of AlgebraicTriangulationNet.
  * ONE WHOLE MASKED STEP against the step the REFERENCE ITSELF takes on CPU with its unprojection restricted to every sample's valid views
    (tests/golden/train_step_view_mask.npz, tools/make_golden_train_view_mask.py): the body and every gate of
    tests/test_gpu_train_many_views.py::test_whole_training_step_at_ten_views_vs_reference, driven by the constants and the mask the fixture stores;
  * one tape, many masks: a 9-view model takes three steps with three masks on one plan and one tape, each step's parameter gradients bitwise those of a
    fresh model's recording step with that mask, fp32 and act16;
  * an all-ones mask gives the unmasked step's gradients bit for bit;
  * conf_norm: the returned vol_confidences follow the inference rule and the head still trains;
  * the algebraic model's masked tail against its restatement in torch-CPU fp64 on every sample's valid views."""
import os
import re

import numpy as np
import pytest
import torch

from gpu_util import check, record
from oracle import spec, synth
from oracle import vol_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ZERO_GRAD = re.compile(r"^volume_net\.(.*\.(block\.0|res_branch\.0|res_branch\.3|skip_con\.0)|output_layer)\.bias$")


def test_whole_masked_training_step_vs_reference(golden_dir):
    """model.train() with masked_training; forward with batch["view_mask"] = 1111 / 1011 / 0101; MAE(kp * 0.1) + 0.01 * VolumetricCELoss; backward; Adam --
    keypoints at 1e-4 + 2 x kp_noise, every parameter's gradient at 1e-3 + 4 x its stored noise, the BatchNorm running statistics (taken over ALL images,
    the masked views' included, on both sides) at 1e-4 and the parameters after the step at 2e-2 lr, against the reference's own step on CPU."""
    import lt_train
    from mvn.models import loss as L
    from mvn.models.triangulation import VolumetricTriangulationNet
    from test_gpu_models import _cameras
    G = np.load(os.path.join(golden_dir, "train_step_view_mask.npz"))
    c = {str(k): int(v) for k, v in zip(G["case_keys"], G["case"])}
    method, vs, fs = str(G["method"]), int(G["vol_stride"]), int(G["feat_stride"])
    mask = G["view_mask"]
    assert mask.shape == (c["B"], c["NV"]) and mask.tolist() == [[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 1]]
    cfg = synth.vol_config(c["nl"], c["V"], method, 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(c["nl"], 17, False), seed=c["seed"], sharpen=60.0, basic_block=c["nl"] < 50)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    TAG = "[view_mask] "
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    m.train()
    m.masked_training = True
    lr, pf_lr, vn_lr = [float(v) for v in G["lrs"]]
    opt = lt_train.Adam([{"params": list(m.backbone.parameters())}, {"params": list(m.process_features.parameters()), "lr": pf_lr},
                         {"params": list(m.volume_net.parameters()), "lr": vn_lr}], lr=lr)
    batch = {"cameras": _cameras(inp, c["B"]), "pred_keypoints_3d": inp["pred_keypoints_3d"], "view_mask": mask}
    np.random.seed(c["seed"] + 100)
    kp, feats, vols, conf, cuboids, cvs, bps = m(inp["images"].to(DEV), torch.zeros(c["B"], c["NV"], 3, 4, device=DEV), batch)
    kp_noise, loss_noise = float(G["kp_noise"]), float(G["loss_noise"])
    d = (kp.detach().cpu().double() - torch.from_numpy(G["kp"]).double()).abs() / torch.from_numpy(G["kp"]).double().abs().clamp(min=1.0)
    record(TAG + "train/step forward keypoints (train-mode BN), rel with 1 mm floor", {"err": float(d.max()), "tol": 1e-4 + 2 * kp_noise, "reference_self_noise": kp_noise})
    print("keypoints: err %.3e, gate %.3e (reference self-noise %.3e)" % (float(d.max()), 1e-4 + 2 * kp_noise, kp_noise))
    assert float(d.max()) <= 1e-4 + 2 * kp_noise, float(d.max())
    check(TAG + "train/step forward volumes", vols.detach().cpu()[:, :, ::vs, ::vs, ::vs], G["vol_sub"], 1e-3 + 10 * kp_noise)
    check(TAG + "train/step forward features", feats.detach().cpu().reshape(c["B"] * c["NV"], *feats.shape[2:])[:, :, ::fs, ::fs], G["feat_sub"], 1e-4)
    assert conf is None
    gt, val = torch.from_numpy(G["gt"]).to(DEV), torch.from_numpy(G["val"]).to(DEV)
    mae = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val)
    ce = L.VolumetricCELoss()(cvs, vols, gt, val)
    assert abs(float(mae.detach()) - float(G["mae"])) <= (1e-4 + 2 * loss_noise) * float(G["mae"]), (float(mae.detach()), float(G["mae"]))
    assert abs(float(ce.detach()) - float(G["ce"])) <= 1e-3 * float(G["ce"]), (float(ce.detach()), float(G["ce"]))
    opt.zero_grad()
    (mae + 0.01 * ce).backward()
    named = dict(m.named_parameters())
    gn2, table = 0.0, []
    gnorm_ref = float(G["grad_norm"])
    n_zero = 0
    for n in G["names"]:
        n = str(n)
        p = named[n]
        assert p.grad is not None, "no gradient for " + n
        gr = p.grad.detach().double().cpu()
        ref_norm, ref_max, ref_sum = [float(v) for v in G["gn/" + n]]
        noise = float(G["noise/" + n])
        gn2 += float(gr.pow(2).sum())
        if ZERO_GRAD.search(n) or noise > 0.05:
            # a convolution bias in front of a training-mode BatchNorm or the output layer's bias under the softmax: the exact gradient is 0, both sides
            # hold rounding noise of their channel sums
            assert float(gr.abs().max()) <= 10 * ref_max + 1e-6 * gnorm_ref, (n, float(gr.abs().max()), ref_max)
            n_zero += 1
            continue
        f = gr.reshape(-1)
        sub = f[::max(1, f.numel() // 129)][:129]
        e = float((sub - torch.from_numpy(G["g/" + n]).double()).abs().max()) / ref_max
        en = abs(float(gr.norm()) - ref_norm) / ref_norm
        table.append((max(e, en) / (1e-3 + 4 * noise), max(e, en), noise, n))
    table.sort(reverse=True)
    print("worst parameter gradients (err / gate, err, reference self-noise):", *["%.2f %.2e %.2e %s" % t for t in table[:8]], sep="\n  ")
    errs = sorted(t[1] for t in table)
    record(TAG + "train/step parameter gradients vs the reference's step (max|d|/max|ref| on samples, and norm; gate 1e-3 + 4 x reference self-noise)",
           {"worst_err_over_gate": table[0][0], "worst_err": errs[-1], "median_err": errs[len(errs) // 2], "parameters_compared": len(table),
            "zero_gradient_parameters": n_zero, "median_reference_self_noise": sorted(t[2] for t in table)[len(table) // 2]})
    assert table[0][0] <= 1.0, table[:8]
    assert len(table) > 100, len(table)
    for n in G["no_grad"]:
        assert named[str(n)].grad is None
    gn = float(np.sqrt(gn2))
    print("global gradient norm: ours %.6e, reference %.6e" % (gn, gnorm_ref))
    assert abs(gn - gnorm_ref) <= 2e-3 * gnorm_ref, (gn, gnorm_ref)
    record(TAG + "train/step global gradient norm", {"ours": gn, "reference": gnorm_ref})
    # running statistics (momentum 0.1, unbiased variance): over every image, masked views included
    bufs = dict(m.named_buffers())
    w_rs = 0.0
    for key in G.files:
        if key.startswith("rs/"):
            b = bufs[key[3:]].detach().double().cpu().reshape(-1)
            sub = b[::max(1, b.numel() // 129)][:129]
            ref = torch.from_numpy(G[key]).double()
            w_rs = max(w_rs, float((sub - ref).abs().max() / ref.abs().max().clamp(min=1e-30)))
    record(TAG + "train/step BatchNorm running statistics", {"err": w_rs, "tol": 1e-4})
    print("running statistics: err %.3e" % w_rs)
    assert w_rs <= 1e-4, w_rs
    # the Adam step: only the elements the reference knows the sign of are compared (see the ten-view test)
    opt.step()
    torch.cuda.synchronize()
    w_p, w_name, n_known = 0.0, None, 0
    for n in G["names"]:
        n = str(n)
        if ZERO_GRAD.search(n):
            continue
        f = named[n].detach().double().cpu().reshape(-1)
        sub = f[::max(1, f.numel() // 129)][:129]
        ref = torch.from_numpy(G["p1/" + n]).double()
        gs = torch.from_numpy(G["g/" + n]).double().abs()
        known = gs > 100 * (float(G["noise/" + n]) + 1e-3) * float(G["gn/" + n][1])
        n_known += int(known.sum())
        lr_n = lr if n.startswith("backbone.") else pf_lr if n.startswith("process_features.") else vn_lr
        e = float(((sub - ref).abs() * known).max()) / lr_n      # in units of one full Adam step
        if e > w_p:
            w_p, w_name = e, n
    record(TAG + "train/step parameters after Adam, worst |d| in units of lr", {"err": w_p, "tol": 2e-2, "name": w_name, "elements_compared": n_known})
    print("Adam: worst |d| %.3e lr (%s), %d elements compared" % (w_p, w_name, n_known))
    assert w_p <= 2e-2, (w_p, w_name)
    assert n_known > 1000, n_known


# ---- one tape, many masks -----------------------------------------------------------------------------------------------------------------------------------
NINE_MASKS = (np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 0, 1, 1, 1, 1, 0]], dtype=np.uint8),
              np.array([[1, 0, 1, 0, 1, 0, 1, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 1]], dtype=np.uint8),
              np.array([[0, 0, 0, 1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1, 0]], dtype=np.uint8))


def _vol_model(NV, method, precision, masked_training, seed=12):
    from mvn.models.triangulation import VolumetricTriangulationNet
    cfg = synth.vol_config(18, 32, method, 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(18, 17, method.startswith("conf")), seed=seed, sharpen=60.0, basic_block=True)
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    m.train()
    m.train_precision = precision
    m.masked_training = masked_training
    return m


def _step(m, inp, mask):
    """One training forward / backward: ({name: gradient (cpu)}, the forward's 7-tuple)."""
    from mvn.models import loss as L
    from test_gpu_models import _cameras
    B = inp["images"].shape[0]
    batch = {"cameras": _cameras(inp, B), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    if mask is not None:
        batch["view_mask"] = mask
    gt = torch.as_tensor(np.asarray(inp["pred_keypoints_3d"]))[:, :, :3].float().to(DEV)
    val = torch.ones(B, 17, 1, device=DEV)
    np.random.seed(77)
    out = m(inp["images"].to(DEV), None, batch)
    kp, _, vols, _, _, cvs, _ = out
    loss = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val) + 0.01 * L.VolumetricCELoss()(cvs, vols, gt, val)
    for p in m.parameters():
        p.grad = None
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().float().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}, out


@pytest.mark.parametrize("precision", ["fp32", "act16"])
def test_one_tape_serves_every_mask(precision):
    """The nine-view recipe of tests/test_gpu_train_many_views.py at 32^3 voxels.  Three steps with three different masks run ONE plan and ONE tape with an
    unchanged number of recorded operations (a new mask is another step, not another recording), and each step's parameter gradients are BITWISE those of
    a fresh model's first (recording) step with that mask: the mask reaches the replayed launches through the geometry block alone."""
    inp = synth.make_inputs(2, 9, 128, seed=31, inside=False)
    m = _vol_model(9, "softmax", precision, True)
    book = []
    for i, mask in enumerate(NINE_MASKS):
        g, _ = _step(m, inp, mask)
        plans = list(m._train_plans.values())
        book.append((len(plans), id(plans[0]), id(plans[0].tape), len(plans[0].tape.fwd_ops), plans[0].NV, plans[0].masked))
        fresh, _ = _step(_vol_model(9, "softmax", precision, True), inp, mask)
        assert set(g) == set(fresh) and len(g) > 50 and all(np.isfinite(v).all() for v in g.values())
        assert max(float(np.abs(v).max()) for n, v in g.items() if n.startswith("backbone.")) > 0          # the gradient did pass the unprojection
        for n in g:
            assert np.array_equal(g[n], fresh[n]), "step %d (mask %s): gradient of %s differs from a fresh recording with that mask" % (i, mask.tolist(), n)
        if i:
            assert any(not np.array_equal(g[n], first[n]) for n in g), "another mask, the same gradients"
        else:
            first = g
    assert book[0] == book[1] == book[2] and book[0][0] == 1 and book[0][4:] == (9, True), book


def test_all_ones_mask_is_the_unmasked_step():
    """4 views, masked_training with an all-ones mask against the plain step: parameter gradients and keypoints bit for bit (another plan key, another pair
    of entries, the same arithmetic)."""
    inp = synth.make_inputs(2, 4, 128, seed=31, inside=False)
    plain, po = _step(_vol_model(4, "softmax", "fp32", False), inp, None)
    mm = _vol_model(4, "softmax", "fp32", True)
    ones, oo = _step(mm, inp, np.ones((2, 4), dtype=np.uint8))
    assert set(plain) == set(ones) and len(ones) > 50
    assert torch.equal(po[0], oo[0]) and torch.equal(po[2], oo[2])
    for n in plain:
        assert np.array_equal(plain[n], ones[n]), n
    # and without a mask the model takes the unmasked plan, under the key it always had
    _step(mm, inp, None)
    keys = list(mm._train_plans)
    assert len(keys) == 2 and keys[0][-1] == "view_mask" and keys[0][:-1] == keys[1]


def test_conf_norm_confidences_follow_the_inference_rule_and_the_head_trains():
    """conf_norm with masks 1011 / 0101: the returned vol_confidences are normalised over the valid views (they sum to 1 there) and exactly 0 for the masked
    ones; the vol_confidences head still receives a gradient through lt_unproject_masked_bwd's grad_conf, finite and not zero."""
    inp = synth.make_inputs(2, 4, 128, seed=31, inside=False)
    mask = np.array([[1, 0, 1, 1], [0, 1, 0, 1]], dtype=np.uint8)
    m = _vol_model(4, "conf_norm", "fp32", True)
    g, out = _step(m, inp, mask)
    conf = out[3].detach().cpu()
    on = torch.from_numpy(mask).bool()
    assert tuple(conf.shape) == (2, 4, 32) and bool((conf[~on] == 0).all()) and bool((conf[on] > 0).all())
    assert float((conf.sum(1) - 1).abs().max()) <= 1e-6
    head = [n for n in g if "vol_confidences" in n]
    assert head and all(np.isfinite(g[n]).all() for n in g)
    assert max(float(np.abs(g[n]).max()) for n in head) > 0, "the vol_confidences head got no gradient"


# ---- the algebraic model ----------------------------------------------------------------------------------------------------------------------------------
def test_algebraic_masked_tail_vs_fp64_on_the_valid_views(monkeypatch):
    """B = 2, NV = 4, masks 1111 / 0101, 128 x 128.  The backbone's heatmap logits and raw confidences are taken from the GPU as they are; the tail --
    2D soft-argmax, confidences normalised over the valid views + 1e-5, keypoints to image pixels, DLT -- is restated in torch-CPU fp64 (the oracle's
    restatements of the reference's ops) sample by sample on the valid views alone.  The 3D joints at the DLT forward's gate (1e-4); the gradients into
    the heatmap logits and into the raw confidences at the DLT backward's gate of tests/test_gpu_backward.py (2e-3: both pass through the DLT, the
    soft-argmax behind it has the tighter gate 1e-4); a masked view's slices are exactly zero; without the flag the step is refused."""
    from mvn.models import triangulation as TR
    from mvn.utils import multiview
    cfg = synth.alg_config(18, True)
    cfg.model.heatmap_multiplier = 1.0
    cfg.model["heatmap_multiplier"] = 1.0
    sd = synth.make_state_dict(spec.alg_net_spec(18, 17, True), seed=21, basic_block=True)
    B, NV, J, HW = 2, 4, 17, 128
    inp = synth.make_inputs(B, NV, HW, seed=21, inside=False)
    # the cameras: the first four of a FIVE-camera ring.  A four-camera ring puts views 1 and 3 -- all that the mask 0101 leaves of sample 1 -- face to
    # face: two nearly collinear rays per joint, a DLT that has no depth to find, in any precision
    K, R, t = [a[:NV] for a in synth.ring_cameras(NV + 1, HW)]
    P = torch.from_numpy(K @ np.concatenate([R, t], -1)).float()[None].repeat(B, 1, 1, 1)
    mask = np.array([[1, 1, 1, 1], [0, 1, 0, 1]], dtype=np.uint8)
    m = TR.AlgebraicTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(inp["images"].to(DEV), P.to(DEV), {"view_mask": mask})
    m.masked_training = True
    seen = {}
    fwd, bwd = TR._AlgTrainPlan.forward, TR._AlgTrainPlan.backward

    def forward(self, x):
        out = fwd(self, x)
        seen["hm"], seen["conf_raw"] = out[0].detach().cpu().double(), out[1].detach().cpu().double()
        return out

    def backward(self, g_hm, g_conf):
        seen["g_hm"], seen["g_conf"] = g_hm.detach().cpu(), g_conf.detach().cpu()
        return bwd(self, g_hm, g_conf)
    monkeypatch.setattr(TR._AlgTrainPlan, "forward", forward)
    monkeypatch.setattr(TR._AlgTrainPlan, "backward", backward)
    kp3, kp2, hm, conf = m(inp["images"].to(DEV), P.to(DEV), {"view_mask": mask})
    GX = torch.randn(B, J, 3, generator=torch.Generator().manual_seed(3))
    (kp3 * GX.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    on = torch.from_numpy(mask).bool()
    assert bool((conf.detach().cpu()[~on] == 0).all()) and bool((conf.detach().cpu()[on] > 1e-5).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.requires_grad)
    # the tail in fp64, sample by sample on the valid views
    h, w = seen["hm"].shape[2:]
    h64 = seen["hm"].clone().requires_grad_(True)
    c64 = seen["conf_raw"].clone().requires_grad_(True)
    k64, _ = O.integrate_tensor_2d(h64 * 1.0, True, dtype=torch.float64)
    k64 = k64.reshape(B, NV, J, 2) * torch.tensor([HW / w, HW / h], dtype=torch.float64)
    cr = c64.reshape(B, NV, J)
    x64 = []
    for b in range(B):
        idx = np.nonzero(mask[b])[0].tolist()
        cn = cr[b, idx] / cr[b, idx].sum(0, keepdim=True) + 1e-5
        x64.append(O.triangulate_batch_of_points(P[b:b + 1, idx].double(), k64[b:b + 1, idx], cn[None], dtype=torch.float64))
    x64 = torch.cat(x64)
    (x64 * GX.double()).sum().backward()
    from gpu_util import rel_err
    print("keypoints_3d: max|d|/max|ref| = %.3e (gate 1e-4); d/d heatmap logits %.3e, d/d raw confidences %.3e (gate 2e-3)" % (
        rel_err(kp3.detach().cpu(), x64.detach().float()), rel_err(seen["g_hm"], h64.grad.float()), rel_err(seen["g_conf"], c64.grad.float())))
    check("train-alg/masked tail keypoints_3d vs fp64 on the valid views", kp3.detach().cpu(), x64.detach().float(), 1e-4)
    g_hm, g_conf = seen["g_hm"].reshape(B, NV, J, h, w), seen["g_conf"].reshape(B, NV, J)
    assert bool((g_hm[~on] == 0).all()) and bool((g_conf[~on] == 0).all()), "a masked view's heatmaps or confidences received a gradient"
    assert float(g_hm[on].abs().max()) > 0 and float(g_conf[on].abs().max()) > 0
    e = check("train-alg/masked tail d/d heatmap logits vs fp64 on the valid views", seen["g_hm"], h64.grad.float(), 2e-3)
    print("d/d heatmap logits: max|d|/max|ref| = %.3e" % e)
    e = check("train-alg/masked tail d/d raw confidences vs fp64 on the valid views", seen["g_conf"], c64.grad.float(), 2e-3)
    print("d/d raw confidences: max|d|/max|ref| = %.3e" % e)
    # the functional op: the flag lifts the refusal, the default keeps it
    pts = kp2.detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        multiview.triangulate_batch_of_points(P.to(DEV), pts, conf.detach(), view_mask=mask)
    x = multiview.triangulate_batch_of_points(P.to(DEV), pts, conf.detach(), view_mask=mask, masked_backward=True)
    x.sum().backward()
    assert bool((pts.grad.cpu()[~on] == 0).all()) and float(pts.grad.abs().max()) > 0
