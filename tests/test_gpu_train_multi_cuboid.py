"""GPU (-m gpu): training with several cuboids per frame (``multi_cuboid_training``) -- lt_unproject_grid_indexed_fwd / lt_unproject_indexed_bwd inside the
recorded step of VolumetricTriangulationNet.
  * ONE WHOLE STEP against the step the REFERENCE ITSELF takes on CPU on the frames repeated per cuboid, with its backbone run on the distinct frames only
    (tests/golden/train_step_multi_cuboid.npz, tools/make_golden_train_multi_cuboid.py): the gates of tests/test_gpu_train_many_views.py;
  * one tape, many assignments: another frame_of of the same P replays the same tape, bit for bit a fresh model's first step with that assignment;
  * frame_of = 0 .. F-1 is the plain step bit for bit; with masked_training, an all-ones mask is the unmasked multi-cuboid step bit for bit;
  * the default refuses; the autograd node of op.unproject_heatmaps(indexed_backward=True) against the fp64 statement."""
import os
import re

import numpy as np
import pytest
import torch

from gpu_util import check, record
from oracle import spec, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ZERO_GRAD = re.compile(r"^volume_net\.(.*\.(block\.0|res_branch\.0|res_branch\.3|skip_con\.0)|output_layer)\.bias$")


def test_whole_multi_cuboid_training_step_vs_reference(golden_dir):
    """model.train() with multi_cuboid_training; F = 2 frames, frame_of = (0, 1, 1, 0, 1); MAE(kp * 0.1) + 0.01 * VolumetricCELoss on the P = 5 joints sets;
    backward; Adam -- keypoints at 1e-4 + 2 x kp_noise, every parameter's gradient at 1e-3 + 4 x its stored noise, the BatchNorm running statistics (over
    the F frames on both sides) at 1e-4 and the parameters after the step at 2e-2 lr, against the reference's own step on CPU."""
    import lt_train
    from mvn.models import loss as L
    from mvn.models.triangulation import VolumetricTriangulationNet
    from test_gpu_models import _cameras
    G = np.load(os.path.join(golden_dir, "train_step_multi_cuboid.npz"))
    c = {str(k): int(v) for k, v in zip(G["case_keys"], G["case"])}
    method, vs, fs = str(G["method"]), int(G["vol_stride"]), int(G["feat_stride"])
    fof, rep = G["frame_of"], G["frame_rep"]
    P, F = c["B"], len(rep)
    assert fof.tolist() == [0, 1, 1, 0, 1] and rep.tolist() == [0, 1] and P == 5 and c["NV"] == 4
    cfg = synth.vol_config(c["nl"], c["V"], method, 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(c["nl"], 17, False), seed=c["seed"], sharpen=60.0, basic_block=c["nl"] < 50)
    inp = synth.make_inputs(P, c["NV"], c["H"], seed=c["seed"], inside=False)          # sample p: cuboid p; frame f's images: those of sample rep[f]
    images = inp["images"][torch.from_numpy(rep.astype(np.int64))].contiguous()
    TAG = "[multi_cuboid] "
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    m.train()
    m.multi_cuboid_training = True
    lr, pf_lr, vn_lr = [float(v) for v in G["lrs"]]
    opt = lt_train.Adam([{"params": list(m.backbone.parameters())}, {"params": list(m.process_features.parameters()), "lr": pf_lr},
                         {"params": list(m.volume_net.parameters()), "lr": vn_lr}], lr=lr)
    batch = {"cameras": _cameras(inp, F), "pred_keypoints_3d": inp["pred_keypoints_3d"], "cuboid_frame": fof}
    np.random.seed(c["seed"] + 100)
    kp, feats, vols, conf, cuboids, cvs, bps = m(images.to(DEV), torch.zeros(F, c["NV"], 3, 4, device=DEV), batch)
    assert kp.shape[0] == P and vols.shape[0] == P and cvs.shape[0] == P and bps.shape[0] == P and len(cuboids) == P and feats.shape[0] == F
    kp_noise, loss_noise = float(G["kp_noise"]), float(G["loss_noise"])
    d = (kp.detach().cpu().double() - torch.from_numpy(G["kp"]).double()).abs() / torch.from_numpy(G["kp"]).double().abs().clamp(min=1.0)
    record(TAG + "train/step forward keypoints (train-mode BN), rel with 1 mm floor", {"err": float(d.max()), "tol": 1e-4 + 2 * kp_noise, "reference_self_noise": kp_noise})
    print("keypoints: err %.3e, gate %.3e (reference self-noise %.3e)" % (float(d.max()), 1e-4 + 2 * kp_noise, kp_noise))
    assert float(d.max()) <= 1e-4 + 2 * kp_noise, float(d.max())
    check(TAG + "train/step forward volumes", vols.detach().cpu()[:, :, ::vs, ::vs, ::vs], G["vol_sub"], 1e-3 + 10 * kp_noise)
    by_cuboid = feats.detach().cpu()[torch.from_numpy(fof.astype(np.int64))]          # the fixture holds the reference's features, one set per cuboid
    check(TAG + "train/step forward features", by_cuboid.reshape(P * c["NV"], *feats.shape[2:])[:, :, ::fs, ::fs], G["feat_sub"], 1e-4)
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
            # a convolution bias in front of a training-mode BatchNorm or the output layer's bias under the softmax: the exact gradient is 0
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
    # running statistics (momentum 0.1, unbiased variance): over the F frames
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


# ---- one tape, many assignments -------------------------------------------------------------------------------------------------------------------------
F, P, NV = 2, 5, 4


def _vol_model(method="softmax", precision="fp32", multi=True, masked=False, seed=12):
    from mvn.models.triangulation import VolumetricTriangulationNet
    cfg = synth.vol_config(18, 32, method, 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(18, 17, method.startswith("conf")), seed=seed, sharpen=60.0, basic_block=True)
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    m.train()
    m.train_precision = precision
    m.multi_cuboid_training, m.masked_training = multi, masked
    return m


_INP = {}


def _inputs():
    """F frames of images and P base points, made once and never written to."""
    if not _INP:
        inp = synth.make_inputs(P, NV, 128, seed=31, inside=False)
        _INP.update(inp, images=inp["images"][:F].contiguous())
    return _INP


def _step(m, frame_of, mask=None, n_kp=None):
    """One training forward / backward on the F frames: ({name: gradient (cpu)}, the forward's 7-tuple).  frame_of None: the plain step on the F frames
    with the first n_kp base points."""
    from mvn.models import loss as L
    from test_gpu_models import _cameras
    inp = _inputs()
    n = len(frame_of) if frame_of is not None else n_kp
    kp3d = inp["pred_keypoints_3d"][:n]
    batch = {"cameras": _cameras(inp, F), "pred_keypoints_3d": kp3d}
    if frame_of is not None:
        batch["cuboid_frame"] = frame_of
    if mask is not None:
        batch["view_mask"] = mask
    gt = torch.as_tensor(np.asarray(kp3d))[:, :, :3].float().to(DEV)
    val = torch.ones(n, 17, 1, device=DEV)
    np.random.seed(77)
    out = m(inp["images"].to(DEV), None, batch)
    kp, _, vols, _, _, cvs, _ = out
    loss = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val) + 0.01 * L.VolumetricCELoss()(cvs, vols, gt, val)
    for p in m.parameters():
        p.grad = None
    loss.backward()
    torch.cuda.synchronize()
    return {n_: p.grad.detach().float().cpu().numpy().copy() for n_, p in m.named_parameters() if p.grad is not None}, out


def _same(a, b, what):
    assert set(a) == set(b) and len(a) > 50 and all(np.isfinite(v).all() for v in a.values())
    for n in a:
        assert np.array_equal(a[n], b[n]), "%s: gradient of %s differs" % (what, n)


def test_one_tape_serves_every_assignment_and_the_default_refuses():
    """Two steps with two assignments of the same P run ONE plan and ONE tape with an unchanged number of recorded operations, and the second step's
    parameter gradients are BITWISE those of a fresh model's first (recording) step with that assignment: frame_of reaches the replayed launches through the
    geometry block alone.  Without the flag the step is refused with the message it always had."""
    m = _vol_model()
    a, b = [0, 1, 1, 0, 1], [1, 1, 0, 0, 0]
    g1, o1 = _step(m, a)
    plans = list(m._train_plans.values())
    book = (len(plans), id(plans[0]), id(plans[0].tape), len(plans[0].tape.fwd_ops), plans[0].cuboids)
    assert max(float(np.abs(v).max()) for n, v in g1.items() if n.startswith("backbone.")) > 0          # the gradient did pass the unprojection
    g2, o2 = _step(m, b)
    plans = list(m._train_plans.values())
    assert book == (len(plans), id(plans[0]), id(plans[0].tape), len(plans[0].tape.fwd_ops), plans[0].cuboids) and book[0] == 1 and book[4] == P, book
    fresh, of = _step(_vol_model(), b)
    _same(g2, fresh, "second step on the recorded tape against a fresh recording")
    assert torch.equal(o2[0], of[0]) and torch.equal(o2[2], of[2])
    assert any(not np.array_equal(g1[n], g2[n]) for n in g1), "another assignment, the same gradients"
    with pytest.raises(NotImplementedError, match="no indexed unprojection backward"):
        _step(_vol_model(multi=False), a)


def test_one_cuboid_per_frame_is_the_plain_step():
    """frame_of = (0, 1): parameter gradients, keypoints and volumes bit for bit those of the plain training step (another plan key, another pair of entries,
    the same arithmetic); and without cuboid_frame the model takes the plain plan, under the key it always had."""
    plain, po = _step(_vol_model(multi=False), None, n_kp=F)
    mm = _vol_model()
    ar, ao = _step(mm, [0, 1])
    _same(plain, ar, "frame_of = arange against the plain step")
    assert torch.equal(po[0], ao[0]) and torch.equal(po[2], ao[2])
    _step(mm, None, n_kp=F)
    keys = list(mm._train_plans)
    assert len(keys) == 2 and keys[0][-2:] == ("cuboids", F) and keys[0][:-2] == keys[1]


def test_all_ones_mask_is_the_unmasked_multi_cuboid_step():
    a = [0, 1, 1, 0, 1]
    plain, po = _step(_vol_model(), a)
    both = _vol_model(masked=True)
    ones, oo = _step(both, a, mask=np.ones((F, NV), dtype=np.uint8))
    _same(plain, ones, "all-ones mask against the unmasked multi-cuboid step")
    assert torch.equal(po[0], oo[0]) and torch.equal(po[2], oo[2])
    with pytest.raises(NotImplementedError, match="no masked backward"):          # both flags are required
        _step(_vol_model(masked=False), a, mask=np.ones((F, NV), dtype=np.uint8))
    # a real mask: finite, and a masked view's images still reach the backbone's statistics but its features get no gradient from the volume
    g, _ = _step(both, a, mask=np.array([[1, 0, 1, 1], [0, 1, 1, 1]], dtype=np.uint8))
    assert all(np.isfinite(v).all() for v in g.values()) and any(not np.array_equal(g[n], ones[n]) for n in g)


@pytest.mark.parametrize("agg", ["sum", "max", "softmax", "conf"])
def test_autograd_node_vs_the_fp64_statement(agg):
    """op.unproject_heatmaps(frame_index=..., indexed_backward=True): the forward is the inference path's bits, the gradients of the heatmaps and the
    confidences are the fp64 statement's at 1e-4 of max|ref|; the default still refuses."""
    import unproject_bwd_indexed_ref as X
    from mvn.utils import op
    hm, proj, conf, cv, G = X.gaussian_case(4)
    fof = list(X.GATE_FRAME_OF)
    f = hm.to(DEV).requires_grad_(True)
    cf = conf.to(DEV).requires_grad_(True) if agg == "conf" else None
    with pytest.raises(NotImplementedError, match="no indexed backward"):
        op.unproject_heatmaps(f, proj.to(DEV), cv.to(DEV), agg, cf, frame_index=fof)
    vol = op.unproject_heatmaps(f, proj.to(DEV), cv.to(DEV), agg, cf, frame_index=fof, indexed_backward=True)
    with torch.no_grad():
        assert torch.equal(vol, op.unproject_heatmaps(f, proj.to(DEV), cv.to(DEV), agg, cf, frame_index=fof))
    (vol * G.to(DEV)).sum().backward()
    rf, rc = X.indexed_ref_backward(hm, proj, cv, G, agg, fof, conf)
    check("op/unproject indexed autograd %s: d/d heatmaps" % agg, f.grad.cpu(), rf, 1e-4)
    if agg == "conf":
        check("op/unproject indexed autograd conf: d/d confidences", cf.grad.cpu(), rc, 1e-4)
