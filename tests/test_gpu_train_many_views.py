"""GPU (-m gpu): the training step of VolumetricTriangulationNet with more than eight camera views -- the unprojection backward's many-view kernels
inside the recorded step.
  * ONE WHOLE STEP at 10 views against the step the REFERENCE ITSELF takes on CPU (tests/golden/train_step_nv10.npz,
    tools/make_golden_train_many_views.py): the body and every gate of tests/test_gpu_train.py::test_whole_training_step_vs_reference, driven by the
    constants the fixture stores;
  * a 9-view step recorded twice and replayed, fp32 and act16: bitwise-equal parameter gradients."""
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


def test_whole_training_step_at_ten_views_vs_reference(golden_dir):
    """model.train(); forward; MAE(kp * 0.1) + 0.01 * VolumetricCELoss; backward; Adam (train.py:148-243, :430-437) at 10 views -- every parameter's
    gradient, the BatchNorm running statistics and the parameters after the step against the reference's own step on CPU, within the reference's
    measured self-noise."""
    import lt_train
    from mvn.models import loss as L
    from mvn.models.triangulation import VolumetricTriangulationNet
    from test_gpu_models import _cameras
    G = np.load(os.path.join(golden_dir, "train_step_nv10.npz"))
    c = {str(k): int(v) for k, v in zip(G["case_keys"], G["case"])}
    method, vs, fs = str(G["method"]), int(G["vol_stride"]), int(G["feat_stride"])
    assert c["NV"] > 8
    cfg = synth.vol_config(c["nl"], c["V"], method, 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(c["nl"], 17, False), seed=c["seed"], sharpen=60.0, basic_block=c["nl"] < 50)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    TAG = "[nv%d] " % c["NV"]
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    m.train()
    lr, pf_lr, vn_lr = [float(v) for v in G["lrs"]]
    opt = lt_train.Adam([{"params": list(m.backbone.parameters())}, {"params": list(m.process_features.parameters()), "lr": pf_lr},
                         {"params": list(m.volume_net.parameters()), "lr": vn_lr}], lr=lr)
    batch = {"cameras": _cameras(inp, c["B"]), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    np.random.seed(c["seed"] + 100)
    kp, feats, vols, conf, cuboids, cvs, bps = m(inp["images"].to(DEV), torch.zeros(c["B"], c["NV"], 3, 4, device=DEV), batch)
    # the reference's own deviation between 1 and 8 threads / under a 1e-6 relative change of the images rides on every gate below
    kp_noise, loss_noise = float(G["kp_noise"]), float(G["loss_noise"])
    d = (kp.detach().cpu().double() - torch.from_numpy(G["kp"]).double()).abs() / torch.from_numpy(G["kp"]).double().abs().clamp(min=1.0)
    record(TAG + "train/step forward keypoints (train-mode BN), rel with 1 mm floor", {"err": float(d.max()), "tol": 1e-4 + 2 * kp_noise, "reference_self_noise": kp_noise})
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
            # a convolution bias in front of a training-mode BatchNorm (V2V's Conv3d / ConvTranspose3d layers, v2v.py:10-16, :57-61) or
            # the output layer's bias under the softmax: the exact gradient is 0, both sides hold rounding noise of their channel sums
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
    for n in G["no_grad"]:
        assert named[str(n)].grad is None
    gn = float(np.sqrt(gn2))
    assert abs(gn - float(G["grad_norm"])) <= 2e-3 * float(G["grad_norm"]), (gn, float(G["grad_norm"]))
    record(TAG + "train/step global gradient norm", {"ours": gn, "reference": float(G["grad_norm"])})
    # running statistics (momentum 0.1, unbiased variance)
    bufs = dict(m.named_buffers())
    w_rs = 0.0
    for key in G.files:
        if key.startswith("rs/"):
            b = bufs[key[3:]].detach().double().cpu().reshape(-1)
            sub = b[::max(1, b.numel() // 129)][:129]
            ref = torch.from_numpy(G[key]).double()
            w_rs = max(w_rs, float((sub - ref).abs().max() / ref.abs().max().clamp(min=1e-30)))
    record(TAG + "train/step BatchNorm running statistics", {"err": w_rs, "tol": 1e-4})
    assert w_rs <= 1e-4, w_rs
    # the Adam step: parameter deltas (the first step moves every element by ~lr * sign(g); compare the moved parameters)
    opt.step()
    torch.cuda.synchronize()
    # Adam's first step is lr * g / (|g| + 1e-8), a sign function of the gradient: elements whose reference gradient is below the
    # reference's own noise (exact zeros of dead channels on our side, 1e-12 on the reference's) can differ by 2 lr -- only the elements
    # the reference knows the sign of are compared (lt_adam_step itself: test_adam_step_vs_torch)
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
    assert w_p <= 2e-2, (w_p, w_name)
    assert n_known > 1000, n_known
    # the REPLAYED training forward reads the updated parameters: same result as a fresh model (fresh recording) with the new state dict
    np.random.seed(c["seed"] + 100)
    kp_replay = m(inp["images"].to(DEV), None, batch)[0].detach().clone()
    m2 = VolumetricTriangulationNet(cfg, device=DEV)
    m2.load_state_dict(m.state_dict(), strict=True)
    m2.to(DEV)
    m2.train()
    sd_before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    np.random.seed(c["seed"] + 100)
    kp_fresh = m2(inp["images"].to(DEV), None, batch)[0].detach()
    check(TAG + "train/step replayed forward after Adam vs a fresh recording with the updated weights", kp_replay.cpu(), kp_fresh.cpu(), 1e-6)
    assert float((kp_replay.cpu() - torch.from_numpy(G["kp"])).abs().max()) > 1e-3      # and the step did move the prediction
    # and the next inference forward uses the UPDATED weights (plan cache fingerprint)
    m.eval()
    with torch.no_grad():
        kp2 = m(inp["images"].to(DEV), None, batch)[0]
    assert torch.isfinite(kp2).all()


def _nine_view_grads(precision):
    """Two training forward / backward passes of a 9-view batch on a fresh model: {pass: {name: gradient (cpu)}}, and the plan bookkeeping."""
    from mvn.models import loss as L
    from mvn.models.triangulation import VolumetricTriangulationNet
    from test_gpu_models import _cameras
    cfg = synth.vol_config(18, 32, "softmax", 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(18, 17, False), seed=12, sharpen=60.0, basic_block=True)
    inp = synth.make_inputs(2, 9, 128, seed=31, inside=False)
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    m.train()
    m.train_precision = precision
    batch = {"cameras": _cameras(inp, 2), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    gt = torch.as_tensor(np.asarray(inp["pred_keypoints_3d"]))[:, :, :3].float().to(DEV)
    val = torch.ones(2, 17, 1, device=DEV)
    out, book = {}, {}
    for it in range(2):          # the second pass is the REPLAY of the recorded step
        np.random.seed(77)
        kp, _, vols, _, _, cvs, _ = m(inp["images"].to(DEV), None, batch)
        loss = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val) + 0.01 * L.VolumetricCELoss()(cvs, vols, gt, val)
        for p in m.parameters():
            p.grad = None
        loss.backward()
        torch.cuda.synchronize()
        out[it] = {n: p.grad.detach().float().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}
        plans = list(m._train_plans.values())
        book[it] = (len(plans), id(plans[0]), id(plans[0].tape), len(plans[0].tape.fwd_ops), plans[0].NV)
    return out, book


@pytest.mark.parametrize("precision", ["fp32", "act16"])
def test_nine_view_training_step_is_bitwise_repeatable_and_replays(precision):
    """Two independent recordings of a 9-view step (fresh models, same weights / inputs / rotations) and their replays give BITWISE identical parameter
    gradients -- the many-view unprojection backward adds in a fixed order like the rest of the step -- and the second step runs the plan the first one
    recorded (one plan, the same tape, no operation added)."""
    (a, book), (b, _) = _nine_view_grads(precision), _nine_view_grads(precision)
    assert set(a[0]) == set(b[0]) and len(a[0]) > 50
    assert all(np.isfinite(v).all() for v in a[0].values())
    assert max(float(np.abs(v).max()) for n, v in a[0].items() if n.startswith("backbone.")) > 0          # the gradient did pass the unprojection
    for it in (0, 1):
        for n in a[it]:
            assert np.array_equal(a[it][n], b[it][n]), "gradient of %s differs between two runs (step %d)" % (n, it)
    for n in a[0]:
        assert np.array_equal(a[0][n], a[1][n]), "replayed step differs from the recorded one: " + n
    assert book[0] == book[1] and book[0][0] == 1 and book[0][4] == 9, book
