"""GPU (-m gpu): training the 2D backbone on heatmaps.
  * ONE WHOLE STEP of get_pose_net(...) alone (ResNet-18, train(), loss.HeatmapMSELoss, lt_train.Adam) against the step the REFERENCE ITSELF takes on CPU
    (tests/golden/train_step_heatmap2d.npz ``b/``, tools/make_golden_heatmap2d.py), under the rules of tests/test_gpu_finetune.py: logits within
    1e-4 + 2 x the reference's self-noise, the loss within 1e-4 + 2 x its noise, every parameter gradient within 1e-3 + 4 x its stored self-noise (exact-zero
    gradients excepted), the gradient norm within 2e-3, running statistics within 1e-4, parameters after Adam within 2e-2 lr units; a second step replays;
  * AlgebraicTriangulationNet with MSESmooth(3D) + lam x HeatmapMSELoss(normalize=True) on the RETURNED softmaxed heatmaps against ``c/`` (gradients against
    the reference's fp64 step, as the existing algebraic step tests gate them: its fp32 torch.svd backward alone is 1.2e-3 off); with lam = 0 the step's
    gradients are, bit for bit, those of a step that never touches the heatmaps;
  * the surface: eval() unchanged, V2VModel still refuses train(), an older forward cannot be backpropagated, one act16 step is finite."""
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import check, record
from oracle import spec, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "train_step_heatmap2d.npz"))


def _sub129(t):
    f = t.detach().double().cpu().reshape(-1)
    return f[::max(1, f.numel() // 129)][:129]


def _backbone_case(G):
    c = {str(k): int(v) for k, v in zip(G["b/case_keys"], G["b/case"])}          # the seed is the fixture's (the generator picks one the reference is stable on)
    assert {k: v for k, v in c.items() if k != "seed"} == dict(nl=18, N=4, H=128, J=17), "the fixture was generated at another shape"
    cfg = synth.alg_config(c["nl"], False).model.backbone
    cfg.alg_confidences, cfg.vol_confidences = False, False
    sd = synth.make_state_dict(spec.pose_resnet_spec(c["nl"], c["J"]), seed=c["seed"], basic_block=True)
    images = synth.make_inputs(1, c["N"], c["H"], seed=c["seed"], inside=False)["images"][0]
    return c, cfg, sd, images


def _backbone(cfg, sd, precision="fp32"):
    from mvn.models import pose_resnet
    m = pose_resnet.get_pose_net(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    m.train_precision = precision
    return m


def _check_gradients(G, pre, TAG, named, against64):
    """Every parameter gradient within 1e-3 + 4 x its stored self-noise of the reference's (fp64 step: ``against64``), the exact-zero-gradient exception,
    the set of parameters without a gradient, the gradient norm."""
    names, no_grad = [str(n) for n in G[pre + "names"]], [str(n) for n in G[pre + "no_grad"]]
    assert sorted(names + no_grad) == sorted(named)
    assert sorted(n for n, p in named.items() if p.grad is None) == sorted(no_grad), "the parameters without a gradient are not the fixture's"
    gn2, table, n_zero = 0.0, [], 0
    gnorm_ref = float(G[pre + "grad_norm"])
    for n in names:
        gr = named[n].grad.detach().double().cpu()
        ref_norm, ref_max, _ = [float(v) for v in G[pre + "gn/" + n]]
        noise = float(G[pre + "noise/" + n])
        gn2 += float(gr.pow(2).sum())
        if noise > 0.05:          # exact-zero gradients (a bias in front of a training-mode BatchNorm): rounding noise on both sides
            assert float(gr.abs().max()) <= 10 * ref_max + 1e-6 * gnorm_ref, (n, float(gr.abs().max()), ref_max)
            n_zero += 1
            continue
        n64, m64 = [float(v) for v in G[pre + "gn64/" + n]]
        e32 = max(float((_sub129(gr) - torch.from_numpy(G[pre + "g/" + n]).double()).abs().max()) / ref_max, abs(float(gr.norm()) - ref_norm) / ref_norm)
        e64 = max(float((_sub129(gr) - torch.from_numpy(G[pre + "g64/" + n]).double()).abs().max()) / m64, abs(float(gr.norm()) - n64) / n64)
        e = e64 if against64 else e32
        table.append((e / (1e-3 + 4 * noise), e, noise, n, e32, e64))
    table.sort(reverse=True)
    print(TAG, "worst parameter gradients (err / gate, err, reference self-noise, name, vs the fp32 step, vs the fp64 step):",
          *["%.2f %.2e %.2e %s %.2e %.2e" % t for t in table[:6]], sep="\n  ")
    errs = sorted(t[1] for t in table)
    record(TAG + "parameter gradients vs the reference's %s step (gate 1e-3 + 4 x reference self-noise)" % ("fp64" if against64 else "fp32"),
           {"worst_err_over_gate": table[0][0], "worst_err": errs[-1], "median_err": errs[len(errs) // 2], "parameters_compared": len(table),
            "zero_gradient_parameters": n_zero, "vs_the_fp32_step_worst": max(t[4] for t in table), "vs_the_fp64_step_worst": max(t[5] for t in table)})
    assert table[0][0] <= 1.0, table[:6]
    gn = float(np.sqrt(gn2))
    gref = float(G[pre + "grad_norm64"]) if against64 else gnorm_ref
    print(TAG, "global gradient norm", gn, "reference", gnorm_ref, "fp64", float(G[pre + "grad_norm64"]))
    assert abs(gn - gref) <= 2e-3 * gnorm_ref, (gn, gref)
    return names, gn


def _check_state_after_step(G, pre, TAG, m, named, names, lr):
    bufs = dict(m.named_buffers())
    w_rs = 0.0
    for key in G.files:
        if key.startswith(pre + "rs/"):
            ref = torch.from_numpy(G[key]).double()
            w_rs = max(w_rs, float((_sub129(bufs[key[len(pre) + 3:]]) - ref).abs().max() / ref.abs().max().clamp(min=1e-30)))
    record(TAG + "BatchNorm running statistics", {"err": w_rs, "tol": 1e-4})
    assert w_rs <= 1e-4, w_rs
    w_p, w_name, n_known = 0.0, None, 0
    for n in names:
        if float(G[pre + "noise/" + n]) > 0.05:
            continue
        ref = torch.from_numpy(G[pre + "p1/" + n]).double()
        gs = torch.from_numpy(G[pre + "g/" + n]).double().abs()
        known = gs > 100 * (float(G[pre + "noise/" + n]) + 1e-3) * float(G[pre + "gn/" + n][1])
        n_known += int(known.sum())
        e = float(((_sub129(named[n]) - ref).abs() * known).max()) / lr          # in units of one full Adam step
        if e > w_p:
            w_p, w_name = e, n
    record(TAG + "parameters after Adam, worst |d| in units of lr", {"err": w_p, "tol": 2e-2, "name": w_name, "elements_compared": n_known})
    assert w_p <= 2e-2 and n_known > 0, (w_p, w_name, n_known)


def test_backbone_training_step_vs_reference(G):
    import lt_train
    from mvn.models.loss import HeatmapMSELoss
    pre, TAG = "b/", "heatmap2d-train/backbone "
    c, cfg, sd, images = _backbone_case(G)
    m = _backbone(cfg, sd)
    lr = float(G[pre + "lr"])
    opt = lt_train.Adam([p for p in m.parameters() if p.requires_grad], lr=lr)
    x = images.to(DEV)
    hm, feats, algc, volc = m(x)
    assert hm.shape == (4, 17, 32, 32) and hm.requires_grad and hm.grad_fn is not None
    assert feats.shape == (4, 256, 32, 32) and feats.grad_fn is None and not feats.requires_grad and algc is None and volc is None
    ref = torch.from_numpy(G[pre + "hm_sub"]).double()
    floor, hm_noise, loss_noise = float(G[pre + "hm_floor"]), float(G[pre + "hm_noise"]), float(G[pre + "loss_noise"])
    e = float(((hm.detach().cpu().double()[:, :, ::2, ::2] - ref).abs() / ref.abs().clamp(min=floor)).max())
    record(TAG + "forward heatmap logits (train-mode BN), rel with the fixture's floor", {"err": e, "tol": 1e-4 + 2 * hm_noise, "reference_self_noise": hm_noise})
    assert e <= 1e-4 + 2 * hm_noise, e
    check(TAG + "forward features", feats.cpu()[:, ::8, ::4, ::4], G[pre + "feat_sub"], 1e-4)
    gt2d, val = torch.from_numpy(G[pre + "gt2d"].copy()), torch.from_numpy(G[pre + "val"])
    gt2d[val[..., 0] == 0] = float("nan")          # a missing annotation: never read
    crit = HeatmapMSELoss(sigma=float(G[pre + "sigma"]), normalize=False)
    loss = crit(hm, gt2d.to(DEV), val.to(DEV))
    print(TAG, "loss", float(loss.detach()), float(G[pre + "loss"]))
    assert abs(float(loss.detach()) - float(G[pre + "loss"])) <= (1e-4 + 2 * loss_noise) * float(G[pre + "loss"]), (float(loss.detach()), float(G[pre + "loss"]))
    opt.zero_grad()
    loss.backward()
    named = dict(m.named_parameters())
    names, _ = _check_gradients(G, pre, TAG, named, against64=False)
    opt.step()
    torch.cuda.synchronize()
    _check_state_after_step(G, pre, TAG, m, named, names, lr)
    assert all(int(mod.num_batches_tracked) == 1 for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm))
    # a second step replays the tape: one plan, nothing recorded anew
    plans = list(m._train_plans.values())
    assert len(plans) == 1
    tape, n_fwd, n_bwd = plans[0].tape, len(plans[0].tape.fwd_ops), len(plans[0].tape.bwd_ops)
    hm2 = m(x)[0]
    loss2 = crit(hm2, gt2d.to(DEV), val.to(DEV))
    opt.zero_grad()
    loss2.backward()
    opt.step()
    torch.cuda.synchronize()
    plans = list(m._train_plans.values())
    assert len(plans) == 1 and plans[0].tape is tape and (len(tape.fwd_ops), len(tape.bwd_ops)) == (n_fwd, n_bwd)
    assert float(loss2.detach()) < float(loss.detach()) and all(torch.isfinite(p.grad).all() for p in named.values())
    # the replayed forward reads the updated parameters: same result as a fresh recording on a second model loaded with the state after two steps
    m2 = _backbone(cfg, m.state_dict())
    hm3 = m(x)[0].detach()
    check(TAG + "replayed forward vs a fresh recording with the updated weights", hm3.cpu(), m2(x)[0].detach().cpu(), 1e-6)


def _alg_case():
    c = dict(nl=18, B=2, NV=3, H=128, seed=21)
    cfg = synth.alg_config(c["nl"], True)
    cfg.model.heatmap_multiplier = 1.0
    cfg.model["heatmap_multiplier"] = 1.0
    sd = synth.make_state_dict(spec.alg_net_spec(c["nl"], 17, True), seed=c["seed"], basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    return c, cfg, sd, inp


def _alg_model(cfg, sd):
    from mvn.models.triangulation import AlgebraicTriangulationNet
    m = AlgebraicTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    return m


def _alg_losses(G, out, c):
    from mvn.models import loss as L
    pre = "c/"
    kp3, kp2, hm, conf = out
    gt, val = torch.from_numpy(G[pre + "gt"]).to(DEV), torch.from_numpy(G[pre + "val"]).to(DEV)
    gt2d = torch.from_numpy(G[pre + "gt2d"]).to(DEV)
    val2d = val[:, None].repeat(1, c["NV"], 1, 1)
    l3 = L.KeypointsMSESmoothLoss(400)(kp3 * 0.1, gt * 0.1, val)
    lh = L.HeatmapMSELoss(sigma=float(G[pre + "sigma"]), normalize=True)(hm, gt2d, val2d)
    return l3, lh


def test_algebraic_step_with_heatmap_loss_vs_reference(G):
    import lt_train
    pre, TAG = "c/", "heatmap2d-train/alg + heatmap loss "
    c, cfg, sd, inp = _alg_case()
    m = _alg_model(cfg, sd)
    lr, lam = float(G[pre + "lr"]), float(G[pre + "lam"])
    opt = lt_train.Adam([p for p in m.parameters() if p.requires_grad], lr=lr)
    P = torch.from_numpy(G[pre + "P"]).to(DEV)
    out = m(inp["images"].to(DEV), P, {})
    kp3, kp2, hm, conf = out
    assert hm.requires_grad and hm.grad_fn is not None
    kp_noise, loss_noise = float(G[pre + "kp_noise"]), float(G[pre + "loss_noise"])
    d = (kp3.detach().cpu().double() - torch.from_numpy(G[pre + "kp3"]).double()).abs() / torch.from_numpy(G[pre + "kp3"]).double().abs().clamp(min=1.0)
    assert float(d.max()) <= 1e-4 + 2 * kp_noise, float(d.max())
    check(TAG + "forward heatmaps", hm.detach().cpu().reshape(c["B"] * c["NV"], *hm.shape[2:])[:, :, ::2, ::2], G[pre + "hm_sub"], 1e-4)
    l3, lh = _alg_losses(G, out, c)
    loss = l3 + lam * lh
    print(TAG, "loss", float(loss.detach()), float(G[pre + "loss"]), "3D", float(l3.detach()), float(G[pre + "loss3d"]), "heatmap", float(lh.detach()), float(G[pre + "loss_hm"]))
    assert abs(float(lh.detach()) - float(G[pre + "loss_hm"])) <= 1e-4 * float(G[pre + "loss_hm"])
    assert abs(float(loss.detach()) - float(G[pre + "loss"])) <= (1e-4 + 2 * loss_noise) * float(G[pre + "loss"]), (float(loss.detach()), float(G[pre + "loss"]))
    opt.zero_grad()
    loss.backward()
    named = dict(m.named_parameters())
    names, gn = _check_gradients(G, pre, TAG, named, against64=True)
    n3, nh = [float(v) for v in G[pre + "term_grad_norms"]]
    assert abs(gn - n3) >= 0.1 * n3 and abs(gn - lam * nh) >= 0.1 * lam * nh          # both terms are in this gradient
    opt.step()
    torch.cuda.synchronize()
    _check_state_after_step(G, pre, TAG, m, named, names, lr)


def test_lambda_zero_keeps_the_existing_steps_bits(G, monkeypatch):
    """A step whose loss never touches the returned heatmaps backpropagates through lt_softargmax2d_bwd, the entry it always took; the same step with
    0 x HeatmapMSELoss added (an all-zero gradient on the heatmaps, through lt_softargmax2d_bwd_full) gives the same gradients bit for bit."""
    c, cfg, sd, inp = _alg_case()
    P = torch.from_numpy(G["c/P"]).to(DEV)
    seen = []
    lib = H.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("lt_softargmax2d_bwd"):
                seen.append(name)
            return getattr(lib, name)
    grads = []
    for touch in (False, True):
        m = _alg_model(cfg, sd)
        out = m(inp["images"].to(DEV), P, {})
        l3, lh = _alg_losses(G, out, c)
        loss = l3 + 0.0 * lh if touch else l3
        del seen[:]
        monkeypatch.setattr(H, "lib", lambda: Spy())
        loss.backward()
        monkeypatch.undo()
        assert seen == (["lt_softargmax2d_bwd_full"] if touch else ["lt_softargmax2d_bwd"]), seen
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    assert all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0]), [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])][:5]
    assert float(sum(g.abs().sum() for g in grads[0].values())) > 0


def test_surface(G):
    from mvn.models.loss import HeatmapMSELoss
    from mvn.models.v2v import V2VModel
    c, cfg, sd, images = _backbone_case(G)
    x = images.to(DEV)
    gt2d, val = torch.from_numpy(G["b/gt2d"]).to(DEV), torch.from_numpy(G["b/val"]).to(DEV)
    crit = HeatmapMSELoss(sigma=2.0)
    # eval() is what it was: the inference plan, untouched by a training forward in between
    m = _backbone(cfg, sd)
    m.eval()
    with torch.no_grad():
        before = [t.clone() for t in m(x)[:2]]
    m.train()
    hm_old = m(x)[0]
    hm_new = m(x)[0]
    with pytest.raises(RuntimeError, match="LATEST"):          # only the latest forward can be backpropagated
        crit(hm_old, gt2d, val).backward()
    crit(hm_new, gt2d, val).backward()
    m.load_state_dict(sd, strict=True)
    m.eval()
    with torch.no_grad():
        after = m(x)
    assert after[2] is None and after[3] is None and all(torch.equal(a, b) for a, b in zip(before, after[:2]))
    assert not after[0].requires_grad
    # V2VModel keeps its refusal
    v = V2VModel(32, 17).to(DEV).train()
    with pytest.raises(NotImplementedError):
        v(torch.zeros(1, 32, 16, 16, 16, device=DEV))
    # frozen parameters: no gradient, the others train
    m = _backbone(cfg, sd)
    m.conv1.requires_grad_(False); m.bn1.requires_grad_(False)
    crit(m(x)[0], gt2d, val).backward()
    assert m.conv1.weight.grad is None and m.bn1.weight.grad is None and m.final_layer.weight.grad is not None and m.layer1[0].conv1.weight.grad is not None
    with pytest.raises(ValueError, match="train_precision"):
        m.train_precision = "fp8v2v"
        m(x)
    # both confidence heads: alg_confidences is differentiable, vol_confidences comes back without a grad_fn and its head ends the step without gradients
    from mvn.models import pose_resnet
    cfg2 = synth.alg_config(18, True).model.backbone
    cfg2.alg_confidences, cfg2.vol_confidences = True, True
    torch.manual_seed(3)
    m = pose_resnet.get_pose_net(cfg2, device=DEV).to(DEV).train()
    hm, feats, algc, volc = m(x)
    assert algc.shape == (4, 17) and algc.requires_grad and volc.shape == (4, 32) and volc.grad_fn is None and not volc.requires_grad and feats.grad_fn is None
    (crit(hm, gt2d, val) + algc.sum()).backward()
    named = dict(m.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n.startswith("vol_confidences."))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in named.items() if not n.startswith("vol_confidences."))
    assert float(named["alg_confidences.head.4.weight"].grad.abs().max()) > 0


def test_backbone_act16_step_is_finite(G):
    from mvn.models.loss import HeatmapMSELoss
    c, cfg, sd, images = _backbone_case(G)
    m = _backbone(cfg, sd, precision="act16")
    gt2d, val = torch.from_numpy(G["b/gt2d"]).to(DEV), torch.from_numpy(G["b/val"]).to(DEV)
    loss = HeatmapMSELoss(sigma=float(G["b/sigma"]))(m(images.to(DEV))[0], gt2d, val)
    loss.backward()
    gn = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in m.parameters() if p.grad is not None)))
    assert np.isfinite(float(loss.detach())) and np.isfinite(gn) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    record("heatmap2d-train/backbone act16 step, deviation from the reference's fp32 step",
           {"loss": float(loss.detach()), "loss_rel_dev": abs(float(loss.detach()) - float(G["b/loss"])) / float(G["b/loss"]),
            "grad_norm": gn, "grad_norm_rel_dev": abs(gn - float(G["b/grad_norm"])) / float(G["b/grad_norm"])})
    print("act16: loss %.6f (fp32 reference %.6f), gradient norm %.4e (%.4e)" % (float(loss.detach()), float(G["b/loss"]), gn, float(G["b/grad_norm"])))
