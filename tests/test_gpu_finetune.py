"""GPU (-m gpu): fine-tuning with frozen parameters -- ``requires_grad_(False)`` ends the recorded backward where nothing trains.
  * ONE WHOLE STEP per setting against the step the REFERENCE ITSELF takes on CPU with the same parameters frozen (tests/golden/train_step_ft_*.npz,
    tools/make_golden_finetune.py): the body and every gate of tests/test_gpu_train.py::test_whole_training_step_vs_reference, and on top of them: no
    gradient for a frozen parameter, frozen parameters and untouched running statistics bit for bit, and what the tape recorded for the backward;
    each setting with the frozen backbone on the inference plan (where the setting allows it) and with LT_TRAIN_NO_FROZEN_PLAN=1 (on the tape);
  * the same for the algebraic model with a frozen trunk (train_step_alg_ft_trunk.npz, body of test_whole_algebraic_training_step_vs_reference);
  * act16 on the frozen-backbone setting within the limits of test_act16_step_with_a_frozen_backbone_batchnorm;
  * a changed frozen backbone is seen by the next step; a thawed one trains again and passes train_step.npz's forward gates."""
import os

import numpy as np
import pytest
import torch

from gpu_util import check, record
from oracle import spec, synth
from test_gpu_train import ZERO_GRAD, _train_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BN = torch.nn.modules.batchnorm._BatchNorm


def _bn_eval(mod):
    for c in mod.modules():
        if isinstance(c, BN):
            c.eval()


def _ft_backbone_eval(m):
    m.backbone.requires_grad_(False)
    m.train(); m.backbone.eval()


def _ft_backbone_trainbn(m):
    m.backbone.requires_grad_(False)
    m.train()


def _ft_bn_affine(m):
    m.train()
    for c in m.modules():
        if isinstance(c, BN):
            c.weight.requires_grad_(False); c.bias.requires_grad_(False)
    _bn_eval(m.backbone)


def _ft_v2v_only(m):
    m.backbone.requires_grad_(False); m.process_features.requires_grad_(False)
    m.train(); m.backbone.eval()


def _alg_ft_trunk(m):
    m.train()
    b = m.backbone
    for mod in (b.conv1, b.bn1, b.layer1, b.layer2, b.layer3):
        mod.requires_grad_(False)
        mod.eval()


SETTINGS = {"ft_backbone_eval": _ft_backbone_eval, "ft_backbone_trainbn": _ft_backbone_trainbn, "ft_bn_affine": _ft_bn_affine, "ft_v2v_only": _ft_v2v_only}
PLAN_ELIGIBLE = ("ft_backbone_eval", "ft_v2v_only")          # fully frozen backbone in eval(): the inference plan, unless the switch keeps it on the tape
BACKBONE_ROWS = {6 * s * s for s in (64, 32, 16, 8, 4)}          # rows (pixels x views) of the backbone's maps at 2 x 3 views of 128^2; V2V's are 2 * 4^k


def _sub129(t):
    f = t.detach().double().cpu().reshape(-1)
    return f[::max(1, f.numel() // 129)][:129]


def _case(G):
    c, cfg, sd, inp = _train_case()
    stored = {str(k): int(v) for k, v in zip(G["case_keys"], G["case"])}
    assert stored == c, "the fixture was generated at another shape / seed than _train_case: %s" % stored
    return c, cfg, sd, inp


def _model(cfg, sd, setting, precision="fp32"):
    from mvn.models.triangulation import VolumetricTriangulationNet
    m = VolumetricTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    setting(m)
    m.train_precision = precision
    return m


def _forward(m, c, inp):
    from test_gpu_models import _cameras
    batch = {"cameras": _cameras(inp, c["B"]), "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    np.random.seed(c["seed"] + 100)
    return m(inp["images"].to(DEV), torch.zeros(c["B"], c["NV"], 3, 4, device=DEV), batch), batch


def _loss(G, out):
    from mvn.models import loss as L
    kp, feats, vols, conf, cuboids, cvs, bps = out
    gt, val = torch.from_numpy(G["gt"]).to(DEV), torch.from_numpy(G["val"]).to(DEV)
    return L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val), L.VolumetricCELoss()(cvs, vols, gt, val)


def _labels(tape, ops):
    return [tape.labels.get(id(fn)) or "op" for fn in ops]


def _bwd_touches_backbone(labels, allow=()):
    """Recorded backward ops over a tensor of the backbone's shapes: BatchNorm backward over its rows, a 2D input-gradient convolution, a weight gradient
    over its rows (``allow``: the weight shapes that may -- process_features reads the backbone's map), pool backward."""
    bad = []
    for lab in labels:
        if lab.startswith("bn_bwd ") and int(lab.split()[1].split("x")[0]) in BACKBONE_ROWS:
            bad.append(lab)
        elif lab.startswith("dgrad ") and "@6x1x" in lab:
            bad.append(lab)
        elif lab.startswith("wgrad ") and int(lab.split(" rows ")[1].split()[0]) in BACKBONE_ROWS and lab.split()[1] not in allow:
            bad.append(lab)
        elif lab.startswith(("avgpool_bwd @6x1x", "maxpool_bwd @6x1x")):          # (V2V's 3D pools are @2x...)
            bad.append(lab)
    return bad


@pytest.mark.parametrize("no_plan", [False, True], ids=["frozen_plan_allowed", "LT_TRAIN_NO_FROZEN_PLAN"])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_whole_finetune_step_vs_reference(golden_dir, monkeypatch, name, no_plan):
    import lt_train
    if no_plan:
        monkeypatch.setenv("LT_TRAIN_NO_FROZEN_PLAN", "1")
    else:
        monkeypatch.delenv("LT_TRAIN_NO_FROZEN_PLAN", raising=False)
    G = np.load(os.path.join(golden_dir, "train_step_%s.npz" % name))
    c, cfg, sd, inp = _case(G)
    vs, fs = int(G["vol_stride"]), int(G["feat_stride"])
    TAG = "[%s%s] " % (name, " on the tape" if no_plan else "")
    m = _model(cfg, sd, SETTINGS[name])
    lr, pf_lr, vn_lr = [float(v) for v in G["lrs"]]
    opt = lt_train.Adam([{"params": list(m.backbone.parameters())}, {"params": list(m.process_features.parameters()), "lr": pf_lr},
                         {"params": list(m.volume_net.parameters()), "lr": vn_lr}], lr=lr)
    out, batch = _forward(m, c, inp)
    kp, feats, vols, conf, cuboids, cvs, bps = out
    kp_noise, loss_noise = float(G["kp_noise"]), float(G["loss_noise"])
    d = (kp.detach().cpu().double() - torch.from_numpy(G["kp"]).double()).abs() / torch.from_numpy(G["kp"]).double().abs().clamp(min=1.0)
    record(TAG + "ft/step forward keypoints, rel with 1 mm floor", {"err": float(d.max()), "tol": 1e-4 + 2 * kp_noise, "reference_self_noise": kp_noise})
    print(TAG, "keypoints", float(d.max()), "gate", 1e-4 + 2 * kp_noise)
    assert float(d.max()) <= 1e-4 + 2 * kp_noise, float(d.max())
    check(TAG + "ft/step forward volumes", vols.detach().cpu()[:, :, ::vs, ::vs, ::vs], G["vol_sub"], 1e-3 + 10 * kp_noise)
    check(TAG + "ft/step forward features", feats.detach().cpu().reshape(c["B"] * c["NV"], *feats.shape[2:])[:, :, ::fs, ::fs], G["feat_sub"], 1e-4)
    assert conf is None
    mae, ce = _loss(G, out)
    print(TAG, "mae", float(mae.detach()), float(G["mae"]), "ce", float(ce.detach()), float(G["ce"]))
    assert abs(float(mae.detach()) - float(G["mae"])) <= (1e-4 + 2 * loss_noise) * float(G["mae"]), (float(mae.detach()), float(G["mae"]))
    assert abs(float(ce.detach()) - float(G["ce"])) <= 1e-3 * float(G["ce"]), (float(ce.detach()), float(G["ce"]))
    opt.zero_grad()
    (mae + 0.01 * ce).backward()
    named = dict(m.named_parameters())
    names, no_grad = [str(n) for n in G["names"]], [str(n) for n in G["no_grad"]]
    assert sorted(names + no_grad) == sorted(named) and no_grad
    assert sorted(no_grad) == sorted(n for n, p in named.items() if not p.requires_grad), "the fixture's frozen set is not this setting's"
    gn2, table, n_zero = 0.0, [], 0
    gnorm_ref = float(G["grad_norm"])
    for n in names:
        p = named[n]
        assert p.grad is not None, "no gradient for " + n
        gr = p.grad.detach().double().cpu()
        ref_norm, ref_max, ref_sum = [float(v) for v in G["gn/" + n]]
        noise = float(G["noise/" + n])
        gn2 += float(gr.pow(2).sum())
        if ZERO_GRAD.search(n) or noise > 0.05:          # exact-zero gradients (a bias in front of a training-mode BatchNorm): rounding noise on both sides
            assert float(gr.abs().max()) <= 10 * ref_max + 1e-6 * gnorm_ref, (n, float(gr.abs().max()), ref_max)
            n_zero += 1
            continue
        e = float((_sub129(gr) - torch.from_numpy(G["g/" + n]).double()).abs().max()) / ref_max
        en = abs(float(gr.norm()) - ref_norm) / ref_norm
        table.append((max(e, en) / (1e-3 + 4 * noise), max(e, en), noise, n))
    table.sort(reverse=True)
    print("worst parameter gradients (err / gate, err, reference self-noise):", *["%.2f %.2e %.2e %s" % t for t in table[:8]], sep="\n  ")
    errs = sorted(t[1] for t in table)
    record(TAG + "ft/step parameter gradients vs the reference's step (gate 1e-3 + 4 x reference self-noise)",
           {"worst_err_over_gate": table[0][0], "worst_err": errs[-1], "median_err": errs[len(errs) // 2], "parameters_compared": len(table),
            "zero_gradient_parameters": n_zero, "frozen_parameters": len(no_grad)})
    assert table[0][0] <= 1.0, table[:8]
    for n in no_grad:
        assert named[n].grad is None, "a frozen parameter received a gradient: " + n
    gn = float(np.sqrt(gn2))
    print(TAG, "global gradient norm", gn, gnorm_ref)
    assert abs(gn - gnorm_ref) <= 2e-3 * gnorm_ref, (gn, gnorm_ref)
    # running statistics: the moving ones against the reference's, the others untouched
    bufs = dict(m.named_buffers())
    moving = {str(n) for n in G["rs_moving"]}
    mods = dict(m.named_modules())
    assert moving == {n for n in bufs if n.endswith(("running_mean", "running_var")) and mods[n.rsplit(".", 1)[0]].training}
    w_rs = 0.0
    for key in G.files:
        if key.startswith("rs/"):
            ref = torch.from_numpy(G[key]).double()
            e = float((_sub129(bufs[key[3:]]) - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
            if key[3:] in moving:
                w_rs = max(w_rs, e)
            else:
                assert e == 0.0, key
    record(TAG + "ft/step BatchNorm running statistics (the moving ones)", {"err": w_rs, "tol": 1e-4, "moving": len(moving)})
    assert w_rs <= 1e-4, w_rs
    opt.step()
    torch.cuda.synchronize()
    sd_now = m.state_dict()
    for n in no_grad:
        assert torch.equal(sd_now[n].cpu(), sd[n]), "a frozen parameter moved: " + n
    for n, mod in mods.items():
        if isinstance(mod, BN) and not mod.training:
            assert torch.equal(mod.running_mean.cpu(), sd[n + ".running_mean"]) and torch.equal(mod.running_var.cpu(), sd[n + ".running_var"]), n
            assert int(mod.num_batches_tracked) == int(sd[n + ".num_batches_tracked"]), n
    w_p, w_name, n_known = 0.0, None, 0
    for n in names:
        if ZERO_GRAD.search(n):
            continue
        ref = torch.from_numpy(G["p1/" + n]).double()
        gs = torch.from_numpy(G["g/" + n]).double().abs()
        known = gs > 100 * (float(G["noise/" + n]) + 1e-3) * float(G["gn/" + n][1])
        n_known += int(known.sum())
        lr_n = lr if n.startswith("backbone.") else pf_lr if n.startswith("process_features.") else vn_lr
        e = float(((_sub129(named[n]) - ref).abs() * known).max()) / lr_n      # in units of one full Adam step
        if e > w_p:
            w_p, w_name = e, n
    record(TAG + "ft/step parameters after Adam, worst |d| in units of lr", {"err": w_p, "tol": 2e-2, "name": w_name, "elements_compared": n_known})
    assert w_p <= 2e-2, (w_p, w_name)
    assert n_known > 0
    # ---- what the tape recorded
    plans = list(m._train_plans.values())
    assert len(plans) == 1
    plan, tape = plans[0], plans[0].tape
    bl, fl = _labels(tape, tape.bwd_ops), _labels(tape, tape.fwd_ops)
    trainable = [p for p in named.values() if p.requires_grad]
    assert set(tape.param_grads) == set(trainable) and tape.arena_off == sum((p.numel() + 3) // 4 * 4 for p in trainable)
    n_wgrad = sum(1 for lab in bl if lab.startswith("wgrad "))
    assert n_wgrad == sum(1 for p in trainable if p.dim() >= 4), (n_wgrad, "weight gradients recorded")
    assert plan.frozen_plan == (name in PLAN_ELIGIBLE and not no_plan)
    if name == "ft_bn_affine":          # the arena holds exactly the convolution weights and biases
        assert all(n.endswith(".bias") or p.dim() >= 4 for n, p in named.items() if p.requires_grad)
        assert not any(isinstance(mods[n.rsplit(".", 1)[0]], BN) for n, p in named.items() if p.requires_grad)
        assert any(lab.startswith("bn_bwd ") and int(lab.split()[1].split("x")[0]) in BACKBONE_ROWS for lab in bl)          # frozen affine, frozen statistics, dy still owed
    else:
        pf = "32x256x1x1" if name != "ft_v2v_only" else None
        assert not _bwd_touches_backbone(bl, allow=(pf,)), _bwd_touches_backbone(bl, allow=(pf,))
    assert ("unproject_bwd" in bl) == (name != "ft_v2v_only")
    if plan.frozen_plan:          # the tape's forward starts at process_features
        convs = [lab for lab in fl if lab.startswith("conv ")]
        assert convs[0].startswith("conv conv1x1 256->32 @6x1x32x32"), convs[:3]
        assert not any(lab.startswith(("bn_stats ", "bn_act ")) and int(lab.split()[1].split("x")[0]) in BACKBONE_ROWS for lab in fl)
    else:
        assert any(lab.startswith("bn_act ") and int(lab.split()[1].split("x")[0]) in BACKBONE_ROWS for lab in fl)
    # the REPLAYED forward reads the updated parameters: same result as a fresh recording with the new state dict
    kp_replay = _forward(m, c, inp)[0][0].detach().clone()
    m2 = _model(cfg, m.state_dict(), SETTINGS[name])
    kp_fresh = _forward(m2, c, inp)[0][0].detach()
    check(TAG + "ft/step replayed forward after Adam vs a fresh recording with the updated weights", kp_replay.cpu(), kp_fresh.cpu(), 1e-6)
    assert float((kp_replay.cpu() - torch.from_numpy(G["kp"])).abs().max()) > 1e-3      # and the step did move the prediction
    m.eval()
    with torch.no_grad():
        kp2 = m(inp["images"].to(DEV), None, batch)[0]
    assert torch.isfinite(kp2).all()


@pytest.mark.parametrize("no_plan", [False, True], ids=["frozen_plan", "LT_TRAIN_NO_FROZEN_PLAN"])
def test_act16_finetune_step_with_a_frozen_backbone(golden_dir, monkeypatch, no_plan):
    """train_precision "act16" with the backbone frozen in eval(): the limits of test_act16_step_with_a_frozen_backbone_batchnorm (joints < 6e-2, gradient
    error median <= 0.07, p90 <= 0.22) over the trainable parameters, against the reference's fp32 step of the setting.  A frozen backbone removes bf16
    gradient paths, so these are upper bounds here."""
    if no_plan:
        monkeypatch.setenv("LT_TRAIN_NO_FROZEN_PLAN", "1")
    else:
        monkeypatch.delenv("LT_TRAIN_NO_FROZEN_PLAN", raising=False)
    G = np.load(os.path.join(golden_dir, "train_step_ft_backbone_eval.npz"))
    c, cfg, sd, inp = _case(G)
    m = _model(cfg, sd, _ft_backbone_eval, "act16")
    out, _ = _forward(m, c, inp)
    kp = out[0]
    mae, ce = _loss(G, out)
    (mae + 0.01 * ce).backward()
    named = dict(m.named_parameters())
    errs = []
    for n in G["names"]:
        n = str(n)
        if ZERO_GRAD.search(n):
            continue
        errs.append(float((_sub129(named[n].grad) - torch.from_numpy(G["g/" + n]).double()).abs().max()) / float(G["gn/" + n][1]))
    errs.sort()
    d = float(((kp.detach().cpu().double() - torch.from_numpy(G["kp"]).double()).abs() / torch.from_numpy(G["kp"]).double().abs().clamp(min=1.0)).max())
    st = {"joints_max_rel": d, "mae": float(mae.detach()), "mae_reference": float(G["mae"]), "parameter_gradient_err_median": errs[len(errs) // 2],
          "parameter_gradient_err_p90": errs[int(len(errs) * 0.9)], "parameters": len(errs)}
    record("ft/act16 with a frozen backbone in eval()%s, one step vs the reference's fp32 step" % (" on the tape" if no_plan else " on the inference plan"), st)
    print(st)
    assert d < 6e-2 and errs[len(errs) // 2] <= 0.07 and errs[int(len(errs) * 0.9)] <= 0.22, st
    assert all(named[str(n)].grad is None for n in G["no_grad"])
    assert list(m._train_plans.values())[0].frozen_plan == (not no_plan)
    bn1 = m.backbone.bn1
    assert torch.equal(bn1.running_mean.cpu(), sd["backbone.bn1.running_mean"]) and int(bn1.num_batches_tracked) == int(sd["backbone.bn1.num_batches_tracked"])


@pytest.mark.parametrize("no_plan", [False, True], ids=["frozen_plan", "LT_TRAIN_NO_FROZEN_PLAN"])
def test_a_changed_frozen_backbone_is_seen_and_a_thawed_one_trains(golden_dir, monkeypatch, no_plan):
    """After a step with the backbone frozen in eval(), its first convolution's weights are halved in place: the next training forward's features differ
    from the previous step's and equal those of a fresh model with the changed state dict (1e-6).  On the tape the weights are live, so the edit is made
    through ``.data``; the inference plan is invalidated by PlanCache's fingerprint (data_ptr + version counter of the backbone's tensors), which by
    PlanCache's own contract does not see ``.data`` writes: there the same edit is made in place under no_grad, which bumps the version counter.
    Then ``backbone.requires_grad_(True); model.train()``: every parameter gets a gradient again, and -- the state dict is the one train_step.npz's
    reference started from, no optimiser step was taken -- the forward passes train_step.npz's gates unchanged."""
    if no_plan:
        monkeypatch.setenv("LT_TRAIN_NO_FROZEN_PLAN", "1")
    else:
        monkeypatch.delenv("LT_TRAIN_NO_FROZEN_PLAN", raising=False)
    G = np.load(os.path.join(golden_dir, "train_step_ft_backbone_eval.npz"))
    G0 = np.load(os.path.join(golden_dir, "train_step.npz"))
    c, cfg, sd, inp = _case(G)
    m = _model(cfg, sd, _ft_backbone_eval)
    out, _ = _forward(m, c, inp)
    mae, ce = _loss(G, out)
    (mae + 0.01 * ce).backward()
    feats0 = out[1].detach().clone()
    w = m.backbone.conv1.weight
    if no_plan:
        w.data.mul_(0.5)
    else:
        with torch.no_grad():
            w.mul_(0.5)
    feats1 = _forward(m, c, inp)[0][1].detach().clone()
    assert float((feats1 - feats0).abs().max()) > 1e-3 * float(feats0.abs().max()), "the changed backbone weights were not seen"
    m2 = _model(cfg, m.state_dict(), _ft_backbone_eval)
    feats2 = _forward(m2, c, inp)[0][1].detach()
    check("ft/changed frozen backbone%s: features vs a fresh model with the changed state dict" % (" on the tape" if no_plan else ""), feats1.cpu(), feats2.cpu(), 1e-6)
    # thaw
    with torch.no_grad():
        w.copy_(sd["backbone.conv1.weight"])
    for p in m.parameters():
        p.grad = None
    m.backbone.requires_grad_(True); m.train()
    out, _ = _forward(m, c, inp)
    kp, feats, vols = out[0], out[1], out[2]
    kp_noise = float(G0["kp_noise"])
    d = (kp.detach().cpu().double() - torch.from_numpy(G0["kp"]).double()).abs() / torch.from_numpy(G0["kp"]).double().abs().clamp(min=1.0)
    assert float(d.max()) <= 1e-4 + 2 * kp_noise, float(d.max())
    check("ft/thawed forward volumes", vols.detach().cpu()[:, :, ::4, ::4, ::4], G0["vol_sub"], 1e-3 + 10 * kp_noise)
    check("ft/thawed forward features", feats.detach().cpu().reshape(c["B"] * c["NV"], *feats.shape[2:])[:, :, ::2, ::2], G0["feat_sub"], 1e-4)
    mae, ce = _loss(G0, out)
    (mae + 0.01 * ce).backward()
    named = dict(m.named_parameters())          # every parameter the all-trainable reference step gives a gradient (not the unused heatmap layer)
    assert all(named[str(n)].grad is not None for n in G0["names"]), [str(n) for n in G0["names"] if named[str(n)].grad is None][:5]
    assert sorted(str(n) for n in G0["no_grad"]) == sorted(n for n, p in named.items() if p.grad is None)
    assert len(m._train_plans) == 2 and not list(m._train_plans.values())[-1].frozen_plan


def test_whole_algebraic_finetune_step_vs_reference(golden_dir):
    """AlgebraicTriangulationNet with conv1, bn1, layer1 - layer3 frozen (BatchNorm in eval()); layer4, the deconvolutions, final_layer and the confidence
    head trainable: the body and gates of test_whole_algebraic_training_step_vs_reference against train_step_alg_ft_trunk.npz."""
    import lt_train
    from mvn.models import loss as L
    from mvn.models.triangulation import AlgebraicTriangulationNet
    G = np.load(os.path.join(golden_dir, "train_step_alg_ft_trunk.npz"))
    TA = "ft-alg/"
    c = {str(k): int(v) for k, v in zip(G["case_keys"], G["case"])}          # (the seed is the one at which the reference passes its own gates)
    assert {k: v for k, v in c.items() if k != "seed"} == dict(nl=18, B=2, NV=3, H=128)
    cfg = synth.alg_config(c["nl"], True)
    cfg.model.heatmap_multiplier = 1.0
    cfg.model["heatmap_multiplier"] = 1.0
    sd = synth.make_state_dict(spec.alg_net_spec(c["nl"], 17, True), seed=c["seed"], basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    m = AlgebraicTriangulationNet(cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    _alg_ft_trunk(m)
    lr = float(G["lr"])
    opt = lt_train.Adam([p for p in m.parameters() if p.requires_grad], lr=lr)
    P = torch.from_numpy(G["P"]).to(DEV)
    kp3, kp2, hm, conf = m(inp["images"].to(DEV), P, {})
    kp_noise, loss_noise = float(G["kp_noise"]), float(G["loss_noise"])
    d = (kp3.detach().cpu().double() - torch.from_numpy(G["kp3"]).double()).abs() / torch.from_numpy(G["kp3"]).double().abs().clamp(min=1.0)
    record(TA + "step forward keypoints_3d, rel with 1 mm floor", {"err": float(d.max()), "tol": 1e-4 + 2 * kp_noise, "reference_self_noise": kp_noise})
    assert float(d.max()) <= 1e-4 + 2 * kp_noise, float(d.max())
    check(TA + "step forward keypoints_2d", kp2.detach().cpu(), G["kp2"], 1e-4)
    check(TA + "step forward confidences", conf.detach().cpu(), G["conf"], 1e-4)
    check(TA + "step forward heatmaps", hm.detach().cpu().reshape(c["B"] * c["NV"], *hm.shape[2:])[:, :, ::2, ::2], G["hm_sub"], 1e-4)
    gt, val = torch.from_numpy(G["gt"]).to(DEV), torch.from_numpy(G["val"]).to(DEV)
    loss = L.KeypointsMSESmoothLoss(400)(kp3 * 0.1, gt * 0.1, val)
    assert abs(float(loss.detach()) - float(G["loss"])) <= (1e-4 + 2 * loss_noise) * float(G["loss"]), (float(loss.detach()), float(G["loss"]))
    opt.zero_grad()
    loss.backward()
    named = dict(m.named_parameters())
    names, no_grad = [str(n) for n in G["names"]], [str(n) for n in G["no_grad"]]
    assert sorted(no_grad) == sorted(n for n, p in named.items() if not p.requires_grad) and no_grad
    gn2, table, n_zero = 0.0, [], 0
    gnorm_ref = float(G["grad_norm"])
    for n in names:
        p = named[n]
        assert p.grad is not None, "no gradient for " + n
        gr = p.grad.detach().double().cpu()
        ref_norm, ref_max, _ = [float(v) for v in G["gn/" + n]]
        noise = float(G["noise/" + n])
        gn2 += float(gr.pow(2).sum())
        if noise > 0.05:
            assert float(gr.abs().max()) <= 10 * ref_max + 1e-6 * gnorm_ref, (n, float(gr.abs().max()), ref_max)
            n_zero += 1
            continue
        sub = _sub129(gr)          # gated against the reference's own step in fp64, as in the all-trainable test
        n64, m64 = [float(v) for v in G["gn64/" + n]]
        e = float((sub - torch.from_numpy(G["g64/" + n]).double()).abs().max()) / m64
        en = abs(float(gr.norm()) - n64) / n64
        e32 = max(float((sub - torch.from_numpy(G["g/" + n]).double()).abs().max()) / ref_max, abs(float(gr.norm()) - ref_norm) / ref_norm)
        table.append((max(e, en) / (1e-3 + 4 * noise), max(e, en), noise, n, e32))
    table.sort(reverse=True)
    print("worst parameter gradients (err / gate, err vs the fp64 step, reference self-noise, name, err vs the fp32 step):", *["%.2f %.2e %.2e %s %.2e" % t for t in table[:8]], sep="\n  ")
    errs, e32s = sorted(t[1] for t in table), sorted(t[4] for t in table)
    record(TA + "step parameter gradients vs the reference's fp64 step (gate 1e-3 + 4 x reference self-noise)",
           {"worst_err_over_gate": table[0][0], "worst_err": errs[-1], "median_err": errs[len(errs) // 2], "parameters_compared": len(table),
            "zero_gradient_parameters": n_zero, "frozen_parameters": len(no_grad), "vs_the_fp32_step_worst": e32s[-1]})
    assert table[0][0] <= 1.0, table[:8]
    assert e32s[-1] <= 3e-2, e32s[-1]
    assert len(table) + n_zero == len(names)
    for n in no_grad:
        assert named[n].grad is None, "a frozen parameter received a gradient: " + n
    gn = float(np.sqrt(gn2))
    assert abs(gn - float(G["grad_norm64"])) <= 2e-3 * gnorm_ref and abs(gn - gnorm_ref) <= 1e-2 * gnorm_ref, (gn, gnorm_ref, float(G["grad_norm64"]))
    bufs, mods = dict(m.named_buffers()), dict(m.named_modules())
    moving = {str(n) for n in G["rs_moving"]}
    w_rs = 0.0
    for key in G.files:
        if key.startswith("rs/"):
            ref = torch.from_numpy(G[key]).double()
            e = float((_sub129(bufs[key[3:]]) - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
            if key[3:] in moving:
                w_rs = max(w_rs, e)
            else:
                assert e == 0.0, key
    record(TA + "step BatchNorm running statistics (the moving ones)", {"err": w_rs, "tol": 1e-4})
    assert w_rs <= 1e-4, w_rs
    opt.step()
    torch.cuda.synchronize()
    sd_now = m.state_dict()
    for n in no_grad:
        assert torch.equal(sd_now[n].cpu(), sd[n]), "a frozen parameter moved: " + n
    for n, mod in mods.items():
        if isinstance(mod, BN) and not mod.training:
            assert torch.equal(mod.running_mean.cpu(), sd[n + ".running_mean"]) and int(mod.num_batches_tracked) == int(sd[n + ".num_batches_tracked"]), n
    w_p, w_name, n_known = 0.0, None, 0
    for n in names:
        if float(G["noise/" + n]) > 0.05:
            continue
        ref = torch.from_numpy(G["p1/" + n]).double()
        gs = torch.from_numpy(G["g/" + n]).double().abs()
        known = gs > 100 * (float(G["noise/" + n]) + 1e-3) * float(G["gn/" + n][1])
        n_known += int(known.sum())
        e = float(((_sub129(named[n]) - ref).abs() * known).max()) / lr
        if e > w_p:
            w_p, w_name = e, n
    record(TA + "step parameters after Adam, worst |d| in units of lr", {"err": w_p, "tol": 2e-2, "name": w_name, "elements_compared": n_known})
    assert w_p <= 2e-2 and n_known > 0, (w_p, w_name, n_known)
    # what the tape recorded: one weight gradient per trainable filter (the head's three linears are 1x1 convolutions), nothing over the frozen trunk's maps
    tape = list(m._train_plans.values())[0].tape
    bl = _labels(tape, tape.bwd_ops)
    trainable = [p for p in named.values() if p.requires_grad]
    assert set(tape.param_grads) == set(trainable) and tape.arena_off == sum((p.numel() + 3) // 4 * 4 for p in trainable)
    assert sum(1 for lab in bl if lab.startswith("wgrad ")) == sum(1 for n, p in named.items() if p.requires_grad and n.endswith(".weight") and p.dim() in (2, 4)
                                                                    and not isinstance(mods[n.rsplit(".", 1)[0]], BN))
    # one BatchNorm backward per BatchNorm module of the trainable part (layer4, the head, the deconvolutions), none over the trunk's maps (rows x C of
    # conv1 / layer1 / layer2; layer3's 384 x 256 is also the first deconvolution's shape, which the count covers)
    n_bn = sum(1 for mod in mods.values() if isinstance(mod, BN) and mod.weight.requires_grad)
    assert sum(1 for lab in bl if lab.startswith("bn_bwd ")) == n_bn and n_bn > 0
    assert not any(lab.split()[1] in ("24576x64", "6144x64", "1536x128") for lab in bl if lab.startswith("bn_bwd "))
    assert not any(lab.startswith("maxpool_bwd @6x1x64x64") for lab in bl)          # the stem's pool (the head's pools are trainable territory)
    kp3b = m(inp["images"].to(DEV), P, {})[0]
    loss2 = L.KeypointsMSESmoothLoss(400)(kp3b * 0.1, gt * 0.1, val)
    opt.zero_grad(); loss2.backward(); opt.step()
    assert torch.isfinite(kp3b).all() and float(loss2.detach()) != float(loss.detach())
