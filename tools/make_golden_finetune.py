"""Generates the fine-tuning fixtures under tests/golden/ by running the REFERENCE on the CPU where the reference tree is available (the same loader as
oracle/make_golden.py).  Writes only these files:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_finetune.py [name ...]

One full training step of the reference with some parameters frozen (``requires_grad_(False)``) -- autograd then ends the backward where nothing
trains and returns no gradient for a frozen parameter.  The volumetric recipe is oracle/make_golden.py:gen_train restated (as in
tools/make_golden_train_many_views.py): ResNet-18, 2 samples x 3 views of 128 x 128, 64^3 voxels, view softmax, MAE on keypoints * 0.1 + 0.01 *
VolumetricCELoss, Adam with the three learning-rate groups of train.py:430-437.  The settings:

    train_step_ft_backbone_eval.npz     backbone parameters frozen, backbone.eval(); process_features and V2V trainable, V2V BatchNorm in train()
    train_step_ft_backbone_trainbn.npz  backbone parameters frozen, whole model in train(): the backbone normalises with batch statistics and its
                                        running statistics move
    train_step_ft_bn_affine.npz         every BatchNorm weight / bias of the model frozen, backbone BatchNorm in eval(), V2V BatchNorm in train(); all
                                        convolutions trainable (frozen-affine BatchNorm layers that still owe dy, in both statistics modes)
    train_step_ft_v2v_only.npz          backbone and process_features frozen, backbone.eval(): no gradient reaches the unprojection
    train_step_alg_ft_trunk.npz         AlgebraicTriangulationNet with use_confidences (oracle/make_golden.py:gen_train_alg restated): conv1, bn1,
                                        layer1 - layer3 frozen with their BatchNorm in eval(); layer4, the deconvolutions, final_layer and the
                                        confidence head trainable

Same keys as train_step.npz / train_step_alg.npz.  ``no_grad`` lists every frozen parameter; ``rs/<name>`` is stored for every running statistic that
must move (``rs_moving``) and for every fifth one that must not; ``case`` holds the shape constants and the seed, ``vol_stride`` / ``feat_stride`` the strides of the two sub-sampled tensors.  The reference runs three times (8
threads, 1 thread, images x (1 + 1e-6)): ``noise/<name>``, ``kp_noise``, ``loss_noise``.  Two further runs (images x (1 - 1e-6), 4 threads) are held
to the gates the test applies to a product -- sampled gradient and norm per trainable parameter against 1e-3 + 4 x noise (the algebraic step also
against its fp64 step, as its test does), keypoints against 1e-4 + 2 x kp_noise, the global gradient norm against 2e-3 -- and while the reference fails its own gate the generator re-seeds (seed + 1000).  The volumes and feature maps are sub-sampled to keep
each file below the size limit of a committed fixture."""
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader, spec, synth, truth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CASE = dict(nl=18, B=2, NV=3, H=128, V=64, seed=12)
ALG_CASE = dict(nl=18, B=2, NV=3, H=128, seed=21)
LRS = (1e-4, 1e-3, 1e-3)          # experiments/human36m/train/human36m_vol_softmax.yaml
VOL_STRIDE, FEAT_STRIDE = 8, 2          # (the volumes more coarsely than in train_step.npz: the files stay below the size limit of a committed fixture)
ZERO_GRAD = re.compile(r"^volume_net\.(.*\.(block\.0|res_branch\.0|res_branch\.3|skip_con\.0)|output_layer)\.bias$")
BN = torch.nn.modules.batchnorm._BatchNorm


def _bn_eval(mod):
    for m in mod.modules():
        if isinstance(m, BN):
            m.eval()


def ft_backbone_eval(m):
    m.backbone.requires_grad_(False)
    m.train(); m.backbone.eval()


def ft_backbone_trainbn(m):
    m.backbone.requires_grad_(False)
    m.train()


def ft_bn_affine(m):
    m.train()
    for mod in m.modules():
        if isinstance(mod, BN):
            mod.weight.requires_grad_(False); mod.bias.requires_grad_(False)
    _bn_eval(m.backbone)


def ft_v2v_only(m):
    m.backbone.requires_grad_(False); m.process_features.requires_grad_(False)
    m.train(); m.backbone.eval()


def alg_ft_trunk(m):
    m.train()
    b = m.backbone
    for mod in (b.conv1, b.bn1, b.layer1, b.layer2, b.layer3):
        mod.requires_grad_(False)
        mod.eval()


VOL_SETTINGS = {"ft_backbone_eval": ft_backbone_eval, "ft_backbone_trainbn": ft_backbone_trainbn, "ft_bn_affine": ft_bn_affine, "ft_v2v_only": ft_v2v_only}


def _sub(t, stride):
    sl = (slice(None), slice(None)) + tuple(slice(None, None, stride) for _ in range(t.dim() - 2))
    return t[sl].contiguous().numpy()


def _train_sub(t, n=129):
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // n)][:n].numpy().copy()


def _gradients(out, ref, others, opt):
    """The per-parameter keys of train_step.npz from the first run ``ref`` and the two noise runs ``others``; the Adam step; the running statistics."""
    names, no_grad, noises = [], [], []
    og = [dict(o.named_parameters()) for o in others]
    for n, p in ref.named_parameters():
        if p.grad is None:
            assert not p.requires_grad, n
            no_grad.append(n)
            continue
        names.append(n)
        gmax = float(p.grad.abs().max())
        out["g/" + n] = _train_sub(p.grad)
        out["gn/" + n] = np.array([float(p.grad.double().norm()), gmax, float(p.grad.double().sum())])
        noise = max(float((o[n].grad - p.grad).abs().max()) for o in og) / max(gmax, 1e-30)
        out["noise/" + n] = np.array(noise)
        noises.append(noise)
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    opt.step()
    for n, p in ref.named_parameters():
        if n in names:
            out["p1/" + n] = _train_sub(p)
        else:
            assert torch.equal(p.detach(), sd0[n]), n          # a frozen parameter does not move
    moving, still = [], 0
    mods = dict(ref.named_modules())
    for n, b_ in ref.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            if mods[n.rsplit(".", 1)[0]].training:
                moving.append(n)
                out["rs/" + n] = _train_sub(b_)
            else:
                still += 1
                if still % 5 == 0:
                    out["rs/" + n] = _train_sub(b_)
    out["names"] = np.array(names); out["no_grad"] = np.array(no_grad); out["rs_moving"] = np.array(moving)
    gn = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters() if p.grad is not None)))
    out["grad_norm"] = np.array(gn)
    return names, no_grad, np.sort(np.array(noises)), gn


def _gnorm(model):
    return float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in model.parameters() if p.grad is not None)))


def _own_gate(out, ref, checks, zero, g="g/", gn="gn/"):
    """The reference against the gate the test applies: the worst (error / gate, name) over the trainable parameters of the runs ``checks``, against the
    stored samples ``g`` and (norm, max) ``gn``."""
    worst = (0.0, None)
    for o in checks:
        og = dict(o.named_parameters())
        for n, p in ref.named_parameters():
            if p.grad is None or zero(n) or float(out["noise/" + n]) > 0.05:
                continue
            e = float(np.abs((_train_sub(og[n].grad) - out[g + n]).astype(np.float64)).max()) / float(out[gn + n][1])
            en = abs(float(og[n].grad.double().norm()) - float(out[gn + n][0])) / float(out[gn + n][0])
            ratio = max(e, en) / (1e-3 + 4 * float(out["noise/" + n]))
            if ratio > worst[0]:
                worst = (ratio, n)
    return worst


def run_vol(mvn, name, case):
    import mvn.models.loss as L
    torch.set_num_threads(8)
    c = {k: int(v) for k, v in case.items()}
    cfg = synth.vol_config(c["nl"], c["V"], "softmax", 1.0, "mpii")
    sd = synth.make_state_dict(spec.vol_net_spec(c["nl"], 17, False), seed=c["seed"], sharpen=60.0, basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    Cam = mvn.utils.multiview.Camera
    lr, pf_lr, vn_lr = LRS
    g = torch.Generator().manual_seed(43)
    dgt = torch.randn(c["B"], 17, 3, generator=g) * 40
    val = torch.ones(c["B"], 17, 1); val[1, 5] = 0

    def step(eps=0.0, gt=None):
        ref = mvn.models.triangulation.VolumetricTriangulationNet(cfg, device="cpu")
        ref.load_state_dict(sd, strict=True)
        VOL_SETTINGS[name](ref)
        opt = torch.optim.Adam([{"params": ref.backbone.parameters()}, {"params": ref.process_features.parameters(), "lr": pf_lr},
                                {"params": ref.volume_net.parameters(), "lr": vn_lr}], lr=lr)
        cams = [[Cam(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(c["B"])] for v in range(c["NV"])]
        batch = {"cameras": cams, "pred_keypoints_3d": inp["pred_keypoints_3d"]}
        np.random.seed(c["seed"] + 100)
        kp, feats, vols, vconf, cuboids, cvs, bps = ref(inp["images"] * (1.0 + eps), torch.zeros(c["B"], c["NV"], 3, 4), batch)
        if gt is None:
            gt = kp.detach() + dgt
        mae = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val)
        ce = L.VolumetricCELoss()(cvs, vols, gt, val)
        opt.zero_grad()
        (mae + 0.01 * ce).backward()
        return ref, opt, dict(kp=kp.detach(), feats=feats.detach(), vols=vols.detach(), gt=gt, mae=float(mae), ce=float(ce))

    np.random.seed(c["seed"] + 100)
    thetas = np.random.uniform(0.0, 2 * np.pi, size=c["B"])
    t0 = time.time()
    ref, opt, r = step()
    torch.set_num_threads(1)
    ref1, _, r1 = step(gt=r["gt"])
    torch.set_num_threads(8)
    refp, _, rp = step(eps=1e-6, gt=r["gt"])
    kp = r["kp"]
    kp_noise = max(float(((o["kp"] - kp).abs() / kp.abs().clamp(min=1.0)).max()) for o in (r1, rp))
    out = {"kp": kp.numpy(), "gt": r["gt"].numpy(), "val": val.numpy(), "mae": np.array(r["mae"]), "ce": np.array(r["ce"]),
           "thetas": thetas, "lrs": np.array([lr, pf_lr, vn_lr]), "vol_sub": _sub(r["vols"], VOL_STRIDE), "kp_noise": np.array(kp_noise),
           "loss_noise": np.array(max(abs(o["mae"] - r["mae"]) / r["mae"] for o in (r1, rp))),
           "feat_sub": _sub(r["feats"].reshape(c["B"] * c["NV"], *r["feats"].shape[2:]), FEAT_STRIDE),
           "case": np.array([c[k] for k in ("nl", "B", "NV", "H", "V", "seed")]), "case_keys": np.array(["nl", "B", "NV", "H", "V", "seed"]),
           "vol_stride": np.array(VOL_STRIDE), "feat_stride": np.array(FEAT_STRIDE), "sd_digest": np.array(synth.state_dict_checksum(sd)), "images_digest": truth.images_digest(inp["images"])}
    names, no_grad, noises, gn = _gradients(out, ref, (ref1, refp), opt)
    refm, _, rm = step(eps=-1e-6, gt=r["gt"])
    torch.set_num_threads(4)
    ref4, _, r4 = step(gt=r["gt"])
    torch.set_num_threads(8)
    worst = _own_gate(out, ref, (refm, ref4), lambda n: bool(ZERO_GRAD.search(n)))
    kp_own = max(float(((o["kp"] - kp).abs() / kp.abs().clamp(min=1.0)).max()) for o in (rm, r4)) / (1e-4 + 2 * kp_noise)
    gn_own = max(abs(_gnorm(o) - gn) / gn for o in (refm, ref4)) / 2e-3          # the global gradient norm, gated at 2e-3
    ok = worst[0] <= 1.0 and kp_own <= 1.0 and gn_own <= 1.0
    print("[%s] seed %d: the reference against its own gate: worst parameter gradient %.2f x gate (%s), keypoints %.2f x gate, global norm %.2f x gate -> %s" % (
        name, c["seed"], worst[0], worst[1], kp_own, gn_own, "kept" if ok else "re-seed"))
    print("  train step x5: %.1fs; mae %.4f ce %.4f; %d parameters with gradients (%d frozen), %d moving running statistics, global grad norm %.4e" % (
        time.time() - t0, r["mae"], r["ce"], len(names), len(no_grad), len(out["rs_moving"]), gn))
    print("  reference self-noise (threads / 1e-6 perturbation): kp %.2e; gradients median %.2e, 90%% %.2e, max %.2e" % (
        kp_noise, noises[len(noises) // 2], noises[int(len(noises) * 0.9)], noises[-1]))
    return ok, out


def run_alg(mvn, case):
    import mvn.models.loss as L
    torch.set_num_threads(8)
    c = {k: int(v) for k, v in case.items()}
    cfg = synth.alg_config(c["nl"], True)
    cfg.model.heatmap_multiplier = 1.0          # (gen_train_alg: the yaml's 100 makes the DLT of random-init heatmaps ill-conditioned)
    sd = synth.make_state_dict(spec.alg_net_spec(c["nl"], 17, True), seed=c["seed"], basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(c["B"], 1, 1, 1)
    lr = 1e-5
    g = torch.Generator().manual_seed(44)
    dgt = torch.randn(c["B"], 17, 3, generator=g) * 40
    val = torch.ones(c["B"], 17, 1); val[0, 3] = 0

    def step(eps=0.0, gt=None, dt=torch.float32):
        ref = mvn.models.triangulation.AlgebraicTriangulationNet(cfg, device="cpu")
        ref.load_state_dict(sd, strict=True)
        alg_ft_trunk(ref)
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
           "hm_sub": _sub(r["hm"].reshape(c["B"] * c["NV"], *r["hm"].shape[2:]), 2),
           "case": np.array([c[k] for k in ("nl", "B", "NV", "H", "seed")]), "case_keys": np.array(["nl", "B", "NV", "H", "seed"])}

    def tail_grads(dt):          # the reference's own gradient through torch.svd, fp32 against fp64, on the stored tail inputs (gen_train_alg)
        p2 = r["kp2"].to(dt).clone().requires_grad_(True)
        cf = r["conf"].to(dt).clone().requires_grad_(True)
        x3 = mvn.utils.multiview.triangulate_batch_of_points(P.to(dt), p2, confidences_batch=cf)
        L.KeypointsMSESmoothLoss(400)(x3.to(dt) * 0.1, r["gt"].to(dt) * 0.1, val.to(dt)).backward()
        return p2.grad.double(), cf.grad.double()

    ref64, _, r64 = step(gt=r["gt"], dt=torch.float64)          # the whole step with the reference's modules in fp64: what the alg test gates against
    g64 = dict(ref64.named_parameters())
    (p32, c32), (p64, c64) = tail_grads(torch.float32), tail_grads(torch.float64)
    out["svd32_rel"] = np.array(max(float((p32 - p64).abs().max() / p64.abs().max()), float((c32 - c64).abs().max() / c64.abs().max())))
    for n, p in ref.named_parameters():
        if p.grad is not None:
            out["g64/" + n] = _train_sub(g64[n].grad)
            out["gn64/" + n] = np.array([float(g64[n].grad.norm()), float(g64[n].grad.abs().max())])
    out["grad_norm64"] = np.array(float(torch.sqrt(sum(p.grad.pow(2).sum() for p in ref64.parameters() if p.grad is not None))))
    names, no_grad, noises, gn = _gradients(out, ref, (ref1, refp), opt)
    refm, _, rm = step(eps=-1e-6, gt=r["gt"])
    torch.set_num_threads(4)
    ref4, _, r4 = step(gt=r["gt"])
    torch.set_num_threads(8)
    # the alg test gates a product against the fp64 step: so is the reference's fp32 step here, next to the two further fp32 runs against the first
    worst = max(_own_gate(out, ref, (refm, ref4), lambda n: False), _own_gate(out, ref, (ref, refm, ref4), lambda n: False, "g64/", "gn64/"), key=lambda w: w[0])
    kp_own = max(float(((o["kp3"] - kp).abs() / kp.abs().clamp(min=1.0)).max()) for o in (rm, r4)) / (1e-4 + 2 * kp_noise)
    gn64 = float(out["grad_norm64"])          # the global norm: within 2e-3 of the fp64 step's and 1e-2 of the fp32 step's (both in units of the latter)
    gn_own = max(max(abs(_gnorm(o) - gn64) / gn / 2e-3, abs(_gnorm(o) - gn) / gn / 1e-2) for o in (ref, refm, ref4))
    ok = worst[0] <= 1.0 and kp_own <= 1.0 and gn_own <= 1.0
    print("[alg_ft_trunk] seed %d: the reference against its own gate: worst parameter gradient %.2f x gate (%s), keypoints %.2f x gate, global norm %.2f x gate -> %s" % (
        c["seed"], worst[0], worst[1], kp_own, gn_own, "kept" if ok else "re-seed"))
    print("  alg train step x6: %.1fs; loss %.4f; %d parameters with gradients (%d frozen), global grad norm %.4e (fp64 %.4e)" % (
        time.time() - t0, r["loss"], len(names), len(no_grad), gn, float(out["grad_norm64"])))
    print("  reference self-noise: kp %.2e; gradients median %.2e, 90%% %.2e, max %.2e; fp32 svd backward %.2e" % (
        kp_noise, noises[len(noises) // 2], noises[int(len(noises) * 0.9)], noises[-1], float(out["svd32_rel"])))
    return ok, out


def main():
    torch.manual_seed(0)
    mvn = ref_loader.load()
    which = sys.argv[1:] or list(VOL_SETTINGS) + ["alg_ft_trunk"]
    for name in which:
        case = dict(ALG_CASE if name == "alg_ft_trunk" else CASE)
        while True:
            ok, out = run_alg(mvn, case) if name == "alg_ft_trunk" else run_vol(mvn, name, case)
            if ok:
                break
            case["seed"] += 1000
        path = os.path.join(GOLD, "train_step_%s.npz" % name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote %s: %d bytes" % (path, size))
        assert size < truth.MAX_BYTES, size


if __name__ == "__main__":
    main()
