"""Generates tests/golden/heatmap2d_ops.npz and tests/golden/train_step_heatmap2d.npz by running the REFERENCE on the CPU where the reference tree is
available (the same loader as oracle/make_golden.py).  Writes only those two files (data: arrays and names, no code):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_heatmap2d.py

heatmap2d_ops.npz -- the 2D Gaussian targets (the reference's op.render_points_as_2d_gaussians / gaussian_2d_pdf).  Per case ``c<k>/``: points and
sigmas (6, 2), shape (h, w), normalize; ``ref32`` the reference's render in fp32; ``f64`` the same function of the reference evaluated in fp64 (its
inputs as doubles); ``ref_err`` per heatmap max|ref32 - f64| * norm, the reference's own fp32 error relative to the Gaussian's peak 1 / norm.  The four
shapes are the ones the kernel tests run: fewer pixels than a wave, a vector-path map under 256 pixels, one over 256 pixels that is no multiple of it,
an odd width.  Points: on a pixel centre, between pixels, outside the map in x and in y (which side changes from case to case: all four occur), far
outside (the target underflows to 0); anisotropic sigmas from 0.5 to 3.5.

train_step_heatmap2d.npz -- two whole training steps of the reference with a heatmap loss, stored like oracle/make_golden.py's gen_train_alg stores
its step (sub-sampled gradients, per-parameter self-noise from an 8-thread / 1-thread / images x (1 + 1e-6) run, the same step in fp64, running
statistics, parameters after torch.optim.Adam; keys prefixed ``b/`` and ``c/``):
  b/  the 2D backbone ALONE: get_pose_net, ResNet-18 (basic blocks), 4 images of 128^2 (heatmaps 32^2), 17 joints, no confidence heads, train();
      target render_points_as_2d_gaussians(gt, sigma 2, normalize=False); loss sum(validity (hm - G)^2) / (h w max(1, sum validity)), one joint invalid;
      Adam lr 1e-5.  The seed is the first from 31 on which the reference's own gradients survive additive image noise (gen_backbone).
  c/ AlgebraicTriangulationNet (gen_train_alg's case: heatmap_multiplier 1, use_confidences) with MSESmooth(3D) + lam * that heatmap loss
      (normalize=True) on the RETURNED softmaxed heatmaps; lam balances the two terms' gradient norms (both printed), so that each moves the total by
      well over 10 %.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader, spec, synth, truth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SHAPES = [(5, 7), (8, 12), (33, 24), (32, 33)]
SIGMAS = np.array([[0.5, 3.5], [3.5, 0.5], [1.0, 2.0], [2.5, 1.5], [2.0, 2.0], [1.25, 3.0]], dtype=np.float32)
NSUB = 129


def op_points(h, w, k):
    """Six keypoints for case k of an (h, w) map: pixel centre, between pixels, outside in x, outside in y, a corner pixel's inside, far outside."""
    x_out = -2.5 if k % 2 == 0 else w + 1.25
    y_out = -3.0 if (k // 2) % 2 == 0 else h + 2.2
    return np.array([[3.0, 2.0], [w / 2 + 0.37, h / 2 - 0.61], [x_out, 1.0], [w - 1.5, y_out], [0.25, h - 1.3], [1.0e4, -1.0e4]], dtype=np.float32)


def gen_ops(mvn):
    render = mvn.utils.op.render_points_as_2d_gaussians
    out, k = {}, 0
    for h, w in SHAPES:
        for normalize in (False, True):
            pts, sg = torch.from_numpy(op_points(h, w, k)), torch.from_numpy(SIGMAS)
            r32 = render(pts, sg, (h, w), normalize=normalize)
            r64 = render(pts.double(), sg.double(), (h, w), normalize=normalize)
            assert r32.dtype == torch.float32 and r64.dtype == torch.float64
            norm = 2 * np.pi * sg[:, 0].double() ** 2 if normalize else torch.ones(len(sg), dtype=torch.float64)
            err = (r32.double() - r64).abs().amax(dim=(1, 2)) * norm
            p = "c%d/" % k
            out.update({p + "points": pts.numpy(), p + "sigmas": sg.numpy(), p + "shape": np.array([h, w]), p + "normalize": np.array(int(normalize)),
                        p + "ref32": r32.numpy(), p + "f64": r64.numpy(), p + "ref_err": err.numpy()})
            print("  ops case %d: %dx%d normalize=%d: reference fp32 error relative to the peak, per heatmap: %s" % (
                k, h, w, normalize, " ".join("%.1e" % e for e in err.tolist())))
            k += 1
    out["n_cases"] = np.array(k)
    path = os.path.join(GOLD, "heatmap2d_ops.npz")
    np.savez_compressed(path, **out)
    return path


def subsample(t, n=NSUB):
    """At most n evenly strided values of a tensor, as a flat numpy array."""
    flat = t.detach().reshape(-1)
    return flat[::max(1, flat.numel() // n)][:n].numpy().copy()


def heatmap_loss(mvn, hm, gt2d, val, sigma, normalize):
    """The heatmap loss written with the reference's functions: hm (..., J, h, w), gt2d (..., J, 2) heatmap pixels, val (..., J, 1)."""
    h, w = hm.shape[-2:]
    pts = gt2d.reshape(-1, 2)
    target = mvn.utils.op.render_points_as_2d_gaussians(pts, torch.full_like(pts, sigma), (h, w), normalize=normalize).reshape(hm.shape)
    return torch.sum((hm - target) ** 2 * val[..., None]) / (h * w * torch.clamp(torch.sum(val), min=1))


def store_step(out, pre, runs, ref64, opt):
    """Gradients of runs[0] (the fixture's step), their self-noise against the other runs, the fp64 step's, the state after opt.step()."""
    ref = runs[0]
    others = [dict(r.named_parameters()) for r in runs[1:]]
    g64 = dict(ref64.named_parameters())
    names, no_grad, noises = [], [], []
    for n, p in ref.named_parameters():
        if p.grad is None:
            no_grad.append(n)
            continue
        names.append(n)
        gmax = float(p.grad.abs().max())
        out[pre + "g/" + n] = subsample(p.grad)
        out[pre + "gn/" + n] = np.array([float(p.grad.double().norm()), gmax, float(p.grad.double().sum())])
        noise = max(float((o[n].grad - p.grad).abs().max()) for o in others) / max(gmax, 1e-30)
        out[pre + "noise/" + n] = np.array(noise)
        noises.append(noise)
        out[pre + "g64/" + n] = subsample(g64[n].grad)
        out[pre + "gn64/" + n] = np.array([float(g64[n].grad.norm()), float(g64[n].grad.abs().max())])
    gn = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters() if p.grad is not None)))
    out[pre + "grad_norm"] = np.array(gn)
    out[pre + "grad_norm64"] = np.array(float(torch.sqrt(sum(p.grad.pow(2).sum() for p in ref64.parameters() if p.grad is not None))))
    opt.step()
    for n, p in ref.named_parameters():
        if n in names:
            out[pre + "p1/" + n] = subsample(p)
    for n, b_ in ref.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            out[pre + "rs/" + n] = subsample(b_)
    out[pre + "names"], out[pre + "no_grad"] = np.array(names), np.array(no_grad, dtype=str)
    noises = np.sort(np.array(noises))
    print("  %s %d parameters with gradients (%d without), global grad norm %.4e (fp64 step %.4e); self-noise median %.2e, 90%% %.2e, max %.2e" % (
        pre, len(names), len(no_grad), gn, float(out[pre + "grad_norm64"]), noises[len(noises) // 2], noises[int(len(noises) * 0.9)], noises[-1]))


def three_runs(step):
    """The fixture's run (8 threads), a 1-thread run, a run on images x (1 + 1e-6), and the fp64 run."""
    torch.set_num_threads(8)
    a = step()
    torch.set_num_threads(1)
    b = step()
    torch.set_num_threads(8)
    c = step(eps=1e-6)
    d = step(dt=torch.float64)
    return a, b, c, d


STABLE_NOISE, STABLE_GATE = (1e-6, 3e-6), 2.5e-4


def gen_backbone(mvn, out, seed=31):
    """Training-mode BatchNorm over 4 images, ReLUs and a max-pool make the step's gradients a DISCONTINUOUS function of the forward: on some seeds an
    activation sits so close to a switch that additive image noise of 1e-6 -- a forward deviation of the size any other fp32 implementation has -- flips it
    and moves the reference's own gradients by 1e-3 and more, in fp64 as in fp32 (seed 31: median 6e-4, max 1.7e-3; at 3e-7 it moves them by 1e-6).  The
    stored self-noise cannot show that: images x (1 + 1e-6) is undone exactly by the first BatchNorm.  So, as tools/make_golden_train_view_mask.py does,
    the seed is advanced until the REFERENCE passes a gate of its own: under additive image noise of 1e-6 and of 3e-6 every parameter gradient stays
    within 2.5e-4 (of its largest entry) of the unperturbed step's.  Only the reference is looked at; the stored noise keeps the three-run recipe."""
    while not _gen_backbone(mvn, out, seed):
        seed += 1


def _gen_backbone(mvn, out, seed):
    c = dict(nl=18, N=4, H=128, J=17, seed=seed)
    cfg = synth.alg_config(c["nl"], False).model.backbone
    cfg.alg_confidences, cfg.vol_confidences = False, False
    sd = synth.make_state_dict(spec.pose_resnet_spec(c["nl"], c["J"]), seed=c["seed"], basic_block=True)
    images = synth.make_inputs(1, c["N"], c["H"], seed=c["seed"], inside=False)["images"][0]
    g = torch.Generator().manual_seed(45)
    gt2d = torch.rand(c["N"], c["J"], 2, generator=g) * 36 - 2          # heatmap pixels of a 32 x 32 map; a few keypoints just outside it
    val = torch.ones(c["N"], c["J"], 1); val[1, 5] = 0
    lr, sigma = 1e-5, 2.0

    def step(eps=0.0, dt=torch.float32, noise=0.0):
        ref = mvn.models.pose_resnet.get_pose_net(cfg, device="cpu")
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.to(dt)
        opt = torch.optim.Adam(ref.parameters(), lr=lr)
        x = images * (1.0 + eps)
        if noise:
            x = x + noise * torch.randn(images.shape, generator=torch.Generator().manual_seed(1))
        hm, feats, algc, volc = ref(x.to(dt))
        assert algc is None and volc is None
        loss = heatmap_loss(mvn, hm, gt2d.to(dt), val.to(dt), sigma, False)
        opt.zero_grad()
        loss.backward()
        return ref, opt, dict(hm=hm.detach(), feats=feats.detach(), loss=float(loss))

    t0 = time.time()
    torch.set_num_threads(8)
    base = dict(step()[0].named_parameters())
    for amp in STABLE_NOISE:
        moved = max(float((p.grad - base[n].grad).abs().max() / base[n].grad.abs().max()) for n, p in step(noise=amp)[0].named_parameters())
        print("  b/ seed %d: additive image noise %.0e moves the reference's gradients by at most %.2e (gate %.1e)" % (seed, amp, moved, STABLE_GATE))
        if moved > STABLE_GATE:
            return False
    (ref, opt, r), (ref1, _, r1), (refp, _, rp), (ref64, _, r64) = three_runs(step)
    hm = r["hm"]
    floor =float(hm.double().pow(2).mean().sqrt())          # an entry near zero carries the absolute error of a sum of rms-sized terms
    hm_noise = max(float(((o["hm"] - hm).abs() / hm.abs().clamp(min=floor)).max()) for o in (r1, rp))
    pre = "b/"
    out.update({pre + "case_keys": np.array(sorted(c)), pre + "case": np.array([c[k] for k in sorted(c)]), pre + "gt2d": gt2d.numpy(), pre + "val": val.numpy(),
                pre + "sigma": np.array(sigma), pre + "lr": np.array(lr), pre + "loss": np.array(r["loss"]), pre + "loss64": np.array(r64["loss"]),
                pre + "loss_noise": np.array(max(abs(o["loss"] - r["loss"]) / r["loss"] for o in (r1, rp))),
                pre + "hm_sub": hm[:, :, ::2, ::2].numpy().copy(), pre + "hm_floor": np.array(floor), pre + "hm_noise": np.array(hm_noise),
                pre + "feat_sub": r["feats"][:, ::8, ::4, ::4].numpy().copy()})
    print("  b/ backbone step x4: %.1fs; loss %.6f (fp64 %.6f, noise %.1e); logits rms %.3e, self-noise %.2e" % (
        time.time() - t0, r["loss"], r64["loss"], float(out[pre + "loss_noise"]), floor, hm_noise))
    store_step(out, pre, [ref, ref1, refp], ref64, opt)
    return True


def gen_alg(mvn, out):
    import mvn.models.loss as L
    c = dict(nl=18, B=2, NV=3, H=128, seed=21)          # gen_train_alg's case
    cfg = synth.alg_config(c["nl"], True)
    cfg.model.heatmap_multiplier = 1.0
    sd = synth.make_state_dict(spec.alg_net_spec(c["nl"], 17, True), seed=c["seed"], basic_block=True)
    inp = synth.make_inputs(c["B"], c["NV"], c["H"], seed=c["seed"], inside=False)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(c["B"], 1, 1, 1)
    lr, sigma = 1e-5, 2.0
    g = torch.Generator().manual_seed(46)
    dgt = torch.randn(c["B"], 17, 3, generator=g) * 40
    d2d = torch.randn(c["B"], c["NV"], 17, 2, generator=g) * 1.5
    val = torch.ones(c["B"], 17, 1); val[0, 3] = 0
    val2d = val[:, None].repeat(1, c["NV"], 1, 1)
    fixed = {}

    def step(eps=0.0, dt=torch.float32, lam=None, parts=False):
        ref = mvn.models.triangulation.AlgebraicTriangulationNet(cfg, device="cpu")
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.to(dt)
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, ref.parameters()), lr=lr)
        kp3, kp2, hm, conf = ref((inp["images"] * (1.0 + eps)).to(dt), P.to(dt), {})
        if not fixed:          # the targets of every run: the first run's predictions plus noise
            h, w = hm.shape[-2:]
            fixed["gt"] = kp3.detach() + dgt
            fixed["gt2d"] = (kp2.detach() * torch.tensor([w / c["H"], h / c["H"]]) + d2d).float()
        l3 = L.KeypointsMSESmoothLoss(400)(kp3 * 0.1, fixed["gt"].to(dt) * 0.1, val.to(dt))
        lh = heatmap_loss(mvn, hm, fixed["gt2d"].to(dt), val2d.to(dt), sigma, True)
        if parts:          # the two terms' gradient norms, each alone
            norms = []
            for term in (l3, lh):
                opt.zero_grad()
                term.backward(retain_graph=True)
                norms.append(float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters() if p.grad is not None))))
            return norms
        opt.zero_grad()
        (l3 + lam * lh).backward()
        return ref, opt, dict(kp3=kp3.detach(), kp2=kp2.detach(), hm=hm.detach(), conf=conf.detach(), l3=float(l3), lh=float(lh), loss=float(l3 + lam * lh))

    t0 = time.time()
    torch.set_num_threads(8)
    n3, nh = step(parts=True)
    lam = float("%.1e" % (n3 / nh))
    print("  c/ gradient norm of MSESmooth(3D) alone %.4e, of the heatmap loss alone %.4e -> lam = %.1e" % (n3, nh, lam))
    (ref, opt, r), (ref1, _, r1), (refp, _, rp), (ref64, _, r64) = three_runs(lambda **kw: step(lam=lam, **kw))
    kp = r["kp3"]
    kp_noise = max(float(((o["kp3"] - kp).abs() / kp.abs().clamp(min=1.0)).max()) for o in (r1, rp))
    pre = "c/"
    out.update({pre + "kp3": kp.numpy(), pre + "kp2": r["kp2"].numpy(), pre + "conf": r["conf"].numpy(), pre + "gt": fixed["gt"].numpy(), pre + "gt2d": fixed["gt2d"].numpy(),
                pre + "val": val.numpy(), pre + "P": P.numpy(), pre + "lr": np.array(lr), pre + "sigma": np.array(sigma), pre + "lam": np.array(lam),
                pre + "loss": np.array(r["loss"]), pre + "loss3d": np.array(r["l3"]), pre + "loss_hm": np.array(r["lh"]), pre + "loss64": np.array(r64["loss"]),
                pre + "loss_noise": np.array(max(abs(o["loss"] - r["loss"]) / r["loss"] for o in (r1, rp))), pre + "kp_noise": np.array(kp_noise),
                pre + "term_grad_norms": np.array([n3, nh]),
                pre + "hm_sub": r["hm"].reshape(c["B"] * c["NV"], *r["hm"].shape[2:])[:, :, ::2, ::2].numpy().copy()})
    store_step(out, pre, [ref, ref1, refp], ref64, opt)
    gt_ = float(out[pre + "grad_norm"])
    print("  c/ alg step x6: %.1fs; loss %.5f = %.5f + lam * %.5e; total gradient norm %.4e: %.0f %% away from the 3D term's, %.0f %% from lam x the heatmap term's" % (
        time.time() - t0, r["loss"], r["l3"], r["lh"], gt_, 100 * abs(gt_ - n3) / n3, 100 * abs(gt_ - lam * nh) / (lam * nh)))
    assert abs(gt_ - n3) >= 0.1 * n3 and abs(gt_ - lam * nh) >= 0.1 * lam * nh, "a term moves the gradient norm by less than 10 %"


def main():
    torch.manual_seed(0)
    mvn = ref_loader.load()
    paths = [gen_ops(mvn)]
    out = {}
    gen_backbone(mvn, out)
    gen_alg(mvn, out)
    paths.append(os.path.join(GOLD, "train_step_heatmap2d.npz"))
    np.savez_compressed(paths[-1], **out)
    for p in paths:
        size = os.path.getsize(p)
        print("wrote %s: %d bytes" % (p, size))
        assert size < truth.MAX_BYTES, size


if __name__ == "__main__":
    main()
