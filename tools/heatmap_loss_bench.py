"""The fused heatmap loss against the same loss as tensor expressions, measured (GPU box): python tools/heatmap_loss_bench.py [--batch 8] [--rounds 5] [--steps 3]

The algebraic training shape (ResNet-152, 4 views of 384 x 384, 17 joints, ``--batch`` samples per step: 32 images, 544 heatmaps of 96 x 96), per precision
(fp32, act16), in a fresh child process under its own time limit (a non-zero status ends the script):

    step, fused        one full training step of AlgebraicTriangulationNet -- forward, MSESmooth(3D) + HeatmapMSELoss(normalize=True) on the returned heatmaps,
                       backward, Adam -- with loss.HeatmapMSELoss (one lt_heatmap_mse_fwd launch, the target never written)
    step, expressions  the same step with the loss written the way the reference writes it: an (N J, h, w, 2) grid, three repeats, the target, the square
    loss alone         forward + backward of the loss on a (N J, h, w) prediction, both ways

The two variants ALTERNATE round by round in one process (same clocks, same allocator state); reported: the median of the rounds' ms, their spread (max - min),
and the peak memory of the loss alone.  No threshold is promised: the numbers go to profiles/heatmap_loss_bench.json (and are printed)."""
import argparse
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "learnable-triangulation-pytorch_amd")); sys.path.insert(0, R)


def expression_loss(hm, gt2d, val, sigma, normalize):
    """The heatmap loss as tensor expressions on the GPU, materialising what the reference materialises (op.py:178-196)."""
    import numpy as np
    import torch
    h, w = hm.shape[-2:]
    pts = gt2d.reshape(-1, 2)
    n = pts.shape[0]
    yy, xx = torch.meshgrid(torch.arange(h, device=hm.device), torch.arange(w, device=hm.device), indexing="ij")
    grid = torch.stack([xx, yy], dim=-1).float().unsqueeze(0).repeat(n, 1, 1, 1).reshape(-1, 2)
    means = pts[:, None, None, :].repeat(1, h, w, 1).reshape(-1, 2)
    sig = torch.full_like(pts, sigma)[:, None, None, :].repeat(1, h, w, 1).reshape(-1, 2)
    g = torch.exp(-((grid[:, 0] - means[:, 0]) ** 2 / sig[:, 0] ** 2 + (grid[:, 1] - means[:, 1]) ** 2 / sig[:, 1] ** 2) / 2)
    if normalize:
        g = g / (2 * np.pi * sig[:, 0] * sig[:, 0])
    target = g.reshape(hm.shape)
    v = val.reshape(hm.shape[:-2] + (1, 1))
    return torch.sum((hm - target) ** 2 * v) / (h * w * torch.clamp(torch.sum(val), min=1))


def child(a):
    import numpy as np
    import torch
    import bench
    import lt_train
    from mvn.models import loss as L
    from mvn.models.triangulation import AlgebraicTriangulationNet
    from mvn.utils.cfg import ConfigDict
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, NV, J, HW = a.batch, 4, 17, 384
    cfg = ConfigDict({"model": {"name": "alg", "init_weights": False, "checkpoint": "", "use_confidences": True, "heatmap_multiplier": 1.0, "heatmap_softmax": True,
                                "backbone": {"name": "resnet152", "style": "simple", "init_weights": False, "checkpoint": "", "num_joints": J, "num_layers": 152}}})
    m = AlgebraicTriangulationNet(cfg, device=dev)
    m.to(dev).train()
    m.train_precision = a.precision
    images, batch, (K, Rm, t) = bench.synthetic_batch(B, NV, HW, 1000)
    images = images.to(dev)
    P = torch.from_numpy(K @ np.concatenate([Rm, t], -1)).float()[None].repeat(B, 1, 1, 1).to(dev)
    opt = lt_train.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-5)
    g = torch.Generator().manual_seed(5)
    gt = (torch.randn(B, J, 3, generator=g) * 100).to(dev)
    h = w = HW // 4
    gt2d = (torch.rand(B, NV, J, 2, generator=g) * (w - 1)).to(dev)
    val = torch.ones(B, J, 1, device=dev); val[0, 3] = 0
    val2d = val[:, None].repeat(1, NV, 1, 1)
    crit3, fused = L.KeypointsMSESmoothLoss(400), L.HeatmapMSELoss(sigma=2.0, normalize=True)
    variants = {"fused": lambda hm: fused(hm, gt2d, val2d), "expressions": lambda hm: expression_loss(hm, gt2d, val2d, 2.0, True)}

    def step(kind):
        kp3, _, hm, _ = m(images, P, {})
        loss = crit3(kp3 * 0.1, gt * 0.1, val) + variants[kind](hm)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            last = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, last

    for kind in ("fused", "expressions", "fused", "expressions"):          # the recording step and a replay of each
        last = step(kind)
    rounds = {"fused": [], "expressions": []}
    for _ in range(a.rounds):
        for kind in rounds:
            ms, last = timed(lambda: step(kind), a.steps)
            rounds[kind].append(ms)
    assert bool(torch.isfinite(last)), float(last)
    # the loss alone: forward + backward on a prediction of the step's shape
    pred = torch.randn(B, NV, J, h, w, device=dev).softmax(-1).requires_grad_(True)
    alone, peak = {"fused": [], "expressions": []}, {}

    def loss_only(kind):
        pred.grad = None
        l = variants[kind](pred)
        l.backward()
        return l.detach()
    for kind in alone:
        loss_only(kind)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        loss_only(kind)
        torch.cuda.synchronize()
        peak[kind] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
    for _ in range(a.rounds):
        for kind in alone:
            alone[kind].append(timed(lambda: loss_only(kind), 20)[0])
    both = [float(loss_only(k)) for k in alone]
    med = lambda v: float(np.median(v))
    res = {"precision": a.precision, "batch": B, "heatmaps": B * NV * J, "heatmap_hw": [h, w],
           "step_ms": {k: {"rounds": v, "median": med(v), "spread": max(v) - min(v)} for k, v in rounds.items()},
           "loss_alone_ms": {k: {"rounds": v, "median": med(v), "spread": max(v) - min(v), "peak_extra_memory_mb": peak[k]} for k, v in alone.items()},
           "loss_values_fused_vs_expressions": both}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--precisions", default="fp32,act16")
    ap.add_argument("--timeout", type=int, default=280, help="seconds per child process")
    ap.add_argument("--precision", help="(child) run this one precision")
    a = ap.parse_args()
    if a.precision:
        return child(a)
    out = {"shape": "AlgebraicTriangulationNet, ResNet-152, 4 views x 384^2, 17 joints, %d samples per step" % a.batch, "rounds": a.rounds,
           "steps_per_round": a.steps, "method": "variants alternate round by round in one process; median and max - min over the rounds", "results": []}
    for prec in a.precisions.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--precision", prec, "--batch", str(a.batch),
               "--rounds", str(a.rounds), "--steps", str(a.steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            print(p.stdout[-4000:])
            print("heatmap_loss_bench: %s ended with status %d; nothing more is started" % (prec, p.returncode))
            sys.exit(p.returncode)
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        out["results"].append(r)
        for what in ("step_ms", "loss_alone_ms"):
            print("%-6s %-14s fused %9.3f ms (spread %.3f)   expressions %9.3f ms (spread %.3f)" % (
                prec, what, r[what]["fused"]["median"], r[what]["fused"]["spread"], r[what]["expressions"]["median"], r[what]["expressions"]["spread"]), flush=True)
    os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
    path = os.path.join(R, "profiles", "heatmap_loss_bench.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote " + path)


if __name__ == "__main__":
    main()
