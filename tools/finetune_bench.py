"""Fine-tuning with frozen parameters, measured (GPU box): python tools/finetune_bench.py [--batch 8] [--rounds 5] [--steps 4] [--precisions act16,fp32]

BASELINE config 2's shape (ResNet-152, 4 views of 384 x 384, 64^3 voxels), ``--batch`` samples per step, one full training step (forward, MAE + 0.01 x
VolumetricCELoss, backward, three-group Adam) in three settings per precision:

    all_trainable          every parameter trainable, model.train(): the yardstick (its op list is what the step has always recorded)
    frozen_train_bn        backbone.requires_grad_(False), model.train(): the backbone's backward is not recorded, its BatchNorm keeps batch statistics
    frozen_eval            backbone.requires_grad_(False), model.train(); backbone.eval(): the backbone runs as an inference plan in front of the tape
                           (LT_TRAIN_NO_FROZEN_PLAN=1 in the environment: on the tape, backward pruned)

Every setting runs in a fresh child process under its own time limit (a non-zero status ends the script): ``--rounds`` rounds of ``--steps`` steps behind
a warm-up, each round between two device synchronisations; reported per setting: the median of the rounds' ms per step, their spread (max - min), and
torch.cuda.max_memory_allocated.  For frozen_eval the per-op times of the tape (TrainTape.profile) are summed by op kind next to it.  Writes
profiles/finetune_bench.json (and prints it)."""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "learnable-triangulation-pytorch_amd")); sys.path.insert(0, R)
SETTINGS = ("all_trainable", "frozen_train_bn", "frozen_eval")


def child(a):
    import numpy as np
    import torch
    import bench
    import lt_train
    from mvn.models import loss as L
    from mvn.models.triangulation import VolumetricTriangulationNet
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = VolumetricTriangulationNet(bench.vol_config(152, 64, "fp32"), device=dev)
    m.to(dev)
    m.train()
    if a.setting != "all_trainable":
        m.backbone.requires_grad_(False)
    if a.setting == "frozen_eval":
        m.backbone.eval()
    m.train_precision = a.precision
    images, batch, _ = bench.synthetic_batch(a.batch, 4, 384, 1000)
    images = images.to(dev)
    opt = lt_train.Adam([{"params": list(m.backbone.parameters())}, {"params": list(m.process_features.parameters()), "lr": 1e-3},
                         {"params": list(m.volume_net.parameters()), "lr": 1e-3}], lr=1e-4)
    g = torch.Generator().manual_seed(5)
    gt = (torch.as_tensor(np.asarray(batch["pred_keypoints_3d"]))[:, :, :3].float() + torch.randn(a.batch, 17, 3, generator=g) * 30).to(dev)
    val = torch.ones(a.batch, 17, 1, device=dev)
    mae, ce = L.KeypointsMAELoss(), L.VolumetricCELoss()
    np.random.seed(1234)

    def step():
        kp, _, vols, _, _, cvs, _ = m(images, None, batch)
        loss = mae(kp * 0.1, gt * 0.1, val) + 0.01 * ce(cvs, vols, gt, val)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()

    for _ in range(3):          # the recording step and two replays
        last = step()
    rounds = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            last = step()
        torch.cuda.synchronize()
        rounds.append(1e3 * (time.perf_counter() - t0) / a.steps)
    assert bool(torch.isfinite(last)), float(last)
    plan = list(m._train_plans.values())[0]
    tape = plan.tape
    res = {"setting": a.setting, "precision": a.precision, "batch": a.batch, "ms_per_step_rounds": rounds, "ms_per_step_median": float(np.median(rounds)),
           "ms_per_step_spread": max(rounds) - min(rounds), "peak_memory_gb": torch.cuda.max_memory_allocated(dev) / 1e9,
           "frozen_backbone_plan": bool(getattr(plan, "frozen_plan", False)), "forward_ops": len(tape.fwd_ops), "backward_ops": len(tape.bwd_ops),
           "trainable_parameters": sum(p.numel() for p in m.parameters() if p.requires_grad), "loss_last": float(last)}
    if a.setting == "frozen_eval":
        kinds = {}
        for name, ops in (("fwd", tape.fwd_ops), ("bwd", tape.bwd_ops)):
            k = collections.defaultdict(float)
            for lab, ms in tape.profile(ops, reps=2):
                k[lab.split(" ")[0]] += ms
            kinds[name] = {n: round(v, 3) for n, v in sorted(k.items(), key=lambda kv: -kv[1])}
        res["tape_ms_by_op_kind"] = kinds
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--precisions", default="act16,fp32")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--setting", choices=SETTINGS, help="(child) run this one setting")
    ap.add_argument("--precision", help="(child)")
    a = ap.parse_args()
    if a.setting:
        return child(a)
    out = {"shape": "ResNet-152, 4 views x 384^2, 64^3 voxels, %d samples per step" % a.batch, "rounds": a.rounds, "steps_per_round": a.steps,
           "frozen_plan_switch": os.environ.get("LT_TRAIN_NO_FROZEN_PLAN"), "results": []}
    for prec in a.precisions.split(","):
        for setting in SETTINGS:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--setting", setting, "--precision", prec, "--batch", str(a.batch),
                   "--rounds", str(a.rounds), "--steps", str(a.steps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                print(p.stdout[-4000:])
                print("finetune_bench: %s / %s ended with status %d; nothing more is started" % (setting, prec, p.returncode))
                sys.exit(p.returncode)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
            r = json.loads(line[7:])
            out["results"].append(r)
            print("%-6s %-16s %8.2f ms/step (spread %.2f)  peak %.2f GB  fwd/bwd ops %d/%d" % (
                prec, setting, r["ms_per_step_median"], r["ms_per_step_spread"], r["peak_memory_gb"], r["forward_ops"], r["backward_ops"]), flush=True)
    # the three checks of the fine-tuning step, against the all-trainable step of the same run
    checks = {}
    for prec in a.precisions.split(","):
        rs = {r["setting"]: r for r in out["results"] if r["precision"] == prec}
        base, tb, ev = rs["all_trainable"], rs["frozen_train_bn"], rs["frozen_eval"]
        sp = base["ms_per_step_spread"]
        checks[prec] = {"frozen_eval_faster_by_more_than_the_spread": base["ms_per_step_median"] - ev["ms_per_step_median"] > sp,
                        "frozen_eval_peak_memory_lower": ev["peak_memory_gb"] < base["peak_memory_gb"],
                        "frozen_train_bn_not_slower_by_more_than_the_spread": tb["ms_per_step_median"] - base["ms_per_step_median"] <= sp}
    out["checks"] = checks
    os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
    path = os.path.join(R, "profiles", "finetune_bench.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(checks))
    print("wrote " + path)


if __name__ == "__main__":
    main()
