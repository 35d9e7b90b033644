"""The soft-argmax tail with and without per-joint statistics, in one process; prints one JSON line and writes profiles/keypoint_stats_bench.json.

    python tools/keypoint_stats_bench.py [--batch 8] [--joints 17] [--volume 64] [--reps 300] [--rounds 7] [--out profiles/keypoint_stats_bench.json]

Shape: the tail op of BASELINE config 2 (8 samples, 17 joints, 64^3 voxels), with the two layouts the plans hand it: planar logits (the bf16 V2V tail's:
the vectorised kernels) and channels-last logits (fp32 plans).  Four launches, interleaved round by round so that clock drift hits all of them:
  planar / channels_last              lt_softargmax3d_fwd          the tail as it is: partial, finalize, probabilities;
  planar_stats / channels_last_stats  lt_softargmax3d_stats_fwd    the same partial and finalize, the probabilities pass that also reduces the statistics,
                                                                    and their finalize.
Timing: device events around --reps back-to-back calls (per call = elapsed / reps), after a warm-up of every variant; per variant the median of the --rounds
round values and the spread (max - min of the round values).  Bytes: the algorithmic traffic -- the logits twice, the probabilities once, the coordinates
once; with statistics the coordinates once more.  The joints and probabilities of the two entry points are compared bit for bit before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "learnable-triangulation-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--reps", type=int, default=300)          # ~0.1 s per timed window at this shape
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_stats_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "keypoint_stats_bench needs a GPU"
    import lt_hip as H
    B, J, V = args.batch, args.joints, args.volume
    nvox = V ** 3
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(B, J, nvox, generator=g) * 5.0).to(DEV).contiguous()
    lg = {"planar": logits, "channels_last": logits.permute(0, 2, 1).contiguous()}
    ax = torch.linspace(-1250.0, 1250.0, V)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, nvox, 3)
    coords = (grid + torch.randn(B, 1, 3, generator=g) * 100.0).to(DEV).contiguous()
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.lt_softargmax3d_stats_workspace(B, J, nvox), dtype=torch.uint8, device=DEV)
    names = ["planar", "planar_stats", "channels_last", "channels_last_stats"]
    kp = {n: torch.empty(B, J, 3, device=DEV) for n in names}
    probs = {n: torch.empty(B, J, nvox, device=DEV) for n in names}
    rec = torch.empty(B, J, 8, device=DEV)
    idx = torch.empty(B, J, dtype=torch.int32, device=DEV)

    def launch(name):
        layout = name.replace("_stats", "")
        cl = int(layout == "channels_last")
        if name.endswith("_stats"):
            H.check(lib.lt_softargmax3d_stats_fwd(lg[layout].data_ptr(), coords.data_ptr(), 1.0, 1, cl, J, kp[name].data_ptr(), probs[name].data_ptr(), rec.data_ptr(),
                                                  idx.data_ptr(), B, J, nvox, ws.data_ptr(), st), "lt_softargmax3d_stats_fwd")
        else:
            H.check(lib.lt_softargmax3d_fwd(lg[layout].data_ptr(), coords.data_ptr(), 1.0, 1, cl, J, kp[name].data_ptr(), probs[name].data_ptr(), B, J, nvox,
                                            ws.data_ptr(), st), "lt_softargmax3d_fwd")

    def timed(name):
        e0, e1 = H.Event(), H.Event()
        e0.record(st)
        for _ in range(args.reps):
            launch(name)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / args.reps

    for _ in range(3):
        for n in names:
            launch(n)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(kp[l], kp[l + "_stats"])) and bool(torch.equal(probs[l], probs[l + "_stats"])) for l in ("planar", "channels_last"))
    peak_is_max = bool(torch.equal(rec[..., 0], probs["channels_last_stats"].max(dim=2).values))
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            rounds[n].append(timed(n))
    plain_bytes = 3 * B * J * nvox * 4 + B * nvox * 12
    res = {"shape": {"batch": B, "joints": J, "volume": V, "dtype": "fp32 logits"}, "reps": args.reps, "rounds": args.rounds,
           "joints_and_probabilities_bit_identical": same, "peak_is_the_largest_probability": peak_is_max,
           "algorithmic_bytes": {"plain": plain_bytes, "stats": plain_bytes + B * nvox * 12}}
    for n in names:
        v = rounds[n]
        res[n + "_ms"] = float(np.median(v))
        res[n + "_ms_min"] = float(np.min(v))
        res[n + "_spread_ms"] = float(np.max(v) - np.min(v))
        res[n + "_algorithmic_gb_per_s"] = (plain_bytes + (B * nvox * 12 if n.endswith("_stats") else 0)) / (res[n + "_ms"] * 1e-3) / 1e9
    for l in ("planar", "channels_last"):
        res[l + "_stats_minus_plain_ms"] = res[l + "_stats_ms"] - res[l + "_ms"]
        res[l + "_stats_over_plain"] = res[l + "_stats_ms"] / res[l + "_ms"]
    res["bytes_stats_over_plain"] = (plain_bytes + B * nvox * 12) / plain_bytes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
