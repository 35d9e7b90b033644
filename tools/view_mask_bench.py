"""The masked quad gather against the unmasked one, in one process; prints one JSON line and writes profiles/view_mask_bench.json.

    python tools/view_mask_bench.py [--batch 8] [--views 4] [--maps 96] [--volume 64] [--reps 1000] [--rounds 7] [--out profiles/view_mask_bench.json]

Shape: the gather of BASELINE config 2 (bf16, 4 views of 96 x 96 x 32 feature maps, 64^3 voxels, 8 samples; the ring cameras of oracle/synth.py, the cuboid
at the point they look at), through the grid entry the models record.  Three launches, interleaved round by round so that clock drift hits all of them:
  (a) unmasked      lt_unproject_grid_fwd           the quad kernel as it was;
  (b) masked_ones   lt_unproject_grid_masked_fwd    all-ones mask: the same arithmetic, plus the mask bits and one scalar branch per view;
  (c) masked_3of4   lt_unproject_grid_masked_fwd    view 1 of every sample masked: no loads, no blend, no exp2 for that view.
Timing: device events around --reps back-to-back launches (per launch = elapsed / reps), after a warm-up of every variant; per variant the median of the
--rounds round values and the spread (max - min of the round values).  Bytes: the algorithmic traffic of SURVEY 8d (the valid views' maps once + the volume
once + the returned coordinates)."""
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

from oracle import synth  # noqa: E402
from oracle import vol_oracle as O  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=4, choices=[4, 8])
    ap.add_argument("--maps", type=int, default=96)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--reps", type=int, default=1000)          # ~0.12 s per timed window at this shape
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_mask_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "view_mask_bench needs a GPU"
    import lt_hip as H
    B, NV, hw, V, Cc = args.batch, args.views, args.maps, args.volume, 32
    g = torch.Generator().manual_seed(5)
    K, R, t = synth.ring_cameras(NV, 4 * hw)
    P = torch.from_numpy(O.resized_projection(K, R, t, (4 * hw, 4 * hw), (hw, hw))).float()[None].repeat(B, 1, 1, 1).contiguous().to(DEV)
    feats = torch.randn(B, NV, hw, hw, Cc, generator=g).to(DEV).bfloat16().contiguous()
    side = 2500.0
    base = (torch.randn(B, 3, generator=g) * 100).numpy().astype(np.float64)
    pos = torch.from_numpy((base - side / 2).astype(np.float32)).to(DEV)
    cen = torch.from_numpy(base.astype(np.float32)).to(DEV)
    rot = torch.eye(3).reshape(1, 9).repeat(B, 1).contiguous().to(DEV)
    step = float(np.float32(side / (V - 1)))
    coords = torch.empty(B, V, V, V, 3, dtype=torch.float32, device=DEV)
    outs = {k: torch.empty(B, V, V, V, Cc, dtype=torch.bfloat16, device=DEV) for k in ("unmasked", "masked_ones", "masked_3of4")}
    ones = torch.ones(B, NV, dtype=torch.uint8, device=DEV)
    part = ones.clone()
    part[:, 1] = 0
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    code, agg = H.LT_BF16, H.AGG["softmax"]

    def launch(name):
        o = outs[name]
        if name == "unmasked":
            H.check(lib.lt_unproject_grid_fwd(code, feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0, coords.data_ptr(), None,
                                              o.data_ptr(), B, NV, Cc, hw, hw, V, agg, st), "lt_unproject_grid_fwd")
        else:
            m = ones if name == "masked_ones" else part
            H.check(lib.lt_unproject_grid_masked_fwd(code, feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0, coords.data_ptr(), None,
                                                     m.data_ptr(), o.data_ptr(), B, NV, Cc, hw, hw, V, agg, st), "lt_unproject_grid_masked_fwd")

    def timed(name):
        e0, e1 = H.Event(), H.Event()
        e0.record(st)
        for _ in range(args.reps):
            launch(name)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / args.reps

    names = list(outs)
    for _ in range(3):
        for n in names:
            launch(n)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["unmasked"], outs["masked_ones"]))
    finite = bool(torch.isfinite(outs["masked_3of4"].float()).all())
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            rounds[n].append(timed(n))
    esz = 2
    nbytes = lambda nv: B * nv * hw * hw * Cc * esz + B * V ** 3 * Cc * esz + B * V ** 3 * 12
    res = {"shape": {"batch": B, "views": NV, "maps": [hw, hw, Cc], "volume": V, "dtype": "bf16"}, "reps": args.reps, "rounds": args.rounds,
           "all_ones_mask_bit_identical_to_unmasked": same, "masked_3of4_finite": finite}
    for n in names:
        v = rounds[n]
        res[n + "_ms"] = float(np.median(v))
        res[n + "_ms_min"] = float(np.min(v))
        res[n + "_spread_ms"] = float(np.max(v) - np.min(v))
        res[n + "_algorithmic_gb_per_s"] = nbytes(NV - 1 if n == "masked_3of4" else NV) / (res[n + "_ms"] * 1e-3) / 1e9
    res["masked_ones_minus_unmasked_ms"] = res["masked_ones_ms"] - res["unmasked_ms"]
    res["masked_ones_within_unmasked_spread"] = bool(res["masked_ones_ms"] <= res["unmasked_ms"] + res["unmasked_spread_ms"])
    res["masked_3of4_over_unmasked"] = res["masked_3of4_ms"] / res["unmasked_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
