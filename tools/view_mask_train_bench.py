"""The masked unprojection backward against the unmasked one, in one process; prints one JSON line and writes profiles/view_mask_train_bench.json.

    python tools/view_mask_train_bench.py [--batch 8] [--views 4 16] [--maps 96] [--volume 64] [--reps 10] [--rounds 7] [--dtype bf16]

Shape: the unprojection backward of BASELINE config 2 (8 samples, 4 views of 96 x 96 x 32 feature maps, 64^3 voxels, view softmax; the ring cameras of
oracle/synth.py, the cuboid at the point they look at), and the same at 16 views (the many-view kernels); maps in bf16 (the act16 step) unless --dtype fp32.
Workspace as the training step hands it over (one buffer, capped at op.UNPROJECT_BWD_WORKSPACE_CAP: at 16 views the entry walks the batch in chunks).
Three calls per view count, interleaved round by round so that clock drift hits all of them:
  (a) unmasked      lt_unproject_bwd            K0 / K1 / K2 as they were;
  (b) masked_ones   lt_unproject_masked_bwd     all-ones mask: the same arithmetic, plus the mask bits and one scalar branch per view and pass;
  (c) masked_3of4   lt_unproject_masked_bwd     every fourth view (1, 5, 9, ...) of every sample masked: no projection, no samples, no dx stores and no
                                                bricks to gather for those views -- their tiles are still zero-filled and stored.
Timing: device events around --reps back-to-back calls (per call = elapsed / reps), after a warm-up of every variant; per variant the median of the --rounds
round values and the spread (max - min of the round values)."""
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
NAMES = ("unmasked", "masked_ones", "masked_3of4")


def measure(B, NV, hw, V, dtype, reps, rounds):
    import lt_hip as H
    from mvn.utils import op
    Cc = 32
    g = torch.Generator().manual_seed(5)
    K, R, t = synth.ring_cameras(NV, 4 * hw)
    P = torch.from_numpy(O.resized_projection(K, R, t, (4 * hw, 4 * hw), (hw, hw))).float()[None].repeat(B, 1, 1, 1).contiguous().to(DEV)
    feats = torch.randn(B, NV, hw, hw, Cc, generator=g).to(DEV).to(dtype).contiguous()
    base = (torch.randn(B, 3, generator=g) * 100).numpy().astype(np.float64)
    coords = op.build_coord_volumes(base, 2500.0, V, device=DEV)
    gout = torch.randn(B, V, V, V, Cc, generator=g).to(DEV)
    ones = torch.ones(B, NV, dtype=torch.uint8, device=DEV)
    part = ones.clone()
    part[:, 1::4] = 0
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    per_sample = lib.lt_unproject_bwd_workspace(1, NV, Cc, V, V, V)
    nws = int(max(16, min(per_sample * B, max(per_sample, op.UNPROJECT_BWD_WORKSPACE_CAP))))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    outs = {n: torch.empty(B, NV, hw, hw, Cc, dtype=torch.float32, device=DEV) for n in NAMES}
    code, agg = H.dtype_code(dtype), H.AGG["softmax"]

    def launch(name):
        o = outs[name]
        if name == "unmasked":
            H.check(lib.lt_unproject_bwd(code, feats.data_ptr(), P.data_ptr(), coords.data_ptr(), None, gout.data_ptr(), o.data_ptr(), None, B, NV, Cc, hw, hw,
                                         V, V, V, agg, ws.data_ptr(), nws, st), "lt_unproject_bwd")
        else:
            m = ones if name == "masked_ones" else part
            H.check(lib.lt_unproject_masked_bwd(code, feats.data_ptr(), P.data_ptr(), coords.data_ptr(), None, m.data_ptr(), gout.data_ptr(), o.data_ptr(), None,
                                                B, NV, Cc, hw, hw, V, V, V, agg, ws.data_ptr(), nws, st), "lt_unproject_masked_bwd")

    def timed(name):
        e0, e1 = H.Event(), H.Event()
        e0.record(st)
        for _ in range(reps):
            launch(name)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / reps

    for _ in range(2):
        for n in NAMES:
            launch(n)
    torch.cuda.synchronize()
    res = {"views": NV, "workspace_bytes": nws, "batch_chunks": -(-B // max(1, min(B, nws // per_sample))),
           "all_ones_mask_bit_identical_to_unmasked": bool(torch.equal(outs["unmasked"], outs["masked_ones"])),
           "masked_3of4_finite": bool(torch.isfinite(outs["masked_3of4"]).all()),
           "masked_3of4_masked_views_zero": bool((outs["masked_3of4"][:, 1::4] == 0).all())}
    vals = {n: [] for n in NAMES}
    for _ in range(rounds):
        for n in NAMES:
            vals[n].append(timed(n))
    for n in NAMES:
        v = vals[n]
        res[n + "_ms"] = float(np.median(v))
        res[n + "_ms_min"] = float(np.min(v))
        res[n + "_spread_ms"] = float(np.max(v) - np.min(v))
    res["masked_ones_over_unmasked"] = res["masked_ones_ms"] / res["unmasked_ms"]
    res["masked_ones_within_unmasked_spread"] = bool(res["masked_ones_ms"] <= res["unmasked_ms"] + res["unmasked_spread_ms"])
    res["masked_3of4_over_unmasked"] = res["masked_3of4_ms"] / res["unmasked_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--maps", type=int, default=96)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_mask_train_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "view_mask_train_bench needs a GPU"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    res = {"shape": {"batch": args.batch, "maps": [args.maps, args.maps, 32], "volume": args.volume, "dtype": args.dtype, "aggregation": "softmax"},
           "reps": args.reps, "rounds": args.rounds}
    for NV in args.views:
        res["views_%d" % NV] = measure(args.batch, NV, args.maps, args.volume, dtype, args.reps, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
