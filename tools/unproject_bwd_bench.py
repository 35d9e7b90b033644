"""lt_unproject_bwd alone at 8, 9, 16 and 31 camera views, in one process; prints one JSON line and writes profiles/unproject_bwd_many_views.json.

    python tools/unproject_bwd_bench.py [--batch 2] [--views 8,9,16,31] [--maps 96] [--volume 64] [--reps 20] [--rounds 7] [--out profiles/unproject_bwd_many_views.json]

Shape: the model's -- C = 32, 96 x 96 feature maps, 64^3 voxels, fp32 and bf16 maps, 2 samples, the whole batch's workspace; the ring cameras of oracle/synth.py,
the cuboid at the point they look at.  NV = 8 runs the register kernels and is the yardstick of the same run; NV > 8 runs the many-view kernels.  Aggregations:
softmax (K1 samples every view three times beyond 8 views), conf_norm (K1 in groups of 8 views, with the confidence gradient and its finalizer) and sum (K1
only copies the upstream gradient per view: softmax minus sum is what the sampling passes of K1 cost, K0 and K2 being the same launches in both).
Timing: device events around --reps back-to-back calls (per call = elapsed / reps), after a warm-up of every variant; the variants are interleaved round by
round so that clock drift hits all of them; per variant the median of the --rounds round values and the spread (max - min).  Reported per sample and per
(sample x view)."""
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
AGGS = ("softmax", "conf_norm", "sum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--views", default="8,9,16,31")
    ap.add_argument("--maps", type=int, default=96)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unproject_bwd_many_views.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "unproject_bwd_bench needs a GPU"
    import lt_hip as H
    B, hw, V, Cc = args.batch, args.maps, args.volume, 32
    views = [int(v) for v in args.views.split(",")]
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(5)
    ax = torch.linspace(-1250.0, 1250.0, V)
    cv = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)[None].repeat(B, 1, 1, 1, 1).contiguous().to(DEV)
    G = torch.randn(B, V, V, V, Cc, generator=g).to(DEV)
    variants = {}
    for NV in views:
        K, R, t = synth.ring_cameras(NV, 4 * hw)
        P = torch.from_numpy(O.resized_projection(K, R, t, (4 * hw, 4 * hw), (hw, hw))).float()[None].repeat(B, 1, 1, 1).contiguous().to(DEV)
        f32 = torch.randn(B, NV, hw, hw, Cc, generator=g).to(DEV)
        conf = (torch.rand(B, NV, Cc, generator=g) + 0.1).to(DEV)
        nws = lib.lt_unproject_bwd_workspace(B, NV, Cc, V, V, V)
        bufs = dict(P=P, conf=conf, gf=torch.empty(B, NV, hw, hw, Cc, device=DEV), gc=torch.empty(B, NV, Cc, device=DEV),
                    ws=torch.empty(nws, dtype=torch.uint8, device=DEV), nws=nws)
        for dt, feats in (("fp32", f32), ("bf16", f32.bfloat16().contiguous())):
            for agg in AGGS:
                variants[(NV, dt, agg)] = dict(bufs, feats=feats)

    def launch(key):
        NV, dt, agg = key
        b = variants[key]
        is_conf = agg.startswith("conf")
        H.check(lib.lt_unproject_bwd(H.LT_F32 if dt == "fp32" else H.LT_BF16, b["feats"].data_ptr(), b["P"].data_ptr(), cv.data_ptr(),
                                     b["conf"].data_ptr() if is_conf else None, G.data_ptr(), b["gf"].data_ptr(), b["gc"].data_ptr() if is_conf else None,
                                     B, NV, Cc, hw, hw, V, V, V, H.AGG[agg], b["ws"].data_ptr(), b["nws"], st), "lt_unproject_bwd")

    def timed(key):
        e0, e1 = H.Event(), H.Event()
        e0.record(st)
        for _ in range(args.reps):
            launch(key)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / args.reps

    keys = list(variants)
    for _ in range(2):
        for k in keys:
            launch(k)
    torch.cuda.synchronize()
    rounds = {k: [] for k in keys}
    for _ in range(args.rounds):
        for k in keys:
            rounds[k].append(timed(k))
    res = {"shape": {"batch": B, "maps": [hw, hw, Cc], "volume": V, "views": views}, "reps": args.reps, "rounds": args.rounds, "table": []}
    per_view = {}
    for k in keys:
        NV, dt, agg = k
        v = rounds[k]
        ms = float(np.median(v))
        per_view[k] = ms / B / NV
        res["table"].append({"views": NV, "maps_dtype": dt, "aggregation": agg, "kernels": "register (NV <= 8)" if NV <= 8 else "many-view",
                             "ms_per_call": ms, "spread_ms": float(np.max(v) - np.min(v)), "ms_per_sample": ms / B, "ms_per_sample_view": ms / B / NV,
                             "workspace_bytes_per_sample": variants[k]["nws"] // B})
    for row in res["table"]:
        base = per_view.get((8, row["maps_dtype"], row["aggregation"]))
        if base:
            row["per_view_over_8_views"] = row["ms_per_sample_view"] / base
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
