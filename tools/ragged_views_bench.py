"""The ragged forward (batch["view_counts"]) against the padded forward (batch["view_mask"]) on the same samples, in one process; prints one JSON line and
writes profiles/ragged_views_bench.json.

    python tools/ragged_views_bench.py [--layers 152] [--size 384] [--volume 64] [--steps 10] [--rounds 5] [--out profiles/ragged_views_bench.json]

Shape: BASELINE config 2 (ResNet-152, 384^2 images, 64^3 voxels), bf16, 8 samples, VolumetricTriangulationNet with view softmax.  Two count sets:
  small_gaps  4,4,4,3,4,2,4,3   T = 28 images against 8 x 4 = 32 padded;
  mixed_rigs  8,8,4,4,4,4,4,4   T = 40 images against 8 x 8 = 64 padded.
Per set two routes over the same samples: ``ragged`` (mvn.datasets.utils.ragged_batch of the padded batch) and ``padded`` (the view_mask forward).  Both plans
are warmed up (recorded and captured), their joints compared at the timed size, then timed alternately in interleaved rounds: the host clock around --steps
forwards that end in a synchronise, per forward = elapsed / steps.  Per route: the median of the round values and their spread (max - min).
``gather``: the ragged quad gather with every count equal to NVcap against the masked quad gather with an all-ones mask at config 2's gather shape (device
events around --gather-reps launches), the same interleaving.  No GPU: the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "learnable-triangulation-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import spec, synth  # noqa: E402
from oracle import vol_oracle as O  # noqa: E402

DEV = "cuda:0"
SETS = {"small_gaps": [4, 4, 4, 3, 4, 2, 4, 3], "mixed_rigs": [8, 8, 4, 4, 4, 4, 4, 4]}


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "spread_ms": float(np.max(v) - np.min(v)), "rounds_ms": [float(x) for x in v]}


def forward_set(name, counts, vol, args):
    from mvn.datasets.utils import ragged_batch
    from mvn.utils.multiview import Camera
    B, NV = len(counts), max(counts)
    inp = synth.make_inputs(B, NV, args.size, seed=13)
    mask = np.array([[1] * n + [0] * (NV - n) for n in counts], dtype=np.uint8)
    cams = [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(B)] for v in range(NV)]
    padded_batch = {"cameras": cams, "pred_keypoints_3d": inp["pred_keypoints_3d"], "view_mask": mask}
    images = inp["images"].to(DEV)
    images_r, _, ragged = ragged_batch(images, None, padded_batch)
    images_r = images_r.contiguous()
    routes = {"ragged": lambda: vol(images_r, None, ragged), "padded": lambda: vol(images, None, padded_batch)}
    outs = {}
    for _ in range(2):          # records and captures both plans, then one replay each
        for r, f in routes.items():
            outs[r] = f()[0]
    torch.cuda.synchronize()
    diff = float((outs["ragged"] - outs["padded"]).abs().max())
    assert bool(torch.isfinite(outs["ragged"]).all()) and bool(torch.isfinite(outs["padded"]).all()), name

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    rounds = {r: [] for r in routes}
    for _ in range(args.rounds):
        for r, f in routes.items():
            rounds[r].append(timed(f))
    res = {"counts": counts, "images_ragged": int(sum(counts)), "images_padded": B * NV, "NVcap": 4 if NV <= 4 else 8,
           "joints_max_abs_diff_ragged_vs_padded_mm": diff, "ragged": stats(rounds["ragged"]), "padded": stats(rounds["padded"])}
    res["saved_ms"] = res["padded"]["median_ms"] - res["ragged"]["median_ms"]
    res["ragged_faster_by_more_than_padded_spread"] = bool(res["saved_ms"] > res["padded"]["spread_ms"])
    res["time_ratio"] = res["ragged"]["median_ms"] / res["padded"]["median_ms"]
    res["image_ratio"] = sum(counts) / float(B * NV)
    return res


def gather(args):
    import lt_hip as H
    lib = H.lib()
    res = {}
    for NV in (4, 8):
        B, hw, V, Cc = 8, args.size // 4, args.volume, 32
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
        outs = {k: torch.empty(B, V, V, V, Cc, dtype=torch.bfloat16, device=DEV) for k in ("masked_ones", "ragged_full")}
        ones = torch.ones(B, NV, dtype=torch.uint8, device=DEV)
        vb = (torch.arange(B + 1, dtype=torch.int32) * NV).to(DEV)
        st = torch.cuda.current_stream().cuda_stream
        agg = H.AGG["softmax"]

        def launch(name):
            o = outs[name]
            if name == "masked_ones":
                H.check(lib.lt_unproject_grid_masked_fwd(H.LT_BF16, feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                                         coords.data_ptr(), None, ones.data_ptr(), o.data_ptr(), B, NV, Cc, hw, hw, V, agg, st),
                        "lt_unproject_grid_masked_fwd")
            else:
                H.check(lib.lt_unproject_grid_ragged_fwd(H.LT_BF16, feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                                         coords.data_ptr(), None, vb.data_ptr(), o.data_ptr(), B, B * NV, NV, Cc, hw, hw, V, agg, st),
                        "lt_unproject_grid_ragged_fwd")

        def timed(name):
            e0, e1 = H.Event(), H.Event()
            e0.record(st)
            for _ in range(args.gather_reps):
                launch(name)
            e1.record(st)
            torch.cuda.synchronize()
            return e0.elapsed_ms(e1) / args.gather_reps

        for _ in range(3):
            for n in outs:
                launch(n)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["masked_ones"], outs["ragged_full"]))
        rounds = {n: [] for n in outs}
        for _ in range(args.rounds):
            for n in outs:
                rounds[n].append(timed(n))
        r = {"shape": {"batch": B, "views": NV, "maps": [hw, hw, Cc], "volume": V, "dtype": "bf16"}, "reps": args.gather_reps,
             "ragged_full_bit_identical_to_masked_ones": same, "masked_ones": stats(rounds["masked_ones"]), "ragged_full": stats(rounds["ragged_full"])}
        r["ragged_minus_masked_ms"] = r["ragged_full"]["median_ms"] - r["masked_ones"]["median_ms"]
        r["within_masked_spread"] = bool(abs(r["ragged_minus_masked_ms"]) <= r["masked_ones"]["spread_ms"])
        res["NVcap%d" % NV] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gather-reps", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_views_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_views_bench needs a GPU"
    from mvn.models.triangulation import VolumetricTriangulationNet
    nl = args.layers
    sd = synth.make_state_dict(spec.vol_net_spec(nl, 17, False), seed=62, basic_block=nl < 50)
    vol = VolumetricTriangulationNet(synth.vol_config(nl, args.volume, "softmax"), device=DEV)
    vol.load_state_dict(sd, strict=True)
    vol.eval()
    vol.compute_dtype = torch.bfloat16
    res = {"shape": {"layers": nl, "size": args.size, "volume": args.volume, "dtype": "bf16", "samples": 8}, "steps": args.steps, "rounds": args.rounds,
           "clock": "host perf_counter around `steps` forwards ending in a synchronise; gather: device events around `reps` launches"}
    with torch.no_grad():
        for name, counts in SETS.items():
            res[name] = forward_set(name, counts, vol, args)
        res["gather"] = gather(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
