"""Training with several cuboids per frame (``multi_cuboid_training``, batch["cuboid_frame"]) against what a user does without it -- the training step on
the frames repeated once per cuboid -- in one process; prints one JSON line and writes profiles/multi_cuboid_train_bench.json.

    python tools/multi_cuboid_train_bench.py [--frames 8] [--per-frame 4] [--views 4] [--size 384] [--volume 64] [--layers 152] [--precision act16]
                                             [--reps 3] [--rounds 5] [--launches 10] [--skip-step]

Shape: BASELINE config 2 (ResNet-152 backbone, 4 views of 384^2, 64^3 voxels), bf16 activations (train_precision act16), synthetic weights; F = 8 frames
with 4 cuboids each, P = 32, as tools/multi_cuboid_bench.py.
  ``kernel``  lt_unproject_indexed_bwd alone (F frames, P cuboids, bf16 maps, 32 channels, view softmax) next to lt_unproject_bwd on the features gathered
              by frame_of (P samples): hipEvents around --launches launches of each, alternating, --rounds rounds; per entry the median of the rounds, per
              launch, and the spread (max - min of the rounds).  Both get their whole workspace.  The indexed entry writes F maps' gradients, the unindexed
              one P maps' (which autograd would still have to add up per frame; that addition is not in its time).
  ``step``    one model, two recorded plans: (a) multi: forward + loss + backward on the F frames with cuboid_frame; (b) repeated: the same on the P repeated
              samples.  Host wall clock from the call to the completion of the last kernel (torch.cuda.synchronize on both sides), --reps steps per round
              per route, alternating in --rounds rounds; per route the median of the round medians and the spread.  The claim this project accepts: (b) - (a)
              above 3 x the repeated route's spread (``saved_over_repeated_spread`` > 3)."""
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

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "multi_cuboid_train_bench.json")


def stat(xs):
    return {"ms": float(np.median(xs)), "ms_min": float(np.min(xs)), "spread_ms": float(np.max(xs) - np.min(xs)), "rounds": [float(x) for x in xs]}


def kernel_times(F, n, NV, h, w, V, rounds, launches, frame_of):
    """lt_unproject_indexed_bwd against lt_unproject_bwd on gathered features, bf16 maps / 32 channels / view softmax."""
    import lt_hip as H
    from oracle import vol_oracle as O
    lib = H.lib()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(F, NV, h, w, 32, generator=g).to(DEV, torch.bfloat16)
    K, R, t = synth.ring_cameras(NV, 4 * h)
    proj = torch.from_numpy(O.resized_projection(K, R, t, (4 * h, 4 * w), (h, w))).float()[None].repeat(F, 1, 1, 1).to(DEV).contiguous()
    ax = torch.linspace(-1250.0, 1250.0, V)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    coords = (grid[None] + (torch.randn(n, 3, generator=g) * 200)[:, None, None, None, :]).to(DEV).contiguous()
    gout = torch.randn(n, V, V, V, 32, generator=g).to(DEV)
    fof = torch.tensor(frame_of, dtype=torch.int32, device=DEV)
    idx = fof.long()
    gfeats_in, gproj = feats[idx].contiguous(), proj[idx].contiguous()
    out_f = torch.empty(F, NV, h, w, 32, device=DEV)
    out_p = torch.empty(n, NV, h, w, 32, device=DEV)
    nws_i, nws_u = lib.lt_unproject_indexed_bwd_workspace(n, NV, 32, V, V, V), lib.lt_unproject_bwd_workspace(n, NV, 32, V, V, V)
    ws = torch.empty(max(nws_i, nws_u), dtype=torch.uint8, device=DEV)
    st = H.cur_stream()
    agg = H.AGG["softmax"]
    indexed = lambda: H.check(lib.lt_unproject_indexed_bwd(H.LT_BF16, feats.data_ptr(), proj.data_ptr(), coords.data_ptr(), None, None, fof.data_ptr(), gout.data_ptr(),
                                                           out_f.data_ptr(), None, F, n, NV, 32, h, w, V, V, V, agg, ws.data_ptr(), nws_i, st), "lt_unproject_indexed_bwd")
    plain = lambda: H.check(lib.lt_unproject_bwd(H.LT_BF16, gfeats_in.data_ptr(), gproj.data_ptr(), coords.data_ptr(), None, gout.data_ptr(), out_p.data_ptr(), None,
                                                 n, NV, 32, h, w, V, V, V, agg, ws.data_ptr(), nws_u, st), "lt_unproject_bwd")

    def timed(fn):
        e0, e1 = H.Event(), H.Event()
        fn()
        e0.record(st)
        for _ in range(launches):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / launches
    for _ in range(2):
        indexed(), plain()
    torch.cuda.synchronize()
    # the two entries on the same data: the indexed result against the unindexed one added up per frame (fp32 addition order differs: a tolerance, not bits)
    summed = torch.zeros_like(out_f).index_add_(0, idx, out_p)
    diff = float((out_f - summed).abs().max() / summed.abs().max())
    res = {"indexed": [], "gathered_unindexed": []}
    for _ in range(rounds):
        res["indexed"].append(timed(indexed))
        res["gathered_unindexed"].append(timed(plain))
    r = {k: stat(v) for k, v in res.items()}
    r["indexed_over_unindexed"] = r["indexed"]["ms"] / r["gathered_unindexed"]["ms"]
    r["max_rel_diff_vs_summed_unindexed"] = diff
    r["workspace_bytes"] = {"indexed": int(nws_i), "gathered_unindexed": int(nws_u)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--per-frame", type=int, default=4)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--precision", default="act16", choices=["fp32", "bf16", "act16", "fp8v2v"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true", help="the kernel comparison alone")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_cuboid_train_bench needs a GPU"
    from mvn.models import loss as L
    from mvn.models.triangulation import VolumetricTriangulationNet
    from mvn.utils.multiview import Camera
    F, NV, nl = args.frames, args.views, args.layers
    n = F * args.per_frame
    frame_of = np.repeat(np.arange(F), args.per_frame).astype(np.int32)
    res = {"frames": F, "cuboids": n, "shape": [F, NV, args.size, args.size], "volume": args.volume, "layers": nl, "precision": args.precision, "reps": args.reps,
           "rounds": args.rounds, "launches": args.launches}
    h = args.size // 4
    res["kernel"] = kernel_times(F, n, NV, h, h, args.volume, args.rounds, args.launches, frame_of.tolist())
    torch.cuda.empty_cache()

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    write()          # the kernel figures are kept even if the two recorded plans of the step do not fit the device's memory
    if not args.skip_step:
        sd = synth.make_state_dict(spec.vol_net_spec(nl, 17, False), seed=62, basic_block=nl < 50)
        m = VolumetricTriangulationNet(synth.vol_config(nl, args.volume, "softmax"), device=DEV)
        m.load_state_dict(sd, strict=True)
        m.to(DEV)
        m.train()
        m.train_precision = args.precision
        m.multi_cuboid_training = True
        inp = synth.make_inputs(F, NV, args.size, seed=13)
        images = inp["images"].to(DEV).contiguous()
        images_rep = images[torch.from_numpy(frame_of).long().to(DEV)].contiguous()          # the repeated route's input, gathered once outside the timing
        kp = np.random.RandomState(3).randn(n, 17, 3) * 150.0
        gt = torch.as_tensor(kp)[:, :, :3].float().to(DEV)
        val = torch.ones(n, 17, 1, device=DEV)
        cams = lambda nb: [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(nb)] for v in range(NV)]
        cams_f, cams_p = cams(F), cams(n)

        def step(x, batch):
            out = m(x, None, batch)
            loss = L.KeypointsMAELoss()(out[0] * 0.1, gt * 0.1, val) + 0.01 * L.VolumetricCELoss()(out[5], out[2], gt, val)
            for p in m.parameters():
                p.grad = None
            loss.backward()

        multi = lambda: step(images, {"cameras": cams_f, "pred_keypoints_3d": kp, "cuboid_frame": frame_of})
        repeated = lambda: step(images_rep, {"cameras": cams_p, "pred_keypoints_3d": kp})

        def wall_ms(fn):
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))
        for _ in range(2):          # the first step of each route records its tape
            multi(), repeated()
        torch.cuda.synchronize()
        med = {"multi": [], "repeated": []}
        for _ in range(args.rounds):
            med["multi"].append(wall_ms(multi))
            med["repeated"].append(wall_ms(repeated))
        res["step"] = {k: stat(v) for k, v in med.items()}
        res["step"]["speedup_vs_repeated"] = res["step"]["repeated"]["ms"] / res["step"]["multi"]["ms"]
        res["step"]["saved_ms"] = res["step"]["repeated"]["ms"] - res["step"]["multi"]["ms"]
        res["step"]["saved_over_repeated_spread"] = res["step"]["saved_ms"] / max(res["step"]["repeated"]["spread_ms"], 1e-9)
        res["step"]["claim_met"] = bool(res["step"]["saved_over_repeated_spread"] > 3.0)
        res["step"]["peak_memory_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
