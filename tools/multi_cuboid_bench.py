"""Several cuboids per frame (batch["cuboid_frame"]) against what a user does without it -- the plain forward on the frames repeated once per cuboid --
in one process; prints one JSON line.

    python tools/multi_cuboid_bench.py [--frames 8] [--per-frame 4] [--views 4] [--size 384] [--volume 64] [--layers 152] [--dtype bf16] [--reps 10] [--rounds 5]

Shape: BASELINE config 2 (ResNet-152 backbone, 4 views of 384^2, 64^3 voxels), bf16, synthetic weights; F = 8 frames with 4 cuboids each, P = 32.
  (a) multi     VolumetricTriangulationNet.forward with batch["cuboid_frame"]: the backbone on the F frames, the gather, V2V and the soft-argmax on P cuboids;
  (b) repeated  the plain forward on images[cuboid_frame]: P samples, the backbone P / F times too often.
(a) is measured under both workgroup mappings of the indexed gather (LT_UNPROJ_PIN=cuboid | frame, csrc/unproject.hip).  The switch is read when a launch
is enqueued, i.e. when the plan's graph is captured: each mapping gets a model of its own (same weights), captured under its setting.
Timing: host wall clock from the call to the completion of its last kernel (torch.cuda.synchronize on both sides).  --rounds rounds, each --reps forwards
of every route, interleaved so that clock drift hits all; per route the median of the round medians, and the spread (max - min of the round medians).
``gather``: lt_unproject_grid_indexed_fwd alone at the same shape (hipEvents around 20 launches, median of --rounds such batches, per launch), per mapping,
for the balanced assignment (4 cuboids on every frame) and an unbalanced one (11, 7, 5, 3, 2, 2, 1, 1 cuboids per frame), next to lt_unproject_grid_fwd on
P gathered samples.  The forward is 40 x the gather, so the mapping is chosen on the gather's own time."""
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
PINS = ("cuboid", "frame")


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def stat(xs):
    return {"ms": float(np.median(xs)), "ms_min": float(np.min(xs)), "spread_ms": float(np.max(xs) - np.min(xs))}


def gather_times(F, n, NV, h, w, V, rounds, frame_of, launches=20):
    """The gather alone, bf16 / 32 channels / softmax (the fused kernel): {mapping: stats} and the unindexed entry on gathered inputs."""
    import lt_hip as H
    lib = H.lib()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(F, NV, h, w, 32, generator=g).to(DEV, torch.bfloat16)
    K, R, t = synth.ring_cameras(NV, 4 * h)
    from oracle import vol_oracle as O
    proj = torch.from_numpy(O.resized_projection(K, R, t, (4 * h, 4 * w), (h, w))).float()[None].repeat(F, 1, 1, 1).to(DEV).contiguous()
    base = (torch.randn(n, 3, generator=g) * 200).numpy().astype(np.float64)
    pos = torch.from_numpy((base - 1250.0).astype(np.float32)).to(DEV)
    cen = torch.from_numpy(base.astype(np.float32)).to(DEV)
    rot = torch.eye(3).reshape(1, 9).repeat(n, 1).to(DEV).contiguous()
    step = float(np.float32(2500.0 / (V - 1)))
    fof = torch.tensor(frame_of, dtype=torch.int32, device=DEV)
    idx = fof.long()
    gf, gp = feats[idx].contiguous(), proj[idx].contiguous()
    out = torch.empty(n, V, V, V, 32, dtype=torch.bfloat16, device=DEV)
    coords = torch.empty(n, V, V, V, 3, device=DEV)
    st = H.cur_stream()
    indexed = lambda: H.check(lib.lt_unproject_grid_indexed_fwd(H.LT_BF16, feats.data_ptr(), proj.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                                                coords.data_ptr(), None, None, fof.data_ptr(), out.data_ptr(), F, n, NV, 32, h, w, V, H.AGG["softmax"], st),
                              "lt_unproject_grid_indexed_fwd")
    plain = lambda: H.check(lib.lt_unproject_grid_fwd(H.LT_BF16, gf.data_ptr(), gp.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0, coords.data_ptr(), None,
                                                      out.data_ptr(), n, NV, 32, h, w, V, H.AGG["softmax"], st), "lt_unproject_grid_fwd")

    def timed(fn):
        e0, e1 = H.Event(), H.Event()
        for _ in range(3):
            fn()
        e0.record(st)
        for _ in range(launches):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / launches
    res = {k: [] for k in PINS + ("repeated",)}
    bits = {}
    for _ in range(rounds):
        for pin in PINS:
            os.environ["LT_UNPROJ_PIN"] = pin
            res[pin].append(timed(indexed))
            bits[pin] = out.clone()
        res["repeated"].append(timed(plain))
        bits["repeated"] = out.clone()
    os.environ.pop("LT_UNPROJ_PIN", None)
    r = {k: stat(v) for k, v in res.items()}
    r["bit_identical"] = bool(torch.equal(bits["cuboid"], bits["frame"]) and torch.equal(bits["cuboid"], bits["repeated"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--per-frame", type=int, default=4)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_cuboid_bench needs a GPU"
    from mvn.models.triangulation import VolumetricTriangulationNet
    from mvn.utils.multiview import Camera
    F, NV, nl = args.frames, args.views, args.layers
    n = F * args.per_frame
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[args.dtype]
    sd = synth.make_state_dict(spec.vol_net_spec(nl, 17, False), seed=62, basic_block=nl < 50)

    def model():
        vol = VolumetricTriangulationNet(synth.vol_config(nl, args.volume, "softmax"), device=DEV)
        vol.load_state_dict(sd, strict=True)
        vol.eval()
        vol.compute_dtype = dtype
        return vol
    nets = {"repeated": model(), "cuboid": model(), "frame": model()}
    inp = synth.make_inputs(F, NV, args.size, seed=13)
    images = inp["images"].to(DEV).contiguous()
    frame_of = np.repeat(np.arange(F), args.per_frame).astype(np.int32)
    kp = np.random.RandomState(3).randn(n, 17, 3) * 150.0
    cams = lambda nb: [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(nb)] for v in range(NV)]
    cams_f, cams_p = cams(F), cams(n)
    images_rep = images[torch.from_numpy(frame_of).long().to(DEV)].contiguous()          # the repeated route's input, gathered once outside the timing

    def multi(pin):
        os.environ["LT_UNPROJ_PIN"] = pin          # read at capture (the first forward) and by eager launches
        return nets[pin](images, None, {"cameras": cams_f, "pred_keypoints_3d": kp, "cuboid_frame": frame_of})

    def repeated():
        return nets["repeated"](images_rep, None, {"cameras": cams_p, "pred_keypoints_3d": kp})

    with torch.no_grad():
        outs = {pin: multi(pin) for pin in PINS}          # records and captures each plan under its mapping
        ref = repeated()
        torch.cuda.synchronize()
        # the two mappings must agree bit for bit.  Against the repeated route bit identity is NOT promised at this shape: its backbone runs on P * NV images,
        # ours on F * NV, and the plan picks batch-dependent kernels (split-K, tiles) -- the features then differ in the last bf16 bit before any cuboid is
        # involved; the coordinates and base points, which no backbone touches, must be equal
        pins_same = all(torch.equal(outs["cuboid"][i], outs["frame"][i]) for i in (0, 1, 2, 5, 6))
        first = [int(np.argmax(frame_of == f)) for f in range(F)]
        feats_same = bool(torch.equal(outs["cuboid"][1], ref[1][first]))
        geometry_same = bool(torch.equal(outs["cuboid"][5], ref[5]) and torch.equal(outs["cuboid"][6], ref[6]))
        kp_diff = float((outs["cuboid"][0].double() - ref[0].double()).abs().max())
        feat_diff = float((outs["cuboid"][1].double() - ref[1][first].double()).abs().max() / ref[1].double().abs().max())
        for _ in range(3):
            multi("cuboid"), multi("frame"), repeated()
        med = {k: [] for k in PINS + ("repeated",)}
        for _ in range(args.rounds):
            for pin in PINS:
                med[pin].append(wall_ms(lambda: multi(pin), args.reps))
            med["repeated"].append(wall_ms(repeated, args.reps))
        os.environ.pop("LT_UNPROJ_PIN", None)
        h = outs["cuboid"][1].shape[3]
        gather = {}
        if dtype == torch.bfloat16 and NV in (4, 8) and args.volume % 16 == 0:
            uneven = np.repeat(np.arange(8), [11, 7, 5, 3, 2, 2, 1, 1]).astype(np.int32)
            gather["balanced"] = gather_times(F, n, NV, h, h, args.volume, args.rounds, frame_of.tolist())
            if F == 8 and n == 32:
                gather["unbalanced_11_7_5_3_2_2_1_1"] = gather_times(F, n, NV, h, h, args.volume, args.rounds, uneven.tolist())
    res = {"frames": F, "cuboids": n, "shape": [F, NV, args.size, args.size], "volume": args.volume, "layers": nl, "dtype": args.dtype, "reps": args.reps,
           "rounds": args.rounds, "multi_pin_cuboid": stat(med["cuboid"]), "multi_pin_frame": stat(med["frame"]), "repeated": stat(med["repeated"]),
           "mappings_bit_identical": bool(pins_same), "coords_and_base_points_equal_repeated": geometry_same, "features_equal_repeated": feats_same,
           "features_max_rel_diff_vs_repeated": feat_diff, "joints_max_abs_diff_vs_repeated_mm": kp_diff, "gather": gather}
    best = min(PINS, key=lambda p: med_of(res, p))
    res["multi_ms"] = med_of(res, best)
    res["speedup_vs_repeated"] = res["repeated"]["ms"] / res["multi_ms"]
    res["saved_ms"] = res["repeated"]["ms"] - res["multi_ms"]
    res["saved_over_repeated_spread"] = res["saved_ms"] / max(res["repeated"]["spread_ms"], 1e-9)
    print(json.dumps(res))


def med_of(res, pin):
    return res["multi_pin_" + pin]["ms"]


if __name__ == "__main__":
    main()
