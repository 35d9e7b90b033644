"""The algebraic model's tail (2D soft-argmax + confidences / DLT) with and without per-joint statistics, in one process; prints one JSON line and writes
profiles/alg_keypoint_stats_bench.json.

    python tools/alg_keypoint_stats_bench.py [--batch 8] [--views 4] [--joints 17] [--heatmap 96] [--reps 300] [--rounds 7] [--parent-lib PATH] [--out ...]

Shape: the algebraic model's production tail (8 samples x 4 views, 17 joints, 96 x 96 heatmaps, 384 px images, with the confidence head).  Variants,
interleaved round by round so that clock drift hits all of them:
  plain         lt_softargmax2d_fwd + lt_alg_tail_fwd                the tail as it is;
  stats         lt_softargmax2d_stats_fwd + lt_alg_tail_stats_fwd    the same two launches with the statistics;
  sa2 / sa2_stats, tail / tail_stats                                 each launch of the two pairs alone;
  parent_plain  (--parent-lib: a liblt_hip.so built from the parent commit) the plain pair of that build, loaded next to this one: the yardstick.
Timing: device events around --reps back-to-back calls (per call = elapsed / reps), after a warm-up of every variant; per variant the median of the --rounds
round values and the spread (max - min of the round values).  Before anything is timed the outputs the variants share are compared bit for bit."""
import argparse
import ctypes as C
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
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--heatmap", type=int, default=96)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alg_keypoint_stats_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "alg_keypoint_stats_bench needs a GPU"
    import lt_hip as H
    from oracle import synth
    B, NV, J, hw = args.batch, args.views, args.joints, args.heatmap
    N, img = B * NV, 4 * args.heatmap
    g = torch.Generator().manual_seed(11)
    # heatmaps with one bump each where a joint within 300 mm of the origin projects, so that the DLT has a sensible system
    K, R, t = synth.ring_cameras(NV, img)
    P = torch.from_numpy(K @ np.concatenate([R, t], -1))[None].repeat(B, 1, 1, 1).float().contiguous()
    X = torch.randn(B, J, 3, generator=g).double() * 150.0
    hh = torch.einsum("bvik,bjk->bvji", P.double(), torch.cat([X, torch.ones(B, J, 1, dtype=torch.float64)], -1))
    c = ((hh[..., :2] / hh[..., 2:3]) / 4.0).float().clamp(4.0, hw - 5.0)
    yy, xx = torch.meshgrid(torch.arange(hw, dtype=torch.float32), torch.arange(hw, dtype=torch.float32), indexing="ij")
    hm = (torch.exp(-((xx - c[..., 0, None, None]) ** 2 + (yy - c[..., 1, None, None]) ** 2) / 8.0) + 0.02 * torch.randn(B, NV, J, hw, hw, generator=g))
    hm = hm.reshape(N * J, hw, hw).to(DEV).contiguous()
    conf_raw = (torch.rand(B, NV, J, generator=g) + 0.2).to(DEV).contiguous()
    Pd = P.to(DEV)
    mult, scale = 100.0, float(np.float32(img / hw))
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    f = lambda *s: torch.empty(*s, device=DEV)
    buf = {n: {"kp_hm": f(N * J, 2), "probs": f(N * J, hw, hw), "kp2d": f(B, NV, J, 2), "conf": f(B, NV, J), "kp3d": f(B, J, 3)} for n in ("plain", "stats", "parent_plain")}
    rec, idx = f(N * J, 5), torch.empty(N * J, dtype=torch.int32, device=DEV)
    cov2d, err, cov3d = f(B, NV, J, 3), f(B, NV, J), f(B, J, 6)
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("lt_softargmax2d_fwd", "lt_alg_tail_fwd"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = H.SIGNATURES[name]

    def sa2(l, o):
        H.check(l.lt_softargmax2d_fwd(hm.data_ptr(), mult, 1, o["kp_hm"].data_ptr(), o["probs"].data_ptr(), N * J, hw, hw, st), "lt_softargmax2d_fwd")

    def tail(l, o):
        H.check(l.lt_alg_tail_fwd(o["kp_hm"].data_ptr(), conf_raw.data_ptr(), J, Pd.data_ptr(), scale, scale, o["kp2d"].data_ptr(), o["conf"].data_ptr(),
                                  o["kp3d"].data_ptr(), B, NV, J, st), "lt_alg_tail_fwd")

    def sa2_stats(o):
        H.check(lib.lt_softargmax2d_stats_fwd(hm.data_ptr(), mult, 1, o["kp_hm"].data_ptr(), o["probs"].data_ptr(), rec.data_ptr(), idx.data_ptr(), N * J, hw, hw, st),
                "lt_softargmax2d_stats_fwd")

    def tail_stats(o):
        H.check(lib.lt_alg_tail_stats_fwd(o["kp_hm"].data_ptr(), conf_raw.data_ptr(), J, Pd.data_ptr(), scale, scale, None, rec.data_ptr(), o["kp2d"].data_ptr(),
                                          o["conf"].data_ptr(), o["kp3d"].data_ptr(), cov2d.data_ptr(), err.data_ptr(), cov3d.data_ptr(), B, NV, J, st),
                "lt_alg_tail_stats_fwd")

    variants = {"plain": lambda: (sa2(lib, buf["plain"]), tail(lib, buf["plain"])), "stats": lambda: (sa2_stats(buf["stats"]), tail_stats(buf["stats"])),
                "sa2": lambda: sa2(lib, buf["plain"]), "sa2_stats": lambda: sa2_stats(buf["stats"]),
                "tail": lambda: tail(lib, buf["plain"]), "tail_stats": lambda: tail_stats(buf["stats"])}
    if parent is not None:
        variants["parent_plain"] = lambda: (sa2(parent, buf["parent_plain"]), tail(parent, buf["parent_plain"]))
    names = list(variants)

    def timed(name):
        e0, e1 = H.Event(), H.Event()
        e0.record(st)
        for _ in range(args.reps):
            variants[name]()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / args.reps

    for _ in range(3):
        for n in names:
            variants[n]()
    torch.cuda.synchronize()
    same = lambda a, b: all(bool(torch.equal(buf[a][k], buf[b][k])) for k in buf[a])
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            rounds[n].append(timed(n))
    res = {"shape": {"batch": B, "views": NV, "joints": J, "heatmap": hw, "image": img, "heatmap_multiplier": mult, "softmax": True, "confidences": True},
           "reps": args.reps, "rounds": args.rounds, "outputs_bit_identical_stats_vs_plain": same("plain", "stats"),
           "peak_is_the_largest_probability": bool(torch.equal(rec[:, 0], buf["stats"]["probs"].reshape(N * J, -1).max(dim=1).values)),
           "statistics_finite": bool(torch.isfinite(cov3d).all()) and bool(torch.isfinite(err).all()) and bool(torch.isfinite(cov2d).all()),
           "heatmap_bytes_read_and_written": 4 * N * J * hw * hw * 4}
    if parent is not None:
        res["outputs_bit_identical_parent_vs_plain"] = same("plain", "parent_plain")
    for n in names:
        v = rounds[n]
        res[n + "_ms"] = float(np.median(v))
        res[n + "_ms_min"] = float(np.min(v))
        res[n + "_spread_ms"] = float(np.max(v) - np.min(v))
    res["stats_minus_plain_ms"] = res["stats_ms"] - res["plain_ms"]
    res["stats_over_plain"] = res["stats_ms"] / res["plain_ms"]
    if parent is not None:
        res["plain_over_parent_plain"] = res["plain_ms"] / res["parent_plain_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
