"""RANSACTriangulationNet vs AlgebraicTriangulationNet forward time, the same two models as plan-level C ABI plans (lt_plan_create_alg /
lt_plan_forward_alg), and lt_triangulate_ransac alone; prints one JSON line.

    python tools/ransac_bench.py [--batch 8] [--views 4] [--size 384] [--layers 152] [--reps 20] [--dtypes fp32,bf16]

Forward: B x NV views of size^2, ResNet-<layers>, each compute dtype of --dtypes, synthetic weights; device events around each
forward after warm-up, median over reps.  Python forwards: the modules (keys algebraic_forward_ms, ransac_forward_ms for fp32, with a
_bf16 suffix for bf16); C plans: lt_plan_forward_alg with a captured graph, on the same stream (keys c_algebraic_plan_ms ...).  Kernel:
B = 100, NV = 4, J = 17 problems (ring cameras, joints projected and quantised to the 4-pixel grid of argmax x 4, one outlier view in
three), exhaustive pairs with the Huber refinement, device events."""
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

from oracle import spec, synth  # noqa: E402

DEV = "cuda:0"


def time_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


class CAlgPlan:
    """lt_plan_create_alg / lt_plan_forward_alg through ctypes, outputs in tensors allocated once."""

    def __init__(self, model, sd, layers, B, NV, size, dtype, conf):
        import ctypes as C
        import lt_hip as H
        self.C, self.H = C, H
        pc = H.AlgPlanConfig()
        pc.model, pc.dtype, pc.num_layers, pc.style_caffe, pc.num_joints = model, H.dtype_code(dtype), layers, 0, 17
        pc.B, pc.NV, pc.H, pc.W = B, NV, size, size
        pc.use_confidences, pc.heatmap_softmax, pc.heatmap_multiplier = int(conf), 1, 100.0
        pc.direct_optimization, pc.reprojection_error_epsilon, pc.use_graph = 1, 15.0, 1
        keep = [v.detach().float().contiguous() for v in sd.values()]
        arr = (H.NamedTensor * len(sd))()
        for i, (k, t) in enumerate(zip(sd.keys(), keep)):
            arr[i].name, arr[i].data, arr[i].ndim = k.encode(), t.data_ptr(), max(1, t.dim())
            for j, n in enumerate(t.shape if t.dim() else (1,)):
                arr[i].shape[j] = n
        self.plan = C.c_void_p()
        H.check(H.lib().lt_plan_create_alg(C.byref(pc), arr, len(sd), C.byref(self.plan)), "lt_plan_create_alg")
        info = H.PlanInfo()
        H.check(H.lib().lt_plan_info(self.plan, C.byref(info)), "lt_plan_info")
        h, w = info.heatmap_h, info.heatmap_w
        ransac = model == H.LT_MODEL_RANSAC
        self.kp3 = torch.empty(B, 17, 3, device=DEV)
        self.kp2 = torch.empty(B, NV, 17, 2, dtype=torch.int64 if ransac else torch.float32, device=DEV)
        self.hm = torch.empty(B, NV, 17, h, w, device=DEV)
        self.conf = torch.empty(B, NV, 17, device=DEV)

    def __call__(self, images, P):
        self.H.check(self.H.lib().lt_plan_forward_alg(self.plan, images.data_ptr(), P.data_ptr(), self.kp3.data_ptr(), self.kp2.data_ptr(), self.hm.data_ptr(),
                                                      self.conf.data_ptr(), torch.cuda.current_stream().cuda_stream), "lt_plan_forward_alg")

    def close(self):
        self.H.lib().lt_plan_destroy(self.plan)


def forward_times(args):
    from mvn.models.triangulation import AlgebraicTriangulationNet, RANSACTriangulationNet
    import lt_hip as H
    inp = synth.make_inputs(args.batch, args.views, args.size, seed=3)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(args.batch, 1, 1, 1).to(DEV).contiguous()
    images = inp["images"].to(DEV).contiguous()
    out = {}
    alg_cfg = synth.alg_config(args.layers, True)
    rcfg = synth.alg_config(args.layers, False)
    rcfg.model.name = "ransac"
    rcfg.model.direct_optimization = True
    for dt_name in args.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt_name]
        sfx = "" if dt_name == "fp32" else "_" + dt_name
        for name, cls, cfg, conf, model in (("algebraic", AlgebraicTriangulationNet, alg_cfg, True, H.LT_MODEL_ALG),
                                            ("ransac", RANSACTriangulationNet, rcfg, False, H.LT_MODEL_RANSAC)):
            sd = synth.make_state_dict(spec.alg_net_spec(args.layers, 17, conf), seed=5, basic_block=args.layers < 50)
            m = cls(cfg, device=DEV)
            m.load_state_dict(sd, strict=True)
            m.eval()
            m.compute_dtype = dtype
            with torch.no_grad():
                med, mn = time_ms(lambda: m(images, P, {}), args.reps)
            out[name + "_forward_ms" + sfx] = med
            out[name + "_forward_ms_min" + sfx] = mn
            del m
            torch.cuda.empty_cache()
            cp = CAlgPlan(model, sd, args.layers, args.batch, args.views, args.size, dtype, conf)
            med, mn = time_ms(lambda: cp(images, P), args.reps)
            out["c_" + name + "_plan_ms" + sfx] = med
            out["c_" + name + "_plan_ms_min" + sfx] = mn
            cp.close()
            del cp, sd
            torch.cuda.empty_cache()
        out["ransac_over_algebraic" + sfx] = out["ransac_forward_ms" + sfx] / out["algebraic_forward_ms" + sfx]
    return out


def kernel_time(reps):
    from mvn.utils import multiview
    B, NV, J = 100, 4, 17
    K, R, t = synth.ring_cameras(NV, 384)
    Pm = (K @ np.concatenate([R, t], -1)).astype(np.float32)
    rs = np.random.RandomState(0)
    X = rs.uniform(-1000, 1000, (B, J, 3))
    q = np.einsum("vrk,bjk->bvjr", Pm.astype(np.float64), np.concatenate([X, np.ones((B, J, 1))], -1))
    pts = (np.round(q[..., :2] / q[..., 2:] / 4) * 4).astype(np.int64)
    out_v = rs.randint(0, NV, (B, J))
    bad = rs.rand(B, J) < 1 / 3
    for b, j in zip(*np.nonzero(bad)):
        pts[b, out_v[b, j], j] = rs.randint(0, 96, 2) * 4
    P = torch.from_numpy(Pm)[None].repeat(B, 1, 1, 1).to(DEV)
    pt = torch.from_numpy(pts).to(DEV)
    med, mn = time_ms(lambda: multiview.triangulate_ransac_batch(P, pt, None, 15, True), reps)
    return {"ransac_kernel_ms_B100_NV4_J17": med, "ransac_kernel_ms_min": mn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtypes", default="fp32,bf16", help="compute dtypes of the forwards, comma-separated (fp32, bf16)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ransac_bench needs a GPU"
    res = {"shape": [args.batch, args.views, args.size, args.size], "layers": args.layers, "dtypes": args.dtypes.split(",")}
    res.update(kernel_time(max(args.reps, 50)))
    res.update(forward_times(args))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
