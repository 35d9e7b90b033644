#!/usr/bin/env python
"""Shader-clock accounting of the halo kernels' per-tile phases (GPU, profiling build liblt_hip_trace.so).

    trace_halo.py [B] [--no-residual]        the 3^3 32 -> 32 layer at 64^3: column walk, or the persistent kernel under LT_HALO_NO_COL=1
    trace_halo.py [B] --k7 [--residual]      V2V's front layer, 7^3 32 -> 16 at 64^3 (affine + ReLU as in the model): column walk, or the
                                             one-tile kernel under LT_HALO_NO_COL7=1 (64 workgroups sampled across the launch, one tile each)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learnable-triangulation-pytorch_amd")
# LT_TRACE_DEFS="LT_ABL_NO_STORE": extra defines for an ablation of the traced kernel (results wrong by design, timing only)
EXTRA = os.environ.get("LT_TRACE_DEFS", "").split()
VARIANT = "trace" + "".join("_" + d.lower() for d in EXTRA)
os.environ["LT_HIP_LIB"] = os.path.join(PKG, "lib", "liblt_hip_%s.so" % VARIANT)
sys.path.insert(0, PKG)
if not os.path.exists(os.environ["LT_HIP_LIB"]):   # profiling build of the same sources (hipcc is on the GPU box too)
    import lt_build
    lt_build.build_variant(VARIANT, ["LT_TRACE"] + EXTRA)
import numpy as np
import torch

import lt_engine as E
import lt_hip as H

NAMES3 = ["total", "wait+barrier", "halo issue / tile setup", "res issue", "tap loop (+ deferred epilogue)", "barrier", "epilogue / bookkeeping"]
NAMES7 = ["total", "wait: halo / plane group landed", "tile setup (+ residual request)", "-", "tap nest (49 chunks)", "drain / seam barrier",
          "epilogue / bookkeeping"]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    k7 = "--k7" in sys.argv
    B = int(args[0]) if args else 16
    with_res = "--residual" in sys.argv if k7 else "--no-residual" not in sys.argv
    lib = H.lib()
    lib.lt_trace_read_halo.restype = C.c_int
    lib.lt_trace_read_halo.argtypes = [C.c_void_p, C.c_int]
    dev, dt = "cuda:0", torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    ks, cout = (7, 16) if k7 else (3, 32)
    x = torch.randn(B, 64, 64, 64, 32, device=dev).to(dt)
    w = torch.randn(cout, 32, ks, ks, ks) * 0.05
    res = E.Act(torch.randn(B, 64, 64, 64, cout, device=dev).to(dt)) if with_res else None
    bn = (torch.ones(cout), torch.zeros(cout), torch.zeros(cout), torch.ones(cout)) if k7 else None
    b = E.PlanBuilder(dev, dt)
    b.conv(E.Act(x), w, torch.zeros(cout) if k7 else None, bn, stride=1, pad=ks // 2, relu=True, residual=res)
    plan = b.finish()
    for _ in range(3):
        plan.run_eager(st)
    e0, e1 = H.Event(), H.Event()
    e0.record(st)
    plan.run_eager(st)
    e1.record(st)
    us = e0.elapsed_ms(e1) * 1e3
    buf = np.zeros(8 * 64, dtype=np.int64)
    lib.lt_trace_read_halo(buf.ctypes.data, buf.size)
    r = buf.reshape(-1, 8)
    r = r[r[:, 7] > 0]
    nt = r[:, 7].mean()
    if k7:
        kern, layer, names = "one-tile" if os.environ.get("LT_HALO_NO_COL7") else "column-walk", "7^3 32->16", NAMES7
    else:
        kern, layer, names = "persistent" if os.environ.get("LT_HALO_NO_COL") else "column-walk", "3^3 32->32", NAMES3
    print(kern + (" [" + " ".join(EXTRA) + "]" if EXTRA else "") + " %s @64^3 B=%d%s: %.0f us, %d workgroups sampled, %.1f tiles each"
          % (layer, B, " +residual" if with_res else "", us, len(r), nt))
    for k, nm in enumerate(names):
        if nm != "-":
            print("  %-32s %9.0f cycles/tile" % (nm, r[:, k].mean() / nt))
    if k7:
        tiles_per_cu = B * 16 * 8 * 8 / 256.0
        print("  launch time / tiles per CU       %9.2f us/tile  (256 CUs, %.0f tiles each: includes what the stamps cannot see)" % (us / tiles_per_cu, tiles_per_cu))


if __name__ == "__main__":
    main()
