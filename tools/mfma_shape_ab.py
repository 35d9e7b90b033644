#!/usr/bin/env python
"""A/B of the bf16 MFMA shape (16x16x32 against 32x32x16) of conv2d_halo_kernel and conv3d_halo_col_kernel, per instantiation, in ONE process on one device:
the layer at the benchmark's shape, Gaussian inputs and weights (never zeros: on zeros both shapes run at the same clock and the ranking is the cycle ratio), the
two settings of the kernel's switch (LT_H2D_MF32, LT_HALO_COL_MF32) in interleaved rounds (read per launch call), median and min per setting; then each setting run back to back for
--seconds with the shader clock and socket power sampled (bench.ClockSampler).
    python tools/mfma_shape_ab.py [--rounds 9] [--seconds 3] [--out file.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "learnable-triangulation-pytorch_amd")):
    sys.path.insert(0, p)
import torch

import bench
import lt_engine as E
import lt_hip as H

CASES = [   # name, switch, instantiation (2D: tile rows, phases; 3D: kind), samples, spatial, channels, kernel, stride, pad, transposed, residual, LT_H2D_TH
    ("3^3 32->32 @64^3 x 64, residual (column walk)", "LT_HALO_COL_MF32", (0,), 64, (64, 64, 64), 32, 3, 1, 1, False, True, None),
    ("3x3 256->256 @24^2 x 256 (8-row tiles)", "LT_H2D_MF32", (8, 1), 256, (1, 24, 24), 256, 3, 1, 1, False, False, None),
    ("3x3 256->256 @24^2 x 256 (4-row tiles)", "LT_H2D_MF32", (4, 1), 256, (1, 24, 24), 256, 3, 1, 1, False, False, "4"),
    ("4x4 transposed 256->256 @48^2 x 256", "LT_H2D_MF32", (8, 4), 256, (1, 48, 48), 256, 4, 2, 1, True, False, None),
]


def bn(c, g):
    return (0.2 + 0.4 * torch.rand(c, generator=g), torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1, 0.5 + torch.rand(c, generator=g))


def set_switch(switch, on):
    if on:
        os.environ[switch] = "1"
    else:
        os.environ.pop(switch, None)


def shape_of(inst):
    return H.lib().lt_sel_halo_col_mfma(*inst) if len(inst) == 1 else H.lib().lt_sel_halo2d_mfma(*inst)


def timed(plan, st, n):
    e0, e1 = H.Event(), H.Event()
    e0.record(st)
    for _ in range(n):
        plan.run_eager(st)
    e1.record(st)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_ms(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    report = {"cases": []}
    for name, SWITCH, inst, N, sp, ch, k, stride, pad, transposed, has_res, th in CASES:
        if th is None:
            os.environ.pop("LT_H2D_TH", None)
        else:
            os.environ["LT_H2D_TH"] = th
        set_switch(SWITCH, False)
        default = shape_of(inst)
        nd = 2 if sp[0] == 1 else 3
        b = E.PlanBuilder(dev, torch.bfloat16)
        x = E.Act(torch.relu(torch.randn(N, *sp, ch, generator=g)).to(dev, torch.bfloat16))
        res = E.Act(torch.relu(torch.randn(N, *sp, ch, generator=g)).to(dev, torch.bfloat16)) if has_res else None
        w = torch.randn(ch, ch, *([k] * nd), generator=g) / (ch * (k / stride) ** nd) ** 0.5
        y = b.conv(x, w, None, bn(ch, g), stride=stride, pad=pad, transposed=transposed, relu=True, residual=res)
        assert nd == 3 or b.last_info["desc"].phase[0].weight_frag_layout == 2, "not the 2D halo kernel"
        plan = b.finish()
        outs = {}
        for on in (False, True):
            set_switch(SWITCH, on)
            for _ in range(3):
                plan.run_eager(st)
            torch.cuda.synchronize()
            outs[on] = y.t.clone()
        differ = float((outs[False].view(torch.int16) != outs[True].view(torch.int16)).float().mean())
        us = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                set_switch(SWITCH, on)
                us[on].append(timed(plan, st, 50))
        row = {"case": name, "switch": SWITCH, "default_shape": default, "share_of_outputs_that_differ": differ, "gflop": plan.flops / 1e9}
        for on in (False, True):
            set_switch(SWITCH, on)
            shape = shape_of(inst)
            smp = bench.ClockSampler(0)
            t0 = time.time()
            while time.time() - t0 < args.seconds:
                for _ in range(50):
                    plan.run_eager(st)
                torch.cuda.synchronize()
            t1 = time.time()
            held = timed(plan, st, 50)
            clk = smp.window(t0 + 0.4 * (t1 - t0), time.time()) or {}
            key = "switch_set" if on else "switch_unset"
            row[key] = {"mfma": shape, "median_us": statistics.median(us[on]), "min_us": min(us[on]), "rounds_us": [round(v, 2) for v in us[on]],
                                      "back_to_back_us": held, "sclk_mhz": clk.get("sclk_mhz"), "power_w": clk.get("power_w"), "clock_reads": clk.get("samples")}
            print("%-44s %s: median %.1f us, min %.1f us | back to back %.1f us at sclk %s MHz, %s W" % (
                name, "16x16x32" if shape == 16 else "32x32x16", row[key]["median_us"], row[key]["min_us"], held,
                clk.get("sclk_mhz"), clk.get("power_w")), flush=True)
        print("%-44s share of output words that differ between the shapes: %.4f" % (name, differ), flush=True)
        report["cases"].append(row)
        set_switch(SWITCH, False)
        del plan, b, x, y, res, outs
        torch.cuda.empty_cache()
    os.environ.pop("LT_H2D_TH", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
