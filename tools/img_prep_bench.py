"""Cost of the per-view image preparation: lt_crop_resize_u8 on the GPU against the CPU pieces of the reference dataset path.

    python tools/img_prep_bench.py [--views 256] [--iters 50] [--undistort]

256 views cut from 1000 x 1000 uint8 frames with square crops of 300..900 px (partly outside the frame allowed) into 384 x 384:
  * kernel time from device events after warm-up, and the algorithmic bytes (pixels of bbox & frame x 3 read + H*W*3*4 written per
    view) over that time as a fraction of the 6.3 TB/s achievable HBM bandwidth;
  * host ms / view of the CPU pieces present here: PIL crop, numpy float64 normalize_image, the float64 -> fp32 staging copy
    (cv2's resize is timed only when cv2 is importable; otherwise it is reported as not measured);
  * how many CPUs the CPU path would need at 5600 views / s (1400 samples / s x 4 views) from those numbers.
--undistort times lt_undistort_crop_resize_u8 (on-the-fly lens undistortion in front of the same crop / resize / normalise) on the
same views with H36M-like intrinsics and distortion (two cameras), next to lt_crop_resize_u8, the two launches alternated in one
loop; plus the host ms per view of the source-window computation and the host ms of building one camera's maps.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "learnable-triangulation-pytorch_amd")]
from mvn.utils import img  # noqa: E402

HBM = 6.3e12
RATE = 5600.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-views", type=int, default=16)
    ap.add_argument("--undistort", action="store_true", help="time lt_undistort_crop_resize_u8 next to lt_crop_resize_u8")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (1000, 1000, 3), dtype=np.uint8) for _ in range(8)]
    views, boxes = [], []
    for i in range(a.views):
        s = int(rng.integers(300, 901))
        l, u = int(rng.integers(-50, 1050 - s)), int(rng.integers(-50, 1050 - s))
        views.append(frames[i % len(frames)]); boxes.append((l, u, l + s, u + s))
    boxes = np.array(boxes, np.int64)
    H = W = 384
    inside = sum(max(0, min(r, 1000) - max(l, 0)) * max(0, min(lo, 1000) - max(u, 0)) for l, u, r, lo in boxes)
    algo_bytes = inside * 3 + a.views * H * W * 3 * 4
    res = {"views": a.views, "out": [H, W], "algorithmic_bytes": int(algo_bytes)}

    dev = torch.device("cuda:0")
    if a.undistort:
        print(json.dumps(undistort(a, views, boxes, res, dev, H, W)))
        return
    block, desc = img.pack_regions(views, boxes)
    src = torch.from_numpy(block).to(dev)
    dd = torch.from_numpy(desc).to(dev)
    out = torch.empty((a.views, 3, H, W), device=dev)
    lut = img.normalize_lut(dev)
    for _ in range(5):
        img.launch_crop_resize(src, dd, desc, (H, W), lut, out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); img.launch_crop_resize(src, dd, None, (H, W), lut, out); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    res.update(kernel_ms_median=ms, kernel_ms_min=float(np.min(ts)), kernel_us_per_view=1e3 * ms / a.views,
               achieved_TBps=algo_bytes / (ms * 1e-3) / 1e12, fraction_of_6p3TBps=algo_bytes / (ms * 1e-3) / HBM)

    n = min(a.cpu_views, a.views)
    t0 = time.perf_counter(); crops = [img.crop_image(views[i], tuple(int(x) for x in boxes[i])) for i in range(n)]
    crop_ms = (time.perf_counter() - t0) * 1e3 / n
    resized = [np.ascontiguousarray(c[:H, :W]) if c.shape[0] >= H and c.shape[1] >= W else np.zeros((H, W, 3), np.uint8) for c in crops]
    if img.cv2 is not None:
        t0 = time.perf_counter(); resized = [img.cv2.resize(c, (W, H), interpolation=img.cv2.INTER_AREA) for c in crops]
        res["cv2_resize_ms_per_view"] = (time.perf_counter() - t0) * 1e3 / n
    else:
        res["cv2_resize_ms_per_view"] = "not measured (cv2 not importable)"
    t0 = time.perf_counter(); normed = [img.normalize_image(r) for r in resized]
    norm_ms = (time.perf_counter() - t0) * 1e3 / n
    stage = torch.empty((n, H, W, 3), dtype=torch.float32)
    t0 = time.perf_counter(); stage.copy_(torch.from_numpy(np.stack(normed)))
    stage_ms = (time.perf_counter() - t0) * 1e3 / n
    host_ms = crop_ms + norm_ms + stage_ms + (res["cv2_resize_ms_per_view"] if img.cv2 is not None else 0.0)
    res.update(pil_crop_ms_per_view=crop_ms, normalize_f64_ms_per_view=norm_ms, stage_f64_to_f32_ms_per_view=stage_ms,
               host_ms_per_view_measured=host_ms, cpus_needed_at_5600_views_per_s=host_ms * 1e-3 * RATE,
               cpus_needed_note="from the measured pieces only" + ("" if img.cv2 is not None else ", cv2 resize excluded (lower bound)"))
    print(json.dumps(res))


def undistort(a, views, boxes, res, dev, H, W):
    cams = [(np.array([[1146.0, 0.0, 508.5], [0.0, 1145.0, 514.0], [0.0, 0.0, 1.0]], np.float32),
             np.array([-0.21, 0.25, -0.0011, -0.0016, -0.0042], np.float32)),
            (np.array([[1150.0, 0.0, 500.0], [0.0, 1148.5, 507.0], [0.0, 0.0, 1.0]], np.float32),
             np.array([-0.19, 0.21, 0.0012, 0.0009, -0.0021], np.float32))]
    t0 = time.perf_counter()
    maps = [img.undistort_maps(K, d, 1000, 1000) for K, d in cams]
    blocks = [img.device_map(m) for m in maps]
    mono = [img.map_is_monotone(m[0]) for m in maps]
    map_ms = (time.perf_counter() - t0) * 1e3 / len(cams)
    views_maps = [(maps[i % 2][0], mono[i % 2], (i % 2) * blocks[0].nbytes, 1000) for i in range(a.views)]
    t0 = time.perf_counter()
    desc_u, wins, total = img.undistort_descriptors(views, boxes, views_maps)
    win_ms = (time.perf_counter() - t0) * 1e3 / a.views
    ublock = np.empty(max(total, 1), np.uint8)
    for i, wn in enumerate(wins):
        if wn.size:
            ublock[desc_u[i, 0]:desc_u[i, 0] + wn.size].reshape(wn.shape)[...] = wn
    usrc, udesc = torch.from_numpy(ublock).to(dev), torch.from_numpy(desc_u).to(dev)
    dmaps = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks])).to(dev)
    block, desc = img.pack_regions(views, boxes)
    src, dd = torch.from_numpy(block).to(dev), torch.from_numpy(desc).to(dev)
    out_p = torch.empty((a.views, 3, H, W), device=dev)
    out_u = torch.empty((a.views, 3, H, W), device=dev)
    lut = img.normalize_lut(dev)
    img.launch_crop_resize(src, dd, desc, (H, W), lut, out_p)                           # host-side validation once
    img.launch_undistort_crop_resize(usrc, udesc, desc_u, dmaps, (H, W), lut, out_u)
    for _ in range(5):
        img.launch_crop_resize(src, dd, None, (H, W), lut, out_p)
        img.launch_undistort_crop_resize(usrc, udesc, None, dmaps, (H, W), lut, out_u)
    torch.cuda.synchronize()
    tp, tu = [], []
    for _ in range(a.iters):
        for fn, ts in ((lambda: img.launch_crop_resize(src, dd, None, (H, W), lut, out_p), tp),
                       (lambda: img.launch_undistort_crop_resize(usrc, udesc, None, dmaps, (H, W), lut, out_u), tu)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
    mp, mu = float(np.median(tp)), float(np.median(tu))
    res.update(mode="undistort", crop_resize_kernel_ms_median=mp, undistort_kernel_ms_median=mu, undistort_kernel_ms_min=float(np.min(tu)),
               undistort_us_per_view=1e3 * mu / a.views, ratio_undistort_to_crop_resize=mu / mp,
               undistort_views_per_s=a.views / (mu * 1e-3), headroom_at_5600_views_per_s=a.views / (mu * 1e-3) / RATE,
               window_bytes_shipped=int(total), host_source_window_ms_per_view=win_ms, host_build_map_ms_per_camera=map_ms,
               map_bytes_per_camera=int(blocks[0].nbytes))
    return res


if __name__ == "__main__":
    main()
