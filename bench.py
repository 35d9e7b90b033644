#!/usr/bin/env python
"""Headline benchmark: multi-view samples/sec of the volumetric-softmax forward path
(BASELINE.json config 2: 4 views 384x384, 64^3 voxel cube, ResNet-152 backbone) on N MI355X.

    python bench.py --gpus N --steps K --warmup W

N > 1: either launched by ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`` (the driver's way: the
ranks find RANK / LOCAL_RANK / WORLD_SIZE in the environment), or started plainly -- bench.py then runs ITSELF in a child process under
torch.distributed.run (127.0.0.1, a free port), one process per GPU, backend "nccl" (= RCCL over xGMI).

A "step" = one forward of B samples per GPU (B x NV views -> B skeletons) on synthetic inputs already resident in HBM,
through the reference-shaped module API (VolumetricTriangulationNet.forward) whose arithmetic is liblt_hip.so.  Samples are
independent units, so ranks shard the batch with NO data-path collective (weak scaling); the only communication is the
barrier + MAX-reduce of the timing (on device tensors).  Rank 0 prints ONE JSON line.

A plain run measures the headline alone: it sets up, warms up, times the K steps, writes the outputs if ``--dump-outputs`` is given
and prints the line.  Everything else below -- the CPU baseline and parity, the per-kernel roofline with its PMC passes and the shader
clock, the fp32 parity-mode leg, the batch sweep, the config-4 and training child legs -- runs only with ``--full``.

With ``--full`` the line also carries
  roofline      the dominant kernel family (convolutions on MFMA): algorithmic FLOP per step (2*MAC of every conv launch) /
                summed launch durations, measured with hipEvent pairs around every launch on the launch stream (eager pass
                after the timed region); ``traffic`` = HBM bytes per step of the same launches from the committed rocprofv3
                PMC passes of this command (``traffic_source`` says which file; it is NOT re-measured in the run);
  roofline_hbm  the same for the HBM-bound kernels (unprojection gather, 3D soft-argmax), algorithmic bytes from SURVEY.md 8(d);
  parity        joints of the TIMED kernel set (samples 0 and 1 of the timed batch) against the CPU oracle on the same weights
                and inputs: max relative error (1 mm floor) and MPJPE; weights are the sharpened set of SURVEY.md 8(d)
                (V2V output layer scaled to logit std ~5) so that the 3D soft-argmax is input-sensitive;
  fp32_parity_mode  the same workload on the exact-fp32 kernel set (the mode that meets the 1e-4 gate): samples/s, roofline
                fraction against the fp32 MFMA peak, and its parity figures;
  batch_sweep   samples/s at the reference's own batch sizes (5 = train, 10 = val; human36m_vol_softmax.yaml:17-18) and B = 1;
  cpu_baseline  the CPU oracle (torch-CPU restatement of the reference path, same ATen ops, same weights) timed on this
                box's host cores on a bounded sample BEFORE the GPU timing (rank 0, N = 1 only).

``--dump-outputs DIR`` also writes the arrays the last timed step returned (rank 0) as DIR/<name>.npy (dump_outputs); inputs and weights
are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import re
import shutil
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "learnable-triangulation-pytorch_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}   # dense MFMA peaks, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
# SURVEY.md 8(d) defines the sharpened weight set by its effect: logit std ~5 (max prob ~1e-2, joints spread over the cube; input-
# sensitive yet well conditioned -- NOT near-argmax).  With the ctor-default xavier V2V weights and the randomised BatchNorm statistics
# used here the un-scaled logits have std 0.32, so the gain is 16 (x250 measured std 80: a near-argmax where the reference's own
# thread-count noise exceeds the gate; the parity block prints the std it actually got)
SHARPEN = 16.0


def vol_config(num_layers, volume_size, dtype):
    """experiments/human36m/train/human36m_vol_softmax.yaml:26-53 of the reference, as a ConfigDict."""
    from mvn.utils.cfg import ConfigDict
    return ConfigDict({"model": {
        "name": "vol", "kind": "mpii", "volume_aggregation_method": "softmax", "init_weights": False, "checkpoint": "",
        "use_gt_pelvis": False, "cuboid_side": 2500.0, "volume_size": volume_size, "volume_multiplier": 1.0,
        "volume_softmax": True, "heatmap_softmax": True, "heatmap_multiplier": 100.0, "compute_dtype": dtype,
        "backbone": {"name": "resnet%d" % num_layers, "style": "simple", "init_weights": False, "checkpoint": "",
                     "num_joints": 17, "num_layers": num_layers}}})


def synthetic_batch(B, NV, image, seed):
    """randn images, NV ring cameras (r=4000 mm, h=1000 mm, f=1.2*H) looking at the origin,
    pelvis ~ N(0, 100 mm)."""
    from mvn.utils.multiview import Camera
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, NV, 3, image, image, generator=g)
    cams, Ks, Rs, ts = [], [], [], []
    for v in range(NV):
        phi = 2.0 * np.pi * v / NV
        Cc = np.array([4000.0 * np.cos(phi), 4000.0 * np.sin(phi), 1000.0])
        fwd = -Cc / np.linalg.norm(Cc)
        right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        t = (-R @ Cc).reshape(3, 1)
        K = np.array([[1.2 * image, 0, image / 2.0], [0, 1.2 * image, image / 2.0], [0, 0, 1.0]])
        cams.append([Camera(R, t, K) for _ in range(B)])
        Ks.append(K); Rs.append(R); ts.append(t)
    kp = np.random.RandomState(seed).randn(B, 17, 3) * 100.0
    return images, {"cameras": cams, "pred_keypoints_3d": kp}, (np.stack(Ks), np.stack(Rs), np.stack(ts))


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_leg(state_dict, args, images, batch, geom):
    """The oracle (oracle/vol_oracle.py: the reference's forward restated on torch-CPU fp32 -- the same ATen conv / batch_norm /
    grid_sample / softmax calls the reference issues, pinned to the reference's own outputs by tests/golden) on the host cores
    of this box, same weights.  One forward of sample 1 (warm-up) and as many timed forwards of sample 0 as fit ~budget_s
    (at least 1): their joints are also the parity references for samples 0 and 1 of the timed GPU batch."""
    from oracle import vol_oracle
    from oracle.synth import AttrDict
    cfg = AttrDict(vol_config(args.layers, args.volume, "fp32"))
    K, R, t = geom
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = max(1, min(avail, args.cpu_threads))   # oneDNN on >64 threads thrashes on these small layers (measured: 256 threads -> 170 s/forward)
    torch.set_num_threads(cores)
    run = lambda i: vol_oracle.volumetric_forward(sd, cfg, images[i:i + 1], K, R, t, batch["pred_keypoints_3d"][i:i + 1], stages=True)
    budget_s = args.cpu_budget_s
    nref = max(1, min(args.cpu_parity_samples, images.shape[0]))
    refs = [None] * nref
    if nref > 1:
        refs[1] = run(1)
    n, t0 = 0, time.perf_counter()
    while n < 1 or (time.perf_counter() - t0 < budget_s and n < 16):
        refs[0] = run(0); n += 1
    dt = time.perf_counter() - t0
    base = {"value": n / dt, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "kind_note": "oracle/ restatement issuing the reference's own ATen ops; pinned: oracle/make_golden.py runs the imported reference and the oracle on the same "
                         "inputs and all 88 stage comparisons differ by exactly 0.0 (tests/golden/*), so timing the port times the reference's arithmetic",
            "cpu_model": cpu_model_name(), "logical_cpus": os.cpu_count(),
            "sample": "%d forwards of B=1 (%d views %dx%d, %d^3 voxels, ResNet-%d, fp32), %.1f s" % (
                n, args.views, args.image, args.image, args.volume, args.layers, dt)}
    return base, refs


def parity_block(kp_gpu, refs, dtype, cuboid_side=2500.0):
    """Joints of the timed kernel set vs the oracle: SURVEY.md 8(d) gate formula (max |d| / max(|ref|, 1 mm)) and MPJPE."""
    kp = kp_gpu[:len(refs)].float().cpu().numpy()
    ref = np.concatenate([r["keypoints_3d"].numpy() for r in refs])
    rel = np.abs(kp - ref) / np.maximum(np.abs(ref), 1.0)
    lg = np.concatenate([r["logits"].numpy().ravel() for r in refs])
    # the oracle's (= the reference's) own fp32 soft-argmax against the exact fp64 one of its logits: torch's softmax / einsum over V^3
    # voxels carry a reduction error (3e-5 at 64^3, 2.9e-4 at 128^3) that bounds how close ANY kernel can be to the reference
    exact = []
    for r in refs:
        l64 = r["logits"].double().reshape(1, r["logits"].shape[1], -1)
        p64 = torch.softmax(l64, dim=2)
        exact.append(torch.einsum("bjn,bnc->bjc", p64, r["coord_volumes"].double().reshape(1, -1, 3)).numpy())
    exact = np.concatenate(exact)
    rel_exact = np.abs(kp.astype(np.float64) - exact) / np.maximum(np.abs(exact), 1.0)
    ref_self = np.abs(ref.astype(np.float64) - exact) / np.maximum(np.abs(exact), 1.0)
    dabs = np.abs(kp.astype(np.float64) - ref.astype(np.float64))
    dabs_exact = np.abs(kp.astype(np.float64) - exact)
    return {"dtype": dtype, "samples": len(refs), "joints_max_rel": float(rel.max()),
            "joints_max_abs_mm": float(dabs.max()), "joints_max_abs_mm_vs_exact": float(dabs_exact.max()),
            "joints_max_abs_over_cuboid_side": float(dabs.max() / cuboid_side), "cuboid_side_mm": float(cuboid_side),
            "joints_max_rel_vs_exact_softargmax_of_ref_logits": float(rel_exact.max()), "reference_own_fp32_reduction_error": float(ref_self.max()),
            "mpjpe_mm": float(np.sqrt(((kp - ref) ** 2).sum(-1)).mean()), "gate": 1e-4, "meets_gate": bool(rel.max() <= 1e-4 + ref_self.max() and rel_exact.max() <= 1e-4),
            "against": "CPU oracle (fp32, pinned to the reference's outputs), same weights and inputs, samples 0..%d of the timed batch" % (len(refs) - 1),
            "ref_logit_std": float(lg.std()), "ref_joint_spread_mm": float(ref.std(axis=1).mean())}


def self_launch(args):
    """--gpus N > 1 without a torchrun environment: run under torch.distributed.run, one process per GPU, in a child process; exits with its code."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["LT_BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.run(cmd, env=env).returncode)


def sub_leg(argv, timeout_s):
    """One more configuration in the SAME driver-run line: bench.py re-run as a child process (fresh plan memory; a failing leg cannot
    take the headline down), its one JSON line parsed and embedded.  Used for BASELINE config 4 and the training step."""
    import subprocess
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LT_BENCH_SELF_LAUNCHED"):
        env.pop(k, None)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout_s, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return {"error": "timed out after %d s" % timeout_s, "argv": argv}
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or len(lines) != 1:
        return {"error": "rc %d" % r.returncode, "stderr_tail": r.stderr[-600:], "argv": argv}
    out = json.loads(lines[0])
    out["leg_wall_s"] = time.perf_counter() - t0
    out["argv"] = argv
    return out


def pmc_leg(args, timeout_s=90, train=False, keep_per_kernel=False):
    """HBM traffic and MFMA-busy of THIS run's kernels, measured now: three child runs of this script (one forward each after setup, eager
    launches) under ``rocprofv3 --kernel-trace --pmc <counters>`` -- FETCH_SIZE, WRITE_SIZE and the SQ / GRBM counters in SEPARATE passes, as
    MI355X_MICROARCH.md prescribes -- summarised by tools/pmc_summary.py (FETCH_SIZE x2 on gfx950, KiB -> bytes).  Returns None when
    rocprofv3 is missing or a pass fails (the caller then falls back to the committed file and says so)."""
    import shutil
    import subprocess
    import tempfile
    rp = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rp is None:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    out = tempfile.mkdtemp(prefix="lt_pmc_", dir="/tmp")
    child = [sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "0", "--no-graph",          # plain runs: nothing but the steps
             "--preroll-s", "0", "--batch", str(args.batch), "--views", str(args.views), "--volume", str(args.volume), "--image", str(args.image),
             "--layers", str(args.layers), "--dtype", args.dtype]
    nsteps = 3                     # forwards per pass: 2 setup + 1 timed
    if train:                      # training step: 2 warm-up steps (the first one records the tape) + 1 timed
        child += ["--train", "--train-dtype", args.train_dtype]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LT_BENCH_SELF_LAUNCHED"):
        env.pop(k, None)
    passes = (("pmc_fetch", ["FETCH_SIZE"]), ("pmc_write", ["WRITE_SIZE"]),
              ("pmc_mfma", ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "GRBM_GUI_ACTIVE"]))
    if not train:          # forward legs: the VALU instruction count too (the unprojection gather is VALU-bound: priced against its issue time, VERDICT r4 "next" 6)
        passes += (("pmc_valu", ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE"]),)
    t0 = time.perf_counter()
    try:
        for name, counters in passes:
            cmd = [rp, "--kernel-trace", "--pmc"] + counters + ["--output-format", "csv", "-d", os.path.join(out, name), "-o", "bench", "--"] + child
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, env=env, cwd="/tmp")
            if r.returncode != 0:
                if name == "pmc_valu":          # optional pass: the traffic / MFMA figures stand without it
                    shutil.rmtree(os.path.join(out, name), ignore_errors=True)
                    continue
                return None
        res = pmc_summary.summarise(out, nsteps, args.batch, args.train_dtype if train else args.dtype, args.views, args.volume, "",
                                    " --steps 1 --warmup 0 (3 %s per pass), run by bench.py itself" % ("training steps" if train else "forwards"))
    except (subprocess.TimeoutExpired, OSError, KeyError, ValueError):
        return None
    finally:
        shutil.rmtree(out, ignore_errors=True)
    if not res.get("conv_family_bytes_per_step"):
        return None
    # every kernel of the step together (the training legs report the whole step): busy cycles of the MFMA pipes / shader cycles of all launches
    mf = sum(v.get("mfma_busy_frac", 0.0) * v.get("shader_cycles_per_step", 0.0) for v in res["per_kernel"].values())
    cyc = sum(v.get("shader_cycles_per_step", 0.0) for v in res["per_kernel"].values())
    res["all_kernels_mfma_busy_frac"] = mf / cyc if cyc else None
    res["all_kernels_bytes_per_step"] = res["total_fetch_bytes_per_step"] + res["total_write_bytes_per_step"]
    if train:
        # the STEP's traffic: what the recording step does once (weight packing, index maps, uploads: family "setup+copies") is not part of a replayed step and is
        # reported next to it (round 6; until round 5 it was averaged in: ~3 GB then, ~17 GB with the fragment-order index maps)
        setup = sum(v.get("fetch_bytes_per_step_corrected", 0.0) + v.get("write_bytes_per_step", 0.0) for k, v in res["per_kernel"].items() if train_family(k) == "setup+copies")
        res["recording_step_setup_bytes"] = setup * nsteps
        res["all_kernels_bytes_per_step"] -= setup
    per = res.pop("per_kernel", None)
    if keep_per_kernel:
        res["per_kernel"] = per
    # kernel families by share of the step's shader cycles (training legs: the BatchNorm passes / weight gradients / convolutions split)
    if train and per and cyc:
        # shares of the STEP's kernel time: the profiled passes run three steps of which the first records the tape (weight packing, index maps, uploads --
        # "setup+copies"), so those kernels are left out of the denominator and reported next to the shares as a fraction of everything profiled
        step_cyc = sum(v.get("shader_cycles_per_step", 0.0) for k, v in per.items() if train_family(k) != "setup+copies")
        share = {}
        for k, v in per.items():
            if train_family(k) != "setup+copies":
                share[train_family(k)] = share.get(train_family(k), 0.0) + v.get("shader_cycles_per_step", 0.0) / step_cyc
        res["kernel_share"] = {k: round(v, 3) for k, v in sorted(share.items(), key=lambda kv: -kv[1])}
        res["kernel_share"]["(recording-step setup, of all profiled)"] = round(1.0 - step_cyc / cyc, 3)
        res["kernel_share_other_top"] = [[k, round(v.get("shader_cycles_per_step", 0.0) / step_cyc, 4)] for k, v in
                                         sorted(per.items(), key=lambda kv: -kv[1].get("shader_cycles_per_step", 0.0)) if train_family(k) == "other"][:8]
    res["leg_wall_s"] = time.perf_counter() - t0
    return res


def train_family(k):
    """Kernel name (tools/pmc_summary.kernel_key) -> family of the training step's kernel-time split."""
    if k.startswith(("conv_pack", "stem_pack", "pack_w", "__amd_rocclr", "at::native", "void at::native")):
        # weight packing / index maps / uploads of the RECORDING step (the passes profile 3 steps, the first one records) and runtime copies.  torch's own
        # elementwise kernels belong here: the recording step builds its index maps with them (round 6: the fragment-order maps go through the device packers
        # as byte planes -- ~350 launches, once); a replayed step runs ~20 tiny ones (the reference's loss expressions on (B, 17, 3) tensors)
        return "setup+copies"
    if k.startswith(("bn_", "colsum", "channel_sum")):
        return "batchnorm+sums"
    if "wgrad" in k or k.startswith("pack_n8"):
        return "wgrad"
    if k.startswith(("conv", "pwchain", "stem_pool", "bneck", "splitk", "xr_kernel")):
        return "conv fwd+dgrad"
    if k.startswith(("unproj", "coord_volumes")):
        return "unproject fwd+bwd"
    if k.startswith(("gather", "adam", "cast", "convert", "amax", "quant", "scale_product", "zero", "add_", "pad_")):
        return "params+casts"
    if k.startswith(("sa3", "softargmax", "vol_ce", "maxpool", "global_avgpool", "nchw", "layout")):
        return "pool+softargmax+loss"
    return "other"


def _r(v, nd=4):
    """Rounded to ``nd`` significant digits (floats only): the driver keeps an 8 KB tail of stdout, the line has to fit with room to spare."""
    if isinstance(v, float):
        return float("%.*g" % (nd, v)) if np.isfinite(v) else None
    return v


def _parity_short(p):
    if not p:
        return None
    return {"dtype": p["dtype"], "samples": p["samples"], "joints_max_rel": _r(p["joints_max_rel"], 3), "joints_max_rel_vs_exact": _r(p["joints_max_rel_vs_exact_softargmax_of_ref_logits"], 3),
            "ref_own_err": _r(p["reference_own_fp32_reduction_error"], 3), "max_abs_mm": _r(p["joints_max_abs_mm"], 3), "max_abs_over_cuboid_side": _r(p["joints_max_abs_over_cuboid_side"], 3),
            "mpjpe_mm": _r(p["mpjpe_mm"], 3), "gate": p["gate"], "meets_gate": p["meets_gate"], "ref_logit_std": _r(p["ref_logit_std"], 3)}


def _parity_tiny(p):
    """The three figures of a parity record a child leg keeps in the driver line (its full record goes to stderr / bench_full.json)."""
    if not p:
        return None
    return {"max_abs_mm": _r(p["joints_max_abs_mm"], 3), "mpjpe_mm": _r(p["mpjpe_mm"], 3), "joints_max_rel_vs_exact": _r(p["joints_max_rel_vs_exact_softargmax_of_ref_logits"], 3),
            "meets_gate": p["meets_gate"]}


def _train_short(t):
    """One training leg in ~250 bytes: rate, batch, time, whole-step roofline fraction, live PMC traffic / MFMA-busy where measured, first / last loss."""
    if not t or "error" in t:
        return t and {"error": t["error"]}
    rf = t.get("roofline") or {}
    # (no first / last loss here any more: the legs run different batches, so their pairs said nothing next to each other -- VERDICT r5 weak 1; the
    #  same-batch comparison of the precisions is the train_trajectory leg, the losses of every leg stay in its full record)
    o = {"value": _r(t["value"]), "B": t["config"]["per_gpu_batch"], "ms": _r(t["ms_per_step"]), "frac": _r(rf.get("frac"), 3), "peak": rf.get("peak"),
         "mem_gb": _r(t.get("peak_memory_gb"), 3)}
    if rf.get("traffic"):
        o["traffic_gb"] = _r(rf["traffic"] / 1e9)
        o["mfma_busy_frac"] = _r(rf.get("mfma_busy_frac"), 3)
    rc = t.get("rccl") or {}
    if t.get("n_gpus", 1) > 1:          # an N-GPU training line diagnoses itself: per-rank rates, replicas, what the exchange left exposed behind the backward
        o["per_rank"] = [_r(v, 3) for v in t.get("per_rank_samples_per_s", [])]
        for k in ("replicas_identical_after_training", "gradient_buckets_per_step", "allreduce_window_ms_per_step", "backward_main_stream_ms", "exposed_behind_main_stream_ms"):
            if rc.get(k) is not None:
                o[k] = _r(rc[k], 4) if isinstance(rc[k], float) else rc[k]
    if t.get("kernel_share"):          # the four families that carry the step; the rest (and the recording-step note) stays in the full record
        o["kernel_share"] = {k: v for k, v in list(t["kernel_share"].items())[:4]}
    return o


def compact_line(res, full=True):
    """The ONE stdout line (driver contract), <= 4 KB (4.0 KB on round 5's final record): every headline figure, one-number summaries of every leg; the full records of the legs go to
    stderr (one ``# leg <name>: {json}`` line each, as they finish) and to gpurun_out/bench_full.json (VERDICT r4 "next" 3: the 14 KB line of round 4 did
    not fit the driver's 8 KB tail).  ``full=False``: the line of a plain run, which writes no full record."""
    out = {k: res[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config") if k in res}
    out["value"], out["ms_per_step"] = _r(res["value"], 6), _r(res["ms_per_step"], 6)
    if res.get("n_gpus", 1) > 1:
        out["per_rank_samples_per_s"] = [_r(v) for v in res.get("per_rank_samples_per_s", [])]
    rc = res.get("rccl") or {}
    out["rccl"] = {k: rc[k] for k in ("nranks", "backend", "version", "world_size") if k in rc}
    if rc.get("devices"):
        out["rccl"]["distinct_devices"] = len(set(rc["devices"]))
    rf = res.get("roofline")
    if rf:
        out["roofline"] = {"kernel": "conv family (all %d conv launches of a step)" % rf.get("launches", 0), "bound": "mfma", "achieved": _r(rf["achieved"]), "peak": rf["peak"], "unit": rf["unit"],
                           "frac": _r(rf["frac"]), "traffic": rf.get("traffic") and float("%.4g" % rf["traffic"]), "traffic_over_algorithmic": _r(rf.get("traffic_over_algorithmic"), 3),
                           "traffic_source": "live rocprofv3 --pmc" if (rf.get("traffic_source") or "").startswith("measured in this run") else rf.get("traffic_source"),
                           "mfma_busy_frac": _r(rf.get("mfma_busy_frac"), 3), "flop_per_step": rf["flop_per_step"], "ms_in_kernel": _r(rf["ms_per_step_in_kernel"]),
                           "end_to_end_frac": _r(rf["end_to_end_frac"])}
        if rf.get("sclk_mhz"):
            out["roofline"].update(sclk_mhz=rf["sclk_mhz"], power_w=rf.get("power_w"))
    hb = res.get("roofline_hbm")
    if hb:
        out["roofline_hbm"] = {k: {kk: _r(v.get(kk)) for kk in ("achieved", "frac", "bytes_per_step", "traffic", "ms_per_step_in_kernel", "valu_issue_frac", "lane_insts_per_voxel") if v.get(kk) is not None}
                               for k, v in hb.items()}
    if res.get("parity"):
        out["parity"] = _parity_short(res["parity"])
    f32 = res.get("fp32_parity_mode")
    if f32:
        out["fp32_parity_mode"] = {"value": _r(f32["value"]), "B": f32["per_gpu_batch"], "frac": _r((f32.get("roofline") or {}).get("frac"), 3), "parity": _parity_short(f32.get("parity"))}
    if res.get("batch_sweep"):
        out["batch_sweep"] = {k: _r(v["samples_per_s"]) for k, v in res["batch_sweep"].items()}
    c4 = res.get("config4")
    if c4:
        if "error" in c4:
            out["config4"] = {"error": c4["error"]}
        else:
            r4, h4 = c4.get("roofline") or {}, (c4.get("roofline_hbm") or {}).get("unproject") or {}
            out["config4"] = {"value": _r(c4["value"]), "B": c4["config"]["per_gpu_batch"], "ms": _r(c4["ms_per_step"]), "conv_frac": _r(r4.get("frac"), 3),
                              "conv_traffic_over_algorithmic": _r(r4.get("traffic_over_algorithmic"), 3),
                              "unproject": {kk: _r(h4.get(kk), 3) for kk in ("frac", "ms_per_step_in_kernel", "traffic", "bytes_per_step", "valu_issue_frac") if h4.get(kk) is not None},
                              "parity_bf16": _parity_tiny(c4.get("parity")), "parity_fp32": _parity_tiny((c4.get("fp32_parity_mode") or {}).get("parity"))}
    for k in ("train", "train_mixed", "train_mixed_b16", "train_mixed_b32", "train_fp8v2v"):
        if k in res:
            out[k] = _train_short(res[k])
    if res.get("train_fp8v2v_note"):
        out["train_fp8v2v"] = res["train_fp8v2v_note"]
    tj = res.get("train_trajectory")
    if tj:
        out["train_trajectory"] = {"error": tj["error"]} if "error" in tj else {
            "B": tj["config"]["per_gpu_batch"], "steps": tj["steps"], "first_fp32": _r(tj["curves"]["fp32"][0]) if "fp32" in tj["curves"] else None, "final": {k: _r(v) for k, v in tj["final"].items()},
            "final_rel_to_fp32": {k: _r(v, 3) for k, v in (tj.get("final_rel_to_fp32") or {}).items()},
            "max_rel_gap_to_fp32": {k: _r(v, 3) for k, v in (tj.get("max_rel_gap_to_fp32_over_the_run") or {}).items()}}
    cb = res.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {"value": _r(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"], "cpu_model": cb["cpu_model"], "sample": cb["sample"],
                               "kind_note": "oracle/ = the reference's ATen ops, pinned at 0.0 on all 88 stages (tests/golden)"}
    if res.get("dumped_outputs"):
        out["dumped_outputs"] = res["dumped_outputs"]["dir"]
    if not full:
        return out
    out["full_record"] = "stderr '# leg ...' lines; gpurun_out/bench_full.json"
    return out


def emit_detail(name, rec):
    """A leg's full record on stderr (the one stdout line stays short)."""
    try:
        sys.stderr.write("# leg %s: %s\n" % (name, json.dumps(rec)))
        sys.stderr.flush()
    except Exception:
        pass


class ClockSampler:
    """Shader clock and socket power DURING the timed steps (rank 0 of a 1-GPU run): ``rocm-smi --showclocks --showpower`` polled ~5 times a second by a shell
    loop in its own process (no GIL, no HIP calls in this one), every sample stamped with the wall clock; ``window(t0, t1)`` averages those that fell inside
    the timed region.  Why it is on the line: the bf16 forward runs at the socket power limit and the clock settles near 2.09 GHz -- 0.87 of the 2.4 GHz the
    MFMA peaks assume (profiles/r06_clock_power_bf16_fp32.log) -- so ``roofline.frac`` is read next to the clock it was measured at.  Never fails the run."""

    def __init__(self, device_index):
        self.proc, self.path = None, None
        smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
        if not os.path.exists(smi):
            return
        try:
            fd, self.path = tempfile.mkstemp(prefix="lt_clk_", suffix=".log")
            os.close(fd)
            # a sample counts only when BOTH stamps -- before and after rocm-smi ran (it takes ~0.2 s) -- lie inside the window
            loop = ("while :; do echo \"T $(date +%%s.%%N)\"; %s -d %d --showclocks --showpower 2>/dev/null | grep -E 'sclk|Power'; echo \"E $(date +%%s.%%N)\"; sleep 0.1; done > %s" % (
                smi, device_index, self.path))
            self.proc = subprocess.Popen(["bash", "-c", loop], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, preexec_fn=os.setsid)
        except Exception:
            self.proc = None

    def stop(self):
        if self.proc is not None:
            try:
                os.killpg(os.getpgid(self.proc.pid), 15)          # the exact process group started above
                self.proc.wait(timeout=5)
            except Exception:
                pass
            self.proc = None

    def window(self, t0, t1):
        self.stop()
        if not self.path:
            return None
        try:
            sclk, power, t, cur = [], [], None, [None, None]
            for line in open(self.path):
                if line.startswith("T "):
                    t, cur = float(line.split()[1]), [None, None]
                elif line.startswith("E "):
                    if t is not None and t >= t0 and float(line.split()[1]) <= t1 and cur[0] is not None:
                        sclk.append(cur[0])
                        if cur[1] is not None:
                            power.append(cur[1])
                    t = None
                else:
                    m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", line)
                    if m:
                        cur[0] = int(m.group(1))
                    m = re.search(r"Power \(W\): ([\d.]+)", line)
                    if m:
                        cur[1] = float(m.group(1))
            os.unlink(self.path)
            if not sclk:
                return None
            return {"sclk_mhz": round(sum(sclk) / len(sclk)), "power_w": round(sum(power) / len(power)) if power else None, "samples": len(sclk)}
        except Exception:
            return None


DUMP_BUDGET_BYTES = 64 << 20     # --dump-outputs: all .npy files together
DUMP_SAMPLE_ELEMS = 2 << 20      # outputs up to this many elements are written whole, larger ones as this many elements at fixed, seeded positions


def forward_outputs(out):
    """The forward's 7-tuple (the reference's return order) as named arrays: what a caller of the timed path receives.  Tensors stay where they are;
    the cuboids are host objects (one position per sample, the same sides for all)."""
    kp, feats, probs, conf, cuboids, coords, base_points = out
    named = {"keypoints_3d": kp, "features": feats, "volumes": probs, "vol_confidences": conf, "coord_volumes": coords, "base_points": base_points,
             "cuboid_positions": np.stack([np.asarray(c.position, dtype=np.float64) for c in cuboids]),
             "cuboid_sides": np.stack([np.asarray(c.sides, dtype=np.float64) for c in cuboids])}
    return {k: v for k, v in named.items() if v is not None}


def dump_outputs(named, path):
    """Write every array as ``path/<name>.npy``: float64 stays float64, everything else becomes float32.  An array of more than DUMP_SAMPLE_ELEMS
    elements is written as the DUMP_SAMPLE_ELEMS elements of its flattened form at sorted positions drawn without replacement by a generator seeded
    with the array's name -- the same positions in every run of the same shape.  Returns {name: {"shape", "written", "sampled"}}."""
    import zlib
    os.makedirs(path, exist_ok=True)
    arrays, info = {}, {}
    for name, t in named.items():
        full_shape = tuple(t.shape)
        n = int(np.prod(full_shape))
        idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(n, DUMP_SAMPLE_ELEMS, replace=False)) if n > DUMP_SAMPLE_ELEMS else None
        if isinstance(t, torch.Tensor):
            t = t.detach()
            if idx is not None:
                t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
            a = (t if t.dtype == torch.float64 else t.float()).cpu().numpy()
        else:
            a = np.asarray(t)
            if idx is not None:
                a = a.reshape(-1)[idx]
        a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        arrays[name] = a
        info[name] = {"shape": list(full_shape), "written": list(a.shape), "sampled": n > DUMP_SAMPLE_ELEMS}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        raise RuntimeError("--dump-outputs: %d bytes exceed the %d-byte budget" % (total, DUMP_BUDGET_BYTES))
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return info


def time_steps(step, n, barrier):
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = step()
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def family_table(ops):
    fam = {}
    for o in ops:
        f = fam.setdefault(o["kind"], {"ms": 0.0, "flops": 0, "bytes": 0, "launches": 0})
        f["ms"] += o["ms"]; f["flops"] += o["flops"]; f["bytes"] += o["bytes"]; f["launches"] += 1
    conv = dict(fam["conv"])
    for extra in ("pwchain", "stem"):   # the fused pointwise tail and the fused stem are convolution work too
        if extra in fam:
            conv = {k: conv[k] + fam[extra][k] for k in conv}
    return fam, conv


def make_bench_model(args, dev, dtype=None):
    """The benchmark's network: random-init weights of the architecture (seed 0), BatchNorm running statistics randomised so that folding is not a no-op,
    V2V output layer sharpened so that the 3D soft-argmax is input-sensitive."""
    from mvn.models.triangulation import VolumetricTriangulationNet
    torch.manual_seed(0)
    model = VolumetricTriangulationNet(vol_config(args.layers, args.volume, dtype or args.dtype), device=dev)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
            elif name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=g) * 0.1)
        model.volume_net.output_layer.weight.mul_(SHARPEN)
    return model


def condition_weights(model, seed=11):
    """Variance-preserving random weights for the TRAJECTORY leg: filters ~ N(0, 1.5 / fan_in), the last BatchNorm gamma of every residual branch in
    [0.1, 0.2], the others in [0.8, 1.2] (what a trained ResNet looks like to a perturbation).  With PyTorch's default init (kaiming_uniform(a = sqrt 5), all
    gammas 1) the 152-layer backbone at 16 images per BatchNorm turns ONE 2^-9 rounding of its input images into a 10 % change of the first loss in exact
    fp32 -- a property of that init, under which no two arithmetics can be compared step by step (the control run of this leg shows what is left)."""
    import math
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() >= 4:
                transposed = "deconv" in name or "upsample" in name
                fan_in = (p.shape[0] * p[0, 0].numel() / (2 ** (p.dim() - 2))) if transposed else p[0].numel()
                gain = SHARPEN_COND if name.endswith("output_layer.weight") else 1.0
                p.copy_(torch.randn(p.shape, generator=g) * (gain * math.sqrt(1.5 / fan_in)))
            elif name.endswith((".weight",)) and p.dim() == 1:          # BatchNorm gamma
                last = name.endswith("bn3.weight") or name.endswith("res_branch.4.weight")
                lo, hi = (0.1, 0.2) if last else (0.8, 1.2)
                p.copy_(lo + (hi - lo) * torch.rand(p.shape, generator=g))
            elif p.dim() == 1:                                             # biases / BatchNorm beta
                p.copy_(torch.randn(p.shape, generator=g) * (0.0 if name.endswith("output_layer.bias") else 0.05))
    return model


SHARPEN_COND = 3.0          # output-layer gain of the conditioned weights: input-sensitive soft-argmax (joints spread over the cube), not a near-argmax


def trajectory(make_model, images, batch, gt, precisions, steps, dev, seed=4321, lrs=(1e-4, 1e-3, 1e-3)):
    """The SAME training run in several precisions (VERDICT r4 "next" 1b): identical initial weights (``make_model()`` is called once per
    precision and must be deterministic), identical batch at every step, identical cuboid rotations (numpy seed), the reference's loss
    (MAE + 0.01 x VolumetricCELoss, train.py:217-230) and three-group Adam (train.py:430-437), ``steps`` updates.  Returns {precision: [loss per step]}."""
    import lt_train
    from mvn.models import loss as L
    B = images.shape[0]
    val = torch.ones(B, 17, 1, device=dev)
    out = {}
    for prec in precisions:
        model = make_model()
        model.to(dev)
        model.train()
        imgs = images
        if prec == "fp32_bf16_images":          # CONTROL: the exact fp32 step with its input images rounded to bf16 once, nothing else changed
            prec, imgs = "fp32", images.bfloat16().float()
            out_key = "fp32_bf16_images"
        else:
            out_key = prec
        model.train_precision = prec
        opt = lt_train.Adam([{"params": list(model.backbone.parameters())}, {"params": list(model.process_features.parameters()), "lr": lrs[1]},
                             {"params": list(model.volume_net.parameters()), "lr": lrs[2]}], lr=lrs[0])
        mae, ce = L.KeypointsMAELoss(), L.VolumetricCELoss()
        np.random.seed(seed)
        losses = []
        for _ in range(steps):
            kp, _, vols, _, _, cvs, _ = model(imgs, None, batch)
            loss = mae(kp * 0.1, gt * 0.1, val) + 0.01 * ce(cvs, vols, gt, val)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        out[out_key] = [float(l) for l in losses]
        del model, opt, kp, vols, cvs, loss
        torch.cuda.empty_cache()
    return out


def trajectory_leg(args, dev, images, batch, workload):
    """--train-trajectory: one JSON line with the loss curves of fp32 / act16 / fp8v2v on ONE shared batch (``--batch`` samples, ``--steps`` Adam updates)."""
    B = args.batch
    g = torch.Generator().manual_seed(5)
    gt = (torch.as_tensor(np.asarray(batch["pred_keypoints_3d"]))[:, :, :3].float() + torch.randn(B, 17, 3, generator=g) * 30).to(dev)
    precs = [p for p in args.trajectory_precisions.split(",") if p]
    t0 = time.perf_counter()
    curves = trajectory(lambda: condition_weights(make_bench_model(args, dev)), images, batch, gt, precs, args.steps, dev)
    ref = curves.get("fp32")
    res = {"metric": "training-loss trajectory, same weights / batch / rotations in every precision", "unit": "loss", "n_gpus": 1, "steps": args.steps,
           "config": {"workload": "training steps of: " + workload, "per_gpu_batch": B, "loss": "KeypointsMAELoss(scale 0.1) + 0.01 * VolumetricCELoss",
                      "optimizer": "Adam lr 1e-4 / 1e-3 / 1e-3 (3 groups)", "fixed_batch": True,
                      "weights": "random, variance-preserving (bench.condition_weights); 'fp32_bf16_images' = CONTROL: the fp32 run with its images rounded to bf16 once"},
           "curves": {k: [round(v, 4) for v in c] for k, c in curves.items()},
           "final": {k: c[-1] for k, c in curves.items()},
           "final_rel_to_fp32": {k: (c[-1] - ref[-1]) / abs(ref[-1]) for k, c in curves.items()} if ref else None,
           "max_rel_gap_to_fp32_over_the_run": {k: max(abs(a - b) / abs(b) for a, b in zip(c, ref)) for k, c in curves.items()} if ref else None,
           "wall_s": time.perf_counter() - t0}
    print(json.dumps(res))


TRAIN_DTYPE_NOTE = {
    "fp32": "f32",
    "bf16": "bf16 MFMA for the convolutions, their input gradients and their weight gradients (fp32 accumulation); f32 activations, BatchNorm, master weights, optimiser",
    "act16": "bf16 MFMA for the convolutions, their input gradients and their weight gradients (fp32 accumulation); bf16 activations and activation gradients "
             "(BASELINE config 5's 16-bit activations); f32 BatchNorm statistics, parameter gradients, master weights, optimiser",
    "fp8v2v": "act16 with V2V's 3x3x3 convolutions and their input gradients on the fp8 (e4m3, per-tensor amax scale) MFMA -- BASELINE config 5 as named",
}


def train_leg(args, model, dev, world, rank, barrier, images, batch, workload):
    """--train: BASELINE config 5's step in its present form -- train-mode forward (batch-statistics BatchNorm), MAE + 0.01 x
    VolumetricCELoss (train.py:217-230), backward, gradient all-reduce over RCCL for N > 1 (overlapped with the backward,
    lt_dist.GradReducer), the reference's three-group Adam (train.py:430-437).  fp32 throughout (the reference trains in fp32);
    every kernel is liblt_hip's.  Not the headline metric: its own JSON line."""
    os.environ["LT_TRAIN_TIMING"] = "1"          # the exchange-window / backward event timings of the N-GPU diagnosis (off in production training)
    import lt_dist
    import lt_train
    from mvn.models import loss as L
    B = args.batch
    model.to(dev)
    model.train()
    model.train_precision = args.train_dtype
    np.random.seed(1234 + rank)          # the cuboid rotations of the steps (triangulation.py:318-319): the same sequence every run
    # DistributedDataParallel's semantics (train.py:453): rank 0's parameters and buffers on every rank before the first step (the ranks
    # build their models from the same seed here, attach() makes it true whatever they did), buffers re-broadcast at every forward
    model.grad_reducer = lt_dist.GradReducer().attach(model) if world > 1 else None
    opt = lt_train.Adam([{"params": list(model.backbone.parameters())}, {"params": list(model.process_features.parameters()), "lr": 1e-3},
                         {"params": list(model.volume_net.parameters()), "lr": 1e-3}], lr=1e-4)
    g = torch.Generator().manual_seed(5 + rank)
    gt = (torch.as_tensor(np.asarray(batch["pred_keypoints_3d"]))[:, :, :3].float() + torch.randn(B, 17, 3, generator=g) * 30).to(dev)
    val = torch.ones(B, 17, 1, device=dev)
    mae, ce = L.KeypointsMAELoss(), L.VolumetricCELoss()
    losses = []

    def step():
        kp, _, vols, _, _, cvs, _ = model(images, None, batch)
        loss = mae(kp * 0.1, gt * 0.1, val) + 0.01 * ce(cvs, vols, gt, val)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()

    for _ in range(max(2, args.warmup)):
        losses.append(step())
    dt_local, _ = time_steps(lambda: losses.append(step()), args.steps, barrier)
    value, total, dt = lt_dist.job_throughput(B * args.steps, dt_local, dev)
    per_rank = lt_dist.gather_floats(B * args.steps / dt_local, dev)
    lv = [float(l) for l in losses]
    assert all(np.isfinite(lv)), lv
    comm = lt_dist.comm_info(dev)          # from the communicator: ranks that took part in an all-reduce, backend, RCCL version, devices
    # self-diagnosis of the N-GPU step (every rank takes part in the collectives inside; rank 0 prints): are the replicas still identical, how many
    # buckets / bytes went through the all-reduce per step, how long the exchange window was next to the backward, what it left exposed
    plan = next(iter(model.__dict__.get("_train_plans", {}).values()), None)
    bt = plan.tape.backward_timing() if plan is not None and plan.tape is not None else None
    if bt:
        comm.update(bt)
    if world > 1:
        comm["replicas_identical_after_training"] = model.grad_reducer.replicas_identical(model, buffers=False)
        comm.update(model.grad_reducer.stats())
        comm["per_rank_samples_per_s"] = per_rank
    if rank == 0:
        # algorithmic flops: forward 2*MAC of every convolution, backward twice that (input + weight gradients)
        P = model._build_plan(1, args.views, args.image, args.image, dev, dry_run=True)
        fwd_flops = P["plan"].flops * B if hasattr(P["plan"], "flops") else None
        res = {"metric": "multi-view samples/sec (%d-view vol-softmax training step: fwd + bwd + Adam)" % args.views, "value": value, "unit": "samples/s",
               "n_gpus": world, "steps": args.steps, "warmup": max(2, args.warmup), "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None,
               "dtype": TRAIN_DTYPE_NOTE[args.train_dtype],
               "data": "synthetic",
               "config": {"workload": "training step of: " + workload, "per_gpu_batch": B, "global_batch": B * world,
                          "parallelism": "data parallel x%d, bucketed gradient all-reduce (RCCL) overlapped with the backward" % world if world > 1 else "1 GPU",
                          "loss": "KeypointsMAELoss(scale 0.1) + 0.01 * VolumetricCELoss", "optimizer": "Adam lr 1e-4 / 1e-3 / 1e-3 (3 groups)"},
               "per_rank_samples_per_s": per_rank, "loss_first_last": [lv[0], lv[-1]], "losses": [round(v, 4) for v in lv],
               "rccl": comm,
               "peak_memory_gb": torch.cuda.max_memory_allocated(dev) / 1e9}
        if fwd_flops:
            ach = 3 * fwd_flops / (1e-3 * res["ms_per_step"]) / 1e12
            # the peak the step's FLOPs run against: every convolution product of the mixed step (forward, input gradient, weight gradient) is a bf16
            # MFMA, every one of the fp32 step an exact-fp32 MFMA -- so the whole-step figure is priced against that dtype's dense peak
            pk = PEAK_TFLOPS["fp32" if args.train_dtype == "fp32" else "bf16"]
            live = pmc_leg(args, timeout_s=240, train=True) if (world == 1 and not args.no_pmc_leg) else None
            res["roofline"] = {"kernel": "whole step (convolutions: forward + input gradient + weight gradient = 3 x forward MACs)", "bound": "mfma",
                               "achieved": ach, "peak": pk, "unit": "TFLOP/s", "frac": ach / pk,
                               "peak_basis": "dense %s MFMA peak: all three convolution products of this step run on that MFMA%s" % (
                                   "fp32" if args.train_dtype == "fp32" else "bf16",
                                   " (the non-scaled fp8 MFMA of the V2V convolutions issues at the bf16 rate, MI355X_MICROARCH.md)" if args.train_dtype == "fp8v2v" else ""),
                               "traffic": live["all_kernels_bytes_per_step"] if live else None,
                               "mfma_busy_frac": live["all_kernels_mfma_busy_frac"] if live else None,
                               "traffic_source": ("measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE | SQ counters, three child runs of this "
                                                  "command (all kernels of a step; %.0f s)" % live["leg_wall_s"]) if live else None}
            if live and live.get("kernel_share"):
                res["kernel_share_other_top"] = live.get("kernel_share_other_top")
                res["kernel_share"] = live["kernel_share"]          # share of the step's summed kernel time (both streams) by family, from the same PMC passes
        print(json.dumps(res))
    barrier()
    lt_dist.shutdown()


def preflight(args, world, rank, local):
    """``bench.py --gpus N --preflight``: make the first N-GPU run on hardware boring.  Three checks, each through the process group the timed runs use,
    one JSON line from rank 0 (``ok`` = all of them passed), then exit:
      1. census -- an all-reduce of ones counts the ranks, an all-gather collects every rank's device (name / PCI bus id): N ranks on N DISTINCT devices;
      2. one 64 MB fp32 all-reduce, timed (two warm-ups, three timed; max over ranks): algorithmic and bus bandwidth 2 (N - 1) / N x bytes / t -- an xGMI ring is
         per-link bound (~153 GB/s per link, MI355X guide), so a healthy 8-GPU node shows a few hundred GB/s here and a mis-routed one (PCIe) ~20;
      3. one data-parallel training step (reference train.py:450-460: DistributedDataParallel semantics through lt_dist.GradReducer -- rank 0's weights
         broadcast, per-rank batches, bucketed gradient all-reduce overlapped with the backward, Adam): finite loss, ``replicas_identical`` afterwards.
    --stub-cpu runs the same three checks over gloo with a stand-in model (tests/test_distributed_cpu.py)."""
    import lt_dist
    stub = args.stub_cpu
    if stub:
        dev = torch.device("cpu")
    else:
        if torch.cuda.device_count() <= local:
            raise RuntimeError("rank %d needs cuda:%d but only %d GPU(s) are visible" % (rank, local, torch.cuda.device_count()))
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    sync = (lambda: None) if stub else torch.cuda.synchronize
    comm = lt_dist.comm_info(dev)
    devices = comm.get("devices") or []
    census_ok = comm.get("nranks") == world and (stub or world == 1 or len(set(devices)) == world)
    # ---- one 64 MB all-reduce, timed
    n = (64 << 20) // 4
    buf = torch.ones(n, dtype=torch.float32, device=dev)
    times = []
    for it in range(5):
        sync(); lt_dist.barrier(); sync()
        t0 = time.perf_counter()
        if world > 1:
            torch.distributed.all_reduce(buf)
        sync()
        dt = lt_dist.max_over_ranks(time.perf_counter() - t0, dev)
        if it >= 2:
            times.append(dt)
        buf.fill_(1.0)
    t_ar = sorted(times)[len(times) // 2]
    allreduce = {"bytes": 4 * n, "ms": 1e3 * t_ar, "algorithmic_gb_per_s": 4 * n / t_ar / 1e9 if world > 1 else None,
                 "bus_gb_per_s": (2 * (world - 1) / world) * 4 * n / t_ar / 1e9 if world > 1 else None}
    # ---- one data-parallel training step
    torch.manual_seed(100 + rank)          # the ranks START different on purpose: attach() has to make them identical
    step_info = {}
    if stub:
        net = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.BatchNorm1d(256), torch.nn.Linear(256, 64))
        red = lt_dist.GradReducer(bucket_bytes=32 << 10).attach(net) if world > 1 else None
        x = torch.randn(8, 64, generator=torch.Generator().manual_seed(7 + rank))
        loss = net(x).pow(2).mean()
        loss.backward()
        arena = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
        if red is not None:
            for o in range(0, arena.numel(), 8192):
                red.reduce_inplace(arena[o:o + 8192])
            red.wait_all()
        o = 0
        with torch.no_grad():
            for p in net.parameters():
                p.sub_(1e-3 * arena[o:o + p.numel()].view(p.shape)); o += p.numel()
        step_info = {"loss": float(loss), "model": "stand-in (Linear + BatchNorm1d + Linear)"}
        model = net
    else:
        import lt_train
        from mvn.models import loss as L
        pre = argparse.Namespace(**vars(args))
        pre.layers, pre.volume = 50, 32          # a small member of the family (ResNet-50, 32^3 voxels, 2 samples of 4 x 256^2): seconds, same code path
        B, image = 2, 256
        model = make_bench_model(pre, dev)
        model.to(dev); model.train(); model.train_precision = "act16"
        red = model.grad_reducer = lt_dist.GradReducer().attach(model) if world > 1 else None
        images_cpu, batch, _ = synthetic_batch(B, args.views, image, 1000 + rank)
        images = images_cpu.to(dev)
        opt = lt_train.Adam([{"params": list(model.parameters())}], lr=1e-4)
        gt = (torch.as_tensor(np.asarray(batch["pred_keypoints_3d"]))[:, :, :3].float()).to(dev)
        val = torch.ones(B, 17, 1, device=dev)
        np.random.seed(1234 + rank)
        t0 = time.perf_counter()
        kp, _, vols, _, _, cvs, _ = model(images, None, batch)
        loss = L.KeypointsMAELoss()(kp * 0.1, gt * 0.1, val) + 0.01 * L.VolumetricCELoss()(cvs, vols, gt, val)
        opt.zero_grad(); loss.backward(); opt.step()
        sync()
        step_info = {"loss": float(loss), "model": "ResNet-50 backbone, 32^3 voxels, 2 samples x %d views x %dx%d per rank, act16" % (args.views, image, image),
                     "record_and_step_s": time.perf_counter() - t0}
        plan = next(iter(model.__dict__.get("_train_plans", {}).values()), None)
        bt = plan.tape.backward_timing() if plan is not None and plan.tape is not None else None
        if bt:
            step_info.update(bt)
    step_info["loss_finite_on_every_rank"] = lt_dist.sum_over_ranks(1.0 if np.isfinite(step_info["loss"]) else 0.0, dev) == world
    if world > 1:
        step_info["replicas_identical_after_training"] = bool(red.replicas_identical(model, buffers=False))
        step_info.update(red.stats())
    ok = bool(census_ok and step_info["loss_finite_on_every_rank"] and (world == 1 or step_info["replicas_identical_after_training"]))
    lt_dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "preflight", "ok": ok, "n_gpus": world, "backend": comm.get("backend"), "rccl": comm, "census_ok": bool(census_ok),
                          "allreduce_64MB": allreduce, "train_step": step_info, "self_launched": os.environ.get("LT_BENCH_SELF_LAUNCHED") == "1"}))
    lt_dist.shutdown()
    if not ok:
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="samples per GPU per step (default 64; 16 for 128^3 volumes: 128 images fill the 256 CUs with 288-row tiles; 8 for --train)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--image", type=int, default=384)
    ap.add_argument("--volume", type=int, default=64)
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU leg (then no parity block either)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the fp32 parity-mode leg and the batch sweep")
    ap.add_argument("--ops-json", default="", help="write the per-launch timing table here")
    ap.add_argument("--cpu-threads", type=int, default=32, help="host threads for the CPU baseline leg")
    ap.add_argument("--tile", type=int, default=0, help="force a conv tile id (LT_TILE_*), 0 = auto")
    ap.add_argument("--preroll-s", type=float, default=1.0, help="untimed steady-state run before the W warm-up steps (clocks settle)")
    ap.add_argument("--train-dtype", default="fp32", choices=["fp32", "bf16", "act16", "fp8v2v"], help="--train: act16 = bf16 MFMA + bf16 activations / activation gradients; fp8v2v = act16 + fp8 V2V convolutions; fp32 (the reference's precision, default) or bf16 = the "
                    "convolutions and their input gradients on the bf16 MFMA (bf16 copies of the operands, fp32 accumulation / storage), everything else fp32")
    ap.add_argument("--train", action="store_true", help="time the training step (fwd + bwd + Adam, fp32) instead of the forward; its own JSON line")
    ap.add_argument("--train-trajectory", action="store_true", help="--steps Adam updates on ONE fixed batch of --batch samples in each of --trajectory-precisions "
                    "(same weights, batch, rotations): the loss curves side by side, its own JSON line")
    ap.add_argument("--trajectory-precisions", default="fp32,fp32_bf16_images,act16,fp8v2v")
    ap.add_argument("--full-line", action="store_true", help="print the full record on stdout instead of the compact line (child legs are run this way)")
    ap.add_argument("--force-pmc-leg", action="store_true", help="measure roofline.traffic live even with --no-extras (the config-4 child leg of a --full run)")
    ap.add_argument("--no-pmc-leg", action="store_true", help="do not measure roofline.traffic live (rocprofv3 child runs, ~1 min); use the committed PMC file")
    ap.add_argument("--no-legs", action="store_true", help="skip the config-4 and training legs of a --full run (config 2, N = 1)")
    ap.add_argument("--cpu-budget-s", type=float, default=20.0, help="CPU baseline leg: timed forwards of sample 0 until this many seconds (at least one)")
    ap.add_argument("--cpu-parity-samples", type=int, default=2, help="samples of the timed batch the CPU oracle evaluates as parity references")
    ap.add_argument("--fp32-parity-batch", type=int, default=0, help="with --no-extras: also run this many samples through the exact-fp32 kernel set and report their "
                    "parity (the config-4 child leg of a --full run: the --full line then shows config 4 inside the tolerance)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write the arrays the last timed step returned (rank 0's "
                    "shard) as DIR/<name>.npy, float32 / float64, at most 64 MB in all: small outputs whole, large ones as a fixed seeded sample of "
                    "their elements (see dump_outputs).  Forward runs only")
    ap.add_argument("--full", action="store_true", help="measure everything besides the headline: the CPU baseline and parity, the per-kernel roofline (live PMC "
                    "passes, shader clock), the fp32 parity-mode leg, the batch sweep, the config-4 and training child legs, the live PMC figures of --train.  "
                    "Without it a run sets up, warms up, times the steps, dumps (--dump-outputs) and prints the line; the --no-* options above subtract from --full")
    ap.add_argument("--stub-cpu", action="store_true", help="TEST ONLY: gloo backend, no GPU, step() is a sleep (exercises launcher + timing plumbing)")
    ap.add_argument("--preflight", action="store_true", help="N-GPU sanity run before a scaling session (VERDICT r5 'next' 7): communicator census (ranks, distinct "
                    "devices, RCCL version), ONE timed 64 MB all-reduce, ONE data-parallel training step with the replicas checked identical, then exit with its own JSON line")
    args = ap.parse_args()
    if args.dump_outputs and (args.train or args.train_trajectory or args.preflight or args.stub_cpu):
        ap.error("--dump-outputs writes what the timed forward returns: not with --train, --train-trajectory, --preflight or --stub-cpu")
    if not args.full:
        # a plain run: the headline and nothing else (no CPU leg, no profiled passes, no PMC child runs, no extra legs)
        if args.ops_json or args.force_pmc_leg or args.fp32_parity_batch:
            ap.error("--ops-json, --force-pmc-leg and --fp32-parity-batch measure more than the headline: they need --full")
        args.no_cpu_baseline = args.no_profile = args.no_extras = args.no_pmc_leg = True
    if not args.batch:
        # 64 samples (256 images) per GPU per step from round 4 on: two full rounds of 288-row tiles on the 256 CUs and half the per-sample share of the
        # ~220 launches' fixed cost (+3 % over 32 samples; 48 samples = 1.5 rounds is slower than either); rounds 1-3 timed 32, which stays in batch_sweep
        args.batch = 4 if args.train_trajectory else 8 if args.train else 16 if args.volume >= 128 else 64

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)       # does not return (exits with the launcher's code)

    import lt_dist
    world, rank, local = lt_dist.init("gloo" if args.stub_cpu else "nccl")   # "nccl" on PyTorch-ROCm is RCCL (xGMI inside the node)
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    barrier = lt_dist.barrier
    B = args.batch
    c2 = (args.views, args.image, args.volume, args.layers) == (4, 384, 64, 152)
    c4 = (args.views, args.volume, args.layers) == (8, 128, 152)
    workload = "%svolumetric-softmax forward, %d views %dx%d, %d^3 voxel cube, ResNet-%d, random-init weights" % (
        "BASELINE config 2: " if c2 else "BASELINE config 4: " if c4 else "", args.views, args.image, args.image, args.volume, args.layers)

    if args.preflight:
        return preflight(args, world, rank, local)

    if args.stub_cpu:       # launcher / collective plumbing without a GPU (tests/test_distributed_cpu.py)
        dev = torch.device("cpu")
        # the exchange of a training step as well, on a stand-in model: attach (rank 0's weights everywhere), a gradient arena that goes through
        # GradReducer in buckets every "step", an SGD update -- so that the line carries the keys an N-GPU --train line diagnoses itself with
        torch.manual_seed(100 + rank)
        net = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.BatchNorm1d(256), torch.nn.Linear(256, 64))
        red = lt_dist.GradReducer(bucket_bytes=32 << 10).attach(net) if world > 1 else None
        arena = torch.zeros(sum(p.numel() for p in net.parameters()))
        el = 0.0
        for it in range(args.steps):
            t0 = time.perf_counter()
            time.sleep(0.002 * (1 + rank))
            el += time.perf_counter() - t0          # this rank's own "compute" (the exchange below synchronises the ranks step by step)
            if red is not None:
                arena.copy_(torch.randn(arena.numel(), generator=torch.Generator().manual_seed(1000 * it + rank)))
                for o in range(0, arena.numel(), 8192):
                    red.reduce_inplace(arena[o:o + 8192])
                red.wait_all()
                o = 0
                with torch.no_grad():
                    for p in net.parameters():
                        p.sub_(1e-3 * arena[o:o + p.numel()].view(p.shape)); o += p.numel()
        barrier()
        value, total, dt = lt_dist.job_throughput(B * args.steps, el, dev)
        per_rank = lt_dist.gather_floats(B * args.steps / el, dev)
        comm = lt_dist.comm_info(dev)          # the same communicator facts the GPU lines carry (backend gloo here)
        if red is not None:
            comm["replicas_identical_after_training"] = red.replicas_identical(net, buffers=False)
            comm.update(red.stats())
            comm["per_rank_samples_per_s"] = per_rank
        if rank == 0:
            print(json.dumps({"metric": "stub", "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": 1e3 * dt / args.steps, "total_samples": total, "per_rank_samples_per_s": per_rank,
                              "self_launched": os.environ.get("LT_BENCH_SELF_LAUNCHED") == "1", "backend": "gloo", "rccl": comm}))
        lt_dist.shutdown()
        return

    if torch.cuda.device_count() <= local:
        raise RuntimeError("rank %d needs cuda:%d but only %d GPU(s) are visible" % (rank, local, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    # random-init weights of the architecture; BatchNorm statistics randomised so that folding is not a no-op; V2V output layer
    # sharpened so that the parity block below measures an input-sensitive soft-argmax, not a cube centroid
    model = make_bench_model(args, dev)
    model.eval()
    model.use_graph = not args.no_graph
    model.tile_override = args.tile
    model.copy_outputs = True
    images_cpu, batch, geom = synthetic_batch(B, args.views, args.image, 1000 + rank)   # rank r owns its own shard of samples

    # ---- CPU leg first (rank 0, N = 1): the reported baseline AND the parity references; the GPU is idle meanwhile, so the timed
    # region below is not a blip at the start of a CPU-dominated run
    cpu_base, refs = None, None
    if world == 1 and rank == 0 and not args.no_cpu_baseline and not args.train and not args.train_trajectory:
        cpu_base, refs = cpu_leg(model.state_dict(), args, images_cpu, batch, geom)
    images = images_cpu.to(dev)
    if args.train_trajectory:
        del model
        trajectory_leg(args, dev, images, batch, workload)
        lt_dist.shutdown()
        return
    if args.train:
        return train_leg(args, model, dev, world, rank, barrier, images, batch, workload)

    def step():
        return model(images, None, batch)

    # setup, not a step of the contract: the first call records the plan and captures the hipGraph, the second is the graph's
    # first replay (upload); then an untimed steady-state pre-roll (power / clocks settle), the W warm-up steps, the K timed steps
    for _ in range(2):
        out = step()
    torch.cuda.synchronize()
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < args.preroll_s:
        out = step(); torch.cuda.synchronize()
    # (the clocks go on the roofline block only: no sampler where no roofline is computed)
    sampler = ClockSampler(local) if (world == 1 and rank == 0 and not args.no_profile and os.environ.get("LT_BENCH_NO_CLOCKS") != "1") else None
    for _ in range(args.warmup):
        out = step()
    t_w0 = time.time()
    dt_local, out = time_steps(step, args.steps, barrier)
    t_w1 = time.time()
    clocks = sampler.window(t_w0, t_w1) if sampler else None
    value, total_samples, dt = lt_dist.job_throughput(B * args.steps, dt_local, dev)   # all ranks' samples / slowest rank
    per_rank = lt_dist.gather_floats(B * args.steps / dt_local, dev)
    assert torch.isfinite(out[0]).all()
    dumped = dump_outputs(forward_outputs(out), args.dump_outputs) if (args.dump_outputs and rank == 0) else None
    comm = lt_dist.comm_info(dev)          # all ranks: an all-reduce of ones through the communicator (nranks), backend, RCCL version, devices

    result = None
    if rank == 0:
        result = {
            "metric": "multi-view samples/sec (%d-view vol-softmax forward)" % args.views, "value": value, "unit": "samples/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": workload, "per_gpu_batch": B, "global_batch": B * world,
                       "parallelism": "batch-sharded replicas x%d, no data-path collective" % world,
                       "hip_graph": not args.no_graph, "self_launched": os.environ.get("LT_BENCH_SELF_LAUNCHED") == "1"},
            "per_rank_samples_per_s": per_rank, "rccl": comm,
        }
        if dumped is not None:
            result["dumped_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": dumped}
        if refs is not None:
            result["parity"] = parity_block(out[0], refs, args.dtype, model.cuboid_side)
        if not args.no_profile:
            plan = list(model._plans.values())[-1]["plan"]
            side = model._side_stream(dev)
            with torch.cuda.stream(side):
                plan.run_profiled(side.cuda_stream, reps=1)
                ops = plan.run_profiled(side.cuda_stream, reps=3)
            fam, conv = family_table(ops)
            peak = PEAK_TFLOPS[args.dtype]
            ach = conv["flops"] / (conv["ms"] * 1e-3) / 1e12
            # HBM traffic per step: measured in THIS run by the PMC leg (rocprofv3 children of this script) when it is available; else from the
            # committed PMC passes of this command (tools/pmc_summary.py; same batch and dtype only) -- traffic_source says which
            pmc, pmc_file = {}, None
            live = None
            if world == 1 and not args.no_pmc_leg and (not args.no_extras or args.force_pmc_leg):
                live = pmc_leg(args)
            for name in ([] if live else ["r06_hbm_traffic_pmc.json", "r05_hbm_traffic_pmc.json", "r03_hbm_traffic_pmc.json", "r02_hbm_traffic_pmc.json", "r01_hbm_traffic_pmc.json"]):
                try:
                    pm = json.load(open(os.path.join(ROOT, "profiles", name)))
                except (OSError, ValueError):
                    continue
                if pm.get("per_gpu_batch") == B and pm.get("dtype", "bf16") == args.dtype and pm.get("views", 4) == args.views and pm.get("volume", 64) == args.volume:
                    pmc, pmc_file = pm, "profiles/" + name
                    break
            src = None if pmc_file is None else pmc_file + " (rocprofv3 --pmc passes of this command, committed; not re-measured in this run)"
            if live:
                pmc = live
                src = "measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE | SQ counters, three child runs of this command (%s; %.0f s)" % (
                    "eager launches, 3 forwards per pass", live["leg_wall_s"])
            result["roofline"] = {"kernel": "conv family: conv_igemm2/3/6/7, bneck / bneck_ds, xr, conv3d_halo*, conv_pw, stem_pool, pwchain (all %d launches of one step)" % conv["launches"],
                                  "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                                  "traffic": pmc.get("conv_family_bytes_per_step"), "traffic_source": src,
                                  "mfma_busy_frac": pmc.get("conv_family_mfma_busy_frac"),
                                  "flop_per_step": conv["flops"], "ms_per_step_in_kernel": conv["ms"], "launches": conv["launches"],
                                  # algorithmic bytes of the same launches (every launch's input + output + weights once): traffic above it = re-reads
                                  "algorithmic_bytes_per_step": conv["bytes"],
                                  "traffic_over_algorithmic": (pmc["conv_family_bytes_per_step"] / conv["bytes"]) if (pmc.get("conv_family_bytes_per_step") and conv["bytes"]) else None,
                                  "end_to_end_frac": conv["flops"] / (1e-3 * result["ms_per_step"]) / 1e12 / peak}
            if clocks:
                # the clock the chip held during the timed steps (socket power next to it): peak x sclk / 2400 is the roof at THAT clock
                result["roofline"].update(sclk_mhz=clocks["sclk_mhz"], power_w=clocks["power_w"], clock_samples=clocks["samples"],
                                          frac_at_measured_clock=(ach / (peak * clocks["sclk_mhz"] / 2400.0)) if clocks["sclk_mhz"] else None)
            hb = {}
            for k in ("unproject", "softargmax3d", "coord_volumes"):
                if k in fam:
                    a = fam[k]["bytes"] / (fam[k]["ms"] * 1e-3) / 1e9
                    hb[k] = {"bound": "hbm", "achieved": a, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": a / PEAK_HBM_GBS,
                             "bytes_per_step": fam[k]["bytes"], "ms_per_step_in_kernel": fam[k]["ms"],
                             "traffic": (pmc.get("hbm_kernels_bytes_per_step") or {}).get(k), "traffic_source": src}
                    vl = (pmc.get("valu") or {}).get(k)
                    if vl and vl.get("issue_frac") is not None:
                        # the gather is VALU-bound, not HBM-bound: its wave-level VALU instruction count (SQ_INSTS_VALU, live PMC pass) x 2 cycles per
                        # wave64 instruction on a SIMD-32, over the kernel's SIMD-cycles -- the fraction of its own issue roof the kernel runs at
                        hb[k]["valu_issue_frac"] = vl["issue_frac"]
                        nvox = B * args.volume ** 3
                        hb[k]["lane_insts_per_voxel"] = vl["wave_insts_per_step"] * 64.0 / nvox if k == "unproject" else None
            result["roofline_hbm"] = hb
            result["kernel_time_ms_per_step"] = {k: round(v["ms"], 4) for k, v in fam.items()}
            if args.ops_json:
                os.makedirs(os.path.dirname(os.path.abspath(args.ops_json)), exist_ok=True)
                json.dump(ops, open(args.ops_json, "w"), indent=0)
        if world == 1 and args.no_extras and args.fp32_parity_batch and refs is not None and args.dtype != "fp32":
            # ---- parity of the exact-fp32 kernel set on the first samples of the timed batch (not a timing leg)
            nb32 = min(args.fp32_parity_batch, B)
            im_b = images[:nb32]
            batch_b = {"cameras": [c[:nb32] for c in batch["cameras"]], "pred_keypoints_3d": batch["pred_keypoints_3d"][:nb32]}
            model.compute_dtype = torch.float32
            model.invalidate_plans()
            torch.cuda.empty_cache()
            for _ in range(2):
                o32 = model(im_b, None, batch_b)
            n32 = 3
            dt32, o32 = time_steps(lambda: model(im_b, None, batch_b), n32, lambda: None)
            result["fp32_parity_mode"] = {"value": nb32 * n32 / dt32, "unit": "samples/s", "steps": n32, "per_gpu_batch": nb32, "ms_per_step": 1e3 * dt32 / n32,
                                          "parity": parity_block(o32[0], refs[:nb32], "fp32", model.cuboid_side)}
            model.compute_dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.dtype]
            model.invalidate_plans()
            del o32
        if world == 1 and not args.no_extras:
            # ---- the same workload on the exact-fp32 kernel set (the mode that meets the 1e-4 gate)
            if args.dtype != "fp32":
                model.compute_dtype = torch.float32
                for _ in range(2):
                    o32 = step()
                n32 = 3
                dt32, o32 = time_steps(step, n32, lambda: None)
                leg = {"value": B * n32 / dt32, "unit": "samples/s", "steps": n32, "per_gpu_batch": B, "ms_per_step": 1e3 * dt32 / n32}
                if not args.no_profile:
                    plan32 = list(model._plans.values())[-1]["plan"]
                    side = model._side_stream(dev)
                    with torch.cuda.stream(side):
                        _, conv32 = family_table(plan32.run_profiled(side.cuda_stream, reps=1))
                    a32 = conv32["flops"] / (conv32["ms"] * 1e-3) / 1e12
                    leg["roofline"] = {"bound": "mfma", "achieved": a32, "peak": PEAK_TFLOPS["fp32"], "unit": "TFLOP/s", "frac": a32 / PEAK_TFLOPS["fp32"]}
                if refs is not None:
                    leg["parity"] = parity_block(o32[0], refs, "fp32", model.cuboid_side)
                result["fp32_parity_mode"] = leg
                model.compute_dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.dtype]
                model.invalidate_plans()
                del o32
                torch.cuda.empty_cache()
            # ---- the reference's own batch sizes (train 5, val 10) and single-sample latency
            sweep = {}
            for bs in (1, 5, 10, 32):
                if bs >= B:
                    continue
                im_b = images[:bs]
                batch_b = {"cameras": [c[:bs] for c in batch["cameras"]], "pred_keypoints_3d": batch["pred_keypoints_3d"][:bs]}
                sb = lambda: model(im_b, None, batch_b)
                for _ in range(4):
                    sb()
                nb = 20
                dtb, _ = time_steps(sb, nb, lambda: None)
                sweep[str(bs)] = {"samples_per_s": bs * nb / dtb, "ms_per_step": 1e3 * dtb / nb}
            result["batch_sweep"] = sweep
            if c2 and not args.no_legs:
                # ---- the other BASELINE configurations in the same driver-run line (VERDICT r2 "next" 4): config 4 (8 views, 128^3) with its
                # own roofline / roofline_hbm / parity, and the training step (config 5's step on one GPU, fp32 like the reference)
                del out
                model.invalidate_plans()
                torch.cuda.empty_cache()
                result["config4"] = sub_leg(["--full", "--views", "8", "--volume", "128", "--batch", "16", "--steps", "8", "--warmup", "3", "--no-extras", "--full-line",
                                             "--cpu-budget-s", "1", "--cpu-parity-samples", "1", "--preroll-s", "0.3", "--force-pmc-leg", "--fp32-parity-batch", "2"], 600)
                emit_detail("config4", result["config4"])
                # (live PMC passes -- three profiled child runs that each re-record the tape, ~90 s -- on ONE training leg: the act16 one)
                result["train"] = sub_leg(["--full", "--train", "--batch", "4", "--steps", "8", "--warmup", "2", "--no-pmc-leg"], 600)
                # config 5's reduced-precision step as BASELINE names it: 16-bit activations (bf16) + bf16 MFMA for every convolution product (train_precision
                # "act16"), and the same with V2V's 3x3x3 convolutions on the fp8 MFMA ("fp8v2v"); fp32 BatchNorm statistics, master weights, optimiser.
                # Not parity modes -- their loss values are printed next to the fp32 leg's, same seeds.  (Round 3's "bf16" mode -- bf16 MFMA over fp32
                # activations -- is still selectable: --train-dtype bf16.)
                result["train_mixed"] = sub_leg(["--full", "--train", "--train-dtype", "act16", "--batch", "8", "--steps", "6", "--warmup", "2"], 600)
                result["train_mixed_b16"] = sub_leg(["--full", "--train", "--train-dtype", "act16", "--batch", "16", "--steps", "5", "--warmup", "2", "--no-pmc-leg"], 600)
                # 32 samples per GPU per step: 147 GB of the 288 GB -- the batch this memory is for (the step's ~620 dependent launches per direction are
                # latency-bound at 8 samples: 32 images per BatchNorm layer; DESIGN.md "Round 5")
                result["train_mixed_b32"] = sub_leg(["--full", "--train", "--train-dtype", "act16", "--batch", "32", "--steps", "4", "--warmup", "2", "--no-pmc-leg"], 900)
                # 'fp8v2v' (act16 + e4m3 V2V convolutions) is NOT a default timing leg any more (VERDICT r4 "next" 1: faster than act16 or out): measured at
                # 139.1 vs 143.6 samples/s -- V2V's 3x3x3 layers at 32-128 channels are not MFMA-bound (the fp8 halo kernel: 99 us vs bf16's 104), so
                # e4m3 operands cannot pay for their amax / quantise passes.  Still selectable (--train --train-dtype fp8v2v), gated as a whole step
                # (tests/test_gpu_train.py) and part of the trajectory leg below.
                result["train_fp8v2v_note"] = "not timed by default: slower than act16 (139.1 vs 143.6 samples/s, round 5) -- bench.py --train --train-dtype fp8v2v"
                # the SAME run in the three precisions: identical weights, one fixed batch of 4 samples, identical rotations, 20 Adam updates (VERDICT r4 "next" 1b)
                result["train_trajectory"] = sub_leg(["--full", "--train-trajectory", "--batch", "4", "--steps", "20"], 900)
                for k in ("train", "train_mixed", "train_mixed_b16", "train_mixed_b32", "train_trajectory"):
                    emit_detail(k, result[k])
        if cpu_base is not None:
            result["cpu_baseline"] = cpu_base
    barrier()
    if rank == 0:
        emit_detail("full", result)
        if not args.full_line and not args.no_extras:          # (the top-level --full run only: the child legs would overwrite it)
            try:
                os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                json.dump(result, open(os.path.join(ROOT, "gpurun_out", "bench_full.json"), "w"), indent=1)
            except OSError:
                pass
        print(json.dumps(result if args.full_line else compact_line(result, full=args.full)))
    lt_dist.shutdown()


if __name__ == "__main__":
    main()
