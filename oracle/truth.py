"""TEST INFRASTRUCTURE (see oracle/__init__.py).

fp64 ground truth for the golden fixtures: the oracle (oracle/vol_oracle.py) in its fp64 mode, on exactly the inputs of the
fp32 fixture beside it -- the same seeds, synthetic weights and images, and the inputs the reference defines in fp32 (projection
matrices, coordinate volumes) promoted as they are.  Everything after them runs in fp64.

oracle/make_golden.py ``truth`` writes what these functions return to tests/golden/truth_<name>.npz, together with the measured
error of the reference's fp32 outputs against it (``ref32_err/<key>``); tests/test_oracle_truth_cpu.py checks that they reproduce
the committed files.  Keys are those of the fp32 fixture; the volumetric sub-samples are twice as coarse (STRIDE_FACTOR below).  Joints are kept in fp64; intermediates are the fp32
rounding of the fp64 truth (<= 6e-8 relative, far below any gate).
"""
import os
import sys

import numpy as np
import torch

from . import spec, synth
from . import vol_oracle as O

F64 = torch.float64
ALG_CASES = ("alg_c1", "alg_relu_noconf")
NETS = ((152, 128, False), (50, 128, True), (18, 64, False))      # gen_nets: (depth, image size, confidence heads)
JOINT_KEYS = ("kp", "kp2", "kp3", "kp3_of_ref2d")
# the truth of a volumetric fixture keeps every STRIDE_FACTOR-th point of the fixture's strided sub-samples (its stride is STRIDE_FACTOR x
# the fixture's): at the fixture's own stride the fp32-rounded truth of c2_b4 takes 4.9 MB, and a file in the repository stays below 1 MiB
STRIDE_FACTOR = 2
MAX_BYTES = 1 << 20
REF_KEY = {"kp3_of_ref2d": "kp3"}          # the fp32 fixture's counterpart of a truth key: the reference's DLT of its own 2D keypoints


def _tests_dir():
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    if d not in sys.path:
        sys.path.insert(0, d)
    return d


def vol_cases():
    _tests_dir()
    from test_oracle_golden import VOL_CASES
    return list(VOL_CASES)


def coarser(a, factor):
    """Every ``factor``-th point over the trailing spatial dims of a strided (N, C, spatial...) sub-sample: the fixture's array at the truth's points."""
    a = np.asarray(a)
    return a[(slice(None), slice(None)) + tuple(slice(None, None, factor) for _ in range(a.ndim - 2))]


def _sub(t, s):
    sl = (slice(None), slice(None)) + tuple(slice(None, None, s) for _ in range(t.dim() - 2))
    return t[sl].contiguous().numpy()


def images_digest(images):
    return np.array([float(images.double().sum()), float((images.double() ** 2).sum())])


def vol_truth(tag, stride):
    """The fp64 volumetric forward of fixture vol_<tag> (run_vol_case's inputs), sub-sampled at ``stride`` (STRIDE_FACTOR x the fixture's)."""
    _tests_dir()
    from test_oracle_golden import build_vol_case
    cfg, sd, inp, c = build_vol_case(tag)
    thetas = None
    if c["rotate"]:                 # run_vol_case: np.random.seed(seed + 100); uniform(0, 2 pi, B)
        np.random.seed(c["seed"] + 100)
        thetas = np.random.uniform(0.0, 2 * np.pi, size=c["B"])
    o = O.volumetric_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"], inp["pred_keypoints_3d"], thetas=thetas,
                             stages=True, dtype=F64)
    B, NV = c["B"], c["NV"]
    f = o["features"]
    res = {"kp": o["keypoints_3d"].numpy(),
           "feat_sub": _sub(f.reshape(B * NV, *f.shape[2:]), stride).astype(np.float32),
           "unproj_sub": _sub(o["unprojected"], stride).astype(np.float32),
           "logits_sub": _sub(o["logits"], stride).astype(np.float32),
           "vol_sub": _sub(o["volumes"], stride).astype(np.float32),
           "stride": np.array(stride),
           "sd_digest": np.array(synth.state_dict_checksum(sd)), "images_digest": images_digest(inp["images"])}
    if o["vol_confidences"] is not None:
        res["vol_conf"] = o["vol_confidences"].numpy().astype(np.float32)
    return res


def nets_truth(which=None):
    """The fp64 backbones of nets.npz (gen_nets: generator seed 9, the V2V input drawn first, then one image batch per depth)."""
    gen = torch.Generator().manual_seed(9)
    torch.randn(1, 32, 32, 32, 32, generator=gen)
    res = {}
    for nl, hw, conf in NETS:
        x = torch.randn(2, 3, hw, hw, generator=gen)
        if which is not None and nl not in which:
            continue
        sd = synth.make_state_dict(spec.pose_resnet_spec(nl, 17, conf, conf, ""), seed=nl, basic_block=(nl < 50))
        with torch.no_grad():
            hm, ft, ac, vc = O.pose_resnet(sd, x, nl, prefix="", dtype=F64)
        res["rn%d_feat_s2" % nl] = _sub(ft, 2).astype(np.float32)
        res["rn%d_hm" % nl] = hm.numpy().astype(np.float32)
        res["rn%d_sd_digest" % nl] = np.array(synth.state_dict_checksum(sd))
        res["rn%d_images_digest" % nl] = images_digest(x)
        if conf:
            res["rn%d_algc" % nl] = ac.numpy().astype(np.float32)
            res["rn%d_volc" % nl] = vc.numpy().astype(np.float32)
    return res


def alg_setup(name):
    """(config, state dict, inputs, fp32 projection matrices) of gen_alg ('alg_c1') / gen_alg2 ('alg_relu_noconf')."""
    if name == "alg_c1":
        cfg = synth.alg_config(50, True)
        sd = synth.make_state_dict(spec.alg_net_spec(50, 17, True), seed=50)
        inp = synth.make_inputs(2, 4, 256, seed=1)
    else:
        cfg = synth.alg_config(18, False)
        cfg.model.heatmap_softmax = False
        cfg.model.heatmap_multiplier = 1.0
        sd = synth.make_state_dict(spec.alg_net_spec(18, 17, False), seed=51, basic_block=True)
        inp = synth.make_inputs(2, 3, 128, seed=9)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(2, 1, 1, 1)
    return cfg, sd, inp, P


def alg_truth(name, ref):
    """The fp64 algebraic forward of fixture <name>.npz, plus ``kp3_of_ref2d``: the fp64 DLT of the reference's own 2D keypoints and
    confidences (``ref``, the fp32 fixture) -- what the DLT kernel is fed in the GPU tests."""
    cfg, sd, inp, P = alg_setup(name)
    o = O.algebraic_forward(sd, cfg, inp["images"], inp["K"], inp["R"], inp["t"], dtype=F64)
    B, NV, J, h, w = o["heatmaps"].shape
    s = 4 if name == "alg_c1" else 2
    k3 = O.triangulate_batch_of_points(P, torch.from_numpy(ref["kp2"]), torch.from_numpy(ref["conf"]), dtype=F64)
    return {"kp3": o["keypoints_3d"].numpy(), "kp2": o["keypoints_2d"].numpy().astype(np.float32), "conf": o["alg_confidences"].numpy().astype(np.float32),
            "hm_sub": _sub(o["heatmaps"].reshape(B * NV, J, h, w), s).astype(np.float32), "kp3_of_ref2d": k3.numpy(),
            "sd_digest": np.array(synth.state_dict_checksum(sd)), "images_digest": images_digest(inp["images"])}


# ---- error measures (the GPU tests use the same ones) -----------------------------------------------------------------------
def max_rel(a, truth):
    """max|a - truth| / max|truth|."""
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    assert a.shape == truth.shape, (a.shape, truth.shape)
    return float(np.abs(a - truth).max() / max(float(np.abs(truth).max()), 1e-300))


def joints_rel(a, truth):
    """Joints: max |a - truth| / max(|truth|, 1 mm), element-wise."""
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    assert a.shape == truth.shape, (a.shape, truth.shape)
    return float((np.abs(a - truth) / np.maximum(np.abs(truth), 1.0)).max())


def joints_norm_rel(a, truth):
    """Joints, norm-wise: max |a - truth| / (largest |component| of the sample's joints), for (B, J, 3)."""
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float((np.abs(a - truth) / np.abs(truth).max(axis=(1, 2), keepdims=True)).max())


def err_of(key, a, truth):
    return joints_rel(a, truth) if key in JOINT_KEYS else max_rel(a, truth)


def vol_cases_cfg(tag):
    """build_vol_case's defaults with the case's own arguments."""
    _tests_dir()
    from test_oracle_golden import build_vol_case
    return build_vol_case(tag)[3]
