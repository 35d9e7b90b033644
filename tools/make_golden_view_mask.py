"""Generates tests/golden/view_mask_small.npz by running the REFERENCE on the CPU where the reference tree is available (the same loader as
oracle/make_golden.py).  Writes only that file:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_view_mask.py

A view mask has an exact meaning: sample b with mask row m gives what the reference gives for that sample run on the views {v : m[v]} alone.  So the
fixture runs every sample ALONE (B = 1) on its valid views only -- three samples with masks 1111, 1011, 0101 -- through

    vol_softmax/    VolumetricTriangulationNet, volume_aggregation_method softmax
    vol_conf_norm/  VolumetricTriangulationNet, conf_norm (the confidences normalised over the valid views)
    alg/            AlgebraicTriangulationNet with confidences
    cascade/        the two-stage route: the algebraic joints' pelvis centres the volumetric cuboid

ResNet-18, 17 joints, 128 x 128 images, 32^3 voxels, heatmap_multiplier 1.0 (see tools/make_golden_cascade.py), the ring cameras of oracle/synth.py.  Beside the
reference's fp32 outputs it keeps the fp64 truth (the oracle on the same subsets) and ``ref32_err/<key>``, the reference's own error against it.  Per-view
outputs are stored at full (B, NV, ...) shape with NaN in the masked views.  Re-seeds, as the cascade generator does, until the reference's own joint error is
<= 0.25e-4 in every case and the cascade's truth pelvises lie within cuboid_side / 4 of the point the cameras look at.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader, spec, synth, truth  # noqa: E402
from oracle import vol_oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "view_mask_small.npz")
NL, J, B, NV, HW, V = 18, 17, 3, 4, 128, 32
MASKS = np.array([[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 1]], dtype=np.uint8)
ALG_SEED, VOL_SEED, CONF_SEED, INPUT_SEED = 71, 72, 73, 23
STRIDE = 4
F64 = torch.float64
MAX_REF_NOISE = 0.25e-4


def setup(seeds=(ALG_SEED, VOL_SEED, CONF_SEED, INPUT_SEED)):
    """Configs, state dicts and inputs of the four cases -- tests/test_view_mask_cpu.py and tests/test_gpu_view_mask_models.py build the same from the seeds the
    fixture stores."""
    alg_seed, vol_seed, conf_seed, input_seed = [int(s) for s in seeds]
    acfg = synth.alg_config(NL, True, J)
    acfg.model.heatmap_multiplier = 1.0
    cfgs = {"alg": acfg, "vol_softmax": synth.vol_config(NL, V, "softmax", 1.0, "mpii"), "vol_conf_norm": synth.vol_config(NL, V, "conf_norm", 1.0, "mpii")}
    sds = {"alg": synth.make_state_dict(spec.alg_net_spec(NL, J, True), seed=alg_seed, basic_block=True),
           "vol_softmax": synth.make_state_dict(spec.vol_net_spec(NL, J, False), seed=vol_seed, basic_block=True),
           "vol_conf_norm": synth.make_state_dict(spec.vol_net_spec(NL, J, True), seed=conf_seed, basic_block=True)}
    inp = synth.make_inputs(B, NV, HW, seed=input_seed)
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(B, 1, 1, 1)
    return cfgs, sds, inp, P


def _scatter(x, idx, shape):
    """(1, n, ...) values of the valid views -> (NV, ...) with NaN in the masked ones."""
    out = np.full(shape, np.nan, dtype=x.dtype)
    out[idx] = x[0]
    return out


def run(mvn, seeds):
    cfgs, sds, inp, P = setup(seeds)
    Cam = mvn.utils.multiview.Camera
    T = mvn.models.triangulation
    alg = T.AlgebraicTriangulationNet(cfgs["alg"], device="cpu")
    alg.load_state_dict(sds["alg"], strict=True)
    alg.eval()
    vols = {}
    for name in ("vol_softmax", "vol_conf_norm"):
        m = T.VolumetricTriangulationNet(cfgs[name], device="cpu")
        assert list(m.state_dict().keys()) == list(sds[name].keys()), name
        m.load_state_dict(sds[name], strict=True)
        m.eval()
        vols[name] = m
    ref = {k: [] for k in ("vol_softmax/kp", "vol_conf_norm/kp", "vol_conf_norm/conf", "alg/kp3", "alg/kp2", "alg/conf", "cascade/alg_kp3", "cascade/base_points",
                           "cascade/kp")}
    tru = {k: [] for k in ref}
    vol_sub = []
    for b in range(B):
        idx = np.nonzero(MASKS[b])[0]
        n = len(idx)
        img = inp["images"][b:b + 1, idx].contiguous()
        K, R, t = inp["K"][idx], inp["R"][idx], inp["t"][idx]
        cams = [[Cam(R[v], t[v], K[v])] for v in range(n)]
        pred = inp["pred_keypoints_3d"][b:b + 1]
        with torch.no_grad():
            a3, a2, _, ac = alg(img, P[b:b + 1, idx].contiguous(), {"cameras": cams})
            outs = {name: vols[name](img, torch.zeros(1, n, 3, 4), {"cameras": cams, "pred_keypoints_3d": pred}) for name in vols}
            casc = vols["vol_softmax"](img, torch.zeros(1, n, 3, 4), {"cameras": cams, "pred_keypoints_3d": a3.numpy()})
        ta = O.algebraic_forward(sds["alg"], cfgs["alg"], img, K, R, t, dtype=F64)
        tv = {name: O.volumetric_forward(sds[name], cfgs[name], img, K, R, t, pred, dtype=F64) for name in vols}
        tc = O.volumetric_forward(sds["vol_softmax"], cfgs["vol_softmax"], img, K, R, t, ta["keypoints_3d"].numpy(), dtype=F64)
        for name in vols:
            ref[name + "/kp"].append(outs[name][0][0].numpy())
            tru[name + "/kp"].append(tv[name]["keypoints_3d"][0].numpy())
        ref["vol_conf_norm/conf"].append(_scatter(outs["vol_conf_norm"][3].numpy(), idx, (NV, 32)))
        tru["vol_conf_norm/conf"].append(_scatter(tv["vol_conf_norm"]["vol_confidences"].numpy(), idx, (NV, 32)))
        vol_sub.append(outs["vol_softmax"][2][0, :, ::STRIDE, ::STRIDE, ::STRIDE].contiguous().numpy())
        ref["alg/kp3"].append(a3[0].numpy()); tru["alg/kp3"].append(ta["keypoints_3d"][0].numpy())
        ref["alg/kp2"].append(_scatter(a2.numpy(), idx, (NV, J, 2))); tru["alg/kp2"].append(_scatter(ta["keypoints_2d"].numpy(), idx, (NV, J, 2)))
        ref["alg/conf"].append(_scatter(ac.numpy(), idx, (NV, J))); tru["alg/conf"].append(_scatter(ta["alg_confidences"].numpy(), idx, (NV, J)))
        ref["cascade/alg_kp3"].append(a3[0].numpy()); tru["cascade/alg_kp3"].append(ta["keypoints_3d"][0].numpy())
        ref["cascade/base_points"].append(casc[6][0].numpy()); tru["cascade/base_points"].append(O.base_points_from_batch(ta["keypoints_3d"].numpy(), "mpii")[0])
        ref["cascade/kp"].append(casc[0][0].numpy()); tru["cascade/kp"].append(tc["keypoints_3d"][0].numpy())
    ref = {k: np.stack(v) for k, v in ref.items()}
    tru = {k: np.stack(v) for k, v in tru.items()}
    on = MASKS.astype(bool)
    err = {}
    for k in ref:
        if k.endswith("conf"):
            err[k] = truth.max_rel(ref[k][on], tru[k][on])
        elif k.endswith("kp2"):
            err[k] = truth.joints_rel(ref[k][on], tru[k][on])
        else:
            err[k] = truth.joints_rel(ref[k], tru[k])
    side = float(cfgs["vol_softmax"].model.cuboid_side)
    dist = float(np.linalg.norm(tru["cascade/base_points"], axis=1).max())
    print("seeds %s: truth pelvises max |.| %.1f mm (limit %.1f); reference fp32 vs fp64: %s" % (list(seeds), dist, side / 4, {k: "%.2e" % v for k, v in err.items()}))
    ok = dist <= side / 4 and all(err[k] <= MAX_REF_NOISE for k in ("vol_softmax/kp", "vol_conf_norm/kp", "cascade/kp"))
    out = {}
    for k, v in ref.items():
        out[k] = v
    for k, v in tru.items():
        out["truth/" + k] = v if (k.endswith("kp") or k.endswith("kp3") or k.endswith("base_points")) else v.astype(np.float32)
    for k, v in err.items():
        out["ref32_err/" + k] = np.array(v)
    out.update({"vol_softmax/vol_sub": np.stack(vol_sub), "stride": np.array(STRIDE), "masks": MASKS, "seeds": np.array(seeds),
                "alg_sd_digest": np.array(synth.state_dict_checksum(sds["alg"])), "vol_sd_digest": np.array(synth.state_dict_checksum(sds["vol_softmax"])),
                "conf_sd_digest": np.array(synth.state_dict_checksum(sds["vol_conf_norm"])), "images_digest": truth.images_digest(inp["images"])})
    return ok, out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mvn = ref_loader.load()
    seeds = (ALG_SEED, VOL_SEED, CONF_SEED, INPUT_SEED)
    while True:
        ok, out = run(mvn, seeds)
        if ok:
            break
        seeds = tuple(s + 1000 for s in seeds)
        print("  not well posed with these weights and images, re-seeding to %s" % (seeds,))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s: %d bytes" % (OUT, size))
    assert size < truth.MAX_BYTES, size


if __name__ == "__main__":
    main()
