"""Generates tests/golden/train_step_view_mask.npz by running the REFERENCE on the CPU where the reference tree is available (the same loader as
oracle/make_golden.py).  Writes only that file:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_view_mask.py

One full training step of the reference's VolumetricTriangulationNet on a batch with MISSING VIEWS: what ``batch["view_mask"]`` means in training.  The
recipe is tools/make_golden_train_many_views.py's -- its ``run`` is used as it is: MAE on keypoints * 0.1 + 0.01 * VolumetricCELoss, Adam with the three
learning-rate groups, the reference run under other thread counts and under images x (1 +- 1e-6) for the per-parameter self-noise, re-seeding until the
reference passes its own gate -- with ResNet-18, 3 samples, 4 views, 128 x 128 images, 32^3 voxels, view softmax and the masks 1111 / 1011 / 0101.

The reference has no mask.  Its backbone runs on ALL images (the masked views' included: its training-mode BatchNorm statistics are taken over every
image, as this project's masked step takes them), and for the duration of the run its ``op.unproject_heatmaps`` is wrapped to call itself sample by
sample on the sample's valid views alone -- so the volume of a sample, and everything autograd derives behind it, is the reference's own on those views;
a masked view's features receive no gradient from the volume.  Same keys as train_step_nv10.npz, plus ``view_mask`` (B, NV) uint8.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_train_many_views as MV  # noqa: E402
from oracle import ref_loader, truth  # noqa: E402

OUT = os.path.join(MV.GOLD, "train_step_view_mask.npz")
CASE = dict(nl=18, B=3, NV=4, H=128, V=32, seed=21)
VIEW_MASK = np.array([[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 1]], dtype=np.uint8)
VOL_STRIDE, FEAT_STRIDE = 4, 4


def masked_unproject(unproject, view_mask):
    """The reference's unproject_heatmaps, called per sample on the sample's valid views alone."""
    def wrapped(heatmaps, proj_matricies, coord_volumes, volume_aggregation_method="sum", vol_confidences=None):
        vols = []
        for b in range(heatmaps.shape[0]):
            idx = np.nonzero(view_mask[b])[0].tolist()
            conf = None if vol_confidences is None else vol_confidences[b:b + 1, idx]
            vols.append(unproject(heatmaps[b:b + 1, idx], proj_matricies[b:b + 1, idx], coord_volumes[b:b + 1],
                                  volume_aggregation_method=volume_aggregation_method, vol_confidences=conf))
        return torch.cat(vols, dim=0)
    return wrapped


def main():
    torch.manual_seed(0)
    mvn = ref_loader.load()
    MV.VOL_STRIDE, MV.FEAT_STRIDE = VOL_STRIDE, FEAT_STRIDE
    plain = mvn.utils.op.unproject_heatmaps
    mvn.utils.op.unproject_heatmaps = masked_unproject(plain, VIEW_MASK)
    try:
        case = dict(CASE)
        while True:
            ok, out = MV.run(mvn, case)
            if ok:
                break
            case["seed"] += 1000
    finally:
        mvn.utils.op.unproject_heatmaps = plain
    out["view_mask"] = VIEW_MASK
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s: %d bytes" % (OUT, size))
    assert size < truth.MAX_BYTES, size


if __name__ == "__main__":
    main()
