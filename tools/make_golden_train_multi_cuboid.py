"""Generates tests/golden/train_step_multi_cuboid.npz by running the REFERENCE on the CPU where the reference tree is available (the same loader as
oracle/make_golden.py).  Writes only that file:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_multi_cuboid.py

One full training step of the reference's VolumetricTriangulationNet with SEVERAL CUBOIDS PER FRAME: what ``batch["cuboid_frame"]`` means in training.  The
recipe is tools/make_golden_train_many_views.py's -- its ``run`` is used as it is: MAE on keypoints * 0.1 + 0.01 * VolumetricCELoss, Adam with the three
learning-rate groups, the reference run under other thread counts and under images x (1 +- 1e-6) for the per-parameter self-noise, re-seeding until the
reference passes its own gate -- with ResNet-18, 4 views, 128 x 128 images, 32^3 voxels, view softmax, F = 2 frames and P = 5 cuboids, frame_of =
(0, 1, 1, 0, 1).

The reference has no frame index: it gets one sample per cuboid, the cuboid's frame repeated (``run`` builds a batch of P samples; sample p stands for
cuboid p, and the images of frame f are those of the first sample that names it, ``frame_rep``).  For the duration of the run its ``backbone`` is wrapped so
that the real backbone runs on the F distinct frames only and its outputs are expanded with index_select by frame_of -- training-mode BatchNorm statistics
are then over the F frames and autograd sums the per-cuboid gradients into them, which is what this project's multi-cuboid step computes.  Same keys as
train_step_nv10.npz (the per-sample entries have P rows), plus ``frame_of`` (P,) and ``frame_rep`` (F,) int32.

Re-seeding: ``run`` keeps a seed when two further reference runs pass the test's gate (1e-3 + 4 x noise per parameter).  Here BatchNorm's statistics are
over F * NV = 8 images, the fewest of all the training fixtures, and the stored noise of a parameter is the larger of TWO draws, so a seed that the reference
itself passes at 0.8 x the gate leaves no room for a third draw of the same scatter (a product's fp32 step is one).  This generator therefore keeps a seed
only where the reference stays within OWN_GATE_MARGIN = 0.5 of its own gate (read from ``run``'s report line); the criterion sees reference runs only.
"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_train_many_views as MV  # noqa: E402
from oracle import ref_loader, truth  # noqa: E402

OUT = os.path.join(MV.GOLD, "train_step_multi_cuboid.npz")
FRAME_OF = np.array([0, 1, 1, 0, 1], dtype=np.int32)
FRAME_REP = np.array([int(np.nonzero(FRAME_OF == f)[0][0]) for f in range(int(FRAME_OF.max()) + 1)], dtype=np.int32)          # (0, 1)
CASE = dict(nl=18, B=len(FRAME_OF), NV=4, H=128, V=32, seed=31)
VOL_STRIDE, FEAT_STRIDE = 4, 4
OWN_GATE_MARGIN = 0.5


def frames_once(net_cls, frame_of, frame_rep):
    """The reference's net with its backbone called on the distinct frames only: the (P * NV) images it is handed are the frames repeated per cuboid; the
    wrapped forward picks the F frames, runs the real backbone on them and expands every output back to the P cuboids by frame_of."""
    idx, rep = torch.from_numpy(frame_of.astype(np.int64)), torch.from_numpy(frame_rep.astype(np.int64))
    P, F = len(frame_of), len(frame_rep)

    class FramesOnce(net_cls):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            inner = self.backbone.forward

            def forward(images):
                NV = images.shape[0] // P
                x = images.view(P, NV, *images.shape[1:]).index_select(0, rep).reshape(F * NV, *images.shape[1:])
                outs = inner(x)
                return tuple(None if o is None else o.view(F, NV, *o.shape[1:]).index_select(0, idx).reshape(P * NV, *o.shape[1:]) for o in outs)
            self.backbone.forward = forward
    return FramesOnce


def main():
    torch.manual_seed(0)
    mvn = ref_loader.load()
    MV.VOL_STRIDE, MV.FEAT_STRIDE = VOL_STRIDE, FEAT_STRIDE
    plain = mvn.models.triangulation.VolumetricTriangulationNet
    mvn.models.triangulation.VolumetricTriangulationNet = frames_once(plain, FRAME_OF, FRAME_REP)
    try:
        case = dict(CASE)
        while True:
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                ok, out = MV.run(mvn, case)
            print(log.getvalue(), end="")
            own = re.search(r"worst parameter gradient ([0-9.]+) x gate .*keypoints ([0-9.]+) x gate", log.getvalue())
            if ok and max(float(own.group(1)), float(own.group(2))) <= OWN_GATE_MARGIN:
                break
            case["seed"] += 1000
    finally:
        mvn.models.triangulation.VolumetricTriangulationNet = plain
    out["frame_of"], out["frame_rep"] = FRAME_OF, FRAME_REP
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s: %d bytes" % (OUT, size))
    assert size < truth.MAX_BYTES, size


if __name__ == "__main__":
    main()
