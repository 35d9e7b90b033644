"""Shared by tests/test_heatmap2d_cpu.py and tests/test_gpu_heatmap2d_kernels.py: the op cases of tests/golden/heatmap2d_ops.npz
(tools/make_golden_heatmap2d.py) and the inputs the loss / soft-argmax-backward tests build on them."""
import os

import numpy as np

SHAPES = [(5, 7), (8, 12), (33, 24), (32, 33)]          # under one wave, scalar | vector, < 256 px | vector, 792 px (4 backward workgroups) | odd w, > 256 px
_CACHE = {}


def op_cases(golden_dir):
    """[{points (6,2), sigmas (6,2), shape (h,w), normalize, ref32, f64, ref_err (6,)}] -- loaded once per session, never modified."""
    if "ops" not in _CACHE:
        G = np.load(os.path.join(golden_dir, "heatmap2d_ops.npz"))
        cases = []
        for k in range(int(G["n_cases"])):
            p = "c%d/" % k
            c = {key: G[p + key] for key in ("points", "sigmas", "ref32", "f64", "ref_err")}
            c["shape"], c["normalize"] = tuple(int(v) for v in G[p + "shape"]), bool(int(G[p + "normalize"]))
            for a in c.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cases.append(c)
        _CACHE["ops"] = cases
    return _CACHE["ops"]


def amplitude(sigmas, normalize):
    """The Gaussian's peak value 1 / norm per heatmap (norm = 2 pi sx sx, or 1): what the render's error is measured against."""
    s = np.asarray(sigmas, dtype=np.float64)
    return 1.0 / (2 * np.pi * s[:, 0] * s[:, 0]) if normalize else np.ones(len(s))


def loss_inputs(case, NJ, validity, seed=0):
    """pred (NJ,h,w) fp32 -- the target plus noise of a tenth of its amplitude, so that pred - G neither vanishes nor drowns G --, points, sigmas (the
    case's first NJ rows; NJ == 1: the between-pixels row) and validity (NJ,) fp32 or None: 'mixed' (rows 1 and 4 off), 'zero', 'ones', None (NULL).
    Rows with validity 0 carry NaN points and sigmas."""
    from mvn.utils.multiview import render_gaussians_2d
    h, w = case["shape"]
    rows = [1] if NJ == 1 else list(range(NJ))
    pts, sg = case["points"][rows].copy(), case["sigmas"][rows].copy()
    rs = np.random.RandomState(100 + seed)
    amp = amplitude(sg, case["normalize"])[:, None, None]
    pred = (render_gaussians_2d(pts, sg, (h, w), case["normalize"]) + amp * 0.1 * rs.randn(NJ, h, w)).astype(np.float32)
    if validity is None:
        val = None
    elif validity == "zero":
        val = np.zeros(NJ, dtype=np.float32)
    elif validity == "ones":
        val = np.ones(NJ, dtype=np.float32)
    else:
        val = np.ones(NJ, dtype=np.float32)
        val[[i for i in (1, 4) if i < NJ]] = 0
        if NJ == 1:
            val[0] = 1
    if val is not None:
        pts[val == 0] = np.nan
        sg[val == 0] = np.nan
    return pred, pts, sg, val


def softargmax_inputs(h, w, NJ, softmax, seed=0):
    """Heatmap logits (NJ,h,w) fp32 with a bump and noise (ReLU mode: about half the pixels off), gradients on the coordinates (NJ,2) and on the returned
    heatmaps (NJ,h,w)."""
    rs = np.random.RandomState(200 + seed)
    y, x = np.mgrid[0:h, 0:w]
    hm = np.stack([2.0 * np.exp(-((x - rs.uniform(0, w)) ** 2 + (y - rs.uniform(0, h)) ** 2) / 8.0) + rs.randn(h, w) for _ in range(NJ)]).astype(np.float32)
    if not softmax:
        hm -= 0.2
    return hm, rs.randn(NJ, 2).astype(np.float32), rs.randn(NJ, h, w).astype(np.float32)
