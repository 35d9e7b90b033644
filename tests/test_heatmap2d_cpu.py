"""CPU: the 2D heatmap targets, the heatmap loss and the soft-argmax backward with a gradient on both outputs -- their numpy fp64 statements
(mvn.utils.multiview.render_gaussians_2d / heatmap_mse_2d / softargmax2d_backward) against the reference's render (tests/golden/heatmap2d_ops.npz,
tools/make_golden_heatmap2d.py), central differences and torch fp64 autograd; the CPU paths of op.gaussian_2d_pdf / render_points_as_2d_gaussians; and
the three new C entry points' signatures and argument checks, which answer without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from heatmap2d_cases import SHAPES, amplitude, loss_inputs, op_cases, softargmax_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lt_render_gaussians_2d", "lt_heatmap_mse_fwd", "lt_softargmax2d_bwd_full")


def _fixture_covers_the_shapes_and_both_normalisers(cases):
    assert sorted({c["shape"] for c in cases}) == sorted(SHAPES)
    assert {(c["shape"], c["normalize"]) for c in cases} == {(s, n) for s in SHAPES for n in (False, True)}
    for c in cases:
        h, w = c["shape"]
        p, s = c["points"], c["sigmas"]
        assert (s[:, 0] != s[:, 1]).sum() >= 4 and s.min() == 0.5 and s.max() == 3.5          # anisotropic, 0.5 .. 3.5
        assert bool((c["f64"][5] == 0).all()) and p[5, 0] > 1e3          # far outside: the target underflows to 0
    # outside the map on each of the four sides, over the cases
    assert any(c["points"][2, 0] < 0 for c in cases) and any(c["points"][2, 0] > c["shape"][1] - 1 for c in cases)
    assert any(c["points"][3, 1] < 0 for c in cases) and any(c["points"][3, 1] > c["shape"][0] - 1 for c in cases)


def test_numpy_statement_matches_the_reference_render(golden_dir):
    """Within the reference's OWN stored fp32 error (relative to the Gaussian's peak) of its fp32 render, both normalisers -- the sigma_x * sigma_x
    normaliser with anisotropic sigmas included -- and equal to the reference's fp64 evaluation to fp64 rounding."""
    from mvn.utils.multiview import render_gaussians_2d
    _fixture_covers_the_shapes_and_both_normalisers(op_cases(golden_dir))
    for c in op_cases(golden_dir):
        g = render_gaussians_2d(c["points"], c["sigmas"], c["shape"], c["normalize"])
        amp = amplitude(c["sigmas"], c["normalize"])
        e64 = np.abs(g - c["f64"]).max(axis=(1, 2)) / amp
        e32 = np.abs(g - c["ref32"].astype(np.float64)).max(axis=(1, 2)) / amp
        assert (e64 <= 1e-14).all(), e64
        assert (e32 <= c["ref_err"] + 1e-14).all(), (e32, c["ref_err"])
        if c["normalize"]:          # sigma_x twice: the peak of an on-pixel keypoint is 1 / (2 pi sx^2), whatever sy is
            assert abs(g[0, 2, 3] * 2 * np.pi * float(c["sigmas"][0, 0]) ** 2 - 1) < 1e-12
            assert abs(g[0, 2, 3] * 2 * np.pi * float(c["sigmas"][0, 0]) * float(c["sigmas"][0, 1]) - 1) > 0.5


def test_op_cpu_paths_match_the_fixture(golden_dir):
    from mvn.utils import op
    for c in op_cases(golden_dir):
        h, w = c["shape"]
        pts, sg = torch.from_numpy(c["points"].copy()), torch.from_numpy(c["sigmas"].copy())
        out = op.render_points_as_2d_gaussians(pts, sg, (h, w), normalize=c["normalize"])
        assert out.shape == (6, h, w) and out.dtype == torch.float32
        amp = amplitude(c["sigmas"], c["normalize"])
        e = np.abs(out.numpy().astype(np.float64) - c["f64"]).max(axis=(1, 2)) / amp
        assert (e <= np.maximum(2 * c["ref_err"], 1e-7)).all(), (e, c["ref_err"])          # the same fp32 expression: the reference's error, give or take a rounding
        yy, xx = np.mgrid[0:h, 0:w]
        grid = torch.from_numpy(np.stack([xx, yy], -1).reshape(-1, 2).astype(np.float32))
        one = op.gaussian_2d_pdf(grid.double(), pts[1:2].double().expand(h * w, 2), sg[1:2].double().expand(h * w, 2), normalize=c["normalize"])
        assert np.abs(one.numpy().reshape(h, w) - c["f64"][1]).max() <= 1e-14 * amp[1]


@pytest.mark.parametrize("normalize", [False, True])
def test_loss_gradient_matches_central_differences(golden_dir, normalize):
    from mvn.utils.multiview import heatmap_mse_2d
    c = [k for k in op_cases(golden_dir) if k["shape"] == (5, 7) and k["normalize"] == normalize][0]
    pred, pts, sg, val = loss_inputs(c, 6, "mixed")
    val = val.copy(); val[2] = 0.5          # validity is a weight: the formulas hold for any value
    pred = pred.astype(np.float64)
    loss, terms, grad = heatmap_mse_2d(pred, pts, sg, val, normalize)
    assert np.isfinite(loss) and abs(loss - terms.sum() / (35 * max(1.0, val.sum()))) < 1e-15
    eps = 1e-6 * np.abs(pred).max()
    rs = np.random.RandomState(3)
    for _ in range(40):
        i, y, x = rs.randint(6), rs.randint(5), rs.randint(7)
        d = np.zeros_like(pred); d[i, y, x] = eps
        num = (heatmap_mse_2d(pred + d, pts, sg, val, normalize)[0] - heatmap_mse_2d(pred - d, pts, sg, val, normalize)[0]) / (2 * eps)
        assert abs(num - grad[i, y, x]) <= 1e-7 * np.abs(grad).max(), (i, y, x, num, grad[i, y, x])


def test_invalid_joints_with_nan_keypoints_and_all_invalid(golden_dir):
    from mvn.utils.multiview import heatmap_mse_2d
    c = op_cases(golden_dir)[2]
    pred, pts, sg, val = loss_inputs(c, 6, "mixed")
    assert np.isnan(pts[1]).all() and np.isnan(pts[4]).all()
    loss, terms, grad = heatmap_mse_2d(pred, pts, sg, val, c["normalize"])
    assert np.isfinite(loss) and loss > 0 and np.isfinite(grad).all()
    assert terms[1] == 0 and terms[4] == 0 and (grad[[1, 4]] == 0).all() and (np.abs(grad[[0, 2, 3, 5]]).max(axis=(1, 2)) > 0).all()
    pred, pts, sg, val = loss_inputs(c, 6, "zero")
    loss, terms, grad = heatmap_mse_2d(pred, pts, sg, val, c["normalize"])
    assert loss == 0.0 and (terms == 0).all() and (grad == 0).all()          # denominator clamped to 1: 0 / (h w), not 0 / 0
    # validity None is all ones
    pred, pts, sg, _ = loss_inputs(c, 6, None)
    a, b = heatmap_mse_2d(pred, pts, sg, None, c["normalize"]), heatmap_mse_2d(pred, pts, sg, np.ones(6), c["normalize"])
    assert a[0] == b[0] and (a[2] == b[2]).all()


@pytest.mark.parametrize("softmax", [True, False], ids=["softmax", "relu"])
@pytest.mark.parametrize("which", ["both", "coords_only", "probs_only"])
def test_softargmax_backward_statement_matches_fp64_autograd(softmax, which):
    """The formula of lt_softargmax2d_bwd_full in numpy fp64 against torch fp64 autograd through the reference's expression of integrate_tensor_2d."""
    from mvn.utils.multiview import softargmax2d_backward
    from oracle import vol_oracle as O
    mult = 1.7
    for h, w in SHAPES:
        hm, gc, gp = softargmax_inputs(h, w, 3, softmax)
        x = torch.from_numpy(hm).double()[None].requires_grad_(True)
        coords, probs = O.integrate_tensor_2d(x * mult, softmax, dtype=torch.float64)
        L = 0
        if which != "probs_only":
            L = L + (coords * torch.from_numpy(gc).double()[None]).sum()
        if which != "coords_only":
            L = L + (probs * torch.from_numpy(gp).double()[None]).sum()
        L.backward()
        ours = softargmax2d_backward(probs.detach().numpy()[0], coords.detach().numpy()[0], None if which == "probs_only" else gc,
                                     None if which == "coords_only" else gp, mult=mult, softmax=softmax)
        ref = x.grad.numpy()[0]
        assert np.abs(ours - ref).max() <= 1e-12 * np.abs(ref).max(), (h, w, np.abs(ours - ref).max(), np.abs(ref).max())


def test_new_symbols_are_declared_and_exported():
    import lt_hip as H
    hdr = open(os.path.join(ROOT, "include", "lt_hip.h")).read()
    lib = H.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        res, args = H.SIGNATURES[name]
        assert res is C.c_int and getattr(lib, name).argtypes == args
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(args), (name, decl)


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    """NULL pointers, sizes < 1 and h * w >= 2^31 are LT_ERR_INVALID with a message, before any device work (this machine may have no GPU)."""
    import lt_hip as H
    lib = H.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def refused(rc, word):
        msg = (lib.lt_last_error() or b"").decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.lt_render_gaussians_2d(None, p, p, 1, 2, 2, 1, None), "lt_render_gaussians_2d")
    refused(lib.lt_render_gaussians_2d(p, None, p, 1, 2, 2, 1, None), "null")
    refused(lib.lt_render_gaussians_2d(p, p, None, 1, 2, 2, 1, None), "null")
    for n, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2)):
        refused(lib.lt_render_gaussians_2d(p, p, p, n, h, w, 1, None), "bad shape")
    refused(lib.lt_render_gaussians_2d(p, p, p, 1, 1 << 16, 1 << 15, 1, None), "int32")
    for bad in range(4):          # pred, points, sigmas, terms; validity and grad_pred may be NULL
        a = [p, p, p, None, 0, p, None, 1, 2, 2, None]
        a[bad if bad < 3 else 5] = None
        refused(lib.lt_heatmap_mse_fwd(*a), "null")
    for NJ, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):
        refused(lib.lt_heatmap_mse_fwd(p, p, p, None, 0, p, None, NJ, h, w, None), "bad shape")
    refused(lib.lt_heatmap_mse_fwd(p, p, p, None, 0, p, None, 1, 1 << 16, 1 << 15, None), "int32")
    for bad in (0, 1, 6):          # probs, coords, grad_heatmaps
        a = [p, p, p, p, 1.0, 1, p, 1, 2, 2, None]
        a[bad] = None
        refused(lib.lt_softargmax2d_bwd_full(*a), "null")
    refused(lib.lt_softargmax2d_bwd_full(p, p, None, None, 1.0, 1, p, 1, 2, 2, None), "both null")
    for NJ, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):
        refused(lib.lt_softargmax2d_bwd_full(p, p, p, p, 1.0, 1, p, NJ, h, w, None), "bad shape")
    refused(lib.lt_softargmax2d_bwd_full(p, p, p, p, 1.0, 1, p, 1, 1 << 16, 1 << 15, None), "int32")


def test_heatmap_loss_module_refuses_cpu_tensors_and_bad_shapes():
    from mvn.models.loss import HeatmapMSELoss
    crit = HeatmapMSELoss(sigma=2.0, normalize=False)
    assert crit.sigma == 2.0 and crit.normalize is False
    with pytest.raises(RuntimeError, match="GPU"):
        crit(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2), torch.ones(2, 3, 1))
