"""GPU (-m gpu): every branch of the 2D heatmap kernels -- lt_render_gaussians_2d, lt_heatmap_mse_fwd (csrc/heatmap2d.hip) and
lt_softargmax2d_bwd_full (csrc/softargmax.hip) -- through the raw C ABI, against their numpy fp64 statements (mvn.utils.multiview) and fp64 autograd.

Shapes (heatmap2d_cases.SHAPES): (5, 7) fewer pixels than one wave, scalar path; (8, 12) vector path under 256 pixels; (33, 24) vector path, 792 pixels
(no multiple of 256, four backward workgroups); (32, 33) odd width over 256 pixels.  NJ 1 or 6.  Keypoints on a pixel centre, between pixels, outside
the map on every side, far outside (the target underflows to 0); anisotropic sigmas 0.5 .. 3.5; validity mixed, all zero, all one, NULL.

Gates.  Render: |ours - fp64| <= 1e-6 x the Gaussian's peak 1 / norm -- an fp32 exp's error relative to the peak is at most max_t(t e^-t) = 0.37
times a few units of 2^-23, plus the roundings of the two factors' product; the reference's own fp32 error on the same inputs is stored in the fixture
and recorded next to ours.  Loss terms and gradient: 1e-5 of the loss / of the largest gradient entry, against fp64.  The soft-argmax backward: 1e-5 of
the largest entry of fp64 autograd.  Everything else is bit for bit."""
import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from heatmap2d_cases import SHAPES, amplitude, loss_inputs, op_cases, softargmax_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def _cases(golden_dir, shape):
    return [c for c in op_cases(golden_dir) if c["shape"] == shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_render_vs_fp64_and_the_reference(golden_dir, shape):
    from mvn.utils import op
    from mvn.utils.multiview import render_gaussians_2d
    h, w = shape
    for c in _cases(golden_dir, shape):
        for rows in (list(range(6)), [1]):
            pts, sg = _dev(c["points"][rows]), _dev(c["sigmas"][rows])
            out = torch.full((len(rows), h, w), NAN, device=DEV)
            H.check(H.lib().lt_render_gaussians_2d(pts.data_ptr(), sg.data_ptr(), out.data_ptr(), len(rows), h, w, int(c["normalize"]), _st()), "lt_render_gaussians_2d")
            again = torch.full((len(rows), h, w), NAN, device=DEV)
            H.check(H.lib().lt_render_gaussians_2d(pts.data_ptr(), sg.data_ptr(), again.data_ptr(), len(rows), h, w, int(c["normalize"]), _st()), "lt_render_gaussians_2d")
            assert torch.equal(out, again), "two launches differ"
            truth = c["f64"][rows]
            assert np.abs(render_gaussians_2d(c["points"][rows], c["sigmas"][rows], shape, c["normalize"]) - truth).max() <= 1e-14 * amplitude(c["sigmas"][rows], c["normalize"]).max()
            err = np.abs(out.cpu().numpy().astype(np.float64) - truth).max(axis=(1, 2)) / amplitude(c["sigmas"][rows], c["normalize"])
            ref_err = c["ref_err"][rows]
            tag = "heatmap2d/render %dx%d normalize=%d n=%d" % (h, w, c["normalize"], len(rows))
            print(tag, "ours / peak:", " ".join("%.1e" % e for e in err), "| reference fp32:", " ".join("%.1e" % e for e in ref_err))
            record(tag + " max|d| / peak", {"err": float(err.max()), "tol": 1e-6, "reference_fp32_err": float(ref_err.max()),
                                            "over_four_times_the_reference": bool((err > 4 * np.maximum(ref_err, 2.0 ** -24)).any())})
            assert (err <= 1e-6).all(), (tag, err)
            if len(rows) == 6:
                assert bool((out[5] == 0).all())          # far outside: exactly 0
        # the public op on GPU tensors is that launch
        pts, sg = _dev(c["points"]), _dev(c["sigmas"])
        pub = op.render_points_as_2d_gaussians(pts, sg, shape, normalize=c["normalize"])
        ref = torch.empty_like(pub)
        H.check(H.lib().lt_render_gaussians_2d(pts.data_ptr(), sg.data_ptr(), ref.data_ptr(), 6, h, w, int(c["normalize"]), _st()), "lt_render_gaussians_2d")
        assert torch.equal(pub, ref)


def _mse(pred, pts, sg, val, normalize, with_grad, misalign=False):
    NJ, h, w = pred.shape
    p, q, s, v = _dev(pred), _dev(pts), _dev(sg), _dev(val)
    if misalign:          # a prediction whose rows are not 16-byte aligned takes the scalar path whatever w is
        buf = torch.empty(p.numel() + 1, dtype=torch.float32, device=DEV)
        buf[1:].copy_(p.reshape(-1))
        p = buf[1:].view(NJ, h, w)
        assert p.data_ptr() % 16 != 0
    terms = torch.full((NJ,), NAN, device=DEV)
    grad = torch.full((NJ, h, w), NAN, device=DEV) if with_grad else None
    H.check(H.lib().lt_heatmap_mse_fwd(p.data_ptr(), q.data_ptr(), s.data_ptr(), H.ptr(v), int(normalize), terms.data_ptr(), H.ptr(grad), NJ, h, w, _st()), "lt_heatmap_mse_fwd")
    return terms, grad


@pytest.mark.parametrize("validity", ["mixed", "zero", "ones", None], ids=["mixed", "all_zero", "all_one", "null"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_heatmap_mse_vs_fp64(golden_dir, shape, validity):
    from mvn.utils.multiview import heatmap_mse_2d
    h, w = shape
    for c in _cases(golden_dir, shape):
        for NJ in (6, 1):
            pred, pts, sg, val = loss_inputs(c, NJ, validity)
            loss64, terms64, grad64 = heatmap_mse_2d(pred, pts, sg, val, c["normalize"])
            terms, grad = _mse(pred, pts, sg, val, c["normalize"], True)
            t2, g2 = _mse(pred, pts, sg, val, c["normalize"], True)
            assert torch.equal(terms, t2) and torch.equal(grad, g2), "two launches differ"
            t3, _ = _mse(pred, pts, sg, val, c["normalize"], False)
            assert torch.equal(terms, t3), "grad_pred = NULL changes the terms"
            tag = "heatmap2d/mse %dx%d normalize=%d NJ=%d validity=%s" % (h, w, c["normalize"], NJ, validity)
            tn, gn = terms.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
            assert np.isfinite(tn).all() and np.isfinite(gn).all(), tag
            off = np.zeros(NJ, dtype=bool) if val is None else val == 0
            assert (tn[off] == 0).all() and (gn[off] == 0).all(), tag + ": a row with validity 0 is not exactly zero"
            den = h * w * max(1.0, NJ if val is None else float(val.sum()))
            if validity == "zero":          # loss 0 with the denominator clamped to 1: nothing to be relative to, everything exactly 0
                assert (tn == 0).all() and (gn == 0).all() and loss64 == 0 and (grad64 == 0).all()
                continue
            tsum, gmax = terms64.sum(), np.abs(grad64).max()
            e_t, e_l, e_g = np.abs(tn - terms64).max() / tsum, abs(tn.sum() / den - loss64) / loss64, np.abs(gn - grad64).max() / gmax
            record(tag, {"terms_err": float(e_t), "loss_err": float(e_l), "grad_err": float(e_g), "tol": 1e-5})
            assert e_t <= 1e-5 and e_l <= 1e-5 and e_g <= 1e-5, (tag, e_t, e_l, e_g)
            # the scalar path on the same numbers (rows not 16-byte aligned): same gates
            ts, gs = _mse(pred, pts, sg, val, c["normalize"], True, misalign=True)
            e_ts, e_gs = np.abs(ts.cpu().numpy() - terms64).max() / tsum, np.abs(gs.cpu().numpy() - grad64).max() / gmax
            assert e_ts <= 1e-5 and e_gs <= 1e-5, (tag, "scalar path", e_ts, e_gs)
            if w % 4:
                assert torch.equal(ts, terms) and torch.equal(gs, grad)          # an odd width was on the scalar path already


def test_heatmap_loss_module_vs_fp64(golden_dir):
    """loss.HeatmapMSELoss: value and gradient against the fp64 statement, leading dimensions, (…, J, 1) and (…, J) validity, per-joint sigmas, the scalar
    sigma, NaN keypoints of invalid joints, an upstream factor."""
    from mvn.models.loss import HeatmapMSELoss
    from mvn.utils.multiview import heatmap_mse_2d
    c = [k for k in _cases(golden_dir, (33, 24)) if k["normalize"]][0]
    pred, pts, sg, val = loss_inputs(c, 6, "mixed")
    h, w = c["shape"]
    for lead in ((6,), (2, 3)):
        for vshape in (lead + (1,), lead):
            x = _dev(pred).reshape(lead + (h, w)).requires_grad_(True)
            L = HeatmapMSELoss(normalize=True)(x, _dev(pts).reshape(lead + (2,)), _dev(val).reshape(vshape), sigmas=_dev(sg).reshape(lead + (2,)))
            (3.0 * L).backward()
            l64, _, g64 = heatmap_mse_2d(pred, pts, sg, val, True)
            assert abs(float(L.detach()) - l64) <= 1e-5 * l64
            assert np.abs(x.grad.cpu().numpy().reshape(6, h, w) - 3.0 * g64).max() <= 1e-5 * 3.0 * np.abs(g64).max()
            assert bool((x.grad.reshape(6, h, w)[[1, 4]] == 0).all())
    x = _dev(pred).requires_grad_(True)
    L = HeatmapMSELoss(sigma=1.5, normalize=False)(x, _dev(pts), _dev(val))
    L.backward()
    l64, _, g64 = heatmap_mse_2d(pred, pts, np.full((6, 2), 1.5), val, False)
    assert abs(float(L.detach()) - l64) <= 1e-5 * l64 and np.abs(x.grad.cpu().numpy() - g64).max() <= 1e-5 * np.abs(g64).max()
    with torch.no_grad():
        assert abs(float(HeatmapMSELoss(sigma=1.5)(_dev(pred), _dev(pts), _dev(val))) - l64) <= 1e-5 * l64
    with pytest.raises(ValueError, match="keypoints_2d_gt"):
        HeatmapMSELoss()(_dev(pred), _dev(pts)[:5], _dev(val))


def _bwd(entry, probs, coords, gc, gp, mult, softmax):
    NJ, h, w = probs.shape
    out = torch.full((NJ, h, w), NAN, device=DEV)
    if entry == "old":
        H.check(H.lib().lt_softargmax2d_bwd(probs.data_ptr(), coords.data_ptr(), gc.data_ptr(), mult, int(softmax), out.data_ptr(), NJ, h, w, _st()), "lt_softargmax2d_bwd")
    else:
        H.check(H.lib().lt_softargmax2d_bwd_full(probs.data_ptr(), coords.data_ptr(), H.ptr(gc), H.ptr(gp), mult, int(softmax), out.data_ptr(), NJ, h, w, _st()),
                "lt_softargmax2d_bwd_full")
    return out


@pytest.mark.parametrize("softmax", [True, False], ids=["softmax", "relu"])
@pytest.mark.parametrize("NJ", [1, 6])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_softargmax2d_bwd_full(shape, NJ, softmax):
    from oracle import vol_oracle as O
    h, w = shape
    mult = 1.7
    hm, gc, gp = softargmax_inputs(h, w, NJ, softmax)
    hd, gcd, gpd = _dev(hm), _dev(gc), _dev(gp)
    coords, probs = torch.empty(NJ, 2, device=DEV), torch.empty(NJ, h, w, device=DEV)
    H.check(H.lib().lt_softargmax2d_fwd(hd.data_ptr(), mult, int(softmax), coords.data_ptr(), probs.data_ptr(), NJ, h, w, _st()), "lt_softargmax2d_fwd")
    tag = "heatmap2d/softargmax2d_bwd_full %dx%d NJ=%d %s" % (h, w, NJ, "softmax" if softmax else "relu")
    # grad_probs = NULL: the old entry's bits
    old = _bwd("old", probs, coords, gcd, None, mult, softmax)
    assert torch.equal(_bwd("full", probs, coords, gcd, None, mult, softmax), old), tag + ": grad_probs = NULL differs from lt_softargmax2d_bwd"
    # grad_coords = NULL: the bits of a zero coordinate gradient
    a, b = _bwd("full", probs, coords, None, gpd, mult, softmax), _bwd("full", probs, coords, torch.zeros_like(gcd), gpd, mult, softmax)
    assert torch.equal(a, b), tag + ": grad_coords = NULL differs from zero coordinate gradients"
    both = _bwd("full", probs, coords, gcd, gpd, mult, softmax)
    assert torch.equal(both, _bwd("full", probs, coords, gcd, gpd, mult, softmax)), tag + ": two launches differ"
    for name, ours, use_c, use_p in (("both", both, True, True), ("heatmaps only", a, False, True)):
        x = torch.from_numpy(hm).double()[None].requires_grad_(True)
        c64, p64 = O.integrate_tensor_2d(x * mult, softmax, dtype=torch.float64)
        L = (p64 * torch.from_numpy(gp).double()[None]).sum()
        if use_c:
            L = L + (c64 * torch.from_numpy(gc).double()[None]).sum()
        L.backward()
        ref = x.grad[0].numpy()
        e = np.abs(ours.cpu().numpy() - ref).max() / np.abs(ref).max()
        record(tag + " " + name, {"err": float(e), "tol": 1e-5})
        assert e <= 1e-5, (tag, name, e)


@pytest.mark.parametrize("softmax", [True, False], ids=["softmax", "relu"])
def test_integrate_tensor_2d_autograd(softmax):
    """op.integrate_tensor_2d under autograd: a loss on the coordinates alone takes the old entry (today's gradient, bit for bit); a loss on the heatmaps
    alone, and on both, matches fp64 autograd."""
    from mvn.utils import op
    from oracle import vol_oracle as O
    h, w, N, J = 33, 24, 2, 3
    hm, gc, gp = softargmax_inputs(h, w, N * J, softmax, seed=5)
    hm, gc, gp = hm.reshape(N, J, h, w), gc.reshape(N, J, 2), gp.reshape(N, J, h, w)
    seen = []
    lib = H.lib()

    class Spy:          # which entry the node's backward takes
        def __getattr__(self, name):
            if name.startswith("lt_softargmax2d_bwd"):
                seen.append(name)
            return getattr(lib, name)

    def run(use_c, use_p, stats=False):
        x = _dev(hm).requires_grad_(True)
        out = op.integrate_tensor_2d_with_stats(x, softmax) if stats else op.integrate_tensor_2d(x, softmax)
        c, p = out[0], out[1]
        assert c.requires_grad and p.requires_grad
        L = 0
        if use_c:
            L = L + (c * _dev(gc)).sum()
        if use_p:
            L = L + (p * _dev(gp)).sum()
        real = H.lib
        H.lib = lambda: Spy()
        try:
            L.backward()
        finally:
            H.lib = real
        return c.detach(), p.detach(), x.grad

    c, p, g = run(True, False)
    assert seen == ["lt_softargmax2d_bwd"], seen
    today = _bwd("old", p.reshape(N * J, h, w), c.reshape(N * J, 2), _dev(gc).reshape(N * J, 2), None, 1.0, softmax).reshape(N, J, h, w)
    assert torch.equal(g, today)
    assert torch.equal(run(True, False, stats=True)[2], today)
    for use_c, use_p in ((False, True), (True, True)):
        del seen[:]
        g = run(use_c, use_p)[2]
        assert seen == ["lt_softargmax2d_bwd_full"], seen
        x = torch.from_numpy(hm).double().requires_grad_(True)
        c64, p64 = O.integrate_tensor_2d(x, softmax, dtype=torch.float64)
        L = (p64 * torch.from_numpy(gp).double()).sum()
        if use_c:
            L = L + (c64 * torch.from_numpy(gc).double()).sum()
        L.backward()
        e = float((g.cpu().double() - x.grad).abs().max() / x.grad.abs().max())
        assert e <= 1e-5, (use_c, use_p, e)
