"""The test infrastructure of the indexed unprojection backward (tests/unproject_bwd_indexed_ref.py), checked without a GPU: indexed_ref_backward against
fp64 autograd through the restated forward (unproject_ref.ref_unproject) on the inputs gathered by frame_of; the conditions the GPU tests' gates rest on (the
lattice sums stay exact when a frame adds three cuboids; no 'max' winner of the Gaussian gate cases differs between fp32 and fp64); the opt-in defaults and
the refusals that need no device; the workspace query."""
import ctypes as C

import pytest
import torch

import exact
import lt_hip as H
import unproject_bwd_indexed_ref as X
import unproject_bwd_ref as R
import unproject_ref as U


@pytest.fixture(autouse=True)
def _gather_path(monkeypatch):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)


def _autograd_indexed(hm, proj, conf, cv, G, agg, frame_of, mask=None):
    idx = torch.tensor(frame_of)
    h64 = hm.double().requires_grad_(True)
    c64 = conf.double().requires_grad_(True) if agg.startswith("conf") else None
    out, _ = U.ref_unproject(h64[idx], proj[idx], cv, agg, None if c64 is None else c64[idx], mask=None if mask is None else mask[idx].bool())
    P, Cc = cv.shape[0], hm.shape[2]
    (out.reshape(P, -1, Cc) * G.double().reshape(P, Cc, -1).permute(0, 2, 1)).sum().backward()
    return h64.grad, (None if c64 is None else c64.grad)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_indexed_reference_equals_fp64_autograd_of_the_indexed_composition(masked):
    """F = 3 frames (one without a cuboid), P = 5 cuboids, every aggregation: 1e-12 of max|ref|, the empty frame exactly zero."""
    frame_of = [2, 0, 2, 2, 0]
    hm, proj, conf, cv, G = X.gaussian_case(4, C=8, hw=(12, 14), vs=(5, 4, 6), F=3, P=5, seed=11)
    mask = torch.tensor([[1, 0, 1, 1], [1, 1, 1, 1], [0, 1, 1, 0]], dtype=torch.uint8) if masked else None
    for agg in X.AGGS:
        gf, gc = X.indexed_ref_backward(hm, proj, cv, G, agg, frame_of, conf, mask)
        af, ac = _autograd_indexed(hm, proj, conf, cv, G, agg, frame_of, mask)
        assert float(af.abs().max()) > 0
        assert float((gf - af).abs().max()) <= 1e-12 * float(af.abs().max()), agg
        assert float(gf[1].abs().max()) == 0
        if masked:
            assert float(gf[mask == 0].abs().max()) == 0
        if agg.startswith("conf"):
            assert float((gc - ac).abs().max()) <= 1e-12 * float(ac.abs().max()), agg
            assert float(gc[1].abs().max()) == 0
        else:
            assert gc is None


def test_one_cuboid_per_frame_is_the_unindexed_reference():
    hm, proj, conf, cv, G = X.gaussian_case(4, C=8, hw=(12, 14), vs=(5, 4, 6), F=3, P=3, seed=12)
    for agg in X.AGGS:
        gf, gc = X.indexed_ref_backward(hm, proj, cv, G, agg, [0, 1, 2], conf)
        rf, rc = R.ref_backward(hm, proj, cv, G, agg, conf)[:2]
        assert float((gf - rf).abs().max()) <= 1e-13 * float(rf.abs().max()), agg
        assert gc is None or float((gc - rc).abs().max()) <= 1e-13 * float(rc.abs().max()), agg


@pytest.mark.parametrize("C", [4, 8, 32])
@pytest.mark.parametrize("vs", [(8, 4, 12), (5, 6, 7)], ids=["8x4x12", "ragged"])
def test_lattice_sums_over_a_frames_cuboids_stay_exact(C, vs):
    """The bit-exact GPU test adds up to three cuboids into one frame: the per-pixel bound of the SUM (the per-cuboid magnitudes added over frame_of) still
    satisfies the exactness condition on the grid of the contributions, for the features and for the confidence gradient."""
    frames, cv, G = X.lattice_frames_case(4, C, vs, 900 + C)
    for agg in X.EXACT_AGGS:
        mag_f = torch.zeros(X.LATTICE_F, *frames.hm.shape[1:], dtype=torch.float64)
        mag_c = torch.zeros(X.LATTICE_F, *frames.conf.shape[1:], dtype=torch.float64)
        grid = float("inf")
        for p, f in enumerate(X.LATTICE_FRAME_OF):
            _, _, mag, rec = R.ref_backward(frames.hm[f:f + 1], frames.P[f:f + 1], cv[p:p + 1], G[p:p + 1], agg, frames.conf[f:f + 1])
            mag_f[f] += mag.feats[0]
            grid = min(grid, exact.grid_of(rec.taps.wt) * exact.grid_of(rec.dx))
            if agg == "conf":
                mag_c[f] += mag.conf[0]
                exact.assert_exact("conf sums", float(mag_c.max()), exact.grid_of(rec.vals))
        exact.assert_exact("lattice %s C=%d: per-pixel sum over a frame's cuboids" % (agg, C), float(mag_f.max()), grid)
        assert float(mag_f[1].abs().max()) == 0 and float(mag_f[2].abs().max()) > 0


@pytest.mark.parametrize("NV", [4, 10])
def test_gate_cases_have_no_max_winner_that_flips_between_fp32_and_fp64(NV):
    hm, proj, conf, cv, G = X.gaussian_case(NV)
    assert X.max_winners_agree(hm, proj, conf, cv, G, X.GATE_FRAME_OF)
    # and camera 0 sees part of every grid at depth <= 0 (the rule that zeroes the sample is on trial)
    z = torch.cat([cv.reshape(len(cv), -1, 3).double(), torch.ones(len(cv), cv[0][..., 0].numel(), 1, dtype=torch.float64)], 2) @ proj[0, 0, 2].double()
    assert bool(((z <= 0).sum(1) > 0).all()) and bool(((z > 0).sum(1) > 0).all())


def test_opt_in_defaults_and_refusals_without_a_device():
    from mvn.models.triangulation import VolumetricTriangulationNet
    from mvn.utils import op
    from oracle import synth
    assert VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").multi_cuboid_training is False
    hm = torch.zeros(2, 2, 4, 8, 8, requires_grad=True)
    args = (hm, torch.zeros(2, 2, 3, 4), torch.zeros(3, 4, 4, 4, 3), "sum")
    with pytest.raises(NotImplementedError, match="no indexed backward"):
        op.unproject_heatmaps(*args, frame_index=[0, 1, 1])
    with pytest.raises(NotImplementedError, match="no masked backward"):          # a view_mask follows its own rule
        op.unproject_heatmaps(*args, frame_index=[0, 1, 1], indexed_backward=True, view_mask=torch.ones(2, 2))
    with pytest.raises(RuntimeError, match="must live on the GPU"):                # opted in: the launch path, which has no CPU form
        op.unproject_heatmaps(*args, frame_index=[0, 1, 1], indexed_backward=True)


def _entry_rc(frame_of=1, F=2, P=3, Cc=8, NV=2, ws=1 << 20):
    """lt_unproject_indexed_bwd with non-null dummy addresses: every refusal below is raised before anything is dereferenced or launched."""
    p = 4096
    return H.lib().lt_unproject_indexed_bwd(H.LT_F32, p, p, p, None, None, p if frame_of else None, p, p, None, F, P, NV, Cc, 8, 8, 4, 4, 4, H.AGG["sum"], p, ws, None)


def test_entry_refusals_need_no_device(monkeypatch):
    lib = H.lib()
    assert H.SIGNATURES["lt_unproject_indexed_bwd"] == (C.c_int, [H.i32] + [H.vp] * 9 + [H.i32] * 10 + [H.vp, C.c_size_t, H.vp])
    assert _entry_rc(frame_of=0) == -1 and b"frame_of" in lib.lt_last_error()
    assert _entry_rc(P=0) == -1 and _entry_rc(F=0) == -1
    assert _entry_rc(Cc=12) == -2 and b"power of two" in lib.lt_last_error()
    assert _entry_rc(NV=33) == -2
    assert _entry_rc(ws=64) == -1 and b"workspace" in lib.lt_last_error()
    monkeypatch.setenv("LT_UNPROJ_BWD_ATOMICS", "1")
    assert _entry_rc() == -2 and b"LT_UNPROJ_BWD_ATOMICS" in lib.lt_last_error()


def test_workspace_query_grows_with_the_cuboids_and_is_zero_off_the_gather(monkeypatch):
    lib = H.lib()
    q = lambda P, Cc=32, NV=4, v=(16, 16, 16): lib.lt_unproject_indexed_bwd_workspace(P, NV, Cc, *v)
    assert 0 < q(1) < q(2) < q(5) and q(5) <= 5 * q(1)
    assert q(5) - q(4) >= 4 * 16 ** 3 * 32 * 4                       # a cuboid's share holds its dxs (NV * nvox * C fp32)
    assert q(1) == lib.lt_unproject_bwd_workspace(1, 4, 32, 16, 16, 16)          # one cuboid: the unindexed entry's blocks
    assert q(0) == 0 and q(3, Cc=12) == 0 and q(3, Cc=128) == 0
    # the chunked sizes the GPU tests hand over: the partials of all cuboids and 1, 2, .. cuboids' shares; the last is the query itself
    sizes = [X.ws_bytes(lib, 5, 4, 32, (16, 16, 16), k) for k in (1, 2, 5)]
    assert sizes[0] < sizes[1] < sizes[2] == q(5)
    from mvn.utils import op
    assert [op.indexed_bwd_workspace(5, 4, 32, 16, 16, 16, chunk=k) for k in (1, 2, 5)] == sizes
    assert op.indexed_bwd_workspace(5, 4, 32, 16, 16, 16, cap=sizes[1] + 100) == sizes[1] and op.indexed_bwd_workspace(5, 4, 32, 16, 16, 16, cap=0) == sizes[0]
    monkeypatch.setenv("LT_UNPROJ_BWD_ATOMICS", "1")
    assert q(5) == 0
