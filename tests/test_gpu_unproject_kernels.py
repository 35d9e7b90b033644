"""GPU (-m gpu): every branch of the unprojection forward (csrc/unproject.hip) -- unproject_kernel<T, CH, SMALL_NV, MASKED>, the eight
unproject_qn_kernel<NVL, GRID, MASKED>, brick_of() in both orders, both sample-to-workgroup maps and unproject_dispatch() -- through the four C entry
points, against the fp64 statement of the operation in tests/unproject_ref.py (itself pinned to the oracle by tests/test_unproject_ref_cpu.py).

Every case id names the branch it enters and the case ASSERTS from unproject_plan() that it does, before it compares numbers.  The output is NaN before
every call and must be finite after it: every voxel is written.  Inputs are finite; only the map of a view that is masked out of a call may hold NaN.

Gates.  fp32: max|d| <= 1e-5 max|ref| against fp64 (the gate of test_unproject_vs_reference_golden).  bf16, against fp64 on the bf16-rounded maps:
max|d| <= 1e-2 max|ref| with gpu_util.check's rms bound, AND per element |d| <= 2^-8 |ref| + 4 yard: 2^-8 is the worst relative error of one rounding to
nearest bf16 (8 significant bits), i.e. the store itself; yard is the largest absolute error of the FP32 kernel against the same reference on the same
rounded maps, measured in the case, and 4 is the allowance for v_rcp_f32 / v_exp_f32 in place of IEEE division and expf.  The achieved fraction of every gate
is recorded in the suite's parity report (gpu_util.record)."""
import numpy as np
import pytest
import torch

import lt_hip as H
import unproject_ref as U
from gpu_util import bf16_round, check, record
from oracle import synth
from oracle import vol_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


# ---- the four entry points ---------------------------------------------------------------------------------------------------------------------------
def _fwd(hm, P, cv, agg, conf=None, mask=None):
    """lt_unproject_fwd / lt_unproject_masked_fwd.  hm (B,NV,C,h,w) on the device in the kernel's type -> (B,v0,v1,v2,C)."""
    B, NV, C, h, w = hm.shape
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    v0, v1, v2 = cv.shape[1:4]
    out = torch.full((B, v0, v1, v2, C), NAN, dtype=hm.dtype, device=DEV)
    cp = conf.data_ptr() if agg.startswith("conf") else None
    if mask is None:
        H.check(H.lib().lt_unproject_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), cp, out.data_ptr(), B, NV, C, h, w, v0, v1, v2,
                                         H.AGG[agg], H.cur_stream()), "lt_unproject_fwd")
    else:
        H.check(H.lib().lt_unproject_masked_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), cp, mask.data_ptr(), out.data_ptr(), B, NV,
                                                C, h, w, v0, v1, v2, H.AGG[agg], H.cur_stream()), "lt_unproject_masked_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "%s: a voxel was not written, or not finite" % agg
    return out


def _fwd_grid(hm, P, grid, V, cmu, agg, conf=None, mask=None):
    """lt_unproject_grid_fwd / lt_unproject_grid_masked_fwd -> (volume, written coordinates)."""
    B, NV, C, h, w = hm.shape
    pos, cen, rot, step = grid
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    out = torch.full((B, V, V, V, C), NAN, dtype=hm.dtype, device=DEV)
    coords = torch.full((B, V, V, V, 3), NAN, dtype=torch.float32, device=DEV)
    cp = conf.data_ptr() if agg.startswith("conf") else None
    if mask is None:
        H.check(H.lib().lt_unproject_grid_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, int(cmu),
                                              coords.data_ptr(), cp, out.data_ptr(), B, NV, C, h, w, V, H.AGG[agg], H.cur_stream()), "lt_unproject_grid_fwd")
    else:
        H.check(H.lib().lt_unproject_grid_masked_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step,
                                                     int(cmu), coords.data_ptr(), cp, mask.data_ptr(), out.data_ptr(), B, NV, C, h, w, V, H.AGG[agg],
                                                     H.cur_stream()), "lt_unproject_grid_masked_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(coords).all()), "%s: a voxel or a coordinate was not written" % agg
    return out, coords


def _grid(B, V, seed, thetas):
    """The cuboid description of lt_coord_volumes / the grid entries (rotated about z), and the grid lt_coord_volumes writes for it."""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(B, 3, generator=g) * 100).numpy().astype(np.float64)
    side = 2500.0
    pos = torch.from_numpy((base - side / 2).astype(np.float32)).to(DEV)
    cen = torch.from_numpy(base.astype(np.float32)).to(DEV)
    rot = torch.from_numpy(np.stack([O.rotation_matrix((0, 0, 1), th) for th in thetas]).astype(np.float32)).reshape(B, 9).to(DEV).contiguous()
    return pos, cen, rot, float(np.float32(side / (V - 1)))


def _coord_volumes(grid, B, V, cmu):
    pos, cen, rot, step = grid
    cv = torch.full((B, V, V, V, 3), NAN, dtype=torch.float32, device=DEV)
    H.check(H.lib().lt_coord_volumes(pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, B, V, int(cmu), cv.data_ptr(), H.cur_stream()), "lt_coord_volumes")
    torch.cuda.synchronize()
    return cv


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def _cameras(B, NV, h, w, inside=True):
    K, R, t = synth.ring_cameras(NV, 96, inside=inside)
    return torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (h, w))).float()[None].repeat(B, 1, 1, 1).contiguous()


def _maps(B, NV, C, h, w, seed):
    """randn maps and confidences"""
    g = torch.Generator().manual_seed(seed)
    hm = torch.randn(B, NV, C, h, w, generator=g)
    return hm, torch.rand(B, NV, C, generator=g) + 0.1


def _coords(B, vs, seed):
    """A rotated cuboid grid per sample (its middle v0 x v1 x v2 voxels), or -- v0 = v1 = 1 -- an arbitrary point set."""
    g = torch.Generator().manual_seed(seed)
    if vs[0] == 1 and vs[1] == 1:
        return (torch.randn(B, 1, 1, vs[2], 3, generator=g) * 600).contiguous()
    base = torch.randn(B, 3, generator=g).numpy() * 100
    return torch.stack([U.box_coords(base[b], 2500.0, vs, 0.3 * b + 0.1) for b in range(B)])


def _mask(rows):
    return torch.tensor([[int(c) for c in r] for r in rows], dtype=torch.uint8)


def _poison(hm, mask, value=NAN):
    out = hm.clone()
    out[mask == 0] = value
    return out


# ---- gates -------------------------------------------------------------------------------------------------------------------------------------------
def _plan_is(plan, **expect):
    assert plan["supported"]
    for k, v in expect.items():
        assert plan[k] == v, "the case does not enter the branch its id names: %s is %r, not %r (%r)" % (k, plan[k], v, plan)


def _gate32(name, got, ref):
    """-> the largest absolute error (the yardstick of the bf16 case on the same inputs)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    check(name, got, ref, 1e-5)
    return float((got - ref).abs().max())


def _gate16(name, got, ref, yard):
    got = got.detach().double().cpu().reshape(ref.shape)
    d = (got - ref).abs()
    frac = float((d / (2.0 ** -8 * ref.abs() + 4 * yard)).max())
    used = float(((d - 2.0 ** -8 * ref.abs()) / yard).clamp(min=0).max()) if yard > 0 else float("inf")      # how much of the factor 4 the case needs
    record(name + " per element", {"err": frac, "tol": 1.0, "yard": yard, "yards_used": used})
    print("%s: max|d| %.3e, max|ref| %.3e, fp32 yard %.3e, per-element fraction %.3f, %.2f of the 4 yards used" % (name, float(d.max()), float(ref.abs().max()), yard,
                                                                                                               frac, used))
    check(name, got, ref, 1e-2)
    assert yard > 0 and frac <= 1.0, "%s: |d| reaches %.3f of 2^-8 |ref| + 4 yard (yard %.3e)" % (name, frac, yard)


def _both_types(name, hm, P, cv, conf, agg, run16, mask=None, samples=None, run32=None, pick=None):
    """A bf16 case: the fp32 kernel on the bf16-rounded maps against fp64 (1e-5; its error is the yardstick), then ``run16`` (the bf16 call under test).
    hm is already bf16-rounded fp32 on the host; a masked view's map is poisoned with NaN on the way to the device, it may not be read.
    samples: ref_samples() of the case when the caller has them; pick: voxel subset (indices into the flattened volume) the reference covers."""
    s = samples if samples is not None else U.ref_samples(hm, P, cv)
    C = hm.shape[2]
    ref = U.aggregate(s.vals, agg, conf, mask)
    hd = (hm if mask is None else _poison(hm, mask)).to(DEV)
    md = None if mask is None else mask.to(DEV)

    def sub(t):
        t = t.reshape(t.shape[0], -1, C)
        return t if pick is None else t[:, pick.to(t.device)]
    got32 = run32(hd) if run32 is not None else _fwd(hd, P.to(DEV), cv.to(DEV), agg, conf.to(DEV), md)
    yard = _gate32(name + " fp32 kernel", sub(got32), ref)
    got16 = run16(hd.bfloat16())
    _gate16(name, sub(got16), ref, yard)
    return got16, got32


# ---- generic kernel ------------------------------------------------------------------------------------------------------------------------------------
GENERIC = U.generic_cases()
CH_OF = {("fp32", 32): 4, ("fp32", 5): 1, ("bf16", 32): 8, ("bf16", 16): 8, ("bf16", 12): 1, ("bf16", 5): 1}       # ChVec<T, CH>
BRICKED = {"7x7x7": False, "1x1x300": False, "4x8x32": True, "8x4x16": True}


@pytest.mark.parametrize("cid", sorted(GENERIC))
def test_generic_kernel_every_channel_vector_view_count_and_chunk_layout(cid):
    """unproject_kernel<T, CH, SMALL_NV> for every (T, CH) with 1, 3, 8 (SMALL_NV), 9 and 12 views (any-NV), all five aggregations each, on linear chunks
    with a partial tail (7^3), the documented point set (1 x 1 x 300), and two non-cubic bricked volumes in raster order; maps 20 x 28 and 28 x 20;
    B = 8 and 16 pin samples to XCDs, 16 reaches the second group of eight.  An all-ones mask gives the bits of the unmasked call."""
    c = GENERIC[cid]
    ty, C, NV, vs, (h, w), B = c["ty"], c["C"], c["NV"], U.VOLUMES[c["vol"]], c["hw"], c["B"]
    seed = sum(map(ord, cid))
    hm, conf = _maps(B, NV, C, h, w, seed)
    if ty == "bf16":
        hm = bf16_round(hm)
    P, cv = _cameras(B, NV, h, w, inside=NV > 1), _coords(B, vs, seed + 1)
    s = U.ref_samples(hm, P, cv)
    Pd, cvd, cd = P.to(DEV), cv.to(DEV), conf.to(DEV)
    ones = torch.ones(B, NV, dtype=torch.uint8, device=DEV)
    for agg in U.AGGS:
        _plan_is(U.unproject_plan(DT[ty], B, NV, C, h, w, *vs, agg), kernel="generic", ch=CH_OF[(ty, C)], small_nv=NV <= 8, bricked=BRICKED[c["vol"]],
                 blocked=False, xcd_pin=B in (8, 16), chunks=-(-vs[0] * vs[1] * vs[2] // 256))
        name = "unproject_kernels/generic/%s/%s" % (cid, agg)
        if ty == "fp32":
            got = _fwd(hm.to(DEV), Pd, cvd, agg, cd)
            _gate32(name, got, U.aggregate(s.vals, agg, conf))
        else:
            got, _ = _both_types(name, hm, P, cv, conf, agg, lambda h16: _fwd(h16, Pd, cvd, agg, cd), samples=s)
        assert torch.equal(_fwd(hm.to(DEV).to(DT[ty]), Pd, cvd, agg, cd, ones), got), "%s: an all-ones mask changes bits" % name


@pytest.mark.parametrize("ty,C,NV,rows", [("fp32", 5, 9, ("101010101", "000000100", "111111110")), ("bf16", 12, 12, ("101010101011", "000000100000", "111111111110")),
                                          ("bf16", 12, 8, ("10110101", "00010000", "11111110")), ("bf16", 32, 9, ("101010101", "000000100", "111111110"))],
                         ids=["fp32_ch1_anynv", "bf16_ch1_anynv", "bf16_ch1_smallnv", "bf16_ch8_anynv"])
def test_generic_kernel_masked_against_ground_truth(ty, C, NV, rows):
    """unproject_kernel<T, CH, SMALL_NV, MASKED = true> where tests/test_gpu_view_mask.py has no ground truth: one channel per lane in both types, bf16 with
    more than 8 views; 28 x 20 maps, 8 x 4 x 16 voxels; against the reference over the valid views, NaN in the masked maps."""
    B, h, w, vs = 3, 28, 20, (8, 4, 16)
    hm, conf = _maps(B, NV, C, h, w, 900 + NV + C)
    hm = bf16_round(hm) if ty == "bf16" else hm
    P, cv, mask = _cameras(B, NV, h, w), _coords(B, vs, 901), _mask(rows)
    s = U.ref_samples(hm, P, cv)
    for agg in U.AGGS:
        _plan_is(U.unproject_plan(DT[ty], B, NV, C, h, w, *vs, agg), kernel="generic", ch=CH_OF[(ty, C)], small_nv=NV <= 8)
        name = "unproject_kernels/generic masked/%s_C%d_NV%d/%s" % (ty, C, NV, agg)
        if ty == "fp32":
            _gate32(name, _fwd(_poison(hm, mask).to(DEV), P.to(DEV), cv.to(DEV), agg, conf.to(DEV), mask.to(DEV)), U.aggregate(s.vals, agg, conf, mask))
        else:
            _both_types(name, hm, P, cv, conf, agg, lambda h16: _fwd(h16, P.to(DEV), cv.to(DEV), agg, conf.to(DEV), mask.to(DEV)), mask=mask, samples=s)


# ---- quad kernel ---------------------------------------------------------------------------------------------------------------------------------------
PARTIAL = {4: ("1011", "0110", "0100", "1101"), 8: ("10110101", "11111110", "00010000", "01111111")}


@pytest.mark.parametrize("NV,h,w", [(4, 20, 28), (4, 28, 20), (8, 20, 28), (8, 28, 20)], ids=lambda v: str(v))
def test_quad_kernel_coordinate_entry_non_square_maps_non_cubic_volume(NV, h, w):
    """unproject_qn_kernel<NVL, false, MASKED>: h != w (inv_h / inv_w, the row stride w, the view stride h w C) at 4 x 8 x 32 voxels (nk = nj = 2 in raster order,
    v0 != v1 != v2), a camera inside the volume; unmasked, all-ones mask (the same bits), partial masks against the reference over the valid views."""
    B, vs = 3, (4, 8, 32)
    hm, conf = _maps(B, NV, 32, h, w, 1000 + NV + h)
    hm = bf16_round(hm)
    P, cv = _cameras(B, NV, h, w), _coords(B, vs, 1001)
    Pd, cvd = P.to(DEV), cv.to(DEV)
    _plan_is(U.unproject_plan(torch.bfloat16, B, NV, 32, h, w, *vs, "softmax"), kernel="quad", nvl=NV // 4, bricked=True, blocked=False, chunks=4, xcd_pin=False)
    s = U.ref_samples(hm, P, cv)
    name = "unproject_kernels/quad coords/NV%d_%dx%d" % (NV, h, w)
    got, _ = _both_types(name, hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, Pd, cvd, "softmax"), samples=s)
    assert torch.equal(_fwd(hm.to(DEV).bfloat16(), Pd, cvd, "softmax", None, torch.ones(B, NV, dtype=torch.uint8, device=DEV)), got)
    mask = _mask(PARTIAL[NV][:B])
    _both_types(name + " masked", hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, Pd, cvd, "softmax", None, mask.to(DEV)), mask=mask, samples=s)


@pytest.mark.parametrize("NV,h,w,cmu", [(4, 20, 28, 0), (4, 28, 20, 1), (8, 28, 20, 0), (8, 20, 28, 1)], ids=lambda v: str(v))
def test_quad_kernel_grid_entry_non_square_maps_rotated_cuboid(NV, h, w, cmu):
    """unproject_qn_kernel<NVL, true, MASKED> at V = 16: the written coordinates are lt_coord_volumes' bit for bit (rotated cuboid, with and without the CMU axis
    permutation), the volume is within the gates of the reference on those coordinates and has the bits of the coordinate entry on them."""
    B, V = 2, 16
    hm, conf = _maps(B, NV, 32, h, w, 1100 + NV + h + cmu)
    hm = bf16_round(hm)
    P = _cameras(B, NV, h, w)
    grid = _grid(B, V, 1101, (0.0, 0.7))
    cvd = _coord_volumes(grid, B, V, cmu)
    cv, Pd = cvd.cpu(), P.to(DEV)
    _plan_is(U.unproject_plan(torch.bfloat16, B, NV, 32, h, w, V, V, V, "softmax"), kernel="quad", nvl=NV // 4, chunks=16, blocked=False)
    s = U.ref_samples(hm, P, cv)
    name = "unproject_kernels/quad grid/NV%d_%dx%d_cmu%d" % (NV, h, w, cmu)

    def run(h16, mask=None):
        out, coords = _fwd_grid(h16, Pd, grid, V, cmu, "softmax", None, mask)
        assert torch.equal(coords, cvd), "the grid entry's coordinates differ from lt_coord_volumes"
        return out
    got, _ = _both_types(name, hm, P, cv, conf, "softmax", run, samples=s)
    assert torch.equal(got, _fwd(hm.to(DEV).bfloat16(), Pd, cvd, "softmax")), "grid entry and coordinate entry differ on the same coordinates"
    assert torch.equal(run(hm.to(DEV).bfloat16(), torch.ones(B, NV, dtype=torch.uint8, device=DEV)), got)
    mask = _mask(PARTIAL[NV][:B])
    _both_types(name + " masked", hm, P, cv, conf, "softmax", lambda h16: run(h16, mask.to(DEV)), mask=mask, samples=s)


@pytest.mark.parametrize("NV,h,w,flat", [(4, 20, 28, 2), (8, 28, 20, 5)], ids=["nv4_20x28", "nv8_28x20"])
def test_probe_points_every_padding_class_in_every_view(NV, h, w, flat, monkeypatch):
    """The points of unproject_ref.probe_points (tests/test_unproject_ref_cpu.py holds them to: every border cell, corner, outside, behind the camera in every
    view -- i.e. in every lane of the quad --, pz == 0 exactly in the flat view, depths of 1e-4) as a 4 x 4 x 16k volume: quad kernel unmasked and masked;
    generic kernel in fp32 and bf16 with all five aggregations."""
    P64 = U.probe_cameras(NV, h, w, flat)
    n = U.probe_size(P64, h, w)
    pr = U.probe_points(P64, h, w, n)
    vs = (4, 4, n // 16)
    cv = pr.X.reshape(1, *vs, 3).contiguous()
    P = torch.from_numpy(P64).float()[None].contiguous()
    hm, conf = _maps(1, NV, 32, h, w, 1200 + NV)
    hm = bf16_round(hm)
    s = U.ref_samples(hm, P, cv)
    assert int((s.cls[0, flat] == U.CLS["z==0"]).sum()) >= 8
    Pd, cvd, cd = P.to(DEV), cv.to(DEV), conf.to(DEV)
    name = "unproject_kernels/probe/NV%d_%dx%d" % (NV, h, w)
    _plan_is(U.unproject_plan(torch.bfloat16, 1, NV, 32, h, w, *vs, "softmax"), kernel="quad", nvl=NV // 4, bricked=True)
    _both_types(name + "/quad", hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, Pd, cvd, "softmax"), samples=s)
    mask = _mask(PARTIAL[NV][:1])
    _both_types(name + "/quad masked", hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, Pd, cvd, "softmax", None, mask.to(DEV)), mask=mask, samples=s)
    monkeypatch.setenv("LT_UNPROJ_NO_Q4", "1")          # read per call: bf16 softmax through the generic kernel too
    for agg in U.AGGS:
        _plan_is(U.unproject_plan(torch.bfloat16, 1, NV, 32, h, w, *vs, agg), kernel="generic", ch=8, small_nv=True)
        _both_types(name + "/generic/" + agg, hm, P, cv, conf, agg, lambda h16: _fwd(h16, Pd, cvd, agg, cd), samples=s)


@pytest.mark.parametrize("vol", ["64x64x96", "32x64x96"])
def test_blocked_brick_order_with_more_than_one_super_block(vol, monkeypatch):
    """brick_of()'s blocked order where the super-block counts differ per axis (ngi, ngj, ngk = 2, 2, 3 and 1, 2, 3): the quad kernel and the fp32 generic kernel
    give the bits they give in raster order (LT_UNPROJ_RASTER=1, read per call), and a fixed random 1/16 of the voxels is within the gates of the reference."""
    vs = U.VOLUMES[vol]
    NV, h, w = 4, 20, 28
    hm, conf = _maps(1, NV, 32, h, w, 1300)
    hm = bf16_round(hm)
    P, cv = _cameras(1, NV, h, w), _coords(1, vs, 1301)
    Pd, cvd = P.to(DEV), cv.to(DEV)
    nvox = vs[0] * vs[1] * vs[2]
    pick = torch.randperm(nvox, generator=torch.Generator().manual_seed(1302))[:nvox // 16].sort()[0]
    s = U.ref_samples(hm, P, cv.reshape(1, -1, 3)[:, pick])
    _plan_is(U.unproject_plan(torch.bfloat16, 1, NV, 32, h, w, *vs, "softmax"), kernel="quad", blocked=True, chunks=nvox // 256)
    _plan_is(U.unproject_plan(torch.float32, 1, NV, 32, h, w, *vs, "softmax"), kernel="generic", ch=4, blocked=True)
    got16, got32 = _both_types("unproject_kernels/blocked/" + vol, hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, Pd, cvd, "softmax"), samples=s, pick=pick)
    monkeypatch.setenv("LT_UNPROJ_RASTER", "1")
    _plan_is(U.unproject_plan(torch.bfloat16, 1, NV, 32, h, w, *vs, "softmax"), kernel="quad", blocked=False, bricked=True)
    assert torch.equal(_fwd(hm.to(DEV).bfloat16(), Pd, cvd, "softmax"), got16), "quad kernel: blocked and raster brick order differ"
    assert torch.equal(_fwd(hm.to(DEV), Pd, cvd, "softmax"), got32), "generic kernel: blocked and raster brick order differ"


def test_quad_kernel_second_group_of_eight_samples():
    """B = 16 at V = 16 through both entries: b = xcd + 8 (j / chunks) with j / chunks == 1.  Every sample has its own maps and its own cuboid."""
    B, NV, h, w, V = 16, 4, 20, 28, 16
    hm, conf = _maps(B, NV, 32, h, w, 1400)
    hm = bf16_round(hm)
    P = _cameras(B, NV, h, w)
    grid = _grid(B, V, 1401, [0.1 * b for b in range(B)])
    cvd = _coord_volumes(grid, B, V, 0)
    cv, Pd = cvd.cpu(), P.to(DEV)
    _plan_is(U.unproject_plan(torch.bfloat16, B, NV, 32, h, w, V, V, V, "softmax"), kernel="quad", xcd_pin=True, chunks=16)
    s = U.ref_samples(hm, P, cv)
    got, _ = _both_types("unproject_kernels/quad B16/coords", hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, Pd, cvd, "softmax"), samples=s)
    out, coords = _fwd_grid(hm.to(DEV).bfloat16(), Pd, grid, V, 0, "softmax")
    assert torch.equal(coords, cvd) and torch.equal(out, got), "grid entry, B = 16"


RANGE = [("quad", "bf16", 32, 4, (4, 8, 32)), ("generic_smallnv", "bf16", 16, 8, (4, 8, 32)), ("generic_anynv", "bf16", 32, 9, (7, 7, 7)),
         ("generic_smallnv", "fp32", 32, 4, (4, 8, 32)), ("generic_anynv", "fp32", 5, 9, (7, 7, 7))]


@pytest.mark.parametrize("reach", [80.0, 100.0], ids=["80", "100"])
@pytest.mark.parametrize("kernel,ty,C,NV,vs", RANGE, ids=["%s_%s" % (r[0], r[1]) for r in RANGE])
def test_view_softmax_of_large_samples(kernel, ty, C, NV, vs, reach):
    """Maps scaled so that the samples reach +-80 and +-100, where the view softmax is a hard maximum: finite and within the gates.  e^80 = 5.5e34 is still
    an fp32 number (the largest is e^88.7), so a softmax that does not subtract the view maximum survives +-80; at +-100 its exponentials are inf or 0 and it
    writes NaN.  (Measured: the quad kernel with the maximum left at 0 passes every +-80 case.)"""
    B, h, w = 2, 20, 28
    hm, conf = _maps(B, NV, C, h, w, 1500 + NV)
    P, cv = _cameras(B, NV, h, w), _coords(B, vs, 1501)
    hm = hm * (reach / float(U.ref_samples(hm, P, cv).vals.abs().max()))          # the samples are linear in the maps: the largest |sample| is ``reach``
    hm = bf16_round(hm) if ty == "bf16" else hm
    s = U.ref_samples(hm, P, cv)
    assert reach - 1 < float(s.vals.abs().max()) < reach + 1 and float(s.vals.min()) < -0.6 * reach and float(s.vals.max()) > 0.6 * reach, \
        "the samples do not reach the range the case is about"
    plan = U.unproject_plan(DT[ty], B, NV, C, h, w, *vs, "softmax")
    _plan_is(plan, kernel="quad") if kernel == "quad" else _plan_is(plan, kernel="generic", small_nv=kernel == "generic_smallnv")
    name = "unproject_kernels/softmax range %d/%s_%s" % (reach, kernel, ty)
    if ty == "fp32":
        _gate32(name, _fwd(hm.to(DEV), P.to(DEV), cv.to(DEV), "softmax"), U.aggregate(s.vals, "softmax"))
    else:
        _both_types(name, hm, P, cv, conf, "softmax", lambda h16: _fwd(h16, P.to(DEV), cv.to(DEV), "softmax"), samples=s)


@pytest.mark.parametrize("ty,C,NV,V,agg", [("bf16", 16, 4, 16, "softmax"), ("bf16", 32, 4, 16, "sum"), ("fp32", 32, 4, 16, "softmax"), ("bf16", 32, 8, 12, "softmax")],
                         ids=["bf16_C16", "bf16_sum", "fp32", "V12"])
def test_grid_entry_outside_the_quad_predicate_is_the_two_separate_calls(ty, C, NV, V, agg):
    """lt_unproject_grid_fwd where no fused kernel exists: lt_coord_volumes + the generic kernel inside.  Coordinates bit for bit, volume torch.equal to
    lt_unproject_fwd on them (the same kernel runs); masked entry with an all-ones mask likewise."""
    B, h, w = 2, 28, 20
    hm, conf = _maps(B, NV, C, h, w, 1600 + C + V)
    hd = hm.to(DEV).to(DT[ty])
    Pd = _cameras(B, NV, h, w).to(DEV)
    grid = _grid(B, V, 1601, (0.0, 0.7))
    _plan_is(U.unproject_plan(DT[ty], B, NV, C, h, w, V, V, V, agg), kernel="generic", bricked=V == 16)
    for cmu in (0, 1):
        cvd = _coord_volumes(grid, B, V, cmu)
        want = _fwd(hd, Pd, cvd, agg, conf.to(DEV))
        for mask in (None, torch.ones(B, NV, dtype=torch.uint8, device=DEV)):
            out, coords = _fwd_grid(hd, Pd, grid, V, cmu, agg, conf.to(DEV), mask)
            assert torch.equal(coords, cvd), "coordinates differ from lt_coord_volumes"
            assert torch.equal(out, want), "volume differs from lt_unproject_fwd on the same coordinates"
