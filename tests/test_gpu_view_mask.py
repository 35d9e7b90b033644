"""Per-sample view masks on the GPU: the masked gather (lt_unproject_masked_fwd / lt_unproject_grid_masked_fwd), the masked algebraic tail
(lt_alg_tail_masked_fwd) and the functional ops that take ``view_mask``.  The meaning is pinned to the unmasked code: sample b with mask row m gets what
the unmasked entry gives for that sample on the views {v : m[v]} alone -- bit for bit wherever the compacted call runs the same kernel."""
import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import bf16_round, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = __import__("oracle.vol_oracle", fromlist=["x"])
synth = __import__("oracle.synth", fromlist=["x"])

AGGS = ("sum", "max", "softmax", "conf", "conf_norm")


def _case(B, NV, C, hw, V, seed, inside=True):
    """Feature maps (B,NV,C,hw,hw), projections with camera 0 inside the cube (depth <= 0 for some voxels), a rotated grid per sample, confidences."""
    g = torch.Generator().manual_seed(seed)
    K, R, t = synth.ring_cameras(NV, 96, inside=inside)
    P = torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (hw, hw))).float()[None].repeat(B, 1, 1, 1).contiguous()
    hm = torch.randn(B, NV, C, hw, hw, generator=g)
    conf = torch.rand(B, NV, C, generator=g) + 0.1
    base = torch.randn(B, 3, generator=g).numpy() * 100
    cv = torch.stack([O.coord_volume(base[b], 2500.0, V, 0.3 * b) for b in range(B)])
    return hm, P, cv, conf


def _mask(rows):
    return torch.tensor([[int(c) for c in r] for r in rows], dtype=torch.uint8)


def _unproject(hm, P, cv, conf, agg, mask=None):
    """The kernel entry itself (every aggregation code, LT_AGG_CONF_NORM included, which the functional op does not pass): channels-last in, (B,V,V,V,C) out."""
    B, NV, C, h, w = hm.shape
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    v0, v1, v2 = cv.shape[1:4]
    out = torch.empty(B, v0, v1, v2, C, dtype=hm.dtype, device=hm.device)
    cp = conf.data_ptr() if agg.startswith("conf") else None
    st = torch.cuda.current_stream().cuda_stream
    if mask is None:
        H.check(H.lib().lt_unproject_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), cp, out.data_ptr(), B, NV, C, h, w, v0, v1, v2,
                                         H.AGG[agg], st), "lt_unproject_fwd")
    else:
        H.check(H.lib().lt_unproject_masked_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), cp, mask.data_ptr(), out.data_ptr(), B, NV, C,
                                                h, w, v0, v1, v2, H.AGG[agg], st), "lt_unproject_masked_fwd")
    torch.cuda.synchronize()
    return out


def _compacted(hm, P, cv, conf, agg, mask):
    """Per sample: the unmasked entry on the valid views alone (zeros for a sample without one)."""
    outs = []
    for b in range(hm.shape[0]):
        idx = torch.nonzero(mask[b].cpu()).flatten().to(hm.device)
        if idx.numel() == 0:
            outs.append(torch.zeros(tuple(cv.shape[1:4]) + (hm.shape[2],), dtype=hm.dtype, device=hm.device))
            continue
        outs.append(_unproject(hm[b:b + 1, idx].contiguous(), P[b:b + 1, idx].contiguous(), cv[b:b + 1].contiguous(), conf[b:b + 1, idx].contiguous(), agg)[0])
    return torch.stack(outs)


def _poison(hm, mask, value):
    """The masked views' maps filled with ``value``."""
    out = hm.clone()
    out[(mask == 0).to(hm.device)] = value
    return out


GENERIC = [  # (NV, C, V, masks, aggregations)
    (4, 32, 16, ("1111", "1011", "0010"), AGGS),             # bricked volume, the float4 path
    (4, 32, 6, ("1111", "1011", "0010"), AGGS),              # linear 256-voxel chunks (216 voxels: a partial chunk)
    (4, 5, 16, ("1111", "1011", "0010"), ("softmax",)),      # C % 4 != 0: one channel per lane
    (4, 5, 6, ("1111", "1011", "0010"), ("softmax",)),
    (9, 32, 6, ("111111111", "101010101", "000000100"), AGGS),   # more than 8 views: the any-NV branch, 9 / 5 / 1 valid
]


@pytest.mark.parametrize("NV,C,V,rows,aggs", GENERIC, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_generic_gather_fp32_equals_the_compacted_call_bit_for_bit(NV, C, V, rows, aggs):
    """fp32: every sample of the masked gather equals lt_unproject_fwd on that sample's valid views, torch.equal -- and NaN in the masked views' maps
    changes no bit (they are never read)."""
    hm, P, cv, conf = [t.to(DEV) for t in _case(3, NV, C, 12, V, seed=100 + NV + C + V)]
    mask = _mask(rows).to(DEV)
    for agg in aggs:
        got = _unproject(_poison(hm, mask, 0.0), P, cv, conf, agg, mask)
        want = _compacted(hm, P, cv, conf, agg, mask)
        assert torch.isfinite(got).all(), agg
        assert torch.equal(got, want), "%s: masked gather differs from the compacted call (max |d| %g)" % (agg, float((got - want).abs().max()))
        nan = _unproject(_poison(hm, mask, float("nan")), P, cv, conf, agg, mask)
        assert torch.equal(nan, got), "%s: NaN in a masked view's map leaked" % agg


@pytest.mark.parametrize("NV,rows", [(4, ("1011", "0110", "1111")), (8, ("10110101", "11111110", "11111111"))], ids=["nv4", "nv8"])
def test_generic_gather_bf16_equals_the_compacted_call_bit_for_bit(NV, rows):
    """bf16 where the masked AND the compacted call take the generic kernel's <= 8-view branch (3, 2, 5, 7 valid views; aggregations other than
    softmax at C = 32, and softmax at C = 16, so that the 4- and 8-view calls do not go to the quad kernel): bit-identical."""
    for C, aggs in ((32, ("sum", "max", "conf", "conf_norm")), (16, ("softmax",))):
        hm, P, cv, conf = [t.to(DEV) for t in _case(3, NV, C, 12, 16, seed=200 + NV + C)]
        hm = hm.bfloat16()
        mask = _mask(rows).to(DEV)
        for agg in aggs:
            got = _unproject(_poison(hm, mask, 0.0), P, cv, conf, agg, mask)
            want = _compacted(hm, P, cv, conf, agg, mask)
            assert torch.equal(got, want), "bf16 %s C%d: masked gather differs from the compacted call" % (agg, C)
            nan = _unproject(_poison(hm, mask, float("nan")), P, cv, conf, agg, mask)
            assert torch.equal(nan, got), "bf16 %s: NaN in a masked view's map leaked" % agg


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_sample_without_a_valid_view_gets_zeros(dtype):
    """Zeros, not NaN (0 / 0 in the softmax and in conf_norm's normaliser): generic kernel in both branches and the quad kernel (bf16, softmax, 4 views)."""
    for NV, rows in ((4, ("0000", "1010", "0000")), (9, ("000000000", "111111111", "000000000"))):
        hm, P, cv, conf = [t.to(DEV) for t in _case(3, NV, 32, 12, 16, seed=300 + NV)]
        hm = _poison(hm.to(dtype), _mask(rows).to(DEV), float("nan"))
        mask = _mask(rows).to(DEV)
        for agg in AGGS:
            got = _unproject(hm, P, cv, conf, agg, mask)
            assert torch.count_nonzero(got[0]) == 0 and torch.count_nonzero(got[2]) == 0, (agg, NV)
            assert torch.isfinite(got[1]).all() and torch.count_nonzero(got[1]) > 0, (agg, NV)


def test_functional_op_takes_the_mask():
    """op.unproject_heatmaps(..., view_mask=): bool / uint8, tensor (host or device) / array; None is the unmasked path; grad is refused."""
    from mvn.utils import op
    hm, P, cv, conf = [t.to(DEV) for t in _case(3, 4, 32, 12, 16, seed=400)]
    rows = ("1111", "1011", "0010")
    mask = _mask(rows)
    want = _compacted(hm, P, cv, conf, "softmax", mask.to(DEV)).permute(0, 4, 1, 2, 3)
    for m in (mask, mask.bool(), mask.to(DEV), mask.bool().to(DEV), mask.numpy(), mask.numpy().astype(bool)):
        got = op.unproject_heatmaps(hm, P, cv, "softmax", view_mask=m)
        assert torch.equal(got, want)
    full = op.unproject_heatmaps(hm, P, cv, "conf", conf, view_mask=torch.ones(3, 4, dtype=torch.bool))
    assert torch.equal(full, op.unproject_heatmaps(hm, P, cv, "conf", conf))
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_mask=torch.ones(3, 3, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="inference only"):
        op.unproject_heatmaps(hm.clone().requires_grad_(True), P, cv, "softmax", view_mask=mask)


# ---- quad gather: bf16, C = 32, 4 or 8 views, view softmax, bricked volume -------------------------------------------------------------------------
def _grid_case(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(B, 3, generator=g) * 100).numpy().astype(np.float64)
    side = 2500.0
    pos = torch.from_numpy((base - side / 2).astype(np.float32))
    cen = torch.from_numpy(base.astype(np.float32))
    from mvn.utils import volumetric
    rot = torch.from_numpy(np.stack([volumetric.get_rotation_matrix([0, 0, 1], 0.3 * b) for b in range(B)]).astype(np.float32)).reshape(B, 9)
    step = float(np.float32(side / (V - 1)))
    return pos.to(DEV), cen.to(DEV), rot.to(DEV).contiguous(), step


def _unproject_grid(hm, P, pos, cen, rot, step, V, mask=None):
    B, NV, C, h, w = hm.shape
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    out = torch.empty(B, V, V, V, C, dtype=hm.dtype, device=hm.device)
    coords = torch.empty(B, V, V, V, 3, dtype=torch.float32, device=hm.device)
    st = torch.cuda.current_stream().cuda_stream
    if mask is None:
        H.check(H.lib().lt_unproject_grid_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                              coords.data_ptr(), None, out.data_ptr(), B, NV, C, h, w, V, H.AGG["softmax"], st), "lt_unproject_grid_fwd")
    else:
        H.check(H.lib().lt_unproject_grid_masked_fwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                                     coords.data_ptr(), None, mask.data_ptr(), out.data_ptr(), B, NV, C, h, w, V, H.AGG["softmax"], st),
                "lt_unproject_grid_masked_fwd")
    torch.cuda.synchronize()
    return out, coords


QUAD = [(3, 4, 16), (3, 8, 16), (8, 4, 16), (3, 4, 32), (8, 8, 32)]      # (B, NV, V): B = 8 pins samples to XCDs, V = 32 walks the bricks in super-blocks
PARTIAL = {4: ("1011", "0110", "0100", "1111", "1101", "0011", "1110", "1000"),
           8: ("10110101", "11111110", "00010000", "11111111", "01111111", "11000011", "10000001", "11101111")}


@pytest.mark.parametrize("B,NV,V", QUAD, ids=["B%d_NV%d_V%d" % c for c in QUAD])
def test_quad_gather_masked(B, NV, V):
    """The masked quad kernel, coordinate-tensor entry and grid entry.  All-ones mask: the bits of the unmasked quad kernel (and of lt_coord_volumes for the
    written grid).  Partial masks against the fp32 masked gather on the same bf16-rounded maps: the yardstick is the gap between the UNMASKED quad kernel and
    the fp32 kernel on all views of the same inputs, the gate twice that (dropping views changes the softmax's conditioning).  NaN in masked maps: no bit moves."""
    hm, P, cv, conf = [t.to(DEV) for t in _case(B, NV, 32, 24, V, seed=500 + B + NV + V, inside=(V == 16))]
    hb = hm.bfloat16()
    ones = torch.ones(B, NV, dtype=torch.uint8, device=DEV)
    mask = _mask(PARTIAL[NV][:B]).to(DEV)
    pos, cen, rot, step = _grid_case(B, V, seed=600 + B)
    cvg = torch.empty(B, V, V, V, 3, dtype=torch.float32, device=DEV)
    H.check(H.lib().lt_coord_volumes(pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, B, V, 0, cvg.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "lt_coord_volumes")
    # all-ones mask == no mask, both entries
    plain = _unproject(hb, P, cv, conf, "softmax")
    assert torch.equal(_unproject(hb, P, cv, conf, "softmax", ones), plain)
    plain_g, coords_g = _unproject_grid(hb, P, pos, cen, rot, step, V)
    ones_g, coords_m = _unproject_grid(hb, P, pos, cen, rot, step, V, ones)
    assert torch.equal(ones_g, plain_g) and torch.equal(coords_m, coords_g) and torch.equal(coords_m, cvg)
    # partial masks
    hb32 = hb.float()
    yard = float((plain.float() - _unproject(hb32, P, cv, conf, "softmax")).abs().max())
    got = _unproject(_poison(hb, mask, 0.0), P, cv, conf, "softmax", mask)
    ref = _unproject(hb32, P, cv, conf, "softmax", mask)
    gap = float((got.float() - ref).abs().max())
    record("view_mask/quad/B%d_NV%d_V%d" % (B, NV, V), {"unmasked_quad_vs_fp32_max_abs": yard, "masked_quad_vs_fp32_masked_max_abs": gap, "gate": 2 * yard})
    print("quad B%d NV%d V%d: unmasked quad vs fp32 %.4e, masked quad vs fp32 masked %.4e (gate %.4e)" % (B, NV, V, yard, gap, 2 * yard))
    assert torch.isfinite(got.float()).all()
    assert gap <= 2 * yard, "masked quad kernel: %.4e from the fp32 masked gather, gate 2 x %.4e" % (gap, yard)
    nan = _unproject(_poison(hb, mask, float("nan")), P, cv, conf, "softmax", mask)
    assert torch.equal(nan, got), "NaN in a masked view's map leaked"
    got_g, coords_p = _unproject_grid(_poison(hb, mask, float("nan")), P, pos, cen, rot, step, V, mask)
    ref_g = _unproject(hb32, P, cvg, conf, "softmax", mask)
    assert torch.equal(coords_p, cvg)
    gap_g = float((got_g.float() - ref_g).abs().max())
    assert gap_g <= 2 * yard, "masked quad kernel (grid entry): %.4e from the fp32 masked gather, gate 2 x %.4e" % (gap_g, yard)


# ---- algebraic tail ---------------------------------------------------------------------------------------------------------------------------------
def _tail(kp_hm, raw, ld, proj, sx, sy, B, NV, J, mask=None):
    k2 = torch.empty(B, NV, J, 2, dtype=torch.float32, device=DEV)
    cf = torch.empty(B, NV, J, dtype=torch.float32, device=DEV)
    k3 = torch.empty(B, J, 3, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rp = None if raw is None else raw.data_ptr()
    if mask is None:
        H.check(H.lib().lt_alg_tail_fwd(kp_hm.data_ptr(), rp, ld, proj.data_ptr(), sx, sy, k2.data_ptr(), cf.data_ptr(), k3.data_ptr(), B, NV, J, st), "lt_alg_tail_fwd")
    else:
        H.check(H.lib().lt_alg_tail_masked_fwd(kp_hm.data_ptr(), rp, ld, proj.data_ptr(), sx, sy, mask.data_ptr(), k2.data_ptr(), cf.data_ptr(), k3.data_ptr(),
                                               B, NV, J, st), "lt_alg_tail_masked_fwd")
    torch.cuda.synchronize()
    return k2, cf, k3


def _tail_case(NV, with_conf, seed):
    B, J, h, w, Hh, W = 3, 17, 32, 32, 128, 128
    g = torch.Generator().manual_seed(seed)
    K, R, t = synth.ring_cameras(NV, Hh)
    Pn = K @ np.concatenate([R, t], -1)
    X = torch.randn(B, J, 3, generator=g).double() * 300
    Xh = torch.cat([X, torch.ones(B, J, 1, dtype=torch.float64)], -1)
    px = torch.einsum("vrk,bjk->bvjr", torch.from_numpy(Pn), Xh)
    kp_img = px[..., :2] / px[..., 2:] + torch.randn(B, NV, J, 2, generator=g).double() * 0.5
    kp_hm = (kp_img * torch.tensor([w / W, h / Hh], dtype=torch.float64)).float().to(DEV).contiguous()
    proj = torch.from_numpy(Pn).float()[None].repeat(B, 1, 1, 1).to(DEV).contiguous()
    ld = 24          # the head's padded row, as in the plan
    raw = (torch.rand(B, NV, ld, generator=g) * 0.8 + 0.1).to(DEV).contiguous() if with_conf else None
    return B, J, kp_hm, proj, raw, ld, W / w, Hh / h


@pytest.mark.parametrize("with_conf", [True, False], ids=["conf", "uniform"])
@pytest.mark.parametrize("NV,rows", [(4, ("1111", "1011", "0101")), (6, ("111111", "101101", "010010"))], ids=["nv4", "nv6"])
def test_alg_tail_masked_equals_the_compacted_tail_bit_for_bit(NV, rows, with_conf):
    """keypoints_3d and the valid views' confidences / keypoints_2d: the bits of lt_alg_tail_fwd on the compacted views (the k-th valid view in partial
    k % 4 of the view sum, the valid views' rows alone in the DLT); masked confidences exactly 0; the masked views' keypoints are NaN and do not leak."""
    B, J, kp_hm, proj, raw, ld, sx, sy = _tail_case(NV, with_conf, seed=700 + NV)
    mask = _mask(rows).to(DEV)
    kp_nan = kp_hm.clone()
    kp_nan[mask == 0] = float("nan")
    k2, cf, k3 = _tail(kp_nan, raw, ld, proj, sx, sy, B, NV, J, mask)
    assert torch.isfinite(k3).all()
    for b in range(B):
        idx = torch.nonzero(mask[b]).flatten()
        n = idx.numel()
        c2, cc, c3 = _tail(kp_hm[b:b + 1, idx].contiguous(), None if raw is None else raw[b:b + 1, idx].contiguous(), ld, proj[b:b + 1, idx].contiguous(), sx, sy,
                           1, n, J)
        assert torch.equal(k3[b], c3[0]), "sample %d: joints differ from the compacted tail" % b
        assert torch.equal(cf[b, idx], cc[0]) and torch.equal(k2[b, idx], c2[0]), b
        off = torch.nonzero(mask[b] == 0).flatten()
        assert torch.count_nonzero(cf[b, off]) == 0
    full = _tail(kp_hm, raw, ld, proj, sx, sy, B, NV, J, torch.ones(B, NV, dtype=torch.uint8, device=DEV))
    plain = _tail(kp_hm, raw, ld, proj, sx, sy, B, NV, J)
    assert all(torch.equal(a, b_) for a, b_ in zip(full, plain)), "all-ones mask differs from lt_alg_tail_fwd"


def test_alg_tail_masked_with_fewer_than_two_views_gives_nan_joints():
    B, J, kp_hm, proj, raw, ld, sx, sy = _tail_case(4, True, seed=711)
    mask = _mask(("1111", "0100", "0000")).to(DEV)
    _, cf, k3 = _tail(kp_hm, raw, ld, proj, sx, sy, B, 4, J, mask)
    assert torch.isfinite(k3[0]).all() and torch.isnan(k3[1]).all() and torch.isnan(k3[2]).all()
    assert torch.count_nonzero(cf[2]) == 0


def test_triangulate_batch_of_points_takes_the_mask():
    """multiview.triangulate_batch_of_points(..., view_mask=): each sample is the DLT of its valid views, bit for bit; NaN points and matrices of masked views
    do not leak; fewer than two valid views and inputs that require grad are refused."""
    from mvn.utils import multiview
    B, J, kp_hm, proj, raw, ld, sx, sy = _tail_case(4, True, seed=720)
    pts = (kp_hm.reshape(B, 4, J, 2) * torch.tensor([sx, sy], device=DEV)).contiguous()
    conf = raw[:, :, :J].contiguous()
    mask = _mask(("1111", "1011", "0101"))
    md = mask.to(DEV)
    pn, Pn = pts.clone(), proj.clone()
    pn[md == 0] = float("nan")
    Pn[md == 0] = float("nan")
    for c in (conf, None):
        got = multiview.triangulate_batch_of_points(Pn, pn, c, view_mask=mask)
        for b in range(B):
            idx = torch.nonzero(md[b]).flatten()
            want = multiview.triangulate_batch_of_points(proj[b:b + 1, idx], pts[b:b + 1, idx], None if c is None else c[b:b + 1, idx])
            assert torch.equal(got[b], want[0]), b
    with pytest.raises(ValueError, match="sample 1 has 1 valid view"):
        multiview.triangulate_batch_of_points(proj, pts, conf, view_mask=_mask(("1111", "0100", "0101")))
    with pytest.raises(NotImplementedError, match="inference only"):
        multiview.triangulate_batch_of_points(proj, pts.clone().requires_grad_(True), conf, view_mask=mask)
