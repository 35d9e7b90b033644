"""Ragged view batches on the GPU: the ragged gather (lt_unproject_ragged_fwd / lt_unproject_grid_ragged_fwd), the ragged algebraic tail
(lt_alg_tail_ragged_fwd) and the functional ops that take ``view_counts``.  The yardstick is the masked entry on the inputs padded to (B, NVcap): sample b's
rows in its first n_b slots, a prefix mask, NaN maps and zero projections in the padding -- torch.equal throughout."""
import numpy as np
import pytest
import torch

import lt_hip as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = __import__("oracle.vol_oracle", fromlist=["x"])
synth = __import__("oracle.synth", fromlist=["x"])

AGGS = ("sum", "max", "softmax", "conf", "conf_norm")
NAN = float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _base(counts):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)


def _case(counts, cap, C, hw, V, seed, inside=True):
    """Ragged inputs -- maps (T,hw,hw,C) channels-last fp32, projections (T,3,4) (camera 0 of the ring inside the cube), confidences (T,C), a rotated grid per
    sample -- and their padded twins (B,cap,...): NaN maps, zero projections and NaN confidences in the slots past a sample's count."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(counts), int(sum(counts))
    K, R, t = synth.ring_cameras(cap, 96, inside=inside)
    ring = torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (hw, hw))).float()
    feats = torch.randn(T, hw, hw, C, generator=g)
    conf = torch.rand(T, C, generator=g) + 0.1
    P = torch.cat([ring[:n] for n in counts]) if T else ring[:0]
    base = torch.randn(B, 3, generator=g).numpy() * 100
    cv = torch.stack([O.coord_volume(base[b], 2500.0, V, 0.3 * b) for b in range(B)])
    fp = torch.full((B, cap, hw, hw, C), NAN)
    Pp = torch.zeros(B, cap, 3, 4)
    cp = torch.full((B, cap, C), NAN)
    r = 0
    for b, n in enumerate(counts):
        fp[b, :n], Pp[b, :n], cp[b, :n] = feats[r:r + n], P[r:r + n], conf[r:r + n]
        r += n
    mask = torch.tensor([[1] * n + [0] * (cap - n) for n in counts], dtype=torch.uint8)
    return [x.to(DEV).contiguous() for x in (feats, P, conf, cv, fp, Pp, cp, mask)]


def _ragged(feats, P, cv, conf, agg, counts, cap, view_base=None):
    T, h, w, C = feats.shape
    B, v0, v1, v2 = cv.shape[:4]
    out = torch.empty(B, v0, v1, v2, C, dtype=feats.dtype, device=DEV)
    vb = _base(counts) if view_base is None else view_base
    H.check(H.lib().lt_unproject_ragged_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if agg.startswith("conf") else None,
                                            vb.data_ptr(), out.data_ptr(), B, T, cap, C, h, w, v0, v1, v2, H.AGG[agg], _st()), "lt_unproject_ragged_fwd")
    torch.cuda.synchronize()
    return out


def _padded(fp, Pp, cv, cp, agg, mask=None):
    """lt_unproject_masked_fwd (mask) or lt_unproject_fwd (None) on the (B, cap, ...) tensors."""
    B, NV, h, w, C = fp.shape
    v0, v1, v2 = cv.shape[1:4]
    out = torch.empty(B, v0, v1, v2, C, dtype=fp.dtype, device=DEV)
    c = cp.data_ptr() if agg.startswith("conf") else None
    if mask is None:
        H.check(H.lib().lt_unproject_fwd(H.dtype_code(fp.dtype), fp.data_ptr(), Pp.data_ptr(), cv.data_ptr(), c, out.data_ptr(), B, NV, C, h, w, v0, v1, v2, H.AGG[agg],
                                         _st()), "lt_unproject_fwd")
    else:
        H.check(H.lib().lt_unproject_masked_fwd(H.dtype_code(fp.dtype), fp.data_ptr(), Pp.data_ptr(), cv.data_ptr(), c, mask.data_ptr(), out.data_ptr(), B, NV, C, h, w,
                                                v0, v1, v2, H.AGG[agg], _st()), "lt_unproject_masked_fwd")
    torch.cuda.synchronize()
    return out


COUNTS = {4: [4, 1, 3], 8: [8, 5, 2], 32: [9, 5, 1]}
GENERIC = [(32, 16, AGGS), (32, 6, AGGS), (5, 16, ("softmax",))]     # (C, V, aggregations): bricked / a partial linear chunk / one channel per lane


@pytest.mark.parametrize("cap", [4, 8, 32], ids=["cap4", "cap8", "cap32"])
@pytest.mark.parametrize("C,V,aggs", GENERIC, ids=["C32_V16", "C32_V6", "C5_V16"])
def test_generic_gather_fp32_equals_the_masked_entry_on_padded_inputs(cap, C, V, aggs):
    counts = COUNTS[cap]
    feats, P, conf, cv, fp, Pp, cp, mask = _case(counts, cap, C, 12, V, seed=100 + cap + C + V)
    for agg in aggs:
        got = _ragged(feats, P, cv, conf, agg, counts, cap)
        want = _padded(fp, Pp, cv, cp, agg, mask)
        assert torch.isfinite(got).all(), agg
        assert torch.equal(got, want), "%s: ragged gather differs from the masked entry (max |d| %g)" % (agg, float((got - want).abs().max()))


@pytest.mark.parametrize("cap", [4, 8], ids=["cap4", "cap8"])
def test_generic_gather_bf16_equals_the_masked_entry_on_padded_inputs(cap):
    """bf16 where the generic kernel runs at 4 and 8 views: aggregations other than softmax at C = 32, softmax at C = 16."""
    counts = COUNTS[cap]
    for C, aggs in ((32, ("sum", "max", "conf", "conf_norm")), (16, ("softmax",))):
        feats, P, conf, cv, fp, Pp, cp, mask = _case(counts, cap, C, 12, 16, seed=200 + cap + C)
        feats, fp = feats.bfloat16(), fp.bfloat16()
        for agg in aggs:
            assert torch.equal(_ragged(feats, P, cv, conf, agg, counts, cap), _padded(fp, Pp, cv, cp, agg, mask)), "bf16 %s C%d" % (agg, C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_zero_count_at_kernel_level_writes_zeros(dtype):
    """The hosts refuse a count of 0; the kernels (generic in both branches, and the quad kernel: bf16, softmax, NVcap 4) write zeros for it."""
    for cap, counts in ((4, [0, 3, 0]), (32, [0, 9, 0])):
        feats, P, conf, cv = _case(counts, cap, 32, 12, 16, seed=300 + cap)[:4]
        for agg in AGGS:
            got = _ragged(feats.to(dtype), P, cv, conf, agg, counts, cap)
            assert torch.count_nonzero(got[0]) == 0 and torch.count_nonzero(got[2]) == 0, (agg, cap)
            assert torch.isfinite(got[1]).all() and torch.count_nonzero(got[1]) > 0, (agg, cap)


def test_a_table_that_points_outside_the_rows_is_clamped():
    """The second line of defence: offsets below 0 and beyond T, and a count above NVcap, read rows inside [0, T) (wrong views, finite values)."""
    counts = [4, 4, 4]
    feats, P, conf, cv = _case(counts, 4, 32, 12, 16, seed=310)[:4]
    for table in ([-5, 0, 4, 40], [0, 12, 12, 12], [7, 9, 11, 100]):
        vb = torch.tensor(table, dtype=torch.int32, device=DEV)
        for f in (feats, feats.bfloat16()):
            assert torch.isfinite(_ragged(f, P, cv, conf, "softmax", counts, 4, view_base=vb).float()).all(), table


# ---- quad gather: bf16, C = 32, NVcap 4 or 8, view softmax, bricked volume --------------------------------------------------------------------------
def _grid_case(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(B, 3, generator=g) * 100).numpy().astype(np.float64)
    side = 2500.0
    pos = torch.from_numpy((base - side / 2).astype(np.float32))
    cen = torch.from_numpy(base.astype(np.float32))
    from mvn.utils import volumetric
    rot = torch.from_numpy(np.stack([volumetric.get_rotation_matrix([0, 0, 1], 0.3 * b) for b in range(B)]).astype(np.float32)).reshape(B, 9)
    return pos.to(DEV), cen.to(DEV), rot.to(DEV).contiguous(), float(np.float32(side / (V - 1)))


def _grid_ragged(feats, P, grid, V, counts, cap):
    pos, cen, rot, step = grid
    T, h, w, C = feats.shape
    B = len(counts)
    out = torch.empty(B, V, V, V, C, dtype=feats.dtype, device=DEV)
    coords = torch.empty(B, V, V, V, 3, dtype=torch.float32, device=DEV)
    H.check(H.lib().lt_unproject_grid_ragged_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                                 coords.data_ptr(), None, _base(counts).data_ptr(), out.data_ptr(), B, T, cap, C, h, w, V, H.AGG["softmax"], _st()),
            "lt_unproject_grid_ragged_fwd")
    torch.cuda.synchronize()
    return out, coords


def _grid_padded(fp, Pp, grid, V, mask=None):
    pos, cen, rot, step = grid
    B, NV, h, w, C = fp.shape
    out = torch.empty(B, V, V, V, C, dtype=fp.dtype, device=DEV)
    coords = torch.empty(B, V, V, V, 3, dtype=torch.float32, device=DEV)
    if mask is None:
        H.check(H.lib().lt_unproject_grid_fwd(H.dtype_code(fp.dtype), fp.data_ptr(), Pp.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                              coords.data_ptr(), None, out.data_ptr(), B, NV, C, h, w, V, H.AGG["softmax"], _st()), "lt_unproject_grid_fwd")
    else:
        H.check(H.lib().lt_unproject_grid_masked_fwd(H.dtype_code(fp.dtype), fp.data_ptr(), Pp.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, 0,
                                                     coords.data_ptr(), None, mask.data_ptr(), out.data_ptr(), B, NV, C, h, w, V, H.AGG["softmax"], _st()),
                "lt_unproject_grid_masked_fwd")
    torch.cuda.synchronize()
    return out, coords


QUAD = [(B, cap, V) for B in (3, 8) for cap in (4, 8) for V in (16, 32)]      # (B, NVcap, V): B = 8 pins samples to XCDs, V = 32 walks the bricks in super-blocks
QCOUNTS = {4: [4, 3, 1, 4, 2, 4, 4, 3], 8: [8, 7, 1, 8, 4, 6, 2, 5]}


@pytest.mark.parametrize("B,cap,V", QUAD, ids=["B%d_cap%d_V%d" % c for c in QUAD])
def test_quad_gather_equals_the_masked_quad_entries_and_is_isolated(B, cap, V):
    """Both entries against the masked quad entries on the padded inputs (output and written coordinates), then isolation: NaN in every row (maps,
    projections) that is not sample b's moves no bit of sample b's output -- for every b, the last included."""
    counts = QCOUNTS[cap][:B]
    feats, P, conf, cv, fp, Pp, cp, mask = _case(counts, cap, 32, 24, V, seed=500 + B + cap + V, inside=(V == 16))
    feats, fp = feats.bfloat16(), fp.bfloat16()
    grid = _grid_case(B, V, seed=600 + B)
    got = _ragged(feats, P, cv, conf, "softmax", counts, cap)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, _padded(fp, Pp, cv, cp, "softmax", mask))
    got_g, coords = _grid_ragged(feats, P, grid, V, counts, cap)
    want_g, want_coords = _grid_padded(fp, Pp, grid, V, mask)
    assert torch.equal(got_g, want_g) and torch.equal(coords, want_coords)
    base = np.concatenate([[0], np.cumsum(counts)])
    for b in range(B):
        fn, Pn = torch.full_like(feats, NAN), torch.full_like(P, NAN)
        fn[base[b]:base[b + 1]], Pn[base[b]:base[b + 1]] = feats[base[b]:base[b + 1]], P[base[b]:base[b + 1]]
        assert torch.equal(_ragged(fn, Pn, cv, conf, "softmax", counts, cap)[b], got[b]), "sample %d reads another sample's rows" % b
        assert torch.equal(_grid_ragged(fn, Pn, grid, V, counts, cap)[0][b], got_g[b]), "sample %d reads another sample's rows (grid entry)" % b


@pytest.mark.parametrize("cap", [4, 32], ids=["cap4", "cap32"])
def test_generic_gather_is_isolated(cap):
    """fp32 generic kernel, both branches: NaN in every row (maps, projections, confidences) that is not sample b's moves no bit of sample b's output."""
    counts = COUNTS[cap]
    feats, P, conf, cv = _case(counts, cap, 32, 12, 16, seed=550 + cap)[:4]
    base = np.concatenate([[0], np.cumsum(counts)])
    for agg in ("softmax", "conf_norm"):
        got = _ragged(feats, P, cv, conf, agg, counts, cap)
        for b in range(len(counts)):
            fn, Pn, cn = torch.full_like(feats, NAN), torch.full_like(P, NAN), torch.full_like(conf, NAN)
            s = slice(int(base[b]), int(base[b + 1]))
            fn[s], Pn[s], cn[s] = feats[s], P[s], conf[s]
            assert torch.equal(_ragged(fn, Pn, cv, cn, agg, counts, cap)[b], got[b]), (agg, b)


@pytest.mark.parametrize("dtype,cap,V", [(torch.bfloat16, 4, 16), (torch.bfloat16, 8, 32), (torch.float32, 4, 16), (torch.float32, 8, 6)],
                         ids=["quad4", "quad8", "fp32_cap4", "fp32_cap8"])
def test_equal_counts_give_the_bits_of_the_unmasked_entries(dtype, cap, V):
    B = 3
    counts = [cap] * B
    feats, P, conf, cv, fp, Pp, cp, mask = _case(counts, cap, 32, 24, V, seed=650 + cap + V, inside=(V == 16))
    feats, fp = feats.to(dtype), fp.to(dtype)
    assert torch.equal(feats.reshape(fp.shape), fp)
    assert torch.equal(_ragged(feats, P, cv, conf, "softmax", counts, cap), _padded(fp, Pp, cv, cp, "softmax"))
    grid = _grid_case(B, V, seed=660)
    got, coords = _grid_ragged(feats, P, grid, V, counts, cap)
    want, want_coords = _grid_padded(fp, Pp, grid, V)
    assert torch.equal(got, want) and torch.equal(coords, want_coords)


# ---- algebraic tail ---------------------------------------------------------------------------------------------------------------------------------
def _tail_case(counts, cap, with_conf, seed):
    """Ragged tail inputs and their padded twins (NaN keypoints and confidences, zero projections in the padding)."""
    B, T, J, h, w, Hh, W = len(counts), int(sum(counts)), 17, 32, 32, 128, 128
    g = torch.Generator().manual_seed(seed)
    K, R, t = synth.ring_cameras(cap, Hh)
    Pn = torch.from_numpy(K @ np.concatenate([R, t], -1))
    X = torch.randn(B, J, 3, generator=g).double() * 300
    Xh = torch.cat([X, torch.ones(B, J, 1, dtype=torch.float64)], -1)
    ld = 24          # the head's padded row, as in the plan
    kp, proj, raw = [], [], []
    kpp, Pp = torch.full((B, cap, J, 2), NAN), torch.zeros(B, cap, 3, 4)
    rawp = torch.full((B, cap, ld), NAN)
    for b, n in enumerate(counts):
        px = torch.einsum("vrk,jk->vjr", Pn[:n], Xh[b])
        k = ((px[..., :2] / px[..., 2:] + torch.randn(n, J, 2, generator=g).double() * 0.5) * torch.tensor([w / W, h / Hh], dtype=torch.float64)).float()
        r = torch.rand(n, ld, generator=g) * 0.8 + 0.1
        kp.append(k); proj.append(Pn[:n].float()); raw.append(r)
        kpp[b, :n], Pp[b, :n], rawp[b, :n] = k, Pn[:n].float(), r
    mask = torch.tensor([[1] * n + [0] * (cap - n) for n in counts], dtype=torch.uint8)
    dev = lambda x: x.to(DEV).contiguous()
    return (B, T, J, ld, W / w, Hh / h, dev(torch.cat(kp)), dev(torch.cat(proj)), dev(torch.cat(raw)) if with_conf else None, dev(kpp), dev(Pp),
            dev(rawp) if with_conf else None, dev(mask))


def _tail_ragged(kp, raw, ld, proj, sx, sy, counts, cap, J):
    B, T = len(counts), kp.shape[0]
    k2 = torch.empty(T, J, 2, dtype=torch.float32, device=DEV)
    cf = torch.empty(T, J, dtype=torch.float32, device=DEV)
    k3 = torch.empty(B, J, 3, dtype=torch.float32, device=DEV)
    H.check(H.lib().lt_alg_tail_ragged_fwd(kp.data_ptr(), None if raw is None else raw.data_ptr(), ld, proj.data_ptr(), sx, sy, _base(counts).data_ptr(), k2.data_ptr(),
                                           cf.data_ptr(), k3.data_ptr(), B, T, cap, J, _st()), "lt_alg_tail_ragged_fwd")
    torch.cuda.synchronize()
    return k2, cf, k3


def _tail_padded(kpp, rawp, ld, Pp, sx, sy, J, mask=None):
    B, NV = kpp.shape[:2]
    k2 = torch.empty(B, NV, J, 2, dtype=torch.float32, device=DEV)
    cf = torch.empty(B, NV, J, dtype=torch.float32, device=DEV)
    k3 = torch.empty(B, J, 3, dtype=torch.float32, device=DEV)
    rp = None if rawp is None else rawp.data_ptr()
    if mask is None:
        H.check(H.lib().lt_alg_tail_fwd(kpp.data_ptr(), rp, ld, Pp.data_ptr(), sx, sy, k2.data_ptr(), cf.data_ptr(), k3.data_ptr(), B, NV, J, _st()), "lt_alg_tail_fwd")
    else:
        H.check(H.lib().lt_alg_tail_masked_fwd(kpp.data_ptr(), rp, ld, Pp.data_ptr(), sx, sy, mask.data_ptr(), k2.data_ptr(), cf.data_ptr(), k3.data_ptr(), B, NV, J,
                                               _st()), "lt_alg_tail_masked_fwd")
    torch.cuda.synchronize()
    return k2, cf, k3


@pytest.mark.parametrize("with_conf", [True, False], ids=["conf", "uniform"])
@pytest.mark.parametrize("counts,cap", [([4, 3, 2], 4), ([6, 4, 2], 8)], ids=["432", "642"])
def test_alg_tail_ragged_equals_the_masked_tail_on_padded_inputs(counts, cap, with_conf):
    B, T, J, ld, sx, sy, kp, proj, raw, kpp, Pp, rawp, mask = _tail_case(counts, cap, with_conf, seed=700 + cap)
    k2, cf, k3 = _tail_ragged(kp, raw, ld, proj, sx, sy, counts, cap, J)
    p2, pc, p3 = _tail_padded(kpp, rawp, ld, Pp, sx, sy, J, mask)
    assert torch.isfinite(k3).all() and torch.equal(k3, p3)
    valid = mask.bool()
    assert torch.equal(k2, p2[valid]) and torch.equal(cf, pc[valid])
    # NVcap only bounds the count: a larger one gives the same bits
    assert all(torch.equal(a, b) for a, b in zip(_tail_ragged(kp, raw, ld, proj, sx, sy, counts, 32, J), (k2, cf, k3)))


def test_alg_tail_ragged_with_equal_counts_gives_the_plain_tail():
    counts = [4, 4, 4]
    B, T, J, ld, sx, sy, kp, proj, raw, kpp, Pp, rawp, mask = _tail_case(counts, 4, True, seed=710)
    k2, cf, k3 = _tail_ragged(kp, raw, ld, proj, sx, sy, counts, 4, J)
    p2, pc, p3 = _tail_padded(kpp, rawp, ld, Pp, sx, sy, J)
    assert torch.equal(k3, p3) and torch.equal(k2, p2.reshape(T, J, 2)) and torch.equal(cf, pc.reshape(T, J))


def test_alg_tail_ragged_with_one_view_gives_nan_joints_for_that_sample_only():
    counts = [4, 1, 3]
    B, T, J, ld, sx, sy, kp, proj, raw = _tail_case(counts, 4, True, seed=711)[:9]
    _, cf, k3 = _tail_ragged(kp, raw, ld, proj, sx, sy, counts, 4, J)
    assert torch.isfinite(k3[0]).all() and torch.isnan(k3[1]).all() and torch.isfinite(k3[2]).all() and torch.isfinite(cf).all()


# ---- functional ops ---------------------------------------------------------------------------------------------------------------------------------
def test_unproject_heatmaps_takes_view_counts():
    from mvn.utils import op
    counts = [4, 1, 3]
    feats, P, conf, cv = _case(counts, 4, 32, 12, 16, seed=800)[:4]
    hm = feats.permute(0, 3, 1, 2).contiguous()          # (T, C, h, w)
    for agg, c in (("softmax", None), ("conf", conf)):
        want = _ragged(feats, P, cv, conf, agg, counts, 4).permute(0, 4, 1, 2, 3)
        for vc in (counts, np.asarray(counts), torch.tensor(counts), torch.tensor(counts, device=DEV)):
            assert torch.equal(op.unproject_heatmaps(hm, P, cv, agg, c, view_counts=vc), want)
    hb = hm.bfloat16()
    assert torch.equal(op.unproject_heatmaps(hb, P, cv, "softmax", view_counts=counts), _ragged(feats.bfloat16(), P, cv, conf, "softmax", counts, 4).permute(0, 4, 1, 2, 3))
    with pytest.raises(NotImplementedError, match="inference only"):
        op.unproject_heatmaps(hm.clone().requires_grad_(True), P, cv, "softmax", view_counts=counts)
    with pytest.raises(ValueError, match="sums to 7"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[4, 1, 2])


def test_triangulate_batch_of_points_takes_view_counts():
    from mvn.utils import multiview
    counts = [4, 3, 2]
    B, T, J, ld, sx, sy, kp, proj, raw = _tail_case(counts, 4, True, seed=820)[:9]
    pts = (kp * torch.tensor([sx, sy], device=DEV)).contiguous()
    conf = raw[:, :J].contiguous()
    base = np.concatenate([[0], np.cumsum(counts)])
    for c in (conf, None):
        got = multiview.triangulate_batch_of_points(proj, pts, c, view_counts=counts)
        for b in range(B):
            s = slice(int(base[b]), int(base[b + 1]))
            want = multiview.triangulate_batch_of_points(proj[s][None], pts[s][None], None if c is None else c[s][None])
            assert torch.equal(got[b], want[0]), b
    with pytest.raises(ValueError, match="sample 1 has 1 view"):
        multiview.triangulate_batch_of_points(proj, pts, conf, view_counts=[4, 1, 4])
    with pytest.raises(NotImplementedError, match="inference only"):
        multiview.triangulate_batch_of_points(proj, pts.clone().requires_grad_(True), conf, view_counts=counts)
