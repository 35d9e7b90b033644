"""The test infrastructure of the unprojection forward (tests/unproject_ref.py), checked without a GPU: the fp64 reference against the oracle, the
restated brick orders as bijections, the probe points' classes (a CONDITION of tests/test_gpu_unproject_kernels.py: it cannot silently lose a class),
the restated dispatch on one shape per outcome, and the coverage of the generic kernel's case table."""
import itertools

import numpy as np
import pytest
import torch

import unproject_ref as U
from oracle import synth
from oracle import vol_oracle as O


def _ring_case(B, NV, C, h, w, vs, inside, seed):
    g = torch.Generator().manual_seed(seed)
    K, R, t = synth.ring_cameras(NV, 96, inside=inside)
    P = torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (h, w))).float()[None].repeat(B, 1, 1, 1).contiguous()
    hm = torch.randn(B, NV, C, h, w, generator=g)
    conf = torch.rand(B, NV, C, generator=g) + 0.1
    base = torch.randn(B, 3, generator=g).numpy() * 100
    cv = torch.stack([U.box_coords(base[b], 2500.0, vs, 0.3 * b + 0.1) for b in range(B)])
    return hm, P, cv, conf


@pytest.mark.parametrize("NV,h,w,vs,inside", [(4, 20, 28, (4, 8, 32), True), (3, 28, 20, (7, 7, 7), True), (9, 24, 24, (8, 4, 16), False),
                                               (1, 20, 28, (1, 1, 300), False)], ids=["nv4_20x28_inside", "nv3_28x20_inside", "nv9_square", "nv1_points"])
def test_ref_unproject_equals_the_oracle_in_fp64(NV, h, w, vs, inside):
    """Every aggregation, non-square maps, a camera inside the cube: 1e-12 of max|ref| from oracle.vol_oracle.unproject_heatmaps(dtype=float64),
    which goes through grid_sample."""
    hm, P, cv, conf = _ring_case(2, NV, 6, h, w, vs, inside, seed=NV * 10 + h)
    s = U.ref_samples(hm, P, cv)
    if inside:
        assert int((s.cls[:, 0] == U.CLS["z<0"]).sum()) > 0, "the camera inside the cube leaves no voxel behind it"
    for agg in U.AGGS:
        got = U.aggregate(s.vals, agg, conf).reshape(2, *vs, 6).permute(0, 4, 1, 2, 3)
        oc = conf.double() / conf.double().sum(1, keepdim=True) if agg == "conf_norm" else conf
        want = O.unproject_heatmaps(hm, P, cv, "conf" if agg == "conf_norm" else agg, oc, dtype=torch.float64)
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= 1e-12, (agg, err)


def test_ref_unproject_with_a_mask_equals_itself_on_the_compacted_views():
    hm, P, cv, conf = _ring_case(3, 5, 4, 20, 28, (4, 4, 16), True, seed=5)
    mask = torch.tensor([[1, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 0]], dtype=torch.uint8)
    nan = hm.clone()
    nan[mask == 0] = float("nan")          # a masked view's map takes no part: it may hold anything
    for agg in U.AGGS:
        s = U.ref_samples(hm, P, cv)
        got = U.aggregate(s.vals, agg, conf, mask)
        assert torch.equal(U.aggregate(U.ref_samples(nan, P, cv).vals, agg, conf, mask), got), agg
        for b in range(3):
            idx = torch.nonzero(mask[b]).flatten()
            if idx.numel() == 0:
                assert torch.count_nonzero(got[b]) == 0
                continue
            want, _ = U.ref_unproject(hm[b:b + 1, idx], P[b:b + 1, idx], cv[b:b + 1], agg, conf[b:b + 1, idx])
            assert torch.equal(got[b], want.reshape(-1, 4)), (agg, b)


@pytest.mark.parametrize("vol", sorted(U.VOLUMES))
def test_chunk_voxels_is_a_bijection_in_both_orders(vol):
    v = U.VOLUMES[vol]
    nvox = v[0] * v[1] * v[2]
    maps = {}
    for raster in (False, True):
        plan = U.unproject_plan(torch.float32, 1, 4, 32, 20, 28, *v, "sum", env={"LT_UNPROJ_RASTER": "1"} if raster else {})
        m = U.chunk_voxels(plan)
        assert m.shape == (-(-nvox // 256), 256)
        hit = m[m >= 0]
        assert hit.size == nvox and np.array_equal(np.sort(hit), np.arange(nvox)), (vol, raster)
        if plan["bricked"]:
            assert (m >= 0).all()
        else:
            assert np.array_equal(m.ravel()[:nvox], np.arange(nvox)) and (m.ravel()[nvox:] == -1).all()
        maps[raster] = (plan, m)
    blocked = all(x % 32 == 0 for x in v)
    assert maps[False][0]["blocked"] == blocked and not maps[True][0]["blocked"]
    assert np.array_equal(maps[False][1], maps[True][1]) == (not blocked), "blocked and raster order must differ exactly where blocked is set"


def test_blocked_order_tells_the_super_block_axes_apart():
    """64 x 64 x 96: ngi, ngj, ngk = 2, 2, 3.  Chunk 128 starts the second super-block along k, chunk 384 the second along j, chunk 768 the second along i."""
    plan = U.unproject_plan(torch.float32, 1, 4, 32, 20, 28, 64, 64, 96, "sum", env={})
    assert plan["blocked"] and plan["chunks"] == 1536
    assert U.brick_of(plan, 0) == (0, 0, 0) and U.brick_of(plan, 1) == (0, 0, 16) and U.brick_of(plan, 2) == (0, 4, 0) and U.brick_of(plan, 16) == (4, 0, 0)
    assert U.brick_of(plan, 128) == (0, 0, 32) and U.brick_of(plan, 384) == (0, 32, 0) and U.brick_of(plan, 768) == (32, 0, 0)
    assert U.brick_of(plan, 1535) == (60, 60, 80)


def test_sample_of_block_covers_every_sample_and_chunk_once():
    for B, vol in ((16, "7x7x7"), (16, "4x8x32"), (8, "1x1x300"), (3, "8x4x16")):
        plan = U.unproject_plan(torch.float32, B, 3, 32, 20, 28, *U.VOLUMES[vol], "sum", env={})
        seen = [U.sample_of_block(plan, k) for k in range(B * plan["chunks"])]
        assert sorted(seen) == [(b, c) for b in range(B) for c in range(plan["chunks"])]
        assert plan["xcd_pin"] == (B % 8 == 0)
        if plan["xcd_pin"]:
            assert all(U.sample_of_block(plan, k)[0] % 8 == k % 8 for k in range(B * plan["chunks"]))


PROBES = [(4, 20, 28, 2), (8, 28, 20, 5)]          # (NV, h, w, the flat view): lane 2 of the quad; lane 1, second view of the lane


@pytest.mark.parametrize("NV,h,w,flat", PROBES, ids=["nv4_20x28", "nv8_28x20"])
def test_probe_points_reach_every_class_in_every_view(NV, h, w, flat):
    """Counted by ref_samples on the fp32-rounded matrices and points, i.e. on what the kernels get.  Every class at least 8 times in every view among the
    rows that aim at it away from a threshold; pz == 0 in the flat view alone (it cannot be exact in fp32 AND fp64 for a ring camera: the fp64 product
    X2 r2 is not rounded to the fp32 value that cancels t).  No table row that is not itself a threshold row (ix in {-1, 0, w-1}, likewise iy) comes within
    1e-3 px of a class boundary in the view it aims at."""
    P64 = U.probe_cameras(NV, h, w, flat)
    n = U.probe_size(P64, h, w)
    pr = U.probe_points(P64, h, w, n)
    assert n % 256 == 0 and tuple(pr.X.shape) == (n, 3) and bool(torch.isfinite(pr.X).all())
    P = torch.from_numpy(P64).float()
    s = U.ref_samples(torch.zeros(1, NV, 1, h, w), P[None], pr.X[None])
    me = torch.from_numpy(pr.view)
    pt = torch.arange(n)
    cls, ix, iy = s.cls[0, me, pt], s.ix[0, me, pt], s.iy[0, me, pt]       # in the view each point aims at
    thr = np.isin(pr.ix, (-1.0, 0.0, w - 1.0)) | np.isin(pr.iy, (-1.0, 0.0, h - 1.0))
    table = torch.from_numpy((pr.kind == U.TABLE) & ~thr)
    front = table & torch.from_numpy(pr.depth > 0)
    # the table rows land where they aim
    assert float((ix[front] - torch.from_numpy(pr.ix)[front]).abs().max()) < 1e-3 and float((iy[front] - torch.from_numpy(pr.iy)[front]).abs().max()) < 1e-3
    for bnd in (-1.0, 0.0, w - 1.0, float(w)):
        assert float((ix[front] - bnd).abs().min()) > 1e-3
    for bnd in (-1.0, 0.0, h - 1.0, float(h)):
        assert float((iy[front] - bnd).abs().min()) > 1e-3
    for v in range(NV):
        mine = table & (me == v)
        for name in U.CLASSES[:-1]:
            assert int((cls[mine] == U.CLS[name]).sum()) >= 8, (v, name)
    zero = torch.from_numpy(pr.kind == U.ZERO)
    assert int(zero.sum()) >= 8 and bool((me[zero] == flat).all()) and bool((cls[zero] == U.CLS["z==0"]).all())
    assert bool((pr.X[zero][:, 2] == 0).all())
    # ... and they would be sampled inside the map if the depth test let pz == 0 through (pz -> 1)
    zx = pr.X[zero].double()
    px, py = (zx[:, 0] * U.FLAT_F) / h * (w - 1), (zx[:, 1] * U.FLAT_F) / w * (h - 1)
    assert bool(((px > 1) & (px < w - 2) & (py > 1) & (py < h - 2)).all())
    # the tiny depths: |u| far outside in fp64 wherever the depth came out positive
    tiny = torch.from_numpy(pr.kind == U.TINY)
    tc = cls[tiny]
    assert bool(((tc == U.CLS["outside"]) | (tc == U.CLS["z<0"])).all())
    assert bool(torch.isfinite(ix[tiny]).all()) and float(ix[tiny].abs().min()) > 1e4


PLAN_TABLE = [
    # id, (dtype, B, NV, C, h, w, v0, v1, v2, agg), env, expected
    ("quad4", (torch.bfloat16, 3, 4, 32, 20, 28, 4, 8, 32, "softmax"), {}, dict(kernel="quad", nvl=1, bricked=True, blocked=False, chunks=4, xcd_pin=False)),
    ("quad8_blocked_pinned", (torch.bfloat16, 8, 8, 32, 24, 24, 64, 64, 96, "softmax"), {}, dict(kernel="quad", nvl=2, blocked=True, chunks=1536, xcd_pin=True)),
    ("quad_raster_switch", (torch.bfloat16, 1, 4, 32, 24, 24, 32, 64, 96, "softmax"), {"LT_UNPROJ_RASTER": "1"}, dict(kernel="quad", blocked=False, bricked=True)),
    ("raster_switch_0_is_off", (torch.bfloat16, 1, 4, 32, 24, 24, 32, 64, 96, "softmax"), {"LT_UNPROJ_RASTER": "0"}, dict(kernel="quad", blocked=True)),
    ("no_q4_switch", (torch.bfloat16, 1, 4, 32, 24, 24, 16, 16, 16, "softmax"), {"LT_UNPROJ_NO_Q4": "1"}, dict(kernel="generic", ch=8, small_nv=True)),
    ("quad_needs_softmax", (torch.bfloat16, 1, 4, 32, 24, 24, 16, 16, 16, "sum"), {}, dict(kernel="generic", ch=8, small_nv=True)),
    ("quad_needs_c32", (torch.bfloat16, 1, 4, 16, 24, 24, 16, 16, 16, "softmax"), {}, dict(kernel="generic", ch=8)),
    ("quad_needs_4_or_8_views", (torch.bfloat16, 1, 3, 32, 24, 24, 16, 16, 16, "softmax"), {}, dict(kernel="generic", ch=8, small_nv=True)),
    ("quad_needs_bricks", (torch.bfloat16, 1, 8, 32, 24, 24, 12, 12, 12, "softmax"), {}, dict(kernel="generic", bricked=False, chunks=7)),
    ("quad_needs_bf16", (torch.float32, 1, 4, 32, 24, 24, 16, 16, 16, "softmax"), {}, dict(kernel="generic", ch=4, small_nv=True)),
    ("quad_needs_maps_below_2^30", (torch.bfloat16, 1, 8, 32, 2048, 2048, 16, 16, 16, "softmax"), {}, dict(kernel="generic", ch=8, supported=True)),
    ("quad_just_below_2^30", (torch.bfloat16, 1, 4, 32, 2048, 4095, 16, 16, 16, "softmax"), {}, dict(kernel="quad", supported=True)),
    ("maps_at_2^31_refused", (torch.float32, 1, 16, 32, 2048, 2048, 16, 16, 16, "sum"), {}, dict(supported=False)),
    ("maps_below_2^31", (torch.float32, 1, 16, 32, 2048, 2047, 16, 16, 16, "sum"), {}, dict(supported=True, small_nv=False)),
    ("fp32_ch1", (torch.float32, 1, 9, 5, 20, 28, 7, 7, 7, "max"), {}, dict(kernel="generic", ch=1, small_nv=False, bricked=False, chunks=2)),
    ("bf16_ch1", (torch.bfloat16, 16, 8, 12, 20, 28, 1, 1, 300, "conf_norm"), {}, dict(kernel="generic", ch=1, small_nv=True, bricked=False, chunks=2, xcd_pin=True)),
    ("blocked_needs_32_on_every_axis", (torch.float32, 1, 4, 32, 24, 24, 32, 32, 48, "sum"), {}, dict(blocked=False, bricked=True)),
]


@pytest.mark.parametrize("cid,args,env,expect", PLAN_TABLE, ids=[c[0] for c in PLAN_TABLE])
def test_unproject_plan_one_shape_per_dispatch_outcome(cid, args, env, expect):
    plan = U.unproject_plan(*args, env=env)
    for k, v in expect.items():
        assert plan[k] == v, (cid, k, plan)


def test_generic_case_table_covers_every_pair():
    """Every (type, C) with every NV, every volume, map shape and batch size; every NV with every volume, ...: all pairs of values of two factors."""
    cs = list(U.generic_cases().values())
    rows = [((c["ty"], c["C"]), c["NV"], c["vol"], c["hw"], c["B"]) for c in cs]
    dom = [set(r[k] for r in rows) for k in range(5)]
    assert dom[0] == set(U.GENERIC_TC) and dom[1] == set(U.GENERIC_NV) and dom[4] == {1, 3, 8, 16}
    for a, b in itertools.combinations(range(5), 2):
        have = set((r[a], r[b]) for r in rows)
        assert not [(x, y) for x in dom[a] for y in dom[b] if (x, y) not in have], (a, b)
    for ty in ("fp32", "bf16"):
        for vol in ("7x7x7", "4x8x32"):
            assert any(c["ty"] == ty and c["vol"] == vol and c["B"] == 16 for c in cs), (ty, vol)
