"""The test infrastructure of the unprojection backward (tests/unproject_bwd_ref.py), checked without a GPU -- here the reference alone is on trial:
the written-out backward against fp64 autograd through unproject_ref.ref_unproject; for every lattice case of tests/test_gpu_unproject_bwd_kernels.py the
conditions its slack-free gate rests on (the fp32 statement equals the fp64 one bit for bit, exact.assert_exact holds, the padding classes and the 'max'
ties the ids promise are there); the structured point sets counted through the gather's restated walk; the no-flip conditions of the realistic cases;
bwd_plan against lt_unproject_bwd_workspace and the refusals of lt_unproject_bwd that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import lt_hip as H
import unproject_bwd_ref as R
import unproject_ref as U
from oracle import synth
from oracle import vol_oracle as O


@pytest.fixture(autouse=True)
def _gather_path(monkeypatch):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)


# ---- the explicit backward is the derivative of the forward reference ------------------------------------------------------------------------------------
def _autograd(hm, P, cv, G, agg, conf):
    h64 = hm.double().requires_grad_(True)
    c64 = conf.double().requires_grad_(True) if agg.startswith("conf") else None
    out, _ = U.ref_unproject(h64, P, cv, agg, c64)
    C = hm.shape[2]
    (out.reshape(hm.shape[0], -1, C) * G.double().reshape(hm.shape[0], C, -1).permute(0, 2, 1)).sum().backward()
    return h64.grad, (None if c64 is None else c64.grad)


def _ring(NV, C, h, w, vs, seed):
    g = torch.Generator().manual_seed(seed)
    K, Rm, t = synth.ring_cameras(NV, 96, inside=True)
    P = torch.from_numpy(O.resized_projection(K, Rm, t, (96, 96), (h, w))).float()[None].repeat(2, 1, 1, 1).contiguous()
    base = torch.randn(2, 3, generator=g).numpy() * 100
    cv = torch.stack([U.box_coords(base[b], 2500.0, vs, 0.3 * b + 0.1) for b in range(2)])
    return torch.randn(2, NV, C, h, w, generator=g), P, cv, torch.rand(2, NV, C, generator=g) + 0.1, torch.randn(2, C, *vs, generator=g)


def _probe(NV, h, w, flat, C, seed):
    P64 = U.probe_cameras(NV, h, w, flat)
    n = U.probe_size(P64, h, w, times=1)
    pr = U.probe_points(P64, h, w, n)
    g = torch.Generator().manual_seed(seed)
    vs = (4, 4, n // 16)
    return (torch.randn(1, NV, C, h, w, generator=g), torch.from_numpy(P64).float()[None].contiguous(), pr.X.reshape(1, *vs, 3).contiguous(),
            torch.rand(1, NV, C, generator=g) + 0.1, torch.randn(1, C, *vs, generator=g))


@pytest.mark.parametrize("name", ["ring_nv4", "ring_nv9", "probe_nv4"])
def test_explicit_backward_equals_fp64_autograd_through_the_forward_reference(name):
    """All five aggregations; ring cameras with camera 0 inside the grid (depth <= 0 voxels), non-square maps; and the forward's probe points, which hit
    every padding class.  1e-12 of max|ref|, features and confidences."""
    hm, P, cv, conf, G = {"ring_nv4": lambda: _ring(4, 6, 20, 28, (5, 6, 7), 1), "ring_nv9": lambda: _ring(9, 4, 28, 20, (4, 4, 9), 2),
                          "probe_nv4": lambda: _probe(4, 20, 28, 2, 3, 3)}[name]()
    for agg in U.AGGS:
        gf, gc, mag, rec = R.ref_backward(hm, P, cv, G, agg, conf)
        if name.startswith("ring"):
            assert int(rec.taps.invalid[:, 0].sum()) > 0
        else:
            s = U.ref_samples(hm, P, cv)
            assert all(int((s.cls[0, v] == k).sum()) > 0 for v in range(4) for k in range(len(U.CLASSES) - 1))
        af, ac = _autograd(hm, P, cv, G, agg, conf)
        assert float(af.abs().max()) > 0
        assert float((gf - af).abs().max()) <= 1e-12 * float(af.abs().max()), agg
        assert bool((gf.abs() <= mag.feats * (1 + 1e-12)).all()), "the magnitude does not bound the gradient"
        if ac is not None:
            assert float((gc - ac).abs().max()) <= 1e-12 * float(ac.abs().max()), agg
            assert bool((gc.abs() <= mag.conf * (1 + 1e-12)).all())
        else:
            assert gc is None


def test_first_max_is_the_lowest_index_among_the_maxima():
    x = torch.tensor([[0.0, 1.0, 2.0, -1.0], [0.0, 3.0, 2.0, -1.0], [0.0, 3.0, 1.0, 0.0]])
    assert R.first_max(x).tolist() == [0, 1, 0, 2]


# ---- every lattice case: the conditions of the slack-free gate ---------------------------------------------------------------------------------------------
def _plans(spec, case, agg):
    B, NV, C, h, w = case.hm.shape
    return R.bwd_plan(spec["dtype"], B, NV, C, h, w, case.vs, agg, env=spec["env"])


@pytest.mark.parametrize("cid", sorted(R.EXACT))
def test_lattice_case_is_exact_in_fp32_and_enters_its_branch(cid):
    """assert_exact holds (inside lattice_reference), the fp32 statement of the backward equals the fp64 one bit for bit, features and confidences; the
    maps are bf16 numbers; bwd_plan names the branch of the id; the case is not degenerate: every view but a deliberately empty one receives a gradient."""
    spec, case = R.EXACT[cid], R.make(R.EXACT, cid)
    assert torch.equal(case.hm, case.hm.bfloat16().float())
    N = case.vs[0] * case.vs[1] * case.vs[2]
    for agg in spec["aggs"]:
        plan = _plans(spec, case, agg)
        R.plan_is(plan, **spec["plan"])
        gf, gc, rec = R.lattice_reference(cid, case, agg, R.conf_terms(plan, N), key=cid)
        f32, c32, _, _ = R.ref_backward(case.hm, case.P, case.cv, case.G, agg, case.conf, dtype=torch.float32)
        assert f32.dtype == torch.float32 and torch.equal(f32, gf), "%s %s: fp32 and fp64 statements differ" % (cid, agg)
        assert gc is None or torch.equal(c32, gc), "%s %s: confidence gradient" % (cid, agg)
        if agg == "sum":
            for v in range(case.hm.shape[1]):
                empty = cid == "empty_view" and v == 1
                assert (float(gf[:, v].abs().max()) == 0) == empty, (cid, v)


def test_class_coverage_case_has_every_class_in_every_view():
    case = R.make(R.EXACT, "classes")
    s = U.ref_samples(case.hm, case.P, case.cv)
    for b in range(2):
        for v in range(3):
            for k, name in enumerate(U.CLASSES):
                assert int((s.cls[b, v] == k).sum()) >= 1, (v, name)
    ix, iy = s.ix[0], s.iy[0]
    front = s.z[0] > 0
    for v in range(3):
        assert int(((ix[v] == -1) & front[v]).sum()) > 0 and int(((ix[v] == case.w - 1) & front[v]).sum()) > 0, "ix == -1 and ix == w - 1 exactly"
        assert int(((iy[v] == -1) & front[v]).sum()) > 0 and int(((iy[v] == case.h - 1) & front[v]).sum()) > 0


@pytest.mark.parametrize("cid", [c for c in sorted(R.EXACT) if "max" in R.EXACT[c]["aggs"] and not c.startswith(("tiny", "pile", "alternate"))])
def test_max_ties_are_plenty(cid):
    """>= 100 voxel-channels where two views tie for the maximum, some of them with an invalid (depth <= 0) view as the first maximum; with more than 8 views
    also ties between view 0 and a view of index 8 or above that view 0 must win.  (Not asked of the one-view cases, nor of pile / alternate: 128 voxels,
    all of them in front of both views, built for the rounds of the gather.)"""
    case = R.make(R.EXACT, cid)
    NV = case.hm.shape[1]
    if NV == 1:
        return
    _, _, rec = R.lattice_reference(cid, case, "max", key=cid)
    best = rec.vals.max(1)[0]                                                   # B, N, C
    ties = (rec.vals == best[:, None]).sum(1) >= 2
    assert int(ties.sum()) >= 100, int(ties.sum())
    # whether the winning view of (b, n, c) is at depth <= 0 for voxel n
    inv_w = torch.stack([rec.taps.invalid[b].t()[torch.arange(rec.winner.shape[1])[:, None], rec.winner[b]] for b in range(rec.winner.shape[0])])
    if cid not in ("refill", "empty_view"):          # no view 0 at depth <= 0 there
        assert int((ties & inv_w).sum()) > 0, "no tie whose first maximum is an invalid view"
    if NV > 8:
        late = (rec.vals[:, 8:] == best[:, None]).any(1) & (rec.winner == 0) & (best != 0)
        assert int(late.sum()) >= 100, int(late.sum())


# ---- the structured point sets ------------------------------------------------------------------------------------------------------------------------------
def _stats(cid, b, v, halves):
    case = R.make(R.EXACT, cid)
    taps = R.ref_taps(case.P, case.cv, case.h, case.w)
    return R.round_stats(taps, b, v, case.vs, case.h, case.w, halves), taps


@pytest.mark.parametrize("cid,halves", [("pile_C4", 2), ("pile_C64", 1)])
def test_pile_has_rounds_with_2_3_and_4_hits_in_one_cell(cid, halves):
    for b in range(2):
        st, _ = _stats(cid, b, 0, halves)
        assert st["multi"][2] > 0 and st["multi"][3] > 0 and st["multi"][4] > 0, st["multi"]
        assert st["hits"] == 128 and st["rounds"] == 32, "every lane of both bricks is a hit of half 0 of tile (0, 0): a row of four lanes is a round"


@pytest.mark.parametrize("cid,halves", [("alternate_C4", 2), ("alternate_C64", 1)])
def test_alternate_has_the_pattern_a_b_a(cid, halves):
    for b in range(2):
        st, _ = _stats(cid, b, 0, halves)
        assert st["alt"] >= 32, st
        assert st["hits"] == 128 and st["rounds"] == 32


def test_refill_fills_the_candidate_list_twice_with_empty_bricks_in_the_walk():
    for b in range(2):
        st, _ = _stats("refill", b, 0, 2)
        assert list(st["cand"].values()) == [343 - 69], st["cand"]
        assert st["cand"][(0, 0)] >= R.G_LIST - 64 + 1 and 343 > 256
        assert len(st["empty"]) == 69 and st["empty"][0] in (0, 2) and all(e2 - e1 == 5 for e1, e2 in zip(st["empty"], st["empty"][1:])), "empty bricks between others"


@pytest.mark.parametrize("cid,halves", [("seams_C16", 2), ("seams_C64", 1)])
def test_seams_straddle_the_half_wave_split_and_the_tile_edges(cid, halves):
    case = R.make(R.EXACT, cid)
    taps = R.ref_taps(case.P, case.cv, case.h, case.w)
    for b in range(2):
        x0, y0, four = taps.x0[b, 0], taps.y0[b, 0], (taps.wt[b, 0] != 0).all(1)
        for x in R.SEAM_X:
            for y in R.SEAM_Y:
                n = int(((x0 == x) & (y0 == y) & ((taps.wt[b, 0] != 0).sum(1) == (2 if x == 16 else 4))).sum())
                assert n >= 9, (x, y, n)
        st = R.round_stats(taps, b, 0, case.vs, case.h, case.w, halves)
        assert st["straddle_half"] >= 27 and st["straddle_tile_x"] >= 27 and st["straddle_tile_y"] >= 36
        assert len(st["cand"]) == 6 and min(st["cand"].values()) > 0, "a tile without a candidate brick"


def test_empty_view_has_no_weighted_tap_in_view_1():
    st, taps = _stats("empty_view", 0, 1, 2)
    assert bool(taps.invalid[:, 1].all()) and len(st["empty"]) == 8 and set(st["cand"].values()) == {0}
    assert not bool(taps.invalid[:, 0].any())


def test_brick_lanes_is_a_bijection_with_the_kernels_order():
    for vs in ((5, 6, 7), (4, 4, 8), (1, 1, 1), (28, 28, 28)):
        BL = R.brick_lanes(vs)
        hit = BL[BL >= 0]
        assert np.array_equal(np.sort(hit), np.arange(vs[0] * vs[1] * vs[2]))
    BL = R.brick_lanes((5, 6, 7))
    assert BL.shape == (8, 64) and BL[0, 0] == 0 and BL[0, 1] == 1 and BL[0, 4] == 7 and BL[0, 16] == 42 and BL[1, 0] == 4 and BL[1, 3] == -1 and BL[2, 0] == 28


# ---- the toleranced layers ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(c for c in R.TOLERANCED if c.endswith("fp32")))
def test_toleranced_lattice_case_has_a_yardstick_and_enters_its_branch(cid):
    """The fp32 statement against the fp64 one, in units of the magnitude: the yardstick the GPU gate multiplies by 8.  It must be a rounding-sized number
    (neither 0, which would make the gate an equality the kernel cannot meet, nor large, which would make it loose)."""
    spec, case = R.TOLERANCED[cid], R.make(R.TOLERANCED, cid)
    for agg in spec["aggs"]:
        R.plan_is(_plans(spec, case, agg), **spec["plan"])
        gf, gc, mag, _ = R.ref_backward(case.hm, case.P, case.cv, case.G, agg, case.conf)
        f32, c32, _, _ = R.ref_backward(case.hm, case.P, case.cv, case.G, agg, case.conf, dtype=torch.float32)
        nz = mag.feats > 0
        assert bool((f32[~nz] == 0).all()) and bool((gf[~nz] == 0).all())
        yard = float(((f32.double() - gf).abs()[nz] / mag.feats[nz]).max())
        print("%s %s: yardstick %.3e" % (cid, agg, yard))
        assert yard < 2e-6 and (yard > 1e-8 or case.hm.shape[1] == 1), yard          # one view: p = 1 and 1 + x - out = 1, exact
        if gc is not None:
            yc = float(((c32.double() - gc).abs() / mag.conf).max())
            print("%s %s: confidence yardstick %.3e" % (cid, agg, yc))
            assert yc < 2e-6, yc


@pytest.mark.parametrize("NV", R.REAL_NV)
@pytest.mark.parametrize("C", R.REAL_C)
def test_realistic_case_does_not_flip_between_fp32_and_fp64(NV, C):
    """The conditions of the 1e-4 max-norm gate: no depth sign and no 'max' winner differs between the fp32 and the fp64 statement, on the fp32 maps and
    on the bf16-rounded ones; every view receives a gradient; camera 0 sees part of the grid at depth <= 0.  A seed that violates one is replaced
    (unproject_bwd_ref.REAL_SEED); nothing is excluded from the comparison."""
    case = R.realistic_case(NV, C)
    for hm in (case.hm, case.hm.bfloat16().float()):
        for agg in U.AGGS:
            gf, _, _, r64 = R.ref_backward(hm, case.P, case.cv, case.G, agg, case.conf)
            f32, _, _, r32 = R.ref_backward(hm, case.P, case.cv, case.G, agg, case.conf, dtype=torch.float32)
            assert torch.equal(r64.taps.invalid, r32.taps.invalid), "a depth sign differs"
            assert 0 < int(r64.taps.invalid[:, 0].sum()) < r64.taps.invalid[:, 0].numel()
            if agg == "max":
                assert torch.equal(r64.winner, r32.winner), "a max winner differs"
            assert all(float(gf[:, v].abs().max()) > 0 for v in range(NV)), agg
            assert float((f32.double() - gf).abs().max()) <= 2e-5 * float(gf.abs().max()), "the fp32 statement itself is not within a fifth of the gate"


# ---- bwd_plan against the library -------------------------------------------------------------------------------------------------------------------------
PLAN_SHAPES = [(1, 3, 4, (5, 6, 7)), (2, 4, 8, (4, 4, 8)), (3, 9, 16, (5, 6, 7)), (1, 31, 32, (64, 64, 64)), (2, 2, 64, (36, 32, 32)), (2, 1, 4, (28, 28, 28)),
               (2, 1, 4, (1, 1, 1)), (1, 3, 12, (5, 6, 7)), (1, 3, 128, (5, 6, 7))]


@pytest.mark.parametrize("B,NV,C,vs", PLAN_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_bwd_plan_agrees_with_the_workspace_entry(B, NV, C, vs):
    plan = R.bwd_plan(torch.float32, B, NV, C, 20, 37, vs, "sum", env={})
    assert H.lib().lt_unproject_bwd_workspace(B, NV, C, *vs) == plan["per_sample"] * B
    assert (plan["path"] == "gather") == (C in (4, 8, 16, 32, 64))


def test_bwd_plan_dispatch_one_shape_per_outcome(monkeypatch):
    f32, bf = torch.float32, torch.bfloat16
    p = R.bwd_plan(f32, 2, 3, 8, 20, 37, (5, 6, 7), "sum", env={})
    R.plan_is(p, path="gather", CW=2, HALVES=2, k1="mv4", finalizer=None, nblk1=2, chunk=2, nchunks=1, tiles=6, nbricks=8, k1_strided=False)
    R.plan_is(R.bwd_plan(bf, 3, 5, 64, 33, 17, (5, 6, 7), "conf", env={}, ws_samples=2), CW=16, HALVES=1, k1="mv8", finalizer="small", chunk=2, nchunks=2, tiles=6)
    R.plan_is(R.bwd_plan(f32, 3, 8, 32, 16, 16, (5, 6, 7), "conf_norm", env={}, ws_samples=1), k1="mv8", chunk=1, nchunks=3, tiles=1, HALVES=2)
    R.plan_is(R.bwd_plan(f32, 1, 9, 16, 20, 37, (5, 6, 7), "max", env={}), k1="passes", finalizer=None, many=True)
    R.plan_is(R.bwd_plan(f32, 1, 9, 16, 20, 37, (5, 6, 7), "softmax", env={}), k1="passes")
    R.plan_is(R.bwd_plan(f32, 1, 17, 16, 20, 37, (5, 6, 7), "conf", env={}), k1="groups", groups=3, finalizer="many")
    R.plan_is(R.bwd_plan(f32, 1, 32, 16, 20, 37, (5, 6, 7), "sum", env={}), k1="groups", groups=4, finalizer=None)
    R.plan_is(R.bwd_plan(f32, 2, 2, 64, 20, 37, (36, 32, 32), "conf", env={}), nblk1=2048, k1_strided=True, k1_items_per_lane=2)
    R.plan_is(R.bwd_plan(f32, 2, 2, 64, 20, 37, (32, 32, 32), "conf", env={}), nblk1=2048, k1_strided=False)
    R.plan_is(R.bwd_plan(f32, 1, 3, 12, 20, 37, (5, 6, 7), "conf", env={}), path="scatter", kernel="scatter")
    R.plan_is(R.bwd_plan(f32, 1, 9, 128, 20, 37, (5, 6, 7), "max", env={}), path="scatter", kernel="scatter_many")
    R.plan_is(R.bwd_plan(f32, 1, 3, 32, 20, 37, (5, 6, 7), "sum", env={"LT_UNPROJ_BWD_ATOMICS": "1"}), path="scatter")
    R.plan_is(R.bwd_plan(f32, 1, 3, 32, 20, 37, (5, 6, 7), "sum", env={"LT_UNPROJ_BWD_ATOMICS": "0"}), path="gather")
    monkeypatch.setenv("LT_UNPROJ_BWD_ATOMICS", "1")
    R.plan_is(R.bwd_plan(f32, 1, 3, 32, 20, 37, (5, 6, 7), "sum"), path="scatter")
    assert H.lib().lt_unproject_bwd_workspace(1, 3, 32, 5, 6, 7) == 0


REFUSALS = [  # id, (NV, C, h, w, vs, agg), env, has_conf, workspace in samples' shares (None: none at all)
    ("no_views", (0, 8, 20, 37, (5, 6, 7), "sum"), {}, False, 1),
    ("33_views", (33, 8, 20, 37, (5, 6, 7), "sum"), {}, False, 1),
    ("C_not_a_multiple_of_4", (3, 6, 20, 37, (5, 6, 7), "sum"), {}, False, 1),
    ("one_row_map", (3, 8, 1, 37, (5, 6, 7), "sum"), {}, False, 1),
    ("maps_at_2^31", (16, 32, 2048, 2048, (5, 6, 7), "sum"), {}, False, 1),
    ("conf_without_confidences", (3, 8, 20, 37, (5, 6, 7), "conf"), {}, False, 1),
    ("scatter_conf_norm", (3, 12, 20, 37, (5, 6, 7), "conf_norm"), {}, True, 1),
    ("atomics_conf_norm", (9, 32, 20, 37, (5, 6, 7), "conf_norm"), {"LT_UNPROJ_BWD_ATOMICS": "1"}, True, 1),
    ("no_workspace", (3, 8, 20, 37, (5, 6, 7), "max"), {}, False, 0),
]


@pytest.mark.parametrize("cid,args,env,has_conf,ws", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bwd_plan_agrees_with_the_refusals_that_need_no_device(cid, args, env, has_conf, ws, monkeypatch):
    """Argument validation runs before any device work, so dummy non-null pointers are enough."""
    NV, C, h, w, vs, agg = args
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    plan = R.bwd_plan(torch.float32, 2, NV, C, h, w, vs, agg, env=env, ws_samples=ws, has_conf=has_conf)
    assert plan["refused"] is not None
    one = ctypes.c_void_p(256)
    lib = H.lib()
    nbytes = plan.get("per_sample", 0) * ws
    if cid == "no_workspace":
        nbytes = plan["per_sample"] - 1
    rc = lib.lt_unproject_bwd(H.LT_F32, one, one, one, one if has_conf else None, one, one, one if has_conf else None, 2, NV, C, h, w, *vs, H.AGG[agg],
                              one, nbytes, None)
    msg = lib.lt_last_error().decode()
    assert rc == plan["refused"][0] and plan["refused"][1] in msg, (rc, msg, plan["refused"])
