"""CPU: the ground the direct tests of csrc/ransac.hip (tests/test_gpu_ransac_kernels.py) stand on.

  * tests/ransac_ref.py, the numpy fp64 restatement, gives the reference's own masks and pre-refinement points on every problem of
    tests/golden/ransac_ops.npz, in both schedule modes;
  * every case table meets the conditions under which "masks equal, points within 1e-6" is a fair demand of the kernel: no error within
    1e-6 of eps (the fixture generator's re-seeding rule), finite points, and the fp64 point itself pinned to 1e-8 (it moves less than
    that when the SVD gets A's rows in reverse order).  A seed that fails one is replaced in the table; the gates stay;
  * the two-cluster construction gives the expected sets under the reference;
  * tests/golden/ransac_branches.npz: every problem well posed, residuals in both of Huber's regimes at each width;
  * CHECKLIST: every branch of ransac_kernel and hm_argmax_kernel the direct tests are there for is reached by a named case.  A table
    that stops reaching its branch fails here: change the table, not the expectation."""
import os

import numpy as np
import pytest

import test_gpu_ransac_kernels as K
from ransac_ref import huber_residuals, ransac_ref, synth_problems

TAGS = ["nv%d_d%d" % (nv, d) for nv in (2, 3, 4, 8) for d in (0, 1)]


@pytest.mark.parametrize("mode", ["replay", "exh"])
@pytest.mark.parametrize("tag", TAGS)
def test_the_restatement_gives_the_reference_s_masks_and_points(golden_dir, tag, mode):
    g = np.load(os.path.join(golden_dir, "ransac_ops.npz"))
    P, pts = g[tag + "_P"], g[tag + "_pts"]
    B, NV, J = pts.shape[:3]
    for b in range(B):
        for j in range(J):
            X, m, _, _ = ransac_ref(P[b], pts[b, :, j], g["%s_replay_draws" % tag][b, j] if mode == "replay" else None)
            assert np.array_equal(m, g["%s_%s_inl" % (tag, mode)][b, j].astype(bool)), (b, j)
            ref = g["%s_%s_pre" % (tag, mode)][b, j]
            assert np.abs(X - ref).max() <= 1e-9 * np.abs(ref).max(), (b, j)


def test_the_shared_generator_still_draws_the_fixture_s_problems(golden_dir):
    """tools/make_golden_ransac.py imports synth_problems from tests/ransac_ref.py: seed 100 NV + direct (+ 1000 per re-seeding)."""
    g = np.load(os.path.join(golden_dir, "ransac_ops.npz"))
    for nv in (2, 3, 4, 8):
        for d in (0, 1):
            tag = "nv%d_d%d" % (nv, d)
            assert any(all(np.array_equal(a, g[tag + k]) for a, k in zip(synth_problems(np.random.RandomState(100 * nv + d + 1000 * r), 4, nv, 17), ("_P", "_pts")))
                       for r in range(4)), tag


@pytest.mark.parametrize("tid", K.all_tables())
def test_every_case_table_meets_the_conditions_of_its_gates(tid):
    X, M, margin, unc, _ = K.reference(tid)
    print("%s: min eps margin %.3e, max self-uncertainty %.3e, inlier sets of %d to %d views" % (tid, margin.min(), unc.max(), M.sum(-1).min(), M.sum(-1).max()))
    assert np.isfinite(X).all()
    assert (margin >= 1e-6).all(), np.argwhere(~(margin >= 1e-6))
    assert (unc <= 1e-8).all(), np.argwhere(~(unc <= 1e-8))


@pytest.mark.parametrize("tid", list(K.TIES))
def test_the_two_cluster_problems_give_the_expected_sets(tid):
    _, M, _, _, facts = K.reference(tid)
    nv, sched = K.TIES[tid]
    assert np.array_equal(M[0, 0], K.tie_expected(nv, sched))
    assert facts[0][0]["rival"] and max(facts[0][0]["sizes"]) == nv // 2      # another set of the same size came later and was not taken


@pytest.mark.parametrize("nv", [16, 32])
def test_the_wide_refinement_fixture_is_well_posed_and_in_both_huber_regimes(golden_dir, nv):
    path = os.path.join(golden_dir, "ransac_branches.npz")
    assert os.path.getsize(path) < 50 * 1024
    g = np.load(path)
    tag = "nv%d_d1" % nv
    P, pts, inl, post = g[tag + "_P"], g[tag + "_pts"], g[tag + "_exh_inl"], g[tag + "_exh_post"]
    assert pts.shape == (1, nv, 12, 2) and g[tag + "_exh_well"].all()
    z = np.concatenate([huber_residuals(P[0], pts[0, :, j], post[0, j], inl[0, j]) for j in range(12)])
    print("%s: inlier sets of %d to %d views, %d residuals in the quadratic regime, %d in the linear" % (tag, inl.sum(-1).min(), inl.sum(-1).max(), (z <= 1).sum(), (z > 1).sum()))
    assert (z <= 1).any() and (z > 1).any()
    assert inl.sum(-1).max() > 8
    for j in range(12):                                 # the fixture's masks and pre-refinement points are the restatement's too
        X, m, margin, unc = ransac_ref(P[0], pts[0, :, j])
        assert np.array_equal(m, inl[0, j].astype(bool)) and margin >= 1e-6 and unc <= 1e-8
        assert np.abs(X - g[tag + "_exh_pre"][0, j]).max() <= 1e-9 * np.abs(X).max()


# ---- the checklist ---------------------------------------------------------------------------------------------------------------------------
def _ransac_facts():
    """case id -> what the reference saw on it."""
    out = {}
    for tid in K.all_tables():
        P, pts, pairs = K.table(tid)
        _, M, _, _, facts = K.reference(tid)
        fl = [f for row in facts for f in row]
        B, NV, J = pts.shape[:3]
        out[tid] = {"id": tid, "NV": NV, "problems": B * J, "pairs": pairs is not None, "n_iters": None if pairs is None else pairs.shape[2],
                    "skipped": sum(f["skipped"] for f in fl), "fallback": sum(f["fallback"] for f in fl), "rival": sum(f["rival"] for f in fl),
                    "only_invalid": sum(f["fallback"] and f["skipped"] > 0 for f in fl), "mixed": sum(0 < f["skipped"] and not f["fallback"] for f in fl),
                    "bit31_set": int(M[..., 31].sum()) if NV == 32 else 0, "bit31_clear": int((~M[..., 31]).sum()) if NV == 32 else 0,
                    "sizes": (int(M.sum(-1).min()), int(M.sum(-1).max())),
                    "descending": pairs is not None and bool((pairs[..., 0] > pairs[..., 1]).any())}
    return out


def _argmax_facts():
    out = {}
    for N, J, h, w, ld in K.ARGMAX_SHAPES:
        kinds = set()
        for r in range(K.argmax_rounds(N, J, h * w)):
            kinds |= set(K.argmax_input(N, J, h, w, ld, r)[2])
        assert kinds == set(K.argmax_kinds(h * w)), (N, J, h, w, ld)       # each planting appears at every shape where it fits
        out["argmax/%s" % ((N, J, h, w, ld),)] = {"N": N, "J": J, "HW": h * w, "ld": ld, "kinds": kinds}
    return out


@pytest.mark.parametrize("N,J,h,w,ld", K.ARGMAX_SHAPES)
def test_torch_max_on_the_cpu_returns_the_planted_index(N, J, h, w, ld):
    """The argmax tests' reference: the first NaN, else the first of the largest values (-0.0 == +0.0), whatever the padding holds."""
    import torch
    for r in range(K.argmax_rounds(N, J, h * w)):
        x, expect, _ = K.argmax_input(N, J, h, w, ld, r)
        assert torch.equal(torch.max(x[..., :J].permute(0, 3, 1, 2).reshape(N, J, -1), -1)[1], expect)


R_, A_ = "ransac", "argmax"
CHECKLIST = [
    ("ransac: NV = 31 fallback mask (1u << NV) - 1", R_, lambda f: f["NV"] == 31 and f["fallback"]),
    ("ransac: NV = 32 fallback mask 0xffffffff", R_, lambda f: f["NV"] == 32 and f["fallback"]),
    ("ransac: NV = 32 exhaustive, the 496-pair walk", R_, lambda f: f["NV"] == 32 and not f["pairs"]),
    ("ransac: 8 < NV < 32 exhaustive", R_, lambda f: 8 < f["NV"] < 32 and not f["pairs"]),
    ("ransac: bit 31 in a winning set", R_, lambda f: f["bit31_set"] and not f["fallback"]),
    ("ransac: bit 31 not in a winning set", R_, lambda f: f["bit31_clear"]),
    ("ransac: many outliers at NV = 32, small winning sets with bit 31", R_, lambda f: f["id"].startswith("outliers/") and f["sizes"][0] <= 8 and f["bit31_set"]),
    ("ransac: many outliers at NV = 32, winning sets without bit 31", R_, lambda f: f["id"].startswith("outliers/") and f["bit31_clear"]),
    ("ransac: invalid draws skipped among valid ones", R_, lambda f: f["mixed"]),
    ("ransac: a valid draw given as (larger, smaller)", R_, lambda f: f["descending"]),
    ("ransac: nbest == 0, every draw invalid", R_, lambda f: f["only_invalid"]),
    ("ransac: strictly larger -- a later set of equal size is not taken", R_, lambda f: f["rival"]),
    ("ransac: first-found wins under a reversed schedule", R_, lambda f: f["id"].startswith("ties/") and f["id"].endswith("/rev") and f["rival"]),
    ("ransac: B J = 1", R_, lambda f: f["problems"] == 1 and f["NV"] == 5),
    ("ransac: B J = 64", R_, lambda f: f["problems"] == 64),
    ("ransac: B J = 65", R_, lambda f: f["problems"] == 65),
    ("ransac: two workgroups with a ragged tail", R_, lambda f: 64 < f["problems"] < 128),
    ("ransac: a pairs stride no fixture has (n_iters = 3)", R_, lambda f: f["n_iters"] == 3 and f["problems"] > 1),
    ("ransac: out_inliers == NULL, n_iters ignored without pairs", R_, lambda f: f["id"].startswith("index/") and not f["pairs"]),
    ("argmax: J = 1 (ts = 1)", A_, lambda f: f["J"] == 1),
    ("argmax: even J (ts = J + 1)", A_, lambda f: f["J"] % 2 == 0 and f["J"] < 32),
    ("argmax: J = AM_JMAX = 32", A_, lambda f: f["J"] == 32),
    ("argmax: J = AM_JMAX with padding channels", A_, lambda f: f["J"] == 32 and f["ld"] > 32),
    ("argmax: H W = 1", A_, lambda f: f["HW"] == 1),
    ("argmax: H W below one wave", A_, lambda f: 1 < f["HW"] < 64),
    ("argmax: H W = 64", A_, lambda f: f["HW"] == 64),
    ("argmax: H W = one 256-pixel chunk", A_, lambda f: f["HW"] == 256),
    ("argmax: H W = 257", A_, lambda f: f["HW"] == 257),
    ("argmax: the maximum at a chunk boundary, alone and tied", A_, lambda f: {"p255", "p255_tie", "p256", "p256_tie"} <= f["kinds"]),
    ("argmax: padding channels of NaN, +inf and 1e30", A_, lambda f: f["ld"] >= f["J"] + 3),
    ("argmax: an all -inf map (the 0x7fffffff initial index)", A_, lambda f: "ninf" in f["kinds"]),
    ("argmax: an all-NaN map", A_, lambda f: "nan" in f["kinds"]),
    ("argmax: +inf twice", A_, lambda f: "pinf_twice" in f["kinds"]),
    ("argmax: -0.0 against +0.0, both orders", A_, lambda f: {"negzero_first", "poszero_first"} <= f["kinds"]),
    ("argmax: N far above the CU count", A_, lambda f: f["N"] >= 300),
]


def test_the_cases_reach_every_branch_of_the_checklist():
    """indices == NULL and keypoints == NULL are run at every argmax shape and the image smaller than the heatmap at ARGMAX_SCALED
    (test_gpu_ransac_kernels._argmax_case); the refinement on wide sets is the fixture test above."""
    facts = {R_: _ransac_facts(), A_: _argmax_facts()}
    reached = {label: [cid for cid, f in facts[fam].items() if pred(f)] for label, fam, pred in CHECKLIST}
    for label, ids in reached.items():
        print("%-66s %s" % (label, ", ".join(ids) if ids else "-- NOT REACHED"))
    assert not [label for label, ids in reached.items() if not ids]
    assert K.ARGMAX_SCALED in K.ARGMAX_SHAPES
