"""Every branch of csrc/ransac.hip's two kernels, directly: ransac_kernel against tests/ransac_ref.py (numpy fp64: equal inlier masks,
points within 1e-6 per problem) and, for the Huber refinement on wide inlier sets, against the reference's own run with scipy
(tests/golden/ransac_branches.npz, tools/make_golden_ransac.py --only branches); hm_argmax_kernel against torch.max on the CPU, bit
for bit.  The case tables are built here without a GPU: tests/test_ransac_ref_cpu.py checks the conditions they rest on (every error at
least 1e-6 away from eps, finite points, the fp64 reference pinned to 1e-8) and that they reach every branch of its checklist."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from ransac_ref import ransac_ref, synth_problems

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 15.0
TOL = 1e-6            # |d|_inf <= TOL |X_ref|_inf per problem: the gate of test_gpu_ransac.py, applied to each problem on its own

# ---- the RANSAC case tables: id -> (P (B,NV,3,4) fp32, pts (B,NV,J,2) int64, pairs (B,J,n,2) int32 or None) ---------------------------------
WIDE = {"wide/nv%d" % nv: (nv, nv) for nv in (5, 16, 31, 32)}                       # id -> (NV, seed): B = 3, J = 23, 69 problems
OUTLIERS = {"outliers/nv%d" % nv: (nv, 40 + nv) for nv in (6, 16, 32)}              # B = 2, J = 9, up to NV - 2 outlier views
INVALID = {"invalid/nv%d" % nv: (nv, 70 + nv) for nv in (4, 31, 32)}                # B = 2, J = 7, n_iters = 7
INDEX = {"index/b%dj%d/%s" % (b, j, m): (b, j, m) for b, j in ((1, 1), (1, 64), (5, 13), (2, 40)) for m in ("exh", "replay")}   # NV = 5
TIES = {"ties/nv%d/%s" % (nv, s): (nv, s) for nv in (4, 6) for s in ("exh", "rev", "swap")}
TIE_SEED = {4: 4, 6: 6}
TIE_A, TIE_B = (-600.0, 300.0, 200.0), (700.0, -500.0, -300.0)
N_INVALID_ITERS = 7


def invalid_draws(NV):
    return [(-1, 2), (0, NV), (3, 3), (NV, NV), (2 ** 30, 1)]


def _invalid_pairs(NV, B, J, rs):
    """Per problem g: g % 3 == 1 only invalid draws (all five kinds among the seven); otherwise valid draws (either order) mixed with
    one to five invalid ones, another mix for every problem."""
    bad = invalid_draws(NV)
    pairs = np.zeros((B, J, N_INVALID_ITERS, 2), np.int32)
    for g in range(B * J):
        if g % 3 == 1:
            sched = [bad[i % 5] for i in rs.permutation(N_INVALID_ITERS)]
        else:
            nbad = 1 + g % 5
            sched = [bad[i] for i in rs.permutation(5)[:nbad]]
            sched += [tuple(int(v) for v in rs.choice(NV, 2, replace=False)) for _ in range(N_INVALID_ITERS - nbad)]
            sched = [sched[i] for i in rs.permutation(N_INVALID_ITERS)]
        pairs[g // J, g % J] = sched
    return pairs


def tie_clusters(NV):
    return list(range(NV // 2)), list(range(NV // 2, NV))


def tie_schedule(NV, sched):
    every = list(itertools.combinations(range(NV), 2))
    c0, c1 = tie_clusters(NV)
    return {"exh": None, "rev": every[::-1], "swap": [(c1[0], c1[1]), (c0[0], c0[1])]}[sched]


def tie_expected(NV, sched):
    """The first hypothesis whose set has the largest size wins: the exhaustive order meets the first cluster's pair first, the other two
    schedules the second cluster's."""
    m = np.zeros(NV, bool)
    m[tie_clusters(NV)[0 if sched == "exh" else 1]] = True
    return m


def _tie_problem(NV):
    """Views [0, NV/2) see point A, the others point B (projected, rounded to pixels): two inlier sets of equal size."""
    P, _ = synth_problems(np.random.RandomState(TIE_SEED[NV]), 1, NV, 1)
    pts = np.zeros((1, NV, 1, 2), np.int64)
    for c, X in zip(tie_clusters(NV), (TIE_A, TIE_B)):
        for v in c:
            q = P[0, v].astype(np.float64) @ np.append(X, 1.0)
            pts[0, v, 0] = np.round(q[:2] / q[2]).astype(np.int64)
    return P, pts


def all_tables():
    return list(WIDE) + list(OUTLIERS) + list(INVALID) + list(TIES) + list(INDEX)


@functools.lru_cache(maxsize=None)
def table(tid):
    if tid in WIDE:
        nv, seed = WIDE[tid]
        return synth_problems(np.random.RandomState(seed), 3, nv, 23) + (None,)
    if tid in OUTLIERS:
        nv, seed = OUTLIERS[tid]
        return synth_problems(np.random.RandomState(seed), 2, nv, 9, max_outliers=nv - 2) + (None,)
    if tid in INVALID:
        nv, seed = INVALID[tid]
        rs = np.random.RandomState(seed)
        return synth_problems(rs, 2, nv, 7) + (_invalid_pairs(nv, 2, 7, rs),)
    if tid in TIES:
        nv, sched = TIES[tid]
        s = tie_schedule(nv, sched)
        return _tie_problem(nv) + (None if s is None else np.array(s, np.int32)[None, None],)
    B, J, mode = INDEX[tid]
    rs = np.random.RandomState(500 + 10 * B + J)
    P, pts = synth_problems(rs, B, 5, J)
    pairs = None
    if mode == "replay":                                # n_iters = 3: a stride of `pairs` no fixture has
        pairs = np.array([[[rs.choice(5, 2, replace=False) for _ in range(3)] for _ in range(J)] for _ in range(B)], np.int32)
    return P, pts, pairs


@functools.lru_cache(maxsize=None)
def reference(tid):
    """tests/ransac_ref.py on every problem of a table, once: X (B,J,3), masks (B,J,NV), eps margins, self-uncertainties (B,J) and the
    per-problem facts (skipped draws, fallback taken, set sizes)."""
    P, pts, pairs = table(tid)
    B, NV, J = pts.shape[:3]
    X, M, mg, un = np.zeros((B, J, 3)), np.zeros((B, J, NV), bool), np.zeros((B, J)), np.zeros((B, J))
    facts = [[{} for _ in range(J)] for _ in range(B)]
    for b in range(B):
        for j in range(J):
            X[b, j], M[b, j], mg[b, j], un[b, j] = ransac_ref(P[b], pts[b, :, j], None if pairs is None else pairs[b, j], EPS, facts[b][j])
    for a in (X, M, mg, un):
        a.setflags(write=False)
    return X, M, mg, un, facts


def _gpu(tid, eps=EPS, direct=False, pairs="table", return_inliers=True):
    from mvn.utils import multiview
    P, pts, tp = table(tid)
    pairs = tp if isinstance(pairs, str) else pairs
    return multiview.triangulate_ransac_batch(torch.from_numpy(P).to(DEV), torch.from_numpy(pts).to(DEV),
                                              None if pairs is None else torch.from_numpy(pairs), eps, direct, return_inliers=return_inliers)


def _check_table(tid):
    """Masks equal, every problem's point within TOL of the fp64 reference; the worst ratio goes to the parity report."""
    kp, inl_d = _gpu(tid)
    X, M = reference(tid)[:2]
    inl = inl_d.cpu().numpy()
    assert np.array_equal(inl, M), "%s: inlier sets differ at %s" % (tid, np.argwhere((inl != M).any(-1)))
    d = np.abs(kp.cpu().double().numpy() - X).max(-1) / np.abs(X).max(-1)
    record("ransac-kernels/%s/pre-refinement points, max over problems of |d|_inf / |X_ref|_inf" % tid, float(d.max()))
    assert (d <= TOL).all(), "%s: problems %s off by %s" % (tid, np.argwhere(~(d <= TOL)), d[~(d <= TOL)])
    return kp, inl_d


@pytest.mark.parametrize("tid", list(WIDE) + list(OUTLIERS))
def test_wide_problems_exhaustive(tid):
    """a. NV up to 32 (bit 31 of the mask, the 496-pair walk), 69 problems = two workgroups with a ragged tail; with up to NV - 2
    outlier views the winning sets are small and bit 31 is in some and not in others."""
    _check_table(tid)


@pytest.mark.parametrize("tid", list(INVALID))
def test_invalid_draws_are_skipped_and_no_valid_draw_means_all_views(tid):
    """b. (-1, 2), (0, NV), (3, 3), (NV, NV), (2^30, 1) among valid draws; problems with no valid draw fall back to every view and give,
    bit for bit, the all-inlier point (eps = 1e30, the identity test_gpu_ransac.py holds against lt_triangulate_dlt)."""
    kp, inl = _check_table(tid)
    fallback = np.array([[f["fallback"] for f in row] for row in reference(tid)[4]])
    assert fallback.any() and not fallback.all()
    assert inl.cpu().numpy()[fallback].all()
    kp_all, inl_all = _gpu(tid, eps=1e30, pairs=None)
    assert inl_all.all()
    fb = torch.from_numpy(fallback)
    assert torch.equal(kp.cpu()[fb].view(torch.int32), kp_all.cpu()[fb].view(torch.int32))


@pytest.mark.parametrize("tid", list(TIES))
def test_first_found_wins_among_sets_of_equal_size(tid):
    """c. Two clusters of views that agree on two different points: whichever cluster's pair the schedule meets first keeps the set."""
    _, inl = _check_table(tid)
    assert np.array_equal(inl[0, 0].cpu().numpy(), tie_expected(*TIES[tid])), inl[0, 0]


@pytest.mark.parametrize("tid", list(INDEX))
def test_every_problem_of_a_batch_equals_that_problem_launched_alone(tid):
    """d. The strides of proj, points, pairs and both outputs: problem (b, j) of the batched launch is, bit for bit, the same problem as
    a B = 1, J = 1 launch -- with and without the inlier output, and (pairs = NULL) whatever n_iters says."""
    from mvn.utils import multiview
    P, pts, pairs = table(tid)
    B, NV, J = pts.shape[:3]
    kp_b, inl_b = _check_table(tid)
    Pd, ptsd = torch.from_numpy(P).to(DEV), torch.from_numpy(pts).to(DEV)
    prd = None if pairs is None else torch.from_numpy(pairs).to(DEV)
    kp_noinl = multiview.triangulate_ransac_batch(Pd, ptsd, prd, EPS, False)            # out_inliers = NULL
    singles = [multiview.triangulate_ransac_batch(Pd[b:b + 1], ptsd[b:b + 1, :, j:j + 1], None if prd is None else prd[b:b + 1, j:j + 1], EPS, False,
                                                  return_inliers=True) for b in range(B) for j in range(J)]
    kp_s = torch.cat([s[0] for s in singles]).reshape(B, J, 3)
    inl_s = torch.cat([s[1] for s in singles]).reshape(B, J, NV)
    raw = []
    if pairs is None:                                   # n_iters is ignored without a schedule
        for n_iters in (0, 7):
            o = torch.empty(B, J, 3, device=DEV)
            H.check(H.lib().lt_triangulate_ransac(Pd.data_ptr(), ptsd.data_ptr(), None, n_iters, EPS, 0, o.data_ptr(), None, B, NV, J, H.cur_stream()),
                    "lt_triangulate_ransac")
            raw.append(o)
    torch.cuda.synchronize()
    bits = lambda t: t.cpu().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(kp_b), bits(kp_s)), (bits(kp_b) != bits(kp_s)).any(-1).nonzero()
    assert torch.equal(inl_b.cpu(), inl_s.cpu())
    assert torch.equal(bits(kp_b), bits(kp_noinl))
    for o in raw:
        assert torch.equal(bits(kp_b), bits(o))


@pytest.mark.parametrize("nv", [16, 32])
def test_huber_refinement_on_wide_inlier_sets(golden_dir, nv):
    """e. Inlier sets of up to 32 views (up to 33 Levenberg-Marquardt starts per lane, the `front` mask over 32 views), residuals in both
    of Huber's regimes, against the reference's triangulate_ransac + scipy: the gates of test_gpu_ransac.py, every problem well posed."""
    from mvn.utils import multiview
    from test_gpu_ransac import _check_ransac
    g = np.load(os.path.join(golden_dir, "ransac_branches.npz"))
    tag = "nv%d_d1" % nv
    P, pts = torch.from_numpy(g[tag + "_P"]).to(DEV), torch.from_numpy(g[tag + "_pts"]).to(DEV)
    kp_pre = multiview.triangulate_ransac_batch(P, pts, None, EPS, False).cpu().double().numpy()
    kp, inl = multiview.triangulate_ransac_batch(P, pts, None, EPS, True, return_inliers=True)
    r = lambda k: g["%s_exh_%s" % (tag, k)]  # noqa: E731
    assert r("well").all()
    _check_ransac("ransac-kernels/refine/%s" % tag, g[tag + "_P"], g[tag + "_pts"], kp_pre, kp.cpu().double().numpy(), inl.cpu().numpy(),
                  r("pre"), r("post"), r("inl"), r("cost"), r("well"), 1)


# ---- hm_argmax_kernel -------------------------------------------------------------------------------------------------------------------------
ARGMAX_SHAPES = [(3, 1, 8, 8, 1), (3, 1, 1, 1, 4), (2, 2, 7, 9, 2), (2, 16, 16, 16, 16), (2, 32, 1, 257, 32), (2, 32, 24, 24, 40), (300, 3, 4, 4, 3),
                 (2, 17, 16, 32, 24)]
ARGMAX_SCALED = (2, 16, 16, 16, 16)      # also run with an image smaller than the heatmap on y
PAD_VALUES = (float("nan"), float("inf"), 1e30)


def argmax_kinds(HW):
    """The plantings that fit a map of HW pixels."""
    k = ["last", "ninf", "nan"]
    if HW >= 2:
        k += ["last_tie", "pinf_twice", "negzero_first", "poszero_first"]
    if HW > 255:
        k += ["p255", "p255_tie"]
    if HW > 256:
        k += ["p256", "p256_tie"]
    return k


def argmax_rounds(N, J, HW):
    """Maps take the kinds in turn; a shape with fewer maps than kinds is run again with the turn moved on until every kind has had a map."""
    k = len(argmax_kinds(HW))
    return -(-k // (N * J))


def argmax_input(N, J, h, w, ld, rnd):
    """-> x (N, h, w, ld) fp32 NHWC, the index every map's maximum was planted at (N, J), the kind of every map."""
    HW = h * w
    g = torch.Generator().manual_seed(N * 1000 + J * 10 + h + 7 * rnd)
    x = torch.round(torch.randn(N, HW, ld, generator=g) * 4) / 4          # plenty of exact ties below the planted values
    kinds = argmax_kinds(HW)
    expect = torch.zeros(N, J, dtype=torch.int64)
    used = []
    for n in range(N):
        for j in range(J):
            m = n * J + j
            kind = kinds[(m + rnd * N * J) % len(kinds)]
            used.append(kind)
            col = x[n, :, j]
            early, late = HW // 3, HW - 1
            if kind == "last":
                col[late] = 100.0; e = late
            elif kind == "last_tie":
                col[late] = 100.0; col[0] = 100.0; e = 0
            elif kind in ("p255", "p256"):
                e = int(kind[1:]); col[e] = 100.0
            elif kind == "p255_tie":
                col[255] = 100.0; col[3] = 100.0; e = 3
            elif kind == "p256_tie":                    # the tie straddles the chunk boundary
                col[256] = 100.0; col[255] = 100.0; e = 255
            elif kind == "ninf":
                col[:] = float("-inf"); e = 0
            elif kind == "nan":
                col[:] = float("nan"); e = 0
            elif kind == "pinf_twice":
                col[early] = float("inf"); col[late] = float("inf"); e = early
            else:                                       # the two zeros are the only non-negative values and compare equal
                col[:] = -(col.abs() + 1.0)
                col[early], col[late] = (-0.0, 0.0) if kind == "negzero_first" else (0.0, -0.0)
                e = early
            expect[n, j] = e
    for c in range(J, ld):                              # padding channels must neither win nor leak into the NCHW copy
        x[:, :, c] = PAD_VALUES[(c - J) % 3]
    return x.reshape(N, h, w, ld).contiguous(), expect, used


def _argmax_launch(xd, N, J, h, w, ld, Hi, Wi, want_idx=True, want_kp=True):
    y = torch.full((N, J, h, w), -7.0, device=DEV)
    idx = torch.full((N, J), -7, dtype=torch.int64, device=DEV) if want_idx else None
    kp = torch.full((N, J, 2), -7, dtype=torch.int64, device=DEV) if want_kp else None
    H.check(H.lib().lt_heatmap_argmax_nchw_f32(xd.data_ptr(), ld, y.data_ptr(), H.ptr(idx), H.ptr(kp), N, J, h, w, Hi, Wi, H.cur_stream()),
            "lt_heatmap_argmax_nchw_f32")
    return y, idx, kp


def _argmax_case(N, J, h, w, ld, image=None):
    Hi, Wi = image or (4 * h, 4 * w + 3)                # default: a non-integer ratio on x
    for rnd in range(argmax_rounds(N, J, h * w)):
        x, expect, _ = argmax_input(N, J, h, w, ld, rnd)
        xd = x.to(DEV)
        y, idx, kp = _argmax_launch(xd, N, J, h, w, ld, Hi, Wi)
        y_a, _, kp_a = _argmax_launch(xd, N, J, h, w, ld, Hi, Wi, want_idx=False)        # indices = NULL
        y_b, idx_b, _ = _argmax_launch(xd, N, J, h, w, ld, Hi, Wi, want_kp=False)        # keypoints = NULL
        torch.cuda.synchronize()
        ref_hm = x[..., :J].permute(0, 3, 1, 2).contiguous()
        _, ref_idx = torch.max(ref_hm.view(N, J, -1), -1)
        assert torch.equal(ref_idx, expect)             # torch.max on the CPU: the first NaN, else the first of the largest
        ref_kp = torch.zeros(N, J, 2, dtype=torch.int64)      # reference triangulation.py:49-51
        ref_kp[..., 0] = (ref_idx % w) * (Wi / w)
        ref_kp[..., 1] = (ref_idx // w) * (Hi / h)
        bits = lambda t: t.cpu().view(torch.int32)  # noqa: E731
        assert torch.equal(bits(y), ref_hm.view(torch.int32))
        assert torch.equal(idx.cpu(), ref_idx), (idx.cpu() != ref_idx).nonzero()
        assert torch.equal(kp.cpu(), ref_kp)
        assert torch.equal(bits(y_a), bits(y)) and torch.equal(kp_a, kp)
        assert torch.equal(bits(y_b), bits(y)) and torch.equal(idx_b, idx)


@pytest.mark.parametrize("N,J,h,w,ld", ARGMAX_SHAPES)
def test_heatmap_argmax_branches(N, J, h, w, ld):
    """f. J = 1, even J, J = 32; H W below a wave, 64, one chunk, 257; padding channels full of NaN, +inf and 1e30; N far above the CU
    count; per map a maximum at a chunk boundary or the last pixel (alone and tied), all -inf, all NaN, +inf twice, -0.0 against +0.0."""
    _argmax_case(N, J, h, w, ld)


def test_heatmap_argmax_with_an_image_smaller_than_the_heatmap():
    N, J, h, w, ld = ARGMAX_SCALED
    _argmax_case(N, J, h, w, ld, image=(3 * h // 4, 5 * w // 2 + 1))       # scale 3/4 on y, 41/16 on x
