"""RANSAC triangulation restated in plain numpy fp64: the reference every direct test of csrc/ransac.hip's ransac_kernel compares with
(tests/test_ransac_ref_cpu.py pins it to the reference's own results in tests/golden/ransac_ops.npz), the Huber cost of scipy's
least_squares(loss='huber') and the synthetic problems the fixtures (tools/make_golden_ransac.py) and the tests share.  Numpy only."""
import itertools

import numpy as np


def dlt_rows(P, pts):
    """The rows of multiview.triangulate_point_from_multiple_views_linear: x P[2] - P[0], y P[2] - P[1] per view, (2n, 4) fp64."""
    P = np.asarray(P, np.float64)
    p = np.asarray(pts, np.float64)
    A = np.zeros((2 * len(P), 4))
    for v in range(len(P)):
        A[2 * v] = p[v][0] * P[v][2, :] - P[v][0, :]
        A[2 * v + 1] = p[v][1] * P[v][2, :] - P[v][1, :]
    return A


def dlt_point(A):
    vh = np.linalg.svd(A, full_matrices=False)[2]
    return vh[3, :3] / vh[3, 3]


def reproj_errors(P, pts, X):
    """0.5 |p_v - pi_v(X)| for every view (multiview.calc_reprojection_error_matrix for one point)."""
    q = np.append(X, 1.0) @ np.asarray(P, np.float64).transpose(0, 2, 1)          # (NV, 3)
    with np.errstate(all="ignore"):
        return 0.5 * np.sqrt(np.sum((np.asarray(pts, np.float64) - q[:, :2] / q[:, 2:]) ** 2, axis=1))


def ransac_ref(P, pts, pairs=None, eps=15.0, facts=None):
    """One problem: P (NV, 3, 4) fp32, pts (NV, 2) integer, pairs (n, 2) = the 2-view hypotheses in order or None = every pair in
    lexicographic order -> (point (3,), inlier mask (NV,) bool, eps_margin, self_uncertainty).

      * a draw with an index outside [0, NV) or two equal indices is skipped;
      * a hypothesis is the DLT (np.linalg.svd of the 4 x 4 matrix A) of the pair's two views, taken in view order; its inlier set is
        the pair plus every view with error 0.5 |p - pi(X)| < eps (a NaN compares false);
      * a set is kept only when strictly larger than the best so far; no valid draw at all: the set is every view;
      * the point is the DLT over the inlier set.
    eps_margin: min |error - eps| over every finite comparison made.  self_uncertainty: the relative change of the point when the SVD
    is given A's rows in reverse order (how far fp64 itself pins the point down).
    facts (a dict, filled when given): "skipped" draws, "fallback" taken, "sizes" of the valid hypotheses' sets, "rival": a later
    hypothesis gave a different set as large as the one kept."""
    NV = len(pts)
    sched = itertools.combinations(range(NV), 2) if pairs is None else [(int(a), int(b)) for a, b in np.asarray(pairs).reshape(-1, 2)]
    rows = dlt_rows(P, pts).reshape(NV, 2, 4)
    best, margin, skipped, sizes, rival = None, np.inf, 0, [], False
    for s0, s1 in sched:
        if not (0 <= s0 < NV and 0 <= s1 < NV) or s0 == s1:
            skipped += 1
            continue
        pair = sorted((s0, s1))
        err = reproj_errors(P, pts, dlt_point(rows[pair].reshape(4, 4)))
        fin = err[np.isfinite(err)]
        if fin.size:
            margin = min(margin, float(np.abs(fin - eps).min()))
        s = err < eps                                  # NaN: False
        s[pair] = True
        sizes.append(int(s.sum()))
        if best is None or s.sum() > best.sum():
            best = s
        elif s.sum() == best.sum() and not np.array_equal(s, best):
            rival = True
    fallback = best is None
    if fallback:
        best = np.ones(NV, bool)
    A = rows[best].reshape(-1, 4)
    X = dlt_point(A)
    Xr = dlt_point(A[::-1])
    with np.errstate(all="ignore"):
        unc = float(np.abs(X - Xr).max() / np.abs(X).max())
    if facts is not None:
        facts.update(skipped=skipped, fallback=fallback, sizes=sizes, rival=rival)
    return X, best, margin, unc


def huber_residuals(P, pts, X, inl):
    """z_v = r_v^2, r_v = 1/2 |p_v - pi_v(X)|, over the inlier views: z <= 1 is Huber's quadratic regime, z > 1 the linear one."""
    z = []
    for v in np.nonzero(inl)[0]:
        q = P[v].astype(np.float64) @ np.append(X, 1.0)
        z.append(0.25 * float(np.sum((pts[v] - q[:2] / q[2]) ** 2)))
    return np.array(z)


def huber_cost(P, pts, X, inl):
    """scipy's least_squares(loss='huber', f_scale=1) cost 0.5 sum_v rho(r_v^2), r_v = 1/2 |p_v - pi_v(X)| over the inlier views."""
    c = 0.0
    for z in huber_residuals(P, pts, X, inl):
        c += z if z <= 1 else 2 * np.sqrt(z) - 1
    return 0.5 * c


def synth_problems(rs, B, NV, J, image=384, max_outliers=None):
    """Cameras on a ring of ~5 m around a 2 m volume, realistic K for 384^2 crops, joints projected and quantised to the 4-pixel grid
    of argmax x 4, 0 to max_outliers (default min(2, NV - 2)) outlier views per problem."""
    if max_outliers is None:
        max_outliers = min(2, NV - 2)
    P = np.zeros((B, NV, 3, 4), np.float32)
    pts = np.zeros((B, NV, J, 2), np.int64)
    for b in range(B):
        for v in range(NV):
            phi = 2 * np.pi * v / NV + rs.uniform(-0.2, 0.2)
            C = np.array([5000 * np.cos(phi), 5000 * np.sin(phi), rs.uniform(800, 1800)])
            fwd = -C / np.linalg.norm(C)
            right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            f = rs.uniform(600, 900)
            K = np.array([[f, 0, image / 2 + rs.uniform(-8, 8)], [0, f * rs.uniform(0.99, 1.01), image / 2 + rs.uniform(-8, 8)], [0, 0, 1]])
            P[b, v] = (K @ np.concatenate([R, (-R @ C)[:, None]], 1)).astype(np.float32)
        X = rs.uniform(-1000, 1000, (J, 3))
        for v in range(NV):
            q = np.concatenate([X, np.ones((J, 1))], 1) @ P[b, v].astype(np.float64).T
            pts[b, v] = (np.round(q[:, :2] / q[:, 2:] / 4) * 4).astype(np.int64)
        for j in range(J):
            nout = rs.randint(0, max_outliers + 1)
            for v in rs.choice(NV, nout, replace=False):
                pts[b, v, j] = rs.randint(0, image // 4, 2) * 4
    return P, pts
