"""Camera model and multi-view helpers with the reference's names (mvn/utils/multiview.py).

Host geometry stays numpy fp64 exactly like the reference; the batched DLT runs in liblt_hip
(lt_triangulate_dlt), the batched RANSAC triangulation too (lt_triangulate_ransac)."""
import numpy as np
import torch

import lt_hip as H


class Camera:
    """Pinhole camera R (3x3), t (3x1), K (3x3) -- reference :5-52."""

    def __init__(self, R, t, K, dist=None, name=""):
        self.R = np.array(R, dtype=np.float64).copy()
        assert self.R.shape == (3, 3)
        self.t = np.array(t, dtype=np.float64).copy()
        assert self.t.size == 3
        self.t = self.t.reshape(3, 1)
        self.K = np.array(K, dtype=np.float64).copy()
        assert self.K.shape == (3, 3)
        self.dist = None if dist is None else np.array(dist).copy().flatten()
        self.name = name

    def update_after_crop(self, bbox):
        left, upper, _, _ = bbox
        self.K[0, 2] -= left
        self.K[1, 2] -= upper

    def update_after_resize(self, image_shape, new_image_shape):
        (h, w), (nh, nw) = image_shape, new_image_shape
        self.K[0, 0] *= nw / w
        self.K[1, 1] *= nh / h
        self.K[0, 2] *= nw / w
        self.K[1, 2] *= nh / h

    @property
    def extrinsics(self):
        return np.hstack([self.R, self.t])

    @property
    def projection(self):
        return self.K.dot(self.extrinsics)


def stack_cameras(cameras):
    """batch['cameras'] (list[NV] of list[B] of Camera-like objects with .R .t .K, datasets/utils.py:26)
    -> K (B,NV,3,3), R (B,NV,3,3), t (B,NV,3,1) fp64."""
    nv, bs = len(cameras), len(cameras[0])
    K = np.empty((bs, nv, 3, 3)); R = np.empty((bs, nv, 3, 3)); t = np.empty((bs, nv, 3, 1))
    for v in range(nv):
        for b in range(bs):
            c = cameras[v][b]
            K[b, v] = c.K; R[b, v] = c.R; t[b, v] = np.asarray(c.t).reshape(3, 1)
    return K, R, t


def resized_projections(K, R, t, image_shape, new_image_shape):
    """Vectorised ``update_after_resize`` + ``projection`` for stacked cameras (fp64)."""
    (h, w), (nh, nw) = image_shape, new_image_shape
    K = K.copy()
    K[..., 0, 0] *= nw / w
    K[..., 1, 1] *= nh / h
    K[..., 0, 2] *= nw / w
    K[..., 1, 2] *= nh / h
    return K @ np.concatenate([R, t], axis=-1)


def euclidean_to_homogeneous(points):
    if isinstance(points, np.ndarray):
        return np.hstack([points, np.ones((len(points), 1))])
    if torch.is_tensor(points):
        return torch.cat([points, points.new_ones((points.shape[0], 1))], dim=1)
    raise TypeError("Works only with numpy arrays and PyTorch tensors.")


def homogeneous_to_euclidean(points):
    if isinstance(points, np.ndarray):
        return (points.T[:-1] / points.T[-1]).T
    if torch.is_tensor(points):
        return points[:, :-1] / points[:, -1:]
    raise TypeError("Works only with numpy arrays and PyTorch tensors.")


def project_3d_points_to_image_plane_without_distortion(proj_matrix, points_3d, convert_back_to_euclidean=True):
    """Host helper (reference :89-110).  Inside the unprojection this projection is fused into
    lt_unproject_fwd; this stand-alone form is for small point sets (numpy, or torch on any device)."""
    both_np = isinstance(proj_matrix, np.ndarray) and isinstance(points_3d, np.ndarray)
    both_t = torch.is_tensor(proj_matrix) and torch.is_tensor(points_3d)
    if not (both_np or both_t):
        raise TypeError("Works only with numpy arrays and PyTorch tensors.")
    res = euclidean_to_homogeneous(points_3d) @ (proj_matrix.T if both_np else proj_matrix.t())
    return homogeneous_to_euclidean(res) if convert_back_to_euclidean else res


class _TriangulateFn(torch.autograd.Function):
    """lt_triangulate_dlt / lt_triangulate_dlt_bwd as one node: what autograd derives in the reference through torch.svd (:163) for the 2D
    points and the confidences (the projection matrices get no gradient, as there)."""

    @staticmethod
    def forward(ctx, P, pts, conf):
        B, NV, J = pts.shape[:3]
        out = torch.empty(B, J, 3, dtype=torch.float32, device=pts.device)
        H.check(H.lib().lt_triangulate_dlt(P.data_ptr(), pts.data_ptr(), H.ptr(conf), out.data_ptr(), B, NV, J, H.cur_stream()), "lt_triangulate_dlt")
        ctx.save_for_backward(P, pts, conf if conf is not None else torch.empty(0, device=pts.device))
        ctx.has_conf = conf is not None
        return out

    @staticmethod
    def backward(ctx, g):
        P, pts, conf = ctx.saved_tensors
        conf = conf if ctx.has_conf else None
        B, NV, J = pts.shape[:3]
        g = g.float().contiguous()
        gpts = torch.empty_like(pts)
        gconf = torch.empty_like(conf) if conf is not None else None
        H.check(H.lib().lt_triangulate_dlt_bwd(P.data_ptr(), pts.data_ptr(), H.ptr(conf), g.data_ptr(), gpts.data_ptr(), H.ptr(gconf), B, NV, J,
                                               H.cur_stream()), "lt_triangulate_dlt_bwd")
        return None, gpts, gconf


def triangulate_batch_of_points(proj_matricies_batch, points_batch, confidences_batch=None, view_mask=None):
    """Confidence-weighted DLT for every (sample, joint) in one launch (reference :171-183 loops B x J
    torch.svd calls).  proj (B,NV,3,4), points (B,NV,J,2), confidences (B,NV,J) -> (B,J,3) fp32.  Differentiable with respect to the
    points and the confidences when they require grad.

    view_mask: optional (B,NV) bool / uint8 tensor or array, non-zero = the view is there.  Sample b then gets the DLT of its valid views
    alone, bit for bit: a masked view's rows are given weight 0 with its point and matrix zeroed, and the kernel's QR skips a row of zeros, so
    NaN in a masked view cannot leak.  A sample needs two valid views (ValueError).  Inference only: NotImplementedError with inputs that
    require grad."""
    H.require_gpu(points_batch, "points_batch")
    P = proj_matricies_batch.to(points_batch.device, torch.float32).contiguous()
    pts = points_batch.float().contiguous()
    conf = None if confidences_batch is None else confidences_batch.float().contiguous()
    if view_mask is not None:
        from mvn.utils import op
        if torch.is_grad_enabled() and (pts.requires_grad or (conf is not None and conf.requires_grad)):
            raise NotImplementedError("triangulate_batch_of_points: view_mask is inference only (no masked backward); call it under torch.no_grad()")
        B, NV, J = pts.shape[:3]
        m = torch.from_numpy(op.view_mask_host(view_mask, B, NV, min_valid=2)).to(pts.device).bool()
        zero = torch.zeros((), dtype=torch.float32, device=pts.device)
        P = torch.where(m[:, :, None, None], P, zero)
        pts = torch.where(m[:, :, None, None], pts, zero)
        conf = torch.where(m[:, :, None], conf if conf is not None else torch.ones(B, NV, J, dtype=torch.float32, device=pts.device), zero)
    if torch.is_grad_enabled() and (pts.requires_grad or (conf is not None and conf.requires_grad)):
        return _TriangulateFn.apply(P, pts, conf)
    B, NV, J = pts.shape[:3]
    out = torch.empty(B, J, 3, dtype=torch.float32, device=pts.device)
    H.check(H.lib().lt_triangulate_dlt(P.data_ptr(), pts.data_ptr(), H.ptr(conf), out.data_ptr(), B, NV, J, H.cur_stream()),
            "lt_triangulate_dlt")
    return out


def triangulate_point_from_multiple_views_linear_torch(proj_matricies, points, confidences=None):
    """Single-point form of the above (reference :141-168)."""
    conf = None if confidences is None else confidences[None, :, None]
    return triangulate_batch_of_points(proj_matricies[None], points[None, :, None, :], conf)[0, 0]


def triangulate_point_from_multiple_views_linear(proj_matricies, points):
    """Host DLT of one point (reference :113-138), numpy fp64: rows x P[2] - P[0] and y P[2] - P[1] per view, the right singular
    vector of the smallest singular value, dehomogenised.  proj_matricies (N, 3, 4), points (N, 2) -> (3,)."""
    assert len(proj_matricies) == len(points)
    P = np.asarray(proj_matricies)
    p = np.asarray(points)
    A = np.zeros((2 * len(P), 4))
    for v in range(len(P)):
        A[2 * v] = p[v][0] * P[v][2, :] - P[v][0, :]
        A[2 * v + 1] = p[v][1] * P[v][2, :] - P[v][1, :]
    vh = np.linalg.svd(A, full_matrices=False)[2]
    return homogeneous_to_euclidean(vh[3, :])


def calc_reprojection_error_matrix(keypoints_3d, keypoints_2d_list, proj_matricies):
    """Half the pixel distance between each view's 2D point and the projection of each 3D point (reference :186-193): keypoints_3d
    (M, 3), keypoints_2d_list (N, 2) (one point per view, compared with every 3D point), proj_matricies (N, 3, 4) -> (M, N)."""
    cols = [0.5 * np.sqrt(np.sum((p2 - project_3d_points_to_image_plane_without_distortion(P, keypoints_3d)) ** 2, axis=1))
            for p2, P in zip(keypoints_2d_list, proj_matricies)]
    return np.vstack(cols).T


def triangulate_ransac_batch(proj_matricies_batch, points_batch, pairs=None, reprojection_error_epsilon=15.0, direct_optimization=True,
                             return_inliers=False):
    """RANSAC triangulation of every (sample, joint) in one lt_triangulate_ransac launch (reference triangulation.py:75-128 per point).
    proj (B, NV, 3, 4), points (B, NV, J, 2) integer pixel coordinates -> keypoints_3d (B, J, 3) fp32 [, inliers (B, J, NV) bool].
    ``pairs`` (B, J, n_iters, 2): the 2-view hypotheses to try in order (e.g. the reference's random draws); None = every pair in
    lexicographic order, which finds at least as large an inlier set as any n_iters draws (the one deliberate deviation from the
    reference: deterministic, no random numbers on the device)."""
    H.require_gpu(points_batch, "points_batch")
    dev = points_batch.device
    P = proj_matricies_batch.to(dev, torch.float32).contiguous()
    pts = points_batch.to(torch.int64).contiguous()
    B, NV, J = pts.shape[:3]
    if tuple(P.shape) != (B, NV, 3, 4) or tuple(pts.shape) != (B, NV, J, 2):
        raise ValueError("proj_matricies_batch (B, NV, 3, 4) and points_batch (B, NV, J, 2) expected, got %s and %s" % (tuple(P.shape), tuple(pts.shape)))
    n_iters = 0
    if pairs is not None:
        pairs = torch.as_tensor(pairs).to(dev, torch.int32).contiguous()
        n_iters = pairs.shape[2]
        if tuple(pairs.shape) != (B, J, n_iters, 2):
            raise ValueError("pairs must be (B, J, n_iters, 2), got %s" % (tuple(pairs.shape),))
    out = torch.empty(B, J, 3, dtype=torch.float32, device=dev)
    inl = torch.empty(B, J, NV, dtype=torch.uint8, device=dev) if return_inliers else None
    H.check(H.lib().lt_triangulate_ransac(P.data_ptr(), pts.data_ptr(), H.ptr(pairs), n_iters, float(reprojection_error_epsilon),
                                          int(bool(direct_optimization)), out.data_ptr(), H.ptr(inl), B, NV, J,
                                          torch.cuda.current_stream(dev).cuda_stream), "lt_triangulate_ransac")
    return (out, inl.bool()) if return_inliers else out
