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


def triangulate_batch_of_points(proj_matricies_batch, points_batch, confidences_batch=None, view_mask=None, masked_backward=False, view_counts=None):
    """Confidence-weighted DLT for every (sample, joint) in one launch (reference :171-183 loops B x J
    torch.svd calls).  proj (B,NV,3,4), points (B,NV,J,2), confidences (B,NV,J) -> (B,J,3) fp32.  Differentiable with respect to the
    points and the confidences when they require grad.

    view_mask: optional (B,NV) bool / uint8 tensor or array, non-zero = the view is there.  Sample b then gets the DLT of its valid views
    alone, bit for bit: a masked view's rows are given weight 0 with its point and matrix zeroed, and the kernel's QR skips a row of zeros, so
    NaN in a masked view cannot leak.  A sample needs two valid views (ValueError).  Inference only by default: NotImplementedError with
    inputs that require grad.  masked_backward=True opts into the differentiable masked DLT: the same construction in front of
    lt_triangulate_dlt / lt_triangulate_dlt_bwd, whose gradient for a row of zeros is zero and which torch.where routes back as zero -- a masked
    view's points and confidences get exactly zero gradient, the valid ones what the DLT of the valid views alone gives.

    view_counts: a ragged batch.  proj (T,3,4), points (T,J,2) and confidences (T,J) hold the views of all samples, sample 0's first; view_counts the B
    counts (2..32 each, summing to T) -> (B,J,3): sample b is the DLT of its own rows alone, bit for bit.  This is the padded route, not a ragged
    kernel (the ragged DLT exists only inside lt_alg_tail_ragged_fwd, behind its confidence normalisation): the rows are scattered into a zero-filled
    (B, largest count) batch on the device and lt_triangulate_dlt runs on that, as the view_mask path above does -- the kernel's QR skips a row of zeros.  Inference only: NotImplementedError with inputs that require grad,
    and together with view_mask (drop the view from the batch instead)."""
    if view_counts is not None:
        from mvn.utils import op
        if view_mask is not None:
            raise NotImplementedError("triangulate_batch_of_points: view_counts with view_mask; drop the missing views from the ragged batch instead of masking them")
        if torch.is_grad_enabled() and (points_batch.requires_grad or (confidences_batch is not None and confidences_batch.requires_grad)):
            raise NotImplementedError("triangulate_batch_of_points: view_counts is inference only (no ragged backward); call it under torch.no_grad(), or pad "
                                      "the batch and use view_mask with masked_backward=True")
        if points_batch.dim() != 3:
            raise ValueError("triangulate_batch_of_points: with view_counts the points are (T, J, 2), got %s" % (tuple(points_batch.shape),))
        T, J = points_batch.shape[:2]
        counts, base, _ = op.view_counts_host(view_counts, T, min_views=2)
        if tuple(proj_matricies_batch.shape) != (T, 3, 4):
            raise ValueError("triangulate_batch_of_points: with view_counts proj_matricies are (T, 3, 4) = (%d, 3, 4), got %s" % (T, tuple(proj_matricies_batch.shape)))
        H.require_gpu(points_batch, "points_batch")
        dev = points_batch.device
        B, top = counts.size, int(counts.max())
        slot = torch.from_numpy(np.concatenate([b * top + np.arange(n) for b, n in enumerate(counts)]).astype(np.int64)).to(dev)
        P = torch.zeros(B * top, 3, 4, dtype=torch.float32, device=dev).index_copy_(0, slot, proj_matricies_batch.to(dev, torch.float32))
        pts = torch.zeros(B * top, J, 2, dtype=torch.float32, device=dev).index_copy_(0, slot, points_batch.float())
        src = torch.ones(T, J, dtype=torch.float32, device=dev) if confidences_batch is None else confidences_batch.float()
        conf = torch.zeros(B * top, J, dtype=torch.float32, device=dev).index_copy_(0, slot, src)
        out = torch.empty(B, J, 3, dtype=torch.float32, device=dev)
        H.check(H.lib().lt_triangulate_dlt(P.data_ptr(), pts.data_ptr(), conf.data_ptr(), out.data_ptr(), B, top, J, H.cur_stream()), "lt_triangulate_dlt")
        return out
    H.require_gpu(points_batch, "points_batch")
    P = proj_matricies_batch.to(points_batch.device, torch.float32).contiguous()
    pts = points_batch.float().contiguous()
    conf = None if confidences_batch is None else confidences_batch.float().contiguous()
    if view_mask is not None:
        from mvn.utils import op
        if not masked_backward and torch.is_grad_enabled() and (pts.requires_grad or (conf is not None and conf.requires_grad)):
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


def triangulate_batch_of_points_with_stats(proj_matricies_batch, points_batch, confidences_batch=None, covariances_2d=None, view_mask=None):
    """triangulate_batch_of_points plus the two quality measures of a triangulated joint (lt_triangulate_dlt_stats; ``triangulation_stats`` states them
    in numpy fp64).  covariances_2d: (B,NV,J,2,2) -- or (B,NV,J,3) as {xx, xy, yy} -- the 2D covariance of every point in image px^2, e.g. the
    ``covariance_2d`` of an AlgKeypointStats or of ``op.integrate_tensor_2d_with_stats`` scaled to image pixels.  Returns (keypoints_3d (B,J,3),
    reprojection_error (B,NV,J) px, covariance (B,J,3,3)): the joints are bit for bit triangulate_batch_of_points' and differentiable in the same way; the
    statistics carry no gradient.  view_mask as there (inference only; here the kernel skips masked views, whose reprojection_error is NaN)."""
    H.require_gpu(points_batch, "points_batch")
    if covariances_2d is None:
        raise ValueError("triangulate_batch_of_points_with_stats: covariances_2d is required ((B, NV, J, 2, 2) or (B, NV, J, 3))")
    dev = points_batch.device
    P = proj_matricies_batch.to(dev, torch.float32).contiguous()
    pts = points_batch.detach().float().contiguous()
    conf = None if confidences_batch is None else confidences_batch.detach().float().contiguous()
    B, NV, J = pts.shape[:3]
    cov = covariances_2d.detach().to(dev, torch.float32)
    if tuple(cov.shape) == (B, NV, J, 2, 2):
        cov = cov.reshape(B, NV, J, 4)[..., [0, 1, 3]]
    if tuple(cov.shape) != (B, NV, J, 3):
        raise ValueError("covariances_2d must be (B, NV, J, 2, 2) or (B, NV, J, 3) = (%d, %d, %d, ...), got %s" % (B, NV, J, tuple(covariances_2d.shape)))
    cov = cov.contiguous()
    mask = None
    needs_grad = torch.is_grad_enabled() and (points_batch.requires_grad or (confidences_batch is not None and confidences_batch.requires_grad))
    if view_mask is not None:
        from mvn.utils import op
        if needs_grad:
            raise NotImplementedError("triangulate_batch_of_points_with_stats: view_mask is inference only (no masked backward); call it under torch.no_grad()")
        mask = torch.from_numpy(op.view_mask_host(view_mask, B, NV, min_valid=2)).to(dev)
    out = torch.empty(B, J, 3, dtype=torch.float32, device=dev)
    err = torch.empty(B, NV, J, dtype=torch.float32, device=dev)
    c3 = torch.empty(B, J, 6, dtype=torch.float32, device=dev)
    H.check(H.lib().lt_triangulate_dlt_stats(P.data_ptr(), pts.data_ptr(), H.ptr(conf), cov.data_ptr(), H.ptr(mask), out.data_ptr(), err.data_ptr(), c3.data_ptr(),
                                             B, NV, J, H.cur_stream()), "lt_triangulate_dlt_stats")
    if needs_grad:          # the same joints as an autograd node
        out = triangulate_batch_of_points(proj_matricies_batch, points_batch, confidences_batch)
    return out, err, c3[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(B, J, 3, 3)


# ---- the numpy fp64 statement of the algebraic joints' statistics (CPU only) ------------------------------------------------------------------------
def heatmap_stats_2d(heatmaps, mult=1.0, softmax=True, coords=None):
    """The numpy fp64 statement of liblt_hip's ``lt_softargmax2d_stats_fwd`` (op.integrate_tensor_2d_with_stats).

    heatmaps (..., h, w): the raw fp32 heatmaps; x = fp32(mult * heatmaps), the one rounding the kernel makes.  coords (..., 2): the (x, y) the soft-argmax
    RETURNED (fp32) -- the moments are taken about them, never as E[c c^T] - mu mu^T; None: the fp64 soft-argmax of x, rounded to fp32.  Per heatmap, over
    the flat index i = y * w + x with pixel centres c_i = (x, y):
      softmax:  p = softmax(x);  peak_index = the smallest i with x_i maximal;  peak = p[peak_index];  mass = 1
      ReLU:     w = relu(x);  mass = sum w;  peak_index as above, on x;  peak = w[peak_index] / mass;  p = w / mass;  mass == 0: peak = 0, covariance = 0
      covariance = sum_i p_i (c_i - coords)(c_i - coords)^T, heatmap pixels^2
    Returns (peak, peak_index (int64), mass, covariance (..., 2, 2)) as fp64 arrays."""
    hm = np.asarray(heatmaps, dtype=np.float32)
    lead, (h, w) = hm.shape[:-2], hm.shape[-2:]
    x = (np.float32(mult) * hm).astype(np.float32).reshape(-1, h * w).astype(np.float64)
    idx = x.argmax(axis=1)                                  # numpy: the first of equal maxima
    if softmax:
        p = np.exp(x - x.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        mass = np.ones(len(x))
    else:
        wgt = np.maximum(x, 0.0)
        mass = wgt.sum(axis=1)
        some = mass > 0
        p = np.where(some[:, None], wgt / np.where(some, mass, 1.0)[:, None], 0.0)
    c = np.stack([np.tile(np.arange(w, dtype=np.float64), h), np.repeat(np.arange(h, dtype=np.float64), w)], axis=1)          # (h * w, 2) as (x, y)
    centre = (p @ c).astype(np.float32) if coords is None else np.asarray(coords, dtype=np.float32).reshape(-1, 2)
    centre = np.where((mass > 0)[:, None], centre.astype(np.float64), 0.0)
    d = c[None] - centre[:, None, :]
    cov = np.einsum("ni,nir,nis->nrs", p, d, d)
    cov[:, 1, 0] = cov[:, 0, 1]
    peak = p[np.arange(len(x)), idx]
    return peak.reshape(lead), idx.reshape(lead), mass.reshape(lead), cov.reshape(lead + (2, 2))


# ---- the numpy fp64 statement of the 2D heatmap targets, the heatmap loss and the soft-argmax backward with both gradients (CPU only) -----------------
def render_gaussians_2d(points, sigmas, image_shape, normalize=True):
    """The numpy fp64 statement of liblt_hip's ``lt_render_gaussians_2d`` (op.render_points_as_2d_gaussians; the reference's op.py:169-196).

    points (n, 2) as (x, y) in heatmap pixels, sigmas (n, 2), image_shape (h, w) -> (n, h, w) fp64:
      G[i, y, x] = exp(-((x - px)^2 / sx^2 + (y - py)^2 / sy^2) / 2) / norm,   norm = 2 pi sx sx if normalize else 1
    sigma_x TWICE in the normaliser: what gaussian_2d_pdf of the reference computes (op.py:172), kept."""
    pts, sg = np.asarray(points, dtype=np.float64).reshape(-1, 2), np.asarray(sigmas, dtype=np.float64).reshape(-1, 2)
    h, w = image_shape
    x, y = np.arange(w, dtype=np.float64)[None, None, :], np.arange(h, dtype=np.float64)[None, :, None]
    px, py, sx, sy = (a[:, None, None] for a in (pts[:, 0], pts[:, 1], sg[:, 0], sg[:, 1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.exp(-((x - px) ** 2 / sx ** 2 + (y - py) ** 2 / sy ** 2) / 2)
        return g / (2 * np.pi * sx * sx) if normalize else g


def heatmap_mse_2d(pred, points, sigmas, validity=None, normalize=False):
    """The numpy fp64 statement of liblt_hip's ``lt_heatmap_mse_fwd`` (loss.HeatmapMSELoss).

    pred (NJ, h, w), points / sigmas (NJ, 2), validity (NJ,) or None (all 1).  With G = render_gaussians_2d(points, sigmas, (h, w), normalize):
      terms[i] = validity[i] * sum_xy (pred[i] - G[i])^2,   loss = sum(terms) / (h w max(1, sum validity)),
      grad[i]  = 2 validity[i] (pred[i] - G[i]) / (h w max(1, sum validity))          (d loss / d pred)
    A heatmap with validity == 0 contributes exactly 0 to both and its points / sigmas are not looked at (they may be NaN) -- unlike the tensor
    expression validity * (pred - G)^2, where 0 * NaN poisons the sum.  Returns (loss, terms (NJ,), grad (NJ, h, w)) in fp64."""
    p = np.asarray(pred, dtype=np.float64)
    NJ, h, w = p.shape
    v = np.ones(NJ) if validity is None else np.asarray(validity, dtype=np.float64).reshape(NJ)
    on = v != 0
    diff = np.zeros_like(p)
    if on.any():
        diff[on] = p[on] - render_gaussians_2d(np.asarray(points).reshape(NJ, 2)[on], np.asarray(sigmas).reshape(NJ, 2)[on], (h, w), normalize)
    den = h * w * max(1.0, float(v.sum()))
    terms = v * (diff ** 2).sum(axis=(1, 2))
    return float(terms.sum() / den), terms, 2.0 * v[:, None, None] * diff / den


def softargmax2d_backward(probs, coords, grad_coords=None, grad_probs=None, mult=1.0, softmax=True):
    """The numpy fp64 statement of liblt_hip's ``lt_softargmax2d_bwd_full``: d L / d heatmaps of op.integrate_tensor_2d given the gradients on its two
    outputs.  probs (NJ, h, w) and coords (NJ, 2) are the forward's outputs; grad_coords (NJ, 2) or None (zero), grad_probs (NJ, h, w) or None (zero).
      softmax:  dh_i = mult p_i ((c_i - coords) . g) + mult p_i (gp_i - sum_k p_k gp_k)
      ReLU:     dh_i = mult [e_i > 0] ((c_i - coords) . g) / sum_k e_k + mult [e_i > 0] gp_i        (the returned heatmaps are e = relu(mult h), op.py:27)"""
    p = np.asarray(probs, dtype=np.float64)
    NJ, h, w = p.shape
    c = np.asarray(coords, dtype=np.float64).reshape(NJ, 2)
    g = np.zeros((NJ, 2)) if grad_coords is None else np.asarray(grad_coords, dtype=np.float64).reshape(NJ, 2)
    x, y = np.arange(w, dtype=np.float64)[None, None, :], np.arange(h, dtype=np.float64)[None, :, None]
    a = (x - c[:, 0, None, None]) * g[:, 0, None, None] + (y - c[:, 1, None, None]) * g[:, 1, None, None]
    if softmax:
        out = mult * p * a
        if grad_probs is not None:
            gp = np.asarray(grad_probs, dtype=np.float64)
            out = out + mult * p * (gp - (p * gp).sum(axis=(1, 2), keepdims=True))
        return out
    on = p > 0
    out = mult * np.where(on, a / p.sum(axis=(1, 2), keepdims=True), 0.0)
    if grad_probs is not None:
        out = out + mult * np.where(on, np.asarray(grad_probs, dtype=np.float64), 0.0)
    return out


def _dlt_rows(P, pts, conf):
    """A (2 n, 4) of one joint: rows c_v (x_{v,r} P_v[2, :] - P_v[r, :])."""
    A = np.empty((2 * len(P), 4))
    for v in range(len(P)):
        for r in range(2):
            A[2 * v + r] = conf[v] * (pts[v, r] * P[v, 2] - P[v, r])
    return A


def triangulation_jacobian(proj, keypoints_2d, confidences=None, view_mask=None):
    """The DLT joint and its Jacobian with respect to the 2D points, confidences held fixed, in numpy fp64: proj (B,NV,3,4), keypoints_2d (B,NV,J,2),
    confidences (B,NV,J) as they enter the system (None = 1), view_mask (B,NV) (None = all valid; masked views are never read) ->
    (X (B,J,3), jac (B,NV,J,3,2) with jac[b, v, j] = dX[b, j] / d keypoints_2d[b, v, j], zero for masked views).

    X = v[:3] / v[3], v the right singular vector of A for its smallest singular value, i.e. the eigenvector of M = A^T A for its smallest eigenvalue
    lambda.  The perturbation formula of a simple eigenvector, d v = (lambda I - M)^+ dM v, gives for a direction g_X in joint space
      g_v = (g_X / v3, -(g_X . v[:3]) / v3^2),   w = (lambda I - M)^+ g_v,   dL/dA = A (w v^T + v w^T),   dL/dx_{v,r} = c_v dL/dA[v,r,:] . P_v[2,:]
    (the formulas of lt_triangulate_dlt_bwd), evaluated for g_X = e_0, e_1, e_2.  Fewer than two valid views: NaN."""
    P = np.asarray(proj, dtype=np.float64)
    pts = np.asarray(keypoints_2d, dtype=np.float64)
    B, NV, J = pts.shape[:3]
    conf = np.ones((B, NV, J)) if confidences is None else np.asarray(confidences, dtype=np.float64)
    mask = np.ones((B, NV), dtype=bool) if view_mask is None else np.asarray(view_mask) != 0
    X = np.full((B, J, 3), np.nan)
    jac = np.zeros((B, NV, J, 3, 2))
    for b in range(B):
        views = np.flatnonzero(mask[b])
        if len(views) < 2:
            jac[b] = np.nan
            continue
        for j in range(J):
            A = _dlt_rows(P[b, views], pts[b, views, j], conf[b, views, j])
            _, sv, vh = np.linalg.svd(A, full_matrices=False)          # at least four rows: four singular values, descending
            lam = sv ** 2
            v = vh[3]
            X[b, j] = v[:3] / v[3]
            for e in range(3):
                gX = np.eye(3)[e]
                gv = np.concatenate([gX / v[3], [-(gX @ v[:3]) / v[3] ** 2]])
                wv = sum(vh[i] * (vh[i] @ gv) / (lam[3] - lam[i]) for i in range(3))
                gA = A @ (np.outer(wv, v) + np.outer(v, wv))
                for k, vw in enumerate(views):
                    for r in range(2):
                        jac[b, vw, j, e, r] = conf[b, vw, j] * (gA[2 * k + r] @ P[b, vw, 2])
    return X, jac


def triangulation_stats(proj, keypoints_2d, confidences, cov2d_img, keypoints_3d, view_mask=None):
    """The numpy fp64 statement of the two statistics of liblt_hip's ``lt_alg_tail_stats_fwd`` / ``lt_triangulate_dlt_stats``.

    proj (B,NV,3,4); keypoints_2d (B,NV,J,2) image px; confidences (B,NV,J) as they enter the system (None = 1); cov2d_img (B,NV,J,2,2) or (B,NV,J,3)
    as {xx, xy, yy}, image px^2; keypoints_3d (B,J,3): the joints the triangulation RETURNED (fp32); view_mask (B,NV), None = all valid.  Returns
      reprojection_error (B,NV,J): || pi(P_v, X) - keypoints_2d[b, v, j] ||_2 with X = keypoints_3d[b, j] and pi the perspective division of P_v [X; 1];
                                   NaN for a masked view;
      covariance (B,J,3,3): sum over the valid views of J_v Sigma_v J_v^T, J_v of ``triangulation_jacobian`` (first order, confidences fixed), in the
                            squared world units of proj; NaN with fewer than two valid views.
    Masked views' keypoints, matrices and covariances are never read."""
    P = np.asarray(proj, dtype=np.float64)
    pts = np.asarray(keypoints_2d, dtype=np.float64)
    B, NV, J = pts.shape[:3]
    S = np.asarray(cov2d_img, dtype=np.float64)
    if S.shape == (B, NV, J, 3):
        S = S[..., [0, 1, 1, 2]].reshape(B, NV, J, 2, 2)
    X = np.asarray(keypoints_3d, dtype=np.float32).astype(np.float64)
    mask = np.ones((B, NV), dtype=bool) if view_mask is None else np.asarray(view_mask) != 0
    _, jac = triangulation_jacobian(P, pts, confidences, mask)
    err = np.full((B, NV, J), np.nan)
    cov = np.zeros((B, J, 3, 3))
    for b in range(B):
        if mask[b].sum() < 2:
            cov[b] = np.nan
            continue
        for v in np.flatnonzero(mask[b]):
            hh = X[b] @ P[b, v, :, :3].T + P[b, v, :, 3]          # (J, 3)
            err[b, v] = np.sqrt(((hh[:, :2] / hh[:, 2:] - pts[b, v]) ** 2).sum(axis=1))
            cov[b] += np.einsum("jer,jrs,jfs->jef", jac[b, v], S[b, v], jac[b, v])
    return err, cov


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
