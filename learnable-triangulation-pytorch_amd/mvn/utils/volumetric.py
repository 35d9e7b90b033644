"""Volume geometry helpers with the reference's names (mvn/utils/volumetric.py of the reference).

``Cuboid3D`` is only the (position, sides) record that ``VolumetricTriangulationNet.forward`` returns
(reference :44-47); the cv2 drawing code is visualisation and out of scope."""
import collections
import math

import numpy as np
import torch


class Cuboid3D:
    def __init__(self, position, sides):
        self.position = position
        self.sides = sides


def cuboid_from_keypoints(kp, kind, cuboid_side):
    """The pelvis and cuboid algebra of ``VolumetricTriangulationNet.forward`` (reference :284-296) on fp32 joints ``kp`` (B, J, 3): the CPU statement
    of liblt_hip's ``lt_cuboid_from_keypoints``, bit for bit.  base = joint 6 ('mpii') or (joint 11 + joint 12) / 2 ('coco', added and halved in
    fp32), promoted to fp64; position = base - cuboid_side / 2 in fp64.  Returns (pos, center): fp32(position), fp32(base), (B, 3) each."""
    kp = np.asarray(kp, dtype=np.float32)
    need = 13 if kind == "coco" else 7
    if kp.ndim != 3 or kp.shape[0] < 1 or kp.shape[1] < need or kp.shape[2] < 3:
        raise ValueError("cuboid_from_keypoints: keypoints of shape %s, kind '%s' reads joint %d of (B, J, 3)" % (kp.shape, kind, need - 1))
    base = np.empty((kp.shape[0], 3), dtype=np.float64)
    for i in range(kp.shape[0]):
        base[i] = (kp[i, 11, :3] + kp[i, 12, :3]) / 2 if kind == "coco" else kp[i, 6, :3]
    sides = np.array([cuboid_side] * 3)
    position = base - sides / 2
    return position.astype(np.float32), base.astype(np.float32)


KeypointStats = collections.namedtuple("KeypointStats", ["peak", "peak_index", "mass", "covariance"])
KeypointStats.__doc__ = """Per-joint statistics of the 3D heatmaps behind volumetric joints (``keypoint_stats`` below states them in numpy fp64): peak (B,J)
fp32, the heatmap's largest normalised value; peak_index (B,J) int32, the smallest flat voxel index of the largest logit, in the index order of
volumes[b, j]; mass (B,J) fp32, 1 in softmax mode and sum relu(logits) in ReLU mode; covariance (B,J,3,3) fp32, symmetric, mm^2: the heatmap's second
moments about the returned joint, in the frame of coord_volumes.  No gradient."""


AlgKeypointStats = collections.namedtuple("AlgKeypointStats", ["peak", "peak_index", "mass", "covariance_2d", "reprojection_error", "covariance"])
AlgKeypointStats.__doc__ = """Per-joint statistics of algebraic (triangulated) joints (``multiview.heatmap_stats_2d`` and ``multiview.triangulation_stats``
state them in numpy fp64).  Per view: peak (B,NV,J) fp32, the 2D heatmap's largest normalised value; peak_index (B,NV,J) int32, the smallest flat index
y * w + x of the largest value; mass (B,NV,J) fp32, 1 in softmax mode and sum relu(heatmap) in ReLU mode; covariance_2d (B,NV,J,2,2) fp32, image px^2:
the heatmap's second moments about the returned 2D keypoint, scaled to image pixels -- the spread of the network's heatmap, not a calibrated error bar;
reprojection_error (B,NV,J) fp32, px: distance between the view's 2D keypoint and the projection of the returned joint (NaN for a masked view).  Per
joint: covariance (B,J,3,3) fp32, squared world units (mm^2 for Human3.6M): covariance_2d pushed through the triangulation to first order, confidences
held fixed.  Values of masked views other than reprojection_error are unspecified.  No gradient."""


def keypoint_stats(values, coords, keypoints, softmax=True, from_probs=False, mass=None):
    """The numpy fp64 statement of liblt_hip's ``lt_softargmax3d_stats_fwd`` (op.integrate_tensor_3d_with_stats, ``keypoint_stats`` of the models).

    values (B, J, *vol): ``x = fp32(mult * logits)`` -- or, with ``from_probs``, the volumes the soft-argmax returned (softmax mode: the probabilities;
    ReLU mode: relu(x), not normalised).  coords (B, *vol, 3): the voxel centres, mm.  keypoints (B, J, 3): the joints the soft-argmax RETURNED (fp32):
    the moments are taken about them, never as E[c c^T] - mu mu^T.  Per (b, j), over the flattened voxels i:
      softmax:  p = softmax(x);  peak_index = the smallest i with x_i maximal;  peak = p[peak_index];  mass = 1;  centre = keypoints[b, j]
      ReLU:     w = relu(x);  mass = sum w;  peak_index as above, on x;  peak = w[peak_index] / mass;  centre = keypoints[b, j] / fp32(mass), one fp32
                division per coordinate (the joints of this mode are not normalised);  p = w / mass;  mass == 0: peak = 0, covariance = 0
      covariance = sum_i p_i (c_i - centre)(c_i - centre)^T
    ``mass``: the fp32 mass that was returned next to ``keypoints`` (ReLU mode), for the centre's division; None: fp32(sum w).  With ``from_probs`` the
    peak voxel is the first maximum of the volumes themselves.  Returns a KeypointStats of fp64 arrays (peak_index: int64)."""
    v = np.asarray(values)
    B, J = v.shape[:2]
    v = v.reshape(B, J, -1).astype(np.float64)
    c = np.asarray(coords, dtype=np.float64).reshape(B, -1, 3)
    kp = np.asarray(keypoints, dtype=np.float32).reshape(B, J, 3)
    if v.shape[2] != c.shape[1]:
        raise ValueError("keypoint_stats: %d voxels in values, %d in coords" % (v.shape[2], c.shape[1]))
    idx = v.argmax(axis=2)                                  # numpy: the first of equal maxima
    if softmax:
        p = v if from_probs else np.exp(v - v.max(axis=2, keepdims=True))
        if not from_probs:
            p = p / p.sum(axis=2, keepdims=True)
        m = np.ones((B, J))
        centre = kp.astype(np.float64)
    else:
        w = np.maximum(v, 0.0)
        m = w.sum(axis=2)
        m32 = m.astype(np.float32) if mass is None else np.asarray(mass, dtype=np.float32).reshape(B, J)
        some = m > 0
        p = np.where(some[..., None], w / np.where(some, m, 1.0)[..., None], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            centre = np.where(some[..., None], (kp / m32[..., None]).astype(np.float64), 0.0)
    peak = np.take_along_axis(p, idx[..., None], axis=2)[..., 0]
    d = c[:, None, :, :] - centre[:, :, None, :]            # (B, J, nvox, 3)
    cov = np.einsum("bjn,bjnr,bjns->bjrs", p, d, d)
    cov = np.triu(cov) + np.swapaxes(np.triu(cov, 1), -1, -2)          # six moments, mirrored: symmetric exactly, as the kernel's records are
    return KeypointStats(peak, idx, m, cov)


def get_rotation_matrix(axis, theta):
    """Counter-clockwise rotation by theta about axis, Euler-Rodrigues form (reference :87-99), fp64."""
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / math.sqrt(float(ax @ ax))
    a = math.cos(theta / 2.0)
    b, c, d = (-ax * math.sin(theta / 2.0)).tolist()
    return np.array([
        [a * a + b * b - c * c - d * d, 2.0 * (b * c + a * d), 2.0 * (b * d - a * c)],
        [2.0 * (b * c - a * d), a * a + c * c - b * b - d * d, 2.0 * (c * d + a * b)],
        [2.0 * (b * d + a * c), 2.0 * (c * d - a * b), a * a + d * d - b * b - c * c]], dtype=np.float64)


def rotate_coord_volume(coord_volume, theta, axis):
    """Rotate a (..., 3) fp32 coordinate grid about the origin (reference :102-114) with lt_rotate_points.
    Inside VolumetricTriangulationNet the rotation is fused into the grid construction (lt_coord_volumes)."""
    import lt_hip as H
    H.require_gpu(coord_volume, "coord_volume")
    x = coord_volume.float().contiguous()
    rot = torch.from_numpy(get_rotation_matrix(axis, theta)).float().to(x.device).contiguous()
    y = torch.empty_like(x)
    H.check(H.lib().lt_rotate_points(x.data_ptr(), rot.data_ptr(), y.data_ptr(), x.numel() // 3, H.cur_stream()), "lt_rotate_points")
    return y
