"""Volume geometry helpers with the reference's names (mvn/utils/volumetric.py of the reference).

``Cuboid3D`` is only the (position, sides) record that ``VolumetricTriangulationNet.forward`` returns
(reference :44-47); the cv2 drawing code is visualisation and out of scope."""
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
