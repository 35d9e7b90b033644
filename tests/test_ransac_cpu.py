"""RANSACTriangulationNet without a GPU: the config surface (reference triangulation.py:17-25), the numpy helpers of
mvn/utils/multiview.py (reference :113-138, :186-193) against the reference's values, and the argument checks of the two C entry points
(they run before any device work)."""
import ctypes
import json
import os

import numpy as np
import pytest
import yaml

import lt_hip as H


def _ransac_cfg(golden_dir, tmp_path):
    from mvn.utils import cfg
    with open(os.path.join(golden_dir, "experiments_human36m.json")) as f:
        content = json.load(f)["eval/human36m_ransac.yaml"]
    p = tmp_path / "human36m_ransac.yaml"
    p.write_text(yaml.safe_dump(content))
    return cfg.load_config(str(p))


def test_ransac_yaml_builds_the_model(golden_dir, tmp_path):
    from mvn.models.triangulation import RANSACTriangulationNet
    c = _ransac_cfg(golden_dir, tmp_path)
    assert c.model.name == "ransac" and c.model.direct_optimization is True
    c.model.init_weights = False
    c.model.backbone.init_weights = False
    c.model.backbone.alg_confidences = True          # forced off by the constructor (reference :21-22)
    c.model.backbone.vol_confidences = True
    m = RANSACTriangulationNet(c, device="cpu")
    assert m.direct_optimization is True
    assert c.model.backbone.alg_confidences is False and c.model.backbone.vol_confidences is False
    c.model.direct_optimization = False
    assert RANSACTriangulationNet(c, device="cpu").direct_optimization is False
    # the reference's state_dict at the fixture's ResNet-18 shape: backbone only, same keys and shapes
    g = np.load(os.path.join(golden_dir, "ransac_net.npz"))
    c.model.backbone.num_layers = 18
    c.model.backbone.name = "resnet18"
    sd = RANSACTriangulationNet(c, device="cpu").state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["sd_shapes"]))


def test_numpy_dlt_and_reprojection_error_match_the_reference(golden_dir):
    from mvn.utils import multiview
    g = np.load(os.path.join(golden_dir, "ransac_ops.npz"))
    P, pts = g["nv4_d1_P"], g["nv4_d1_pts"]
    B, NV, J = pts.shape[:3]
    X = np.stack([[multiview.triangulate_point_from_multiple_views_linear(P[b], pts[b, :, j]) for j in range(J)] for b in range(B)])
    assert X.shape == g["lin_X"].shape and X.dtype == np.float64
    assert np.abs(X - g["lin_X"]).max() <= 1e-9 * np.abs(g["lin_X"]).max()
    E = np.stack([multiview.calc_reprojection_error_matrix(g["rep_X"], pts[0, :, j], P[0]) for j in range(J)])
    assert E.shape == g["rep_err"].shape == (J, J, NV)
    assert np.abs(E - g["rep_err"]).max() <= 1e-9 * np.abs(g["rep_err"]).max()


def test_ransac_entry_points_reject_bad_arguments():
    l = H.lib()
    one = ctypes.c_void_p(1)
    # NV outside 2..32: unsupported; NULL pointers: invalid -- before any launch, so no GPU is needed
    assert l.lt_triangulate_ransac(one, one, None, 0, 15.0, 1, one, None, 2, 1, 17, None) == -2 and b"NV=1" in l.lt_last_error()
    assert l.lt_triangulate_ransac(one, one, None, 0, 15.0, 1, one, None, 2, 33, 17, None) == -2 and b"NV=33" in l.lt_last_error()
    assert l.lt_triangulate_ransac(None, one, None, 0, 15.0, 1, one, None, 2, 4, 17, None) == -1 and b"null" in l.lt_last_error()
    assert l.lt_triangulate_ransac(one, None, None, 0, 15.0, 1, one, None, 2, 4, 17, None) == -1 and b"null" in l.lt_last_error()
    assert l.lt_triangulate_ransac(one, one, None, 0, 15.0, 1, None, None, 2, 4, 17, None) == -1 and b"null" in l.lt_last_error()
    assert l.lt_triangulate_ransac(one, one, one, 0, 15.0, 1, one, None, 2, 4, 17, None) == -1 and b"n_iters" in l.lt_last_error()
    assert l.lt_heatmap_argmax_nchw_f32(None, 17, one, None, one, 8, 17, 32, 32, 128, 128, None) == -1 and b"null" in l.lt_last_error()
    assert l.lt_heatmap_argmax_nchw_f32(one, 17, None, None, one, 8, 17, 32, 32, 128, 128, None) == -1 and b"null" in l.lt_last_error()
    assert l.lt_heatmap_argmax_nchw_f32(one, 16, one, None, one, 8, 17, 32, 32, 128, 128, None) == -1 and b"shape" in l.lt_last_error()
    assert l.lt_heatmap_argmax_nchw_f32(one, 40, one, None, one, 8, 40, 32, 32, 128, 128, None) == -2 and b"J=40" in l.lt_last_error()
    assert l.lt_heatmap_argmax_nchw_f32(one, 17, one, None, one, 8, 17, 32, 32, 0, 128, None) == -1 and b"image size" in l.lt_last_error()


def test_triangulate_ransac_batch_checks_shapes_before_the_library():
    import torch
    from mvn.utils import multiview
    with pytest.raises(RuntimeError, match="GPU"):
        multiview.triangulate_ransac_batch(torch.zeros(1, 4, 3, 4), torch.zeros(1, 4, 17, 2, dtype=torch.int64))
