"""CPU: mvn.datasets.human36m.Human36MMultiViewDataset against the reference dataset's items on a synthetic label table with
PNG frames (tests/golden/h36m_dataset.npz, tools/make_golden_img.py), the deferred-pixel items (defer_image_ops=True), and
make_collate_fn on deferred items."""
import os
import pickle

import numpy as np
import pytest

from mvn.datasets import utils as du
from mvn.datasets.human36m import Human36MMultiViewDataset

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "h36m_dataset.npz"))


@pytest.fixture()
def tree(g, tmp_path):
    labels = pickle.loads(g["labels"].tobytes())
    lp = str(tmp_path / "labels.npy")
    np.save(lp, labels, allow_pickle=True)
    off = g["png_offsets"]
    for i, name in enumerate(g["png_names"]):
        p = tmp_path / str(name)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(g["png_bytes"][off[i]:off[i + 1]].tobytes())
    return str(tmp_path), lp


def _key(ds):
    t = ds.labels["table"]
    return np.asarray(t["frame_idx"]) * 1000 + t["subject_idx"] * 10 + t["action_idx"]


def test_selection_matches_reference(g, tree):
    root, lp = tree
    for split, kw in (("train", dict(train=True)), ("test", dict(test=True)), ("test_damaged", dict(test=True, with_damaged_actions=True)),
                      ("test_n2", dict(test=True, retain_every_n_frames_in_test=2)), ("both", dict(train=True, test=True))):
        ds = Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, **kw)
        assert np.array_equal(_key(ds), g["sel_%s" % split]), split
    with pytest.raises(AssertionError):
        Human36MMultiViewDataset(h36m_root=root, labels_path=lp)


def test_items_match_reference(g, tree):
    root, lp = tree
    for crop in (True, False):
        ds = Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, test=True, crop=crop, scale_bbox=1.5,
                                      ignore_cameras=[1] if crop else [])
        for idx in (0, 1, 3):
            k = "c%d_i%d_" % (int(crop), idx)
            it = ds[idx]
            assert len(it["images"]) == int(g[k + "nviews"])
            for v, im in enumerate(it["images"]):
                ref = g[k + "image%d" % v]
                assert im.dtype == ref.dtype and np.array_equal(im, ref), (k, v)
            assert np.array_equal(np.array(it["detections"], np.float64), g[k + "detections"])
            assert np.array_equal(np.stack([c.K for c in it["cameras"]]).astype(np.float32), g[k + "K"])
            assert np.array_equal(np.stack([c.R for c in it["cameras"]]).astype(np.float32), g[k + "R"])
            assert np.array_equal(np.stack([c.t for c in it["cameras"]]).astype(np.float32), g[k + "t"])
            # the reference's Camera keeps the label file's fp32 arrays (crop shift rounded to fp32, projection in fp32);
            # mvn.utils.multiview.Camera holds fp64, whose exact crop shift rounds to the same fp32
            pr, pg = np.stack(it["proj_matrices"]), g[k + "proj"]
            assert np.abs(pr - pg).max() <= 2e-7 * np.abs(pg).max()
            assert np.array_equal(it["keypoints_3d"], g[k + "keypoints_3d"])
            assert it["indexes"] == int(g[k + "indexes"])


def test_pred_results_and_evaluate(g, tree, tmp_path):
    root, lp = tree
    pp = str(tmp_path / "pred.pkl")
    pickle.dump({"keypoints_3d": g["pred_keypoints_3d"], "indexes": g["pred_indexes"]}, open(pp, "wb"))
    ds = Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, test=True, pred_results_path=pp)
    assert np.array_equal(ds[0]["pred_keypoints_3d"], g["pred_item0"])
    score, full = ds.evaluate(g["eval_pred"])
    assert score == float(g["eval_score"]) and "per_pose_error" in full


@pytest.mark.parametrize("shape", [(384, 384), (24, 20)])
def test_deferred_items_carry_the_cpu_path_cameras(tree, shape):
    root, lp = tree
    for crop in (True, False):
        kw = dict(h36m_root=root, labels_path=lp, image_shape=shape, test=True, crop=crop, scale_bbox=1.5)
        cpu, dfr = Human36MMultiViewDataset(**kw), Human36MMultiViewDataset(defer_image_ops=True, **kw)
        for idx in range(3):
            a, b = cpu[idx], dfr[idx]
            assert "images" not in b and "frames" in b and "bboxes" in b
            assert len(b["frames"]) == len(a["images"]) == len(b["bboxes"])
            for f, bb, im in zip(b["frames"], b["bboxes"], a["images"]):
                assert f.dtype == np.uint8 and f.ndim == 3 and im.shape == shape + (3,)
                assert all(isinstance(x, int) for x in bb)
            assert [tuple(s) for s in a["image_shapes_before_resize"]] == [tuple(s) for s in b["image_shapes_before_resize"]]
            for ca, cb in zip(a["cameras"], b["cameras"]):
                for attr in ("K", "R", "t"):
                    assert np.array_equal(getattr(ca, attr), getattr(cb, attr)) and getattr(ca, attr).dtype == getattr(cb, attr).dtype
            for pa, pb in zip(a["proj_matrices"], b["proj_matrices"]):
                assert np.array_equal(pa, pb)
            assert a["detections"] == b["detections"]
            assert np.array_equal(a["keypoints_3d"], b["keypoints_3d"]) and a["indexes"] == b["indexes"]


def test_collate_of_deferred_items(tree):
    root, lp = tree
    kw = dict(h36m_root=root, labels_path=lp, image_shape=(32, 32), test=True, scale_bbox=1.5)
    cpu, dfr = Human36MMultiViewDataset(**kw), Human36MMultiViewDataset(defer_image_ops=True, **kw)
    collate = du.make_collate_fn(randomize_n_views=False)
    bc, bd = collate([cpu[i] for i in range(3)]), collate([dfr[i] for i in range(3)])
    assert "images" not in bd and bc["images"].shape == (3, 3, 32, 32, 3)
    nv = bc["images"].shape[1]
    assert len(bd["frames"]) == nv and all(len(f) == 3 for f in bd["frames"])
    assert bd["bboxes"].shape == (3, nv, 4)
    assert np.array_equal(bc["detections"], bd["detections"])
    assert bd["indexes"] == bc["indexes"]
    for v in range(nv):
        for b in range(3):
            assert bd["frames"][v][b] is dfr[b]["frames"][v] or np.array_equal(bd["frames"][v][b], dfr[b]["frames"][v])
            assert np.array_equal(bd["bboxes"][b, v], dfr[b]["bboxes"][v])
    # the collate of "images" items is the one it always was (tests/test_data_eval.py pins it against the reference)
    np.random.seed(3)
    r1 = collate([cpu[i] for i in range(3)])
    assert np.array_equal(r1["images"], bc["images"]) and r1.keys() == bc.keys()
