"""Generates tests/golden/img_ops.npz and tests/golden/h36m_dataset.npz by running the REFERENCE's mvn/utils/img.py and
mvn/datasets/human36m.py where the reference tree is available (oracle.ref_loader, cv2 stubbed).  Writes only these two files:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_img.py

img_ops.npz: crop_image on small random frames with bboxes inside, straddling and wholly outside the frame; scale_bbox and
get_square_bbox cases; normalize_image / denormalize_image; image_batch_to_numpy / image_batch_to_torch.

h36m_dataset.npz: a synthetic label dict (7 subjects, actions with the damaged S9 trials, 4 cameras, one empty bbox), its frames
(of the first test items) as PNG bytes to be stored under the reference's img_%06d.jpg names (PNG decodes identically everywhere), and the reference
dataset's items for image_shape=None with crop=True and crop=False -- the stubbed cv2.imread decodes with PIL and returns BGR.
"""
import io
import os
import pickle
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SUBJECTS = ["S1", "S5", "S6", "S7", "S8", "S9", "S11"]
ACTIONS = ["Directions-1", "Directions-2", "Greeting-1", "Greeting-2", "SittingDown-1", "SittingDown-2", "Waiting-1", "Waiting-2"]
CAMERAS = ["54138969", "55011271", "58860488", "60457274"]
FRAME_HW = (40, 48)


def img_ops(img, rng):
    out = {}
    frames, boxes, crops = [], [], []
    cases = [(2, 3, 30, 25), (-5, -7, 20, 18), (30, 20, 60, 50), (-20, -20, -5, -3), (50, 41, 70, 60), (0, 0, 48, 40), (-3, 5, 51, 36)]
    for i, b in enumerate(cases):
        f = rng.integers(0, 256, (FRAME_HW[0], FRAME_HW[1], 3), dtype=np.uint8)
        c = img.crop_image(f, b)
        frames.append(f); boxes.append(b)
        out["crop_%d" % i] = c
    out["crop_frames"] = np.stack(frames)
    out["crop_bboxes"] = np.array(boxes, np.int64)
    bbs = rng.integers(-100, 1000, (40, 2))
    sizes = rng.integers(1, 500, (40, 2))
    bbs = np.concatenate([bbs, bbs + sizes], 1)
    scales = np.array([1.0, 1.5, 1.2, 0.8, 2.0, 1.25, 1.1, 1.3] * 5)
    out["bbox_in"] = bbs
    out["bbox_scales"] = scales
    out["scale_bbox"] = np.array([img.scale_bbox(tuple(int(x) for x in b), s) for b, s in zip(bbs, scales)], np.int64)
    out["square_bbox"] = np.array([img.get_square_bbox(tuple(int(x) for x in b)) for b in bbs], np.int64)
    u8 = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    out["norm_in"] = u8
    out["norm_out"] = img.normalize_image(u8)
    dn = rng.normal(0, 1.5, (9, 11, 3))
    out["denorm_in"] = dn
    out["denorm_out"] = img.denormalize_image(dn)
    bt = rng.normal(size=(2, 3, 5, 7)).astype(np.float32)
    out["batch_chw"] = bt
    out["batch_to_numpy"] = img.image_batch_to_numpy(bt)
    bh = rng.normal(size=(2, 5, 7, 3))
    out["batch_hwc"] = bh
    out["batch_to_torch"] = img.image_batch_to_torch(bh).numpy()
    return out


def make_labels(rng):
    rows = []
    for si in range(len(SUBJECTS)):
        for ai in (0, 3, 5, 6, 7):
            for fi in (0, 2):
                rows.append((si, ai, fi))
    table = np.zeros(len(rows), dtype=[("subject_idx", np.int8), ("action_idx", np.int8), ("frame_idx", np.int16),
                                       ("keypoints", np.float32, (17, 3)), ("bbox_by_camera_tlbr", np.int16, (4, 4))])
    for i, (si, ai, fi) in enumerate(rows):
        table[i]["subject_idx"], table[i]["action_idx"], table[i]["frame_idx"] = si, ai, fi
        table[i]["keypoints"] = rng.normal(0, 500, (17, 3))
        for c in range(4):
            t, l = rng.integers(-6, 20), rng.integers(-6, 26)
            table[i]["bbox_by_camera_tlbr"][c] = (t, l, t + rng.integers(8, 30), l + rng.integers(8, 30))
    table[50]["bbox_by_camera_tlbr"][2] = (5, 5, 20, 5)      # S9, first test item: an empty bbox, the view is skipped
    cams = np.zeros((len(SUBJECTS), 4), dtype=[("R", np.float32, (3, 3)), ("t", np.float32, (3, 1)), ("K", np.float32, (3, 3)),
                                               ("dist", np.float32, 5)])
    for s in range(len(SUBJECTS)):
        for c in range(4):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            cams[s, c]["R"] = q
            cams[s, c]["t"] = rng.normal(0, 1000, (3, 1))
            cams[s, c]["K"] = [[rng.uniform(40, 60), 0, rng.uniform(20, 28)], [0, rng.uniform(40, 60), rng.uniform(16, 24)], [0, 0, 1]]
            cams[s, c]["dist"] = rng.normal(0, 0.01, 5)
    return {"subject_names": SUBJECTS, "action_names": ACTIONS, "camera_names": CAMERAS, "table": table, "cameras": cams}


def dataset(mvn_ref, rng):
    import cv2  # the ref_loader stub

    def imread(path):
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
    cv2.imread = imread
    from mvn.datasets import human36m as ref_h36m   # noqa: E402  (the reference's, ref_loader put it first on sys.path)
    labels = make_labels(rng)
    out = {"labels": np.frombuffer(pickle.dumps(labels), np.uint8)}
    with tempfile.TemporaryDirectory() as root:
        lp = os.path.join(root, "labels.npy")
        np.save(lp, labels, allow_pickle=True)
        names, pngs = [], []
        test_rows = ref_h36m.Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, test=True).labels["table"]
        for row in test_rows[:4]:              # the frames of the items fetched below (frames are only read in __getitem__)
            for cam in CAMERAS:
                rel = os.path.join(SUBJECTS[row["subject_idx"]], ACTIONS[row["action_idx"]], "imageSequence", cam, "img_%06d.jpg" % (row["frame_idx"] + 1))
                f = rng.integers(0, 256, (FRAME_HW[0], FRAME_HW[1], 3), dtype=np.uint8)
                b = io.BytesIO()
                Image.fromarray(f).save(b, format="PNG")
                p = os.path.join(root, rel)
                os.makedirs(os.path.dirname(p), exist_ok=True)
                open(p, "wb").write(b.getvalue())
                names.append(rel); pngs.append(b.getvalue())
        out["png_names"] = np.array(names)
        out["png_offsets"] = np.cumsum([0] + [len(p) for p in pngs])
        out["png_bytes"] = np.frombuffer(b"".join(pngs), np.uint8)
        for split, kw in (("train", dict(train=True)), ("test", dict(test=True)), ("test_damaged", dict(test=True, with_damaged_actions=True)),
                          ("test_n2", dict(test=True, retain_every_n_frames_in_test=2)), ("both", dict(train=True, test=True))):
            ds = ref_h36m.Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, **kw)
            out["sel_%s" % split] = np.asarray(ds.labels["table"]["frame_idx"]) * 1000 + ds.labels["table"]["subject_idx"] * 10 + ds.labels["table"]["action_idx"]
        for crop in (True, False):
            ds = ref_h36m.Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, test=True, crop=crop, scale_bbox=1.5,
                                                    ignore_cameras=[1] if crop else [])
            for idx in (0, 1, 3):
                if idx >= len(ds):
                    continue
                it = ds[idx]
                k = "c%d_i%d_" % (int(crop), idx)
                out[k + "nviews"] = np.array(len(it["images"]))
                for v, im in enumerate(it["images"]):
                    out[k + "image%d" % v] = im
                out[k + "detections"] = np.array(it["detections"], np.float64)
                out[k + "K"] = np.stack([c.K for c in it["cameras"]])
                out[k + "R"] = np.stack([c.R for c in it["cameras"]])
                out[k + "t"] = np.stack([c.t for c in it["cameras"]])
                out[k + "proj"] = np.stack(it["proj_matrices"])
                out[k + "keypoints_3d"] = it["keypoints_3d"]
                out[k + "indexes"] = np.array(it["indexes"])
        preds = {"keypoints_3d": rng.normal(size=(len(ds), 17, 3)), "indexes": rng.permutation(len(ds))}
        pp = os.path.join(root, "pred.pkl")
        pickle.dump(preds, open(pp, "wb"))
        ds = ref_h36m.Human36MMultiViewDataset(h36m_root=root, labels_path=lp, image_shape=None, test=True, pred_results_path=pp)
        out["pred_keypoints_3d"] = preds["keypoints_3d"]
        out["pred_indexes"] = preds["indexes"]
        out["pred_item0"] = ds[0]["pred_keypoints_3d"]
        kp = rng.normal(0, 500, (len(ds), 16, 3))
        out["eval_pred"] = kp
        score, _ = ds.evaluate(kp)
        out["eval_score"] = np.array(score)
    return out


def main():
    mvn_ref = ref_loader.load()
    import mvn.utils.img as ref_img   # the reference's (ref_loader put it first on sys.path)
    assert os.path.realpath(ref_img.__file__).startswith(ref_loader.REFERENCE_ROOT)
    rng = np.random.default_rng(20261016)
    np.savez_compressed(os.path.join(GOLD, "img_ops.npz"), **img_ops(ref_img, rng))
    np.savez_compressed(os.path.join(GOLD, "h36m_dataset.npz"), **dataset(mvn_ref, rng))
    for f in ("img_ops.npz", "h36m_dataset.npz"):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()
