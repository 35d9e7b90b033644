"""Human3.6M multi-view dataset with the reference's name and constructor (mvn/datasets/human36m.py of the reference).

Selection of the label table (train / test subjects, the three damaged S9 actions, ``retain_every_n_frames_in_test``,
``ignore_cameras``, ``pred_results_path``), the per-camera items and ``evaluate()`` follow the reference.  Frames are decoded with
``cv2.imread`` when OpenCV is importable, otherwise with PIL converted to BGR; two JPEG decoders may round differently, so pixel
parity with a cv2 run holds only for losslessly stored frames.

``defer_image_ops=True`` leaves the pixel work to the GPU: an item then carries ``frames`` (the decoded uint8 BGR frame of every
view) and ``bboxes`` (the crop box the CPU path would use, frame coordinates) instead of ``images``; cameras,
``image_shapes_before_resize``, ``detections`` and ``keypoints_3d`` are exactly those of the CPU path.  Collate such items with
``make_collate_fn`` and upload them with ``prepare_batch_frames`` (one kernel launch crops, resizes and normalises every view).

``undistort_on_the_fly=True`` (with ``undistort_images=True``) reads the raw ``imageSequence/`` frames and undistorts each view's
crop as it is prepared, instead of reading the ``imageSequence-undistorted/`` copies the reference's offline pass
(human36m_preprocessing/undistort-h36m.py) writes: the view is the bbox crop of cv2.remap(raw frame, maps, INTER_CUBIC) with that
pass's maps (mvn/utils/img.py:undistort_maps, built once per camera and frame size).  Cameras, shapes, detections and targets are
those of the ``undistort_images=True`` file path.  The pixels are the remap of the decoded raw frame, so they differ from the
offline pass's output by the JPEG generation that pass adds when it writes its copy.  With ``defer_image_ops`` the item also carries
``undistort``: per view (K (3, 3) float32 and dist (5,) float32 of the labels file, (frame height, frame width)), the key of the
camera's maps, and ``prepare_batch_frames`` runs the undistortion in its one launch.
"""
import os
from collections import defaultdict

import numpy as np
from PIL import Image
from torch.utils.data import Dataset

from mvn.datasets import evaluation
from mvn.utils.img import crop_image, normalize_image, resize_image, scale_bbox, undistort_crop_u8, undistort_maps
from mvn.utils.multiview import Camera

try:
    import cv2
except ImportError:
    cv2 = None

TRAIN_SUBJECTS = ("S1", "S5", "S6", "S7", "S8")
TEST_SUBJECTS = ("S9", "S11")
DAMAGED_S9_ACTIONS = ("Greeting-2", "SittingDown-2", "Waiting-1")


def imread_bgr(path):
    """uint8 (h, w, 3) BGR frame: cv2.imread, or PIL's RGB decode reversed to BGR without OpenCV."""
    if cv2 is not None:
        return cv2.imread(path)
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


class Human36MMultiViewDataset(Dataset):
    """Human3.6M for multi-view tasks.  ``labels_path``: the 'human36m-multiview-labels-*.npy' dict; ``h36m_root``: its 'processed/'
    image tree.  ``kind`` 'mpii' (16 joints) or 'human36m' (17); ``ignore_cameras``: camera indices to drop;
    ``retain_every_n_frames_in_test``: keep every n-th test frame; ``defer_image_ops``, ``undistort_on_the_fly``: see the module
    docstring."""

    def __init__(self, h36m_root='/Vol1/dbstore/datasets/Human3.6M/processed/',
                 labels_path='/Vol1/dbstore/datasets/Human3.6M/extra/human36m-multiview-labels-SSDbboxes.npy',
                 pred_results_path=None, image_shape=(256, 256), train=False, test=False, retain_every_n_frames_in_test=1,
                 with_damaged_actions=False, cuboid_side=2000.0, scale_bbox=1.5, norm_image=True, kind="mpii", undistort_images=False,
                 ignore_cameras=[], crop=True, defer_image_ops=False, undistort_on_the_fly=False):
        assert train or test, "`Human36MMultiViewDataset` must be constructed with at least one of `test=True` / `train=True`"
        assert kind in ("mpii", "human36m")
        self.h36m_root = h36m_root
        self.labels_path = labels_path
        self.image_shape = None if image_shape is None else tuple(image_shape)
        self.scale_bbox = scale_bbox
        self.norm_image = norm_image
        self.cuboid_side = cuboid_side
        self.kind = kind
        self.undistort_images = undistort_images
        self.ignore_cameras = ignore_cameras
        self.crop = crop
        self.defer_image_ops = defer_image_ops
        if defer_image_ops:
            assert self.image_shape is not None, "defer_image_ops needs an image_shape (the kernel's output size)"
        if undistort_on_the_fly and not undistort_images:
            raise ValueError("undistort_on_the_fly=True undistorts raw frames in place of the undistort_images=True files: "
                             "it needs undistort_images=True")
        self.undistort_on_the_fly = undistort_on_the_fly
        self._maps = {}

        self.labels = np.load(labels_path, allow_pickle=True).item()
        n_cameras = len(self.labels['camera_names'])
        assert all(c in range(n_cameras) for c in self.ignore_cameras)

        table = self.labels['table']
        subject_names = self.labels['subject_names']
        keep = []
        if train:
            mask = np.isin(table['subject_idx'], [subject_names.index(s) for s in TRAIN_SUBJECTS], assume_unique=True)
            keep.append(np.nonzero(mask)[0])
        if test:
            mask = np.isin(table['subject_idx'], [subject_names.index(s) for s in TEST_SUBJECTS], assume_unique=True)
            if not with_damaged_actions:
                damaged = [self.labels['action_names'].index(a) for a in DAMAGED_S9_ACTIONS]
                mask &= ~((table['subject_idx'] == subject_names.index('S9')) & np.isin(table['action_idx'], damaged))
            keep.append(np.nonzero(mask)[0][::retain_every_n_frames_in_test])
        self.labels['table'] = table[np.concatenate(keep)]

        self.num_keypoints = 16 if kind == "mpii" else 17
        assert self.labels['table']['keypoints'].shape[1] == 17, "Use a newer 'labels' file"

        self.keypoints_3d_pred = None
        if pred_results_path is not None:
            pred = np.load(pred_results_path, allow_pickle=True)
            kp = pred['keypoints_3d'][np.argsort(pred['indexes'])]
            self.keypoints_3d_pred = kp[::retain_every_n_frames_in_test]
            assert len(self.keypoints_3d_pred) == len(self), \
                "[train=%s, test=%s] %s has %d samples, but '%s' has %d. Did you follow all preprocessing instructions carefully?" % (
                    train, test, labels_path, len(self), pred_results_path, len(self.keypoints_3d_pred))

    def __len__(self):
        return len(self.labels['table'])

    def image_path(self, subject, action, camera_name, frame_idx):
        folder = 'imageSequence' + ('-undistorted' if self.undistort_images and not self.undistort_on_the_fly else '')
        return os.path.join(self.h36m_root, subject, action, folder, camera_name, 'img_%06d.jpg' % (frame_idx + 1))

    def undistort_key(self, cam, frame_hw):
        """(K, dist, (h, w)) of a labels-file camera: what the camera's undistortion maps depend on."""
        return (np.array(cam['K'], dtype=np.float32), np.array(cam['dist'], dtype=np.float32).reshape(-1), tuple(int(x) for x in frame_hw))

    def undistortion_maps(self, key):
        """undistort_maps of a camera and frame size, built once per dataset (worker) and kept."""
        K, dist, (h, w) = key
        k = (K.tobytes(), dist.tobytes(), h, w)
        if k not in self._maps:
            self._maps[k] = undistort_maps(K, dist, h, w)
        return self._maps[k]

    def __getitem__(self, idx):
        sample = defaultdict(list)
        shot = self.labels['table'][idx]
        subject = self.labels['subject_names'][shot['subject_idx']]
        action = self.labels['action_names'][shot['action_idx']]

        for camera_idx, camera_name in enumerate(self.labels['camera_names']):
            if camera_idx in self.ignore_cameras:
                continue
            bbox = shot['bbox_by_camera_tlbr'][camera_idx][[1, 0, 3, 2]]     # TLBR -> LTRB
            if bbox[2] - bbox[0] == 0:       # an empty bbox marks a missing view (the reference tests this difference)
                continue
            bbox = scale_bbox(bbox, self.scale_bbox)

            path = self.image_path(subject, action, camera_name, shot['frame_idx'])
            assert os.path.isfile(path), "%s doesn't exist" % path
            image = imread_bgr(path)

            cam = self.labels['cameras'][shot['subject_idx'], camera_idx]
            camera = Camera(cam['R'], cam['t'], cam['K'], cam['dist'], camera_name)

            crop_box = bbox if self.crop else (0, 0, image.shape[1], image.shape[0])
            if self.crop:
                camera.update_after_crop(bbox)
            if self.defer_image_ops:
                shape_before_resize = (int(crop_box[3] - crop_box[1]), int(crop_box[2] - crop_box[0]))
                camera.update_after_resize(shape_before_resize, self.image_shape)
                sample['image_shapes_before_resize'].append(shape_before_resize)
                sample['frames'].append(image)
                sample['bboxes'].append(tuple(int(x) for x in crop_box))
                if self.undistort_on_the_fly:
                    sample['undistort'].append(self.undistort_key(cam, image.shape[:2]))
            else:
                if self.undistort_on_the_fly:
                    maps = self.undistortion_maps(self.undistort_key(cam, image.shape[:2]))
                    image = undistort_crop_u8(image, maps, tuple(int(x) for x in crop_box))
                elif self.crop:
                    image = crop_image(image, bbox)
                if self.image_shape is not None:
                    shape_before_resize = image.shape[:2]
                    image = resize_image(image, self.image_shape)
                    camera.update_after_resize(shape_before_resize, self.image_shape)
                    sample['image_shapes_before_resize'].append(shape_before_resize)
                if self.norm_image:
                    image = normalize_image(image)
                sample['images'].append(image)
            sample['detections'].append(bbox + (1.0,))      # the reference's placeholder confidence
            sample['cameras'].append(camera)
            sample['proj_matrices'].append(camera.projection)

        # 3D keypoints with a dummy validity column
        sample['keypoints_3d'] = np.pad(shot['keypoints'][:self.num_keypoints], ((0, 0), (0, 1)), 'constant', constant_values=1.0)
        sample['indexes'] = idx
        if self.keypoints_3d_pred is not None:
            sample['pred_keypoints_3d'] = self.keypoints_3d_pred[idx]
        sample.default_factory = None
        return sample

    def evaluate_using_per_pose_error(self, per_pose_error, split_by_subject):
        t = self.labels['table']
        return evaluation.evaluate_using_per_pose_error(per_pose_error, t['action_idx'], self.labels['action_names'], t['subject_idx'],
                                                        self.labels['subject_names'])

    def evaluate(self, keypoints_3d_predicted, split_by_subject=False, transfer_cmu_to_human36m=False, transfer_human36m_to_human36m=False):
        return evaluation.evaluate(self.labels, keypoints_3d_predicted, num_keypoints=self.num_keypoints, kind=self.kind,
                                   split_by_subject=split_by_subject, transfer_cmu_to_human36m=transfer_cmu_to_human36m,
                                   transfer_human36m_to_human36m=transfer_human36m_to_human36m)
