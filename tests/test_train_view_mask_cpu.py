"""CPU: the opt-in switches of training with view masks.  With the flags at their defaults a mask in train() is refused as it always was (type and message,
before the GPU check); with ``masked_training`` the volumetric and the algebraic model let it through to the 'must live on the GPU' error and the cascade
stays eval-only; the functional ops' ``masked_backward`` defaults to False; the training plan key carries the masked flag and an unmasked key is the tuple
it always was; ``make_collate_fn(mask_views=True)`` keeps the view count fixed and turns the drawn count into ``batch["view_mask"]``, and
``mask_views=False`` is the function it was, np.random call for np.random call."""
import inspect

import numpy as np
import pytest
import torch

from oracle import synth
from test_view_mask_cpu import cameras


def _models():
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet, VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu")
    alg = AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu")
    return vol, alg, CascadeTriangulationNet(alg, vol)


def _batch(inp, m):
    return {"cameras": cameras(inp, 2), "pred_keypoints_3d": inp["pred_keypoints_3d"], "view_mask": m}


def test_default_flags_keep_the_refusals_and_masked_training_lifts_them():
    vol, alg, casc = _models()
    inp = synth.make_inputs(2, 4, 64, seed=1)
    images, P = inp["images"], torch.zeros(2, 4, 3, 4)
    good = np.array([[1, 0, 1, 1], [0, 1, 0, 1]], dtype=bool)
    assert vol.masked_training is False and alg.masked_training is False and not hasattr(casc, "masked_training")
    msg = r"%s: batch\['view_mask'\] is inference only \(there is no masked backward\); call eval\(\) first"
    for net, name in ((vol, "VolumetricTriangulationNet"), (alg, "AlgebraicTriangulationNet")):
        net.train()
        with pytest.raises(NotImplementedError, match=msg % name):          # CPU images: the refusal comes before require_gpu
            net(images, P, _batch(inp, good))
        net.masked_training = True
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            net(images, P, _batch(inp, good))
        with pytest.raises(ValueError, match=r"\(B, NV\) = \(2, 4\)"):          # the mask checks still come first
            net(images, P, _batch(inp, np.ones((2, 3), dtype=bool)))
        net.eval()
    # minimum valid views as in inference: one for the volumetric model, two for the algebraic one
    one_view = np.array([[1, 0, 0, 0], [0, 0, 0, 1]], dtype=bool)
    vol.train(); alg.train()
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        vol(images, P, _batch(inp, one_view))
    with pytest.raises(ValueError, match="sample 0 has 1 valid view, at least 2"):
        alg(images, P, _batch(inp, one_view))
    with pytest.raises(ValueError, match="sample 1 has 0 valid views"):
        vol(images, P, _batch(inp, np.array([[1, 1, 1, 1], [0, 0, 0, 0]])))
    # the cascade stays eval-only, whatever its stages' flags say
    casc.train()
    with pytest.raises(NotImplementedError):
        casc(images, P, _batch(inp, good))


def test_functional_ops_default_to_the_refusal():
    from mvn.utils import multiview, op
    for fn in (op.unproject_heatmaps, multiview.triangulate_batch_of_points):
        p = inspect.signature(fn).parameters
        assert p["masked_backward"].default is False and p["view_mask"].default is None, fn.__name__
    assert "masked_backward" not in inspect.signature(multiview.triangulate_batch_of_points_with_stats).parameters


def test_training_plan_key_carries_the_masked_flag():
    vol, _, _ = _models()
    params = tuple(vol.parameters())
    plain = vol._train_plan_key(2, 4, 64, 64, "cpu", params)
    assert plain == vol._train_plan_key(2, 4, 64, 64, "cpu", params, False)
    masked = vol._train_plan_key(2, 4, 64, 64, "cpu", params, True)
    assert masked != plain and masked[:len(plain)] == plain and len(masked) == len(plain) + 1
    # an unmasked key is the tuple it always was
    from torch import nn
    assert plain == (2, 4, 64, 64, "cpu", vol.volume_size, float(vol.cuboid_side), float(vol.volume_multiplier), bool(vol.volume_softmax),
                     vol.volume_aggregation_method, bool(vol.transfer_cmu_to_human36m), vol.num_joints, tuple(p.requires_grad for p in params), id(None), "fp32",
                     tuple(c.training for c in vol.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm)))
    from mvn.models.triangulation import _VolTrainPlan
    assert _VolTrainPlan(vol, 2, 4, 64, 64, "cpu").masked is False and _VolTrainPlan(vol, 2, 4, 64, 64, "cpu", masked=True).masked is True


# ---- the collate function -----------------------------------------------------------------------------------------------------------------------------------
def _items(n_items, n_views, seed=0):
    g = np.random.RandomState(seed)
    return [{"images": [g.rand(4, 4, 3).astype(np.float32) + v for v in range(n_views)], "detections": [np.full(5, v) for v in range(n_views)],
             "cameras": ["cam%d_%d" % (i, v) for v in range(n_views)], "keypoints_3d": g.rand(17, 4), "indexes": i, "pred_keypoints_3d": g.rand(17, 3)}
            for i in range(n_items)]


def test_mask_views_keeps_the_view_count_and_masks_the_drawn_count():
    from mvn.datasets.utils import make_collate_fn
    items = _items(4, 12)
    collate = make_collate_fn(randomize_n_views=True, min_n_views=3, max_n_views=8, mask_views=True)
    counts = set()
    for seed in range(12):
        np.random.seed(seed)
        batch = collate(items)
        m = batch["view_mask"]
        assert m.shape == (4, 8) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
        assert batch["images"].shape[:2] == (4, 8) and len(batch["cameras"]) == 8 and batch["detections"].shape[:2] == (4, 8)
        n = m.sum(axis=1)
        assert (n == n[0]).all() and 3 <= n[0] <= 8, "exactly n_views valid views in every row, n_views drawn once per batch"
        counts.add(int(n[0]))
        views = [int(c[0].split("_")[1]) for c in batch["cameras"]]          # the kept views: a choice of 8 of the 12, in ascending index order
        assert views == sorted(views) and len(set(views)) == 8 and [int(d[0, 0]) for d in batch["detections"].swapaxes(0, 1)] == views
    assert len(counts) >= 3, "the view count varies from batch to batch: %r" % counts
    np.random.seed(0)
    m = collate(items)["view_mask"]
    assert 3 <= m[0].sum() < 8 and len({tuple(r) for r in m.tolist()}) > 1, "seed 0: rows differ across the samples"
    # fewer views than max_n_views: all of them are kept
    np.random.seed(1)
    b = make_collate_fn(True, 2, 31, mask_views=True)(_items(2, 5))
    assert b["view_mask"].shape == (2, 5) and [c[0].split("_")[1] for c in b["cameras"]] == list("01234")
    # without randomize_n_views there is nothing to mask
    assert "view_mask" not in make_collate_fn(False, mask_views=True)(_items(2, 5))


@pytest.mark.parametrize("seed", [0, 7])
def test_mask_views_false_is_the_function_it_was(seed):
    """The reference's two draws, restated: n_views = randint(min, min(total, max) + 1), then choice(total, n_views, replace=False).  The batch is built from
    exactly those views in that order, carries no mask, and np.random is left where those two calls leave it -- for the default and for the explicit False."""
    from mvn.datasets.utils import make_collate_fn
    items = _items(3, 12)
    np.random.seed(seed)
    n_views = np.random.randint(3, min(12, 8) + 1)
    indexes = np.random.choice(np.arange(12), size=n_views, replace=False)
    state = np.random.get_state()
    for collate in (make_collate_fn(True, 3, 8), make_collate_fn(True, 3, 8, mask_views=False)):
        np.random.seed(seed)
        batch = collate(items)
        after = np.random.get_state()
        assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
        assert "view_mask" not in batch
        assert batch["cameras"] == [[it["cameras"][i] for it in items] for i in indexes]
        assert np.array_equal(batch["images"], np.stack([np.stack([it["images"][i] for it in items], axis=0) for i in indexes], axis=0).swapaxes(0, 1))
        assert set(batch) == {"images", "detections", "cameras", "keypoints_3d", "indexes", "pred_keypoints_3d"}
