"""CPU: ragged view batches (samples with different numbers of views, no padding).  ``ragged_batch`` turns a padded batch with a view mask into the ragged
form; every refusal of the functional ops, the models and the three kernel entries fires without a GPU; the entries are exported with their declared
signatures."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import synth

ERR_INVALID = -1


def _cameras(inp, nb):
    from mvn.utils.multiview import Camera
    return [[Camera(inp["R"][v], inp["t"][v], inp["K"][v]) for _ in range(nb)] for v in range(inp["K"].shape[0])]


# ---- ragged_batch ---------------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_compacts_the_fixtures_masks(golden_dir):
    from mvn.datasets.utils import ragged_batch
    masks = np.load(os.path.join(golden_dir, "view_mask_small.npz"))["masks"]
    assert masks.tolist() == [[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 1]]
    B, NV = masks.shape
    inp = synth.make_inputs(B, NV, 32, seed=3)
    P = torch.randn(B, NV, 3, 4)
    cams = _cameras(inp, B)
    batch = {"cameras": cams, "view_mask": masks, "pred_keypoints_3d": inp["pred_keypoints_3d"]}
    im, Pr, rb = ragged_batch(inp["images"], P, batch)
    assert rb["view_counts"] == [4, 3, 2] and "view_mask" not in rb and "view_mask" in batch          # the caller's batch is left alone
    assert tuple(im.shape) == (9, 3, 32, 32) and tuple(Pr.shape) == (9, 3, 4) and len(rb["cameras"]) == 9
    assert rb["pred_keypoints_3d"] is batch["pred_keypoints_3d"]
    r = 0
    for b in range(B):
        for v in np.flatnonzero(masks[b]):
            assert torch.equal(im[r], inp["images"][b, v]) and torch.equal(Pr[r], P[b, v]) and rb["cameras"][r] is cams[v][b], (b, v)
            r += 1
    assert r == 9
    # bool / tensor masks, and no projections
    im2, none, rb2 = ragged_batch(inp["images"], None, dict(batch, view_mask=torch.from_numpy(masks).bool()))
    assert none is None and torch.equal(im2, im) and rb2["view_counts"] == [4, 3, 2]


def test_ragged_batch_of_a_full_batch_is_the_padded_batch_reshaped():
    from mvn.datasets.utils import ragged_batch
    inp = synth.make_inputs(2, 3, 32, seed=4)
    P = torch.randn(2, 3, 3, 4)
    cams = _cameras(inp, 2)
    for batch in ({"cameras": cams, "view_mask": np.ones((2, 3), dtype=bool)}, {"cameras": cams}):
        im, Pr, rb = ragged_batch(inp["images"], P, batch)
        assert torch.equal(im, inp["images"].reshape(6, 3, 32, 32)) and torch.equal(Pr, P.reshape(6, 3, 4)) and rb["view_counts"] == [3, 3]
        assert all(rb["cameras"][b * 3 + v] is cams[v][b] for b in range(2) for v in range(3))
    with pytest.raises(ValueError, match="sample 1 has 0 valid views"):
        ragged_batch(inp["images"], P, {"cameras": cams, "view_mask": np.array([[1, 1, 0], [0, 0, 0]])})


# ---- the host's check of the counts ---------------------------------------------------------------------------------------------------------------------
def test_view_counts_host():
    from mvn.utils import op
    counts, base, cap = op.view_counts_host([4, 3, 2], 9)
    assert counts.dtype == np.int32 and counts.tolist() == [4, 3, 2] and base.dtype == np.int32 and base.tolist() == [0, 4, 7, 9] and cap == 4
    for vc in (np.array([4, 3, 2]), torch.tensor([4, 3, 2]), torch.tensor([4, 3, 2], dtype=torch.int32)):
        assert op.view_counts_host(vc, 9)[1].tolist() == [0, 4, 7, 9]
    assert [op.view_counts_host([n, 1])[2] for n in (1, 4, 5, 8, 9, 32)] == [4, 4, 8, 8, 32, 32]          # NVcap: the smallest of 4, 8, 32
    with pytest.raises(ValueError, match="sums to 9 views over 3 samples, the batch holds 10"):
        op.view_counts_host([4, 3, 2], 10)
    with pytest.raises(ValueError, match="sample 1 has 0 views"):
        op.view_counts_host([4, 0, 2])
    with pytest.raises(ValueError, match="sample 2 has 1 view, 2 to 32"):
        op.view_counts_host([4, 3, 1], min_views=2)
    with pytest.raises(ValueError, match="sample 0 has 33 views"):
        op.view_counts_host([33, 2])
    with pytest.raises(ValueError, match="flat list"):
        op.view_counts_host([])
    with pytest.raises(ValueError, match="flat list"):
        op.view_counts_host([[4, 3]])
    with pytest.raises(TypeError, match="integers"):
        op.view_counts_host([4.0, 3.0])


# ---- refusals, all before any device work -------------------------------------------------------------------------------------------------------------------
def test_functional_ops_refuse_before_any_launch():
    from mvn.utils import multiview, op
    hm, P, cv, conf = torch.zeros(9, 32, 8, 8), torch.zeros(9, 3, 4), torch.zeros(3, 4, 4, 16, 3), torch.ones(9, 32)
    with pytest.raises(ValueError, match="sums to 8"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[4, 2, 2])
    with pytest.raises(ValueError, match="sample 2 has 0 views"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[4, 5, 0])
    with pytest.raises(ValueError, match="sample 0 has 33 views"):
        op.unproject_heatmaps(torch.zeros(35, 32, 8, 8), torch.zeros(35, 3, 4), cv[:2], "softmax", view_counts=[33, 2])
    with pytest.raises(ValueError, match="holds 3 samples"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[5, 4])
    with pytest.raises(ValueError, match=r"\(T, 3, 4\)"):
        op.unproject_heatmaps(hm, P[:8], cv, "softmax", view_counts=[4, 3, 2])
    with pytest.raises(ValueError, match=r"\(T, C, h, w\)"):
        op.unproject_heatmaps(hm[None], P, cv, "softmax", view_counts=[4, 3, 2])
    with pytest.raises(NotImplementedError, match="drop the missing views"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[4, 3, 2], view_mask=np.ones((3, 4), dtype=bool))
    with pytest.raises(NotImplementedError, match="frame_index"):
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[4, 3, 2], frame_index=[0, 1, 2])
    with pytest.raises(NotImplementedError, match="inference only"):
        op.unproject_heatmaps(hm.clone().requires_grad_(True), P, cv, "softmax", view_counts=[4, 3, 2])
    with pytest.raises(NotImplementedError, match="inference only"):
        op.unproject_heatmaps(hm, P, cv, "conf", conf.clone().requires_grad_(True), view_counts=[4, 3, 2])
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):          # valid arguments on the CPU: no fall-back to eager torch
        op.unproject_heatmaps(hm, P, cv, "softmax", view_counts=[4, 3, 2])
    pts, cf = torch.zeros(9, 17, 2), torch.ones(9, 17)
    with pytest.raises(ValueError, match="sample 2 has 1 view, 2 to 32"):
        multiview.triangulate_batch_of_points(P, pts, cf, view_counts=[4, 4, 1])
    with pytest.raises(ValueError, match="sums to 8"):
        multiview.triangulate_batch_of_points(P, pts, cf, view_counts=[4, 2, 2])
    with pytest.raises(ValueError, match=r"\(T, J, 2\)"):
        multiview.triangulate_batch_of_points(P, pts[None], cf, view_counts=[4, 3, 2])
    with pytest.raises(NotImplementedError, match="drop the missing views"):
        multiview.triangulate_batch_of_points(P, pts, cf, view_counts=[4, 3, 2], view_mask=np.ones((3, 4), dtype=bool))
    with pytest.raises(NotImplementedError, match="inference only"):
        multiview.triangulate_batch_of_points(P, pts.clone().requires_grad_(True), cf, view_counts=[4, 3, 2])
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):
        multiview.triangulate_batch_of_points(P, pts, cf, view_counts=[4, 3, 2])


def _ragged_inputs(mask=((1, 1, 1, 1), (1, 0, 1, 1)), hw=64):
    from mvn.datasets.utils import ragged_batch
    mask = np.array(mask)
    inp = synth.make_inputs(mask.shape[0], mask.shape[1], hw, seed=1)
    return ragged_batch(inp["images"], torch.zeros(mask.shape + (3, 4)),
                        {"cameras": _cameras(inp, mask.shape[0]), "view_mask": mask, "pred_keypoints_3d": inp["pred_keypoints_3d"]})


def test_models_without_a_ragged_plan_refuse_the_batch_and_say_what_to_do():
    from mvn.models.triangulation import AlgebraicTriangulationNet, CascadeTriangulationNet, RANSACTriangulationNet, VolumetricTriangulationNet
    im, Pr, rb = _ragged_inputs()
    rcfg = synth.alg_config(18, False, 17)
    rcfg.model.direct_optimization = True
    nets = [RANSACTriangulationNet(rcfg, device="cpu"),
            CascadeTriangulationNet(AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu"),
                                    VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu"))]
    for net in nets:
        for mode in (net.eval, net.train):
            mode()
            with pytest.raises(NotImplementedError, match=r"view_counts.*pass batch\['view_mask'\] instead"):
                net(im, Pr, rb)


def test_volumetric_model_refuses_bad_ragged_batches_before_any_launch():
    from mvn.models.triangulation import VolumetricTriangulationNet
    im, Pr, rb = _ragged_inputs()
    net = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    with pytest.raises(ValueError, match="sums to 8 views over 2 samples, the batch holds 7"):
        net(im, None, dict(rb, view_counts=[4, 4]))
    with pytest.raises(ValueError, match="sample 1 has 0 views"):
        net(im, None, dict(rb, view_counts=[7, 0]))
    with pytest.raises(ValueError, match="sample 0 has 33 views"):
        net(torch.zeros(35, 3, 64, 64), None, dict(rb, view_counts=[33, 2]))
    with pytest.raises(ValueError, match="flat list of the T = 7 cameras, got 6"):
        net(im, None, dict(rb, cameras=rb["cameras"][:6]))
    with pytest.raises(ValueError, match="flat list of the T = 7 cameras"):
        net(im, None, dict(rb, cameras=[[c] for c in rb["cameras"]]))
    with pytest.raises(ValueError, match="names 2 samples.*has 1 entries"):
        net(im, None, dict(rb, pred_keypoints_3d=rb["pred_keypoints_3d"][:1]))
    with pytest.raises(ValueError, match=r"\(T, 3, H, W\)"):
        net(im[None], None, rb)
    with pytest.raises(NotImplementedError, match="drop the missing views"):
        net(im, None, dict(rb, view_mask=np.ones((2, 4), dtype=bool)))
    with pytest.raises(NotImplementedError, match="cuboid_frame.*padded batch"):
        net(im, None, dict(rb, cuboid_frame=[0, 1]))
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):          # a good ragged batch on the CPU: no fall-back
        net(im, None, rb)
    net.train()
    with pytest.raises(NotImplementedError, match="inference only.*call eval"):
        net(im, None, rb)


def test_algebraic_model_refuses_bad_ragged_batches_before_any_launch():
    from mvn.models.triangulation import AlgebraicTriangulationNet
    im, Pr, rb = _ragged_inputs()
    net = AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu").eval()
    with pytest.raises(ValueError, match="sums to 8 views over 2 samples, the batch holds 7"):
        net(im, Pr, dict(rb, view_counts=[4, 4]))
    with pytest.raises(ValueError, match="sample 1 has 1 view, 2 to 32"):
        net(im, Pr, dict(rb, view_counts=[6, 1]))
    with pytest.raises(ValueError, match="sample 0 has 33 views"):
        net(torch.zeros(35, 3, 64, 64), torch.zeros(35, 3, 4), dict(rb, view_counts=[33, 2]))
    with pytest.raises(ValueError, match=r"\(T, 3, 4\) = \(7, 3, 4\)"):
        net(im, torch.zeros(2, 4, 3, 4), rb)
    with pytest.raises(ValueError, match=r"\(T, 3, H, W\)"):
        net(im[None], Pr, rb)
    with pytest.raises(NotImplementedError, match="drop the missing views"):
        net(im, Pr, dict(rb, view_mask=np.ones((2, 4), dtype=bool)))
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):          # a good ragged batch on the CPU: no fall-back
        net(im, Pr, rb)
    net.keypoint_stats = True
    with pytest.raises(NotImplementedError, match="keypoint_stats.*view_mask.*instead"):
        net(im, Pr, rb)
    net.keypoint_stats = False
    net.train()
    with pytest.raises(NotImplementedError, match="inference only.*call eval"):
        net(im, Pr, rb)


def test_ragged_algebraic_plan():
    """The launches of a plain plan of T images, its own key, and the block of the B + 1 offsets."""
    from mvn.models.triangulation import AlgebraicTriangulationNet
    alg = AlgebraicTriangulationNet(synth.alg_config(18, True, 17), device="cpu").eval()
    keys = [alg._plan_key(3, 4, 64, 64, "cpu"), alg._plan_key(3, 4, 64, 64, "cpu", True), alg._plan_key(3, 4, 64, 64, "cpu", ragged=9),
            alg._plan_key(3, 4, 64, 64, "cpu", ragged=10), alg._plan_key(3, 8, 64, 64, "cpu", ragged=9), alg._plan_key(2, 4, 64, 64, "cpu", ragged=9)]
    assert len(set(keys)) == len(keys) and alg._plan_key(3, 4, 64, 64, "cpu") == alg._plan_key(3, 4, 64, 64, "cpu", False, False, None)
    plain, rag = alg._build_plan(9, 1, 64, 64, "cpu", dry_run=True), alg._build_plan(3, 4, 64, 64, "cpu", dry_run=True, ragged=9)
    assert _launches(rag["plan"]) == _launches(plain["plan"]) and rag["ragged"] == 9 and plain["ragged"] is None
    assert tuple(rag["view_base"].shape) == (4,) and rag["view_base"].dtype == torch.int32 and "view_base" not in plain
    assert rag["x_in"].shape[0] == 9 and tuple(rag["kp2d"].shape) == (9, 17, 2)


def _launches(plan):
    return [(meta["kind"], meta["label"]) for _, meta in plan.ops]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ragged_volumetric_plan(dt):
    """The backbone at T images, lt_unproject_grid_ragged_fwd in the gather's place, otherwise the launch list of a plain plan of T images; its own key;
    view_base behind the rotations of the geometry block's host slot; other counts with the same (B, T, NVcap) reuse the plan."""
    from mvn.models.triangulation import VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    vol.compute_dtype = dt
    B, T, cap = 3, 9, 4
    keys = [vol._plan_key(B, cap, 64, 64, "cpu"), vol._plan_key(B, cap, 64, 64, "cpu", True), vol._plan_key(B, cap, 64, 64, "cpu", ragged=T),
            vol._plan_key(B, cap, 64, 64, "cpu", ragged=T + 1), vol._plan_key(B, 8, 64, 64, "cpu", ragged=T), vol._plan_key(B + 1, cap, 64, 64, "cpu", ragged=T)]
    assert len(set(keys)) == len(keys)
    assert vol._plan_key(B, cap, 64, 64, "cpu") == vol._plan_key(B, cap, 64, 64, "cpu", False, False, None, None)
    plain = vol._build_plan(T, 1, 64, 64, "cpu", dry_run=True)          # a plain plan of T images (T samples of one view)
    before = _launches(plain["plan"])
    masked = vol._build_plan(B, cap, 64, 64, "cpu", dry_run=True, masked=True)
    rag = vol._build_plan(B, cap, 64, 64, "cpu", dry_run=True, ragged=T)
    assert _launches(plain["plan"]) == before and rag["ragged"] == T and plain["ragged"] is None and masked["ragged"] is None
    kinds = lambda P: [k for k, _ in _launches(P["plan"])]
    u, um = kinds(rag).index("unproject"), kinds(masked).index("unproject")
    # in front of the gather: the launches of a plan of T images, label for label; behind it: those of a plan of B samples
    assert kinds(plain).index("unproject") == u and _launches(rag["plan"])[:u] == before[:u]
    assert _launches(rag["plan"])[u:] == _launches(masked["plan"])[um:]
    assert rag["plan"].ops[0][1] is not None and rag["x_in"].shape[0] == T and masked["x_in"].shape[0] == B * cap
    info = lambda P: P["plan"].ops[kinds(P).index("unproject")][1]["info"]
    assert info(rag)["entry"] == "lt_unproject_grid_ragged_fwd" and info(masked)["entry"] == "lt_unproject_grid_masked_fwd"
    assert info(plain)["entry"] == "lt_unproject_grid_fwd" and info(rag)["NV"] == cap and info(rag)["cuboids"] == B
    assert tuple(info(rag)["feats"].shape[:1]) == (T,) and tuple(info(rag)["vol"].shape[:1]) == (B,)
    # the geometry block: proj T*12 | pos, centre, rot B*15 | view_base B + 1
    n = T * 12 + B * 15
    assert rag["geo"].numel() == n + B + 1 and rag["o_vb"] == n and rag["offs"] == (T * 12, T * 12 + 3 * B, T * 12 + 6 * B)


def test_view_base_is_written_into_the_geometry_block_and_other_counts_reuse_the_plan():
    from mvn.models.triangulation import VolumetricTriangulationNet
    from mvn.utils import op
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    im, Pr, rb = _ragged_inputs(((1, 1, 1, 1), (1, 0, 1, 1), (0, 1, 0, 1)))
    assert rb["view_counts"] == [4, 3, 2]
    rag = vol._build_plan(3, 4, 64, 64, "cpu", dry_run=True, ragged=9)
    n = rag["o_vb"]
    for counts, want in (([4, 3, 2], [0, 4, 7, 9]), ([2, 3, 4], [0, 2, 5, 9])):
        base = op.view_counts_host(counts, 9)[1]
        vol._host_geometry(dict(rb, cameras=[[c] for c in rb["cameras"]], view_base=base), 3, (64, 64), rag)
        assert rag["geo_host"].view(torch.int32)[n:n + 4].tolist() == want
        assert op.view_counts_host(counts, 9)[2] == 4          # the same (B, T, NVcap): the same key, the same plan
    # the floats in front are those of a plain plan of the 9 images
    plain = vol._build_plan(9, 1, 64, 64, "cpu", dry_run=True)
    vol._host_cameras({"cameras": [[c] for c in rb["cameras"]]}, 9, (64, 64), plain)
    assert torch.equal(rag["geo_host"][:9 * 12], plain["geo_host"][:9 * 12])


def test_c_entry_points_check_their_arguments():
    lib = H.lib()
    i32, f32, vp = C.c_int32, C.c_float, C.c_void_p
    for name in ("lt_unproject_ragged_fwd", "lt_unproject_grid_ragged_fwd", "lt_alg_tail_ragged_fwd"):
        assert hasattr(C.CDLL(H.LIB_PATH), name) and name in H.SIGNATURES, name
    assert H.SIGNATURES["lt_unproject_ragged_fwd"] == (C.c_int, [i32] + [vp] * 6 + [i32] * 10 + [vp])
    assert H.SIGNATURES["lt_unproject_grid_ragged_fwd"] == (C.c_int, [i32] + [vp] * 5 + [f32, i32] + [vp] * 4 + [i32] * 8 + [vp])
    assert H.SIGNATURES["lt_alg_tail_ragged_fwd"] == (C.c_int, [vp, vp, i32, vp, f32, f32] + [vp] * 4 + [i32] * 4 + [vp])
    err = lambda: lib.lt_last_error().decode()
    S = H.AGG["sum"]
    #                                  dtype    feats proj coords conf base out B  T  cap C  h  w  v0 v1 v2  agg
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, None, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "null view_base" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, None, 1, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, None, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, None, None, 1, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, 1, None, 3, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 0, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "B 0" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 3, 0, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "T 0" in err()
    for cap in (0, 33, -1):
        assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 3, 9, cap, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "NVcap %d" % cap in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, 9, None) == ERR_INVALID and "aggregation 9" in err()
    assert lib.lt_unproject_ragged_fwd(H.LT_F32, 1, 1, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, H.AGG["conf_norm"], None) == ERR_INVALID and "confidences" in err()
    assert lib.lt_unproject_ragged_fwd(7, 1, 1, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 4, 4, 16, S, None) == ERR_INVALID and "dtype 7" in err()
    #                                       dtype  feats proj pos cen rot step cmu coords conf base out B  T  cap C  h  w  V  agg
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, None, 1, 3, 9, 4, 32, 8, 8, 16, S, None) == ERR_INVALID and "null view_base" in err()
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, None, None, 1, 1, 3, 9, 4, 32, 8, 8, 16, S, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, None, 1, 1, 1.0, 0, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 16, S, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, 1, 1, 0, 9, 4, 32, 8, 8, 16, S, None) == ERR_INVALID and "B 0" in err()
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, 1, 1, 3, -2, 4, 32, 8, 8, 16, S, None) == ERR_INVALID and "T -2" in err()
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, 1, 1, 3, 9, 40, 32, 8, 8, 16, S, None) == ERR_INVALID and "NVcap 40" in err()
    assert lib.lt_unproject_grid_ragged_fwd(H.LT_F32, 1, 1, 1, 1, 1, 1.0, 0, 1, None, 1, 1, 3, 9, 4, 32, 8, 8, 16, -1, None) == ERR_INVALID and "aggregation -1" in err()
    #                                 kp_hm raw ld proj sx   sy  base k2   cf    k3 B  T  cap J
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, 1, 1.0, 1.0, None, None, None, 1, 3, 9, 4, 17, None) == ERR_INVALID and "null view_base" in err()
    assert lib.lt_alg_tail_ragged_fwd(None, None, 17, 1, 1.0, 1.0, 1, None, None, 1, 3, 9, 4, 17, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, None, 1.0, 1.0, 1, None, None, 1, 3, 9, 4, 17, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, 1, 1.0, 1.0, 1, None, None, None, 3, 9, 4, 17, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, 1, 1.0, 1.0, 1, None, None, 1, 0, 9, 4, 17, None) == ERR_INVALID and "B 0" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, 1, 1.0, 1.0, 1, None, None, 1, 3, 0, 4, 17, None) == ERR_INVALID and "T 0" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, 1, 1.0, 1.0, 1, None, None, 1, 3, 9, 33, 17, None) == ERR_INVALID and "NVcap 33" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, None, 17, 1, 1.0, 1.0, 1, None, None, 1, 3, 9, 0, 17, None) == ERR_INVALID and "NVcap 0" in err()
    assert lib.lt_alg_tail_ragged_fwd(1, 1, 16, 1, 1.0, 1.0, 1, None, None, 1, 3, 9, 4, 17, None) == ERR_INVALID and "ld_conf 16" in err()


def test_plan_entries_check_their_arguments():
    """The four plan-level entries: exported with the declared signatures; null arguments, a bad NVcap, a T that B samples cannot hold and a RANSAC model are
    LT_ERR_INVALID before any device call."""
    lib = H.lib()
    i32, vp = C.c_int32, C.c_void_p
    for name in ("lt_plan_create_vol_ragged", "lt_plan_forward_vol_ragged", "lt_plan_create_alg_ragged", "lt_plan_forward_alg_ragged"):
        assert hasattr(C.CDLL(H.LIB_PATH), name) and name in H.SIGNATURES, name
    assert H.SIGNATURES["lt_plan_create_vol_ragged"] == (C.c_int, [C.POINTER(H.VolPlanConfig), i32, C.POINTER(H.NamedTensor), i32, C.POINTER(vp)])
    assert H.SIGNATURES["lt_plan_create_alg_ragged"] == (C.c_int, [C.POINTER(H.AlgPlanConfig), i32, C.POINTER(H.NamedTensor), i32, C.POINTER(vp)])
    assert H.SIGNATURES["lt_plan_forward_vol_ragged"] == (C.c_int, [vp] * 14) and H.SIGNATURES["lt_plan_forward_alg_ragged"] == (C.c_int, [vp] * 9)
    err = lambda: lib.lt_last_error().decode()
    w = (H.NamedTensor * 1)()
    plan = vp()
    vc = H.VolPlanConfig()
    vc.dtype, vc.num_layers, vc.num_joints, vc.B, vc.NV, vc.H, vc.W, vc.volume_size, vc.cuboid_side, vc.aggregation = H.LT_F32, 18, 17, 3, 4, 64, 64, 32, 2500.0, H.AGG["softmax"]
    assert lib.lt_plan_create_vol_ragged(None, 9, w, 1, C.byref(plan)) == ERR_INVALID and "null argument" in err()
    assert lib.lt_plan_create_vol_ragged(C.byref(vc), 9, None, 1, C.byref(plan)) == ERR_INVALID and "null argument" in err()
    assert lib.lt_plan_create_vol_ragged(C.byref(vc), 9, w, 1, None) == ERR_INVALID and "null argument" in err()
    for T in (0, 2, 13):          # B = 3 samples of 1 .. 4 views hold 3 .. 12 images
        assert lib.lt_plan_create_vol_ragged(C.byref(vc), T, w, 1, C.byref(plan)) == ERR_INVALID and "T %d images" % T in err()
    for cap in (0, 33):
        vc.NV = cap
        assert lib.lt_plan_create_vol_ragged(C.byref(vc), 9, w, 1, C.byref(plan)) == ERR_INVALID and ("NV %d" % cap in err() or "bad shape" in err())
    vc.NV, vc.dtype = 4, 7
    assert lib.lt_plan_create_vol_ragged(C.byref(vc), 9, w, 1, C.byref(plan)) == ERR_INVALID and "dtype 7" in err()
    ac = H.AlgPlanConfig()
    ac.model, ac.dtype, ac.num_layers, ac.num_joints, ac.B, ac.NV, ac.H, ac.W = H.LT_MODEL_ALG, H.LT_F32, 18, 17, 3, 4, 64, 64
    assert lib.lt_plan_create_alg_ragged(None, 9, w, 1, C.byref(plan)) == ERR_INVALID and "null argument" in err()
    assert lib.lt_plan_create_alg_ragged(C.byref(ac), 9, w, 0, C.byref(plan)) == ERR_INVALID and "null argument" in err()
    for T in (5, 13):          # at least two views per sample: 6 .. 12 images
        assert lib.lt_plan_create_alg_ragged(C.byref(ac), T, w, 1, C.byref(plan)) == ERR_INVALID and "T %d images" % T in err()
    ac.NV = 33
    assert lib.lt_plan_create_alg_ragged(C.byref(ac), 9, w, 1, C.byref(plan)) == ERR_INVALID and "NV 33" in err()
    ac.NV, ac.model = 4, H.LT_MODEL_RANSAC
    assert lib.lt_plan_create_alg_ragged(C.byref(ac), 9, w, 1, C.byref(plan)) == ERR_INVALID and "LT_MODEL_ALG only" in err()
    assert not plan.value
    assert lib.lt_plan_forward_vol_ragged(None, 1, 1, 1, 1, 1, 1, None, 1, None, None, None, None, None) == ERR_INVALID and "null argument" in err()
    assert lib.lt_plan_forward_alg_ragged(None, 1, 1, 1, 1, None, None, None, None) == ERR_INVALID and "null argument" in err()


def test_no_existing_plan_changes_its_gather():
    """A guard, not evidence of the feature: the plain, masked and indexed plans record the gather entries they always did (only a plan built with
    ``ragged=`` records lt_unproject_grid_ragged_fwd, test_ragged_volumetric_plan)."""
    from mvn.models.triangulation import VolumetricTriangulationNet
    vol = VolumetricTriangulationNet(synth.vol_config(18, 32, "softmax"), device="cpu").eval()
    for kw, entry in (({}, "lt_unproject_grid_fwd"), ({"masked": True}, "lt_unproject_grid_masked_fwd"), ({"cuboids": 3}, "lt_unproject_grid_indexed_fwd")):
        plan = vol._build_plan(2, 4, 64, 64, "cpu", dry_run=True, **kw)
        un = [meta for _, meta in plan["plan"].ops if meta["kind"] == "unproject"]
        assert len(un) == 1 and un[0]["info"]["entry"] == entry
