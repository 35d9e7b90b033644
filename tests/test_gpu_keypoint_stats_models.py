"""GPU (-m gpu): ``keypoint_stats`` through VolumetricTriangulationNet and CascadeTriangulationNet, and lt_plan_set_keypoint_stats through ctypes.  The small
models of tests/test_view_mask_cpu.py:vm_setup (3 samples, 4 views, 128 px, 32^3 voxels, 17 joints) and a copy whose volume_net.output_layer.weight is 250
times larger, so that its heatmaps are peaked; fp32 (channels-last logits) and bf16 (planar logits: the vectorised kernels), graph on and off.

  1. with the flag on, every tensor of the 7-tuple keeps the bits of the flag-off forward, and last_keypoint_stats agrees with the numpy statement
     (mvn.utils.volumetric.keypoint_stats) evaluated on the RETURNED volumes, coord_volumes and keypoints_3d: covariance within 1e-5 of the trace (the
     gate of tests/test_gpu_keypoint_stats_kernels.py), peak == volumes[b, j].flatten()[peak_index] == volumes[b, j].max() exactly;
  2. together with batch["view_mask"]; with copy_outputs off; ReLU volumes;
  3. the cascade gives the statistics of the volumetric model fed the algebraic pelvis;
  4. a batch above max_samples_per_launch: the chunks' statistics are concatenated;
  5. a train() forward leaves None;
  6. the C ABI: lt_plan_set_keypoint_stats + lt_plan_forward_vol / lt_plan_forward_cascade equals the Python host bit for bit, before or after the first
     forward; NULL / NULL restores the plain tail; its refusals."""
import copy

import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from test_gpu_cascade import CascadeCPlan
from test_gpu_plan_abi_alg import AlgCPlan
from test_gpu_view_mask_models import B, DEV, HW, J, NV, V, VolCPlan, _batch, _net, _same, _setup

pytestmark = pytest.mark.gpu
TOL = 1e-5
PEAKED = 250.0


_SDS = {}


def _models(golden_dir, peaked):
    """(cfgs, sds, inp, P) of vm_setup; peaked: the volumetric state dicts with the V2V output layer's weight times 250."""
    g, cfgs, sds, inp, P = _setup(golden_dir)
    if peaked:
        if "p" not in _SDS:
            s = {k: dict(v) for k, v in sds.items()}
            for name in ("vol_softmax", "vol_conf_norm"):
                s[name]["volume_net.output_layer.weight"] = sds[name]["volume_net.output_layer.weight"] * PEAKED
            _SDS["p"] = s
        sds = _SDS["p"]
    return g, cfgs, sds, inp, P


def _check_stats(tag, st, out, softmax=True):
    """last_keypoint_stats against the numpy statement on the returned tensors of the same forward."""
    from mvn.utils import op, volumetric
    kp, vols, coords = out[0], out[2], out[5]
    nb = kp.shape[0]
    assert isinstance(st, op.KeypointStats)
    assert st.peak.shape == (nb, J) and st.mass.shape == (nb, J) and st.peak_index.shape == (nb, J) and st.covariance.shape == (nb, J, 3, 3)
    assert st.peak.dtype == st.mass.dtype == st.covariance.dtype == torch.float32 and st.peak_index.dtype == torch.int32
    assert all(t.device == kp.device and not t.requires_grad for t in st)
    assert torch.equal(st.covariance, st.covariance.transpose(2, 3)) and bool(torch.isfinite(st.covariance).all())
    flat = vols.reshape(nb, J, -1)
    t = volumetric.keypoint_stats(flat.cpu().numpy(), coords.cpu().numpy(), kp.cpu().numpy(), softmax=softmax, from_probs=True, mass=st.mass.cpu().numpy())
    tr = np.trace(t.covariance, axis1=2, axis2=3)
    e = float((np.abs(st.covariance.cpu().double().numpy() - t.covariance).max(axis=(2, 3)) / np.where(tr > 0, tr, 1.0)).max())
    record("kstats/model " + tag, {"cov_err_over_trace": e, "tol": TOL})
    print("kstats/model %s: cov %.3e of the trace" % (tag, e))
    assert e <= TOL, "%s: covariance off by %.3e of the trace > %.1e" % (tag, e, TOL)
    at_peak = flat.gather(2, st.peak_index.long()[..., None])[..., 0]
    if softmax:
        assert torch.equal(st.peak, at_peak) and torch.equal(st.peak, flat.max(dim=2).values), tag + ": peak is not volumes[peak_index] == volumes.max()"
        assert bool((st.mass == 1.0).all())
    else:
        some = st.mass > 0          # a joint whose logits are all <= 0 has no mass: peak 0, covariance 0
        assert torch.equal(at_peak[some], flat.max(dim=2).values[some])
        assert not st.peak[~some].any() and not st.covariance[~some].any()
        assert float(((st.peak.double() - at_peak.double() / st.mass.double())[some].abs() / st.peak.double()[some].clamp_min(1e-30)).max()) <= TOL
        assert float(((st.mass.double() - flat.double().sum(2)).abs()[some] / st.mass.double()[some]).max()) <= TOL
    return t


def _same_stats(a, b, what):
    assert a is not None and b is not None, what
    for n, x, y in zip(a._fields, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), "%s: %s differs" % (what, n)


# ---- 1. the flag keeps the 7-tuple; the statistics are those of the returned heatmaps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("peaked", [False, True], ids=["smooth", "peaked"])
def test_flag_keeps_the_outputs_and_statistics_match_the_returned_volumes(golden_dir, peaked, dtype, graph):
    g, cfgs, sds, inp, P = _models(golden_dir, peaked)
    net = _net("vol_softmax", cfgs, sds, dtype, graph)
    images = inp["images"].to(DEV)
    assert net.keypoint_stats is False
    plain = net(images, None, _batch(inp))
    assert net.last_keypoint_stats is None
    net.keypoint_stats = True
    out = net(images, None, _batch(inp))
    st = net.last_keypoint_stats
    again = net(images, None, _batch(inp))          # the flagged plan's replay
    st2 = net.last_keypoint_stats
    net.keypoint_stats = False
    after = net(images, None, _batch(inp))
    torch.cuda.synchronize()
    what = "%s %s %s" % ("peaked" if peaked else "smooth", dtype, "graph" if graph else "eager")
    assert len(out) == 7
    _same(out, plain, what)
    _same(again, plain, what + " (replay)")
    _same(after, plain, what + " (flag off again)")
    assert net.last_keypoint_stats is None and len(net._plans) == 2          # its own plan, beside the plain one
    _same_stats(st, st2, what + " (replay)")
    t = _check_stats(what, st, out)
    if peaked:
        assert float(st.peak.max()) > 10.0 / V ** 3          # the copy with the larger output weights does have peaks


# ---- 2. with a view mask, without copies, ReLU volumes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_flag_with_a_view_mask_and_without_output_copies(golden_dir, dtype):
    g, cfgs, sds, inp, P = _models(golden_dir, True)
    images = inp["images"].to(DEV)
    net = _net("vol_conf_norm", cfgs, sds, dtype, True)
    plain = net(images, None, _batch(inp, g["masks"]))
    net.keypoint_stats = True
    out = net(images, None, _batch(inp, g["masks"]))
    st = net.last_keypoint_stats
    torch.cuda.synchronize()
    _same(out, plain, "masked %s" % dtype)
    _check_stats("masked %s" % dtype, st, out)
    unmasked = net(images, None, _batch(inp))
    assert not torch.equal(net.last_keypoint_stats.covariance, st.covariance)          # the mask reaches the statistics
    _check_stats("conf_norm %s" % dtype, net.last_keypoint_stats, unmasked)
    # views of the plan's buffers instead of fresh tensors: the same numbers
    net.copy_outputs = False
    views = net(images, None, _batch(inp, g["masks"]))
    torch.cuda.synchronize()
    _same_stats(net.last_keypoint_stats, st, "copy_outputs off %s" % dtype)
    assert torch.equal(views[0], out[0]) and torch.equal(views[2], out[2])


def test_flag_with_relu_volumes(golden_dir):
    g, cfgs, sds, inp, P = _models(golden_dir, False)
    cfg = copy.deepcopy(cfgs["vol_softmax"])
    cfg.model.volume_softmax = False
    images = inp["images"].to(DEV)
    net = _net("vol_softmax", {"vol_softmax": cfg}, sds, torch.float32, True)
    plain = net(images, None, _batch(inp))
    net.keypoint_stats = True
    out = net(images, None, _batch(inp))
    torch.cuda.synchronize()
    _same(out, plain, "relu")
    assert bool((net.last_keypoint_stats.mass > 0).any())
    _check_stats("relu f32", net.last_keypoint_stats, out, softmax=False)


# ---- 3. the cascade -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cascade_gives_the_statistics_of_the_volumetric_model_on_the_algebraic_pelvis(golden_dir, dtype):
    g, cfgs, sds, inp, P = _models(golden_dir, True)
    images, Pd = inp["images"].to(DEV), P.to(DEV)
    casc = _net("cascade", cfgs, sds, dtype, True)
    plain = casc(images, Pd, _batch(inp))
    assert casc.last_keypoint_stats is None
    casc.vol.keypoint_stats = True
    out = casc(images, Pd, _batch(inp))
    st = casc.last_keypoint_stats
    torch.cuda.synchronize()
    _same(out, plain, "cascade %s" % dtype)
    _check_stats("cascade %s" % dtype, st, out[0])
    _same_stats(casc.vol.last_keypoint_stats, st, "cascade.vol")
    vol = _net("vol_softmax", cfgs, sds, dtype, True)
    vol.keypoint_stats = True
    alone = vol(images, None, dict(_batch(inp), pred_keypoints_3d=out[1][0].cpu().numpy()))
    torch.cuda.synchronize()
    assert torch.equal(alone[0], out[0][0]) and torch.equal(alone[2], out[0][2])
    _same_stats(vol.last_keypoint_stats, st, "cascade vs the volumetric model on the algebraic pelvis, %s" % dtype)
    casc.vol.keypoint_stats = False
    casc(images, Pd, _batch(inp))
    assert casc.last_keypoint_stats is None and casc.vol.last_keypoint_stats is None


# ---- 4. more samples than one launch takes ----------------------------------------------------------------------------------------------------------------------------------------
def test_chunked_batch_concatenates_the_statistics(golden_dir, monkeypatch):
    g, cfgs, sds, inp, P = _models(golden_dir, True)
    images = inp["images"].to(DEV)
    net = _net("vol_softmax", cfgs, sds, torch.float32, True)
    net.keypoint_stats = True
    monkeypatch.setattr(net, "max_samples_per_launch", lambda *a: 2)          # 3 samples: chunks of 2 and 1
    with pytest.warns(UserWarning, match="sub-batches"):
        out = net(images, None, _batch(inp))
    st = net.last_keypoint_stats
    torch.cuda.synchronize()
    assert len(net._plans) == 2 and st.peak.shape == (B, J)          # a plan per chunk size
    _check_stats("chunked 2 + 1", st, out)
    # each chunk is a forward of its own samples: the same bits as that forward alone
    for lo, hi in ((0, 2), (2, 3)):
        part = {"cameras": [c[lo:hi] for c in _batch(inp)["cameras"]], "pred_keypoints_3d": inp["pred_keypoints_3d"][lo:hi]}
        alone = _net("vol_softmax", cfgs, sds, torch.float32, True)
        alone.keypoint_stats = True
        o = alone(images[lo:hi], None, part)
        torch.cuda.synchronize()
        assert torch.equal(o[0], out[0][lo:hi]) and torch.equal(o[2], out[2][lo:hi])
        for n, x, y in zip(st._fields, st, alone.last_keypoint_stats):
            assert torch.equal(x[lo:hi], y), "samples %d:%d %s" % (lo, hi, n)
    # the cascade walks the same chunks
    casc = _net("cascade", cfgs, sds, torch.float32, True)
    casc.vol.keypoint_stats = True
    monkeypatch.setattr(casc.vol, "max_samples_per_launch", lambda *a: 2)
    cout = casc(images, P.to(DEV), _batch(inp))
    torch.cuda.synchronize()
    assert casc.last_keypoint_stats.peak.shape == (B, J)
    _check_stats("cascade chunked 2 + 1", casc.last_keypoint_stats, cout[0])


# ---- 5. training ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_train_forward_leaves_no_statistics(golden_dir):
    g, cfgs, sds, inp, P = _models(golden_dir, False)
    net = _net("vol_softmax", cfgs, sds, torch.float32, True).to(DEV)          # training updates the parameters where they live
    net.keypoint_stats = True
    images = inp["images"][:1].to(DEV)
    batch = _batch(inp, nb=1)
    net(images, None, batch)
    assert net.last_keypoint_stats is not None and net.last_keypoint_stats.peak.shape == (1, J)
    net.train()
    out = net(images, None, batch)
    torch.cuda.synchronize()
    assert len(out) == 7 and out[0].requires_grad and net.last_keypoint_stats is None
    net.eval()
    net(images, None, batch)
    assert net.last_keypoint_stats is not None


# ---- 6. the C ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _c_buffers():
    return torch.full((B, J, 8), float("nan"), device=DEV), torch.full((B, J), -7, dtype=torch.int32, device=DEV)


def _untouched(rec, idx):
    return bool(torch.isnan(rec).all()) and bool((idx == -7).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_vol_plan_equals_the_python_host(golden_dir, dtype):
    from mvn.utils import op
    g, cfgs, sds, inp, P = _models(golden_dir, True)
    images = inp["images"].to(DEV).contiguous()
    lib = H.lib()
    net = _net("vol_softmax", cfgs, sds, dtype, True)
    net.keypoint_stats = True
    want = net(images, None, _batch(inp))
    want_st = net.last_keypoint_stats
    torch.cuda.synchronize()
    for first_forward_before in (False, True):          # the call may come before or after the plan's first forward
        cp = VolCPlan(cfgs["vol_softmax"], sds["vol_softmax"], dtype)
        try:
            if first_forward_before:
                kp, vols = cp.forward(images, inp)
                assert torch.equal(kp, want[0]) and torch.equal(vols, want[2])
            rec, idx = _c_buffers()
            assert lib.lt_plan_set_keypoint_stats(cp.plan, rec.data_ptr(), None) == -1 and "come together" in lib.lt_last_error().decode()
            assert lib.lt_plan_set_keypoint_stats(cp.plan, None, idx.data_ptr()) == -1
            H.check(lib.lt_plan_set_keypoint_stats(cp.plan, rec.data_ptr(), idx.data_ptr()), "lt_plan_set_keypoint_stats")
            for rnd in range(2):          # the setting persists
                rec.fill_(float("nan")); idx.fill_(-7)
                kp, vols = cp.forward(images, inp)
                assert torch.equal(kp, want[0]) and torch.equal(vols, want[2]), (dtype, first_forward_before, rnd)
                _same_stats(op.keypoint_stats_from_records(rec, idx), want_st, "C ABI %s first_forward_before=%s forward %d" % (dtype, first_forward_before, rnd))
            # other buffers
            rec2, idx2 = _c_buffers()
            H.check(lib.lt_plan_set_keypoint_stats(cp.plan, rec2.data_ptr(), idx2.data_ptr()), "lt_plan_set_keypoint_stats")
            rec.fill_(float("nan")); idx.fill_(-7)
            cp.forward(images, inp)
            assert _untouched(rec, idx)
            _same_stats(op.keypoint_stats_from_records(rec2, idx2), want_st, "C ABI second buffers")
            # NULL / NULL: the plain tail again
            H.check(lib.lt_plan_set_keypoint_stats(cp.plan, None, None), "lt_plan_set_keypoint_stats")
            rec2.fill_(float("nan")); idx2.fill_(-7)
            kp, vols = cp.forward(images, inp)
            assert torch.equal(kp, want[0]) and torch.equal(vols, want[2]) and _untouched(rec2, idx2) and _untouched(rec, idx)
        finally:
            cp.close()


def test_c_abi_refuses_algebraic_and_ransac_plans(golden_dir):
    g, cfgs, sds, inp, P = _models(golden_dir, False)
    lib = H.lib()
    rec, idx = _c_buffers()
    for model, name in ((H.LT_MODEL_ALG, "algebraic"), (H.LT_MODEL_RANSAC, "RANSAC")):
        ap = AlgCPlan(model, cfgs["alg"], sds["alg"], B, NV, HW, torch.float32)
        try:
            assert lib.lt_plan_set_keypoint_stats(ap.plan, rec.data_ptr(), idx.data_ptr()) == -2 and "volumetric" in lib.lt_last_error().decode(), name
            assert lib.lt_plan_set_keypoint_stats(ap.plan, None, None) == -2, name
        finally:
            ap.close()
    assert lib.lt_plan_set_keypoint_stats(None, rec.data_ptr(), idx.data_ptr()) == -1 and "null plan" in lib.lt_last_error().decode()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_cascade_plan_equals_the_python_host(golden_dir, dtype):
    from mvn.utils import op
    g, cfgs, sds, inp, P = _models(golden_dir, True)
    images = inp["images"].to(DEV).contiguous()
    lib = H.lib()
    net = _net("cascade", cfgs, sds, dtype, True)
    net.vol.keypoint_stats = True
    (kp, feats, vols, _, _, coords, base), (a3, _, _, _) = net(images, P.to(DEV), _batch(inp))
    want_st = net.last_keypoint_stats
    torch.cuda.synchronize()
    cp = CascadeCPlan(cfgs["alg"], sds["alg"], cfgs["vol_softmax"], sds["vol_softmax"], B, NV, HW, dtype)
    try:
        rec, idx = _c_buffers()
        assert lib.lt_plan_set_keypoint_stats(cp.plan, rec.data_ptr(), None) == -1
        o = cp.forward(images, inp["K"], inp["R"], inp["t"])          # a plain forward first
        assert torch.equal(o["kp"], kp) and _untouched(rec, idx)
        H.check(lib.lt_plan_set_keypoint_stats(cp.plan, rec.data_ptr(), idx.data_ptr()), "lt_plan_set_keypoint_stats")
        for rnd in range(2):
            rec.fill_(float("nan")); idx.fill_(-7)
            o = cp.forward(images, inp["K"], inp["R"], inp["t"])
            for name, ours, want in (("keypoints_3d", o["kp"], kp), ("alg_keypoints_3d", o["alg_kp3"], a3), ("base_points", o["base"], base), ("volumes", o["vols"], vols)):
                assert torch.equal(ours, want), "%s forward %d %s" % (dtype, rnd, name)
            _same_stats(op.keypoint_stats_from_records(rec, idx), want_st, "C ABI cascade %s forward %d" % (dtype, rnd))
        H.check(lib.lt_plan_set_keypoint_stats(cp.plan, None, None), "lt_plan_set_keypoint_stats")
        rec.fill_(float("nan")); idx.fill_(-7)
        o = cp.forward(images, inp["K"], inp["R"], inp["t"])
        assert torch.equal(o["kp"], kp) and torch.equal(o["vols"], vols) and _untouched(rec, idx)
    finally:
        cp.close()
