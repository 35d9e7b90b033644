"""GPU (-m gpu): ``keypoint_stats`` through AlgebraicTriangulationNet and CascadeTriangulationNet, and lt_plan_set_alg_keypoint_stats through ctypes.  The
small algebraic model of tests/test_view_mask_cpu.py:vm_setup (ResNet-18 backbone, 4 views of 128 px, 17 joints, with the confidence head), 2 samples.

  1. the flag on or off leaves the 4-tuple bit-identical; unflagged forwards keep their plan and its launch list; the flagged plan is a plan of its own;
  2. last_keypoint_stats equals the functional ops (op.integrate_tensor_2d_with_stats on the raw heatmaps, multiview.triangulate_batch_of_points_with_stats on
     the returned tensors) bit for bit, and the numpy statement at the gates of tests/test_gpu_alg_keypoint_stats_kernels.py;
  3. with batch["view_mask"]: the statistics of the model run on the compacted views;
  4. a train() forward leaves None;
  5. the cascade's last_alg_keypoint_stats is the algebraic model's, last_keypoint_stats stays the volumetric stage's;
  6. the C ABI: lt_plan_set_alg_keypoint_stats before and after the first forward, switched off again, on an algebraic and a cascade plan, equal to the Python
     host bit for bit; its refusals; lt_plan_set_keypoint_stats on an algebraic plan still returns -2."""
import numpy as np
import pytest
import torch

import lt_hip as H
from gpu_util import record
from test_gpu_cascade import CascadeCPlan
from test_gpu_plan_abi_alg import AlgCPlan
from test_gpu_view_mask_models import DEV, HW, J, NV, _batch, _net, _same, _setup

pytestmark = pytest.mark.gpu
TOL = 1e-5
FLOOR_2D = 1e-6
NB = 2


def _inputs(golden_dir):
    g, cfgs, sds, inp, P = _setup(golden_dir)
    return cfgs, sds, inp, inp["images"][:NB].to(DEV).contiguous(), P[:NB].to(DEV)


def _same_stats(a, b, what, on=None):
    """Bitwise, field by field; on: (B, NV) bool, compare the per-view fields on those views only (a masked view's values are unspecified)."""
    assert a is not None and b is not None, what
    for n, x, y in zip(a._fields, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, n)
        if on is not None and n != "covariance":
            x, y = x[on], y[on]
        assert torch.equal(x, y), "%s: %s differs" % (what, n)


def _check_stats(tag, st, out, proj, net, raw_hm=None, mask=None):
    """last_keypoint_stats of a forward against its returned 4-tuple: shapes, the functional ops bit for bit, the numpy statement at the gates."""
    from mvn.utils import multiview, op
    kp3d, kp2d, heatmaps, conf = out
    nb = kp3d.shape[0]
    h, w = heatmaps.shape[-2:]
    on = torch.ones(nb, NV, dtype=torch.bool) if mask is None else torch.from_numpy(np.asarray(mask).astype(bool))
    assert isinstance(st, op.AlgKeypointStats)
    assert st.peak.shape == st.mass.shape == st.peak_index.shape == st.reprojection_error.shape == (nb, NV, J)
    assert st.covariance_2d.shape == (nb, NV, J, 2, 2) and st.covariance.shape == (nb, J, 3, 3) and st.peak_index.dtype == torch.int32
    assert all(t.device == kp3d.device and not t.requires_grad for t in st) and all(t.dtype == torch.float32 for i, t in enumerate(st) if i != 1)
    assert torch.equal(st.covariance, st.covariance.transpose(2, 3)) and bool(torch.isfinite(st.covariance).all())
    assert torch.equal(st.covariance_2d[on], st.covariance_2d.transpose(3, 4)[on])
    # softmax mode: the peak is the returned heatmap's value at the peak pixel, which is its maximum
    flat = heatmaps.reshape(nb, NV, J, -1)
    assert torch.equal(st.peak, flat.gather(3, st.peak_index.long()[..., None])[..., 0]) and torch.equal(st.peak, flat.max(dim=3).values) and bool((st.mass == 1).all())
    # the functional triangulation on the returned tensors
    k3, err, cov = multiview.triangulate_batch_of_points_with_stats(proj, kp2d, conf, st.covariance_2d, view_mask=mask)
    assert torch.equal(k3, kp3d) and torch.equal(cov, st.covariance), tag + ": triangulate_batch_of_points_with_stats differs"
    assert torch.equal(err[on], st.reprojection_error[on]) and bool(torch.isnan(st.reprojection_error[~on]).all())
    # the numpy statement
    sx, sy = float(np.float32(HW / w)), float(np.float32(HW / h))
    if raw_hm is not None:          # the functional soft-argmax on the network's raw heatmaps (times the multiplier): the same records
        c, p, (peak, pidx, mass, cov_hm) = op.integrate_tensor_2d_with_stats(raw_hm.reshape(nb * NV, J, h, w) * net.heatmap_multiplier, net.heatmap_softmax)
        assert torch.equal(p.reshape(heatmaps.shape), heatmaps) and torch.equal(peak.reshape(nb, NV, J), st.peak) and torch.equal(pidx.reshape(nb, NV, J), st.peak_index)
        assert torch.equal(mass.reshape(nb, NV, J), st.mass)
        S = torch.tensor([sx, sy], dtype=torch.float64, device=cov_hm.device)
        want2 = (cov_hm.double() * S[:, None] * S[None, :]).float().reshape(nb, NV, J, 2, 2)
        assert torch.equal(want2[on], st.covariance_2d[on]), tag + ": covariance_2d is not S Sigma_hm S rounded once"
        speak, sidx, smass, scov = multiview.heatmap_stats_2d((raw_hm.reshape(nb * NV, J, h, w) * net.heatmap_multiplier).cpu().numpy(), 1.0, True, coords=c.cpu().numpy())
        assert np.array_equal(sidx.reshape(nb, NV, J), st.peak_index.cpu().numpy())
        e_peak = float((np.abs(st.peak.cpu().double().numpy().reshape(-1, J) - speak) / speak).max())
        tr2 = scov[..., 0, 0] + scov[..., 1, 1]
        e_c2 = float((np.abs(cov_hm.cpu().double().numpy() - scov).max(axis=(2, 3)) / np.maximum(TOL * tr2, FLOOR_2D)).max())
        assert e_peak <= TOL and e_c2 <= 1.0, (tag, e_peak, e_c2)
    terr, tcov = multiview.triangulation_stats(proj.cpu().numpy(), kp2d.cpu().numpy(), conf.cpu().numpy(), st.covariance_2d.cpu().numpy(), kp3d.cpu().numpy(),
                                               None if mask is None else np.asarray(mask))
    onn = on.numpy()
    e_err = float((np.abs(st.reprojection_error.cpu().double().numpy() - terr)[onn] / terr[onn]).max())
    tr = np.trace(tcov, axis1=2, axis2=3)
    e_cov = float((np.abs(st.covariance.cpu().double().numpy() - tcov).max(axis=(2, 3)) / tr).max())
    record("alg_kstats/model " + tag, {"reproj_rel": e_err, "cov3d_err_over_trace": e_cov, "tol": TOL})
    print("alg_kstats/model %s: reproj %.3e, cov3d %.3e of the trace" % (tag, e_err, e_cov))
    assert e_err <= TOL and e_cov <= TOL, (tag, e_err, e_cov)


# ---- 1, 2. the flag keeps the 4-tuple; the statistics are those of the returned tensors ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_flag_keeps_the_outputs_and_the_unflagged_plan(golden_dir, dtype):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    net = _net("alg", cfgs, sds, dtype, True)
    assert net.keypoint_stats is False and net.last_keypoint_stats is None
    plain = net(images, Pd, _batch(inp, nb=NB))
    assert net.last_keypoint_stats is None and len(net._plans) == 1
    (key0, plan0), = [(k, v["plan"]) for k, v in net._plans.items()]
    launches0 = [(m["kind"], m["label"]) for _, m in plan0.ops]
    net.keypoint_stats = True
    out = net(images, Pd, _batch(inp, nb=NB))
    st = net.last_keypoint_stats
    again = net(images, Pd, _batch(inp, nb=NB))
    st2 = net.last_keypoint_stats
    net.keypoint_stats = False
    after = net(images, Pd, _batch(inp, nb=NB))
    torch.cuda.synchronize()
    what = "alg %s" % dtype
    assert len(out) == 4
    _same(out, plain, what)
    _same(again, plain, what + " (replay)")
    _same(after, plain, what + " (flag off again)")
    assert net.last_keypoint_stats is None and len(net._plans) == 2          # the flagged plan beside the plain one, which was reused
    assert net._plans[key0]["plan"] is plan0 and [(m["kind"], m["label"]) for _, m in plan0.ops] == launches0          # the unflagged plan and its launch list
    assert net._plan_key(NB, NV, HW, HW, images.device) == key0 and net._plan_key(NB, NV, HW, HW, images.device, False, True) in net._plans
    _same_stats(st, st2, what + " (replay)")
    # the two plans record the same launches; only the flagged one's soft-argmax op carries the statistics' buffers
    Pp = net._build_plan(NB, NV, HW, HW, images.device, dry_run=True)
    Pf = net._build_plan(NB, NV, HW, HW, images.device, dry_run=True, stats=True)
    kinds = lambda P: [(m["kind"], m["label"]) for _, m in P["plan"].ops]
    assert kinds(Pp) == kinds(Pf) and Pp["kstats"] is None and Pf["plan"].ops[-1][1]["info"]["entry"] == "lt_softargmax2d_stats_fwd"
    _check_stats(what, st, out, Pd, net)
    if dtype == torch.float32:
        assert float(st.reprojection_error.max()) > 0 and float(st.covariance_2d[..., 0, 0].min()) > 0


def test_statistics_equal_the_functional_ops_on_the_networks_heatmaps(golden_dir):
    """The raw heatmaps of the forward are the flagged plan's NCHW buffer; the functional soft-argmax on them gives the model's heatmaps and 2D records bit for
    bit."""
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    net = _net("alg", cfgs, sds, torch.float32, True)
    net.keypoint_stats = True
    out = net(images, Pd, _batch(inp, nb=NB))
    st = net.last_keypoint_stats
    raw = net._plans[net._plan_key(NB, NV, HW, HW, images.device, False, True)]["hm_nchw"].clone().reshape(out[2].shape)
    torch.cuda.synchronize()
    _check_stats("alg f32 functional", st, out, Pd, net, raw_hm=raw)


# ---- 3. with a view mask -----------------------------------------------------------------------------------------------------------------------------------------
def test_flag_with_a_view_mask_equals_the_model_on_the_compacted_views(golden_dir):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    mask = np.array([[1, 0, 1, 1], [0, 1, 0, 1]], dtype=np.uint8)
    net = _net("alg", cfgs, sds, torch.float32, True)
    plain = net(images, Pd, _batch(inp, mask, nb=NB))
    net.keypoint_stats = True
    out = net(images, Pd, _batch(inp, mask, nb=NB))
    st = net.last_keypoint_stats
    torch.cuda.synchronize()
    _same(out, plain, "alg masked")
    assert len(net._plans) == 2
    _check_stats("alg masked", st, out, Pd, net, mask=mask)
    for b in range(NB):          # each sample alone on its valid views: the same joints and statistics
        keep = np.flatnonzero(mask[b])
        alone = _net("alg", cfgs, sds, torch.float32, True)
        alone.keypoint_stats = True
        sub = {"cameras": [[c[b]] for v, c in enumerate(_batch(inp, nb=NB)["cameras"]) if mask[b, v]], "pred_keypoints_3d": inp["pred_keypoints_3d"][b:b + 1]}
        o = alone(images[b:b + 1, keep].contiguous(), Pd[b:b + 1, keep].contiguous(), sub)
        s1 = alone.last_keypoint_stats
        torch.cuda.synchronize()
        assert torch.equal(o[0][0], out[0][b]), "sample %d: joints" % b
        assert torch.equal(s1.covariance[0], st.covariance[b]), "sample %d: covariance" % b
        for name in ("peak", "peak_index", "mass", "covariance_2d", "reprojection_error"):
            assert torch.equal(getattr(s1, name)[0], getattr(st, name)[b, keep]), "sample %d: %s" % (b, name)


# ---- 4. training --------------------------------------------------------------------------------------------------------------------------------------------------
def test_train_forward_leaves_no_statistics(golden_dir):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    net = _net("alg", cfgs, sds, torch.float32, True).to(DEV)
    net.keypoint_stats = True
    net(images[:1], Pd[:1], _batch(inp, nb=1))
    assert net.last_keypoint_stats is not None and net.last_keypoint_stats.peak.shape == (1, NV, J)
    net.train()
    out = net(images[:1], Pd[:1], _batch(inp, nb=1))
    torch.cuda.synchronize()
    assert len(out) == 4 and out[0].requires_grad and net.last_keypoint_stats is None
    net.eval()
    net(images[:1], Pd[:1], _batch(inp, nb=1))
    assert net.last_keypoint_stats is not None


# ---- 5. the cascade -------------------------------------------------------------------------------------------------------------------------------------------------
def test_cascade_leaves_the_algebraic_stages_statistics(golden_dir):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    casc = _net("cascade", cfgs, sds, torch.float32, True)
    plain = casc(images, Pd, _batch(inp, nb=NB))
    assert casc.last_alg_keypoint_stats is None and casc.last_keypoint_stats is None
    casc.vol.keypoint_stats = True
    casc(images, Pd, _batch(inp, nb=NB))
    vol_st = casc.last_keypoint_stats
    assert casc.last_alg_keypoint_stats is None and vol_st is not None
    casc.alg.keypoint_stats = True
    out = casc(images, Pd, _batch(inp, nb=NB))
    st = casc.last_alg_keypoint_stats
    torch.cuda.synchronize()
    _same(out, plain, "cascade")
    for n, x, y in zip(vol_st._fields, vol_st, casc.last_keypoint_stats):          # the volumetric stage's statistics: unchanged
        assert torch.equal(x, y), n
    alg = _net("alg", cfgs, sds, torch.float32, True)
    alg.keypoint_stats = True
    alone = alg(images, Pd, _batch(inp, nb=NB))
    torch.cuda.synchronize()
    _same(alone, out[1], "cascade's algebraic stage")
    _same_stats(st, alg.last_keypoint_stats, "cascade vs the algebraic model alone")
    casc.alg.keypoint_stats = False
    casc(images, Pd, _batch(inp, nb=NB))
    assert casc.last_alg_keypoint_stats is None and casc.last_keypoint_stats is not None


# ---- 6. the C ABI -------------------------------------------------------------------------------------------------------------------------------------------------
def _c_buffers():
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    return {"rec": nan(NB, NV, J, 5), "idx": torch.full((NB, NV, J), -7, dtype=torch.int32, device=DEV), "cov2d": nan(NB, NV, J, 3), "err": nan(NB, NV, J),
            "cov3d": nan(NB, J, 6)}


def _reset(bufs):
    for k, t in bufs.items():
        t.fill_(-7 if k == "idx" else float("nan"))


def _untouched(bufs):
    return all(bool((t == -7).all()) if k == "idx" else bool(torch.isnan(t).all()) for k, t in bufs.items())


def _set(plan, bufs):
    p = (lambda k: bufs[k].data_ptr()) if bufs else (lambda k: None)
    return H.lib().lt_plan_set_alg_keypoint_stats(plan, p("rec"), p("idx"), p("cov2d"), p("err"), p("cov3d"))


def _as_stats(bufs):
    from mvn.utils import op
    return op.alg_keypoint_stats_from_records(bufs["rec"], bufs["idx"], bufs["cov2d"], bufs["err"], bufs["cov3d"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_c_abi_alg_plan_equals_the_python_host(golden_dir, dtype):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    lib = H.lib()
    net = _net("alg", cfgs, sds, dtype, True)
    net.keypoint_stats = True
    want = net(images, Pd, _batch(inp, nb=NB))
    want_st = net.last_keypoint_stats
    torch.cuda.synchronize()
    for first_forward_before in (False, True):          # the call may come before or after the plan's first forward
        cp = AlgCPlan(H.LT_MODEL_ALG, cfgs["alg"], sds["alg"], NB, NV, HW, dtype)
        try:
            if first_forward_before:
                o = cp.forward(images, Pd)
                assert torch.equal(o["kp3d"], want[0]) and torch.equal(o["hm"], want[2])
            bufs = _c_buffers()
            for missing in bufs:          # a mixture of NULL and non-NULL pointers
                p = lambda k: None if k == missing else bufs[k].data_ptr()
                assert lib.lt_plan_set_alg_keypoint_stats(cp.plan, p("rec"), p("idx"), p("cov2d"), p("err"), p("cov3d")) == -1
                assert "come together" in lib.lt_last_error().decode()
            H.check(_set(cp.plan, bufs), "lt_plan_set_alg_keypoint_stats")
            for rnd in range(2):          # the setting persists
                _reset(bufs)
                o = cp.forward(images, Pd)
                for name, ours, ref in (("kp3d", o["kp3d"], want[0]), ("kp2d", o["kp2d"], want[1]), ("hm", o["hm"], want[2]), ("conf", o["conf"], want[3])):
                    assert torch.equal(ours, ref), (dtype, first_forward_before, rnd, name)
                _same_stats(_as_stats(bufs), want_st, "C ABI alg %s first_forward_before=%s forward %d" % (dtype, first_forward_before, rnd))
            H.check(_set(cp.plan, None), "lt_plan_set_alg_keypoint_stats")          # all NULL: the plain tail again
            _reset(bufs)
            o = cp.forward(images, Pd)
            assert torch.equal(o["kp3d"], want[0]) and torch.equal(o["hm"], want[2]) and _untouched(bufs)
            # the volumetric statistics' entry point still refuses this plan
            assert lib.lt_plan_set_keypoint_stats(cp.plan, bufs["rec"].data_ptr(), bufs["idx"].data_ptr()) == -2
        finally:
            cp.close()


def test_c_abi_alg_plan_with_a_mask_equals_the_python_host(golden_dir):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    mask = np.ascontiguousarray(np.array([[1, 0, 1, 1], [0, 1, 0, 1]], dtype=np.uint8))
    on = torch.from_numpy(mask.astype(bool)).to(DEV)
    net = _net("alg", cfgs, sds, torch.float32, True)
    net.keypoint_stats = True
    want = net(images, Pd, _batch(inp, mask, nb=NB))
    want_st = net.last_keypoint_stats
    torch.cuda.synchronize()
    cp = AlgCPlan(H.LT_MODEL_ALG, cfgs["alg"], sds["alg"], NB, NV, HW, torch.float32)
    try:
        import ctypes as C
        H.check(H.lib().lt_plan_set_view_mask(cp.plan, mask.ctypes.data_as(C.c_void_p)), "lt_plan_set_view_mask")
        bufs = _c_buffers()
        H.check(_set(cp.plan, bufs), "lt_plan_set_alg_keypoint_stats")
        o = cp.forward(images, Pd)
        assert torch.equal(o["kp3d"], want[0]) and torch.equal(o["conf"], want[3])
        _same_stats(_as_stats(bufs), want_st, "C ABI alg masked", on=on)
        assert bool(torch.isnan(bufs["err"][~on]).all())
    finally:
        cp.close()


def test_c_abi_cascade_plan_equals_the_python_host(golden_dir):
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    lib = H.lib()
    net = _net("cascade", cfgs, sds, torch.float32, True)
    net.alg.keypoint_stats = True
    (kp, feats, vols, _, _, coords, base), (a3, _, _, _) = net(images, Pd, _batch(inp, nb=NB))
    want_st = net.last_alg_keypoint_stats
    torch.cuda.synchronize()
    cp = CascadeCPlan(cfgs["alg"], sds["alg"], cfgs["vol_softmax"], sds["vol_softmax"], NB, NV, HW, torch.float32)
    try:
        bufs = _c_buffers()
        o = cp.forward(images, inp["K"], inp["R"], inp["t"])          # a plain forward first
        assert torch.equal(o["kp"], kp) and _untouched(bufs)
        assert lib.lt_plan_set_alg_keypoint_stats(cp.plan, bufs["rec"].data_ptr(), None, None, None, None) == -1
        H.check(_set(cp.plan, bufs), "lt_plan_set_alg_keypoint_stats")
        for rnd in range(2):
            _reset(bufs)
            o = cp.forward(images, inp["K"], inp["R"], inp["t"])
            for name, ours, ref in (("keypoints_3d", o["kp"], kp), ("alg_keypoints_3d", o["alg_kp3"], a3), ("base_points", o["base"], base), ("volumes", o["vols"], vols)):
                assert torch.equal(ours, ref), "forward %d %s" % (rnd, name)
            _same_stats(_as_stats(bufs), want_st, "C ABI cascade forward %d" % rnd)
        H.check(_set(cp.plan, None), "lt_plan_set_alg_keypoint_stats")
        _reset(bufs)
        o = cp.forward(images, inp["K"], inp["R"], inp["t"])
        assert torch.equal(o["kp"], kp) and torch.equal(o["vols"], vols) and _untouched(bufs)
    finally:
        cp.close()


def test_c_abi_refusals(golden_dir):
    from test_gpu_view_mask_models import VolCPlan
    cfgs, sds, inp, images, Pd = _inputs(golden_dir)
    lib = H.lib()
    bufs = _c_buffers()
    rp = AlgCPlan(H.LT_MODEL_RANSAC, cfgs["alg"], sds["alg"], NB, NV, HW, torch.float32)
    try:
        assert _set(rp.plan, bufs) == -2 and "RANSAC" in lib.lt_last_error().decode()
        assert _set(rp.plan, None) == -2
    finally:
        rp.close()
    vp = VolCPlan(cfgs["vol_softmax"], sds["vol_softmax"], torch.float32)
    try:
        assert _set(vp.plan, bufs) == -2 and "volumetric" in lib.lt_last_error().decode()
    finally:
        vp.close()
    assert _set(None, bufs) == -1 and "null plan" in lib.lt_last_error().decode()
    ap = AlgCPlan(H.LT_MODEL_ALG, cfgs["alg"], sds["alg"], NB, NV, HW, torch.float32)
    try:          # the existing entry point keeps refusing algebraic plans
        assert lib.lt_plan_set_keypoint_stats(ap.plan, bufs["rec"].data_ptr(), bufs["idx"].data_ptr()) == -2 and "volumetric" in lib.lt_last_error().decode()
    finally:
        ap.close()
