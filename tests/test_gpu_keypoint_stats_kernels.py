"""GPU (-m gpu): lt_softargmax3d_stats_fwd, the soft-argmax whose probabilities pass also reduces per-joint statistics of the 3D heatmap (peak, peak voxel,
mass, covariance about the returned joint), at the shapes, pointers and arguments where it changes its code path.  Pattern, inputs and case list: those of
tests/test_gpu_geometry_kernels.py (its _coords / _sa3_logits / SA3_CASES), plus the edges the new kernels add.
Kernels: csrc/softargmax.hip sa3_probs_stats_kernel<CL> (generic planar and channels-last: a wave owns joints wave, wave + 4, ..., its lanes walk the 256
voxels of an iteration 64 at a time, 2048-voxel chunks), sa3_probs_stats_planar_kernel (vectorised planar: the lane-to-voxel map and 4096-voxel chunks of
sa3_partial_planar_kernel), sa3_stats_finalize_kernel (one wave per (b, j) over the chunk records, a second trip of its loop beyond 64 chunks).
Truth: mvn.utils.volumetric.keypoint_stats, numpy fp64 on the fp32 product x = mult * logit, about the centre the call RETURNED (fp32 joints; ReLU: joints /
mass in fp32), as include/lt_hip.h defines it.
Gates and where they come from:
  covariance   every element within 1e-5 of the trace of that joint's truth.  The project's probability gate (1e-5, tests/test_gpu_geometry_kernels.py): the
               weights are the probabilities; the centred evaluation in plain fp32 torch on the CPU stays <= 1.8e-6 of the trace on these inputs up to 32768
               voxels.
  peak, mass   1e-5 relative, per element (the same gate; the CPU yardstick is 3.8e-6 on the peak, a 3x margin for another summation order and expf).
  peak_index   exact: the maximum of every (b, j) is given a margin of 0.5 in x over the runner-up (the ties test instead makes two maxima bit-equal).
  kp, probs    bitwise those of lt_softargmax3d_fwd for the same arguments; softmax: peak bitwise probs[peak_index]; a second call: equal bits;
               probs == NULL: the same stats, peak_index and kp bits whenever the NULL does not move the call to another kernel.
Every case asserts the branch it enters through _ss_plan(), which restates the launch arithmetic of sa3_forward()."""
import numpy as np
import pytest
import torch

from gpu_util import record
from test_gpu_geometry_kernels import DEV, INVALID, NAN, SA3_CASES, UNSUPPORTED, _cdiv, _coords, _f32, _gen, _lib, _off1, _sa3_fwd, _sa3_logits, _sa3_plan, _st

pytestmark = pytest.mark.gpu
TOL = 1e-5
MARGIN = 0.5


# ---- the launch arithmetic, restated (sa3_forward with statistics) ---------------------------------------------------------------------------------------------------
def _ss_plan(J, nvox, channels_last, logits_ptr, coords_ptr, probs_ptr):
    """The path and grid of the statistics pass: the vectorised kernel exactly when lt_softargmax3d_fwd takes its vectorised kernels (so kp and probs are its
    bits), one workgroup per (chunk, b) in every path; generic / channels-last: joints per wave = ceil(J / 4) <= 8 accumulator slots."""
    p = _sa3_plan(J, nvox, channels_last, logits_ptr, coords_ptr, probs_ptr)
    kernel = "channels_last" if channels_last else ("vectorised" if p["vec"] else "generic_planar")
    chunk = 4096 if p["vec"] else 2048
    return dict(kernel=kernel, vec=p["vec"], nchunks=_cdiv(nvox, chunk), chunk=chunk, slots=_cdiv(J, 4), finalize_trips=_cdiv(_cdiv(nvox, chunk), 64))


def _ss_fwd(lg_dev, cd_dev, mult, softmax, channels_last, B, J, nvox, probs_dev, ld=None, stats=True, index=True):
    """One lt_softargmax3d_stats_fwd call; returns (rc, joints, records, peak voxels)."""
    H, lib = _lib()
    kp = torch.full((B, J, 3), NAN, device=DEV)
    rec = torch.full((B, J, 8), NAN, device=DEV)
    idx = torch.full((B, J), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(1, lib.lt_softargmax3d_stats_workspace(B, J, nvox)), dtype=torch.uint8, device=DEV)
    rc = lib.lt_softargmax3d_stats_fwd(lg_dev.data_ptr(), cd_dev.data_ptr(), mult, softmax, channels_last, J if ld is None else ld, kp.data_ptr(), H.ptr(probs_dev),
                                       rec.data_ptr() if stats else None, idx.data_ptr() if index else None, B, J, nvox, ws.data_ptr(), _st())
    return rc, kp, rec, idx


def _with_margin(lg, mult_min=0.37):
    """The same logits with the maximum of every (b, j) raised until it leads the runner-up by MARGIN in x = mult * logit for every mult >= mult_min."""
    lg = lg.clone()
    top = lg.argmax(dim=2, keepdim=True)
    lg.scatter_(2, top, lg.gather(2, top) + (MARGIN + 0.01) / mult_min)
    return lg.contiguous()


def _cov33(rec):
    return rec[..., [2, 3, 4, 3, 5, 6, 4, 6, 7]].reshape(rec.shape[:-1] + (3, 3))


def _verify(tag, lg, cd, mult, softmax, cl, expect=None, misalign=None, exact_index=True):
    """One (logits, coordinates, mult, mode, layout): the branch, the call, every gate of the module docstring.  Returns (records, peak voxels) on the CPU."""
    from mvn.utils import volumetric
    H, lib = _lib()
    B, J, nvox = lg.shape
    src = lg.permute(0, 2, 1).contiguous() if cl else lg
    lgd = _off1(src) if misalign == "logits" else src.to(DEV)
    cdd = _off1(cd) if misalign == "coords" else cd.to(DEV)
    probs = torch.full((B, J, nvox), NAN, device=DEV)
    if misalign == "probs":
        probs = _off1(probs)
    plan = _ss_plan(J, nvox, cl, lgd.data_ptr(), cdd.data_ptr(), probs.data_ptr())
    for k, v in (expect or {}).items():
        assert plan[k] == v, (tag, k, plan)
    rc, kp, rec, idx = _ss_fwd(lgd, cdd, mult, softmax, cl, B, J, nvox, probs)
    H.check(rc, "lt_softargmax3d_stats_fwd")
    # kp and probs: the bits of lt_softargmax3d_fwd
    probs0 = _off1(torch.full((B, J, nvox), NAN, device=DEV)) if misalign == "probs" else torch.full((B, J, nvox), NAN, device=DEV)
    rc0, kp0 = _sa3_fwd(lgd, cdd, mult, softmax, cl, B, J, nvox, probs0)
    H.check(rc0, "lt_softargmax3d_fwd")
    assert torch.equal(kp, kp0), tag + ": joints differ from lt_softargmax3d_fwd's"
    assert torch.equal(probs, probs0), tag + ": probabilities differ from lt_softargmax3d_fwd's"
    # a second call: equal bits
    rc2, kp2, rec2, idx2 = _ss_fwd(lgd, cdd, mult, softmax, cl, B, J, nvox, probs)
    H.check(rc2, "lt_softargmax3d_stats_fwd (second call)")
    assert torch.equal(rec2.view(torch.int32), rec.view(torch.int32)) and torch.equal(idx2, idx) and torch.equal(kp2, kp), tag + ": a second call gives other bits"
    # probs == NULL: the same pass without the stores
    if _ss_plan(J, nvox, cl, lgd.data_ptr(), cdd.data_ptr(), None)["vec"] == plan["vec"]:
        rcn, kpn, recn, idxn = _ss_fwd(lgd, cdd, mult, softmax, cl, B, J, nvox, None)
        H.check(rcn, "lt_softargmax3d_stats_fwd (probs NULL)")
        assert torch.equal(recn.view(torch.int32), rec.view(torch.int32)) and torch.equal(idxn, idx) and torch.equal(kpn, kp), tag + ": probs == NULL gives other bits"
    rec_c, idx_c, kp_c, probs_c = rec.cpu(), idx.cpu(), kp.cpu(), probs.cpu()
    assert bool(torch.isfinite(rec_c).all()), tag
    # truth: fp64 on the fp32 product, about the returned centre
    x = (lg * _f32(mult)).numpy()
    t = volumetric.keypoint_stats(x, cd.numpy(), kp_c.numpy(), softmax=bool(softmax), mass=None if softmax else rec_c[..., 1].numpy())
    if exact_index:
        top2 = torch.from_numpy(x).topk(min(2, nvox), dim=2).values
        if nvox > 1:
            assert float((top2[..., 0] - top2[..., 1]).min()) >= MARGIN, tag + ": the inputs give the maximum no margin"
        assert np.array_equal(idx_c.numpy().astype(np.int64), t.peak_index), (tag, idx_c, t.peak_index)
    got_peak, got_mass, got_cov = rec_c[..., 0].double().numpy(), rec_c[..., 1].double().numpy(), _cov33(rec_c).double().numpy()
    assert np.array_equal(got_cov, np.swapaxes(got_cov, 2, 3))
    tr = np.trace(t.covariance, axis1=2, axis2=3)
    e_cov = float((np.abs(got_cov - t.covariance).max(axis=(2, 3)) / np.where(tr > 0, tr, 1.0)).max())
    rel = lambda a, r: float((np.abs(a - r) / np.where(r != 0, np.abs(r), 1.0)).max())
    e_peak, e_mass = rel(got_peak, t.peak), rel(got_mass, t.mass)
    record(tag, {"cov_err_over_trace": e_cov, "peak_rel_err": e_peak, "mass_rel_err": e_mass, "tol": TOL})
    print("%s: cov %.3e of the trace, peak %.3e, mass %.3e" % (tag, e_cov, e_peak, e_mass))
    assert e_cov <= TOL, "%s: covariance off by %.3e of the trace > %.1e" % (tag, e_cov, TOL)
    assert e_peak <= TOL, "%s: peak off by %.3e > %.1e" % (tag, e_peak, TOL)
    assert e_mass <= TOL, "%s: mass off by %.3e > %.1e" % (tag, e_mass, TOL)
    if softmax:
        assert bool((rec_c[..., 1] == 1.0).all())
        at_peak = probs_c.gather(2, idx_c.long()[..., None])[..., 0]
        assert torch.equal(rec_c[..., 0].view(torch.int32), at_peak.view(torch.int32)), tag + ": peak is not probs[peak_index] bit for bit"
        assert torch.equal(at_peak, probs_c.max(dim=2).values)
    return rec_c, idx_c


def _case(cid, B, J, nvox, layout, softmax, expect, misalign=None, logits="randn"):
    cl = int(layout == "channels_last")
    for mult in (1.0, 0.37):
        tag = "kstats/sa3 %s softmax=%d mult=%g" % (cid, softmax, mult)
        g = _gen(tag)
        lg, cd = _with_margin(_sa3_logits(logits, B, J, nvox, softmax, g)), _coords(B, nvox, g)
        _verify(tag, lg, cd, mult, softmax, cl, expect, misalign)


# ---- the cases: SA3_CASES of tests/test_gpu_geometry_kernels.py, by the kernel of the statistics pass they enter, and the new kernels' own edges ----------------------
CASES = {}


def _ss_expect(kw):
    cl = kw["layout"] == "channels_last"
    vec = kw["expect"].get("vec", False)
    e = dict(kernel="channels_last" if cl else ("vectorised" if vec else "generic_planar"), vec=vec)
    if "nchunks" in kw["expect"]:
        e["nchunks"] = kw["expect"]["nchunks"]
    return e


for _cid, _kw in SA3_CASES.items():
    _take = ("nvox343_ragged" in _cid or "nvox125" in _cid or "nvox2197_two_chunks" in _cid or "misaligned" in _cid or "vectorised_J" in _cid or "finalize_second_trip" in _cid
             or "ramp" in _cid or ("channels_last_JP" in _cid and _kw["J"] in (1, 9, 17, 25, 32)))
    if _take:
        CASES[_cid] = dict(_kw, expect=_ss_expect(_kw))
# the joints-per-wave edges of sa3_probs_stats_kernel: one joint per wave (4), a second slot for wave 0 only (5), all eight slots (29: wave 0 only; 32: every wave)
for _J, _slots in ((3, 1), (4, 1), (5, 2), (29, 8), (32, 8)):
    CASES["generic_planar_J%d_%d_slots_nvox343" % (_J, _slots)] = dict(B=2, J=_J, nvox=343, layout="planar", expect=dict(kernel="generic_planar", slots=_slots))
    CASES["channels_last_J%d_%d_slots_nvox343" % (_J, _slots)] = dict(B=2, J=_J, nvox=343, layout="channels_last", expect=dict(kernel="channels_last", slots=_slots))
# the chunk edges: 2048 voxels (generic planar: an odd count or one that is no multiple of 4; channels-last: any), 4096 voxels (vectorised: multiples of 4)
for _n, _c in ((2047, 1), (2049, 2)):
    CASES["generic_planar_J5_nvox%d_%d_chunks" % (_n, _c)] = dict(B=2, J=5, nvox=_n, layout="planar", expect=dict(kernel="generic_planar", nchunks=_c))
for _n, _c in ((2047, 1), (2048, 1), (2049, 2)):
    CASES["channels_last_J5_nvox%d_%d_chunks" % (_n, _c)] = dict(B=2, J=5, nvox=_n, layout="channels_last", expect=dict(kernel="channels_last", nchunks=_c))
CASES["vectorised_J5_nvox4092_last_lane_of_the_chunk_idle"] = dict(B=2, J=5, nvox=4092, layout="planar", expect=dict(kernel="vectorised", nchunks=1))
# one voxel
CASES["generic_planar_J5_nvox1"] = dict(B=2, J=5, nvox=1, layout="planar", expect=dict(kernel="generic_planar", nchunks=1))
CASES["channels_last_J5_nvox1"] = dict(B=2, J=5, nvox=1, layout="channels_last", expect=dict(kernel="channels_last", nchunks=1))


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
@pytest.mark.parametrize("cid", list(CASES))
def test_softargmax3d_stats_fwd(cid, softmax):
    kw = CASES[cid]
    if "finalize_second_trip" in cid:
        assert _cdiv(kw["nvox"], 4096 if "vectorised" in cid else 2048) > 64
        kw = dict(kw, expect=dict(kw["expect"], finalize_trips=2))
    _case(cid, softmax=softmax, **kw)


def test_case_list_covers_what_the_issue_names():
    ids = list(CASES)
    has = lambda *parts: any(all(p in i for p in parts) for i in ids)
    for n in (343, 125, 2197):
        assert has("generic_planar", "nvox%d" % n)
    for w in ("logits", "coords", "probs"):
        assert has("nvox512_misaligned_" + w)
    for J in (1, 9, 17, 25, 32):
        assert has("channels_last_JP", "_J%d_nvox343" % J)
    for n in (4, 1028, 4096, 4100):
        assert has("vectorised_J", "nvox%d_" % n)
    assert has("finalize_second_trip_generic_planar_nvox132651") and has("finalize_second_trip_channels_last_nvox132651") and has("finalize_second_trip_vectorised_nvox270336")
    assert has("ramp_up") and has("ramp_down") and has("nvox1")


PATHS = [("generic_planar", 343, 0), ("channels_last", 343, 1), ("vectorised", 4100, 0)]


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
@pytest.mark.parametrize("path,nvox,cl", PATHS)
def test_far_cuboid(path, nvox, cl, softmax):
    """The cuboid at (1e5, -2e5, 5e4) mm: E[c c^T] - mu mu^T in fp32 is off by 0.17 to 0.27 of the trace here; the moments about the joint keep the gate."""
    B, J = 2, 5
    tag = "kstats/sa3 far_cuboid %s softmax=%d" % (path, softmax)
    g = _gen(tag)
    lg = _with_margin(_sa3_logits("randn", B, J, nvox, softmax, g))
    cd = (torch.tensor([1e5, -2e5, 5e4]) + (torch.rand(B, nvox, 3, generator=g) - 0.5) * 2500.0).contiguous()
    _verify(tag, lg, cd, 0.37, softmax, cl, dict(kernel=path))


@pytest.mark.parametrize("path,nvox,cl", PATHS)
def test_one_hot_volume(path, nvox, cl):
    """One logit 60 above the rest: peak is 1 to the last bit or so, the covariance is what the e^-60 tails leave."""
    B, J = 2, 5
    tag = "kstats/sa3 one_hot %s" % path
    g = _gen(tag)
    lg = torch.randn(B, J, nvox, generator=g) * 0.5
    hot = torch.randint(0, nvox, (B, J, 1), generator=g)
    lg.scatter_(2, hot, float(lg.max()) + 60.0)
    rec, idx = _verify(tag, lg.contiguous(), _coords(B, nvox, g), 1.0, 1, cl, dict(kernel=path))
    assert torch.equal(idx.long(), hot[..., 0]) and bool((rec[..., 0] > 0.999999).all())


@pytest.mark.parametrize("path,nvox,cl", PATHS)
def test_relu_without_mass(path, nvox, cl):
    """ReLU mode, every logit <= 0: mass 0, peak 0, covariance 0 (and no NaN from the 0 / 0 of the centre); the peak voxel is still that of x."""
    B, J = 2, 5
    tag = "kstats/sa3 relu_no_mass %s" % path
    g = _gen(tag)
    lg = -(torch.rand(B, J, nvox, generator=g) + MARGIN + 0.1)              # all negative ...
    top = torch.randint(0, nvox, (B, J, 1), generator=g)
    lg.scatter_(2, top, 0.0)                                                 # ... but the maximum: exactly 0, more than the margin above the rest
    rec, idx = _verify(tag, lg.contiguous(), _coords(B, nvox, g), 1.0, 0, cl, dict(kernel=path))
    assert not rec.any() and torch.equal(idx.long(), top[..., 0])


# two bit-equal maxima: where the second one sits relative to the first, by path
TIES = [
    # generic planar / channels-last: a joint's voxels go to ONE wave; lane = voxel % 64, four runs of 64 per 256-voxel iteration, 2048-voxel chunks
    ("generic_planar", 4101, 0, "same_lane_next_run", 70, 70 + 64), ("generic_planar", 4101, 0, "same_lane_next_iteration", 70, 70 + 256),
    ("generic_planar", 4101, 0, "neighbouring_lanes", 70, 71), ("generic_planar", 4101, 0, "higher_lane_first", 71, 64 + 70),
    ("generic_planar", 4101, 0, "different_chunks", 70, 2048 + 3), ("generic_planar", 4101, 0, "last_chunk_one_live_lane", 2050, 4100),
    ("channels_last", 4101, 1, "same_lane_next_run", 70, 70 + 64), ("channels_last", 4101, 1, "same_lane_next_iteration", 70, 70 + 256),
    ("channels_last", 4101, 1, "neighbouring_lanes", 70, 71), ("channels_last", 4101, 1, "higher_lane_first", 71, 64 + 70),
    ("channels_last", 4101, 1, "different_chunks", 70, 2048 + 3), ("channels_last", 4101, 1, "last_chunk_one_live_lane", 2050, 4100),
    # vectorised: thread t owns voxels 4t .. 4t + 3 of each 1024-voxel group, four groups per 4096-voxel chunk, waves of 64 threads
    ("vectorised", 8200, 0, "same_lane_same_group", 8, 9), ("vectorised", 8200, 0, "same_lane_next_group", 8, 8 + 1024),
    ("vectorised", 8200, 0, "different_lanes_of_a_wave", 9, 40), ("vectorised", 8200, 0, "higher_lane_lower_group", 4 * 63 + 1, 1024 + 2),
    ("vectorised", 8200, 0, "different_waves", 9, 4 * 64 + 1), ("vectorised", 8200, 0, "higher_wave_lower_group", 4 * 200, 1024 + 4),
    ("vectorised", 8200, 0, "different_chunks", 9, 4096 + 2), ("vectorised", 8200, 0, "last_chunk_one_live_lane", 4097, 8196),
]


@pytest.mark.parametrize("path,nvox,cl,where,i1,i2", TIES, ids=["%s-%s" % (t[0], t[3]) for t in TIES])
def test_ties_go_to_the_lower_index(path, nvox, cl, where, i1, i2):
    B, J = 2, 6
    assert i1 < i2 < nvox
    if where == "different_chunks" or "last_chunk" in where:
        chunk = 4096 if path == "vectorised" else 2048
        assert i1 // chunk != i2 // chunk or "last_chunk" in where
    for softmax in (1, 0):
        tag = "kstats/sa3 ties %s %s softmax=%d" % (path, where, softmax)
        g = _gen(tag)
        lg = _sa3_logits("randn", B, J, nvox, softmax, g)
        top = lg.max() + 3.0
        lg[:, :, i1] = top
        lg[:, :, i2] = top
        rec, idx = _verify(tag, lg.contiguous(), _coords(B, nvox, g), 0.37, softmax, cl, dict(kernel=path), exact_index=False)
        assert bool((idx == i1).all()), (tag, idx)


@pytest.mark.parametrize("path,nvox,cl", PATHS)
def test_probs_null_same_bits(path, nvox, cl):
    """probs == NULL: the same kernels without the stores; stats, peak_index and kp keep their bits (17 joints, both modes)."""
    H, lib = _lib()
    B, J = 2, 17
    g = _gen("kstats probs_null " + path)
    lg, cd = _sa3_logits("randn", B, J, nvox, 1, g), _coords(B, nvox, g)
    lgd, cdd = (lg.permute(0, 2, 1).contiguous() if cl else lg).to(DEV), cd.to(DEV)
    probs = torch.empty(B, J, nvox, device=DEV)
    for p in (probs, None):
        assert _ss_plan(J, nvox, cl, lgd.data_ptr(), cdd.data_ptr(), H.ptr(p))["kernel"] == path
    for softmax in (1, 0):
        rc1, kp1, rec1, idx1 = _ss_fwd(lgd, cdd, 0.37, softmax, cl, B, J, nvox, probs)
        rc0, kp0, rec0, idx0 = _ss_fwd(lgd, cdd, 0.37, softmax, cl, B, J, nvox, None)
        H.check(rc1); H.check(rc0)
        assert bool(torch.isfinite(rec1).all()) and torch.equal(rec0.view(torch.int32), rec1.view(torch.int32)) and torch.equal(idx0, idx1) and torch.equal(kp0, kp1)


def test_refusals():
    """NULL stats / peak_index: LT_ERR_INVALID; 33 joints and padded channels-last rows: LT_ERR_UNSUPPORTED (ld < J: LT_ERR_INVALID); nothing is written."""
    H, lib = _lib()
    lg, cd = torch.zeros(2, 343, 40, device=DEV), torch.zeros(2, 343, 3, device=DEV)
    untouched = lambda kp, rec, idx: bool(torch.isnan(kp).all()) and bool(torch.isnan(rec).all()) and bool((idx == -7).all())
    rc, kp, rec, idx = _ss_fwd(lg, cd, 1.0, 1, 0, 2, 5, 343, None, stats=False)
    assert rc == INVALID and b"stats" in lib.lt_last_error() and untouched(kp, rec, idx)
    rc, kp, rec, idx = _ss_fwd(lg, cd, 1.0, 1, 0, 2, 5, 343, None, index=False)
    assert rc == INVALID and b"peak_index" in lib.lt_last_error() and untouched(kp, rec, idx)
    rc, kp, rec, idx = _ss_fwd(lg, cd, 1.0, 1, 1, 2, 5, 343, None, ld=8)
    assert rc == UNSUPPORTED and b"ld == J" in lib.lt_last_error() and untouched(kp, rec, idx)
    rc, kp, rec, idx = _ss_fwd(lg, cd, 1.0, 1, 1, 2, 5, 343, None, ld=4)
    assert rc == INVALID and untouched(kp, rec, idx)
    for cl in (0, 1):
        rc, kp, rec, idx = _ss_fwd(lg, cd, 1.0, 1, cl, 2, 33, 343, None)
        assert rc == UNSUPPORTED and b"J=33" in lib.lt_last_error() and untouched(kp, rec, idx)


def test_functional_op_returns_the_same_joints_and_volumes():
    """op.integrate_tensor_3d_with_stats: coordinates and volumes bit for bit those of integrate_tensor_3d_with_coordinates, with and without autograd (the
    gradients too); the statistics carry no gradient and match the numpy statement."""
    from mvn.utils import op, volumetric
    B, J, V = 2, 5, 7
    g = _gen("kstats functional op")
    vol = _with_margin((torch.randn(B, J, V ** 3, generator=g) * 3.0)).reshape(B, J, V, V, V).to(DEV)
    cv = _coords(B, V ** 3, g).reshape(B, V, V, V, 3).to(DEV)
    for softmax in (True, False):
        kp0, pr0 = op.integrate_tensor_3d_with_coordinates(vol, cv, softmax)
        kp1, pr1, st = op.integrate_tensor_3d_with_stats(vol, cv, softmax)
        assert torch.equal(kp0, kp1) and torch.equal(pr0, pr1) and isinstance(st, op.KeypointStats)
        assert st.peak.shape == (B, J) and st.mass.shape == (B, J) and st.covariance.shape == (B, J, 3, 3) and st.peak_index.dtype == torch.int32
        assert torch.equal(st.covariance, st.covariance.transpose(2, 3)) and not any(t.requires_grad for t in st)
        t = volumetric.keypoint_stats(vol.cpu().numpy(), cv.cpu().numpy(), kp1.cpu().numpy(), softmax=softmax, mass=st.mass.cpu().numpy())
        assert np.array_equal(st.peak_index.cpu().numpy(), t.peak_index)
        tr = np.trace(t.covariance, axis1=2, axis2=3)
        assert float((np.abs(st.covariance.cpu().double().numpy() - t.covariance).max(axis=(2, 3)) / tr).max()) <= TOL
        # through autograd: the same node, the same gradient
        grads = []
        for fn in (op.integrate_tensor_3d_with_coordinates, op.integrate_tensor_3d_with_stats):
            v = vol.clone().requires_grad_(True)
            out = fn(v, cv, softmax)
            assert torch.equal(out[0], kp0) and torch.equal(out[1], pr0)
            (out[0].sum() + (out[1] * out[1]).sum()).backward()
            grads.append(v.grad)
            if len(out) == 3:
                assert not any(t_.requires_grad for t_ in out[2]) and torch.equal(out[2].covariance, st.covariance) and torch.equal(out[2].peak, st.peak)
        assert torch.equal(grads[0], grads[1])
