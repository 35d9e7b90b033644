"""GPU (-m gpu): lt_softargmax2d_stats_fwd (csrc/softargmax.hip sa2_stats_kernel: one workgroup of 256 lanes per heatmap, the statistics out of the third
pass), lt_alg_tail_stats_fwd (alg_tail_stats_kernel<MASKED>: one lane per (sample, joint), dlt_stats_finish in dlt_solve's place) and the functional form
lt_triangulate_dlt_stats (dlt_stats_kernel), at the shapes where they can go wrong.
Truth: the numpy fp64 statement (mvn.utils.multiview.heatmap_stats_2d / triangulation_stats) fed with the kernel's own fp32 inputs and returned centres.
Gates (those of tests/test_gpu_keypoint_stats_kernels.py):
  covariances  every element within 1e-5 of the covariance's trace; the 2D ones with an absolute floor of 1e-6 px^2 for maps whose trace is (nearly) 0:
               coordinates stay below 128 px, whose fp32 ulp is 7.6e-6, so the floor is far above ulp^2 times the mass.
  peak, mass, reproj_err   1e-5 relative.
  peak_index   exact.
  coords, probs, keypoints_2d, confidences, keypoints_3d: the bits of lt_softargmax2d_fwd / lt_alg_tail_fwd / lt_alg_tail_masked_fwd; peak is bitwise
  probs[peak_index] in softmax mode; probs == NULL and a second call: equal bits."""
import numpy as np
import pytest
import torch

from gpu_util import check, record
from oracle import synth
from oracle import vol_oracle as O
from test_gpu_geometry_kernels import DEV, NAN, _gen, _lib, _st

pytestmark = pytest.mark.gpu
TOL = 1e-5
FLOOR_2D = 1e-6


# ---- lt_softargmax2d_stats_fwd ------------------------------------------------------------------------------------------------------------------------------------
def _sa2_stats(hm_dev, mult, softmax, with_probs=True):
    H, lib = _lib()
    NJ, h, w = hm_dev.shape
    c = torch.full((NJ, 2), NAN, device=DEV)
    p = torch.full((NJ, h, w), NAN, device=DEV) if with_probs else None
    rec = torch.full((NJ, 5), NAN, device=DEV)
    idx = torch.full((NJ,), -7, dtype=torch.int32, device=DEV)
    H.check(lib.lt_softargmax2d_stats_fwd(hm_dev.data_ptr(), mult, softmax, c.data_ptr(), H.ptr(p), rec.data_ptr(), idx.data_ptr(), NJ, h, w, _st()),
            "lt_softargmax2d_stats_fwd")
    return c, p, rec, idx


def _sa2_plain(hm_dev, mult, softmax):
    H, lib = _lib()
    NJ, h, w = hm_dev.shape
    c = torch.full((NJ, 2), NAN, device=DEV)
    p = torch.full((NJ, h, w), NAN, device=DEV)
    H.check(lib.lt_softargmax2d_fwd(hm_dev.data_ptr(), mult, softmax, c.data_ptr(), p.data_ptr(), NJ, h, w, _st()), "lt_softargmax2d_fwd")
    return c, p


def _bits(t):
    return t.view(torch.int32)


def _verify_sa2(tag, hm, mult, softmax):
    """One (heatmaps, mult, mode): the bits of the plain kernel, the repeat, probs == NULL, every gate of the module docstring.  Returns the CPU results."""
    from mvn.utils import multiview
    hd = hm.to(DEV)
    c, p, rec, idx = _sa2_stats(hd, mult, softmax)
    c0, p0 = _sa2_plain(hd, mult, softmax)
    assert torch.equal(_bits(c), _bits(c0)), tag + ": coords differ from lt_softargmax2d_fwd's"          # bitwise, NaN coordinates (ReLU without mass) included
    assert torch.equal(_bits(p), _bits(p0)), tag + ": probs differ from lt_softargmax2d_fwd's"
    c2, p2, rec2, idx2 = _sa2_stats(hd, mult, softmax)
    assert torch.equal(_bits(rec2), _bits(rec)) and torch.equal(idx2, idx) and torch.equal(_bits(c2), _bits(c)), tag + ": a second call gives other bits"
    cn, _, recn, idxn = _sa2_stats(hd, mult, softmax, with_probs=False)
    assert torch.equal(_bits(recn), _bits(rec)) and torch.equal(idxn, idx) and torch.equal(_bits(cn), _bits(c)), tag + ": probs == NULL gives other bits"
    rec_c, idx_c, c_c, p_c = rec.cpu(), idx.cpu(), c.cpu(), p.cpu()
    assert bool(torch.isfinite(rec_c).all()), tag
    peak, tidx, mass, cov = multiview.heatmap_stats_2d(hm.numpy(), mult, bool(softmax), coords=c_c.numpy())
    assert np.array_equal(idx_c.numpy().astype(np.int64), tidx), (tag, idx_c, tidx)
    NJ = hm.shape[0]
    at_peak = p_c.reshape(NJ, -1).gather(1, idx_c.long()[:, None])[:, 0]
    if softmax:
        assert torch.equal(rec_c[:, 0], at_peak), tag + ": peak is not probs[peak_index]"
        assert bool((rec_c[:, 1] == 1.0).all())
    got = rec_c.double().numpy()
    rel = lambda a, r: float((np.abs(a - r) / np.where(r != 0, np.abs(r), 1.0)).max())
    e_peak, e_mass = rel(got[:, 0], peak), rel(got[:, 1], mass)
    tr = cov[:, 0, 0] + cov[:, 1, 1]
    d = np.abs(np.stack([got[:, 2] - cov[:, 0, 0], got[:, 3] - cov[:, 0, 1], got[:, 4] - cov[:, 1, 1]], 1)).max(axis=1)
    e_cov = float((d / np.maximum(TOL * tr, FLOOR_2D)).max())          # in units of the gate
    record("alg_kstats/sa2 " + tag, {"peak_rel": e_peak, "mass_rel": e_mass, "cov_err_over_gate": e_cov, "cov_err_over_trace": float((d / np.where(tr > 0, tr, 1.0)).max())})
    print("alg_kstats/sa2 %s: peak %.3e mass %.3e cov %.3e of its gate (max |d| %.3e px^2, trace %.3e .. %.3e)" % (tag, e_peak, e_mass, e_cov, d.max(), tr.min(), tr.max()))
    assert e_peak <= TOL and e_mass <= TOL, (tag, e_peak, e_mass)
    assert e_cov <= 1.0, "%s: a covariance element off by %.3e of max(1e-5 trace, 1e-6 px^2)" % (tag, e_cov)
    return rec_c, idx_c, c_c, p_c


def _heatmaps(NJ, h, w, g, relu):
    """Noise plus one bump per map at a random place; ReLU inputs are mostly negative, like a network's."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    cx, cy = torch.rand(NJ, 1, 1, generator=g) * (w - 1), torch.rand(NJ, 1, 1, generator=g) * (h - 1)
    s = 0.6 + 0.15 * min(h, w) * torch.rand(NJ, 1, 1, generator=g)
    bump = torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    hm = 0.05 * torch.randn(NJ, h, w, generator=g) + (0.2 * bump - 0.05 if relu else 0.08 * bump)
    return hm.contiguous()


SA2_SHAPES = {"NJ3_3x5_15_values_most_lanes_idle": (3, 3, 5), "NJ2_16x16_exactly_256_values": (2, 16, 16), "NJ5_24x40_960_values_not_a_multiple_of_256": (5, 24, 40),
              "NJ34_96x96_the_production_map": (34, 96, 96)}


@pytest.mark.parametrize("mult", [1.0, 100.0], ids=["mult1", "mult100"])
@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
@pytest.mark.parametrize("sid", list(SA2_SHAPES))
def test_softargmax2d_stats(sid, softmax, mult):
    NJ, h, w = SA2_SHAPES[sid]
    hm = _heatmaps(NJ, h, w, _gen("sa2 stats %s %d" % (sid, softmax)), relu=not softmax)
    rec, idx, c, p = _verify_sa2("%s %s mult %g" % (sid, "softmax" if softmax else "relu", mult), hm, mult, softmax)
    if not softmax:
        assert bool((rec[:, 1] > 0).all())          # these maps do have mass


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
def test_softargmax2d_stats_one_hot_map(softmax):
    """All of the weight on one pixel: peak 1, covariance exactly 0 (the centre is that pixel, every other weight is 0)."""
    h, w = 24, 40
    hm = torch.zeros(3, h, w)
    spots = [(0, 0), (13, 27), (h - 1, w - 1)]
    for n, (y, x) in enumerate(spots):
        hm[n, y, x] = 200.0          # softmax: exp(-200) is 0 in fp32
    rec, idx, c, p = _verify_sa2("one-hot %s" % ("softmax" if softmax else "relu"), hm, 1.0, softmax)
    assert idx.tolist() == [y * w + x for y, x in spots]
    assert rec[:, 0].tolist() == [1.0] * 3 and not rec[:, 2:].any()
    assert rec[:, 1].tolist() == ([1.0] * 3 if softmax else [200.0] * 3)
    assert c.tolist() == [[float(x), float(y)] for y, x in spots]


def test_softargmax2d_stats_relu_without_mass():
    """Every value <= 0: mass 0, peak 0, covariance 0, NaN coordinates as lt_softargmax2d_fwd's; the peak pixel is still that of x.  A map with mass next to it
    is not disturbed."""
    g = _gen("sa2 relu no mass")
    hm = -torch.rand(3, 16, 16, generator=g) - 0.01
    hm[1] = _heatmaps(1, 16, 16, g, relu=True)[0]
    hm[2, 5, 7] = 0.0          # the largest x of map 2, and still no mass
    H, lib = _lib()
    c, p, rec, idx = _sa2_stats(hm.to(DEV), 2.0, 0)
    c0, p0 = _sa2_plain(hm.to(DEV), 2.0, 0)
    rec, idx, c = rec.cpu(), idx.cpu(), c.cpu()
    assert torch.equal(_bits(c), _bits(c0.cpu())) and torch.equal(p.cpu(), p0.cpu())
    assert bool(torch.isnan(c[0]).all()) and bool(torch.isnan(c[2]).all()) and bool(torch.isfinite(c[1]).all())
    for n in (0, 2):
        assert rec[n].tolist() == [0.0] * 5, rec[n]
    assert idx[0] == hm[0].flatten().argmax() and idx[2] == 5 * 16 + 7
    assert rec[1, 1] > 0 and rec[1, 0] > 0 and rec[1, 2] > 0 and bool(torch.isfinite(rec).all())


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
def test_softargmax2d_stats_ties_go_to_the_lower_index(softmax):
    """Bit-equal maxima at two places: within one lane's stride (i and i + 256: the same lane), across the lanes of a wave, across waves, and across waves with
    the LOWER index in the HIGHER lane.  96 x 96 = 9216 values: lane = i % 256, wave = lane / 64."""
    h = w = 96
    pairs = [(300, 300 + 256), (300 + 512, 300), (5, 40), (1000, 1000 + 17), (10, 200), (70 + 256, 130), (255, 256), (9215, 3)]
    hm = 0.01 * torch.randn(len(pairs), h, w, generator=_gen("sa2 ties %d" % softmax))
    for n, (a, b) in enumerate(pairs):
        hm[n].view(-1)[a] = hm[n].view(-1)[b] = 0.75
    rec, idx, c, p = _verify_sa2("ties %s" % ("softmax" if softmax else "relu"), hm, 3.0, softmax)
    assert idx.tolist() == [min(a, b) for a, b in pairs]
    for n, (a, b) in enumerate(pairs):
        assert p[n].view(-1)[a] == p[n].view(-1)[b]


# ---- lt_alg_tail_stats_fwd ------------------------------------------------------------------------------------------------------------------------------------------
def _tail_inputs(B, NV, J, ld, g):
    """Ring cameras at 256 px, joints within 300 mm of the origin, 2 px of noise, 4 image px per heatmap px; raw confidences in (0.2, 1.2) in rows of ld floats;
    2D records with random positive-definite covariances of a few heatmap px^2."""
    K, R, t = synth.ring_cameras(NV, 256)
    P = torch.from_numpy(K @ np.concatenate([R, t], -1))[None].repeat(B, 1, 1, 1).float().contiguous()
    X = torch.randn(B, J, 3, generator=g).double()
    X = X / X.norm(dim=-1, keepdim=True) * 300.0 * torch.rand(B, J, 1, generator=g).double()
    hh = torch.einsum("bvik,bjk->bvji", P.double(), torch.cat([X, torch.ones(B, J, 1, dtype=torch.float64)], -1))
    kp_hm = ((hh[..., :2] / hh[..., 2:3] + torch.randn(B, NV, J, 2, generator=g).double() * 2.0) / 4.0).float().contiguous()
    conf_raw = (torch.rand(B, NV, ld, generator=g) + 0.2).contiguous()
    L = torch.randn(B, NV, J, 2, 2, generator=g)
    S = L @ L.transpose(-1, -2) + 0.3 * torch.eye(2)
    rec = torch.stack([torch.rand(B, NV, J, generator=g), torch.ones(B, NV, J), S[..., 0, 0], S[..., 0, 1], S[..., 1, 1]], -1).contiguous()
    return P, kp_hm, conf_raw, rec


SX, SY = 4.0, 3.5          # two different scales: the xy element of S Sigma S is theirs


def _tail_stats(P, kp_hm, conf_raw, ld, rec, mask, B, NV, J):
    H, lib = _lib()
    o = {"kp2d": torch.full((B, NV, J, 2), NAN, device=DEV), "conf": torch.full((B, NV, J), NAN, device=DEV), "kp3d": torch.full((B, J, 3), NAN, device=DEV),
         "cov2d": torch.full((B, NV, J, 3), NAN, device=DEV), "err": torch.full((B, NV, J), -7.0, device=DEV), "cov3d": torch.full((B, J, 6), NAN, device=DEV)}
    H.check(lib.lt_alg_tail_stats_fwd(kp_hm.data_ptr(), H.ptr(conf_raw), ld, P.data_ptr(), SX, SY, H.ptr(mask), rec.data_ptr(), o["kp2d"].data_ptr(),
                                      o["conf"].data_ptr(), o["kp3d"].data_ptr(), o["cov2d"].data_ptr(), o["err"].data_ptr(), o["cov3d"].data_ptr(), B, NV, J, _st()),
            "lt_alg_tail_stats_fwd")
    return o


def _tail_plain(P, kp_hm, conf_raw, ld, mask, B, NV, J):
    H, lib = _lib()
    kp2d, conf, kp3d = torch.full((B, NV, J, 2), NAN, device=DEV), torch.full((B, NV, J), NAN, device=DEV), torch.full((B, J, 3), NAN, device=DEV)
    if mask is None:
        H.check(lib.lt_alg_tail_fwd(kp_hm.data_ptr(), H.ptr(conf_raw), ld, P.data_ptr(), SX, SY, kp2d.data_ptr(), conf.data_ptr(), kp3d.data_ptr(), B, NV, J, _st()),
                "lt_alg_tail_fwd")
    else:
        H.check(lib.lt_alg_tail_masked_fwd(kp_hm.data_ptr(), H.ptr(conf_raw), ld, P.data_ptr(), SX, SY, mask.data_ptr(), kp2d.data_ptr(), conf.data_ptr(),
                                           kp3d.data_ptr(), B, NV, J, _st()), "lt_alg_tail_masked_fwd")
    return kp2d, conf, kp3d


def _cov33(c6):
    return c6[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(c6.shape[:-1] + (3, 3))


def _masks(B, NV):
    """None, all ones, and one (NV < 4: that leaves two) or two views masked, another pattern per sample."""
    some = np.ones((B, NV), dtype=np.uint8)
    for b in range(B):
        some[b, (b + 1) % NV] = 0
        if NV >= 4 and b % 2 == 0:
            some[b, (b + 3) % NV] = 0
    return {"no_mask": None, "all_ones": np.ones((B, NV), dtype=np.uint8), "some_masked": some}


def _verify_tail(tag, P, kp_hm, conf_raw, ld, rec, mask_np, B, NV, J):
    from mvn.utils import multiview
    H, lib = _lib()
    dev = lambda t: None if t is None else t.to(DEV)
    Pd, kd, cd, rd = dev(P), dev(kp_hm), dev(conf_raw), dev(rec)
    md = None if mask_np is None else torch.from_numpy(mask_np).to(DEV)
    o = _tail_stats(Pd, kd, cd, ld, rd, md, B, NV, J)
    kp2d0, conf0, kp3d0 = _tail_plain(Pd, kd, cd, ld, md, B, NV, J)
    assert torch.equal(o["kp2d"], kp2d0) and torch.equal(o["conf"], conf0) and torch.equal(o["kp3d"], kp3d0), tag + ": the three existing outputs differ from the plain tail's"
    o2 = _tail_stats(Pd, kd, cd, ld, rd, md, B, NV, J)
    on = np.ones((B, NV), dtype=bool) if mask_np is None else mask_np.astype(bool)
    ont = torch.from_numpy(on)
    for k in o:
        a, b = o[k].cpu(), o2[k].cpu()
        if k in ("cov2d", "err", "kp2d"):          # a masked view's entries are unspecified or NaN
            a, b = a[ont], b[ont]
        assert torch.equal(a, b), "%s: a second call gives other %s" % (tag, k)
    c = {k: v.cpu() for k, v in o.items()}
    assert bool(torch.isfinite(c["kp3d"]).all()) and bool(torch.isfinite(c["cov3d"]).all()) and bool(torch.isfinite(c["err"][ont]).all())
    assert bool(torch.isnan(c["err"][~ont]).all()), tag + ": a masked view's reproj_err is not NaN"
    # cov2d_img = S Sigma_hm S in fp64, rounded once: the nearest fp32, nothing less
    r64 = rec.double().numpy()
    s = np.array([float(np.float32(SX)), float(np.float32(SY))])
    want2 = np.stack([s[0] * s[0] * r64[..., 2], s[0] * s[1] * r64[..., 3], s[1] * s[1] * r64[..., 4]], -1)
    assert np.array_equal(c["cov2d"].numpy()[on], want2.astype(np.float32)[on]), tag + ": cov2d_img is not the rounded fp64 product"
    # the truth on the kernel's own outputs
    err, cov = multiview.triangulation_stats(P.numpy(), c["kp2d"].numpy(), c["conf"].numpy(), c["cov2d"].numpy(), c["kp3d"].numpy(), None if mask_np is None else mask_np)
    e_err = float((np.abs(c["err"].double().numpy() - err)[on] / err[on]).max())
    tr = np.trace(cov, axis1=2, axis2=3)
    got3 = _cov33(c["cov3d"]).double().numpy()
    e_cov = float((np.abs(got3 - cov).max(axis=(2, 3)) / tr).max())
    record("alg_kstats/tail " + tag, {"reproj_rel": e_err, "cov3d_err_over_trace": e_cov, "tol": TOL})
    print("alg_kstats/tail %s: reproj %.3e, cov3d %.3e of the trace" % (tag, e_err, e_cov))
    assert e_err <= TOL and e_cov <= TOL, (tag, e_err, e_cov)
    # reproj_err from the returned outputs alone, written out
    X = c["kp3d"].double().numpy()
    hh = np.einsum("bvik,bjk->bvji", P.double().numpy(), np.concatenate([X, np.ones((B, J, 1))], -1))
    mine = np.sqrt(((hh[..., :2] / hh[..., 2:3] - c["kp2d"].double().numpy()) ** 2).sum(-1))
    assert float((np.abs(c["err"].double().numpy() - mine)[on] / mine[on]).max()) <= TOL
    # the functional form on the returned tensors: the same joints and statistics, bit for bit
    out = torch.full((B, J, 3), NAN, device=DEV); e2 = torch.full((B, NV, J), -7.0, device=DEV); c3 = torch.full((B, J, 6), NAN, device=DEV)
    H.check(lib.lt_triangulate_dlt_stats(Pd.data_ptr(), o["kp2d"].data_ptr(), o["conf"].data_ptr(), o["cov2d"].data_ptr(), H.ptr(md), out.data_ptr(), e2.data_ptr(),
                                         c3.data_ptr(), B, NV, J, _st()), "lt_triangulate_dlt_stats")
    assert torch.equal(out, o["kp3d"]) and torch.equal(c3, o["cov3d"]) and torch.equal(e2.cpu()[ont], c["err"][ont]) and bool(torch.isnan(e2.cpu()[~ont]).all()), tag
    return c


TAIL_SHAPES = {"B1_NV2_J1_minimum": (1, 2, 1), "B2_NV4_J17": (2, 4, 17), "B3_NV8_J5": (3, 8, 5), "B1_NV10_J2": (1, 10, 2), "B5_NV4_J17_85_lanes_two_workgroups": (5, 4, 17)}


@pytest.mark.parametrize("conf", ["conf_ld_J", "conf_ld_J_plus_3", "conf_null"])
@pytest.mark.parametrize("sid", list(TAIL_SHAPES))
def test_alg_tail_stats(sid, conf):
    B, NV, J = TAIL_SHAPES[sid]
    if "two_workgroups" in sid:
        assert -(-B * J // 64) == 2
    ld = J + 3 if conf == "conf_ld_J_plus_3" else J
    P, kp_hm, conf_raw, rec = _tail_inputs(B, NV, J, ld, _gen("alg tail stats %s %s" % (sid, conf)))
    if conf == "conf_null":
        conf_raw = None
    for mname, mask in _masks(B, NV).items():
        if mname == "some_masked" and NV == 2:          # two views: masking one leaves no DLT -- NaN joints and NaN cov3d, as the masked plain tail
            dev = lambda t: None if t is None else t.to(DEV)
            Pd, kd, cd, rd, md = dev(P), dev(kp_hm), dev(conf_raw), dev(rec), torch.from_numpy(mask).to(DEV)
            o = _tail_stats(Pd, kd, cd, ld, rd, md, B, NV, J)
            kp2d0, conf0, kp3d0 = _tail_plain(Pd, kd, cd, ld, md, B, NV, J)
            assert bool(torch.isnan(o["kp3d"]).all()) and bool(torch.isnan(kp3d0).all()) and bool(torch.isnan(o["cov3d"]).all()) and bool(torch.isnan(o["err"]).all())
            assert torch.equal(o["conf"], conf0) and torch.equal(o["kp2d"], kp2d0)
            continue
        c = _verify_tail("%s %s %s" % (sid, conf, mname), P, kp_hm, conf_raw, ld, rec, mask, B, NV, J)
        if mname == "some_masked":          # NaN in everything a masked view owns leaks nowhere
            m = torch.from_numpy(mask.astype(bool))
            Pn, kn, rn = P.clone(), kp_hm.clone(), rec.clone()
            Pn[~m] = NAN; kn[~m] = NAN; rn[~m] = NAN
            cn = None
            if conf_raw is not None:
                cn = conf_raw.clone(); cn[~m] = NAN
            o = _tail_stats(Pn.to(DEV), kn.to(DEV), None if cn is None else cn.to(DEV), ld, rn.to(DEV), torch.from_numpy(mask).to(DEV), B, NV, J)
            for k in ("kp3d", "cov3d", "conf"):
                assert torch.equal(o[k].cpu(), c[k]), "%s: NaN of a masked view reaches %s" % (sid, k)
            for k in ("kp2d", "cov2d", "err"):
                assert torch.equal(o[k].cpu()[m], c[k][m]), "%s: NaN of a masked view reaches %s of a valid view" % (sid, k)


def test_alg_tail_stats_one_valid_view_gives_nan():
    B, NV, J = 3, 4, 5
    P, kp_hm, conf_raw, rec = _tail_inputs(B, NV, J, J, _gen("alg tail one valid view"))
    mask = np.array([[1, 1, 0, 1], [0, 0, 1, 0], [1, 1, 1, 1]], dtype=np.uint8)
    o = _tail_stats(P.to(DEV), kp_hm.to(DEV), conf_raw.to(DEV), J, rec.to(DEV), torch.from_numpy(mask).to(DEV), B, NV, J)
    kp2d0, conf0, kp3d0 = _tail_plain(P.to(DEV), kp_hm.to(DEV), conf_raw.to(DEV), J, torch.from_numpy(mask).to(DEV), B, NV, J)
    c = {k: v.cpu() for k, v in o.items()}
    assert bool(torch.isnan(c["kp3d"][1]).all()) and bool(torch.isnan(c["cov3d"][1]).all()) and bool(torch.isnan(c["err"][1]).all())
    assert bool(torch.isnan(kp3d0.cpu()[1]).all()) and torch.equal(c["kp3d"][[0, 2]], kp3d0.cpu()[[0, 2]]) and torch.equal(c["conf"], conf0.cpu())
    for b in (0, 2):
        assert bool(torch.isfinite(c["kp3d"][b]).all()) and bool(torch.isfinite(c["cov3d"][b]).all())


def test_triangulate_dlt_bwd_still_agrees_with_fp64_autograd():
    """lt_triangulate_dlt_bwd now shares dlt_grad_w / dlt_grad_row with the statistics: the gate of tests/test_gpu_geometry_kernels.py:test_triangulate_dlt_bwd
    (1e-5 against the oracle's DLT under fp64 autograd on the same fp32-rounded inputs), on one case of more than one workgroup."""
    H, lib = _lib()
    B, NV, J = 5, 4, 17
    g = _gen("alg kstats dlt bwd")
    P, kp_hm, conf_raw, _ = _tail_inputs(B, NV, J, J, g)
    pts = (kp_hm * 4.0).contiguous()
    GX = torch.randn(B, J, 3, generator=g)
    p64, c64 = pts.double().requires_grad_(True), conf_raw.double().requires_grad_(True)
    (O.triangulate_batch_of_points(P.double(), p64, c64, dtype=torch.float64) * GX.double()).sum().backward()
    gp, gc = torch.full((B, NV, J, 2), NAN, device=DEV), torch.full((B, NV, J), NAN, device=DEV)
    Pd, pd, cd, GXd = P.to(DEV), pts.to(DEV), conf_raw.to(DEV), GX.to(DEV)
    H.check(lib.lt_triangulate_dlt_bwd(Pd.data_ptr(), pd.data_ptr(), cd.data_ptr(), GXd.data_ptr(), gp.data_ptr(), gc.data_ptr(), B, NV, J, _st()),
            "lt_triangulate_dlt_bwd")
    check("alg_kstats/dlt_bwd d/d points", gp.cpu(), p64.grad, 1e-5)
    check("alg_kstats/dlt_bwd d/d confidences", gc.cpu(), c64.grad, 1e-5)
    # the statistics' Jacobian is that backward's: J_v^T g_X
    from mvn.utils import multiview
    _, jac = multiview.triangulation_jacobian(P.numpy(), pts.numpy(), conf_raw.numpy())
    want = np.einsum("bvjer,bje->bvjr", jac, GX.double().numpy())
    check("alg_kstats/statement jacobian^T g vs lt_triangulate_dlt_bwd", gp.cpu(), torch.from_numpy(want), 1e-5)


# ---- the functional ops: the plain ops' results and gradients, statistics without a gradient ------------------------------------------------------------------
def test_functional_ops_keep_the_plain_ops_results_and_gradients():
    from mvn.utils import multiview, op
    g = _gen("alg kstats functional ops")
    hm = _heatmaps(6, 24, 40, g, relu=False).reshape(2, 3, 24, 40).to(DEV)
    a, b = hm.clone().requires_grad_(True), hm.clone().requires_grad_(True)
    c0, p0 = op.integrate_tensor_2d(a * 3.0, True)
    c1, p1, st = op.integrate_tensor_2d_with_stats(b * 3.0, True)
    assert torch.equal(c0, c1) and torch.equal(p0, p1) and c1.requires_grad and not any(t.requires_grad for t in st)
    G = torch.randn(2, 3, 2, generator=g).to(DEV)
    (c0 * G).sum().backward()
    (c1 * G).sum().backward()
    assert torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0)
    with torch.no_grad():
        c2, p2, st2 = op.integrate_tensor_2d_with_stats(hm * 3.0, True)
    assert torch.equal(c2, c1) and torch.equal(p2, p1) and all(torch.equal(x, y) for x, y in zip(st, st2))
    peak, pidx, mass, cov = st
    assert peak.shape == mass.shape == pidx.shape == (2, 3) and pidx.dtype == torch.int32 and cov.shape == (2, 3, 2, 2) and torch.equal(cov, cov.transpose(2, 3))
    assert torch.equal(peak, p1.reshape(2, 3, -1).max(dim=2).values)
    # the triangulation
    B, NV, J = 2, 4, 5
    P, kp_hm, conf_raw, rec = _tail_inputs(B, NV, J, J, g)
    Pd, pts, conf = P.to(DEV), (kp_hm * 4.0).to(DEV), conf_raw.to(DEV)
    cov2 = rec[..., [2, 3, 3, 4]].reshape(B, NV, J, 2, 2).to(DEV)
    pa, ca, pb, cb = pts.clone().requires_grad_(True), conf.clone().requires_grad_(True), pts.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    x0 = multiview.triangulate_batch_of_points(Pd, pa, ca)
    x1, err, c3 = multiview.triangulate_batch_of_points_with_stats(Pd, pb, cb, cov2)
    assert torch.equal(x0, x1) and x1.requires_grad and not err.requires_grad and not c3.requires_grad
    GX = torch.randn(B, J, 3, generator=g).to(DEV)
    (x0 * GX).sum().backward()
    (x1 * GX).sum().backward()
    assert torch.equal(pa.grad, pb.grad) and torch.equal(ca.grad, cb.grad)
    with torch.no_grad():
        x2, err2, c32 = multiview.triangulate_batch_of_points_with_stats(Pd, pts, conf, cov2)
        x3, err3, c33 = multiview.triangulate_batch_of_points_with_stats(Pd, pts, conf, rec[..., 2:].to(DEV))          # the packed {xx, xy, yy} form
    assert torch.equal(x2, x1) and torch.equal(err2, err) and torch.equal(c32, c3) and torch.equal(err3, err) and torch.equal(c33, c3)
    assert c3.shape == (B, J, 3, 3) and torch.equal(c3, c3.transpose(2, 3)) and err.shape == (B, NV, J)
    mask = np.array([[1, 1, 0, 1], [1, 1, 1, 1]], dtype=np.uint8)
    with pytest.raises(NotImplementedError, match="inference only"):
        multiview.triangulate_batch_of_points_with_stats(Pd, pts.clone().requires_grad_(True), conf, cov2, view_mask=mask)
    with pytest.raises(ValueError, match="covariances_2d"):
        multiview.triangulate_batch_of_points_with_stats(Pd, pts, conf)
    with torch.no_grad():
        xm, em, cm = multiview.triangulate_batch_of_points_with_stats(Pd, pts, conf, cov2, view_mask=mask)
        xw = multiview.triangulate_batch_of_points(Pd, pts, conf, view_mask=mask)
    assert torch.equal(xm, xw) and bool(torch.isnan(em[0, 2]).all()) and bool(torch.isfinite(em[0, [0, 1, 3]]).all()) and torch.equal(em[1], err[1]) and torch.equal(cm[1], c3[1])
