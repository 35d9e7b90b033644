"""GPU (-m gpu): the kernels that turn the network's output into joints and the loss back into a logits gradient, one C entry point at a time, at
the shapes, pointers and arguments where each of them changes its code path, against plain fp64 torch on the CPU written here (or the oracle package).
Kernels: csrc/softargmax.hip (sa3_partial_kernel<JP, CL>, sa3_partial_planar_kernel, sa3_finalize_kernel, sa3_probs_kernel<CL>, sa3_probs_planar_kernel,
sa2_kernel, sa2_bwd_kernel, dlt_bwd_kernel), csrc/backward.hip (sa3_bwd_kernel, sa3_pg_kernel, vol_ce_kernel), csrc/unproject.hip (coord_volumes_kernel).
Gates (all through gpu_util.check: max|d| <= tol * max|ref|) and where each comes from:
  lt_softargmax3d_fwd      coordinates 2e-5 softmax / 2e-4 ReLU, probabilities 1e-5 softmax / 1e-6 ReLU, |sum p - 1| < 1e-4: the numbers of
                           test_softargmax3d_large_sharp / test_softargmax3d_planar_ragged (tests/test_gpu_kernels.py), in check()'s form
  lt_softargmax3d_bwd*     1e-4, the file-wide gate of tests/test_gpu_backward.py; planar and channels-last outputs bitwise the same values
  lt_volumetric_ce_fwd     the index exact (torch.argmin: first minimum), terms / grad_val 1e-6 against fp64 (two fp32 roundings and a logf)
  lt_softargmax2d_fwd/_bwd coordinates 1e-5, heatmap gradient 1e-4 (test_softargmax2d_and_dlt_backward_vs_autograd_of_the_reference_ops), heatmaps 5e-6
  lt_triangulate_dlt_bwd   1e-5 against fp64 autograd over the SAME fp32-rounded inputs: the kernel is fp64 inside, so the two differ by the rounding of
                           its output (6e-8) and the eigen-gap division (about 1e-8 on these rings), with two orders of magnitude on top
  lt_coord_volumes         bit for bit against oracle.vol_oracle.coord_volume (test_coord_volumes_bit_exact_and_rotated)
Every case id names the branch it enters; _sa3_plan() and the *_grid() helpers restate the launch arithmetic of the entry points and each case ASSERTS
that the branch is really entered before it compares numbers.  The kernels assume finite logits (include/lt_hip.h); none of the inputs here has an
infinity or a NaN."""
import zlib

import numpy as np
import pytest
import torch

from gpu_util import check, record
from oracle import synth
from oracle import vol_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID, UNSUPPORTED = -1, -2
NAN = float("nan")


def _lib():
    import lt_hip as H
    return H, H.lib()


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _cdiv(a, b):
    return -(-a // b)


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ---- the launch arithmetic, restated (lt_softargmax3d_fwd / sa3_planar_vec / sa3_launch_partial, the grids of the other entry points) -----------
def _sa3_plan(J, nvox, channels_last, logits_ptr, coords_ptr, probs_ptr):
    vec = (not channels_last) and nvox % 4 == 0 and logits_ptr % 16 == 0 and coords_ptr % 16 == 0 and (probs_ptr is None or probs_ptr % 16 == 0)
    JP = 17 if J == 17 else (8 if J <= 8 else (16 if J <= 16 else (24 if J <= 24 else 32)))
    return dict(vec=vec, nchunks=_cdiv(nvox, 4096 if vec else 2048), JP=JP)


def _sa3_bwd_grid(nvox):
    return _cdiv(nvox, 2048), min(_cdiv(nvox, 2048), 4096)


def _sa2_bwd_grid(h, w):
    return _cdiv(h * w, 256), min(_cdiv(h * w, 256), 64)


def _coord_volumes_grid(B, V):
    return _cdiv(B * V ** 3, 256), min(_cdiv(B * V ** 3, 256), 8192)


# ---- inputs and fp64 references ---------------------------------------------------------------------------------------------------------------------
def _coords(B, nvox, g):
    """(B, nvox, 3) fp32 millimetres in a 2500 mm cuboid around a non-zero base point per sample (no grid needed: the kernels see nvox and coordinates)."""
    base = torch.tensor([[130.0 + 100.0 * b, -220.0, 310.0 - 50.0 * b] for b in range(B)])
    return (base[:, None, :] + (torch.rand(B, nvox, 3, generator=g) - 0.5) * 2500.0).contiguous()


def _sa3_ref(lg, cd, mult, softmax):
    """fp64 on the fp32 product mult * logit (the one rounding the kernels make): p = softmax / relu, joints = p @ coords (ReLU: not normalised)."""
    x = (lg * _f32(mult)).double()
    p = torch.softmax(x, dim=2) if softmax else torch.relu(x)
    return torch.einsum("bjn,bnc->bjc", p, cd.double()), p


def _off1(t):
    """The same values in a buffer of one float more, from its second element on: 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _sa3_fwd(lg_dev, cd_dev, mult, softmax, channels_last, B, J, nvox, probs_dev, ld=None):
    """One lt_softargmax3d_fwd call; returns (rc, joints)."""
    H, lib = _lib()
    kp = torch.full((B, J, 3), NAN, device=DEV)
    ws = torch.empty(max(1, lib.lt_softargmax3d_workspace(B, J, nvox)), dtype=torch.uint8, device=DEV)
    rc = lib.lt_softargmax3d_fwd(lg_dev.data_ptr(), cd_dev.data_ptr(), mult, softmax, channels_last, J if ld is None else ld, kp.data_ptr(), H.ptr(probs_dev),
                                 B, J, nvox, ws.data_ptr(), _st())
    return rc, kp


def _sa3_logits(kind, B, J, nvox, softmax, g):
    if kind == "randn":
        lg = torch.randn(B, J, nvox, generator=g) * 5.0
    else:          # the online softmax's worst case: every new voxel raises the running maximum (up) / most exponentials underflow at once (down)
        ramp = torch.linspace(-40.0, 40.0, nvox)
        lg = (ramp if kind == "ramp_up" else ramp.flip(0))[None, None, :] + torch.randn(B, J, nvox, generator=g) * 0.5
    return (lg if softmax else lg * 0.01).contiguous()


def _sa3_case(cid, B, J, nvox, layout, softmax, expect, misalign=None, logits="randn"):
    """Both multipliers through one case: inputs, the branch assertion, the call with probabilities against fp64, and the call with probs == NULL, whose
    joints must be bitwise those of the first call whenever it takes the same partial kernel (finalize is shared)."""
    H, lib = _lib()
    cl = int(layout == "channels_last")
    for mult in (1.0, 0.37):
        tag = "geo/sa3_fwd %s softmax=%d mult=%g" % (cid, softmax, mult)
        g = _gen(tag)
        lg, cd = _sa3_logits(logits, B, J, nvox, softmax, g), _coords(B, nvox, g)
        rk, rp = _sa3_ref(lg, cd, mult, softmax)
        src = lg.permute(0, 2, 1).contiguous() if cl else lg
        lgd = _off1(src) if misalign == "logits" else src.to(DEV)
        cdd = _off1(cd) if misalign == "coords" else cd.to(DEV)
        probs = torch.full((B, J, nvox), NAN, device=DEV)
        if misalign == "probs":
            probs = _off1(probs)
        plan = _sa3_plan(J, nvox, cl, lgd.data_ptr(), cdd.data_ptr(), probs.data_ptr())
        for k, v in expect.items():
            assert plan[k] == v, (cid, k, plan)
        rc, kp = _sa3_fwd(lgd, cdd, mult, softmax, cl, B, J, nvox, probs)
        H.check(rc, "lt_softargmax3d_fwd")
        check(tag + " coordinates", kp.cpu(), rk, 2e-5 if softmax else 2e-4)
        check(tag + " probabilities", probs.cpu(), rp, 1e-5 if softmax else 1e-6)
        if softmax:
            s = float((probs.cpu().double().sum(2) - 1.0).abs().max())
            record(tag + " |sum p - 1|", {"err": s, "tol": 1e-4})
            assert s < 1e-4, (tag, s)
        if _sa3_plan(J, nvox, cl, lgd.data_ptr(), cdd.data_ptr(), None)["vec"] == plan["vec"]:
            rc, kp0 = _sa3_fwd(lgd, cdd, mult, softmax, cl, B, J, nvox, None)
            H.check(rc, "lt_softargmax3d_fwd(probs NULL)")
            assert torch.equal(kp0, kp), tag + ": joints with probs == NULL differ from the call with probabilities"


GENERIC = dict(vec=False)
SA3_CASES = {}          # id -> kwargs of _sa3_case


def _add(cid, **kw):
    assert cid not in SA3_CASES
    SA3_CASES[cid] = kw


# the generic planar kernel, entered because nvox % 4 != 0
_add("generic_planar_B2_J5_nvox343_ragged_second_block", B=2, J=5, nvox=343, layout="planar", expect=dict(GENERIC, nchunks=1, JP=8))
_add("generic_planar_B2_J3_nvox125_waves_2_3_empty", B=2, J=3, nvox=125, layout="planar", expect=dict(GENERIC, nchunks=1, JP=8))
_add("generic_planar_B1_J17_nvox2197_two_chunks_ragged", B=1, J=17, nvox=2197, layout="planar", expect=dict(GENERIC, nchunks=2, JP=17))
# ... and because one pointer is 4 bytes past a 16-byte boundary, at a voxel count the vectorised kernels would take
for _which in ("logits", "coords", "probs"):
    _add("generic_planar_B2_J5_nvox512_misaligned_%s" % _which, B=2, J=5, nvox=512, layout="planar", misalign=_which, expect=dict(GENERIC, nchunks=1, JP=8))
# every JP instantiation in both layouts of sa3_partial_kernel
for _J, _JP in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 17), (18, 24), (24, 24), (25, 32), (32, 32)):
    _add("generic_planar_JP%d_J%d_nvox343" % (_JP, _J), B=2, J=_J, nvox=343, layout="planar", expect=dict(GENERIC, JP=_JP))
    _add("channels_last_JP%d_J%d_nvox343" % (_JP, _J), B=2, J=_J, nvox=343, layout="channels_last", expect=dict(GENERIC, JP=_JP))
# the vectorised kernels' edges
for _J in (1, 5, 32):
    _add("vectorised_J%d_nvox4_one_live_lane" % _J, B=2, J=_J, nvox=4, layout="planar", expect=dict(vec=True, nchunks=1))
    _add("vectorised_J%d_nvox1028_second_group_one_live_lane" % _J, B=2, J=_J, nvox=1028, layout="planar", expect=dict(vec=True, nchunks=1))
    _add("vectorised_J%d_nvox4096_exactly_one_chunk" % _J, B=2, J=_J, nvox=4096, layout="planar", expect=dict(vec=True, nchunks=1))
    _add("vectorised_J%d_nvox4100_second_chunk_one_live_lane" % _J, B=2, J=_J, nvox=4100, layout="planar", expect=dict(vec=True, nchunks=2))
# sa3_finalize_kernel's loop: a second trip at more than 64 chunks
_add("finalize_second_trip_generic_planar_nvox132651_65_chunks", B=1, J=2, nvox=132651, layout="planar", expect=dict(GENERIC, nchunks=65))
_add("finalize_second_trip_channels_last_nvox132651_65_chunks", B=1, J=2, nvox=132651, layout="channels_last", expect=dict(GENERIC, nchunks=65))
_add("finalize_second_trip_vectorised_nvox270336_66_chunks", B=1, J=2, nvox=270336, layout="planar", expect=dict(vec=True, nchunks=66))
# the online softmax's worst cases
for _kind in ("ramp_up", "ramp_down"):
    _add("generic_planar_J5_nvox2197_%s" % _kind, B=2, J=5, nvox=2197, layout="planar", logits=_kind, expect=dict(GENERIC, nchunks=2))
    _add("vectorised_J5_nvox4100_%s" % _kind, B=2, J=5, nvox=4100, layout="planar", logits=_kind, expect=dict(vec=True, nchunks=2))


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
@pytest.mark.parametrize("cid", list(SA3_CASES))
def test_softargmax3d_fwd(cid, softmax):
    """lt_softargmax3d_fwd with the kernel's own mult in {1.0, 0.37}, against fp64 on the fp32 product."""
    kw = SA3_CASES[cid]
    if "waves_2_3_empty" in cid:
        assert kw["nvox"] <= 128
    if "finalize_second_trip" in cid:
        assert _cdiv(kw["nvox"], 4096 if "vectorised" in cid else 2048) > 64
    if "one_live_lane" in cid:          # the group of four that starts at the last multiple of 1024 (4096) holds the volume's last four voxels
        assert kw["nvox"] % 1024 == 4
    _sa3_case(cid, softmax=softmax, **kw)


@pytest.mark.parametrize("path,nvox,cl", [("generic_planar", 343, 0), ("channels_last", 343, 1), ("vectorised", 4100, 0)])
def test_softargmax3d_fwd_probs_null_same_joints_bitwise(path, nvox, cl):
    """probs == NULL: the same partial and finalize kernels run, so the joints are bitwise those of the call that also writes the probabilities."""
    H, lib = _lib()
    B, J = 2, 17
    g = _gen("probs_null " + path)
    lg, cd = _sa3_logits("randn", B, J, nvox, 1, g), _coords(B, nvox, g)
    lgd, cdd = (lg.permute(0, 2, 1).contiguous() if cl else lg).to(DEV), cd.to(DEV)
    probs = torch.empty(B, J, nvox, device=DEV)
    for p in (probs, None):
        assert _sa3_plan(J, nvox, cl, lgd.data_ptr(), cdd.data_ptr(), H.ptr(p))["vec"] == (path == "vectorised")
    for softmax in (1, 0):
        rc1, kp1 = _sa3_fwd(lgd, cdd, 0.37, softmax, cl, B, J, nvox, probs)
        rc0, kp0 = _sa3_fwd(lgd, cdd, 0.37, softmax, cl, B, J, nvox, None)
        H.check(rc1); H.check(rc0)
        assert bool(torch.isfinite(kp1).all()) and torch.equal(kp0, kp1), (path, softmax)


def test_softargmax3d_fwd_refuses_padded_rows_and_33_joints():
    """Channels-last rows with ld > J and more than 32 joints are LT_ERR_UNSUPPORTED (ld < J: LT_ERR_INVALID); nothing is written."""
    H, lib = _lib()
    lg, cd = torch.zeros(2, 343, 40, device=DEV), torch.zeros(2, 343, 3, device=DEV)
    rc, kp = _sa3_fwd(lg, cd, 1.0, 1, 1, 2, 5, 343, None, ld=8)
    assert rc == UNSUPPORTED and b"ld == J" in lib.lt_last_error() and bool(torch.isnan(kp).all())
    rc, kp = _sa3_fwd(lg, cd, 1.0, 1, 1, 2, 5, 343, None, ld=4)
    assert rc == INVALID and bool(torch.isnan(kp).all())
    for cl in (0, 1):
        rc, kp = _sa3_fwd(lg, cd, 1.0, 1, cl, 2, 33, 343, None)
        assert rc == UNSUPPORTED and b"J=33" in lib.lt_last_error() and bool(torch.isnan(kp).all())


# ---- lt_softargmax3d_bwd / _bwd_dense ------------------------------------------------------------------------------------------------------------------
SA3_BWD_SHAPES = {"B2_J5_nvox343_one_workgroup_per_plane": (2, 5, 343), "B1_J17_nvox2197_two_workgroups_per_plane": (1, 17, 2197)}
SA3_BWD_VARIANTS = ["joints_only", "joints_sparse", "joints_dense", "joints_sparse_dense"]


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
@pytest.mark.parametrize("mult", [1.0, 0.37], ids=["mult1", "mult0.37"])
@pytest.mark.parametrize("variant", SA3_BWD_VARIANTS)
@pytest.mark.parametrize("sid", list(SA3_BWD_SHAPES))
def test_softargmax3d_bwd(sid, variant, mult, softmax):
    """probs and kp are the fp64 reference forward rounded to fp32, so the kernel differentiates exactly what the reference does: fp64 autograd of
    (kp . Gk).sum() + (p . Gp).sum(), Gp the sparse (one voxel per (b, j); voxel 0 and voxel nvox - 1 among them) plus the dense gradient.  The
    planar and the channels-last output must hold the same values bit for bit."""
    H, lib = _lib()
    B, J, nvox = SA3_BWD_SHAPES[sid]
    wanted, launched = _sa3_bwd_grid(nvox)
    assert wanted == launched == (1 if "one_workgroup" in sid else 2)
    sparse, dense = "sparse" in variant, "dense" in variant
    tag = "geo/sa3_bwd %s %s mult=%g softmax=%d" % (sid, variant, mult, softmax)
    g = _gen(tag)
    lg, cd = _sa3_logits("randn", B, J, nvox, softmax, g), _coords(B, nvox, g)
    Gk = torch.randn(B, J, 3, generator=g)
    Gd = torch.randn(B, J, nvox, generator=g) * 300.0          # of the size of Gk . X (millimetres), so that neither term hides under the other
    idx = torch.randint(0, nvox, (B, J), generator=g).to(torch.int32)
    idx.view(-1)[0], idx.view(-1)[-1] = 0, nvox - 1
    gv = torch.randn(B, J, generator=g) * 300.0
    x = (lg * _f32(mult)).double().requires_grad_(True)
    p = torch.softmax(x, dim=2) if softmax else torch.relu(x)
    kp = torch.einsum("bjn,bnc->bjc", p, cd.double())
    Gp = torch.zeros(B, J, nvox, dtype=torch.float64)
    if sparse:
        Gp.scatter_(2, idx.long()[..., None], gv.double()[..., None])
    if dense:
        Gp = Gp + Gd.double()
    ((kp * Gk.double()).sum() + (p * Gp).sum()).backward()
    ref = x.grad * float(_f32(mult))          # d / d logit = mult * d / d (mult * logit)
    pd, kd, cdd, Gkd = p.detach().float().to(DEV), kp.detach().float().to(DEV), cd.to(DEV), Gk.to(DEV)
    idxd, gvd = (idx.to(DEV), gv.to(DEV)) if sparse else (None, None)
    Gdd = Gd.to(DEV) if dense else None
    ws = torch.empty(B * J, device=DEV) if dense and softmax else None          # ReLU mode needs no sum_i p_i g_i
    outs = []
    for cl in (0, 1):
        gl = torch.full((B, nvox, J) if cl else (B, J, nvox), NAN, device=DEV)
        if dense:
            rc = lib.lt_softargmax3d_bwd_dense(pd.data_ptr(), cdd.data_ptr(), kd.data_ptr(), Gkd.data_ptr(), H.ptr(idxd), H.ptr(gvd), Gdd.data_ptr(), H.ptr(ws), mult,
                                               softmax, cl, gl.data_ptr(), B, J, nvox, _st())
        else:
            rc = lib.lt_softargmax3d_bwd(pd.data_ptr(), cdd.data_ptr(), kd.data_ptr(), Gkd.data_ptr(), H.ptr(idxd), H.ptr(gvd), mult, softmax, cl, gl.data_ptr(), B, J,
                                         nvox, _st())
        H.check(rc, "lt_softargmax3d_bwd")
        outs.append((gl.permute(0, 2, 1) if cl else gl).cpu().contiguous())
        check(tag + (" channels-last" if cl else " planar"), outs[-1], ref, 1e-4)
    assert torch.equal(outs[0], outs[1]), tag + ": the two layouts hold different values"


def test_softargmax3d_bwd_argument_checks():
    """A dense gradient in softmax mode without the B * J floats of workspace, and gp_idx without gp_val: LT_ERR_INVALID, nothing written."""
    H, lib = _lib()
    B, J, nvox = 2, 5, 343
    p, cd, kp, gk = torch.rand(B, J, nvox, device=DEV), torch.rand(B, nvox, 3, device=DEV), torch.rand(B, J, 3, device=DEV), torch.rand(B, J, 3, device=DEV)
    idx, gv = torch.zeros(B, J, dtype=torch.int32, device=DEV), torch.rand(B, J, device=DEV)
    gl = torch.full((B, J, nvox), NAN, device=DEV)
    assert lib.lt_softargmax3d_bwd_dense(p.data_ptr(), cd.data_ptr(), kp.data_ptr(), gk.data_ptr(), None, None, p.data_ptr(), None, 1.0, 1, 0, gl.data_ptr(), B, J, nvox,
                                         _st()) == INVALID
    assert b"workspace" in lib.lt_last_error()
    assert lib.lt_softargmax3d_bwd(p.data_ptr(), cd.data_ptr(), kp.data_ptr(), gk.data_ptr(), idx.data_ptr(), None, 1.0, 1, 0, gl.data_ptr(), B, J, nvox, _st()) == INVALID
    assert b"come together" in lib.lt_last_error()
    assert lib.lt_softargmax3d_bwd(p.data_ptr(), cd.data_ptr(), kp.data_ptr(), gk.data_ptr(), None, gv.data_ptr(), 1.0, 1, 0, gl.data_ptr(), B, J, nvox, _st()) == INVALID
    assert bool(torch.isnan(gl).all())


# ---- lt_volumetric_ce_fwd ---------------------------------------------------------------------------------------------------------------------------------
def _ce_call(cd, pr, gt, val):
    H, lib = _lib()
    B, J, nvox = pr.shape
    terms, gval = torch.full((B, J), NAN, device=DEV), torch.full((B, J), NAN, device=DEV)
    idx = torch.full((B, J), -1, dtype=torch.int32, device=DEV)
    cdd, prd, gtd, vd = cd.contiguous().to(DEV), pr.contiguous().to(DEV), gt.contiguous().to(DEV), val.contiguous().to(DEV)
    H.check(lib.lt_volumetric_ce_fwd(cdd.data_ptr(), prd.data_ptr(), gtd.data_ptr(), vd.data_ptr(), terms.data_ptr(), idx.data_ptr(), gval.data_ptr(), B, J, nvox,
                                     _st()), "lt_volumetric_ce_fwd")
    return terms.cpu(), idx.cpu(), gval.cpu()


def _ce_check(tag, terms, gval, pr, val, want):
    B, J, _ = pr.shape
    pv = pr.double().gather(2, want.long()[..., None])[..., 0] + 1e-6
    check(tag + " terms", terms, val.double() * -torch.log(pv), 1e-6)
    check(tag + " grad_val", gval, -val.double() / pv / (B * J), 1e-6)
    assert bool(torch.isfinite(terms).all()) and bool(torch.isfinite(gval).all())


def test_volumetric_ce_first_minimum_tie_rule_integer_grid():
    """The grid -60 + 8 (i, j, k), V = 16, i-major: every distance is exact in fp32, so ground truth half way between voxels gives exact ties.
    Both mechanisms of the first-minimum rule: ascending order inside a lane (voxels 256 apart) and the index tie-break of the LDS tree."""
    V = 16
    ax = -60.0 + 8.0 * torch.arange(V, dtype=torch.float32)
    cd1 = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    g = _gen("ce integer grid")
    table = [((-32.0, -20.0, -4.0), (855, 1111), 855), ((-36.0, -16.0, -4.0), (855, 871), 855), ((-36.0, -20.0, 0.0), (855, 856), 855),
             ((-500.0, 0.0, 0.0), (119, 120, 135, 136), 119), ((20.0, -12.0, 36.0), (10 * 256 + 6 * 16 + 12,), 10 * 256 + 6 * 16 + 12)]
    assert 855 % 256 == 1111 % 256 and 855 % 256 + 1 == 856 % 256          # the same lane; neighbouring lanes
    B, J = 2, 8
    gt = (torch.rand(B, J, 3, generator=g) - 0.5) * 120.0
    for b in range(B):
        for j, (pt, tied, first) in enumerate(table):
            gt[b, (j + 3 * b) % J] = torch.tensor(pt)
            d = torch.sqrt(((cd1 - torch.tensor(pt)) ** 2).sum(-1))
            assert sorted(torch.nonzero(d == d.min()).reshape(-1).tolist()) == list(tied) and int(torch.argmin(d)) == first
    cd = cd1[None].repeat(B, 1, 1).contiguous()
    want = torch.stack([torch.argmin(torch.sqrt(((cd[b][None] - gt[b][:, None]) ** 2).sum(-1)), dim=1) for b in range(B)]).to(torch.int32)
    pr = torch.rand(B, J, V ** 3, generator=g) * 0.998 + 0.001
    pr[0, 0, 855] = 0.0          # -log(0 + 1e-6) is finite
    assert int(want[0, 0]) == 855
    val = torch.tensor([[1.0, 0.0, 0.5, 1.0, 1.0, 0.5, 1.0, 0.0], [1.0, 0.5, 1.0, 0.0, 1.0, 1.0, 0.5, 1.0]])
    assert float(val[0, 0]) == 1.0          # the zero probability sits under a valid joint
    terms, idx, gval = _ce_call(cd, pr, gt, val)
    assert torch.equal(idx, want), (idx.tolist(), want.tolist())
    _ce_check("geo/vol_ce integer grid", terms, gval, pr, val, want)


def test_volumetric_ce_rotated_grid_matches_fp64_argmin():
    """A rotated, non-integer grid (B 2, J 17, V 12): the index is the fp64 argmin wherever the two nearest voxels are more than 1e-4 (relative) apart
    -- asserted for every (b, j) of this seed, so that no rounding of the fp32 distances can decide."""
    B, J, V = 2, 17, 12
    g = _gen("ce rotated grid")
    base = np.array([[130.0, -220.0, 310.0], [-75.5, 40.25, 990.0]])
    cd = torch.stack([O.coord_volume(base[b], 2500.0, V, 0.4 + 0.9 * b) for b in range(B)]).reshape(B, -1, 3)
    gt = torch.from_numpy(base).float()[:, None, :] + (torch.rand(B, J, 3, generator=g) - 0.5) * 2400.0
    d = torch.sqrt(((cd.double()[:, None] - gt.double()[:, :, None]) ** 2).sum(-1))          # (B, J, nvox)
    two = torch.topk(d, 2, dim=2, largest=False).values
    gap = float(((two[..., 1] - two[..., 0]) / two[..., 0]).min())
    record("geo/vol_ce rotated grid: smallest relative gap between the two nearest voxels", gap)
    assert gap > 1e-4
    want = d.argmin(2).to(torch.int32)
    pr = torch.rand(B, J, V ** 3, generator=g) * 0.998 + 0.001
    val = (torch.rand(B, J, generator=g) > 0.2).float()
    terms, idx, gval = _ce_call(cd, pr, gt, val)
    assert torch.equal(idx, want)
    _ce_check("geo/vol_ce rotated grid", terms, gval, pr, val, want)


# ---- lt_softargmax2d_fwd / _bwd ----------------------------------------------------------------------------------------------------------------------------
SA2_SHAPES = {"NJ12_9x11_fewer_pixels_than_lanes": (12, 9, 11), "NJ3_24x20_two_workgroups": (3, 24, 20), "NJ2_129x128_bwd_grid_stride_wraps": (2, 129, 128)}


@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "relu"])
@pytest.mark.parametrize("mult", [1.0, 100.0], ids=["mult1", "mult100"])
@pytest.mark.parametrize("sid", list(SA2_SHAPES))
def test_softargmax2d_fwd_bwd(sid, mult, softmax):
    """Reference: oracle integrate_tensor_2d in fp64 on the fp32 product, under autograd.  The backward gets what the forward returned, as the op does.
    Heatmaps are N(0, (2 / mult)^2): the softmax sees the std-2 values of test_softargmax2d_and_dlt_backward_vs_autograd_of_the_reference_ops whatever the
    multiplier (the reference's heatmap_multiplier = 100 is made for network outputs of that size).  Std-2 heatmaps times 100 would be one-hot to 1e-26;
    the gradient mult p_i ((x_i - X) g_x + ...) then cancels down to the rounding of the fp32 joint X that the backward is handed, in any implementation:
    the conditioning of the operation, not the kernel, would be measured."""
    H, lib = _lib()
    NJ, h, w = SA2_SHAPES[sid]
    wanted, launched = _sa2_bwd_grid(h, w)
    if "fewer_pixels" in sid:
        assert h * w < 256 and launched == 1
    elif "wraps" in sid:
        assert wanted == 65 and launched == 64
    else:
        assert wanted == launched == 2
    tag = "geo/sa2 %s mult=%g softmax=%d" % (sid, mult, softmax)
    g = _gen(tag)
    hm = torch.randn(NJ, h, w, generator=g) * (2.0 / mult)
    x =(hm * _f32(mult)).double().requires_grad_(True)
    assert bool((x.detach().reshape(NJ, -1).max(1).values > 0).all())          # ReLU: the reference's 0 / 0 is not under test
    rc, rp = O.integrate_tensor_2d(x[None], bool(softmax), dtype=torch.float64)
    G = torch.randn(NJ, 2, generator=g)
    (rc[0] * G.double()).sum().backward()
    ref_g = x.grad * float(_f32(mult))
    hd = hm.to(DEV)
    c, p = torch.full((NJ, 2), NAN, device=DEV), torch.full((NJ, h, w), NAN, device=DEV)
    H.check(lib.lt_softargmax2d_fwd(hd.data_ptr(), mult, softmax, c.data_ptr(), p.data_ptr(), NJ, h, w, _st()), "lt_softargmax2d_fwd")
    check(tag + " coordinates", c.cpu(), rc[0].detach(), 1e-5)
    check(tag + " heatmaps", p.cpu(), rp[0].detach(), 5e-6)
    c0 = torch.full((NJ, 2), NAN, device=DEV)
    H.check(lib.lt_softargmax2d_fwd(hd.data_ptr(), mult, softmax, c0.data_ptr(), None, NJ, h, w, _st()), "lt_softargmax2d_fwd(probs NULL)")
    assert torch.equal(c0, c), tag + ": coordinates with probs == NULL differ"
    gh = torch.full((NJ, h, w), NAN, device=DEV)
    Gd = G.to(DEV)
    H.check(lib.lt_softargmax2d_bwd(p.data_ptr(), c.data_ptr(), Gd.data_ptr(), mult, softmax, gh.data_ptr(), NJ, h, w, _st()), "lt_softargmax2d_bwd")
    check(tag + " d/d heatmaps", gh.cpu(), ref_g, 1e-4)


# ---- lt_triangulate_dlt_bwd ----------------------------------------------------------------------------------------------------------------------------------
DLT_CASES = {"B5_NV4_J17_full_and_partial_workgroup": (5, 4, 17, True), "B2_NV2_J7_minimum_views": (2, 2, 7, True), "B2_NV10_J7": (2, 10, 7, True),
             "B3_NV4_J17_conf_null_grad_conf_null": (3, 4, 17, False)}


@pytest.mark.parametrize("cid", list(DLT_CASES))
def test_triangulate_dlt_bwd(cid):
    """Ring cameras, points within 300 mm of the origin, 2-pixel noise, confidences in (0.2, 1.2).  The fp64 reference (the oracle's DLT under autograd)
    gets the fp32-ROUNDED matrices, points and confidences, so that it differs from the fp64-inside kernel by the kernel's output rounding only."""
    H, lib = _lib()
    B, NV, J, with_conf = DLT_CASES[cid]
    if "full_and_partial" in cid:
        assert _cdiv(B * J, 64) == 2 and (B * J) % 64 != 0
    g = _gen("dlt " + cid)
    K, R, t = synth.ring_cameras(NV, 256)
    P = torch.from_numpy(K @ np.concatenate([R, t], -1))[None].repeat(B, 1, 1, 1).float().contiguous()          # (B, NV, 3, 4), rounded to fp32
    X = torch.randn(B, J, 3, generator=g).double()
    X = X / X.norm(dim=-1, keepdim=True) * 300.0 * torch.rand(B, J, 1, generator=g).double()
    Xh = torch.cat([X, torch.ones(B, J, 1, dtype=torch.float64)], -1)
    proj = torch.einsum("bvik,bjk->bvji", P.double(), Xh)
    pts = (proj[..., :2] / proj[..., 2:3] + torch.randn(B, NV, J, 2, generator=g).double() * 2.0).float().contiguous()
    conf = (torch.rand(B, NV, J, generator=g) + 0.2).contiguous() if with_conf else None
    GX = torch.randn(B, J, 3, generator=g)
    p64 = pts.double().requires_grad_(True)
    c64 = conf.double().requires_grad_(True) if with_conf else None
    x64 = O.triangulate_batch_of_points(P.double(), p64, c64, dtype=torch.float64)
    (x64 * GX.double()).sum().backward()
    Pd, pd, GXd = P.to(DEV), pts.to(DEV), GX.to(DEV)
    cd = conf.to(DEV) if with_conf else None
    gp = torch.full((B, NV, J, 2), NAN, device=DEV)
    gc = torch.full((B, NV, J), NAN, device=DEV) if with_conf else None
    H.check(lib.lt_triangulate_dlt_bwd(Pd.data_ptr(), pd.data_ptr(), H.ptr(cd), GXd.data_ptr(), gp.data_ptr(), H.ptr(gc), B, NV, J, _st()), "lt_triangulate_dlt_bwd")
    check("geo/dlt_bwd %s d/d points" % cid, gp.cpu(), p64.grad, 1e-5)
    if with_conf:
        check("geo/dlt_bwd %s d/d confidences" % cid, gc.cpu(), c64.grad, 1e-5)


# ---- lt_coord_volumes ------------------------------------------------------------------------------------------------------------------------------------------
def test_coord_volumes_B9_V64_past_8192_workgroups():
    """9 x 64^3 = 2 359 296 voxels against the 8192 x 256 = 2 097 152 lanes of the capped grid: the grid-stride loop takes a second trip.  theta = 0,
    every sample with its own base point; bit for bit against the oracle."""
    H, lib = _lib()
    B, V, side = 9, 64, 2500.0
    wanted, launched = _coord_volumes_grid(B, V)
    assert wanted == 9216 and launched == 8192
    g = _gen("coord_volumes past the cap")
    base = (torch.randn(B, 3, generator=g).double() * 400.0).numpy() + np.array([30.0, -20.0, 10.0])
    pos = torch.from_numpy((base - side / 2.0).astype(np.float32)).to(DEV)
    cen = torch.from_numpy(base.astype(np.float32)).to(DEV)
    rot = torch.from_numpy(np.stack([O.rotation_matrix((0, 0, 1), 0.0)] * B).astype(np.float32)).contiguous().to(DEV)
    out = torch.full((B, V, V, V, 3), NAN, device=DEV)
    step = float(np.float32(side / (V - 1)))
    H.check(lib.lt_coord_volumes(pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, B, V, 0, out.data_ptr(), _st()), "lt_coord_volumes")
    ref = torch.stack([O.coord_volume(base[b], side, V) for b in range(B)])
    o = out.cpu()
    assert torch.equal(o, ref), "max|d| = %g" % float((o - ref).abs().max())
    check("geo/coord_volumes B9 V64 past_8192_workgroups (bit exact)", o, ref, 0.0)
