"""GPU (-m gpu): the streaming (non-MFMA) kernels of the training step, one C entry point at a time, at the shapes where each of them changes
its code path -- vector body / scalar tail, the grid cap behind the grid-stride loop, the channel-count branches of csrc/colsum.h -- against a plain
CPU reference written here: fp64 where the kernel rounds, bit for bit where the operation is exact (casts, gathers, pools, fp8 bytes).
Kernels: csrc/train.hip, csrc/colsum.h, csrc/quant_fp8.hip, csrc/pool_layout.hip (and lt_bn_stats_fwd / lt_rotate_points, which share colsum.h / the
grid-stride pattern).  tests/test_gpu_train.py holds the same kernels at three everyday shapes; the tolerances here are the ones used there:
2e-6 forward, 2e-5 dy / dgamma / dbeta, 1e-6 activation backward and channel sums, 1e-5 batch statistics, 8e-3 (+ the rms bound of check()) for a
bf16 output.  Every case id names the branch it enters; _plan() restates colsum_plan() / the launch arithmetic and each case ASSERTS that the
branch is really entered for its shape."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import check, record, to_cl, from_cl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
UNSUPPORTED = -2


def _lib():
    import lt_hip as H
    return H, H.lib()


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _bf(t):
    return t.to(BF).float()


def _cdiv(a, b):
    return -(-a // b)


# ---- the launch arithmetic, restated (csrc/colsum.h colsum_plan / colsum_fast, lt_bn_act_fwd's grid) ----------------------------------------
def _colsum_fast(C):
    if C < 4 or C % 4:
        return False
    c4 = C // 4
    return (c4 & (c4 - 1)) == 0 if c4 <= 256 else c4 % 256 == 0


def _plan(rows, C):
    c4 = C // 4
    cw4 = min(c4, 256)
    rl = 256 // cw4
    ncb = (c4 + 255) // 256
    n = rows // (rl * 8)
    n = max(1, min(n, 2048 // ncb, (512 << 10) // C))
    return dict(nslab=n, ncb=ncb, cw4=cw4, rl=rl)


def _slab_rows(rows, nslab):
    return [rows * (s + 1) // nslab - rows * s // nslab for s in range(nslab)]


def _fwd_grid(rows, C):
    """(workgroups before the cap, rounding factor m, workgroups launched) of lt_bn_act_fwd."""
    c4 = C // 4
    raw = _cdiv(rows * c4, 256)
    blocks = min(raw, 8192)
    m = c4 // int(np.gcd(c4, 256))
    return raw, m, _cdiv(blocks, m) * m


BN_SHAPES = {  # id -> (rows, C)
    "139x4_cw4_1_rl256_rows_lt_rl": (139, 4),
    "139x1024_rl1_no_lds_combine": (139, 1024),
    "139x2048_C2048_ncb2_groups_and_tail": (139, 2048),
    "3x64_rows_lt_rl": (3, 64),
    "1x64_one_row_var0": (1, 64),
    "1000x12_generic_m3": (1000, 12),
    "130000x68_generic_apply_cap_fwd_cap_m17": (130000, 68),
    "33000x256_vec_fwd_cap": (33000, 256),
}
BIG = ("130000x68_generic_apply_cap_fwd_cap_m17", "33000x256_vec_fwd_cap")
VARIANTS = {  # id -> (flags name, residual, accumulate_res)
    "none": ("none", False, 0),
    "relu_post_res_acc": ("relu", True, 1),
    "relu_pre_res_noacc": ("relu_pre", True, 0),
}
# every variant on the small shapes (fast and generic); the two 8-million-element shapes once each per variant family that differs in code
BN_FP32 = [(s, v) for s in BN_SHAPES if s not in BIG for v in VARIANTS] + [(BIG[0], "relu_post_res_acc"), (BIG[0], "none"), (BIG[1], "relu_pre_res_noacc"),
                                                                             (BIG[1], "relu_post_res_acc")]
BN_BF16 = [(s, v) for s in BN_SHAPES if s not in BIG and _colsum_fast(BN_SHAPES[s][1]) for v in VARIANTS] + [(BIG[1], "relu_post_res_acc"),
                                                                                                               ("1000x12_generic_m3", "relu_post_res_acc")]


def _assert_branch(sid):
    """The shape enters the branch its id names (the plan values are quoted in the pull request that added this module)."""
    rows, C = BN_SHAPES[sid]
    raw, m, grid = _fwd_grid(rows, C)
    if not _colsum_fast(C):
        assert sid.startswith(("1000x12", "130000x68"))
    else:
        p = _plan(rows, C)
        sl = _slab_rows(rows, p["nslab"])
    if sid.startswith("139x4_"):
        assert p["cw4"] == 1 and p["rl"] == 256 and rows < p["rl"] and p["nslab"] == 1
    elif sid.startswith("139x1024"):
        assert p["rl"] == 1 and p["ncb"] == 1 and p["cw4"] == 256
    elif sid.startswith("139x2048"):
        assert p["ncb"] == 2 and p["rl"] == 1
        # slabs of 8 and 9 rows: whole groups of ROWS (4: BatchNorm backward, 8: sums / statistics) rows in flight AND a remainder row
        assert p["nslab"] == 17 and set(sl) == {8, 9}
    elif sid.startswith(("3x64", "1x64")):
        assert rows < p["rl"] == 16
    elif sid.startswith("1000x12"):
        assert m == 3 and grid % 3 == 0
    elif sid.startswith("130000x68"):
        assert raw > 8192 and m == 17 and grid == 8194 and (grid * 256) % (C // 4) == 0 and _cdiv(rows * C, 256) > 8192
    elif sid.startswith("33000x256"):
        assert raw > 8192 and m == 1 and grid == 8192


def _bn_reference(sid, vid, bf16, frozen=False):
    """Inputs (the recipe of test_bn_act_fwd_bwd) and the fp64 autograd reference.  frozen: statistics that are NOT the batch's, constants of the graph."""
    rows, C = BN_SHAPES[sid]
    flags_name, with_res, acc = VARIANTS[vid]
    g = torch.Generator().manual_seed(rows + C + (1 if bf16 else 0) + (7 if frozen else 0))
    rnd = _bf if bf16 else (lambda t: t)
    y = rnd(torch.randn(rows, C, generator=g) * 2 + 0.5)
    res = rnd(torch.randn(rows, C, generator=g)) if with_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    dz = rnd(torch.randn(rows, C, generator=g))
    yd = y.double().requires_grad_(True); gd = gamma.double().requires_grad_(True); bd = beta.double().requires_grad_(True)
    rd = res.double().requires_grad_(True) if with_res else None
    if frozen:
        mean, var = (torch.randn(C, generator=g) * 0.3).double(), (torch.rand(C, generator=g) + 0.5).double()
    else:
        mean, var = yd.mean(0), yd.var(0, unbiased=False)
    n = (yd - mean) / torch.sqrt(var + 1e-5) * gd + bd
    masked = 0
    if flags_name == "relu_pre":
        keep = n.detach().abs() > 1e-4          # no upstream gradient where fp32 rounding could flip the ReLU mask
        masked = int((~keep).sum()); dz = dz * keep.float()
        n = F.relu(n)
    if with_res:
        n = n + rd
    if flags_name == "relu":
        keep = n.detach().abs() > 1e-4
        masked = int((~keep).sum()); dz = dz * keep.float()
        n = F.relu(n)
    (n * dz.double()).sum().backward()
    share = masked / float(rows * C)
    return dict(rows=rows, C=C, y=y, res=res, gamma=gamma, beta=beta, dz=dz, mean=mean.detach(), var=var.detach(), z=n.detach(), dy=yd.grad, dgamma=gd.grad,
                dbeta=bd.grad, dres=rd.grad if with_res else None, masked_share=share, flags_name=flags_name, with_res=with_res, acc=acc)


def _flags(H, name):
    return {"none": 0, "relu": H.EPI_RELU_POST, "relu_pre": H.EPI_RELU_PRE}[name]


def _check_dy(tag, ours, R, tol, invstd):
    """dy against the reference; with ONE row the reference is exactly 0 (g - dbeta / 1 cancels), so the error is measured against the terms that
    cancel, gamma * invstd * g, instead of against max|ref| = 0."""
    if R["rows"] == 1:
        scale = float((R["gamma"].double() * invstd * R["dz"].double()).abs().max())
        e = float((ours.double() - R["dy"]).abs().max()) / max(scale, 1e-30)
        record(tag + " (one row: |dy - 0| / max|gamma invstd g|)", {"err": e, "tol": tol})
        assert float(R["dy"].abs().max()) <= 1e-12 * max(scale, 1e-30) and e <= tol, (tag, e)
    else:
        check(tag, ours, R["dy"], tol)


@pytest.mark.parametrize("sid,vid", BN_FP32, ids=["%s-%s" % sv for sv in BN_FP32])
def test_bn_act_fwd_bwd_fp32(sid, vid):
    """lt_bn_stats_fwd, lt_bn_act_fwd (+ z_bf16), lt_bn_act_bwd (+ dy_bf16 on the vector path; refused on the generic one) in fp32."""
    H, lib = _lib()
    _assert_branch(sid)
    R = _bn_reference(sid, vid, False)
    rows, C = R["rows"], R["C"]
    fast = _colsum_fast(C)
    tag = "trk/bn_act fp32 %s %s" % (sid, vid)
    record(tag + " masked share", R["masked_share"])
    assert R["masked_share"] < 1e-3
    flags = _flags(H, R["flags_name"])
    yg, dzg = R["y"].to(DEV), R["dz"].to(DEV)
    resg = R["res"].to(DEV) if R["with_res"] else None
    gg, bg = R["gamma"].to(DEV), R["beta"].to(DEV)
    # the statistics pass (colsum.h with two quantities, eight rows in flight)
    m2, v2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws0 = torch.empty(max(1, lib.lt_bn_stats_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    H.check(lib.lt_bn_stats_fwd(H.LT_F32, yg.data_ptr(), rows, C, m2.data_ptr(), v2.data_ptr(), None, None, 0.1, ws0.data_ptr(), _st()), "stats")
    check(tag + " mean", m2.cpu(), R["mean"], 1e-5)
    if rows > 1:
        check(tag + " var", v2.cpu(), R["var"], 1e-5)
    else:          # E[x^2] - mean^2 with x^2 rounded to fp32 before the fp64 sum: at most 2^-24 x^2 away from the exact 0, never negative
        assert bool((v2.cpu() >= 0).all()) and bool((v2.cpu().double() <= 2.0 ** -23 * R["y"][0].double() ** 2).all())
    mg, vg = R["mean"].float().to(DEV), R["var"].float().to(DEV)
    z = torch.empty_like(yg)
    z16 = torch.empty(rows, C, dtype=BF, device=DEV)
    H.check(lib.lt_bn_act_fwd(yg.data_ptr(), mg.data_ptr(), vg.data_ptr(), gg.data_ptr(), bg.data_ptr(), H.ptr(resg), z.data_ptr(), z16.data_ptr(), rows, C, 1e-5, flags, _st()), "fwd")
    assert torch.equal(z16, z.bfloat16()), "the bf16 copy is the rounded fp32 result"
    check(tag + " fwd", z.cpu(), R["z"], 2e-6)
    dy, dga, dbe = torch.empty_like(yg), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dres = torch.full_like(yg, 3.0) if R["with_res"] else None
    ws = torch.empty(max(1, lib.lt_bn_act_bwd_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    dy16 = torch.empty(rows, C, dtype=BF, device=DEV)

    def bwd(dy16_ptr):
        return lib.lt_bn_act_bwd(dzg.data_ptr(), yg.data_ptr(), H.ptr(resg), mg.data_ptr(), vg.data_ptr(), gg.data_ptr(), bg.data_ptr(), dy.data_ptr(), dy16_ptr,
                                 dga.data_ptr(), dbe.data_ptr(), H.ptr(dres), R["acc"], rows, C, 1e-5, flags, ws.data_ptr(), _st())

    if fast:
        H.check(bwd(dy16.data_ptr()), "bwd")
        assert torch.equal(dy16, dy.bfloat16())
    else:          # the generic path has no bf16 copy of dy: refused, nothing written
        assert bwd(dy16.data_ptr()) == UNSUPPORTED
        assert b"vector path" in lib.lt_last_error() and ("C=%d" % C).encode() in lib.lt_last_error()
        H.check(bwd(None), "bwd")
    invstd = 1.0 / torch.sqrt(R["var"] + 1e-5)
    _check_dy(tag + " dy", dy.cpu(), R, 2e-5, invstd)
    check(tag + " dgamma", dga.cpu(), R["dgamma"], 2e-5)
    check(tag + " dbeta", dbe.cpu(), R["dbeta"], 2e-5)
    if R["with_res"]:
        check(tag + " dres (%s 3)" % ("accumulated onto" if R["acc"] else "overwrites the"), dres.cpu(), R["dres"] + (3.0 if R["acc"] else 0.0), 2e-6)


@pytest.mark.parametrize("sid,vid", BN_BF16, ids=["%s-%s" % sv for sv in BN_BF16])
def test_bn_act_fwd_bwd_bf16_activations(sid, vid):
    """LT_ACT_BF16 | LT_BN_Y_BF16: y, residual, z, dz, dy, dres are bf16 tensors.  Reference: fp64 autograd over the bf16-ROUNDED inputs; bf16 outputs at
    8e-3 (one rounding, plus the rms bound of check()), the fp32 sums and statistics at the fp32 tolerances."""
    H, lib = _lib()
    _assert_branch(sid)
    R = _bn_reference(sid, vid, True)
    rows, C = R["rows"], R["C"]
    tag = "trk/bn_act bf16 %s %s" % (sid, vid)
    record(tag + " masked share", R["masked_share"])
    assert R["masked_share"] < 1e-3
    fl = _flags(H, R["flags_name"]) | H.BN_Y_BF16 | H.ACT_BF16
    yg, dzg = R["y"].to(DEV, BF), R["dz"].to(DEV, BF)
    resg = R["res"].to(DEV, BF) if R["with_res"] else None
    gg, bg = R["gamma"].to(DEV), R["beta"].to(DEV)
    m2, v2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws0 = torch.empty(max(1, lib.lt_bn_stats_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    H.check(lib.lt_bn_stats_fwd(H.LT_BF16, yg.data_ptr(), rows, C, m2.data_ptr(), v2.data_ptr(), None, None, 0.1, ws0.data_ptr(), _st()), "stats")
    check(tag + " mean", m2.cpu(), R["mean"], 1e-5)
    if rows > 1:
        check(tag + " var", v2.cpu(), R["var"], 1e-5)
    mg, vg = R["mean"].float().to(DEV), R["var"].float().to(DEV)
    z = torch.empty(rows, C, dtype=BF, device=DEV)
    H.check(lib.lt_bn_act_fwd(yg.data_ptr(), mg.data_ptr(), vg.data_ptr(), gg.data_ptr(), bg.data_ptr(), H.ptr(resg), z.data_ptr(), None, rows, C, 1e-5, fl, _st()), "fwd")
    check(tag + " fwd", z.float().cpu(), R["z"], 8e-3)
    dy, dga, dbe = torch.empty(rows, C, dtype=BF, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dres = torch.full((rows, C), 3.0, dtype=BF, device=DEV) if R["with_res"] else None
    ws = torch.empty(max(1, lib.lt_bn_act_bwd_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    args = (dzg.data_ptr(), yg.data_ptr(), H.ptr(resg), mg.data_ptr(), vg.data_ptr(), gg.data_ptr(), bg.data_ptr(), dy.data_ptr())
    tail = (dga.data_ptr(), dbe.data_ptr(), H.ptr(dres), R["acc"], rows, C, 1e-5, fl, ws.data_ptr(), _st())
    assert lib.lt_bn_act_bwd(*args, dy.data_ptr(), *tail) == UNSUPPORTED, "with LT_ACT_BF16 dy itself is the bf16 tensor"
    H.check(lib.lt_bn_act_bwd(*args, None, *tail), "bwd")
    invstd = 1.0 / torch.sqrt(R["var"] + 1e-5)
    _check_dy(tag + " dy", dy.float().cpu(), R, 8e-3, invstd)
    check(tag + " dgamma", dga.cpu(), R["dgamma"], 2e-5)
    check(tag + " dbeta", dbe.cpu(), R["dbeta"], 2e-5)
    if R["with_res"]:
        check(tag + " dres", dres.float().cpu(), R["dres"] + (3.0 if R["acc"] else 0.0), 8e-3)


def test_bn_act_fwd_refuses_c17():
    H, lib = _lib()
    t = torch.zeros(8, 17, device=DEV)
    v = torch.ones(17, device=DEV)
    assert lib.lt_bn_act_fwd(t.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), None, t.data_ptr(), None, 8, 17, 1e-5, 0, _st()) == UNSUPPORTED
    assert b"C=17" in lib.lt_last_error()


@pytest.mark.parametrize("sid", ["139x1024_rl1_no_lds_combine", "1000x12_generic_m3"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "act16"])
def test_bn_act_bwd_frozen_statistics(sid, bf16):
    """LT_BN_FROZEN: mean / var are running statistics (here: NOT the batch's), constants of the graph: dy = gamma * invstd * g with no batch terms
    (inv_n = 0), while dgamma / dbeta are still the sums over the batch."""
    H, lib = _lib()
    R = _bn_reference(sid, "relu_post_res_acc", bf16, frozen=True)
    rows, C = R["rows"], R["C"]
    tag = "trk/bn_act frozen %s %s" % ("bf16" if bf16 else "fp32", sid)
    record(tag + " masked share", R["masked_share"])
    assert R["masked_share"] < 1e-3
    # the reference really has no batch terms: dy = gamma * invstd * dz * mask
    invstd = 1.0 / torch.sqrt(R["var"] + 1e-5)
    mask = (R["z"] > 0).double()
    assert torch.allclose(R["dy"], R["gamma"].double() * invstd * R["dz"].double() * mask, rtol=1e-12, atol=0)
    dt = BF if bf16 else torch.float32
    fl = H.EPI_RELU_POST | H.BN_FROZEN | ((H.BN_Y_BF16 | H.ACT_BF16) if bf16 else 0)
    yg, dzg, resg = R["y"].to(DEV, dt), R["dz"].to(DEV, dt), R["res"].to(DEV, dt)
    mg, vg, gg, bg = R["mean"].float().to(DEV), R["var"].float().to(DEV), R["gamma"].to(DEV), R["beta"].to(DEV)
    dy, dga, dbe = torch.empty(rows, C, dtype=dt, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dres = torch.full((rows, C), 3.0, dtype=dt, device=DEV)
    ws = torch.empty(max(1, lib.lt_bn_act_bwd_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    H.check(lib.lt_bn_act_bwd(dzg.data_ptr(), yg.data_ptr(), resg.data_ptr(), mg.data_ptr(), vg.data_ptr(), gg.data_ptr(), bg.data_ptr(), dy.data_ptr(), None,
                              dga.data_ptr(), dbe.data_ptr(), dres.data_ptr(), 1, rows, C, 1e-5, fl, ws.data_ptr(), _st()), "bwd")
    check(tag + " dy", dy.float().cpu(), R["dy"], 8e-3 if bf16 else 2e-5)
    check(tag + " dgamma", dga.cpu(), R["dgamma"], 2e-5)
    check(tag + " dbeta", dbe.cpu(), R["dbeta"], 2e-5)
    check(tag + " dres", dres.float().cpu(), R["dres"] + 3.0, 8e-3 if bf16 else 2e-6)


@pytest.mark.parametrize("sid", list(BN_SHAPES))
def test_channel_sum(sid):
    """lt_channel_sum / lt_channel_sum_dt(bf16) with accumulate 0 and 1 (eight rows in flight on the vector path: 139 x 2048 has slabs of one whole
    group, and of one group and a remainder row)."""
    H, lib = _lib()
    _assert_branch(sid)
    rows, C = BN_SHAPES[sid]
    g = torch.Generator().manual_seed(rows * 3 + C)
    x = torch.randn(rows, C, generator=g)
    prev = torch.randn(C, generator=g) * 5
    ws = torch.empty(max(1, lib.lt_channel_sum_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    for name, xs, dtc in (("fp32", x, H.LT_F32), ("bf16", _bf(x), H.LT_BF16)):
        xg = xs.to(DEV, BF if dtc == H.LT_BF16 else torch.float32)
        ref = xs.double().sum(0)
        for acc in (0, 1):
            out = prev.to(DEV).clone()
            if dtc == H.LT_F32:
                H.check(lib.lt_channel_sum(xg.data_ptr(), rows, C, out.data_ptr(), acc, ws.data_ptr(), _st()), "lt_channel_sum")
            else:
                H.check(lib.lt_channel_sum_dt(dtc, xg.data_ptr(), rows, C, out.data_ptr(), acc, ws.data_ptr(), _st()), "lt_channel_sum_dt")
            check("trk/channel_sum %s %s accumulate=%d" % (name, sid, acc), out.cpu(), ref + (prev.double() if acc else 0.0), 1e-6)


ACT_TOTAL = 2097152 + 1029          # 8197 workgroups wanted, 8192 launched: the stride loop runs, and its second trip ends ragged


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "act16"])
@pytest.mark.parametrize("flags_name", ["none", "relu_post", "relu_pre", "sigmoid"])
def test_act_bwd_past_the_grid_cap(flags_name, bf16):
    """lt_act_bwd over 2 097 152 + 1029 elements.  none / relu_post with a residual (dres overwritten / accumulated), relu_pre and sigmoid without.
    ReLU masks on bf16 tensors are exact (dz or 0, one bf16 addition for the accumulated dres); sigmoid: dz * z * (1 - z) in fp64 from the stored z."""
    H, lib = _lib()
    assert _cdiv(ACT_TOTAL, 256) > 8192
    n = ACT_TOTAL
    g = torch.Generator().manual_seed(11)
    rnd = _bf if bf16 else (lambda t: t)
    dt = BF if bf16 else torch.float32
    a16 = H.ACT_BF16 if bf16 else 0
    dz = rnd(torch.randn(n, generator=g))
    pre, res = rnd(torch.randn(n, generator=g)), rnd(torch.randn(n, generator=g))
    tag = "trk/act_bwd %s %s" % (flags_name, "bf16" if bf16 else "fp32")
    if flags_name == "sigmoid":
        z = rnd(torch.sigmoid(pre))
        ref = dz.double() * z.double() * (1.0 - z.double())
        zg, dzg = z.to(DEV, dt), dz.to(DEV, dt)
        dy = torch.empty(n, dtype=dt, device=DEV)
        H.check(lib.lt_act_bwd(dzg.data_ptr(), zg.data_ptr(), None, dy.data_ptr(), None, 0, n, H.EPI_SIGMOID | a16, _st()), "lt_act_bwd")
        check(tag + " dy", dy.float().cpu(), ref, 8e-3 if bf16 else 1e-6)
        return
    if flags_name == "relu_pre":
        z = F.relu(pre)
        zg, dzg = z.to(DEV, dt), dz.to(DEV, dt)
        dy = torch.empty(n, dtype=dt, device=DEV)
        H.check(lib.lt_act_bwd(dzg.data_ptr(), zg.data_ptr(), None, dy.data_ptr(), None, 0, n, H.EPI_RELU_PRE | a16, _st()), "lt_act_bwd")
        ref = dz * (z > 0).float()
        assert torch.equal(dy.float().cpu(), ref), tag          # exact in both element types
        check(tag + " dy", dy.float().cpu(), ref.double(), 1e-6)
        return
    acc = 1 if flags_name == "relu_post" else 0
    z = rnd(F.relu(pre + res)) if flags_name == "relu_post" else rnd(pre + res)
    zg, dzg, resg = z.to(DEV, dt), dz.to(DEV, dt), res.to(DEV, dt)
    dy, dres = torch.empty(n, dtype=dt, device=DEV), torch.full((n,), 2.0, dtype=dt, device=DEV)
    H.check(lib.lt_act_bwd(dzg.data_ptr(), zg.data_ptr(), resg.data_ptr(), dy.data_ptr(), dres.data_ptr(), acc, n, (H.EPI_RELU_POST if acc else 0) | a16, _st()), "lt_act_bwd")
    gref = dz * (z > 0).float() if flags_name == "relu_post" else dz
    dres_ref = gref + 2.0 if acc else gref          # fp32 addition, then (bf16 tensors) one rounding: the kernel's own arithmetic
    if bf16:
        assert torch.equal(dy.cpu(), gref.to(BF)) and torch.equal(dres.cpu(), dres_ref.to(BF)), tag
    check(tag + " dy", dy.float().cpu(), gref.double(), 8e-3 if bf16 else 1e-6)
    check(tag + " dres", dres.float().cpu(), gref.double() + (2.0 if acc else 0.0), 8e-3 if bf16 else 1e-6)


# ---- pools ---------------------------------------------------------------------------------------------------------------------------------------
POOL_FWD = {  # id -> (nd, k, s, p, NCHW shape by dtype)
    "2d_k3s2p1_15x17_one_vector": (2, 3, 2, 1, {"fp32": (2, 4, 15, 17), "bf16": (2, 8, 15, 17)}),
    "2d_k3s2p1_15x17_C64": (2, 3, 2, 1, {"fp32": (2, 64, 15, 17), "bf16": (2, 64, 15, 17)}),
    "3d_k2s2p0_7x9x11_one_vector": (3, 2, 2, 0, {"fp32": (2, 4, 7, 9, 11), "bf16": (2, 8, 7, 9, 11)}),
    "3d_k2s2p0_6x8x10_C64": (3, 2, 2, 0, {"fp32": (1, 64, 6, 8, 10), "bf16": (1, 64, 6, 8, 10)}),
    # 4096 workgroups of 256 (output pixel, 16-byte channel vector) pairs = 1 048 576: 257 x 256 (x 2) output pixels x 16 (8) vectors is 1 052 672
    "2d_k3s2p1_past_4096_workgroups": (2, 3, 2, 1, {"fp32": (1, 64, 514, 512), "bf16": (1, 64, 514, 1024)}),
}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("pid", list(POOL_FWD))
def test_maxpool_fwd(pid, dt):
    """lt_maxpool_fwd bit for bit against F.max_pool*d on the same (bf16-rounded) values.  (NaN inputs are left out: the kernel takes its maximum with
    fmaxf, which drops a NaN where torch propagates it -- no layer of these networks can produce one in front of a pool.)"""
    H, lib = _lib()
    nd, k, s, p, shapes = POOL_FWD[pid]
    shape = shapes[dt]
    g = torch.Generator().manual_seed(len(pid))
    x = torch.randn(shape, generator=g)
    x = _bf(x) if dt == "bf16" else x
    ref = (F.max_pool2d if nd == 2 else F.max_pool3d)(x, k, s, p)
    tdt = BF if dt == "bf16" else torch.float32
    xg = to_cl(x, None, tdt)
    N, D, Hh, W, C = xg.shape
    kk, ss, pp = ((1, k, k), (1, s, s), (0, p, p)) if nd == 2 else ((k,) * 3, (s,) * 3, (p,) * 3)
    Do, Ho, Wo = [(n + 2 * q - a) // b + 1 for n, q, a, b in zip((D, Hh, W), pp, kk, ss)]
    vec = 8 if dt == "bf16" else 4
    if "past_4096" in pid:
        assert _cdiv(N * Do * Ho * Wo * (C // vec), 256) > 4096
    if "one_vector" in pid:
        assert C == vec
    yg = torch.full((N, Do, Ho, Wo, C), float("nan"), dtype=tdt, device=DEV)
    H.check(lib.lt_maxpool_fwd(H.LT_BF16 if dt == "bf16" else H.LT_F32, xg.data_ptr(), yg.data_ptr(), N, D, Hh, W, C, H.i3(kk), H.i3(ss), H.i3(pp), _st()), "lt_maxpool_fwd")
    ours = from_cl(yg, nd)
    assert ours.shape == ref.shape and torch.equal(ours, ref), "max|d| = %g" % float((ours - ref).abs().max())


@pytest.mark.parametrize("shape", [(2, 64, 15, 17), (3, 16, 20, 24)], ids=["2x64x15x17", "3x16x20x24"])
def test_maxpool_bwd_bf16_overlapping_windows(shape):
    """lt_maxpool_bwd_dt on bf16 tensors with the stem's 3x3 / stride 2 / pad 1 pool: an input collects up to four contributions, one per class
    (oh % 2, ow % 2) of outputs, added in the launch order (0,0) (0,1) (1,0) (1,1), each by a read-add-write that rounds to bf16.  Reference: that
    contract, emulated -- the argmax of max_pool2d(return_indices=True) on the CPU (first maximum in scan order), the classes added in that order
    with a rounding to bf16 after each.  ReLU-ed input: ties at zero; bit for bit where x > 0, and the total (where x == 0 the gradient dies in the
    ReLU backward that follows, and a different choice among tied zeros would only move it between such elements)."""
    H, lib = _lib()
    g = torch.Generator().manual_seed(21)
    x = _bf(F.relu(torch.randn(shape, generator=g)))
    y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    dyv = _bf(torch.randn(y.shape, generator=g))
    N, C, Hh, W = shape
    Ho, Wo = y.shape[2:]
    dx = torch.zeros(N, C, Hh * W)
    oh, ow = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    multi = torch.zeros(N, C, Hh * W)
    for ch in (0, 1):
        for cw in (0, 1):
            sel = ((oh % 2 == ch) & (ow % 2 == cw)).reshape(-1)
            add = torch.zeros_like(dx)
            add.scatter_(2, idx.reshape(N, C, -1)[:, :, sel], dyv.reshape(N, C, -1)[:, :, sel])          # windows of one class never share an input
            multi += torch.zeros_like(dx).scatter_(2, idx.reshape(N, C, -1)[:, :, sel], torch.ones(N, C, int(sel.sum())))
            dx = _bf(dx + add)
    ref = dx.reshape(shape)
    assert int(multi.max()) >= 3, "no input collects three or more contributions: the shape does not test the class order"
    xg, dyg = to_cl(x, None, BF), to_cl(dyv, None, BF)
    dxg = torch.zeros_like(xg)
    Nn, D, H_, W_, Cc = xg.shape
    H.check(lib.lt_maxpool_bwd_dt(H.LT_BF16, xg.data_ptr(), dyg.data_ptr(), dxg.data_ptr(), Nn, D, H_, W_, Cc, H.i3((1, 3, 3)), H.i3((1, 2, 2)), H.i3((0, 1, 1)), _st()), "lt_maxpool_bwd_dt")
    ours = from_cl(dxg, 2)
    m = x > 0
    tag = "trk/maxpool_bwd bf16 3x3s2p1 %s" % "x".join(map(str, shape))
    record(tag + " equal everywhere (ties at zero included)", bool(torch.equal(ours, ref)))
    assert torch.equal(ours * m, ref * m), "max|d| where x > 0 = %g" % float(((ours - ref) * m).abs().max())
    assert abs(float(ours.double().sum()) - float(ref.double().sum())) <= 1e-3 * float(ref.double().abs().sum())


AVG_SHAPES = {"N3_HW1_C64": (3, 1, 64), "N2_HW37_C17": (2, 37, 17), "N2_HW96_C256": (2, 96, 256)}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("aid", list(AVG_SHAPES))
def test_global_avgpool(aid, dt):
    """lt_global_avgpool: HW = 1, C not a multiple of the 64-channel slab with HW % 4 != 0, four slabs (1e-6 fp32 / 4e-3 bf16 as in test_gpu_kernels)."""
    H, lib = _lib()
    N, HW, C = AVG_SHAPES[aid]
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(N, HW, C, generator=g)
    x = _bf(x) if dt == "bf16" else x
    tdt = BF if dt == "bf16" else torch.float32
    xg = x.to(DEV, tdt)
    yg = torch.full((N, C), float("nan"), dtype=tdt, device=DEV)
    H.check(lib.lt_global_avgpool(H.LT_BF16 if dt == "bf16" else H.LT_F32, xg.data_ptr(), yg.data_ptr(), N, HW, C, _st()), "lt_global_avgpool")
    check("trk/global_avgpool %s %s" % (dt, aid), yg.float().cpu(), x.double().mean(1), 4e-3 if dt == "bf16" else 1e-6)


AVGB_SHAPES = dict(AVG_SHAPES, **{"N3_HW161_C4343_past_8192_workgroups": (3, 161, 4343)})


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("acc", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("aid", list(AVGB_SHAPES))
def test_global_avgpool_bwd(aid, acc, dt):
    """lt_global_avgpool_bwd(_dt): dx[n][p][c] (=|+=) dy[n][c] / HW; 3 x 161 x 4343 = 2 097 152 + 517 elements runs the grid-stride loop."""
    H, lib = _lib()
    N, HW, C = AVGB_SHAPES[aid]
    if "past" in aid:
        assert N * HW * C == 2097152 + 517 and _cdiv(N * HW * C, 256) > 8192
    g = torch.Generator().manual_seed(HW * 5 + C)
    rnd = _bf if dt == "bf16" else (lambda t: t)
    tdt = BF if dt == "bf16" else torch.float32
    dyv, prev = rnd(torch.randn(N, C, generator=g)), rnd(torch.randn(N, HW, C, generator=g))
    ref = (dyv.double() / HW)[:, None, :].expand(N, HW, C) + (prev.double() if acc else 0.0)
    dyg, dxg = dyv.to(DEV, tdt), prev.to(DEV, tdt).clone()
    if dt == "fp32":
        H.check(lib.lt_global_avgpool_bwd(dyg.data_ptr(), dxg.data_ptr(), N, HW, C, acc, _st()), "lt_global_avgpool_bwd")
    else:
        H.check(lib.lt_global_avgpool_bwd_dt(H.LT_BF16, dyg.data_ptr(), dxg.data_ptr(), N, HW, C, acc, _st()), "lt_global_avgpool_bwd_dt")
    check("trk/global_avgpool_bwd %s %s accumulate=%d" % (dt, aid, acc), dxg.float().cpu(), ref, 8e-3 if dt == "bf16" else 1e-6)


# ---- casts, gathers, adds: bit for bit ---------------------------------------------------------------------------------------------------------------
def _table():
    """64 fp32 bit patterns at the edges of the fp32 -> bf16 rounding (round to nearest even on the upper 16 bits)."""
    bits = [
        0x00000000, 0x80000000,                                      # +-0
        0x00000001, 0x80000001, 0x007fffff, 0x807fffff,              # smallest / largest fp32 subnormal
        0x00008000, 0x00018000, 0x00007fff, 0x00008001,              # subnormal ties (to even: down to 0, up to 2) and their neighbours
        0x80008000, 0x80018000, 0x007f8000, 0x007e8000,              # ... negative; a subnormal that rounds up into the normals; one that ties down
        0x00800000, 0x80800000, 0x00ffffff,                          # smallest normal, the largest value of its binade
        0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,              # 1 + 2^-8: tie, even below (down); 1 + 3 * 2^-8: tie, even above (up); negative
        0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,              # one ulp either side of the ties
        0x3f800000, 0xbf800000, 0x3f7fffff, 0x3effffff,              # 1, -1, values that round up across a binade
        0x7f7fffff, 0xff7fffff,                                      # largest finite fp32: rounds to +-inf
        0x7f7f8000, 0xff7f8000,                                      # the tie between the largest finite bf16 and inf: rounds to inf (even)
        0x7f7f7fff, 0xff7f7fff, 0x7f7f0000, 0x7f7e8000,              # just below it: the largest finite bf16; that value itself; a tie down to 0x7f7e
        0x7f800000, 0xff800000,                                      # +-inf
        0x7fc00000, 0xffc00000, 0x7fc00001, 0x7fffffff,              # quiet NaNs
        0x7f800001, 0xff800001, 0x7f80ffff, 0x7fa00000, 0x7f808000,  # signalling NaNs, three of them with the payload only in the 16 bits a truncation drops
        0x42280000, 0xc2280000, 0x3dcccccd, 0x40490fdb, 0x477fe000,  # 42, -42, 0.1, pi, 65504
        0x33800000, 0x4b7fffff, 0x4b800000, 0x5f000000, 0x1e3ce508,  # 2^-24, 2^24 - 1, 2^24, 2^63, 1e-20
        0x3f80c000, 0x3f814000, 0x3f7f8000, 0x3f7e8000,              # quarter points; ties just below 1
        0x0000ffff, 0x8000ffff,                                      # subnormals just below the second bf16 subnormal
    ]
    assert len(bits) == 64 and len(set(bits)) == 64
    return torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32)).view(torch.float32)


def _assert_same_bf16(ours, x, what):
    """ours (bf16, cpu) == x.to(bfloat16) bit for bit; where x is NaN only "is NaN" is asked (the hardware conversion of the vector bodies returns the
    canonical quiet NaN, the software one of the tails keeps the upper payload bits and sets the quiet bit: lt_common.h)."""
    ref = x.to(BF)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(ours), nan), what + ": NaN positions differ"
    a, b = ours.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]
    bad = a != b
    assert not bool(bad.any()), "%s: %d values differ from torch's rounding, first: fp32 bits 0x%08x -> ours 0x%04x, torch 0x%04x" % (
        what, int(bad.sum()), int(x[~nan][bad][0].view(torch.int32)) & 0xffffffff, int(a[bad][0]) & 0xffff, int(b[bad][0]) & 0xffff)


def _cast_input(n, seed):
    """n fp32 values: the table in front (as much of it as fits), RANDOM BIT PATTERNS behind it (every exponent, subnormals, infinities and NaNs included),
    and the last n % 8 values -- cast_bf16_kernel's scalar tail -- from the table again."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    t = _table()
    x[:min(n, 64)] = t[:min(n, 64)]
    if n > 64 and n % 8:
        x[n - n % 8:] = t[29:29 + n % 8]          # largest finite .. inf .. NaNs
    return x


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055, 33554432 + 13], ids=lambda n: "n%d%s" % (n, "_past_16384_workgroups" if n > 1 << 25 else ""))
def test_cast_f32_bf16(n):
    """lt_cast_f32_bf16: the 8-wide body rounds with the hardware v_cvt_pk_bf16_f32, the tail with the software f32_to_bf16 -- both must be torch's
    round-to-nearest-even on ties, subnormals, the largest finite values, infinities, signed zeros."""
    H, lib = _lib()
    if n > 1 << 25:
        assert _cdiv(n >> 3, 256) > 16384
    x = _cast_input(n, n)
    xg = x.to(DEV)
    out = torch.full((n + 8,), -7.0, dtype=BF, device=DEV)
    H.check(lib.lt_cast_f32_bf16(xg.data_ptr(), out.data_ptr(), n, _st()), "lt_cast_f32_bf16")
    o = out.cpu()
    assert bool((o[n:].float() == -7.0).all()), "wrote past n"
    _assert_same_bf16(o[:n], x, "lt_cast_f32_bf16 n=%d" % n)


def test_cast_f32_bf16_whole_table_through_body_and_tail():
    """Every table value once through the 8-wide body (n = 64) and once through the scalar tail (n = 7 and n = 15: a body of 8 and a tail of 7)."""
    H, lib = _lib()
    t = _table()
    for n, chunks in ((64, [t]), (7, [t[k:k + 7] for k in range(0, 63, 7)] + [t[57:64]]), (15, [torch.cat([t[:8], t[k:k + 7]]) for k in range(0, 63, 7)] + [torch.cat([t[:8], t[57:64]])])):
        for x in chunks:
            assert x.numel() == n
            xg = x.contiguous().to(DEV)
            out = torch.zeros(n, dtype=BF, device=DEV)
            H.check(lib.lt_cast_f32_bf16(xg.data_ptr(), out.data_ptr(), n, _st()), "lt_cast_f32_bf16")
            _assert_same_bf16(out.cpu(), x, "lt_cast_f32_bf16 table n=%d" % n)


@pytest.mark.parametrize("rows,C,cpad,branch", [(16, 4, 4, "vector"), (1, 67, 67, "scalar_total_not_x4"), (4, 16, 20, "scalar_padding")], ids=lambda v: str(v))
def test_convert_pad_table(rows, C, cpad, branch):
    """lt_convert_pad fp32 -> bf16 over the table: the four-wide branch (C == c_pad, total % 4 == 0) and the scalar one (both store through the hardware
    conversion), and back to fp32 (exact)."""
    H, lib = _lib()
    t = _table()
    x = torch.cat([t, t[:3]])[:rows * C].reshape(rows, C).contiguous()
    assert x.numel() >= 64
    xg = x.to(DEV)
    out = torch.full((rows, cpad), -7.0, dtype=BF, device=DEV)
    H.check(lib.lt_convert_pad(H.LT_F32, xg.data_ptr(), H.LT_BF16, out.data_ptr(), rows, C, cpad, _st()), "lt_convert_pad")
    o = out.cpu()
    _assert_same_bf16(o[:, :C].contiguous().reshape(-1), x.reshape(-1), "lt_convert_pad " + branch)
    assert bool((o[:, C:].view(torch.int16) == 0).all())
    back = torch.empty(rows, cpad, device=DEV)
    H.check(lib.lt_convert_pad(H.LT_BF16, out.data_ptr(), H.LT_F32, back.data_ptr(), rows, cpad, cpad, _st()), "lt_convert_pad back")
    b, want = back.cpu(), o.float()
    assert torch.equal(b.view(torch.int32)[~torch.isnan(want)], want.view(torch.int32)[~torch.isnan(want)]) and torch.equal(torch.isnan(b), torch.isnan(want))


def _gather_case(n, seed, nsrc=None):
    g = torch.Generator().manual_seed(seed)
    nsrc = nsrc or n
    src = torch.randn(nsrc, generator=g)
    t = _table()
    src[:min(nsrc, 64)] = t[:min(nsrc, 64)]
    idx = torch.randperm(nsrc, generator=g)[:n].to(torch.int32)
    if n > 1:
        idx[torch.rand(n, generator=g) < 0.1] = -1
    ref = torch.where(idx >= 0, src[idx.clamp(min=0).long()], torch.zeros(()))
    return src, idx, ref


def _assert_same_f32(ours, ref, what):
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(ours), nan) and torch.equal(ours.view(torch.int32)[~nan], ref.view(torch.int32)[~nan]), what


@pytest.mark.parametrize("n", [1, 1025, 4194304 + 77], ids=lambda n: "n%d%s" % (n, "_past_16384_workgroups" if n > 1 << 22 else ""))
def test_gather_f32_and_bf16(n):
    """lt_gather_f32 / lt_gather_f32_bf16: dst[i] = idx[i] >= 0 ? src[idx[i]] : 0 over a random permutation with ~10 % of -1 entries; the bf16 one rounds
    with the software conversion (the table sits in the source)."""
    H, lib = _lib()
    if n > 1 << 22:
        assert _cdiv(n, 256) > 16384
    src, idx, ref = _gather_case(n, n)
    sg, ig = src.to(DEV), idx.to(DEV)
    d32 = torch.full((n + 4,), -7.0, device=DEV)
    H.check(lib.lt_gather_f32(sg.data_ptr(), ig.data_ptr(), d32.data_ptr(), n, _st()), "lt_gather_f32")
    o = d32.cpu()
    _assert_same_f32(o[:n], ref, "lt_gather_f32 n=%d" % n)
    assert bool((o[n:] == -7.0).all())
    d16 = torch.full((n + 4,), -7.0, dtype=BF, device=DEV)
    H.check(lib.lt_gather_f32_bf16(sg.data_ptr(), ig.data_ptr(), d16.data_ptr(), n, _st()), "lt_gather_f32_bf16")
    o = d16.cpu()
    _assert_same_bf16(o[:n], ref, "lt_gather_f32_bf16 n=%d" % n)
    assert bool((o[n:].float() == -7.0).all())


def test_gather_f32_multi():
    """lt_gather_f32_multi: five jobs (1, 1023, 1024, 1025, 5000 elements; 1 + 1 + 1 + 2 + 5 workgroups of 1024), fp32 and bf16 destinations mixed, the
    job table laid out as lt_train.TrainTape.JOB.  Each destination has 1024 elements of slack behind it that must come back untouched."""
    H, lib = _lib()
    import lt_train
    ns = [1, 1023, 1024, 1025, 5000]
    out16 = [0, 1, 0, 1, 0]
    keep, arr, fb = [], np.zeros(len(ns), dtype=lt_train.TrainTape.JOB), 0
    for i, (n, b16) in enumerate(zip(ns, out16)):
        src, idx, ref = _gather_case(n, 100 + i, nsrc=n + 37)
        sg, ig = src.to(DEV), idx.to(DEV)
        dst = torch.full((n + 1024,), -7.0, dtype=BF if b16 else torch.float32, device=DEV)
        arr[i] = (sg.data_ptr(), ig.data_ptr(), dst.data_ptr(), n, fb, b16)
        fb += (n + 1023) // 1024
        keep.append((sg, ig, dst, ref, n, b16))
    assert fb == 10 and arr.itemsize == 40
    tab = torch.from_numpy(arr.view(np.uint8).copy()).to(DEV)
    H.check(lib.lt_gather_f32_multi(tab.data_ptr(), len(ns), fb, _st()), "lt_gather_f32_multi")
    for sg, ig, dst, ref, n, b16 in keep:
        o = dst.cpu()
        assert bool((o[n:].float() == -7.0).all()), "job n=%d wrote into its slack" % n
        if b16:
            _assert_same_bf16(o[:n], ref, "lt_gather_f32_multi bf16 n=%d" % n)
        else:
            _assert_same_f32(o[:n], ref, "lt_gather_f32_multi n=%d" % n)


@pytest.mark.parametrize("n", [3, 4, 1027, 16777216 + 3, 16777216 + 1024 + 3],
                         ids=["n3_tail_only", "n4_one_vector", "n1027", "n16777219_16384_workgroups", "n16778243_past_16384_workgroups"])
def test_add_f32(n):
    """lt_add_f32: y += x, float4 body and scalar tail, exact.  (16 777 216 + 3 elements are exactly the 16384 workgroups of the cap: one trip each; another
    1024 elements make it 16385 wanted and the grid-stride loop runs.)"""
    H, lib = _lib()
    if n == 16777216 + 1024 + 3:
        assert _cdiv(n >> 2, 256) > 16384
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    xg, yg = x.to(DEV), torch.cat([y, torch.full((4,), -7.0)]).to(DEV)
    H.check(lib.lt_add_f32(yg.data_ptr(), xg.data_ptr(), n, _st()), "lt_add_f32")
    o = yg.cpu()
    assert torch.equal(o[:n], y + x) and bool((o[n:] == -7.0).all())


def test_pad_channels_f32():
    H, lib = _lib()
    g = torch.Generator().manual_seed(4)
    rows = 4099
    x = torch.randn(rows, 17, generator=g)
    xg, out = x.to(DEV), torch.full((rows, 32), float("nan"), device=DEV)
    H.check(lib.lt_pad_channels_f32(xg.data_ptr(), out.data_ptr(), rows, 17, 32, _st()), "lt_pad_channels_f32")
    o = out.cpu()
    assert torch.equal(o[:, :17], x) and bool((o[:, 17:].view(torch.int32) == 0).all())


def test_add_i64_multi():
    """lt_add_i64_multi: 300 int64 scalars scattered over a buffer (two workgroups, the second partly filled), delta 3; their neighbours stay."""
    H, lib = _lib()
    g = torch.Generator().manual_seed(8)
    buf = torch.randint(-2 ** 40, 2 ** 40, (5000,), generator=g, dtype=torch.int64)
    pos = torch.randperm(5000, generator=g)[:300]
    bg = buf.to(DEV)
    ptrs = (bg.data_ptr() + pos * 8).to(torch.int64).to(DEV)
    H.check(lib.lt_add_i64_multi(ptrs.data_ptr(), 300, 3, _st()), "lt_add_i64_multi")
    want = buf.clone()
    want[pos] += 3
    assert torch.equal(bg.cpu(), want)


@pytest.mark.parametrize("n", [1, 3])
def test_scale_product(n):
    H, lib = _lib()
    a, b = torch.tensor([0.0123456789], device=DEV), torch.tensor([7.654321e-3], device=DEV)
    dst = torch.full((n + 3,), -7.0, device=DEV)
    H.check(lib.lt_scale_product(dst.data_ptr(), n, a.data_ptr(), b.data_ptr(), _st()), "lt_scale_product")
    o = dst.cpu()
    assert bool((o[:n] == (a.cpu() * b.cpu())).all()) and bool((o[n:] == -7.0).all())


def test_rotate_points():
    """lt_rotate_points: y = R x for 1000 points (four workgroups, the last one partly filled) against the fp64 product."""
    H, lib = _lib()
    g = torch.Generator().manual_seed(13)
    n = 1000
    x = torch.randn(n, 3, generator=g) * 500.0
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g).double())
    R = q.float()
    xg, Rg, yg = x.to(DEV), R.contiguous().to(DEV), torch.full((n + 1, 3), -7.0, device=DEV)
    H.check(lib.lt_rotate_points(xg.data_ptr(), Rg.data_ptr(), yg.data_ptr(), n, _st()), "lt_rotate_points")
    o = yg.cpu()
    check("trk/rotate_points n=1000", o[:n], x.double() @ R.double().T, 1e-6)
    assert bool((o[n:] == -7.0).all())


# ---- fp8 quantisation: bit for bit against torch.float8_e4m3fn -----------------------------------------------------------------------------------
def _amax_call(H, lib, dt, xg, n, slot):
    if dt == "fp32":
        H.check(lib.lt_amax_f32(xg.data_ptr(), n, slot.data_ptr(), _st()), "lt_amax_f32")
    else:
        H.check(lib.lt_amax_dt(H.LT_BF16, xg.data_ptr(), n, slot.data_ptr(), _st()), "lt_amax_dt")
    return float(slot.cpu()[0])


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 4, 1031, 8388608 + 5], ids=lambda n: "n%d%s" % (n, "_past_1024_workgroups" if n > 1 << 23 else ""))
def test_amax(n, dt):
    """lt_amax_f32 / lt_amax_dt(bf16): *amax = max(*amax, max |x|).  The maximum (-7.5: the sign must not matter) in the last element -- of the scalar tail
    when n % 4 != 0 -- and in the first; a larger value already in the slot stays, a smaller one is replaced; all zeros leave 0; a NaN in the data
    leaves the maximum of the rest (documented: fmaxf drops it, and NaN never compares greater)."""
    H, lib = _lib()
    if n > 1 << 23:
        assert _cdiv(n // 4 + 1, 2048) > 1024
    g = torch.Generator().manual_seed(n)
    tdt = BF if dt == "bf16" else torch.float32
    base = torch.randn(n, generator=g).clamp(-4.0, 4.0)
    base = _bf(base) if dt == "bf16" else base
    xg = base.to(DEV, tdt)

    def slot(v):
        return torch.tensor([v], dtype=torch.float32, device=DEV)

    rest = float(base.abs().max())
    assert _amax_call(H, lib, dt, xg, n, slot(0.0)) == rest
    xg[n - 1] = -7.5
    assert _amax_call(H, lib, dt, xg, n, slot(0.0)) == 7.5, "maximum in the last element"
    assert _amax_call(H, lib, dt, xg, n, slot(9.0)) == 9.0, "a larger value in the slot stays"
    assert _amax_call(H, lib, dt, xg, n, slot(2.0)) == 7.5, "the maximum is taken INTO the slot"
    if n >= 3:
        xg[0] = float("nan")
        assert _amax_call(H, lib, dt, xg, n, slot(0.0)) == 7.5, "a NaN in the data leaves the maximum of the rest"
        xg[n - 1] = base[n - 1].item()
        xg[0] = 7.5
        assert _amax_call(H, lib, dt, xg, n, slot(0.0)) == 7.5, "maximum in the first element"
    xg.zero_()
    assert _amax_call(H, lib, dt, xg, n, slot(0.0)) == 0.0, "all zeros"


def _fp8_ref(x, amax):
    """(bytes, scale) of the kernels' contract: scale = amax > 0 ? amax / 448 : 1 in fp32, q = e4m3(x * (1 / scale)) -- test_conv_fp8_operands' expression."""
    scale = np.float32(amax) / np.float32(448.0) if amax > 0 else np.float32(1.0)
    q = (x * float(np.float32(1.0 / np.float32(scale)))).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), np.float32(scale)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099, 16777216 + 9], ids=lambda n: "n%d%s" % (n, "_past_4096_workgroups" if n > 1 << 24 else ""))
def test_quant_fp8(n, dt):
    """lt_quant_fp8 / lt_quant_fp8_dt(bf16): bytes and scale_out exact, 16-wide body and scalar tail; 16 sentinel bytes behind the output survive; amax = 0
    gives scale 1 and all-zero bytes."""
    H, lib = _lib()
    if n > 1 << 24:
        assert _cdiv(n // 16 + 1, 256) > 4096
    g = torch.Generator().manual_seed(n + 1)
    tdt = BF if dt == "bf16" else torch.float32
    x = torch.randn(n, generator=g) * 3.0
    x = _bf(x) if dt == "bf16" else x
    amax = float(x.abs().max())
    xg = x.to(DEV, tdt)

    def run(xg_, amax_):
        q = torch.full((n + 16,), 0xAB, dtype=torch.uint8, device=DEV)
        am, sc = torch.tensor([amax_], dtype=torch.float32, device=DEV), torch.full((1,), -1.0, device=DEV)
        if dt == "fp32":
            H.check(lib.lt_quant_fp8(xg_.data_ptr(), q.data_ptr(), n, am.data_ptr(), sc.data_ptr(), _st()), "lt_quant_fp8")
        else:
            H.check(lib.lt_quant_fp8_dt(H.LT_BF16, xg_.data_ptr(), q.data_ptr(), n, am.data_ptr(), sc.data_ptr(), _st()), "lt_quant_fp8_dt")
        q = q.cpu()
        assert bool((q[n:] == 0xAB).all()), "wrote past n"
        return q[:n], np.float32(sc.cpu()[0].item())

    q, sc = run(xg, amax)
    qr, scr = _fp8_ref(x, amax)
    assert sc == scr, (sc, scr)
    bad = q != qr
    assert not bool(bad.any()), "%d of %d bytes differ, first at %d: x = %r -> ours 0x%02x, torch 0x%02x" % (int(bad.sum()), n, int(bad.nonzero()[0]), float(x[bad][0]), int(q[bad][0]), int(qr[bad][0]))
    q, sc = run(torch.zeros(n, dtype=tdt, device=DEV), 0.0)
    assert sc == np.float32(1.0) and not bool(q.any())


@pytest.mark.parametrize("n", [3, 4, 1029, 4194304 + 6], ids=lambda n: "n%d%s" % (n, "_past_4096_workgroups" if n > 1 << 22 else ""))
def test_gather_f32_fp8(n):
    """lt_gather_f32_fp8: q[i] = idx[i] >= 0 ? e4m3(src[idx[i]] / scale) : 0, int4 index body and scalar tail; -1 gives the byte 0."""
    H, lib = _lib()
    if n > 1 << 22:
        assert _cdiv(n // 4 + 1, 256) > 4096
    g = torch.Generator().manual_seed(n + 2)
    src = torch.randn(n, generator=g) * 0.05
    idx = torch.randperm(n, generator=g).to(torch.int32)
    idx[torch.rand(n, generator=g) < 0.1] = -1
    idx[n - 1] = -1          # (one in the tail / last vector for certain)
    amax = float(src.abs().max())
    gathered = torch.where(idx >= 0, src[idx.clamp(min=0).long()], torch.zeros(()))
    qr, scr = _fp8_ref(gathered, amax)
    assert not bool(qr[idx < 0].any())
    sg, ig = src.to(DEV), idx.to(DEV)
    q = torch.full((n + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    am, sc = torch.tensor([amax], dtype=torch.float32, device=DEV), torch.full((1,), -1.0, device=DEV)
    H.check(lib.lt_gather_f32_fp8(sg.data_ptr(), ig.data_ptr(), q.data_ptr(), n, am.data_ptr(), sc.data_ptr(), _st()), "lt_gather_f32_fp8")
    q = q.cpu()
    assert bool((q[n:] == 0xAB).all()), "wrote past n"
    assert np.float32(sc.cpu()[0].item()) == scr
    assert torch.equal(q[:n], qr), "%d of %d bytes differ" % (int((q[:n] != qr).sum()), n)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    return float(np.spacing(np.float32(v)))


def _adam_gate(tag, ours_p, ours_m, ours_v, t64, t32, st64):
    """exp_avg / exp_avg_sq against the fp64 run at 1e-6 of their maximum; the parameter: max|ours - truth| <= 4 * max|torch fp32 - truth| + ulp(max|p|)
    (what fp32 can do is measured, not assumed: torch's own fp32 Adam against the same truth).  The achieved ratio is recorded."""
    check(tag + " exp_avg", ours_m.cpu(), st64["exp_avg"], 1e-6)
    check(tag + " exp_avg_sq", ours_v.cpu(), st64["exp_avg_sq"], 1e-6)
    truth = t64.detach()
    e_ours = float((ours_p.detach().cpu().double() - truth).abs().max())
    e_t32 = float((t32.detach().double() - truth).abs().max())
    ulp = _ulp32(float(truth.abs().max()))
    record(tag + " parameter", {"err": e_ours, "torch_fp32_err": e_t32, "ulp_of_max_p": ulp, "ratio_to_torch_fp32": e_ours / e_t32 if e_t32 > 0 else None,
                                "bound": 4 * e_t32 + ulp})
    assert e_ours <= 4 * e_t32 + ulp, "%s: |ours - fp64| = %.3e > 4 * %.3e + %.3e" % (tag, e_ours, e_t32, ulp)


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
def test_adam_multi_seven_steps_two_step_counts(wd):
    """lt_train.Adam (lt_adam_step_multi): tensors of 1, 1023, 1024, 1025 and 5000 elements (1 + 1 + 1 + 2 + 5 workgroups: block offsets inside a job and a
    five-entry binary search), two groups with different lr in ONE launch, 7 steps with gradients scaled 10 ** (step - 3).  The 1024-element tensor gets
    its first gradient in the fourth step: two bias-correction groups from then on, i.e. two launches and two job-table slots per step()."""
    import lt_train
    g = torch.Generator().manual_seed(17)
    sizes = [1, 1023, 1024, 1025, 5000]
    late = 2
    p0 = [torch.randn(n, generator=g) * 3.0 for n in sizes]
    mk = lambda ps: [{"params": ps[:3]}, {"params": ps[3:], "lr": 1e-2}]
    p64 = [torch.nn.Parameter(t.double().clone()) for t in p0]
    p32 = [torch.nn.Parameter(t.clone()) for t in p0]
    ours = [torch.nn.Parameter(t.clone().to(DEV)) for t in p0]
    o64 = torch.optim.Adam(mk(p64), lr=1e-3, weight_decay=wd)
    o32 = torch.optim.Adam(mk(p32), lr=1e-3, weight_decay=wd)
    oo = lt_train.Adam(mk(ours), lr=1e-3, weight_decay=wd)
    for step in range(7):
        for i in range(len(sizes)):
            if i == late and step < 3:
                continue
            gr = torch.randn(sizes[i], generator=g) * (10.0 ** (step - 3))
            p64[i].grad = gr.double(); p32[i].grad = gr.clone(); ours[i].grad = gr.to(DEV)
        o64.step(); o32.step(); oo.step()
        assert len(oo._tables_used) == (1 if step < 3 else 2), "launches in step %d: %r" % (step, oo._tables_used)
    torch.cuda.synchronize()
    assert int(o64.state[p64[late]]["step"]) == 4 and oo.state[ours[late]]["step"] == 4 and oo.state[ours[0]]["step"] == 7
    for i, n in enumerate(sizes):
        _adam_gate("trk/adam multi wd=%g n=%d%s" % (wd, n, " (first gradient in step 4)" if i == late else ""), ours[i], oo.state[ours[i]]["m"], oo.state[ours[i]]["v"],
                   p64[i], p32[i], o64.state[p64[i]])


def test_adam_step_single_tensor_past_the_grid_cap():
    """lt_adam_step called directly: 1 048 576 + 77 elements (4096 workgroups launched, 4097 wanted: the grid-stride loop), weight decay, three steps."""
    H, lib = _lib()
    n = 1048576 + 77
    assert _cdiv(n, 256) > 4096
    g = torch.Generator().manual_seed(19)
    p0 = torch.randn(n, generator=g) * 3.0
    p64, p32 = torch.nn.Parameter(p0.double().clone()), torch.nn.Parameter(p0.clone())
    o64, o32 = torch.optim.Adam([p64], lr=1e-2, weight_decay=1e-2), torch.optim.Adam([p32], lr=1e-2, weight_decay=1e-2)
    pg, mg, vg = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (10.0 ** (step - 2))
        p64.grad, p32.grad = gr.double(), gr.clone()
        o64.step(); o32.step()
        gg = gr.to(DEV)
        H.check(lib.lt_adam_step(pg.data_ptr(), gg.data_ptr(), mg.data_ptr(), vg.data_ptr(), n, 1e-2, 0.9, 0.999, 1e-8, 1e-2, step, _st()), "lt_adam_step")
    torch.cuda.synchronize()
    _adam_gate("trk/adam single n=%d wd=1e-2" % n, pg, mg, vg, p64, p32, o64.state[p64])
