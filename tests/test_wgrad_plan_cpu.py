"""CPU: which weight-gradient kernel, slab layout and grid every direct test case gets -- asked of the library (lt_conv_wgrad_plan /
lt_conv_wgrad_bf16_plan: host only, the entry points launch from the same functions), not restated here.

  * every case of test_gpu_wgrad_kernels.py reaches the branch its comment names (EXPECT and the assertions below);
  * the union of test_gpu_train.W16_CASES, test_gpu_train.CONV_CASES at the tape tests' N = 3 and the tables of test_gpu_wgrad_kernels.py reaches
    every item of CHECKLIST: each kernel, several units per slab in each LDS kernel, ragged and crossing slabs, and for each generic kernel
    family one slab / a few / 8 and more with the XCD remap / several without it / an empty trailing slab;
  * the case builders of test_gpu_wgrad_kernels.py meet the exactness condition (they assert it while they compute the reference).

A retuned planner (wgrad_plan, plan16, plan16u, slab_plan, the routes) that moves a case to another branch fails here with the case's name:
move the case, not the expectation."""
import pytest

import lt_hip as H
import lt_train
import test_gpu_train as T
import test_gpu_wgrad_kernels as WK

FP32, BF16, NHWC = WK.FP32, WK.BF16, WK.NHWC
G_, B3, B2, PW, S7 = WK.G_, WK.B3, WK.B2, WK.PW, WK.S7


class TapeGeom:
    """A CONV_CASES layer as TrainTape asks for its weight gradient (lt_train.wgrad_geometry), with the interface plan_facts wants of a Geom."""

    def __init__(self, case, N=3):
        nd, Cin, Cout, k, s, p, tr, sp = case
        sp3 = ((1,) + tuple(sp)) if nd == 2 else tuple(sp)
        if tr:
            osp = tuple(2 * v for v in sp)
        else:
            osp = tuple((v + 2 * p - k) // s + 1 for v in sp)
        osp3 = ((1,) + osp) if nd == 2 else osp
        w_shape = ((Cin, Cout) if tr else (Cout, Cin)) + (k,) * nd
        self.w = lt_train.wgrad_geometry((N,) + sp3 + (Cin,), (N,) + osp3 + (Cout,), w_shape, s, p, tr)
        self.N, self.G, self.rows = self.w.n_img, (self.w.n_img + 7) // 8, self.w.wrows

    def plan(self, entry):
        w = self.w
        return H.wgrad_plan(entry, w.n_img, *w.gath_dims, w.gath_ch, *w.rows_dims, w.st3, w.pd3, w.rows_ch, w.rows_ld, w.cop, w.kp, w.ntaps, ldx=w.gath_ld)


def _tables():
    """(name, geometry) of every direct weight-gradient case of the suite."""
    out = [("W16_CASES/" + WK.case_id(c), WK.Geom(c)) for c in T.W16_CASES]
    out += [("CONV_CASES/nd%d_%dto%d_k%ds%dp%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_T" if c[6] else ""), TapeGeom(c)) for c in T.CONV_CASES]
    out += [("SLAB_CASES/" + WK.case_id(c), WK.Geom(c)) for c in WK.SLAB_CASES]
    out += [("ACC_CASES/%s%s" % (WK.case_id(c), "" if cop is None else "/cop%d" % cop), WK.Geom(c, cop)) for c, cop in WK.ACC_CASES]
    out += [("LD_CASES/" + WK.case_id(c), WK.Geom(c, None, c[3] + WK.LD_PAD, None if c[4] == WK.K3 else c[2] + WK.LD_PAD)) for c in WK.LD_CASES]
    out += [("NS3_CASES/" + WK.case_id(c), WK.Geom(c)) for c in WK.NS3_CASES]
    return out


def test_the_query_refuses_what_the_entry_points_refuse():
    ok = WK.Geom((3, (1, 8, 8), 32, 64, WK.K33, 1, 1))
    assert all(ok.plan(e) is not None for e in WK.ENTRIES)
    assert WK.Geom((3, (1, 8, 8), 24, 64, WK.K33, 1, 1)).plan(FP32) is None                      # Cin no power of two
    assert WK.Geom((3, (1, 8, 8), 32, 64, WK.K33, 1, 1), None, 48).plan(BF16) is None           # ldy < Cout
    assert WK.Geom((2, (4, 4, 8), 32, 17, WK.K1, 1, 0)).plan(NHWC) is None                       # 17 joints: lt_conv_wgrad_bf16_nhwc_ok says 0
    assert WK.Geom((2, (4, 4, 8), 32, 17, WK.K1, 1, 0)).plan(BF16) is not None


@pytest.mark.parametrize("i", range(len(WK.SLAB_CASES)), ids=[WK.case_id(c) for c in WK.SLAB_CASES])
def test_slab_cases_reach_the_branch_their_comment_names(i):
    g = WK.Geom(WK.SLAB_CASES[i])
    for entry, want in WK.EXPECT[i].items():
        got = WK.plan_facts(g, entry)
        if want is None:
            assert got is None, (entry, got)
            continue
        assert got is not None, entry
        for key, v in want.items():
            assert got[key] == v, "%s %s: %s = %r, the case is there for %r -- whole answer %r" % (WK.case_id(WK.SLAB_CASES[i]), entry, key, got[key], v, got)


def test_accumulate_padded_and_ns3_cases_reach_their_branches():
    acc = [(WK.plan_facts(WK.Geom(c, cop), FP32), WK.plan_facts(WK.Geom(c, cop), BF16), WK.plan_facts(WK.Geom(c, cop), NHWC)) for c, cop in WK.ACC_CASES]
    one = lambda f: f["family"] == G_ and f["slabs"] == 1
    many = lambda f: f["family"] == G_ and f["slabs"] > 1
    assert all(one(f) for f in acc[0])                                                     # direct_acc in all three generic kernels
    assert acc[1][0]["family"] == PW and one(acc[1][1]) and one(acc[1][2])
    assert many(acc[2][0]) and one(acc[2][1]) and one(acc[2][2])
    assert {acc[0][1]["variant"], acc[1][1]["variant"], acc[2][1]["variant"]} >= {1} and {acc[0][2]["variant"], acc[2][2]["variant"]} == {0, 1}
    assert many(acc[3][0]) and many(acc[3][1])                                             # the reduce's accumulate branch behind each generic kernel ...
    assert many(acc[4][2]) and many(acc[4][0]) and many(acc[4][1])
    assert [f["family"] for f in acc[5]] == [B3, B3, B3] and acc[5][1]["variant"] == 32   # ... and behind each LDS kernel
    assert acc[6][1]["family"] == B3 and acc[6][1]["variant"] == 16
    assert acc[7][1]["family"] == S7 and acc[8][0]["family"] == S7
    assert acc[9][0]["family"] == B2 and acc[10][0]["family"] == B2 and WK.ACC_CASES[10][1] > WK.ACC_CASES[10][0][3]
    ld = []
    for c in WK.LD_CASES:
        brick = c[4] == WK.K3
        ld.append((WK.plan_facts(WK.Geom(c, None, c[3] + WK.LD_PAD), FP32), WK.plan_facts(WK.Geom(c, None, c[3] + WK.LD_PAD), BF16),
                   WK.plan_facts(WK.Geom(c, None, c[3] + WK.LD_PAD, None if brick else c[2] + WK.LD_PAD), NHWC)))
    assert [f["family"] for f in ld[0]] == [G_] * 3 and [f["variant"] for f in ld[0]] == [0, 0, 1]
    assert [f["family"] for f in ld[1]] == [G_] * 3 and [f["variant"] for f in ld[1]] == [1, 1, 0]
    assert WK.LD_CASES[0][3] < 64 and WK.LD_CASES[1][3] % 128                              # Cout inside the tile's rows: the mask is what keeps the NaN out
    assert ld[2][0]["family"] == PW
    assert [f["family"] for f in ld[3]] == [B3, B3, B3] and ld[3][1]["variant"] == 32
    assert ld[4][1]["family"] == B3 and ld[4][1]["variant"] == 16
    ns3 = [WK.plan_facts(WK.Geom(c), NHWC) for c in WK.NS3_CASES]
    assert all(f["family"] == G_ for f in ns3) and {f["variant"] for f in ns3} == {0, 1}
    assert any(f["steps"] % 3 for f in ns3) and ns3[0]["remap"]


def _lds(entry, family, variant=None, per=2):
    return lambda e, f: e == entry and f["family"] == family and (variant is None or f["variant"] == variant) and f["per"] >= per


def _gen(entry, pred):
    return lambda e, f: e == entry and f["family"] == G_ and pred(f)


CHECKLIST = [("kernel %s generic, wave tile %d" % (e, v), lambda e_, f, e=e, v=v: e_ == e and f["family"] == G_ and f["variant"] == v)
             for e, vs in ((FP32, (0, 1, 2)), (BF16, (0, 1, 2)), (NHWC, (0, 1))) for v in vs]
CHECKLIST += [
    ("kernel fp32 conv3d_wgrad_brick_kernel", _lds(FP32, B3, per=1)), ("kernel fp32 conv2d_wgrad_brick_kernel", _lds(FP32, B2, per=1)),
    ("kernel fp32 wgrad_pw_kernel", _lds(FP32, PW, per=1)), ("kernel fp32 conv3d_wgrad_k7_kernel", _lds(FP32, S7, per=1)),
    ("kernel bf16 conv3d_wgrad16_brick_kernel<32>", _lds(BF16, B3, 32, 1)), ("kernel bf16 conv3d_wgrad16_brick_kernel<16>", _lds(BF16, B3, 16, 1)),
    ("kernel bf16 conv3d_wgrad16_k7_kernel", _lds(BF16, S7, per=1)), ("kernel nhwc conv3d_wgrad16_brick_u_kernel", _lds(NHWC, B3, 32, 1)),
    ("fp32 brick-3D: >= 2 bricks per slab", _lds(FP32, B3)), ("fp32 brick-2D: >= 2 bricks per slab", _lds(FP32, B2)),
    ("fp32 pointwise: >= 2 chunks per slab", _lds(FP32, PW)), ("fp32 7^3: >= 2 bricks per slab", _lds(FP32, S7)),
    ("bf16 brick<32>: >= 3 bricks per slab", _lds(BF16, B3, 32, 3)), ("bf16 brick<16>: >= 3 bricks per slab", _lds(BF16, B3, 16, 3)),
    ("nhwc brick-u: >= 3 bricks per slab", _lds(NHWC, B3, 32, 3)), ("bf16 7^3: >= 3 bricks per slab", _lds(BF16, S7, per=3)),
    ("train.hip: ragged last slab in an LDS kernel", lambda e, f: e == FP32 and f["ragged"]),
    ("wgrad16.hip: ragged last slab in an LDS kernel", lambda e, f: e != FP32 and f["ragged"]),
    ("fp32: a slab across two images", lambda e, f: e == FP32 and f["crosses"]),
    ("bf16: a slab across two octet groups", lambda e, f: e != FP32 and f["crosses"]),
]
for e in (FP32, BF16, NHWC):
    CHECKLIST += [
        ("%s generic: S = 1" % e, _gen(e, lambda f: f["slabs"] == 1)),
        ("%s generic: 1 < S < 8" % e, _gen(e, lambda f: 1 < f["slabs"] < 8)),
        ("%s generic: S >= 8 with the XCD remap" % e, _gen(e, lambda f: f["slabs"] >= 8 and f["remap"])),
        ("%s generic: S > 1 without the XCD remap" % e, _gen(e, lambda f: f["slabs"] > 1 and not f["remap"])),
        ("%s generic: empty trailing slab" % e, _gen(e, lambda f: f["empty"])),
    ]
CHECKLIST += [("reduce: S >= 4, S % 4 != 0 (the loop of four slabs and its tail)", lambda e, f: f["slabs"] >= 4 and f["slabs"] % 4 != 0)]


def test_the_tables_reach_every_item_of_the_checklist():
    facts = [(name, e, WK.plan_facts(g, e)) for name, g in _tables() for e in WK.ENTRIES]
    facts = [(n, e, f) for n, e, f in facts if f is not None]
    missing = []
    for label, pred in CHECKLIST:
        hit = next(((n, e, f) for n, e, f in facts if pred(e, f)), None)
        print("%-62s %s" % (label, "-- NOT REACHED" if hit is None else "%s [%s] S=%d units=%d per=%d grid=%s" % (hit[0], hit[1], hit[2]["slabs"], hit[2]["units"], hit[2]["per"], hit[2]["grid"])))
        if hit is None:
            missing.append(label)
    assert not missing, "no direct weight-gradient case reaches: %s" % missing


@pytest.mark.parametrize("case", WK.all_cases(), ids=WK.case_id)
def test_wgrad_kernel_cases_meet_the_exactness_condition(case):
    """Builds the operands and the per-tap fp64 reference of a GPU case on the CPU; the builder asserts rows * 225 + 63 < 2^24."""
    S = WK.build(case)
    assert S.want.shape == (S.g.Cout, S.g.kp) and float(S.x.abs().max()) <= 15 and float(S.dy.abs().max()) <= 15


@pytest.mark.parametrize("case", [WK.ACC_CASES[2][0], WK.ACC_CASES[3][0], WK.ACC_CASES[6][0]], ids=WK.case_id)
def test_the_per_tap_reference_equals_autograd(case):
    """The reference of test_gpu_wgrad_kernels.py (one matrix product per tap) against the weight gradient torch's autograd gives for the same
    convolution in fp64: strided 7x7 and 3x3 layers and a 3^3 one."""
    import torch
    import torch.nn.functional as F
    S = WK.build(case)
    g = S.g
    w = torch.zeros(g.Cout, g.Cin, *g.ks, dtype=torch.float64, requires_grad=True)
    z = F.conv3d(S.x.double().permute(0, 4, 1, 2, 3), w, None, g.st3, g.pd)
    (z * S.dy.double().permute(0, 4, 1, 2, 3)).sum().backward()
    assert torch.equal(w.grad.permute(0, 2, 3, 4, 1).reshape(g.Cout, g.kp).float(), S.want)
