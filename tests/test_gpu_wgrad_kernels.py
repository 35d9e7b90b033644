"""GPU (-m gpu): every slab-loop branch of the weight-gradient kernels, BIT FOR BIT against an fp64 sum over the same index set.

The direct tests of test_gpu_exact.py / test_gpu_train.py give every LDS kernel exactly one brick (one 32-row chunk) per slab, never pass
``accumulate`` or a leading dimension wider than the channel count, and never switch the unpacked kernel to three register sets.  The tables
here are chosen with the plan query (lt_conv_wgrad_plan / lt_conv_wgrad_bf16_plan through lt_hip.wgrad_plan): SLAB_CASES walk several units
per workgroup -- the register prefetch of the bf16 brick kernels with its two barriers, ragged last slabs, slabs that cross an image or an
octet group -- and put the generic kernels on grids with the XCD remap, on 8 and more slabs and on empty trailing slabs; ACC_CASES add onto
a preset dw through the epilogue of a single-slab kernel and through the ordered reduce; LD_CASES pad every pixel of dY (and of X where
the entry point takes ``ldx``) with NaN channels that must never reach dw.  tests/test_wgrad_plan_cpu.py asks the query about every case
and fails, naming the case, when a retuned planner moves it off the branch its comment names.

Method of test_conv_wgrad_bit_exact: operands are integers in +-15 (exact in bf16), ``rows * 225`` (+ 63 for a preset dw) stays below 2^24,
so fp32 holds every partial sum exactly in any order and the gate is equality of bit patterns.  The reference is computed one tap at a
time (dy^T @ x shifted by the tap, fp64): the unfold matrix of the 7^3 cases would be a gigabyte."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact as X
import lt_engine as E
import lt_hip as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FP32, BF16, NHWC = H.WGRAD_F32, H.WGRAD_BF16, H.WGRAD_BF16_NHWC
ENTRIES = (FP32, BF16, NHWC)
K1, K33, K77, K3, K7 = (1, 1, 1), (1, 3, 3), (1, 7, 7), (3, 3, 3), (7, 7, 7)

# N, (D, H, W), Cin, Cout, taps per dimension, stride, pad -- the layout of test_gpu_train.W16_CASES.  What each case is there for is asserted
# per entry point by tests/test_wgrad_plan_cpu.py from the EXPECT table below (units = bricks / 32-row chunks / GEMM rows, per = units per slab).
SLAB_CASES = [
    (9, (2, 20, 16), 128, 128, K3, 1, 1),        # bf16 brick<32> and brick-u: 40 bricks, 3 per slab, ragged last slab, slabs across the two octet groups;
                                                 # fp32 brick-3D: 45 bricks, 3 per slab, slabs across images
    (3, (8, 12, 24), 16, 128, K3, 1, 1),         # bf16 brick<16>: 72 bricks, 2 per slab (one prefetch, no steady state)
    (3, (8, 12, 24), 16, 256, K3, 1, 1),         # bf16 brick<16>: 72 bricks, 3 per slab (a brick that is both written from registers and prefetched over)
    (3, (8, 12, 32), 32, 16, K7, 1, 3),          # fp32 7^3: 72 bricks, 2 per slab; bf16 7^3: 192 bricks, 3 per slab
    (10, (5, 8, 32), 32, 16, K7, 1, 3),          # bf16 7^3: 160 bricks, 3 per slab, ragged, across the octet groups; odd D: fp32 generic 32 x 256 tile, 64 slabs
    (3, (1, 24, 24), 256, 256, K33, 1, 1),       # fp32 brick-2D: 27 bricks, 2 per slab, ragged, two ci blocks; packed generic S = 8 on a remapped grid of
                                                 # 18 x 8; nhwc S = 3 on a remapped grid of 72 x 3
    (3, (1, 47, 47), 256, 256, K1, 1, 0),        # fp32 pointwise: 208 chunks, 2 per slab, a last chunk of 3 rows; packed generic S = 56; nhwc S = 32, empty trailing slab
    (16, (1, 20, 20), 64, 128, K33, 1, 1),       # packed and fp32 generic with empty trailing slabs; nhwc S = 8 on a remapped grid
]
ACC_CASES = [  # (case, cout_pad or None = lt_conv_cout_pad): accumulate = 1 through every kind of epilogue
    ((8, (1, 2, 1), 64, 128, K33, 1, 1), None),      # one slab in all three generic kernels: the kernel's own epilogue adds to dw
    ((13, (1, 5, 3), 128, 256, K1, 1, 0), None),     # one slab in both bf16 kernels (the other wave tiles); fp32: the pointwise LDS kernel + reduce
    ((16, (1, 6, 8), 8, 64, K77, 2, 3), None),       # one slab in both bf16 kernels (64 x 128 tiles); fp32 generic: 3 slabs + reduce
    ((3, (1, 12, 16), 32, 64, K33, 2, 1), None),     # packed generic: 3 slabs + reduce; fp32 generic: 2 slabs
    ((5, (4, 6, 8), 16, 32, K1, 1, 0), None),        # nhwc generic: 3 slabs + reduce; fp32 / packed: 8 slabs on a remapped grid
    ((9, (2, 4, 16), 64, 32, K3, 1, 1), None),       # fp32 brick-3D, bf16 brick<32>, brick-u
    ((4, (4, 2, 8), 16, 32, K3, 1, 1), None),        # bf16 brick<16>
    ((8, (3, 4, 8), 32, 16, K7, 1, 3), None),        # bf16 7^3
    ((3, (4, 4, 16), 32, 16, K7, 1, 3), None),       # fp32 7^3
    ((3, (1, 16, 8), 32, 64, K33, 1, 1), None),      # fp32 brick-2D
    ((3, (1, 16, 8), 32, 64, K33, 1, 1), 96),        # ... with cout_pad > Cout: the workspace is zeroed first (rows past Cout are not the kernel's)
]
LD_PAD = 8          # NaN channels behind every pixel: ldy = Cout + 8, ldx = Cin + 8
LD_CASES = [
    (5, (4, 6, 8), 16, 32, K1, 1, 0),            # generic: fp32 / packed 128 x 64 wave tile, nhwc 64 x 128 -- the padding lies INSIDE the tile's rows
    (3, (1, 12, 16), 32, 96, K33, 2, 1),         # generic: fp32 / packed 64 x 128 wave tile, nhwc 128 x 64; Cout = 96 of cout_pad = 128
    (11, (1, 9, 7), 64, 96, K1, 1, 0),           # fp32: the pointwise LDS kernel's own Cout mask
    (9, (2, 4, 16), 64, 32, K3, 1, 1),           # bricks: fp32, bf16 brick<32>, brick-u (ldx == Cin: the kernel's condition)
    (4, (4, 2, 8), 16, 32, K3, 1, 1),            # bf16 brick<16>
]
NS3_CASES = [  # LT_WGRAD16U_NS=3 in a child process: one case per tile orientation of the unpacked kernel
    (16, (1, 20, 20), 64, 128, K33, 1, 1),       # 128 x 64, 8 slabs on a remapped grid, 7 steps per wave (7 % 3 != 0: the loop runs past the rows)
    (24, (1, 12, 12), 256, 64, K1, 1, 0),        # 64 x 128, 6 slabs, 5 steps per wave
]

# What tests/test_wgrad_plan_cpu.py asserts of SLAB_CASES[i] per entry point (keys of lt_hip.wgrad_plan's answer; "per" = units_per_slab; ragged /
# crosses / empty / remap as computed by plan_facts below)
G_, B3, B2, PW, S7 = H.WGRAD_GENERIC, H.WGRAD_BRICK3D, H.WGRAD_BRICK2D, H.WGRAD_POINTWISE, H.WGRAD_K7
EXPECT = [
    {FP32: dict(family=B3, units=45, per=3, crosses=True), BF16: dict(family=B3, variant=32, units=40, per=3, ragged=True, crosses=True),
     NHWC: dict(family=B3, variant=32, units=40, per=3, ragged=True, crosses=True)},
    {BF16: dict(family=B3, variant=16, units=72, per=2), NHWC: None},
    {BF16: dict(family=B3, variant=16, units=72, per=3), NHWC: None},
    {FP32: dict(family=S7, units=72, per=2), BF16: dict(family=S7, units=192, per=3), NHWC: None},
    {FP32: dict(family=G_, variant=2, slabs=64, remap=True), BF16: dict(family=S7, units=160, per=3, ragged=True, crosses=True), NHWC: None},
    {FP32: dict(family=B2, units=27, per=2, ragged=True, grid=(8, 2, 14)), BF16: dict(family=G_, slabs=8, remap=True, grid=(18, 8, 1)),
     NHWC: dict(family=G_, variant=0, slabs=3, remap=True, grid=(72, 3, 1))},
    {FP32: dict(family=PW, units=208, per=2, rows_mod_32=3), BF16: dict(family=G_, slabs=56, remap=True), NHWC: dict(family=G_, variant=0, slabs=32, remap=True, empty=True)},
    {FP32: dict(family=G_, empty=True), BF16: dict(family=G_, empty=True), NHWC: dict(family=G_, variant=0, slabs=8, remap=True)},
]


def case_id(c):
    return "N%d_%s_%dto%d_k%s_s%d" % (c[0], "x".join(map(str, c[1])), c[2], c[3], "".join(map(str, c[4])), c[5])


class Geom:
    """The arguments N .. ntaps of the three entry points for a case of the tables (``cop``: cout_pad override)."""

    def __init__(self, case, cop=None, ldy=None, ldx=None):
        self.N, (self.D, self.Hh, self.W), self.Cin, self.Cout, self.ks, s, p = case
        ks = self.ks
        self.pd = tuple(p if k > 1 else 0 for k in ks)
        self.st3 = tuple(s if k > 1 else 1 for k in ks) if any(k > 1 for k in ks) else (1, 1, 1)
        self.osp = tuple((n + 2 * q - k) // t + 1 for n, q, k, t in zip((self.D, self.Hh, self.W), self.pd, ks, self.st3))
        self.ntaps = ks[0] * ks[1] * ks[2]
        self.cop, self.kp = cop or E.cout_pad_of(self.Cout), self.ntaps * self.Cin
        self.ldy, self.ldx = ldy or self.Cout, ldx or self.Cin
        self.px_out, self.px_in = int(np.prod(self.osp)), self.D * self.Hh * self.W
        self.rows, self.G = self.N * self.px_out, (self.N + 7) // 8

    def args(self, nhwc=False):
        return ((self.N, self.D, self.Hh, self.W, self.Cin) + ((self.ldx,) if nhwc else ()) +
                (*self.osp, H.i3(self.st3), H.i3(self.pd), self.Cout, self.ldy, self.cop, self.kp, self.ntaps))

    def plan(self, entry):
        return H.wgrad_plan(entry, self.N, self.D, self.Hh, self.W, self.Cin, *self.osp, self.st3, self.pd, self.Cout, self.ldy, self.cop, self.kp, self.ntaps, ldx=self.ldx)


def plan_facts(g, entry):
    """lt_hip.wgrad_plan's answer for Geom ``g`` as a dict, with what follows from it: ``ragged`` (the last slab of an LDS kernel holds fewer units),
    ``crosses`` (a slab of an LDS kernel holds units of two images -- fp32 -- or two octet groups -- bf16), ``empty`` (a generic kernel's last slab
    starts past the last row), ``steps`` (nhwc generic: loop steps of four octet rows of the first wave of slab 0).  None: the entry point refuses."""
    p = g.plan(entry)
    if p is None:
        return None
    f = dict(family=p.family, variant=p.variant, slabs=p.slabs, units=int(p.units), per=p.units_per_slab, grid=tuple(p.grid), remap=bool(p.xcd_remap))
    lds = p.family != H.WGRAD_GENERIC
    f["ragged"] = lds and p.units % p.units_per_slab != 0
    f["rows_mod_32"] = g.rows % 32          # pointwise: the last chunk of 32 rows is partly filled
    f["empty"] = (not lds) and (p.slabs - 1) * p.units_per_slab >= p.units
    f["crosses"] = False
    if lds and p.family != H.WGRAD_POINTWISE:          # bricks of one image (octet group) are consecutive
        per_image = p.units // (g.N if entry == FP32 else g.G)
        f["crosses"] = any(s * p.units_per_slab // per_image != (min(p.units, (s + 1) * p.units_per_slab) - 1) // per_image for s in range(p.slabs))
    if entry == NHWC and not lds:
        f["steps"] = (min(int(p.units), p.units_per_slab // 4) + 3) // 4
    return f


class Case:
    """dw[co, tap * Cin + ci] = sum over images and output pixels of dy[., co] * x[. * stride - pad + tap, ci] on integer operands in +-15, one fp64
    matrix product per tap.  ``bound``: rows * 225 + the largest preset dw of the accumulate tests, asserted to be exact in fp32."""

    def __init__(self, case):
        self.case = case
        g = self.g = Geom(case)
        self.name = "wgradk/" + case_id(case)
        gen = X.gen(sum((i + 1) * ord(ch) for i, ch in enumerate(self.name)) % 100003)
        self.x = X.ints((g.N, g.D, g.Hh, g.W, g.Cin), 15, gen)
        self.dy = X.ints((g.N,) + g.osp + (g.Cout,), 15, gen)
        self.base = X.ints((E.cout_pad_of(g.Cout) + 128, g.kp), 63, gen)          # the preset dw of the accumulate tests (rows for any cout_pad used)
        X.assert_exact(self.name, g.rows * 15.0 * 15.0 + 63.0, 1.0)
        xp = F.pad(self.x.double(), (0, 0, g.pd[2], g.pd[2], g.pd[1], g.pd[1], g.pd[0], g.pd[0]))
        dyt = self.dy.double().reshape(g.rows, g.Cout).t().contiguous()
        want = torch.empty(g.Cout, g.kp, dtype=torch.float64)
        (Do, Ho, Wo), (sd, sh, sw) = g.osp, g.st3
        t = 0
        for a in range(g.ks[0]):
            for b in range(g.ks[1]):
                for c in range(g.ks[2]):
                    xs = xp[:, a:a + (Do - 1) * sd + 1:sd, b:b + (Ho - 1) * sh + 1:sh, c:c + (Wo - 1) * sw + 1:sw]
                    want[:, t * g.Cin:(t + 1) * g.Cin] = dyt @ xs.reshape(g.rows, g.Cin)
                    t += 1
        assert float(want.abs().max()) > 0
        self.want = X.as_f32(want)


@functools.lru_cache(maxsize=None)
def build(case):
    return Case(case)


def all_cases():
    """Every case of the tables once (the CPU premise check of tests/test_wgrad_plan_cpu.py builds them without a GPU)."""
    seen = []
    for c in SLAB_CASES + [c for c, _ in ACC_CASES] + LD_CASES + NS3_CASES:
        if c not in seen:
            seen.append(c)
    return seen


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------
def _taps(ks):
    return torch.tensor([(a, b, c, 0) for a in range(ks[0]) for b in range(ks[1]) for c in range(ks[2])], dtype=torch.int32, device=DEV)


def _padded(t, pad):
    """``t`` with ``pad`` NaN channels behind every pixel."""
    if not pad:
        return t
    out = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), NAN)
    out[..., :t.shape[-1]] = t
    return out


def launch(entry, S, cop=None, pad=0, pad_x=0, dw0=None):
    """One call of ``entry`` on Case ``S``.  ``pad`` / ``pad_x``: NaN channels behind every pixel of dY (ldy = Cout + pad) / of X (lt_conv_wgrad_bf16_nhwc: ldx =
    Cin + pad_x; lt_pack_n8_bf16 drops them with ld = Cin + pad_x; lt_conv_wgrad has no ldx and gets the dense X).
    ``dw0``: accumulate = 1 onto a copy of it; None: accumulate = 0 into a dw filled with NaN.  The workspace has exactly the bytes the entry point's
    workspace function asks for.  Returns dw [cout_pad][k_pad] on the CPU, or None where lt_conv_wgrad_bf16_nhwc_ok refuses the shape."""
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = Geom(S.case, cop, S.g.Cout + pad, S.g.Cin + pad_x if entry == NHWC else None)
    if entry == NHWC and not lib.lt_conv_wgrad_bf16_nhwc_ok(*g.args(nhwc=True)):
        return None
    taps = _taps(g.ks)
    dw = torch.full((g.cop, g.kp), NAN, device=DEV) if dw0 is None else dw0[:g.cop].to(DEV).contiguous()
    acc = 0 if dw0 is None else 1
    dy, x = _padded(S.dy, pad).to(DEV), _padded(S.x, pad_x).to(DEV)
    if entry == FP32:
        ws = torch.empty(max(int(lib.lt_conv_wgrad_workspace(g.rows, g.cop, g.kp)), 16), dtype=torch.uint8, device=DEV)
        xd = S.x.to(DEV)          # lt_conv_wgrad has no ldx: x is dense
        H.check(lib.lt_conv_wgrad(dy.data_ptr(), xd.data_ptr(), taps.data_ptr(), dw.data_ptr(), *g.args(), acc, ws.data_ptr(), st), "lt_conv_wgrad")
    else:
        ws = torch.empty(max(int(lib.lt_conv_wgrad_bf16_workspace(g.G * g.px_out, g.cop, g.kp)), 16), dtype=torch.uint8, device=DEV)
        if entry == BF16:          # the pack keeps dY's padding (ldy of the packed operand = Cout + pad) and drops X's (the packed X is dense)
            pa = torch.empty(int(lib.lt_pack_n8_bf16_bytes(g.N, g.px_out, g.ldy)), dtype=torch.uint8, device=DEV)
            pb = torch.empty(int(lib.lt_pack_n8_bf16_bytes(g.N, g.px_in, g.Cin)), dtype=torch.uint8, device=DEV)
            H.check(lib.lt_pack_n8_bf16(dy.data_ptr(), pa.data_ptr(), g.N, g.px_out, g.ldy, g.ldy, st), "lt_pack_n8_bf16")
            H.check(lib.lt_pack_n8_bf16(x.data_ptr(), pb.data_ptr(), g.N, g.px_in, g.Cin, g.Cin + pad_x, st), "lt_pack_n8_bf16")
            H.check(lib.lt_conv_wgrad_bf16(pa.data_ptr(), pb.data_ptr(), taps.data_ptr(), dw.data_ptr(), *g.args(), acc, ws.data_ptr(), st), "lt_conv_wgrad_bf16")
        else:
            dy16, x16 = dy.bfloat16().contiguous(), x.bfloat16().contiguous()
            H.check(lib.lt_conv_wgrad_bf16_nhwc(dy16.data_ptr(), x16.data_ptr(), taps.data_ptr(), dw.data_ptr(), *g.args(nhwc=True), acc, ws.data_ptr(), st),
                    "lt_conv_wgrad_bf16_nhwc")
    torch.cuda.synchronize()
    return dw.cpu()


def compare(c, name, S, dw, base=None):
    """Rows [0, Cout) of ``dw`` against the reference (+ ``base``), bit for bit and free of NaN; rows [Cout, cout_pad): zeros, or ``base`` untouched."""
    Cout = S.g.Cout
    assert not torch.isnan(dw[:Cout]).any(), "%s: NaN left in rows [0, Cout) of dw" % name
    want = S.want if base is None else X.as_f32(S.want.double() + base[:Cout].double())
    c.bits("exact/%s" % name, dw[:Cout], want)
    if dw.shape[0] > Cout:
        c.bits("exact/%s/rows_past_Cout" % name, dw[Cout:], torch.zeros_like(dw[Cout:]) if base is None else base[Cout:dw.shape[0]])


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SLAB_CASES, ids=case_id)
def test_wgrad_slab_loops_bit_exact(case):
    """All three entry points on the SLAB_CASES: several bricks / chunks per workgroup, ragged and crossing slabs, remapped grids, empty trailing slabs."""
    S = build(case)
    with X.Collector() as c:
        for entry in ENTRIES:
            dw = launch(entry, S)
            if dw is not None:
                compare(c, "%s/%s" % (S.name, entry), S, dw)


@pytest.mark.parametrize("case,cop", ACC_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else "cop%s" % v)
def test_wgrad_accumulate_bit_exact(case, cop):
    """accumulate = 1 onto a dw preset to integers in +-63: base + dW bit for bit, through the epilogue of a single-slab generic kernel (direct_acc) and
    through the accumulate branch of the ordered reduce behind every LDS kernel; a cout_pad override runs on lt_conv_wgrad alone."""
    S = build(case)
    with X.Collector() as c:
        for entry in (ENTRIES if cop is None else (FP32,)):
            dw = launch(entry, S, cop=cop, dw0=S.base)
            if dw is not None:
                compare(c, "%s/%s/accumulate%s" % (S.name, entry, "" if cop is None else "/cop%d" % cop), S, dw, S.base)
        if cop is not None:          # the zeroed workspace without accumulate: rows past Cout come out zero
            compare(c, "%s/fp32/cop%d" % (S.name, cop), S, launch(FP32, S, cop=cop))


@pytest.mark.parametrize("case", LD_CASES, ids=case_id)
def test_wgrad_padded_rows_bit_exact(case):
    """ldy = Cout + 8 (and ldx = Cin + 8 where the entry point has one; the brick-u kernel wants ldx == Cin) with NaN in every padding channel: the
    same bits as the reference, i.e. as the unpadded call -- no padding lane reaches an MFMA operand."""
    S = build(case)
    with X.Collector() as c:
        for entry in ENTRIES:
            dw = launch(entry, S, pad=LD_PAD, pad_x=0 if case[4] == K3 else LD_PAD)
            if dw is not None:
                compare(c, "%s/%s/ld+%d" % (S.name, entry, LD_PAD), S, dw)


PACK_CASES = [  # N, P, C, source offset in floats: (vector kernel) | (scalar kernel: misaligned source) | (scalar kernel: C = 17)
    (11, 63, 64, 0), (11, 63, 64, 1), (11, 63, 17, 0),
]


@pytest.mark.parametrize("N,P,C,off", PACK_CASES)
def test_pack_n8_with_padded_rows(N, P, C, off):
    """lt_pack_n8_bf16 with ld = C + 8 and NaN in the padding, through the vector kernel (aligned source) and the scalar kernel (source one float off
    16 bytes; C = 17), and lt_pack_n8_from_bf16 with ld = C + 8: the octets of the bf16-rounded tensor, zeros for the images past N."""
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    ld, Gp = C + 8, (N + 7) // 8
    g = X.gen(N * 1000 + C + off)
    src = torch.randn(N, P, C, generator=g)
    flat = torch.full((N * P * ld + 4,), NAN, device=DEV)
    view = flat[off:off + N * P * ld].view(N, P, ld)
    view[..., :C] = src.to(DEV)
    assert view.data_ptr() % 16 == 4 * off
    want = torch.zeros(Gp * 8, P, C)
    want[:N] = src.bfloat16().float()
    want = want.reshape(Gp, 8, P, C).permute(0, 2, 3, 1).contiguous()          # [G][P][C][8]
    nbytes = int(lib.lt_pack_n8_bf16_bytes(N, P, C))
    assert nbytes == Gp * P * C * 16
    dst = torch.full((nbytes // 2,), NAN, dtype=torch.bfloat16, device=DEV)
    H.check(lib.lt_pack_n8_bf16(view.data_ptr(), dst.data_ptr(), N, P, C, ld, st), "lt_pack_n8_bf16")
    torch.cuda.synchronize()
    assert torch.equal(dst.float().cpu().reshape(Gp, P, C, 8), want)
    if C % 8 == 0 and off == 0:
        s16 = torch.full((N, P, ld), NAN, dtype=torch.bfloat16, device=DEV)
        s16[..., :C] = src.to(DEV).bfloat16()
        dst2 = torch.full((nbytes // 2,), NAN, dtype=torch.bfloat16, device=DEV)
        H.check(lib.lt_pack_n8_from_bf16(s16.data_ptr(), dst2.data_ptr(), N, P, C, ld, st), "lt_pack_n8_from_bf16")
        torch.cuda.synchronize()
        assert torch.equal(dst2.float().cpu().reshape(Gp, P, C, 8), want)


def _ns3_child(out_path):
    """Runs in the child process of test_wgrad16u_three_register_sets (LT_WGRAD16U_NS=3 in its environment): dW of the NS3_CASES into ``out_path``."""
    assert os.environ.get("LT_WGRAD16U_NS") == "3"
    out = {}
    for case in NS3_CASES:
        dw = launch(NHWC, build(case))
        assert dw is not None
        out[case_id(case)] = dw
    torch.save(out, out_path)


def test_wgrad16u_three_register_sets(tmp_path):
    """LT_WGRAD16U_NS=3 (read once per process, so a fresh child process): both tile orientations of conv_wgrad16u_kernel with three register sets in
    flight, one of them with a step count that is no multiple of 3, against the fp64 reference bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = str(tmp_path / "dw_ns3.pt")
    code = ("import sys, os\n"
            "for p in (%r, %r, %r):\n    sys.path.insert(0, p)\n"
            "import test_gpu_wgrad_kernels as WK\nWK._ns3_child(%r)\n") % (root, os.path.join(root, "learnable-triangulation-pytorch_amd"), os.path.join(root, "tests"), out_path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LT_WGRAD16U_NS="3", PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-1500:]
    got = torch.load(out_path)
    steps = []
    with X.Collector() as c:
        for case in NS3_CASES:
            S = build(case)
            steps.append(plan_facts(S.g, NHWC)["steps"])
            compare(c, "%s/nhwc/ns3" % S.name, S, got[case_id(case)])
    assert any(s % 3 for s in steps), steps
