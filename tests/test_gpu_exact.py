"""GPU (-m gpu): every MFMA convolution path BIT FOR BIT against torch on the CPU, on operands of a dyadic grid (tests/exact.py).

The tolerance tests of test_gpu_kernels.py / test_gpu_train.py round their own Gaussian operands and outputs to bf16, so their gates
(max 1.5e-2, rms 4.5e-3) accept a truncating store, a 16-bit partial sum, a rounding slipped into a fused seam, a weight element that is never
read.  Here the operands are small integers with power-of-two epilogue constants: every product and partial sum is exact in fp32 in any
order, the only rounding left is the documented RNE store, and the reference performs it on the exact value -- so the gate is equality of
bit patterns, at the shapes of the tolerance tests (their case tables and run helpers are imported, not copied) and with each path pinned
the way its tolerance test pins it: a forced tile id that errors when the kernel does not cover the shape, can_* plus len(plan.ops), the
LT_* switches.  Where AUTO's route cannot be observed every forcing the suite has is run.

Rounding points of the fused kernels (DESIGN.md "Rounding points"): lt_bottleneck_fwd and lt_expand_reduce_fwd round exactly where the
separate launches store a tensor; lt_bottleneck_ds_fwd, lt_conv_cat2_fwd and lt_conv_skip_fwd keep the branch that the separate launches
store in bf16 in fp32.  The reference follows each kernel, and fused == unfused is asserted bit for bit on operands whose branch is
bf16-representable, where both must agree.

Every case builder below is plain CPU code that asserts the exactness and sensitivity conditions while it computes the reference;
tests/test_exact_cpu.py runs the builders without a GPU (cropped for the largest volumes)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact as X
import lt_engine as E
import lt_hip as H
import test_gpu_kernels as K
import test_gpu_train as T
from gpu_util import from_cl, record, to_cl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
CROP = 12          # CPU-only runs of the builders crop every spatial extent of a large case to this (and N to 1)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(str(name))) % 100003


def _osp(sp, k, s, p, transposed):
    return tuple(2 * v for v in sp) if transposed else tuple((v + 2 * p - k) // s + 1 for v in sp)


class Layer:
    """Operands of one convolution layer and its exact reference under any epilogue (the convolution sums are computed once)."""

    def __init__(self, name, nd, N, cin, cout, k, s, p, sp, transposed=False, crop=False, xr=15, wr=15, x_relu=False, bias=True, bn=True, rr=255,
                 bn_kw=None):
        if crop:
            N, sp = 1, tuple(min(v, CROP) for v in sp)
        self.name, self.nd, self.s, self.p, self.tr, self.cout = name, nd, s, p, transposed, cout
        g = X.gen(_seed(name))
        self.x = X.ints((N, cin) + tuple(sp), xr, g, 0 if x_relu else None)
        self.w = X.ints(((cin, cout) if transposed else (cout, cin)) + (k,) * nd, wr, g)
        self.bias = X.ints((cout,), 63, g) if bias else None
        self.bn = X.dyadic_bn(cout, g, **(bn_kw or {}))[0] if bn else None
        self.res = X.ints((N, cout) + _osp(sp, k, s, p, transposed), rr, g)
        self.acc, self.bound = X.conv_sum(self.x, self.w, s, p, transposed, name)

    def want(self, relu=False, relu_pre=False, res=False, store="bf16", bias=True, bn=True, residual=None):
        """The stored tensor (fp32 view) of act((acc + bias) * scale + shift [+ res]): RNE once for a bf16 store, exact for an fp32 store."""
        r = residual if residual is not None else (self.res if res else None)
        v = X.epilogue(self.acc, self.bound, self.cout, self.bias if bias else None, self.bn if bn else None, relu, relu_pre, r, self.name)
        if store == "bf16":
            X.assert_sensitive(self.name, v)
            return X.rne_bf16(v)
        return X.as_f32(v)

    def run(self, dtype, tile, relu=False, relu_pre=False, res=False, bias=True, bn=True):
        return K.run_conv(self.x, self.w, self.bias if bias else None, self.bn if bn else None, self.s, self.p, dtype, tile, transposed=self.tr,
                          relu=relu, relu_pre=relu_pre, residual=self.res if res else None)


@functools.lru_cache(maxsize=4)
def layer(name, *a, **kw):
    return Layer(name, *a, **dict(kw))


def _dt(dname):
    return (F32, "f32") if dname == "f32" else (BF, "bf16")


# ======================================================================================================================================
# forward: generic tiles
def conv_case(case, crop=False):
    nd, N, cin, cout, k, s, p, sp = K.CONV_CASES[case]
    return layer("conv/" + case, nd, N, cin, cout, k, s, p, sp, crop=crop)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(K.CONV_CASES))
def test_generic_tiles_bit_exact(case, dname):
    """lt_conv_fwd on CONV_CASES x every id of _tiles_for (v1 and v2 ids, ``direct``, ``auto``), bias + folded BatchNorm + residual + ReLU,
    fp32 and bf16 plans.  The scalar ``direct`` kernel goes first: if it matches and an MFMA tile does not, it is the premise about MFMA
    accumulation (exact fp32 partial sums below 2^24) that failed, and the message says so."""
    L = conv_case(case)
    dtype, dn = _dt(dname)
    want = L.want(relu=True, res=True, store=dn)
    tiles = K._tiles_for(K.CONV_CASES[case][3])
    order = ["direct"] + [t for t in tiles if t != "direct"]
    with X.Collector() as c:
        direct_ok = True
        for tname in order:
            ok = c.bits("exact/conv/%s/%s/%s" % (case, dn, tname), L.run(dtype, K.TILES[tname], relu=True, res=True), want)
            if tname == "direct":
                direct_ok = ok
            elif not ok and direct_ok:
                c.failed.append("  (the scalar direct kernel matches: the MFMA tile %s does not accumulate these integer sums exactly, or reads / stores wrongly)" % tname)


def deconv_generic_case(which, crop=False):
    if which == "deconv2d":          # ConvTranspose2d 4x4 s2 p1 + BN + ReLU (the backbone's deconvolution head)
        return layer("deconv2d_generic", 2, 2, 64, 256, 4, 2, 1, (6, 7), transposed=True, crop=crop, bias=False)
    return layer("deconv3d_generic", 3, 1, 128, 64, 2, 2, 0, (4, 4, 4), transposed=True, crop=crop)          # ConvTranspose3d 2^3 s2 + BN + ReLU, then + skip (V2V)


DECONV_TILES = {"deconv2d": ("direct", "auto", "128x128", "64x64", "v2_128x128", "v2_64x64", "v2_256x32"),
                "deconv3d": ("direct", "auto", "128x64", "64x64", "v2_128x64", "v2_64x64", "v2_256x16")}


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["deconv2d", "deconv3d"])
def test_transposed_convs_generic_tiles_bit_exact(which, dname):
    """The stride-2 transposed convolutions as output-parity phases of the generic tiles (the tile ids of test_transposed_convs)."""
    L = deconv_generic_case(which)
    dtype, dn = _dt(dname)
    kw = dict(relu=True, bias=False) if which == "deconv2d" else dict(relu_pre=True, res=True)
    want = L.want(store=dn, **kw)
    with X.Collector() as c:
        for tname in DECONV_TILES[which]:
            c.bits("exact/%s/%s/%s" % (which, dn, tname), L.run(dtype, K.TILES[tname], **kw), want)


def stem_generic_case(crop=False):
    return layer("stem_generic", 2, 2, 3, 64, 7, 2, 3, (37, 41), crop=crop, bias=False)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_stem_conv_padded_channels_bit_exact(dname):
    """The 7x7 / stride-2 stem over 3 channels padded to one 16-byte vector per pixel (zero weights on the padding), generic tiles."""
    L = stem_generic_case()
    dtype, dn = _dt(dname)
    want = L.want(relu=True, bias=False, store=dn)
    with X.Collector() as c:
        for tname in ("direct", "auto", "128x64", "64x64", "v2_128x64", "v2_64x64", "v2_256x16"):
            out = K.run_conv(L.x, L.w, None, L.bn, 2, 3, dtype, K.TILES[tname], relu=True, cin_pad=E.min_cin_of(dtype))
            c.bits("exact/stem/%s/%s" % (dn, tname), out, want)


RES32_CASES = [(2, 64, 128, 3, 1, 1, False, (20, 24)), (3, 32, 17, 1, 1, 0, False, (4, 6, 8)), (2, 32, 64, 4, 2, 1, True, (6, 8)), (3, 32, 64, 3, 1, 1, False, (4, 8, 8))]


def res32_case(case, crop=False):
    nd, cin, cout, k, s_, p_, tr, sp = case
    return layer("res32/%s" % (case,), nd, 2, cin, cout, k, s_, p_, sp, transposed=tr, crop=crop, rr=100000, bias=False, bn=False)


@pytest.mark.parametrize("case", RES32_CASES, ids=lambda c: "nd%d_%dto%d_k%d%s" % (c[0], c[1], c[2], c[3], "_T" if c[6] else ""))
def test_fp32_residual_on_a_bf16_convolution_bit_exact(case):
    """LT_EPI_RES_F32 with LT_EPI_STORE_F32: bf16 operands, an fp32 residual that bf16 cannot represent (integers up to 100000) added in the
    epilogue, fp32 output -- the input-gradient accumulation of the mixed-precision training step.  No rounding anywhere."""
    L = res32_case(case)
    nd, tr = case[0], case[6]
    want = L.want(res=True, store="f32", bias=False, bn=False)
    st = torch.cuda.current_stream().cuda_stream
    with X.Collector() as c:
        for tile in ((0, 4, 14) if not tr else (0,)):
            b = E.PlanBuilder(DEV, BF, tile_override=tile)
            y = b.conv(E.Act(to_cl(L.x, None, BF)), L.w, None, None, stride=L.s, pad=L.p, transposed=tr, residual=E.Act(to_cl(L.res, None, F32)),
                       out_f32=True, residual_f32=True)
            b.finish().run_eager(st); torch.cuda.synchronize()
            c.bits("exact/%s/tile%d" % (L.name, tile), from_cl(y.t, nd), want)


def logits_case(crop=False):
    return layer("logits_1x1x1_32_17", 3, 2, 32, 17, 1, 1, 0, (6, 7, 5), crop=crop, bn=False)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_fp32_store_of_a_ragged_width_bit_exact(dname):
    """1x1x1 32 -> 17 with an fp32 store from fp32 / bf16 compute (V2V's logits: a ragged channel count), the tile ids of
    test_conv_epilogue_variants.  (Its sigmoid head has no exact twin: expf is not exact.)"""
    L = logits_case()
    dtype, dn = _dt(dname)
    want = L.want(store="f32", bn=False)
    st = torch.cuda.current_stream().cuda_stream
    with X.Collector() as c:
        for tile in (0, 4, 14, 3, 13):
            b = E.PlanBuilder(DEV, dtype, tile_override=tile)
            y = b.conv(E.Act(to_cl(L.x, None, dtype)), L.w, L.bias, None, out_f32=True)
            b.finish().run_eager(st); torch.cuda.synchronize()
            assert y.t.dtype == F32
            c.bits("exact/logits_1x1x1_32_17/%s/tile%d" % (dn, tile), from_cl(y.t, 3), want)


LAYER3_SHAPES = [(64, 24), (128, 24), (32, 48)]


def layer3_case(N, H_, crop=False):
    return layer("layer3/%d_%d" % (N, H_), 2, N, 256, 256, 3, 1, 1, (H_, 24), crop=crop, bias=False)


@pytest.mark.parametrize("N,H_", LAYER3_SHAPES)
def test_layer3_3x3_256_default_dispatch_bit_exact(N, H_):
    """3x3 256 -> 256 on 24-wide maps through the DEFAULT dispatch (its route -- 2D halo kernel or 288-row tiles -- cannot be observed from here;
    test_halo2d_* and test_v5_* force each one): ReLU, residual + ReLU."""
    L = layer3_case(N, H_)
    with X.Collector() as c:
        c.bits("exact/layer3/N%d_H%d/relu" % (N, H_), L.run(BF, 0, relu=True, bias=False), L.want(relu=True, bias=False))
        c.bits("exact/layer3/N%d_H%d/res" % (N, H_), L.run(BF, 0, relu=True, res=True, bias=False), L.want(relu=True, res=True, bias=False))


# ======================================================================================================================================
# forward: 288-row family
def v3_case(case, crop=False):
    nd, N, cin, cout, k, s, p, sp, _ = K.V3_CASES[case]
    return layer("v3/" + case, nd, N, cin, cout, k, s, p, sp, crop=crop)


@pytest.mark.parametrize("case", list(K.V3_CASES))
def test_v3_288_bit_exact(case):
    """The 288-row / 3-stage kernels forced with LT_TILE3_288, AUTO (whose route cannot be observed from here), and the V2V-style epilogue
    (ReLU before the residual)."""
    L = v3_case(case)
    res = K.V3_CASES[case][8]
    with X.Collector() as c:
        c.bits("exact/v3/%s/forced" % case, L.run(BF, H.TILE3_288, relu=True, res=res), L.want(relu=True, res=res))
        c.bits("exact/v3/%s/auto" % case, L.run(BF, 0, relu=True, res=res), L.want(relu=True, res=res))
        c.bits("exact/v3/%s/relu_pre" % case, L.run(BF, H.TILE3_288, relu_pre=True, res=res), L.want(relu_pre=True, res=res))


def _v5_env(bsrc, monkeypatch):
    monkeypatch.setenv("LT_CONV_V5", "1")
    if bsrc == "lds":
        monkeypatch.setenv("LT_CONV_NO_V6", "1")
    else:
        monkeypatch.delenv("LT_CONV_NO_V6", raising=False)
    monkeypatch.setenv("LT_CONV_V6_BM144", "1" if bsrc == "registers_144" else "0")
    if bsrc == "v7_mfma32":
        monkeypatch.delenv("LT_CONV_NO_V7", raising=False)
    else:
        monkeypatch.setenv("LT_CONV_NO_V7", "1")


def v5_case(case, crop=False):
    nd, N, cin, cout, k, s, p, sp, _ = K.V5_CASES[case]
    return layer("v5/" + case, nd, N, cin, cout, k, s, p, sp, crop=crop)


@pytest.mark.parametrize("bsrc", ["registers", "registers_144", "lds", "v7_mfma32"])
@pytest.mark.parametrize("case", list(K.V5_CASES))
def test_v5_288x256_bit_exact(case, bsrc, monkeypatch):
    """The 288x256 tile forced with LT_CONV_V5=1: conv_igemm6 (weights as fragments from global memory; 288- and 144-row tiles), conv_igemm5
    (both operands staged, LT_CONV_NO_V6=1) and conv_igemm7 (32x32x16 MFMAs)."""
    _v5_env(bsrc, monkeypatch)
    L = v5_case(case)
    res = K.V5_CASES[case][8]
    with X.Collector() as c:
        c.bits("exact/v5/%s/%s/forced" % (bsrc, case), L.run(BF, H.TILE3_288, relu=True, res=res), L.want(relu=True, res=res))
        c.bits("exact/v5/%s/%s/relu_pre" % (bsrc, case), L.run(BF, H.TILE3_288, relu_pre=True, res=res), L.want(relu_pre=True, res=res))


def deconv4_case(crop=False):
    return layer("deconv4x4_288", 2, 3, 256, 256, 4, 2, 1, (12, 12), transposed=True, crop=crop, bias=False)


@pytest.mark.parametrize("bsrc", ["registers", "lds", "v7_mfma32"])
def test_deconv4x4_phases_bit_exact(bsrc, monkeypatch):
    """ConvTranspose2d 4x4 / stride 2 / pad 1 through the 288x256 kernels (one launch per output parity) and through the implicit GEMM
    that takes all four phases."""
    _v5_env(bsrc, monkeypatch)
    monkeypatch.delenv("LT_CONV_V6_BM144", raising=False)
    L = deconv4_case()
    want = L.want(relu=True, bias=False)
    with X.Collector() as c:
        c.bits("exact/deconv4x4_288x256/%s" % bsrc, L.run(BF, H.TILE3_288, relu=True, bias=False), want)
        c.bits("exact/deconv4x4_288x256/%s/igemm2" % bsrc, L.run(BF, K.TILES["v2_128x128"], relu=True, bias=False), want)


# ======================================================================================================================================
# forward: 3D halo kernels
def halo_case(case, crop=False):
    N, cin, cout, k, sp, _ = K.HALO_CASES[case]
    return layer("halo/" + case, 3, N, cin, cout, k, 1, k // 2, sp, crop=crop)


@pytest.mark.parametrize("case", list(K.HALO_CASES))
def test_halo3d_bit_exact(case, monkeypatch):
    """LDS-resident halo conv3d forced with LT_TILE_HALO and AUTO, bf16 and fp32, residual + ReLU; the persistent / XCD-pinned / 7^3 cases; the
    fp32 7^3 kernel against the generic tile (LT_HALO_NO_F7=1); two channel phases against one (LT_HALO_F3=1); the persistent kernels' epilogue
    without prefetched vectors (no residual, no ReLU), also run for the bf16 7^3 kernels."""
    L = halo_case(case)
    k7 = K.HALO_CASES[case][3] == 7          # the 7^3 loader-wave kernel: also affine only (test_conv3d_halo7_variants)
    with X.Collector() as c:
        for dname in K.HALO_CASES[case][5]:
            dtype, dn = _dt(dname)
            want = L.want(relu=True, res=True, store=dn)
            c.bits("exact/halo3d/%s/%s/forced" % (case, dn), L.run(dtype, H.TILE_HALO, relu=True, res=True), want)
            c.bits("exact/halo3d/%s/%s/auto" % (case, dn), L.run(dtype, 0, relu=True, res=True), want)
            if case.endswith("_f32_big"):
                monkeypatch.setenv("LT_HALO_NO_F7", "1")
                c.bits("exact/halo3d/%s/generic" % case, L.run(dtype, 0, relu=True, res=True), want)
                monkeypatch.delenv("LT_HALO_NO_F7")
            if case == "halo_3x3_32_32_f32_xcdpin":
                monkeypatch.setenv("LT_HALO_F3", "1")
                c.bits("exact/halo3d/%s/one_phase" % case, L.run(dtype, H.TILE_HALO, relu=True, res=True), want)
                monkeypatch.delenv("LT_HALO_F3")
            if "persist" in case or (k7 and dn == "bf16"):
                c.bits("exact/halo3d/%s/%s/nores" % (case, dn), L.run(dtype, H.TILE_HALO), L.want(store=dn))


D7_SHAPES = [(1, (8, 8, 16)), (3, (12, 16, 24))]


def d7_case(N, sp, crop=False):
    return layer("halo7_16_32/%d_%s" % (N, sp), 3, N, 16, 32, 7, 1, 3, sp, crop=crop, bias=False, bn=False)


@pytest.mark.parametrize("N,sp", D7_SHAPES)
def test_halo3d_7x7x7_16_to_32_bit_exact(N, sp, monkeypatch):
    """7^3 16 -> 32 (the input gradient of V2V's front layer) on the halo kernel (forced: errors if no halo kernel takes the shape), through
    AUTO, and on the generic tile (LT_HALO_NO_D7=1)."""
    L = d7_case(N, sp)
    nm = "exact/halo3d_7x7x7_16_32/N%d" % N
    with X.Collector() as c:
        c.bits(nm + "/res", L.run(BF, H.TILE_HALO, res=True, bias=False, bn=False), L.want(res=True, bias=False, bn=False))
        c.bits(nm + "/plain", L.run(BF, 0, bias=False, bn=False), L.want(bias=False, bn=False))
        monkeypatch.setenv("LT_HALO_NO_D7", "1")
        c.bits(nm + "/generic", L.run(BF, 0, bias=False, bn=False), L.want(bias=False, bn=False))


def col_case(case, crop=False):
    N, sp = K.COL_CASES[case]
    return layer("col/" + case, 3, N, 32, 32, 3, 1, 1, sp, crop=crop)


@pytest.mark.parametrize("col", ["1", "0"], ids=["column_walk", "persistent"])
@pytest.mark.parametrize("case", list(K.COL_CASES))
def test_halo3d_column_walk_bit_exact(case, col, monkeypatch):
    """conv3d_halo_col_kernel and the persistent kernel it replaces (LT_HALO_NO_COL=1) on >= 1024 tiles: residual + ReLU (forced), affine only
    and ReLU only (AUTO)."""
    if col == "0":
        monkeypatch.setenv("LT_HALO_NO_COL", "1")
    else:
        monkeypatch.delenv("LT_HALO_NO_COL", raising=False)
    L = col_case(case)
    with X.Collector() as c:
        c.bits("exact/halo3d_col=%s/%s/res" % (col, case), L.run(BF, H.TILE_HALO, relu=True, res=True), L.want(relu=True, res=True))
        c.bits("exact/halo3d_col=%s/%s/plain" % (col, case), L.run(BF, 0), L.want())
        c.bits("exact/halo3d_col=%s/%s/relu_only" % (col, case), L.run(BF, 0, relu=True, bias=False, bn=False), L.want(relu=True, bias=False, bn=False))


WREG_SHAPES = [(1, (8, 8, 16)), (3, (4, 16, 8)), (8, (8, 16, 16))]
WREG_WIDTHS = [(64, 64), (32, 64), (128, 128), (16, 32)]


def wreg_case(N, sp, cin, cout, crop=False):
    return layer("wreg/%d_%d/%d_%s" % (cin, cout, N, sp), 3, N, cin, cout, 3, 1, 1, sp, crop=crop)


@pytest.mark.parametrize("wsrc", ["registers", "lds"])
@pytest.mark.parametrize("cin,cout", WREG_WIDTHS)
@pytest.mark.parametrize("N,sp", WREG_SHAPES)
def test_halo3d_weight_source_bit_exact(N, sp, cin, cout, wsrc, monkeypatch):
    """conv3d_halo_wreg_kernel (weights as fragments from global memory) and the kernels it replaces (LT_HALO_NO_WREG=1: loader-wave halo kernel,
    implicit GEMM for 128 -> 128)."""
    if wsrc == "lds":
        monkeypatch.setenv("LT_HALO_NO_WREG", "1")
    else:
        monkeypatch.delenv("LT_HALO_NO_WREG", raising=False)
    L = wreg_case(N, sp, cin, cout)
    tile = H.TILE_HALO if (wsrc == "registers" or cin != 128) else 0
    name = "exact/halo3d_%d_%d/%s/N%d_%s" % (cin, cout, wsrc, N, "x".join(map(str, sp)))
    with X.Collector() as c:
        c.bits(name + "/res", L.run(BF, tile, relu=True, res=True), L.want(relu=True, res=True))
        c.bits(name + "/plain", L.run(BF, tile), L.want())


def colf32_case(crop=False):
    return layer("col_f32_store", 3, 4, 32, 32, 3, 1, 1, (16, 64, 64), crop=crop, bn=False)


def test_halo3d_column_walk_fp32_store_bit_exact(monkeypatch):
    """The column walk with LT_EPI_STORE_F32 (bf16 operands, fp32 output) and the implicit GEMM on the same operands (LT_HALO_NO_COL=1):
    no rounding at all, both equal the exact sums."""
    L = colf32_case()
    want = L.want(store="f32")
    st = torch.cuda.current_stream().cuda_stream

    def run():
        b = E.PlanBuilder(DEV, BF)
        y = b.conv(E.Act(to_cl(L.x, None, BF)), L.w, L.bias, None, stride=1, pad=1, out_f32=True)
        b.finish().run_eager(st); torch.cuda.synchronize()
        assert y.t.dtype == F32
        return from_cl(y.t, 3)
    with X.Collector() as c:
        monkeypatch.delenv("LT_HALO_NO_COL", raising=False)
        c.bits("exact/halo3d_col/fp32_store/column_walk", run(), want)
        monkeypatch.setenv("LT_HALO_NO_COL", "1")
        c.bits("exact/halo3d_col/fp32_store/implicit_gemm", run(), want)


SPLITK_SHAPES = [(1, (2, 2, 2)), (1, (8, 8, 8)), (5, (4, 4, 4)), (32, (2, 2, 2)), (32, (8, 8, 8))]


def splitk_case(N, sp, crop=False):
    return layer("splitk/%d_%s" % (N, sp), 3, N, 128, 128, 3, 1, 1, sp, crop=crop)


@pytest.mark.parametrize("N,sp", SPLITK_SHAPES)
def test_splitk_tiny_levels_bit_exact(N, sp, monkeypatch):
    """V2V's 3^3 128 -> 128 layers on <= 8^3 voxels: S tap-group phases with fp32 partial sums + lt_splitk_reduce (pinned by len(b.ops) == 2),
    the single launch (LT_CONV_NO_SPLITK=1), and the plain affine epilogue through the pair."""
    L = splitk_case(N, sp)
    monkeypatch.delenv("LT_CONV_NO_SPLITK", raising=False)
    b = E.PlanBuilder(DEV, BF)
    y = b.conv(E.Act(to_cl(L.x, None, BF)), L.w, L.bias, L.bn, stride=1, pad=1, relu=True, residual=E.Act(to_cl(L.res, None, BF)))
    assert len(b.ops) == 2 and "split-K" in b.ops[0][1]["label"], [m["label"] for _, m in b.ops]
    b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = "exact/splitk/N%d_%s" % (N, "x".join(map(str, sp)))
    with X.Collector() as c:
        c.bits(name + "/res_relu", from_cl(y.t, 3), L.want(relu=True, res=True))
        c.bits(name + "/plain", L.run(BF, 0), L.want())
        monkeypatch.setenv("LT_CONV_NO_SPLITK", "1")
        c.bits(name + "/single_launch", L.run(BF, 0, relu=True, res=True), L.want(relu=True, res=True))


# ---- lt_conv_skip_fwd ------------------------------------------------------------------------------------------------------------------
SKIP_SHAPES = [(4, 16, 64, 64), (16, 8, 64, 32), (1, 16, 128, 128)]          # the last: 1024 tiles in one sample (the tolerance test's 64 planes need a 4 x larger reference)
SKIP_BN = dict(a=(0, 0), k=(0, 1), beta=15, mean=7)          # scales 2^-1 .. 1


class SkipCase:
    """relu(bn2(conv3x3x3(y)) + bn_s(conv1x1x1_s(x))).  ``small``: the skip branch's operands are in [0, 3] x [-3, 3], so that the branch is
    bf16-representable (asserted) and the two launches, which store it in bf16, must agree with the fused kernel, which keeps it in fp32."""

    def __init__(self, N, D, Hh, W, small, crop=False):
        if crop:
            N, D, Hh, W = 1, min(D, CROP), min(Hh, CROP), min(W, CROP)
        self.name = "conv_skip/%dx%dx%dx%d/%s" % (N, D, Hh, W, "small" if small else "wide")
        g = X.gen(_seed(self.name))
        self.y = X.ints((N, 32, D, Hh, W), 15, g, 0)
        self.x = X.ints((N, 16, D, Hh, W), 3 if small else 15, g, 0)
        self.w = X.ints((32, 32, 3, 3, 3), 15, g)
        self.ws = X.ints((32, 16, 1, 1, 1), 3 if small else 15, g)
        self.bias, self.bs = X.ints((32,), 63, g), X.ints((32,), 15, g)
        self.bn, self.bns = X.dyadic_bn(32, g)[0], X.dyadic_bn(32, g, **SKIP_BN)[0]
        branch = X.conv_stage(X.Stage(self.x), self.ws, self.bs, self.bns, name=self.name + " skip branch")
        self.representable = bool(X.bf16_representable(branch.v).all())
        assert self.representable == small, "the skip branch is%s bf16-representable" % ("" if self.representable else " not")
        main = X.Stage(self.y)
        # fused: the branch joins the fp32 epilogue unrounded; two launches: the branch is stored (RNE) first
        sums = X.conv_sum(main.v, self.w, 1, 1, False, self.name)
        self.want_fused = X.store_bf16(X.conv_stage(main, self.w, self.bias, self.bn, 1, 1, relu=True, residual=branch, name=self.name, sums=sums), self.name).f32()
        rounded = X.store_bf16(branch, self.name + " skip branch", sensitive=False)
        self.want_two = X.store_bf16(X.conv_stage(main, self.w, self.bias, self.bn, 1, 1, relu=True, residual=rounded, name=self.name, sums=sums), self.name).f32()
        if small:
            assert torch.equal(self.want_fused, self.want_two)


@functools.lru_cache(maxsize=2)
def skip_case(N, D, Hh, W, small, crop=False):
    return SkipCase(N, D, Hh, W, small, crop)


SKIP_RUNS = [(shp, True) for shp in SKIP_SHAPES] + [(SKIP_SHAPES[0], False)]


@pytest.mark.parametrize("shape,small", SKIP_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("branch_representable" if v else "branch_wide"))
def test_conv_skip_bit_exact(shape, small, monkeypatch):
    """lt_conv_skip_fwd (pinned by can_conv_skip + len(plan.ops) == 1) against the reference that keeps the skip branch in fp32, and the two
    launches it replaces against the reference that rounds the branch where they store it.  With a bf16-representable branch all four are the
    same bits (fused == unfused); the wide branch (first shape only) shows that each path rounds where DESIGN.md says it does."""
    S = skip_case(*shape, small)
    ya, xa = E.Act(to_cl(S.y, None, BF)), E.Act(to_cl(S.x, None, BF))

    def run(fused):
        if fused:
            monkeypatch.delenv("LT_NO_CONV_SKIP", raising=False)
        else:
            monkeypatch.setenv("LT_NO_CONV_SKIP", "1")
        b = E.PlanBuilder(DEV, BF)
        assert b.can_conv_skip(ya.shape, S.w, xa.shape, S.ws) == fused
        if fused:
            z = b.conv(ya, S.w, S.bias, S.bn, pad=1, relu=True, skip=(xa, S.ws, S.bs, S.bns))
        else:
            r = b.conv(xa, S.ws, S.bs, S.bns)
            z = b.conv(ya, S.w, S.bias, S.bn, pad=1, relu=True, residual=r)
        plan = b.finish()
        assert len(plan.ops) == (1 if fused else 2)
        plan.run_eager(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return from_cl(z.t, 3)
    zf, z2 = run(True), run(False)
    with X.Collector() as c:
        c.bits("exact/%s/fused" % S.name, zf, S.want_fused)
        c.bits("exact/%s/two_launches" % S.name, z2, S.want_two)
        if small:
            c.bits("exact/%s/fused_vs_two_launches" % S.name, zf, z2)


# ======================================================================================================================================
# forward: 2D halo kernels
H2D_SHAPES = [(1, 8), (3, 24), (9, 16), (16, 24)]


def h2d_case(N, Hh, crop=False):
    return layer("h2d/%d_%d" % (N, Hh), 2, N, 256, 256, 3, 1, 1, (Hh, 24), crop=crop, x_relu=True, bias=False)


def _run_layout(L, monkeypatch, var, halo, layout_halo=2, nphase=1, **kw):
    if halo:
        monkeypatch.delenv(var, raising=False)
    else:
        monkeypatch.setenv(var, "1")
    b = E.PlanBuilder(DEV, BF)
    y = b.conv(E.Act(to_cl(L.x, None, BF)), L.w, None, L.bn, relu=True, **kw)
    assert all(b.last_info["desc"].phase[i].weight_frag_layout == (layout_halo if halo else 3) for i in range(nphase))          # the dispatcher follows the layout
    b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return from_cl(y.t, 2)


@pytest.mark.parametrize("th", ["8", "4"])
@pytest.mark.parametrize("N,Hh", H2D_SHAPES)
def test_halo2d_3x3_256_bit_exact(N, Hh, th, monkeypatch):
    """conv2d_halo_kernel (8 x 24 and 4 x 24 pixel tiles; pinned by the fragment layout the plan packs) and the implicit GEMM it replaces
    (LT_CONV_NO_H2D=1)."""
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    monkeypatch.setenv("LT_H2D_TH", th)
    L = h2d_case(N, Hh)
    want = L.want(relu=True, bias=False)
    name = "exact/halo2d/N%d_H%d/th%s" % (N, Hh, th)
    with X.Collector() as c:
        c.bits(name + "/halo", _run_layout(L, monkeypatch, "LT_CONV_NO_H2D", True, stride=1, pad=1), want)
        c.bits(name + "/implicit_gemm", _run_layout(L, monkeypatch, "LT_CONV_NO_H2D", False, stride=1, pad=1), want)


def h2d_ragged_case(crop=False):
    return layer("h2d/ragged", 2, 128, 256, 256, 3, 1, 1, (24, 24), crop=crop, x_relu=True, bias=False)


def test_halo2d_ragged_last_round_bit_exact(monkeypatch):
    """128 images of 24 x 24: 384 tiles = one round of 256 + a tail that runs as 256 half-height tiles in a second launch; the single launch
    (LT_H2D_NO_TAIL4=1); every image against the reference."""
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    monkeypatch.delenv("LT_H2D_TH", raising=False)
    L = h2d_ragged_case()
    want = L.want(relu=True, bias=False)
    with X.Collector() as c:
        monkeypatch.delenv("LT_H2D_NO_TAIL4", raising=False)
        c.bits("exact/halo2d/ragged/tail4", _run_layout(L, monkeypatch, "LT_CONV_NO_H2D", True, stride=1, pad=1), want)
        monkeypatch.setenv("LT_H2D_NO_TAIL4", "1")
        c.bits("exact/halo2d/ragged/one_launch", _run_layout(L, monkeypatch, "LT_CONV_NO_H2D", True, stride=1, pad=1), want)


DECONV_HALO_SHAPES = [(1, 8, 24), (3, 24, 24), (2, 16, 48), (5, 48, 48)]


def deconv_halo_case(N, Hh, W, crop=False):
    return layer("deconv_halo/%d_%d_%d" % (N, Hh, W), 2, N, 256, 256, 4, 2, 1, (Hh, W), transposed=True, crop=crop, x_relu=True, bias=False)


@pytest.mark.parametrize("N,Hh,W", DECONV_HALO_SHAPES)
def test_deconv4x4_halo_bit_exact(N, Hh, W, monkeypatch):
    """conv2d_halo_kernel<8, 4, 4>: the 4x4 / stride-2 transposed convolution as four output parities over one input halo, and the four
    implicit-GEMM launches it replaces (LT_DECONV_NO_H2D=1)."""
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    L = deconv_halo_case(N, Hh, W)
    want = L.want(relu=True, bias=False)
    name = "exact/deconv4x4_halo/N%d_%dx%d" % (N, Hh, W)
    with X.Collector() as c:
        c.bits(name + "/halo", _run_layout(L, monkeypatch, "LT_DECONV_NO_H2D", True, nphase=4, stride=2, pad=1, transposed=True), want)
        c.bits(name + "/implicit_gemm", _run_layout(L, monkeypatch, "LT_DECONV_NO_H2D", False, nphase=4, stride=2, pad=1, transposed=True), want)


# ======================================================================================================================================
# forward: single-tap layers
def pw_case(case, crop=False):
    N, cin, cout, sp, deconv = K.PW_CASES[case]
    return layer("pw/" + case, 3, N, cin, cout, 2 if deconv else 1, 2 if deconv else 1, 0, sp, transposed=deconv, crop=crop)


@pytest.mark.parametrize("stream", ["1", "0"], ids=["pw_stream", "igemm"])
@pytest.mark.parametrize("case", list(K.PW_CASES))
def test_conv_pw_bit_exact(case, stream, monkeypatch):
    """conv_pw (1x1x1 convolutions and 2x2x2 stride-2 deconvolutions of V2V) and the implicit GEMM it replaces (LT_CONV_NO_PW=1): affine only,
    residual + ReLU."""
    if stream == "0":
        monkeypatch.setenv("LT_CONV_NO_PW", "1")
    else:
        monkeypatch.delenv("LT_CONV_NO_PW", raising=False)
    L = pw_case(case)
    with X.Collector() as c:
        c.bits("exact/conv_pw=%s/%s/affine" % (stream, case), L.run(BF, 0), L.want())
        c.bits("exact/conv_pw=%s/%s/relu_res" % (stream, case), L.run(BF, 0, relu=True, res=True), L.want(relu=True, res=True))


PWCHAIN_CASES = [(3, 17), (2, 32), (1, 17), (3, 5)]
CHAIN_BN = dict(a=(-1, 0), k=(1, 2), beta=31, mean=15)          # scales 2^-1 .. 2^-3


class ChainCase:
    """lt_pwchain_fwd: every layer's output rounded to bf16 (RNE) except the fp32 last one."""

    def __init__(self, nlayers, J, crop=False):
        self.name = "pwchain/L%d_J%d" % (nlayers, J)
        g = X.gen(_seed(self.name))
        self.x = X.ints((2, 8, 8, 16, 32) if not crop else (1, 4, 4, 8, 32), 15, g)          # channels last
        self.layers, cin = [], 32
        cur = X.Stage(self.x.permute(0, 4, 1, 2, 3))
        for i, co in enumerate([32] * (nlayers - 1) + [J]):
            last = i + 1 == nlayers
            w = X.ints((co, cin, 1, 1, 1), 15 if i == 0 else 2, g)
            bias = X.ints((co,), 63, g)
            bn = None if last else X.dyadic_bn(co, g, **CHAIN_BN)[0]
            self.layers.append((w, bias, bn, not last))
            cur = X.conv_stage(cur, w, bias, bn, relu=not last, name="%s layer %d" % (self.name, i))
            if not last:
                cur = X.store_bf16(cur, "%s layer %d" % (self.name, i))
            cin = co
        self.want = cur.f32().permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=2)
def chain_case(nlayers, J, crop=False):
    return ChainCase(nlayers, J, crop)


@pytest.mark.parametrize("planar", [False, True], ids=["channels_last", "planar"])
@pytest.mark.parametrize("nlayers,J", PWCHAIN_CASES)
def test_pwchain_bit_exact(nlayers, J, planar):
    """lt_pwchain_fwd (pinned by can_chain_pointwise), channels-last rows and planar storage."""
    S = chain_case(nlayers, J)
    b = E.PlanBuilder(DEV, BF)
    xa = E.Act(S.x.to(DEV).to(BF))
    assert b.can_chain_pointwise(xa, S.layers)
    y = b.pwchain(xa, S.layers, planar=planar)
    b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert y.t.dtype == F32
    X.assert_bits_equal("exact/%s%s" % (S.name, "/planar" if planar else ""), y.t.cpu().contiguous(), S.want, channels_last=True)


# ======================================================================================================================================
# forward: fused kernels
BLOCK_BN = dict(a=(-1, 0), k=(1, 2), beta=31, mean=15)          # scales 2^-1 .. 2^-3
BNECK_SHAPES = [(256, 64, 1, 8, 16), (256, 64, 3, 24, 32), (512, 128, 1, 8, 16), (512, 128, 2, 16, 48), (256, 64, 9, 16, 16)]


class BneckCase:
    """The identity Bottleneck: t1 and t2 rounded (RNE) where the separate launches store them, which is where lt_bottleneck_fwd rounds too."""

    def __init__(self, C, P, N, Hh, W, crop=False):
        if crop:
            N, Hh, W = 1, min(Hh, CROP), min(W, CROP)
        self.name = "bneck/%d_%d/%dx%dx%d" % (C, P, N, Hh, W)
        g = X.gen(_seed(self.name))
        self.x = X.ints((N, C, Hh, W), 15, g)
        self.ws = [X.ints((P, C, 1, 1), 7, g), X.ints((P, P, 3, 3), 1, g), X.ints((C, P, 1, 1), 1, g)]
        self.bns = [X.dyadic_bn(P, g, **BLOCK_BN)[0], X.dyadic_bn(P, g, **BLOCK_BN)[0], X.dyadic_bn(C, g, **BLOCK_BN)[0]]
        xs = X.Stage(self.x)
        t1 = X.store_bf16(X.conv_stage(xs, self.ws[0], None, self.bns[0], relu=True, name=self.name + " t1"), self.name + " t1")
        t2 = X.store_bf16(X.conv_stage(t1, self.ws[1], None, self.bns[1], 1, 1, relu=True, name=self.name + " t2"), self.name + " t2")
        self.want = X.store_bf16(X.conv_stage(t2, self.ws[2], None, self.bns[2], relu=True, residual=xs, name=self.name + " y"), self.name + " y").f32()


@functools.lru_cache(maxsize=2)
def bneck_case(C, P, N, Hh, W, crop=False):
    return BneckCase(C, P, N, Hh, W, crop)


@pytest.mark.parametrize("C,P,N,Hh,W", BNECK_SHAPES)
def test_bottleneck_fused_bit_exact(C, P, N, Hh, W, monkeypatch):
    """lt_bottleneck_fwd (can_bottleneck + one op) and the three lt_conv_fwd launches it replaces (LT_NO_BNECK=1): both equal the reference,
    hence each other, bit for bit."""
    S = bneck_case(C, P, N, Hh, W)
    x_cl = to_cl(S.x, None, BF)
    y = from_cl(K._bneck_run(x_cl, S.ws, S.bns, True, monkeypatch), 2)
    y3 = from_cl(K._bneck_run(x_cl, S.ws, S.bns, False, monkeypatch), 2)
    with X.Collector() as c:
        c.bits("exact/%s/fused" % S.name, y, S.want)
        c.bits("exact/%s/three_launches" % S.name, y3, S.want)
        c.bits("exact/%s/fused_vs_three_launches" % S.name, y, y3)


BNECK_DS_SHAPES = [(1, 8, 16), (3, 24, 32), (2, 16, 48), (9, 16, 16), (4, 96, 96)]
DS_BN = dict(a=(0, 0), k=(0, 1), beta=15, mean=7)


class BneckDsCase:
    """The first Bottleneck of layer1 (64 -> 64 -> 256 with a downsample branch).  lt_bottleneck_ds_fwd adds the branch in fp32, the four
    launches store it in bf16 first; ``small`` makes the branch bf16-representable so that both must agree."""

    def __init__(self, N, Hh, W, small, crop=False):
        if crop:
            N, Hh, W = 1, min(Hh, CROP), min(W, CROP)
        self.name = "bneck_ds/%dx%dx%d/%s" % (N, Hh, W, "small" if small else "wide")
        g = X.gen(_seed(self.name))
        Cin, P, C_ = 64, 64, 256
        self.x = X.ints((N, Cin, Hh, W), 3 if small else 15, g, 0)
        self.ws = [X.ints((P, Cin, 1, 1), 15, g), X.ints((P, P, 3, 3), 1, g), X.ints((C_, P, 1, 1), 1, g)]
        self.wd = X.ints((C_, Cin, 1, 1), 1 if small else 15, g)
        self.bns = [X.dyadic_bn(P, g, **BLOCK_BN)[0], X.dyadic_bn(P, g, **BLOCK_BN)[0], X.dyadic_bn(C_, g, **BLOCK_BN)[0]]
        self.bnd = X.dyadic_bn(C_, g, **DS_BN)[0]
        xs = X.Stage(self.x)
        t1 = X.store_bf16(X.conv_stage(xs, self.ws[0], None, self.bns[0], relu=True, name=self.name + " t1"), self.name + " t1", sensitive=not small)
        t2 = X.store_bf16(X.conv_stage(t1, self.ws[1], None, self.bns[1], 1, 1, relu=True, name=self.name + " t2"), self.name + " t2", sensitive=not small)
        branch = X.conv_stage(xs, self.wd, None, self.bnd, name=self.name + " branch")
        assert bool(X.bf16_representable(branch.v).all()) == small
        sums = X.conv_sum(t2.v, self.ws[2], 1, 0, False, self.name + " y", gx=t2.grid)
        self.want_fused = X.store_bf16(X.conv_stage(t2, self.ws[2], None, self.bns[2], relu=True, residual=branch, name=self.name + " y", sums=sums), self.name + " y",
                                       sensitive=not small).f32()
        rb = X.store_bf16(branch, sensitive=False)
        self.want_four = X.store_bf16(X.conv_stage(t2, self.ws[2], None, self.bns[2], relu=True, residual=rb, name=self.name + " y", sums=sums), self.name + " y",
                                      sensitive=not small).f32()
        if small:
            assert torch.equal(self.want_fused, self.want_four)


@functools.lru_cache(maxsize=2)
def bneck_ds_case(N, Hh, W, small, crop=False):
    return BneckDsCase(N, Hh, W, small, crop)


BNECK_DS_RUNS = [(shp, False) for shp in BNECK_DS_SHAPES] + [(BNECK_DS_SHAPES[1], True)]


@pytest.mark.parametrize("shape,small", BNECK_DS_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("branch_representable" if v else "branch_wide"))
def test_bottleneck_ds_fused_bit_exact(shape, small, monkeypatch):
    """lt_bottleneck_ds_fwd (can_bottleneck_ds + one op) against the reference that adds the downsample branch unrounded, the four launches
    (LT_NO_BNECK_DS=1) against the reference that rounds it where they store it; with a bf16-representable branch (one several-tile shape) fused ==
    unfused bit for bit."""
    S = bneck_ds_case(*shape, small)
    x_cl = to_cl(S.x, None, BF)

    def run(fused):
        if fused:
            monkeypatch.delenv("LT_NO_BNECK_DS", raising=False)
        else:
            monkeypatch.setenv("LT_NO_BNECK_DS", "1")
        b = E.PlanBuilder(DEV, BF)
        xa = E.Act(x_cl)
        assert b.can_bottleneck_ds(xa, S.ws, (1, 1, 1), S.wd, 1) == fused
        if fused:
            y = b.bottleneck_ds(xa, S.ws, S.bns, S.wd, S.bnd)
        else:
            r = b.conv(xa, S.wd, None, S.bnd)
            t1 = b.conv(xa, S.ws[0], None, S.bns[0], relu=True)
            t2 = b.conv(t1, S.ws[1], None, S.bns[1], pad=1, relu=True)
            y = b.conv(t2, S.ws[2], None, S.bns[2], relu=True, residual=r)
        plan = b.finish()
        assert len(plan.ops) == (1 if fused else 4)
        plan.run_eager(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return from_cl(y.t, 2)
    yf, y4 = run(True), run(False)
    with X.Collector() as c:
        c.bits("exact/%s/fused" % S.name, yf, S.want_fused)
        c.bits("exact/%s/four_launches" % S.name, y4, S.want_four)
        if small:
            c.bits("exact/%s/fused_vs_four_launches" % S.name, yf, y4)


CAT2_SHAPES = [(2, 6, 10, 128, 256, 512, 2), (3, 24, 24, 256, 512, 1024, 2), (2, 12, 12, 512, 1024, 2048, 2), (1, 16, 32, 64, 64, 256, 1), (5, 13, 7, 128, 256, 512, 2)]
CAT2_BN = dict(a=(-1, 0), k=(0, 1), beta=15, mean=7)          # scales 2^-2 .. 1: folded into the weights (exact in bf16)


class Cat2Case:
    """relu(bn3(conv1x1(t2)) + bn_d(conv1x1_d(x), stride s)) as one pointwise convolution over [t2 | x]: both scales folded into the weights
    (a power of two times an integer: exact in bf16), the downsample branch never rounded; the two launches store the branch in bf16."""

    def __init__(self, N, Ho, Wo, P, Cin2, Cc, st, small, crop=False):
        if crop:
            N, Ho, Wo = 1, min(Ho, CROP), min(Wo, CROP)
        self.name = "conv_cat2/%dx%dx%d/%d+%d_%d/s%d/%s" % (N, Ho, Wo, P, Cin2, Cc, st, "small" if small else "wide")
        self.st = st
        g = X.gen(_seed(self.name))
        self.t2 = X.ints((N, P, Ho, Wo), 15, g, 0)
        self.x = X.ints((N, Cin2, Ho * st, Wo * st), 1 if small else 15, g, 0)
        self.w3, self.wd = X.ints((Cc, P, 1, 1), 15, g), X.ints((Cc, Cin2, 1, 1), 1 if small else 7, g)
        self.bn3, self.bnd = X.dyadic_bn(Cc, g, **CAT2_BN)[0], X.dyadic_bn(Cc, g, **CAT2_BN)[0]
        branch = X.conv_stage(X.Stage(self.x), self.wd, None, self.bnd, stride=st, name=self.name + " branch")
        assert bool(X.bf16_representable(branch.v).all()) == small
        main = X.Stage(self.t2)
        sums = X.conv_sum(main.v, self.w3, 1, 0, False, self.name)
        self.want_fused = X.store_bf16(X.conv_stage(main, self.w3, None, self.bn3, relu=True, residual=branch, name=self.name, sums=sums), self.name).f32()
        rb = X.store_bf16(branch, sensitive=False)
        self.want_two = X.store_bf16(X.conv_stage(main, self.w3, None, self.bn3, relu=True, residual=rb, name=self.name, sums=sums), self.name).f32()
        if small:
            assert torch.equal(self.want_fused, self.want_two)


@functools.lru_cache(maxsize=2)
def cat2_case(*a, **kw):
    return Cat2Case(*a, **kw)


CAT2_RUNS = [(shp, False) for shp in CAT2_SHAPES] + [(shp, True) for shp in CAT2_SHAPES[:2]]


@pytest.mark.parametrize("shape,small", CAT2_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("branch_representable" if v else "branch_wide"))
def test_conv_cat2_bit_exact(shape, small, monkeypatch):
    """lt_conv_cat2_fwd (can_conv_cat2 + one op) against the reference with the unrounded branch, the two launches against the reference that
    rounds it; with a bf16-representable branch (first two shapes) fused == unfused bit for bit."""
    monkeypatch.setenv("LT_CAT2_ANY_SIZE", "1")
    st = shape[6]
    S = cat2_case(*shape, small)
    ta, xa = E.Act(to_cl(S.t2, None, BF)), E.Act(to_cl(S.x, None, BF))

    def run(fused):
        b = E.PlanBuilder(DEV, BF)
        if fused:
            assert b.can_conv_cat2(ta.shape, S.w3, xa.shape, S.wd, st)
            y = b.conv_cat2(ta, S.w3, S.bn3, xa, S.wd, S.bnd, st)
        else:
            r = b.conv(xa, S.wd, None, S.bnd, stride=st)
            y = b.conv(ta, S.w3, None, S.bn3, relu=True, residual=r)
        plan = b.finish()
        assert len(plan.ops) == (1 if fused else 2)
        plan.run_eager(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return from_cl(y.t, 2)
    yf, y2 = run(True), run(False)
    with X.Collector() as c:
        c.bits("exact/%s/fused" % S.name, yf, S.want_fused)
        c.bits("exact/%s/two_launches" % S.name, y2, S.want_two)
        if small:
            c.bits("exact/%s/fused_vs_two_launches" % S.name, yf, y2)


XR_SHAPES = [(2, 6, 6), (2, 24, 24), (8, 24, 24), (3, 12, 20)]


class XrCase:
    """The seam between two identity blocks of layer3: y = relu(bn3(conv1x1(t2)) + res) rounded (RNE) where the expand stores it -- the reduce
    of the next block reads THAT -- and t1 = relu(bn1(conv1x1(y)))."""

    def __init__(self, N, Hh, W, crop=False):
        if crop:
            N, Hh, W = 1, min(Hh, CROP), min(W, CROP)
        self.name = "xr/%dx%dx%d" % (N, Hh, W)
        C_, P = 1024, 256
        g = X.gen(_seed(self.name))
        self.t2, self.res = X.ints((N, P, Hh, W), 15, g, 0), X.ints((N, C_, Hh, W), 255, g, 0)
        self.w3, self.w1 = X.ints((C_, P, 1, 1), 7, g), X.ints((P, C_, 1, 1), 1, g)
        self.bn3, self.bn1 = X.dyadic_bn(C_, g, **BLOCK_BN)[0], X.dyadic_bn(P, g, **BLOCK_BN)[0]
        y = X.store_bf16(X.conv_stage(X.Stage(self.t2), self.w3, None, self.bn3, relu=True, residual=X.Stage(self.res), name=self.name + " y"), self.name + " y")
        self.want_y = y.f32()
        self.want_t1 = X.store_bf16(X.conv_stage(y, self.w1, None, self.bn1, relu=True, name=self.name + " t1"), self.name + " t1").f32()


@functools.lru_cache(maxsize=2)
def xr_case(N, Hh, W, crop=False):
    return XrCase(N, Hh, W, crop)


@pytest.mark.parametrize("npb", ["3", "2", "1"])
@pytest.mark.parametrize("N,Hh,W", XR_SHAPES)
def test_expand_reduce_bit_exact(N, Hh, W, npb, monkeypatch):
    """lt_expand_reduce_fwd (can_expand_reduce + one op; tiles of 96 / 64 / 32 pixels by LT_XR_NPB) and the two launches it replaces
    (LT_NO_XR=1): y and t1 of both equal the reference, hence each other."""
    S = xr_case(N, Hh, W)
    t2_cl, res_cl = to_cl(S.t2, None, BF), to_cl(S.res, None, BF)
    monkeypatch.setenv("LT_XR_ANY_SIZE", "1")
    monkeypatch.setenv("LT_XR_NPB", npb)

    def run(fused):
        if fused:
            monkeypatch.delenv("LT_NO_XR", raising=False)
        else:
            monkeypatch.setenv("LT_NO_XR", "1")
        b = E.PlanBuilder(DEV, BF)
        ta, ra = E.Act(t2_cl), E.Act(res_cl)
        assert b.can_expand_reduce(ta, ra, S.w3, S.w1) == fused
        if fused:
            y, t1 = b.expand_reduce(ta, ra, S.w3, S.bn3, S.w1, S.bn1)
        else:
            y = b.conv(ta, S.w3, None, S.bn3, relu=True, residual=ra)
            t1 = b.conv(y, S.w1, None, S.bn1, relu=True)
        plan = b.finish()
        assert len(plan.ops) == (1 if fused else 2)
        plan.run_eager(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return from_cl(y.t, 2), from_cl(t1.t, 2)
    (y, t1), (y2, t12) = run(True), run(False)
    monkeypatch.delenv("LT_NO_XR", raising=False)
    nm = "exact/%s/npb%s" % (S.name, npb)
    with X.Collector() as c:
        c.bits(nm + "/y fused", y, S.want_y)
        c.bits(nm + "/t1 fused", t1, S.want_t1)
        c.bits(nm + "/y two_launches", y2, S.want_y)
        c.bits(nm + "/t1 two_launches", t12, S.want_t1)
        c.bits(nm + "/y fused_vs_two_launches", y, y2)
        c.bits(nm + "/t1 fused_vs_two_launches", t1, t12)


STEM_SHAPES = [(2, (64, 128), 3), (1, (100, 84), 3), (3, (37, 53), 1), (1, (384, 384), 3)]


class StemCase:
    """conv 7x7/2 + BatchNorm + ReLU rounded to bf16 (RNE) where the convolution launch stores it, then the 3x3/2 max pool (exact)."""

    def __init__(self, N, hw, cin, crop=False):
        if crop:
            N, hw = 1, tuple(min(v, 4 * CROP) for v in hw)
        self.name = "stem_pool/%dx%dx%d" % (N, hw[0], hw[1])
        g = X.gen(_seed(self.name))
        self.x, self.w = X.ints((N, cin) + tuple(hw), 15, g), X.ints((64, cin, 7, 7), 15, g)
        self.bn = X.dyadic_bn(64, g)[0]
        conv = X.store_bf16(X.conv_stage(X.Stage(self.x), self.w, None, self.bn, 2, 3, relu=True, name=self.name), self.name)
        self.want = F.max_pool2d(conv.f32(), 3, 2, 1)


@functools.lru_cache(maxsize=2)
def stem_case(N, hw, cin, crop=False):
    return StemCase(N, hw, cin, crop)


@pytest.mark.parametrize("N,hw,cin", STEM_SHAPES)
def test_stem_pool_bit_exact(N, hw, cin):
    """lt_stem_pool_fwd (can_stem_pool) against the reference, the two launches (conv, pool) it replaces against the reference, hence each
    other; and the same kernel reading the fp32 (N, 3, H, W) images in place."""
    S = stem_case(N, hw, cin)
    b = E.PlanBuilder(DEV, BF)
    xa = E.Act(to_cl(S.x, 8, BF))
    assert b.can_stem_pool(xa, S.w, 2, 3, (3, 2, 1))
    y = b.stem_pool(xa, S.w, S.bn)
    y2 = b.maxpool(b.conv(xa, S.w, None, S.bn, stride=2, pad=3, relu=True), 3, 2, 1, nd=2)
    b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with X.Collector() as c:
        c.bits("exact/%s/fused" % S.name, from_cl(y.t, 2), S.want)
        c.bits("exact/%s/two_launches" % S.name, from_cl(y2.t, 2), S.want)
        c.bits("exact/%s/fused_vs_two_launches" % S.name, from_cl(y.t, 2), from_cl(y2.t, 2))
        if cin == 3:
            b2 = E.PlanBuilder(DEV, BF)
            cell = {"ptr": None}
            y3 = b2.stem_pool(E.Act(torch.empty(N, 1, hw[0], hw[1], 8, dtype=BF, device=DEV)), S.w, S.bn, image_cell=cell)
            plan = b2.finish()
            xd = S.x.to(DEV).contiguous()
            cell["ptr"] = xd.data_ptr()
            plan.run(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            c.bits("exact/%s/fp32_images" % S.name, from_cl(y3.t, 2), S.want)


# ======================================================================================================================================
# forward: fp8 operands
class Fp8Case:
    """e4m3 operands: integers in +-7 with one +-7, so amax / 448 = 2^-6 and the quantised values are the integers times 64, exactly; the
    scale product 2^-12 rides in the BatchNorm slot and the integer bias in ``shift``: y = conv(x, w) + bias on integers."""

    def __init__(self, case, crop=False):
        nd, N, cin, cout, k, s_, p_, sp = case
        if crop:
            N, sp = 1, tuple(min(v, CROP) for v in sp)
        self.nd, self.cout, self.k, self.s, self.p, self.sp, self.cin = nd, cout, k, s_, p_, sp, cin
        self.name = "fp8/nd%d_%dto%d_k%d" % (nd, cin, cout, k)
        g = X.gen(_seed(self.name))
        self.x, self.w = X.fp8_ints((N, cin) + tuple(sp), g), X.fp8_ints((cout, cin) + (k,) * nd, g)
        self.bias = X.ints((cout,), 63, g)
        osp = _osp(sp, k, s_, p_, False)
        self.res32, self.res16 = X.ints((N, cout) + osp, 4095, g), X.ints((N, cout) + osp, 255, g)
        self.sx = self.sw = 2.0 ** -6
        self.wq = (self.w / self.sw).to(torch.float8_e4m3fn)
        assert torch.equal(self.wq.float(), self.w * 64.0)                                              # the host-side weight cast is lossless
        self.bn = (torch.full((cout,), self.sx * self.sw), self.bias, torch.zeros(cout), torch.ones(cout) - 1e-5)
        bi, sc, sh = X.fold(cout, None, self.bn)
        assert torch.equal(sc, torch.full((cout,), 2.0 ** -12, dtype=torch.float64)) and torch.equal(sh, self.bias.double())
        self.acc, self.bound = X.conv_sum(self.x * 64.0, self.w * 64.0, s_, p_, False, self.name, gx=64.0, gw=64.0)

    def want(self, res=None, relu=False, store="f32"):
        v = X.epilogue(self.acc, self.bound, self.cout, None, self.bn, relu, False, res, self.name, g_acc=4096.0)
        if store == "bf16":
            X.assert_sensitive(self.name, v)
            return X.rne_bf16(v)
        return X.as_f32(v)


@functools.lru_cache(maxsize=2)
def fp8_case(case, crop=False):
    return Fp8Case(case, crop)


@pytest.mark.parametrize("case", K.FP8_CASES, ids=lambda c: "nd%d_%dto%d_k%d" % (c[0], c[2], c[3], c[4]))
def test_conv_fp8_bit_exact(case):
    """lt_amax_f32 / lt_quant_fp8 (scale 2^-6 and bytes exact), then lt_conv_fwd(dtype = LT_FP8): generic tiles (AUTO and a forced v2 tile) with an
    fp32 store, without and with an fp32 residual + ReLU; a bf16 store with a bf16 residual; the halo kernel (forced) on the shapes it takes."""
    S = fp8_case(case)
    nd, cout = S.nd, S.cout
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    xcl = to_cl(S.x)
    amax = torch.zeros(2, dtype=F32, device=DEV)
    scales = torch.zeros(2, dtype=F32, device=DEV)
    x8 = torch.empty(xcl.shape, dtype=torch.uint8, device=DEV)
    H.check(lib.lt_amax_f32(xcl.data_ptr(), xcl.numel(), amax.data_ptr(), st), "lt_amax_f32")
    H.check(lib.lt_quant_fp8(xcl.data_ptr(), x8.data_ptr(), xcl.numel(), amax.data_ptr(), scales.data_ptr(), st), "lt_quant_fp8")
    torch.cuda.synchronize()
    assert float(amax[0]) == 7.0 and float(scales[0]) == 2.0 ** -6
    xq = (xcl.cpu() * 64.0).to(torch.float8_e4m3fn)
    assert torch.equal(xq.float(), xcl.cpu() * 64.0)
    nq = int((x8.cpu() != xq.view(torch.uint8)).sum())
    record("exact/%s/quantised bytes" % S.name, {"mismatching_words": nq, "words": x8.numel()})
    assert nq == 0
    # the same two kernels over the bf16 copy of the tensor (lt_amax_dt / lt_quant_fp8_dt: the 16-bit-activation training step)
    x16 = xcl.to(BF)
    amax.zero_(); scales.zero_()
    x8b = torch.empty_like(x8)
    H.check(lib.lt_amax_dt(H.LT_BF16, x16.data_ptr(), x16.numel(), amax.data_ptr(), st), "lt_amax_dt")
    H.check(lib.lt_quant_fp8_dt(H.LT_BF16, x16.data_ptr(), x8b.data_ptr(), x16.numel(), amax.data_ptr(), scales.data_ptr(), st), "lt_quant_fp8_dt")
    torch.cuda.synchronize()
    assert float(amax[0]) == 7.0 and float(scales[0]) == 2.0 ** -6
    nqb = int((x8b != x8).sum())
    record("exact/%s/quantised bytes from bf16" % S.name, {"mismatching_words": nqb, "words": x8.numel()})
    assert nqb == 0
    xa = E.Act(x8.view(torch.float8_e4m3fn))
    with X.Collector() as c:
        for with_res in (False, True):
            for tile in (0, K.TILES["v2_256x32"] if E.cout_pad_of(cout) == 32 else K.TILES["v2_128x64"]):
                b = E.PlanBuilder(DEV, torch.float8_e4m3fn, tile_override=tile)
                ra = E.Act(to_cl(S.res32)) if with_res else None
                y = b.conv(xa, S.wq.float(), None, S.bn, stride=S.s, pad=S.p, residual=ra, out_f32=True, residual_f32=with_res, relu=with_res)
                b.finish().run_eager(st); torch.cuda.synchronize()
                c.bits("exact/%s/tile%d%s" % (S.name, tile, "/res" if with_res else ""), from_cl(y.t, nd), S.want(S.res32 if with_res else None, with_res))
        b = E.PlanBuilder(DEV, torch.float8_e4m3fn)
        y = b.conv(xa, S.wq.float(), None, S.bn, stride=S.s, pad=S.p, residual=E.Act(to_cl(S.res16, None, BF)), relu=True)
        b.finish().run_eager(st); torch.cuda.synchronize()
        assert y.t.dtype == BF
        c.bits("exact/%s/bf16_store" % S.name, from_cl(y.t, nd), S.want(S.res16, True, "bf16"))
        sp = S.sp
        if nd == 3 and S.k == 3 and (S.cin, cout) in ((32, 32), (32, 64), (64, 64)) and sp[0] % 4 == 0 and sp[1] % 8 == 0 and sp[2] % 8 == 0:
            for with_res in (False, True):
                b = E.PlanBuilder(DEV, torch.float8_e4m3fn, tile_override=H.TILE_HALO)
                y = b.conv(xa, S.wq.float(), None, S.bn, stride=S.s, pad=S.p, residual=E.Act(to_cl(S.res16, None, BF)) if with_res else None, relu=with_res)
                b.finish().run_eager(st); torch.cuda.synchronize()
                c.bits("exact/%s/halo%s" % (S.name, "/res" if with_res else ""), from_cl(y.t, nd), S.want(S.res16 if with_res else None, with_res, "bf16"))


# ======================================================================================================================================
# training
class WgradCase:
    """dw[co, tap, ci] = sum over images and output pixels of dy[., co] * x[. * stride - pad + tap, ci]: an fp64 einsum per tap over integer
    operands (both bf16-exact), stored in fp32 -- no rounding anywhere."""

    def __init__(self, case):
        N, (D, Hh, W), Cin, Cout, ks, s, p = case
        self.name = "wgrad/N%d_%s_%dto%d_k%s_s%d" % (N, "x".join(map(str, (D, Hh, W))), Cin, Cout, "".join(map(str, ks)), s)
        g = X.gen(_seed(self.name))
        self.pd = tuple(p if k > 1 else 0 for k in ks)
        self.st3 = tuple(s if k > 1 else 1 for k in ks) if any(k > 1 for k in ks) else (1, 1, 1)
        self.osp = tuple((n + 2 * q - k) // t + 1 for n, q, k, t in zip((D, Hh, W), self.pd, ks, self.st3))
        self.x = X.ints((N, D, Hh, W, Cin), 15, g)
        self.dy = X.ints((N,) + self.osp + (Cout,), 15, g)
        rows = N * int(np.prod(self.osp))
        X.assert_exact(self.name, rows * 15.0 * 15.0, 1.0)
        xp = F.pad(self.x.double(), (0, 0, self.pd[2], self.pd[2], self.pd[1], self.pd[1], self.pd[0], self.pd[0]))
        win = xp.unfold(1, ks[0], self.st3[0]).unfold(2, ks[1], self.st3[1]).unfold(3, ks[2], self.st3[2])          # (N, Do, Ho, Wo, Cin, kd, kh, kw)
        assert tuple(win.shape[1:4]) == self.osp
        cols = win.permute(0, 1, 2, 3, 5, 6, 7, 4).reshape(rows, -1)                                             # [rows, ntaps * Cin]
        self.want = X.as_f32(torch.einsum("rk,rc->kc", self.dy.double().reshape(rows, Cout), cols))          # [Cout, ntaps * Cin]


@functools.lru_cache(maxsize=2)
def wgrad_case(case):
    return WgradCase(case)


@pytest.mark.parametrize("case", T.W16_CASES, ids=lambda c: "N%d_%s_%dto%d_k%s_s%d" % (c[0], "x".join(map(str, c[1])), c[2], c[3], "".join(map(str, c[4])), c[5]))
def test_conv_wgrad_bit_exact(case):
    """lt_conv_wgrad (fp32 MFMA), lt_pack_n8_bf16 + lt_conv_wgrad_bf16 (image-octet operands) and lt_conv_wgrad_bf16_nhwc (where it covers the
    shape) against the fp64 einsum -- a reference that is none of our kernels."""
    S = wgrad_case(case)
    lib = H.lib()
    st = torch.cuda.current_stream().cuda_stream
    N, (D, Hh, W), Cin, Cout, ks, s, p = case
    Do, Ho, Wo = S.osp
    st3, pd = S.st3, S.pd
    x, dy = S.x.to(DEV), S.dy.to(DEV)
    taps = torch.tensor([(a, b, c, 0) for a in range(ks[0]) for b in range(ks[1]) for c in range(ks[2])], dtype=torch.int32, device=DEV)
    ntaps = taps.shape[0]
    cop, kp = E.cout_pad_of(Cout), ntaps * Cin
    rows = N * Do * Ho * Wo
    with X.Collector() as c:
        dw = torch.zeros(cop, kp, device=DEV)
        ws = torch.empty(max(int(lib.lt_conv_wgrad_workspace(rows, cop, kp)), 16), dtype=torch.uint8, device=DEV)
        H.check(lib.lt_conv_wgrad(dy.data_ptr(), x.data_ptr(), taps.data_ptr(), dw.data_ptr(), N, D, Hh, W, Cin, Do, Ho, Wo, H.i3(st3), H.i3(pd), Cout, Cout, cop, kp,
                                  ntaps, 0, ws.data_ptr(), st), "lt_conv_wgrad")
        torch.cuda.synchronize()
        c.bits("exact/%s/fp32" % S.name, dw[:Cout].cpu(), S.want)
        pa = torch.empty(int(lib.lt_pack_n8_bf16_bytes(N, Do * Ho * Wo, Cout)), dtype=torch.uint8, device=DEV)
        pb = torch.empty(int(lib.lt_pack_n8_bf16_bytes(N, D * Hh * W, Cin)), dtype=torch.uint8, device=DEV)
        H.check(lib.lt_pack_n8_bf16(dy.data_ptr(), pa.data_ptr(), N, Do * Ho * Wo, Cout, Cout, st), "lt_pack_n8_bf16")
        H.check(lib.lt_pack_n8_bf16(x.data_ptr(), pb.data_ptr(), N, D * Hh * W, Cin, Cin, st), "lt_pack_n8_bf16")
        dw = torch.full((cop, kp), float("nan"), device=DEV)
        ws = torch.empty(max(int(lib.lt_conv_wgrad_bf16_workspace((N + 7) // 8 * Do * Ho * Wo, cop, kp)), 16), dtype=torch.uint8, device=DEV)
        H.check(lib.lt_conv_wgrad_bf16(pa.data_ptr(), pb.data_ptr(), taps.data_ptr(), dw.data_ptr(), N, D, Hh, W, Cin, Do, Ho, Wo, H.i3(st3), H.i3(pd), Cout, Cout,
                                       cop, kp, ntaps, 0, ws.data_ptr(), st), "lt_conv_wgrad_bf16")
        torch.cuda.synchronize()
        c.bits("exact/%s/bf16_packed" % S.name, dw[:Cout].cpu(), S.want)
        if lib.lt_conv_wgrad_bf16_nhwc_ok(N, D, Hh, W, Cin, Cin, Do, Ho, Wo, H.i3(st3), H.i3(pd), Cout, Cout, cop, kp, ntaps):
            x16, dy16 = x.bfloat16().contiguous(), dy.bfloat16().contiguous()
            dw = torch.full((cop, kp), float("nan"), device=DEV)
            H.check(lib.lt_conv_wgrad_bf16_nhwc(dy16.data_ptr(), x16.data_ptr(), taps.data_ptr(), dw.data_ptr(), N, D, Hh, W, Cin, Cin, Do, Ho, Wo, H.i3(st3), H.i3(pd),
                                                Cout, Cout, cop, kp, ntaps, 0, ws.data_ptr(), st), "lt_conv_wgrad_bf16_nhwc")
            torch.cuda.synchronize()
            c.bits("exact/%s/bf16_nhwc" % S.name, dw[:Cout].cpu(), S.want)


class TapeCase:
    """One bias-only layer through TrainTape: z = conv(x) + b, and for an integer upstream gradient dz: dx = conv^T(dz, w), dw, db = sum dz --
    all integer sums (fp64 autograd of torch on the CPU).  Training-mode BatchNorm is left out: its statistics divide."""

    def __init__(self, case, crop=False):
        nd, Cin, Cout, k, s, p, tr, sp = case
        self.name = "tape/nd%d_%dto%d_k%ds%dp%d%s" % (nd, Cin, Cout, k, s, p, "_T" if tr else "")
        g = X.gen(_seed(self.name))
        N = 3
        self.x = X.ints((N, Cin) + tuple(sp), 15, g)
        self.w = X.ints(((Cin, Cout) if tr else (Cout, Cin)) + (k,) * nd, 15, g)
        self.b = X.ints((Cout,), 63, g)
        conv = X._conv_fn(nd, tr)
        xd, wd, bd = (t.double().requires_grad_(True) for t in (self.x, self.w, self.b))
        z = conv(xd, wd, bd, stride=s, padding=p)
        self.dz = X.ints(z.shape, 15, g)
        (z * self.dz.double()).sum().backward()
        self.z, self.dx, self.dw, self.db = z.detach(), xd.grad, wd.grad, bd.grad
        kk = k ** nd
        X.assert_exact(self.name + " z", conv(self.x.abs().double(), self.w.abs().double(), self.b.abs().double(), stride=s, padding=p), 1.0)
        X.assert_exact(self.name + " dx", (Cout if not tr else Cin) * kk * 225.0, 1.0)
        X.assert_exact(self.name + " dw", float(max(self.z.numel() // Cout, self.x.numel() // Cin)) * 225.0, 1.0)

    @staticmethod
    def stored(v, dtype, name):
        if dtype == BF:
            X.assert_sensitive(name, v)
            return X.rne_bf16(v)
        return X.as_f32(v)


@functools.lru_cache(maxsize=2)
def tape_case(case, crop=False):
    return TapeCase(case, crop)


@pytest.mark.parametrize("mixed", [False, True, "act16"], ids=["fp32", "bf16mma", "act16"])
@pytest.mark.parametrize("case", T.CONV_CASES, ids=lambda c: "nd%d_%dto%d_k%ds%dp%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_T" if c[6] else ""))
def test_tape_layer_bias_only_bit_exact(case, mixed):
    """TrainTape in bias_only mode x {fp32, bf16 MFMA, bf16 activations}: z, dx, dw and db exactly (bf16 tensors: RNE of the exact value)."""
    import lt_train
    nd, Cin, Cout, k, s, p, tr, sp = case
    S = tape_case(case)
    wp, bp = torch.nn.Parameter(S.w.to(DEV)), torch.nn.Parameter(S.b.to(DEV))
    act16 = mixed == "act16"
    adt = BF if act16 else F32
    tape = lt_train.TrainTape(DEV, params=[wp, bp], mixed=bool(mixed), act16=act16)
    xa = E.Act(to_cl(S.x, None, adt))
    z = tape.conv(xa, wp, bp, None, stride=s, pad=p, transposed=tr, relu=False, residual=None)
    assert z.t.dtype == adt
    tape.seed(z, to_cl(S.dz, None, adt))
    pg = tape.run_backward()
    torch.cuda.synchronize()
    dx = tape.grad_of(xa)
    nm = "exact/%s/%s" % (S.name, "act16" if act16 else "bf16mma" if mixed else "fp32")
    with X.Collector() as c:
        c.bits(nm + "/z", from_cl(z.t, nd), S.stored(S.z, z.t.dtype, nm + "/z"))
        c.bits(nm + "/dx", from_cl(dx, nd), S.stored(S.dx, dx.dtype, nm + "/dx"))
        c.bits(nm + "/dw", pg[wp].float().cpu(), S.stored(S.dw, pg[wp].dtype, nm + "/dw"))
        c.bits(nm + "/db", pg[bp].float().cpu(), S.stored(S.db, pg[bp].dtype, nm + "/db"))


# ======================================================================================================================================
# every builder, for tests/test_exact_cpu.py: (name, thunk) -- the thunk computes the reference and thereby asserts both conditions
FULL = False          # True: nothing is cropped (a by-hand run of every builder at the GPU tests' own sizes)
BIG = 2.5e8          # multiply-adds above which the CPU-only run crops the case (the GPU tests always run it whole)


def _big():
    return 1e30 if FULL else BIG


def _macs(N, sp, cout, K_):
    return float(N) * float(np.prod(sp)) * cout * K_


def all_cases():
    out = []

    def add(name, thunk):
        out.append((name, thunk))

    def layer_wants(L, variants):
        for kw in variants:
            L.want(**kw)
    for case, (nd, N, cin, cout, k, s, p, sp) in K.CONV_CASES.items():
        add("conv/" + case, lambda case=case, crop=_macs(N, _osp(sp, k, s, p, False), cout, cin * k ** nd) > _big(): layer_wants(conv_case(case, crop), [dict(relu=True, res=True, store="bf16"), dict(relu=True, res=True, store="f32")]))
    for case, v in K.V3_CASES.items():
        crop = _macs(v[1], _osp(v[7], v[4], v[5], v[6], False), v[3], v[2] * v[4] ** v[0]) > _big()
        add("v3/" + case, lambda case=case, r=v[8], crop=crop: layer_wants(v3_case(case, crop), [dict(relu=True, res=r), dict(relu_pre=True, res=r)]))
    for case, v in K.V5_CASES.items():
        crop = _macs(v[1], _osp(v[7], v[4], v[5], v[6], False), v[3], v[2] * v[4] ** v[0]) > _big()
        add("v5/" + case, lambda case=case, r=v[8], crop=crop: layer_wants(v5_case(case, crop), [dict(relu=True, res=r), dict(relu_pre=True, res=r)]))
    for which in ("deconv2d", "deconv3d"):
        kw = dict(relu=True, bias=False) if which == "deconv2d" else dict(relu_pre=True, res=True)
        add("generic/" + which, lambda which=which, kw=kw: layer_wants(deconv_generic_case(which), [dict(store="bf16", **kw), dict(store="f32", **kw)]))
    add("generic/stem", lambda: layer_wants(stem_generic_case(), [dict(relu=True, bias=False, store="bf16"), dict(relu=True, bias=False, store="f32")]))
    for case in RES32_CASES:
        add("res32/%s" % (case,), lambda case=case: layer_wants(res32_case(case), [dict(res=True, store="f32", bias=False, bn=False)]))
    add("logits", lambda: layer_wants(logits_case(), [dict(store="f32", bn=False)]))
    for a in LAYER3_SHAPES:
        add("layer3/%s" % (a,), lambda a=a: layer_wants(layer3_case(*a, _big() < 1e30), [dict(relu=True, bias=False), dict(relu=True, res=True, bias=False)]))
    for a in D7_SHAPES:
        add("halo7_16_32/%s" % (a,), lambda a=a: layer_wants(d7_case(*a, _macs(a[0], a[1], 32, 16 * 343) > _big()), [dict(res=True, bias=False, bn=False), dict(bias=False, bn=False)]))
    add("deconv4x4_288", lambda: layer_wants(deconv4_case(_big() < 1e30), [dict(relu=True, bias=False)]))
    for case, (N, cin, cout, k, sp, dts) in K.HALO_CASES.items():
        crop = _macs(N, sp, cout, cin * k ** 3) > _big()
        add("halo/" + case, lambda case=case, crop=crop, dts=dts: layer_wants(halo_case(case, crop), [dict(relu=True, res=True, store=d) for d in dts] + [dict(store=dts[0])]))
    for case in K.COL_CASES:
        add("col/" + case, lambda case=case: layer_wants(col_case(case, _big() < 1e30), [dict(relu=True, res=True), dict(), dict(relu=True, bias=False, bn=False)]))
    for N, sp in WREG_SHAPES:
        for cin, cout in WREG_WIDTHS:
            crop = _macs(N, sp, cout, cin * 27) > _big()
            add("wreg/%d_%d/%d" % (cin, cout, N), lambda a=(N, sp, cin, cout, crop): layer_wants(wreg_case(*a), [dict(relu=True, res=True), dict()]))
    add("col_f32_store", lambda: layer_wants(colf32_case(_big() < 1e30), [dict(store="f32")]))
    for N, sp in SPLITK_SHAPES:
        crop = _macs(N, sp, 128, 128 * 27) > _big()
        add("splitk/%d_%s" % (N, sp), lambda a=(N, sp, crop): layer_wants(splitk_case(*a), [dict(relu=True, res=True), dict()]))
    for shp in SKIP_SHAPES:
        add("conv_skip/%s/small" % (shp,), lambda shp=shp: skip_case(*shp, True, _big() < 1e30))
    add("conv_skip/wide", lambda: skip_case(*SKIP_SHAPES[0], False, _big() < 1e30))
    for N, Hh in H2D_SHAPES:
        add("h2d/%d_%d" % (N, Hh), lambda a=(N, Hh): layer_wants(h2d_case(*a, _macs(a[0], (a[1], 24), 256, 2304) > _big()), [dict(relu=True, bias=False)]))
    add("h2d/ragged", lambda: layer_wants(h2d_ragged_case(_big() < 1e30), [dict(relu=True, bias=False)]))
    for a in DECONV_HALO_SHAPES:
        add("deconv_halo/%s" % (a,), lambda a=a: layer_wants(deconv_halo_case(*a, _macs(a[0], a[1:], 256, 4096) > _big()), [dict(relu=True, bias=False)]))
    for case in K.PW_CASES:
        add("pw/" + case, lambda case=case: layer_wants(pw_case(case), [dict(), dict(relu=True, res=True)]))
    for a in PWCHAIN_CASES:
        add("pwchain/%s" % (a,), lambda a=a: chain_case(*a))
    for a in BNECK_SHAPES:
        add("bneck/%s" % (a,), lambda a=a: bneck_case(*a, _macs(a[2], a[3:], a[1], 2 * a[0] + 9 * a[1]) > _big()))
    for a in BNECK_DS_SHAPES:
        add("bneck_ds/%s/wide" % (a,), lambda a=a: bneck_ds_case(*a, False, _macs(a[0], a[1:], 64, 64 + 576 + 512) > _big()))
    add("bneck_ds/small", lambda: bneck_ds_case(*BNECK_DS_SHAPES[1], True))
    for a in CAT2_SHAPES:
        add("cat2/%s/wide" % (a,), lambda a=a: cat2_case(*a, False, _macs(a[0], a[1:3], a[5], a[3] + a[4]) > _big()))
    for a in CAT2_SHAPES[:2]:
        add("cat2/%s/small" % (a,), lambda a=a: cat2_case(*a, True, _macs(a[0], a[1:3], a[5], a[3] + a[4]) > _big()))
    for a in XR_SHAPES:
        add("xr/%s" % (a,), lambda a=a: xr_case(*a, _macs(a[0], a[1:], 1024, 512) > _big()))
    for a in STEM_SHAPES:
        add("stem/%s" % (a,), lambda a=a: stem_case(*a, a[1][0] > 128 and _big() < 1e30))
    for case in K.FP8_CASES:
        crop = _macs(case[1], case[7], case[3], case[2] * case[4] ** case[0]) > _big()
        add("fp8/%s" % (case,), lambda a=(case, crop): [fp8_case(*a).want(), fp8_case(*a).want(fp8_case(*a).res32, True), fp8_case(*a).want(fp8_case(*a).res16, True, "bf16")])
    for case in T.W16_CASES:
        add("wgrad/%s" % (case,), lambda case=case: wgrad_case(case))
    for case in T.CONV_CASES:
        add("tape/%s" % (case,), lambda case=case: [TapeCase.stored(tape_case(case).z, BF, "z"), TapeCase.stored(tape_case(case).dx, BF, "dx")])
    return out
