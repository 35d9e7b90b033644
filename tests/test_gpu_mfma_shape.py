"""GPU (-m gpu): the two bf16 MFMA shapes, v_mfma_f32_16x16x32_bf16 and 32x32x16, of conv2d_halo_kernel (LT_H2D_MF32=1: 32x32x16) and of the 3x3x3
column walk conv3d_halo_col_kernel (LT_HALO_COL_MF32=1; K = 864, plus 16 for the computed skip residual), at the same tile per wave.

  1. each shape BIT FOR BIT against exact integer sums (the case builders of test_gpu_exact.py): the layout test -- a wrong lane <-> channel map,
     slot swizzle or weight-row choice is a wrong integer;
  2. shape against shape on Gaussian bf16 data: the shapes add a tap's 32 products in different orders, so the fp32 sums may differ in their last
     bits.  Each sum is within gamma = K 2^-24 sum |x| |w| of the exact one (K terms, fp32 unit roundoff 2^-24 per addition, first order) and each
     output is one bf16 rounding of its sum (2^-8 relative, two of them: 2^-7), hence
         |y16 - y32| <= 2^-7 max(|y16|, |y32|) + 2 gamma,
     gamma in fp64 on the bf16-rounded operands; K = 2304 for the 3x3, 1024 per parity of the 4x4.  No BatchNorm or bias in these runs, so the
     bound needs no scale; ReLU does not expand a difference.  The share of outputs that differ at all goes to the parity report;
  3. dispatch: the shape per instantiation with the switch unset and set, and layers outside the 2D-halo predicate untouched by the switch."""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact as X
import lt_engine as E
import lt_hip as H
import test_gpu_exact as XT
import test_gpu_kernels as K
from gpu_util import bf16_round, from_cl, record, to_cl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SWITCH = "LT_H2D_MF32"
H2D = [(1, 8), (3, 24), (9, 16)]
DECONV = [(1, 8, 24), (2, 16, 48)]
INSTANCES = [(8, 1), (4, 1), (8, 4)]          # (tile rows, phases) of conv2d_halo_kernel


def _shape(inst):
    return H.lib().lt_sel_halo2d_mfma(*inst)


def _set(monkeypatch, on):
    if on:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)


@pytest.mark.parametrize("th", ["8", "4"])
@pytest.mark.parametrize("N,Hh", H2D)
def test_halo2d_3x3_both_shapes_bit_exact(N, Hh, th, monkeypatch):
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    monkeypatch.setenv("LT_H2D_TH", th)
    L = XT.h2d_case(N, Hh)
    want = L.want(relu=True, bias=False)
    with X.Collector() as c:
        for on in (False, True):
            _set(monkeypatch, on)
            c.bits("exact/mfma_shape/halo2d/N%d_H%d/th%s/mfma%d" % (N, Hh, th, _shape((int(th), 1))),
                   XT._run_layout(L, monkeypatch, "LT_CONV_NO_H2D", True, stride=1, pad=1), want)


@pytest.mark.parametrize("N,Hh,W", DECONV)
def test_deconv4x4_both_shapes_bit_exact(N, Hh, W, monkeypatch):
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    L = XT.deconv_halo_case(N, Hh, W)
    want = L.want(relu=True, bias=False)
    with X.Collector() as c:
        for on in (False, True):
            _set(monkeypatch, on)
            c.bits("exact/mfma_shape/deconv4x4/N%d_%dx%d/mfma%d" % (N, Hh, W, _shape((8, 4))),
                   XT._run_layout(L, monkeypatch, "LT_DECONV_NO_H2D", True, nphase=4, stride=2, pad=1, transposed=True), want)


@functools.lru_cache(maxsize=2)
def _gauss(N, Hh, W, k, transposed):
    """Gaussian operands rounded to bf16, the layer's input on the GPU, and gamma / K = 2^-24 sum |x| |w| per output in fp64."""
    g = torch.Generator().manual_seed(1000 * N + 10 * Hh + k)
    x = bf16_round(torch.relu(torch.randn(N, 256, Hh, W, generator=g)))
    w = bf16_round(torch.randn(256, 256, k, k, generator=g) / 48.0)
    ax, aw = x.double().abs(), w.double().abs()
    s = F.conv_transpose2d(ax, aw, None, 2, 1) if transposed else F.conv2d(ax, aw, None, 1, 1)
    return w, to_cl(x, None, BF), s * 2.0 ** -24


def _run(xg, w, transposed):
    b = E.PlanBuilder(DEV, BF)
    y = b.conv(E.Act(xg), w, None, None, stride=2 if transposed else 1, pad=1, transposed=transposed, relu=True)
    assert b.last_info["desc"].phase[0].weight_frag_layout == 2
    b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.t


def _shape_vs_shape(name, inst, K, N, Hh, W, k, transposed, monkeypatch):
    w, xg, g1 = _gauss(N, Hh, W, k, transposed)
    _set(monkeypatch, False)
    ya = _run(xg, w, transposed)
    _set(monkeypatch, True)
    yb = _run(xg, w, transposed)
    _set(monkeypatch, False)
    share = float((ya.view(torch.int16) != yb.view(torch.int16)).float().mean())
    a, b = from_cl(ya, 2).double(), from_cl(yb, 2).double()
    assert float(a.abs().max()) > 0.1
    excess = (a - b).abs() - (2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2 * K * g1)
    record("mfma_shape/%s" % name, {"default_shape": _shape(inst), "share_of_outputs_that_differ": share, "max_abs_difference": float((a - b).abs().max()),
                                    "max_excess_over_bound": float(excess.max())})
    print("%s: share of outputs that differ %.5f, max |d| %.3e, max (|d| - bound) %.3e" % (name, share, float((a - b).abs().max()), float(excess.max())))
    assert float(excess.max()) <= 0.0, "%s: %d outputs beyond the bound" % (name, int((excess > 0).sum()))


@pytest.mark.parametrize("th", ["8", "4"])
@pytest.mark.parametrize("N,Hh", H2D)
def test_halo2d_3x3_shape_against_shape(N, Hh, th, monkeypatch):
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    monkeypatch.setenv("LT_H2D_TH", th)
    _shape_vs_shape("halo2d/N%d_H%d/th%s" % (N, Hh, th), (int(th), 1), 2304, N, Hh, 24, 3, False, monkeypatch)


@pytest.mark.parametrize("N,Hh,W", DECONV)
def test_deconv4x4_shape_against_shape(N, Hh, W, monkeypatch):
    monkeypatch.setenv("LT_H2D_ANY_SIZE", "1")
    _shape_vs_shape("deconv4x4/N%d_%dx%d" % (N, Hh, W), (8, 4), 1024, N, Hh, W, 4, True, monkeypatch)


# ======================================================================================================================================
# conv3d_halo_col_kernel (LT_HALO_COL_MF32=1: 32x32x16): kinds 0 = bf16 store, 1 = computed skip residual, 2 = fp32 store (always 32x32x16)
COL_SWITCH = "LT_HALO_COL_MF32"
# the computed-skip case: the issue named 8 x (8, 32, 64), which is 512 tiles -- under the 1024 the column walk (halo_col_fits) takes; the nearest shape of
# test_gpu_exact.SKIP_SHAPES with the same two-tile columns is 16 x (8, 64, 32) (1024 tiles, two columns per workgroup), and its reference is shared with that file
SKIP_SHAPE = XT.SKIP_SHAPES[1]
assert SKIP_SHAPE == (16, 8, 64, 32)


def _col_shape(kind):
    return H.lib().lt_sel_halo_col_mfma(kind)


def _set_col(monkeypatch, on):
    if on:
        monkeypatch.setenv(COL_SWITCH, "1")
    else:
        monkeypatch.delenv(COL_SWITCH, raising=False)


@pytest.mark.parametrize("case", list(K.COL_CASES))
def test_column_walk_both_shapes_bit_exact(case, monkeypatch):
    monkeypatch.delenv("LT_HALO_NO_COL", raising=False)
    L = XT.col_case(case)
    with X.Collector() as c:
        for on in (False, True):
            _set_col(monkeypatch, on)
            nm = "exact/mfma_shape/halo3d_col/%s/mfma%d" % (case, _col_shape(0))
            c.bits(nm + "/res", L.run(BF, H.TILE_HALO, relu=True, res=True), L.want(relu=True, res=True))
            c.bits(nm + "/plain", L.run(BF, 0), L.want())
            c.bits(nm + "/relu_only", L.run(BF, 0, relu=True, bias=False, bn=False), L.want(relu=True, bias=False, bn=False))


def _run_skip(ya, xa, w, ws, bias, bn, bs, bns):
    b = E.PlanBuilder(DEV, BF)
    assert b.can_conv_skip(ya.shape, w, xa.shape, ws)
    z = b.conv(ya, w, bias, bn, pad=1, relu=True, skip=(xa, ws, bs, bns))
    plan = b.finish()
    assert len(plan.ops) == 1
    plan.run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return z.t


def test_conv_skip_both_shapes_bit_exact(monkeypatch):
    monkeypatch.delenv("LT_NO_CONV_SKIP", raising=False)
    S = XT.skip_case(*SKIP_SHAPE, True)
    ya, xa = E.Act(to_cl(S.y, None, BF)), E.Act(to_cl(S.x, None, BF))
    with X.Collector() as c:
        for on in (False, True):
            _set_col(monkeypatch, on)
            c.bits("exact/mfma_shape/%s/mfma%d" % (S.name, _col_shape(1)), from_cl(_run_skip(ya, xa, S.w, S.ws, S.bias, S.bn, S.bs, S.bns), 3), S.want_fused)


def _abs_sums64(ax, aw):
    """sum |x| |w| of a 3x3x3 / pad 1 convolution per output, in fp64 on the GPU (im2col rows x one fp64 GEMM per sample); channels-first result on the CPU."""
    cout = aw.shape[0]
    wm = aw.to(DEV).double().reshape(cout, -1).t().contiguous()
    outs = []
    for x1 in ax:
        xp = F.pad(x1.to(DEV).double(), (1, 1, 1, 1, 1, 1))
        cols = xp.unfold(1, 3, 1).unfold(2, 3, 1).unfold(3, 3, 1)          # C, D, H, W, 3, 3, 3
        D, Hh, W = cols.shape[1:4]
        rows = cols.permute(1, 2, 3, 0, 4, 5, 6).reshape(D * Hh * W, -1)
        outs.append((rows @ wm).reshape(D, Hh, W, cout).permute(3, 0, 1, 2).cpu())
    return torch.stack(outs)


@functools.lru_cache(maxsize=1)
def _gauss3d(N, sp):
    g = torch.Generator().manual_seed(77 + N + sp[0])
    x = bf16_round(torch.relu(torch.randn(N, 32, *sp, generator=g)))
    xs = bf16_round(torch.relu(torch.randn(N, 16, *sp, generator=g)))
    w = bf16_round(torch.randn(32, 32, 3, 3, 3, generator=g) / 864 ** 0.5)
    ws = bf16_round(torch.randn(32, 16, 1, 1, 1, generator=g) / 4.0)
    res = bf16_round(torch.randn(N, 32, *sp, generator=g))
    g1 = 864 * 2.0 ** -24 * _abs_sums64(x.abs(), w.abs())
    gs = 16 * 2.0 ** -24 * torch.einsum("ncdhw,oc->nodhw", xs.double().abs(), ws.double().abs()[:, :, 0, 0, 0])
    return x, xs, w, ws, res, g1, gs


def _compare(name, kind, ya, yb, gamma):
    share = float((ya.view(torch.int16) != yb.view(torch.int16)).float().mean())
    a, b = from_cl(ya, 3).double(), from_cl(yb, 3).double()
    assert float(a.abs().max()) > 0.1
    excess = (a - b).abs() - (2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2 * gamma)
    record("mfma_shape/%s" % name, {"default_shape": _col_shape(kind), "share_of_outputs_that_differ": share, "max_abs_difference": float((a - b).abs().max()),
                                    "max_excess_over_bound": float(excess.max())})
    print("%s: share of outputs that differ %.5f, max |d| %.3e, max (|d| - bound) %.3e" % (name, share, float((a - b).abs().max()), float(excess.max())))
    assert float(excess.max()) <= 0.0, "%s: %d outputs beyond the bound" % (name, int((excess > 0).sum()))


@pytest.mark.parametrize("case", list(K.COL_CASES))
def test_column_walk_shape_against_shape(case, monkeypatch):
    """K = 864; residual + ReLU and the bare sums, no BatchNorm or bias (the bound then needs no scale; the residual joins the fp32 sum before the one rounding)."""
    monkeypatch.delenv("LT_HALO_NO_COL", raising=False)
    N, sp = K.COL_CASES[case]
    x, _, w, _, res, g1, _ = _gauss3d(N, tuple(sp))
    xg, rg = E.Act(to_cl(x, None, BF)), E.Act(to_cl(res, None, BF))

    def run(with_res):
        b = E.PlanBuilder(DEV, BF)
        y = b.conv(xg, w, None, None, stride=1, pad=1, relu=with_res, residual=rg if with_res else None)
        b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return y.t
    for with_res in (True, False):
        _set_col(monkeypatch, False)
        ya = run(with_res)
        _set_col(monkeypatch, True)
        yb = run(with_res)
        _set_col(monkeypatch, False)
        _compare("halo3d_col/%s/%s" % (case, "res" if with_res else "plain"), 0, ya, yb, g1)


def test_conv_skip_shape_against_shape(monkeypatch):
    """The computed skip residual adds a K = 16 sum to the K = 864 one: gamma is the sum of the two bounds."""
    monkeypatch.delenv("LT_NO_CONV_SKIP", raising=False)
    N, sp = SKIP_SHAPE[0], SKIP_SHAPE[1:]
    x, xs, w, ws, _, g1, gs = _gauss3d(N, tuple(sp))
    ya, xa = E.Act(to_cl(x, None, BF)), E.Act(to_cl(xs, None, BF))
    _set_col(monkeypatch, False)
    za = _run_skip(ya, xa, w, ws, None, None, None, None)
    _set_col(monkeypatch, True)
    zb = _run_skip(ya, xa, w, ws, None, None, None, None)
    _set_col(monkeypatch, False)
    _compare("conv_skip/%s" % "x".join(map(str, SKIP_SHAPE)), 1, za, zb, g1 + gs)


COL_DEFAULT_SHAPE = {0: 16, 1: 16, 2: 32}          # the measured winners (profiles/mfma_shape_ab.json); the fp32-store (training) instantiation keeps 32x32x16


def test_column_walk_dispatch(monkeypatch):
    monkeypatch.delenv(COL_SWITCH, raising=False)
    for kind, want in COL_DEFAULT_SHAPE.items():
        assert _col_shape(kind) == want, kind
    assert _col_shape(3) == 0 and _col_shape(-1) == 0
    # the switch moves no shape between kernels: a column-walk shape and the 7^3 front layer's predicate answer alike under either setting
    for on in (False, True):
        _set_col(monkeypatch, on)
        assert H.lib().lt_sel_halo7_col(H.dtype_code(BF), H.dims((8, 8, 32, 64, 32))) == 1
        assert H.lib().lt_sel_halo7_col(H.dtype_code(BF), H.dims((8, 4, 32, 64, 32))) == 0
        w5, ws5 = H.wshape(torch.zeros(32, 32, 3, 3, 3)), H.wshape(torch.zeros(32, 16, 1, 1, 1))
        assert H.lib().lt_sel_conv_skip(H.dtype_code(BF), H.dims((16, 8, 64, 32, 32)), w5, H.dims((16, 8, 64, 32, 16)), ws5) == 1
        assert H.lib().lt_sel_conv_skip(H.dtype_code(BF), H.dims((8, 8, 32, 64, 32)), w5, H.dims((8, 8, 32, 64, 16)), ws5) == 0          # 512 tiles
    monkeypatch.setenv(COL_SWITCH, "1")
    for kind in COL_DEFAULT_SHAPE:
        assert _col_shape(kind) == 32, kind


DEFAULT_SHAPE = {(8, 1): 16, (4, 1): 16, (8, 4): 16}          # the measured winners (profiles/mfma_shape_ab.json)


def test_dispatch(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    for inst in INSTANCES:
        assert _shape(inst) == DEFAULT_SHAPE[inst], inst
    assert _shape((4, 4)) == 0 and _shape((16, 1)) == 0          # no such instantiation
    monkeypatch.setenv(SWITCH, "1")
    for inst in INSTANCES:
        assert _shape(inst) == 32, inst
    # a layer outside the 2D-halo predicate (20-wide maps: the implicit GEMM's layout 3) is packed alike under either setting; a layer inside it keeps layout 2
    b = E.PlanBuilder(DEV, BF)
    w = torch.zeros(256, 256, 3, 3)
    for on in (False, True):
        _set(monkeypatch, on)
        assert b.frag_layout(E.make_conv_spec(w, None, None, (32, 1, 24, 20, 256), 1, 1, BF, False, 0), w, False, False) == 3
        assert b.frag_layout(E.make_conv_spec(w, None, None, (32, 1, 24, 24, 256), 1, 1, BF, False, 0), w, False, False) == 2          # 96 tiles >= 60
