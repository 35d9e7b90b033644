"""GPU (-m gpu): conv3d_halo7_col_kernel, the column walk of V2V's front layer (7^3, 32 -> 16, bf16), against the one-tile kernel it replaces
(LT_HALO_NO_COL7=1), against exact integer sums and against torch.

The column walk runs the one-tile kernel's tap nest unchanged and differs only in what happens between two nests (the ten-plane halo ring,
the weight ring carried across tiles, the epilogue under the next plane group), so its output must be the one-tile kernel's BIT FOR BIT:
that comparison carries the file.  The shapes are the smallest that reach every branch of the walk:

  pin_1col_2deep   256 columns, XCD-pinned dealing, one column per workgroup, one seam
  pin_1col_6deep   six tiles per column: the ring rotations 0, 4, 8, 2, 6 and the wrap back to 0
  pin_2col_2deep   two columns per workgroup: plane ring and weight ring restart between columns
  raster_uneven    320 columns on 256 workgroups: raster dealing, workgroups with one and with two columns

Every column touches both d faces, and the cases cover all h / w faces, so padding is reached everywhere."""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact as X
import lt_engine as E
import lt_hip as H
from gpu_util import bf16_round, check, to_cl
from test_gpu_exact import BF, layer
from test_gpu_kernels import HALO_CASES, _bn, _bn_ref, run_conv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {
    "pin_1col_2deep": (8, (8, 32, 64)),
    "pin_1col_6deep": (8, (24, 32, 64)),
    "pin_2col_2deep": (16, (8, 32, 64)),
    "raster_uneven": (5, (8, 64, 64)),
}
SWITCH = "LT_HALO_NO_COL7"


def _takes_col(N, sp, cin=32):
    return bool(H.lib().lt_sel_halo7_col(H.dtype_code(BF), H.dims((N,) + tuple(sp) + (cin,))))


@functools.lru_cache(maxsize=2)
def _operands(case, cout=16):
    """Gaussian operands of a case, already on the GPU in the kernels' layout (shared by the tests of that case, never modified)."""
    N, sp = CASES[case]
    g = torch.Generator().manual_seed(700 + len(case) + cout)
    x = torch.randn(N, 32, *sp, generator=g)
    w = torch.randn(cout, 32, 7, 7, 7, generator=g) * (1.0 / (32 * 343) ** 0.5)
    bias = torch.randn(cout, generator=g) * 0.1
    bn = _bn(cout, g)
    res = torch.randn(N, cout, *sp, generator=g)
    return x, w, bias, bn, res, to_cl(x, None, BF), to_cl(res, None, BF)


def _raw(ops, with_res):
    """The stored bf16 tensor (N, D, H, W, C) of the layer, through AUTO dispatch."""
    _, w, bias, bn, _, xg, rg = ops
    b = E.PlanBuilder(DEV, BF)
    y = b.conv(E.Act(xg), w, bias, bn, stride=1, pad=3, relu=with_res, residual=E.Act(rg) if with_res else None)
    b.finish().run_eager(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.t


def _both(ops, with_res, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    col = _raw(ops, with_res)
    monkeypatch.setenv(SWITCH, "1")
    one = _raw(ops, with_res)
    monkeypatch.delenv(SWITCH)
    return col, one


@pytest.mark.parametrize("case", list(CASES))
def test_column_walk_is_bit_identical_to_the_one_tile_kernel(case, monkeypatch):
    """Gaussian bf16 data, residual + ReLU and affine only: torch.equal on the raw bf16 words of the two kernels' outputs."""
    N, sp = CASES[case]
    monkeypatch.delenv(SWITCH, raising=False)
    assert _takes_col(N, sp)
    ops = _operands(case)
    for with_res in (True, False):
        col, one = _both(ops, with_res, monkeypatch)
        assert col.dtype == torch.bfloat16 and col.shape == one.shape and float(one.float().abs().max()) > 0.1
        assert torch.equal(col.view(torch.int16), one.view(torch.int16)), "%s/%s: %d words differ" % (
            case, "res" if with_res else "plain", int((col.view(torch.int16) != one.view(torch.int16)).sum()))


def test_column_walk_scalar_store_path_is_bit_identical(monkeypatch):
    """12 output channels (padded to 16 in the kernel): the element-wise epilogue of both kernels, with and without a residual."""
    ops = _operands("pin_1col_2deep", 12)
    for with_res in (True, False):
        col, one = _both(ops, with_res, monkeypatch)
        assert float(one.float().abs().max()) > 0.1
        assert torch.equal(col.view(torch.int16), one.view(torch.int16)), "cout 12/%s" % ("res" if with_res else "plain")


def col7_case(case, crop=False):
    N, sp = CASES[case]
    return layer("halo7col/" + case, 3, N, 32, 16, 7, 1, 3, sp, crop=crop)


@pytest.mark.parametrize("case", ["pin_1col_6deep", "raster_uneven"])
def test_column_walk_integer_operands_bit_exact(case, monkeypatch):
    """Small integers and power-of-two epilogue constants (tests/exact.py): a wrong plane, ring slot or tap is a wrong integer, not noise."""
    monkeypatch.delenv(SWITCH, raising=False)
    assert _takes_col(*CASES[case])
    L = col7_case(case)
    with X.Collector() as c:
        c.bits("exact/halo7_col/%s/res" % case, L.run(BF, H.TILE_HALO, relu=True, res=True), L.want(relu=True, res=True))
        c.bits("exact/halo7_col/%s/plain" % case, L.run(BF, 0), L.want())


@pytest.mark.parametrize("case", ["pin_1col_2deep", "raster_uneven"])
def test_column_walk_against_torch(case, monkeypatch):
    """F.conv3d on bf16-rounded operands, the 7^3 tolerance of test_conv3d_halo7_variants."""
    monkeypatch.delenv(SWITCH, raising=False)
    x, w, bias, bn, res, _, _ = _operands(case)
    rd = bf16_round
    conv = _bn_ref(F.conv3d(rd(x), rd(w), bias, 1, 3), bn)
    out = run_conv(x, w, bias, bn, 1, 3, BF, H.TILE_HALO, relu=True, residual=res)
    check("conv3d_halo7_col/%s/res" % case, out, torch.relu(conv + rd(res)), 1.5e-2)
    out2 = run_conv(x, w, bias, bn, 1, 3, BF, 0)
    check("conv3d_halo7_col/%s/plain" % case, out2, conv, 1.5e-2)


def test_dispatch(monkeypatch):
    """The cases above take the column walk; the shapes of the one-tile kernel's own tests (one column, 16 columns) stay on it; the switch
    sends every shape back."""
    monkeypatch.delenv(SWITCH, raising=False)
    for case, (N, sp) in CASES.items():
        assert _takes_col(N, sp), case
    for case in ("halo_7x7_32_16", "halo_7x7_32_16_big"):
        N, cin, cout, k, sp, _ = HALO_CASES[case]
        assert (cin, cout, k) == (32, 16, 7) and not _takes_col(N, sp), case
    assert not _takes_col(8, (4, 32, 64))          # one tile per column
    assert not _takes_col(8, (8, 32, 56))          # 224 columns
    assert not _takes_col(9, (8, 40, 48))          # 270 columns: not a multiple of 8
    assert not _takes_col(8, (10, 32, 64))         # D is not a multiple of the tile
    assert not _takes_col(8, (8, 32, 64), cin=16)
    monkeypatch.setenv(SWITCH, "1")
    for case, (N, sp) in CASES.items():
        assert not _takes_col(N, sp), case
