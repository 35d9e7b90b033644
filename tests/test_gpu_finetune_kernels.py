"""GPU (-m gpu): lt_bn_act_bwd with optional outputs (csrc/train.hip), the BatchNorm backward of a fine-tuning step with frozen parameters.
  * dgamma = dbeta = NULL (frozen affine parameters): dy, dres and the bf16 copy of dy are BIT FOR BIT those of the full call -- with batch statistics
    the same three kernels run and the finalized sums land in the workspace; with LT_BN_FROZEN one elementwise pass runs (no reduce, no finalize, no
    workspace), whose dy = gamma invstd g is the full call's gamma invstd (g - 0 dbeta - 0 x^ dgamma) for finite sums;
  * dy = NULL (only the parameter gradients): dgamma / dbeta bit for bit those of the full call, nothing else written;
  * one case per statistics mode against fp64 autograd at the tolerances of test_gpu_train_kernels.py::test_bn_act_bwd_frozen_statistics.
Inputs: test_gpu_train_kernels._bn_reference's recipe at the shapes listed below."""
import pytest
import torch

from gpu_util import check, record
import test_gpu_train_kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

SHAPES = {  # id -> (rows, C)
    "37x4_smallest_vector_ragged_rows": (37, 4),
    "515x64_vector": (515, 64),
    "96x17_generic": (96, 17),
    "33x1028_generic_c_mod_4": (33, 1028),          # 257 float4 per row: NOT a shape of the vector path (colsum_fast wants a multiple of 1024 above 1024)
    "33x2048_vector_second_channel_block": (33, 2048),          # ... this one is: blockIdx.y == 1 of the vector apply kernel
}
VARIANTS = {  # id -> (flags name, residual, accumulate_res)
    "none": ("none", False, 0),
    "relu_post_res_acc": ("relu", True, 1),
    "relu_post_res_noacc": ("relu", True, 0),
    "relu_pre_res_noacc": ("relu_pre", True, 0),
}
CASES = [(s, v, b) for s in SHAPES for v in VARIANTS for b in (False, True) if not b or SHAPES[s][1] % 4 == 0]
_REF = {}


def _reference(monkeypatch, sid, vid, bf16, frozen):
    """_bn_reference at this module's shapes and variants; computed once per case and shared."""
    key = (sid, vid, bf16, frozen)
    if key not in _REF:
        monkeypatch.setitem(K.BN_SHAPES, sid, SHAPES[sid])
        monkeypatch.setitem(K.VARIANTS, vid, VARIANTS[vid])
        _REF[key] = K._bn_reference(sid, vid, bf16, frozen=frozen)
    return _REF[key]


class _Call:
    """One layer's device tensors and the three ways of calling lt_bn_act_bwd on them."""

    def __init__(self, R, bf16, frozen):
        self.H, self.lib = K._lib()
        H = self.H
        self.R, self.rows, self.C = R, R["rows"], R["C"]
        self.dt = dt = BF if bf16 else torch.float32
        self.flags = K._flags(H, R["flags_name"]) | (H.BN_FROZEN if frozen else 0) | ((H.BN_Y_BF16 | H.ACT_BF16) if bf16 else 0)
        self.y, self.dz = R["y"].to(DEV, dt), R["dz"].to(DEV, dt)
        self.res = R["res"].to(DEV, dt) if R["with_res"] else None
        self.mean, self.var = R["mean"].float().to(DEV), R["var"].float().to(DEV)
        self.gamma, self.beta = R["gamma"].to(DEV), R["beta"].to(DEV)
        self.want16 = (not bf16) and K._colsum_fast(self.C)          # the bf16 copy of dy: where the full call takes it
        self.ws = torch.empty(max(1, self.lib.lt_bn_act_bwd_workspace(self.rows, self.C)), dtype=torch.uint8, device=DEV)

    def run(self, dy=True, pg=True, ws=True):
        """-> (rc, dy, dy16, dgamma, dbeta, dres); buffers not asked for stay None, the others start from a pattern the kernel must overwrite."""
        H, lib, rows, C = self.H, self.lib, self.rows, self.C
        o_dy = torch.full((rows, C), 7.0, dtype=self.dt, device=DEV) if dy else None
        o_16 = torch.full((rows, C), 7.0, dtype=BF, device=DEV) if (dy and self.want16) else None
        o_dg, o_db = (torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)) if pg else (None, None)
        o_dr = torch.full((rows, C), 3.0, dtype=self.dt, device=DEV) if (dy and self.res is not None) else None
        rc = lib.lt_bn_act_bwd(self.dz.data_ptr(), self.y.data_ptr(), H.ptr(self.res), self.mean.data_ptr(), self.var.data_ptr(), self.gamma.data_ptr(),
                               self.beta.data_ptr(), H.ptr(o_dy), H.ptr(o_16), H.ptr(o_dg), H.ptr(o_db), H.ptr(o_dr), self.R["acc"], rows, C, 1e-5, self.flags,
                               self.ws.data_ptr() if ws else None, K._st())
        torch.cuda.synchronize()
        return rc, o_dy, o_16, o_dg, o_db, o_dr


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_stats"])
@pytest.mark.parametrize("sid,vid,bf16", CASES, ids=["%s-%s-%s" % (s, v, "act16" if b else "fp32") for s, v, b in CASES])
def test_bn_act_bwd_optional_outputs_match_the_full_call(monkeypatch, sid, vid, bf16, frozen):
    R = _reference(monkeypatch, sid, vid, bf16, frozen)
    for k in ("y", "dz", "gamma", "beta", "mean", "var"):
        assert bool(torch.isfinite(R[k]).all())
    c = _Call(R, bf16, frozen)
    assert K._colsum_fast(c.C) == ("vector" in sid)
    rc, dy, dy16, dga, dbe, dres = c.run()
    assert rc == 0, c.lib.lt_last_error()
    assert bool(torch.isfinite(dga).all()) and bool(torch.isfinite(dbe).all())
    # frozen affine parameters: the same dy / dres / bf16 copy, no parameter gradient written anywhere
    rc, dy_a, dy16_a, _, _, dres_a = c.run(pg=False)
    assert rc == 0, c.lib.lt_last_error()
    assert torch.equal(dy_a, dy), "dy without dgamma / dbeta differs from the full call"
    if dres is not None:
        assert torch.equal(dres_a, dres)
    if dy16 is not None:
        assert torch.equal(dy16_a, dy16) and torch.equal(dy16, dy.bfloat16())
    # only the parameter gradients
    rc, _, _, dga_b, dbe_b, _ = c.run(dy=False)
    assert rc == 0, c.lib.lt_last_error()
    assert torch.equal(dga_b, dga) and torch.equal(dbe_b, dbe)
    if frozen:          # the elementwise pass reads no workspace
        rc, dy_c, dy16_c, _, _, dres_c = c.run(pg=False, ws=False)
        assert rc == 0, c.lib.lt_last_error()
        assert torch.equal(dy_c, dy) and (dres is None or torch.equal(dres_c, dres)) and (dy16 is None or torch.equal(dy16_c, dy16))
    else:
        assert c.run(pg=False, ws=False)[0] == -1 and b"workspace" in c.lib.lt_last_error()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "act16"])
@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_stats"])
def test_bn_act_bwd_optional_outputs_vs_fp64_autograd(monkeypatch, frozen, bf16):
    """Each of the two reduced calls against fp64 autograd of the layer: dy / dres of the call without parameter gradients, dgamma / dbeta of the call
    without dy (tolerances of test_bn_act_bwd_frozen_statistics: 2e-5 fp32 dy and sums, 2e-6 dres, 8e-3 for a bf16 tensor)."""
    sid, vid = "515x64_vector", "relu_post_res_acc"
    R = _reference(monkeypatch, sid, vid, bf16, frozen)
    tag = "ftk/bn_act_bwd optional outputs %s %s" % ("frozen" if frozen else "batch", "bf16" if bf16 else "fp32")
    record(tag + " masked share", R["masked_share"])
    assert R["masked_share"] < 1e-3
    c = _Call(R, bf16, frozen)
    rc, dy, _, _, _, dres = c.run(pg=False, ws=not frozen)
    assert rc == 0, c.lib.lt_last_error()
    check(tag + " dy", dy.float().cpu(), R["dy"], 8e-3 if bf16 else 2e-5)
    check(tag + " dres", dres.float().cpu(), R["dres"] + 3.0, 8e-3 if bf16 else 2e-6)
    rc, _, _, dga, dbe, _ = c.run(dy=False)
    assert rc == 0, c.lib.lt_last_error()
    check(tag + " dgamma", dga.cpu(), R["dgamma"], 2e-5)
    check(tag + " dbeta", dbe.cpu(), R["dbeta"], 2e-5)
