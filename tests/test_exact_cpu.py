"""CPU: the premises of the bit-exact GPU gates (tests/exact.py, tests/test_gpu_exact.py), checked without a GPU.

  * lt_engine.fold_bn turns the dyadic BatchNorm tuples into exact powers of two;
  * under the exactness condition the fp32 torch reference equals the fp64 one, once per kernel family;
  * every case table of test_gpu_exact.py meets the exactness and the sensitivity condition (its builders assert both while they compute
    the reference; the largest volumes are cropped here and bounded analytically by K * max|x| * max|w| where the GPU tests run them whole);
  * the host side of lt_conv_fwd -- weight packing, tap tables, transposed phases, the fold -- interpreted by emul.emulate_conv on integer
    operands equals the torch reference exactly;
  * the mutations that gpu_util.check accepts on Gaussian operands are rejected by assert_bits_equal on exact operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import emul
import exact as X
import gpu_util
import lt_engine as E
import test_gpu_exact as G
import test_gpu_kernels as K


@pytest.fixture(autouse=True)
def _no_report():
    """gpu_util.check / assert_bits_equal record into the GPU parity report: keep the CPU suite out of it."""
    saved = dict(gpu_util.REPORT)
    yield
    gpu_util.REPORT.clear()
    gpu_util.REPORT.update(saved)


@pytest.mark.parametrize("p4", [0.25, 1.0, 4.0, 16.0])
def test_fold_bn_of_a_dyadic_batchnorm_is_exact(p4):
    """var = fl32(4^k) - fl32(1e-5) folds to invstd == 2^-k exactly, and scale / shift to the intended dyadic values."""
    c = 64
    g = X.gen(int(p4 * 4))
    gamma = torch.pow(2.0, torch.randint(-2, 3, (c,), generator=g).float())
    beta, mean = X.ints((c,), 31, g), X.ints((c,), 15, g)
    var = torch.full((c,), float(np.float32(p4) - np.float32(1e-5)))
    bi, sc, sh = E.fold_bn(c, None, (gamma, beta, mean, var), c)
    inv = 1.0 / np.sqrt(p4)
    assert torch.equal(sc, gamma * inv) and torch.equal(sh, beta - mean * gamma * inv) and float(bi.abs().max()) == 0.0
    X.fold(c, X.ints((c,), 63, g), (gamma, beta, mean, var))          # the helper's own assertion agrees
    bn, _ = X.dyadic_bn(c, g)
    _, sc2, _ = X.fold(c, None, bn)
    assert set(np.log2(sc2.numpy()).tolist()) <= set(float(v) for v in range(-3, 3))


def test_fold_assertion_rejects_a_batchnorm_that_is_not_dyadic():
    g = X.gen(3)
    bn = (torch.ones(8), X.ints((8,), 31, g), X.ints((8,), 15, g), torch.full((8,), 0.7))
    with pytest.raises(AssertionError, match="power of two"):
        X.fold(8, None, bn)


FAMILIES = {  # one shape per kernel family: (nd, N, cin, cout, k, stride, pad, spatial, transposed)
    "conv2d 3x3 256->256 (K = 2304)": (2, 2, 256, 256, 3, 1, 1, (24, 24), False),
    "conv2d 1x1 1024->256": (2, 1, 1024, 256, 1, 1, 0, (12, 12), False),
    "conv3d 3^3 32->32": (3, 2, 32, 32, 3, 1, 1, (8, 16, 16), False),
    "conv3d 7^3 32->16": (3, 1, 32, 16, 7, 1, 3, (8, 16, 8), False),
    "deconv2d 4x4 s2": (2, 2, 256, 256, 4, 2, 1, (8, 12), True),
    "deconv3d 2^3 s2": (3, 1, 64, 32, 2, 2, 0, (4, 8, 8), True),
    "stem 7x7 s2": (2, 2, 3, 64, 7, 2, 3, (37, 41), False),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fp32_reference_equals_fp64_under_the_exactness_condition(family):
    nd, N, cin, cout, k, s, p, sp, tr = FAMILIES[family]
    x, w, b, bn, _ = X.conv_operands(nd, N, cin, cout, k, sp, 11, transposed=tr)
    a64, bound = X.conv_sum(x, w, s, p, tr, family)
    a32, _ = X.conv_sum(x, w, s, p, tr, family, force_f32=True)
    assert torch.equal(a64, a32)
    if family.startswith("conv2d 3x3 256"):
        assert float(a64.abs().max()) < 2 ** 24 and float(bound.max()) < 2 ** 24
    conv = X._conv_fn(nd, tr)
    assert torch.equal(conv(x, w, None, s, p).double(), a64)          # (the plain fp32 call, whatever algorithm torch picks)


def test_fp32_einsum_equals_fp64_for_the_weight_gradient():
    g = X.gen(5)
    dy, x = X.ints((3456, 64), 15, g), X.ints((3456, 256), 15, g)
    X.assert_exact("wgrad", 3456 * 225.0, 1.0)
    assert torch.equal(torch.einsum("rk,rc->kc", dy, x).double(), torch.einsum("rk,rc->kc", dy.double(), x.double()))


CASES = G.all_cases()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case_tables_meet_both_conditions(name):
    """Builds the operands and the reference of a GPU case on the CPU: the builder asserts the fold, the exactness condition of every stage and
    the sensitivity condition of every bf16 store."""
    dict(CASES)[name]()


def test_the_conditions_reject_what_they_should():
    g = X.gen(9)
    x, w = X.ints((1, 256, 8, 8), 255, g), X.ints((256, 256, 3, 3), 255, g)
    with pytest.raises(AssertionError, match="exactness"):
        X.conv_sum(x, w, 1, 1)
    with pytest.raises(AssertionError, match="sensitivity"):
        X.assert_sensitive("small integers", X.ints((1000,), 100, g))
    with pytest.raises(AssertionError, match="off their grid"):
        X.conv_sum(x * 0.5, w, 1, 1)


EMUL_CASES = list(K.CONV_CASES) + ["deconv2d_4x4", "deconv3d_2x2x2", "stem_padded"]


@pytest.mark.parametrize("case", EMUL_CASES)
def test_emulate_conv_of_integer_weights_equals_the_reference_exactly(case):
    """make_conv_spec (packing, tap tables, transposed phases, fold_bn) interpreted by emul.emulate_conv == torch, bit for bit."""
    tr, cin_pad = False, None
    if case == "deconv2d_4x4":
        nd, N, cin, cout, k, s, p, sp, tr = 2, 2, 64, 256, 4, 2, 1, (6, 7), True
    elif case == "deconv3d_2x2x2":
        nd, N, cin, cout, k, s, p, sp, tr = 3, 1, 128, 64, 2, 2, 0, (4, 4, 4), True
    elif case == "stem_padded":
        nd, N, cin, cout, k, s, p, sp, cin_pad = 2, 2, 3, 64, 7, 2, 3, (37, 41), 8
    else:
        nd, N, cin, cout, k, s, p, sp = K.CONV_CASES[case]
    x, w, b, bn, _ = X.conv_operands(nd, N, cin, cout, k, sp, G._seed(case), transposed=tr)
    res = X.ints((N, cout) + G._osp(sp, k, s, p, tr), 255, X.gen(1))
    acc, bound = X.conv_sum(x, w, s, p, tr, case)
    want = X.as_f32(X.epilogue(acc, bound, cout, b, bn, True, False, res, case))
    xc = x.unsqueeze(2) if nd == 2 else x
    xc = xc.permute(0, 2, 3, 4, 1).contiguous()
    if cin_pad:
        xc = torch.cat([xc, torch.zeros(*xc.shape[:-1], cin_pad - cin)], dim=-1)
    spec = E.make_conv_spec(w, b, bn, tuple(xc.shape), s, p, torch.bfloat16, tr, emul.EPI_RELU_POST)
    rc = (res.unsqueeze(2) if nd == 2 else res).permute(0, 2, 3, 4, 1).contiguous()
    got = emul.emulate_conv(spec, xc, rc).permute(0, 4, 1, 2, 3)
    X.assert_bits_equal("emul/" + case, got[:, :, 0] if nd == 2 else got, want)


# ---- the mutation table: mistakes a kernel rewrite makes, against both gates ----------------------------------------------------------------------------------------------------
def _trunc_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _layer3(x, w, res, mutation):
    """relu(conv3x3(x, w) + res) stored in bf16 -- correct, or with one of the mistakes a kernel rewrite makes.  fp32 torch throughout."""
    x, w = x.clone(), w.clone()
    if mutation == "weight_element_never_read":
        i = (w != 0).reshape(-1).nonzero()[0]
        w.view(-1)[i] = 0.0
    if mutation == "input_element_never_read":
        assert float(x[-1, -1, -1, -1]) != 0.0
        x[-1, -1, -1, -1] = 0.0
    if mutation == "half_k_partial_in_bf16":
        h = x.shape[1] // 2
        conv = gpu_util.bf16_round(F.conv2d(x[:, :h], w[:, :h], None, 1, 1)) + F.conv2d(x[:, h:], w[:, h:], None, 1, 1)
    else:
        conv = F.conv2d(x, w, None, 1, 1)
    if mutation == "conv_rounded_before_the_residual_add":
        conv = gpu_util.bf16_round(conv)
    v = torch.relu(conv + res)
    return _trunc_bf16(v) if mutation == "truncating_store" else gpu_util.bf16_round(v)


MUTATIONS = ["truncating_store", "half_k_partial_in_bf16", "conv_rounded_before_the_residual_add", "weight_element_never_read", "input_element_never_read"]


@pytest.fixture(scope="module")
def layer3_operands():
    g = X.gen(2024)
    rd = gpu_util.bf16_round
    gx, gw = rd(torch.randn(2, 256, 24, 24, generator=g)), rd(torch.randn(256, 256, 3, 3, generator=g) / 2304 ** 0.5)
    gres = rd(torch.randn(2, 256, 24, 24, generator=g))
    ix, iw, ires = X.ints((2, 256, 24, 24), 15, g), X.ints((256, 256, 3, 3), 15, g), X.ints((2, 256, 24, 24), 255, g)
    ix[-1, -1, -1, -1] = 7.0
    return (gx, gw, gres), (ix, iw, ires)


def test_exact_operands_pass_the_correct_layer(layer3_operands):
    (gx, gw, gres), (ix, iw, ires) = layer3_operands
    gpu_util.check("mutation/none/gauss", _layer3(gx, gw, gres, None), torch.relu(F.conv2d(gx, gw, None, 1, 1) + gres), 1.5e-2)
    X.assert_bits_equal("mutation/none/exact", _layer3(ix, iw, ires, None), X.conv_ref(ix, iw, None, None, 1, 1, relu=True, residual=ires))


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutations_pass_the_tolerance_gate_and_fail_the_bit_gate(layer3_operands, mutation):
    """The layer3 shape (3x3, 256 -> 256, 2 x 24 x 24).  On Gaussian operands gpu_util.check at the suite's bf16 tolerance accepts the first four
    mutations (the dropped input element it catches by a hair, so no acceptance is asserted for it); on exact operands assert_bits_equal rejects all
    five, and by a wide margin where the mutation touches every output."""
    (gx, gw, gres), (ix, iw, ires) = layer3_operands
    ref = torch.relu(F.conv2d(gx, gw, None, 1, 1) + gres)
    if mutation != "input_element_never_read":
        gpu_util.check("mutation/%s/gauss" % mutation, _layer3(gx, gw, gres, mutation), ref, 1.5e-2)          # today's gate lets it through
    want = X.conv_ref(ix, iw, None, None, 1, 1, relu=True, residual=ires)
    got = _layer3(ix, iw, ires, mutation)
    with pytest.raises(AssertionError, match="words differ"):
        X.assert_bits_equal("mutation/%s/exact" % mutation, got, want)
    share = float(X.bits_differ(got, want).float().mean())
    if mutation in ("truncating_store", "half_k_partial_in_bf16", "conv_rounded_before_the_residual_add"):
        assert share > 0.05, share          # not one unlucky word: a large share of the output
