"""Slack-free gates for the MFMA convolution kernels: operands on a dyadic grid (small integers, power-of-two scales).

Every product and every partial sum of such operands is exact in fp32 IN ANY SUMMATION ORDER, on the MFMA as in plain C++, so the only rounding
a kernel may perform is its documented round-to-nearest-even store, and the reference performs that one rounding on the exact value.  Kernel
and reference must then agree BIT FOR BIT: a truncating store, a 16-bit partial sum, a rounding in a fused seam, one operand element never
read -- all of which gpu_util.check's bf16-sized tolerance accepts on Gaussian operands -- change a large share of the output words.

Two conditions make a case meaningful, and the reference asserts both for every stage of every case:

  exactness    on the grid g of the stage (the largest power of two dividing all of its terms) conv(|x|, |w|) / g < 2^24: no partial sum,
               in whatever order, leaves the 24-bit significand of fp32.  (Where the volume is too large for a second convolution the
               analytic bound K * max|x| * max|w| is used.)
  sensitivity  at least 10 % of the values in front of a bf16 store are NOT bf16-representable, otherwise a wrong rounding mode or a 16-bit
               intermediate could hide.

The reference is torch on the CPU in fp64 where affordable and fp32 elsewhere (exact under the same bound; tests/test_exact_cpu.py asserts
fp32 == fp64 once per kernel family).  There is no sigmoid case: expf is not exact.  This is a plain helper module, not a conftest."""
import numpy as np
import torch
import torch.nn.functional as F

import gpu_util

LIMIT = float(2 ** 24)
SENSITIVE = 0.10
F64_MACS = 2e9          # references up to this many multiply-adds run in fp64


# ---------------------------------------------------------------------------------------------------------------------------------------
# operand generators (seeded)
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(shape, r, g, lo=None):
    """fp32 tensor of integers, uniform in [-r, r] (or [lo, r])."""
    lo = -r if lo is None else lo
    return torch.randint(lo, r + 1, tuple(shape), generator=g).float()


def dyadic_bn(c, g, a=(-1, 1), k=(-1, 2), beta=31, mean=15):
    """An eval-mode BatchNorm tuple (gamma, beta, mean, var) whose fold is dyadic: gamma = 2^a, integer beta and mean, and
    var = fl32(4^k) - fl32(1e-5), which lt_engine.fold_bn turns into invstd == 2^-k exactly for 4^k in {0.25, 1, 4, 16}."""
    ea = torch.randint(a[0], a[1] + 1, (c,), generator=g)
    ek = torch.randint(k[0], k[1] + 1, (c,), generator=g)
    gamma = torch.pow(2.0, ea.float())
    var = torch.from_numpy((np.float32(4.0) ** ek.numpy().astype(np.float32)).astype(np.float32) - np.float32(1e-5))
    bn = (gamma, ints((c,), beta, g), ints((c,), mean, g), var)
    bn_exp = (ea - ek).float()
    return bn, bn_exp


def fold(cout, bias, bn):
    """(bias, scale, shift) of y = (acc + bias) * scale + shift through lt_engine.fold_bn, asserted to be the intended dyadic values
    before anything is launched: scale a power of two, shift = beta - mean * scale without rounding."""
    import lt_engine as E
    bi, sc, sh = E.fold_bn(cout, bias, bn, cout)
    if bn is not None:
        gam, beta, mean, var = (t.double() for t in bn)
        k2 = torch.round(torch.log2(var + 1e-5))                  # var + eps = 4^k
        want_sc = gam * torch.pow(2.0, -k2 / 2)
        m, _ = torch.frexp(sc.double())
        assert bool((m == 0.5).all()), "folded BatchNorm scale is not a power of two: %r" % sc[(m != 0.5)][:4]
        assert torch.equal(sc.double(), want_sc), "folded scale != gamma * 2^-k"
        assert torch.equal(sh.double(), beta - mean * want_sc), "folded shift != beta - mean * scale"
    return bi.double(), sc.double(), sh.double()


def fp8_ints(shape, g):
    """Integers in [-7, 7] with at least one +-7: amax / 448 = 2^-6 exactly, and every multiple of 64 up to 448 is an e4m3 value, so the
    per-tensor quantisation (device lt_amax_* / lt_quant_fp8*, or the host-side weight cast) is lossless."""
    t = ints(shape, 7, g)
    t.view(-1)[0] = 7.0
    return t


# ---------------------------------------------------------------------------------------------------------------------------------------
# the two conditions
def grids_of(t):
    """Per element: the largest power of two dividing it (inf for 0)."""
    t = t.double()
    m, e = torch.frexp(t)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double().clamp(min=1.0)                      # lowest set bit of the 53-bit significand
    g = torch.pow(2.0, e.double() - 53.0 + torch.log2(low))
    return torch.where(t == 0, torch.full_like(g, float("inf")), g)


def grid_of(t):
    """Largest power of two dividing every element of ``t``."""
    return float(grids_of(t).min()) if t.numel() else float("inf")


def on_grid(t, g):
    q = t.double() / g
    return bool((q == q.round()).all())


def assert_exact(name, bound, grid):
    """The exactness condition of one stage: ``bound`` (a tensor or a number, >= every partial sum in magnitude) on ``grid``."""
    b = torch.as_tensor(bound).double()
    gr = torch.as_tensor(grid).double()
    ratio = float((b / gr).max())
    assert ratio < LIMIT, "%s: exactness condition violated, bound / grid = %.4g >= 2^24" % (name, ratio)
    return ratio


def bf16_representable(v):
    v = v.double()
    return v == v.float().to(torch.bfloat16).double()


def sensitivity(v):
    """Share of ``v`` (values in front of a bf16 store) that bf16 cannot represent."""
    return float((~bf16_representable(v)).double().mean())


def assert_sensitive(name, v):
    s = sensitivity(v)
    assert s >= SENSITIVE, "%s: sensitivity condition violated, only %.1f %% of the values in front of the bf16 store are not representable" % (name, 100 * s)
    return s


def as_f32(v, name="value"):
    """An exact value as the fp32 number an fp32 store writes: no rounding allowed."""
    f = v.float()
    assert torch.equal(f.double(), v.double()), name + ": exact value is not an fp32 number"
    return f


def rne_bf16(v):
    """THE rounding of a bf16 store, applied to exact values (fp64 or fp32 that hold them exactly): round to nearest even."""
    f = v.float()
    assert torch.equal(f.double(), v.double()), "value in front of the store is not exact in fp32"
    return f.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
def _conv_fn(nd, transposed):
    return {(2, False): F.conv2d, (3, False): F.conv3d, (2, True): F.conv_transpose2d, (3, True): F.conv_transpose3d}[(nd, transposed)]


def conv_sum(x, w, stride=1, pad=0, transposed=False, name="conv", gx=1.0, gw=1.0, force_f32=False):
    """The exact convolution sums of grid operands as an fp64 tensor, with the exactness condition asserted.  fp64 arithmetic up to
    F64_MACS multiply-adds, fp32 beyond (exact under the same condition); the magnitude bound is conv(|x|, |w|) where the convolution is
    small and K * max|x| * max|w| for the largest volumes.  Returns (sums, bound) -- bound a tensor like sums or a number."""
    nd = x.dim() - 2
    assert on_grid(x, gx) and on_grid(w, gw), name + ": operands off their grid"
    conv = _conv_fn(nd, transposed)
    cout = w.shape[1] if transposed else w.shape[0]
    kk = int(np.prod(w.shape[2:]))
    K = kk * (w.shape[0] if transposed else w.shape[1])
    if transposed:
        macs = float(x.shape[0]) * float(np.prod(x.shape[2:])) * K * cout
    else:
        st = (stride,) * nd if isinstance(stride, int) else tuple(stride)
        pd = (pad,) * nd if isinstance(pad, int) else tuple(pad)
        osp = [(n + 2 * q - kk_) // t + 1 for n, q, kk_, t in zip(x.shape[2:], pd, w.shape[2:], st)]
        macs = float(x.shape[0]) * float(np.prod(osp)) * K * cout
    dt = torch.float64 if (macs <= F64_MACS and not force_f32) else torch.float32
    if macs <= F64_MACS:
        bound = conv(x.abs().to(dt), w.abs().to(dt), None, stride, pad).double()
    else:
        bound = float(K) * float(x.abs().max()) * float(w.abs().max())
    assert_exact(name + " sums", bound, gx * gw)
    return conv(x.to(dt), w.to(dt), None, stride, pad).double(), bound


def epilogue(acc, bound, cout, bias=None, bn=None, relu=False, relu_pre=False, residual=None, name="conv", g_acc=1.0, g_res=1.0, return_grid=False):
    """y = act((acc + bias) * scale + shift [+ residual]) on exact fp64 values, the kernels' order (include/lt_hip.h), with the exactness
    condition asserted per channel on the grid of that channel's terms.  Returns the exact value in front of the store."""
    nd = acc.dim() - 2
    bi, sc, sh = fold(cout, bias, bn)
    sh_ = [1, -1] + [1] * nd
    v = (acc + bi.reshape(sh_)) * sc.reshape(sh_) + sh.reshape(sh_)
    grid = torch.minimum(torch.minimum(g_acc * sc, grids_of(bi) * sc), grids_of(sh)).clamp(max=g_res if residual is not None else float("inf"))
    b = torch.as_tensor(bound).double()
    bmax = b.transpose(0, 1).reshape(cout, -1).amax(dim=1) if b.dim() else b.expand(cout)
    top = (bmax + bi.abs()) * sc + sh.abs()
    if residual is not None:
        assert on_grid(residual, g_res)
        top = top + float(residual.abs().max())
    assert_exact(name + " epilogue", top, grid)
    if relu_pre:
        v = torch.relu(v)
    if residual is not None:
        v = v + residual.double()
    if relu:
        v = torch.relu(v)
    v = v + 0.0          # (-0 + 0 = +0)
    return (v, float(grid.min())) if return_grid else v


class Stage:
    """An exact tensor (fp64 values, (N, C, [D,] H, W)) and the grid all of its elements lie on: what one launch hands to the next."""

    def __init__(self, v, grid=1.0):
        self.v, self.grid = v.double(), float(grid)
        assert on_grid(self.v, self.grid)

    def f32(self):
        f = self.v.float()
        assert torch.equal(f.double(), self.v), "stage value is not an fp32 number"
        return f


def conv_stage(st, w, bias=None, bn=None, stride=1, pad=0, relu=False, relu_pre=False, residual=None, name="stage", gw=1.0, transposed=False, sums=None):
    """One layer of a chain on exact values: Stage -> Stage in front of the store (both conditions of the stage are the caller's to ask:
    exactness is asserted here, ``store_bf16`` asserts sensitivity).  ``residual``: a Stage.  ``gw``: the grid of scale-folded weights.
    ``sums``: the (sums, bound) of ``conv_sum`` on the same operands, where two epilogues share one convolution."""
    cout = w.shape[1] if transposed else w.shape[0]
    acc, bound = sums if sums is not None else conv_sum(st.v, w, stride, pad, transposed, name, gx=st.grid, gw=gw)
    v, g = epilogue(acc, bound, cout, bias, bn, relu, relu_pre, None if residual is None else residual.v, name, g_acc=st.grid * gw,
                    g_res=1.0 if residual is None else residual.grid, return_grid=True)
    return Stage(v, g)


def store_bf16(st, name="stage", sensitive=True):
    """The launch's bf16 store of an exact stage (RNE): coarser values on the same grid."""
    if sensitive:
        assert_sensitive(name, st.v)
    return Stage(rne_bf16(st.v).double(), st.grid)


def conv_ref(x, w, bias=None, bn=None, stride=1, pad=0, transposed=False, relu=False, relu_pre=False, residual=None, store="bf16", name="conv",
             force_f32=False, want_sensitive=True):
    """The whole layer: exact sums, exact epilogue, ONE rounding -- RNE to bf16 -- where the kernel stores bf16 (none for an fp32 store, where
    the exact value must itself be an fp32 number).  Returns the stored tensor as fp32 (N, C, [D,] H, W)."""
    cout = w.shape[1] if transposed else w.shape[0]
    acc, bound = conv_sum(x, w, stride, pad, transposed, name, force_f32=force_f32)
    v = epilogue(acc, bound, cout, bias, bn, relu, relu_pre, residual, name)
    if store == "bf16":
        if want_sensitive:
            assert_sensitive(name, v)
        return rne_bf16(v)
    f = v.float()
    assert torch.equal(f.double(), v), name + ": exact value is not an fp32 number"
    return f


def conv_operands(nd, N, cin, cout, k, sp, seed, transposed=False, xr=15, wr=15, br=63, rr=255, bias=True, bn=True, residual=None, x_relu=False):
    """Integer operands of one layer: activations in +-xr (>= 0 with ``x_relu``), weights in +-wr, an integer bias, a dyadic BatchNorm and an
    integer residual of shape ``residual`` in +-rr (rr <= 256: the residual of a bf16 plan is itself stored in bf16)."""
    g = gen(seed)
    x = ints((N, cin) + tuple(sp), xr, g, 0 if x_relu else None)
    w = ints(((cin, cout) if transposed else (cout, cin)) + (k,) * nd, wr, g)
    b = ints((cout,), br, g) if bias else None
    bnp = dyadic_bn(cout, g)[0] if bn else None
    res = ints(residual, rr, g) if residual is not None else None
    return x, w, b, bnp, res


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparison
def _ordered(t):
    """Bit pattern -> integer that is monotone in the value (ulp distance = difference)."""
    if t.dtype == torch.bfloat16:
        i = t.contiguous().view(torch.int16).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def bits_differ(got, want):
    assert got.dtype == want.dtype and got.dtype in (torch.float32, torch.bfloat16), (got.dtype, want.dtype)
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    return got.contiguous().view(it) != want.contiguous().view(it)


def assert_bits_equal(name, got, want, channels_last=False):
    """Compare BIT PATTERNS (fp32 or bf16 words; an fp32 view of bf16 data compares the same).  ``got`` / ``want``: (N, C, [D,] H, W), or
    (N, D, H, W, C) with ``channels_last``.  On failure reports the number of differing words, the first differing (n, d, h, w, c) and the
    largest distance in ulps.  The mismatch count is recorded under ``name`` through gpu_util.record, so it lands in the parity report."""
    got = torch.as_tensor(got).detach().cpu()
    want = torch.as_tensor(want).detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s != %s" % (name, tuple(got.shape), tuple(want.shape))
    if not channels_last and got.dim() >= 4:
        if got.dim() == 4:
            got, want = got.unsqueeze(2), want.unsqueeze(2)
        got, want = got.permute(0, 2, 3, 4, 1), want.permute(0, 2, 3, 4, 1)
    got, want = got.contiguous(), want.contiguous()
    diff = bits_differ(got, want)
    n = int(diff.sum())
    gpu_util.record(name, {"mismatching_words": n, "words": diff.numel()})
    if n:
        first = tuple(int(v) for v in diff.nonzero()[0])
        if got.dtype == torch.float32 and bool(bf16_representable(got).all()) and bool(bf16_representable(want).all()):
            ulps = (_ordered(got.to(torch.bfloat16)) - _ordered(want.to(torch.bfloat16))).abs()          # bf16 words carried in fp32
        else:
            ulps = (_ordered(got) - _ordered(want)).abs()
        raise AssertionError("%s: %d of %d words differ (%.2f %%), first at (n, d, h, w, c) = %s: got %r want %r, largest distance %d ulp"
                             % (name, n, diff.numel(), 100.0 * n / diff.numel(), first, float(got[first]), float(want[first]), int(ulps.max())))
    return 0


class Collector:
    """Runs every comparison of a test before failing it, so that one GPU run shows all mismatches of a kernel family."""

    def __init__(self):
        self.failed = []

    def bits(self, name, got, want, channels_last=False):
        try:
            assert_bits_equal(name, got, want, channels_last)
            return True
        except AssertionError as e:
            self.failed.append(str(e))
            return False

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None and self.failed:
            raise AssertionError("%d mismatching comparisons:\n" % len(self.failed) + "\n".join(self.failed))
        return False
