// Kernel selection of the plan hosts (include/lt_hip.h: lt_sel_*): which fused launch covers a layer or block, how many split-K tap groups a
// convolution is cut into, and the fragment layout its weights are packed in.  lt_engine.PlanBuilder and the plan-level ABI (plan.hip) both call
// these, so the two hosts record the same plan.  Where a kernel has no fallback (the column walk of lt_conv_skip_fwd, conv2d_halo_kernel for a layer
// packed in layout 2), the geometry test is the dispatcher's own (conv_common.h).
//
// Host-only code: no kernel, no device call.
#include "conv_common.h"

using namespace lt;

namespace {

bool wshape_is(const lt_wshape* w, int nd, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4 = 0) {
    const int64_t s[5] = {s0, s1, s2, s3, s4};
    if (w->nd != nd) return false;
    for (int i = 0; i < nd; ++i)
        if (w->s[i] != s[i]) return false;
    return true;
}

bool pointwise(const lt_wshape* w) {
    for (int i = 2; i < w->nd; ++i)
        if (w->s[i] != 1) return false;
    return true;
}

}  // namespace

extern "C" int lt_sel_conv_skip(int32_t dtype, const int32_t x[5], const lt_wshape* w, const int32_t skip_x[5], const lt_wshape* skip_w) {
    if (dtype != LT_BF16 || env_on("LT_NO_CONV_SKIP") || env_on("LT_HALO_NO_COL") || env_on("LT_HALO_NO_PERSIST") || env_on("LT_CONV_NO_HALO")) return 0;
    if (!wshape_is(w, 5, 32, 32, 3, 3, 3) || !wshape_is(skip_w, 5, 32, 16, 1, 1, 1)) return 0;
    const int N = x[0], D = x[1], H = x[2], W = x[3];
    if (x[4] != 32 || skip_x[0] != N || skip_x[1] != D || skip_x[2] != H || skip_x[3] != W || skip_x[4] != 16) return 0;
    // batches beyond 2^31 elements run as sample chunks inside the entry point: every chunk has to fit the kernel
    const int nc = lt_conv_chunk_samples(N, (long long)D * H * W * 32);
    if (nc < 1) return 0;
    return halo_col_fits(nc, D, H, W) && halo_col_fits(N - (N - 1) / nc * nc, D, H, W);
}

extern "C" int lt_sel_halo7_col(int32_t dtype, const int32_t x[5]) {
    if (dtype != LT_BF16 || x[4] != 32 || env_on("LT_HALO_NO_COL7")) return 0;
    return halo7_col_fits(x[0], x[1], x[2], x[3]);
}

extern "C" int lt_sel_halo2d_mfma(int32_t tile_rows, int32_t nphase) {
    if ((tile_rows != 8 && tile_rows != 4) || (nphase != 1 && nphase != 4) || (tile_rows == 4 && nphase == 4)) return 0;
    return halo2d_mfma(tile_rows, nphase);
}

extern "C" int lt_sel_halo_col_mfma(int32_t kind) { return kind < 0 || kind > 2 ? 0 : halo_col_mfma(kind); }

extern "C" int lt_sel_conv_cat2(int32_t dtype, const int32_t t2[5], const lt_wshape* we, const int32_t x[5], const lt_wshape* wd, int32_t s) {
    if (dtype != LT_BF16 || env_on("LT_NO_CONV_CAT2") || env_on("LT_CONV_NO_V7") || env_on("LT_CONV_NO_V3")) return 0;
    const int N = t2[0], Ho = t2[2], Wo = t2[3], P = t2[4];
    if (t2[1] != 1 || we->nd != 4 || wd->nd != 4 || !pointwise(we) || !pointwise(wd)) return 0;
    const long long Cc = we->s[0], Cin2 = wd->s[1];
    if (we->s[1] != P || wd->s[0] != Cc || (s != 1 && s != 2) || x[0] != N || x[1] != 1 || x[2] != Ho * s || x[3] != Wo * s || x[4] != Cin2) return 0;
    if (P % 32 || Cin2 % 32 || (P + Cin2) % 64 || Cc % 256 || (P & (P - 1))) return 0;
    // one kernel with 288 x 256 tiles, one workgroup per CU: below ~200 tiles (lt_conv_fwd's own rule for that tile) the separate launches on smaller
    // tiles fill the chip better
    const long long tiles = (((long long)N * Ho * Wo + 287) / 288) * (Cc / 256);
    if (tiles < 200 && !env_on("LT_CAT2_ANY_SIZE")) return 0;
    return (long long)N * Ho * Wo * Cc < (1ll << 31) && (long long)N * x[2] * x[3] * Cin2 < (1ll << 31);
}

// V2V's 128 -> 128 layers at the 8^3 / 4^3 / 2^3 levels: 18 launches of ~30 us each whatever the batch, K = 3456 a 54-step latency chain for the one or
// few workgroups the few output rows give.  S is chosen so that tiles x S fills the chip (<= 8: lt_conv_fwd's phase limit).
extern "C" int lt_sel_splitk_slices(const lt_conv_desc* d, const lt_wshape* w, int32_t transposed) {
    if (d->dtype != LT_BF16 || transposed || (d->flags & (LT_EPI_STORE_F32 | LT_EPI_SIGMOID)) || env_on("LT_CONV_NO_SPLITK")) return 1;
    if (w->nd != 5 || w->s[2] != 3 || w->s[3] != 3 || w->s[4] != 3) return 1;
    for (int i = 0; i < 3; ++i)
        if (d->stride[i] != 1 || d->pad[i] != 1) return 1;
    if (d->Cin < 128 || d->Cin % 64 || d->Cout % 4 || d->Cout != d->cout_pad || d->D * d->H * d->W > 512) return 1;
    const long long rows = (long long)d->N * d->Do * d->Ho * d->Wo;
    const int bm = rows >= 8192 ? 128 : 64;
    const long long tiles = ((rows + bm - 1) / bm) * (d->cout_pad / bm);
    const long long S = 256 / tiles;
    return S > 8 ? 8 : S < 1 ? 1 : (int)S;
}

extern "C" int lt_sel_bottleneck(int32_t dtype, const int32_t x[5], const lt_wshape w[3], const int32_t strides[3]) {
    if (dtype != LT_BF16 || env_on("LT_NO_BNECK")) return 0;
    if (x[1] != 1 || strides[0] != 1 || strides[1] != 1 || strides[2] != 1) return 0;
    const int C = x[4];
    const int64_t P = w[0].s[0];
    if (!((C == 256 && P == 64) || (C == 512 && P == 128))) return 0;
    if (!wshape_is(&w[0], 4, P, C, 1, 1) || !wshape_is(&w[1], 4, P, P, 3, 3) || !wshape_is(&w[2], 4, C, P, 1, 1)) return 0;
    return x[2] % 8 == 0 && x[3] % 16 == 0 && (long long)x[0] * x[2] * x[3] * C < (1ll << 31);
}

extern "C" int lt_sel_bottleneck_ds(int32_t dtype, const int32_t x[5], const lt_wshape w[3], const int32_t strides[3], const lt_wshape* wd, int32_t sd) {
    if (dtype != LT_BF16 || env_on("LT_NO_BNECK") || env_on("LT_NO_BNECK_DS")) return 0;
    if (x[1] != 1 || strides[0] != 1 || strides[1] != 1 || strides[2] != 1 || sd != 1) return 0;
    if (x[4] != 64 || !wshape_is(&w[0], 4, 64, 64, 1, 1) || !wshape_is(&w[1], 4, 64, 64, 3, 3) || !wshape_is(&w[2], 4, 256, 64, 1, 1) ||
        !wshape_is(wd, 4, 256, 64, 1, 1))
        return 0;
    return x[2] % 8 == 0 && x[3] % 16 == 0 && (long long)x[0] * x[2] * x[3] * 256 < (1ll << 31);
}

extern "C" int lt_sel_expand_reduce(int32_t dtype, const int32_t t2[5], const int32_t res[5], const lt_wshape* we, const lt_wshape* wr) {
    if (dtype != LT_BF16 || env_on("LT_NO_XR")) return 0;
    if (t2[1] != 1 || res[1] != 1 || t2[0] != res[0] || t2[2] != res[2] || t2[3] != res[3] || res[4] != 1024 || t2[4] != 256) return 0;
    // one tile per workgroup and one workgroup per CU.  With 96-row tiles only, 1 / 2 samples (24 / 48 tiles) lost 8 % / 2.5 % end to end to the two
    // launches (144-row tiles x 4 column tiles, two workgroups per CU) and the builder fused from 64 tiles on; the launcher now picks 64- and 32-row tiles
    // for small row counts (measured, forward samples/s, 96 / 64 / 32-row tiles / two launches: 1 sample 277 / 286 / 297 / 301, 2 samples 446 / 461 / 470 /
    // 454, 5 samples 857 / 876 / 836 / 827, 10 samples 1186 / 1135 / 1122 / 1104), so the seam is fused from 2 samples = 36 tiles of 96 rows on
    if ((long long)t2[0] * t2[2] * t2[3] < 36 * 96 && !env_on("LT_XR_ANY_SIZE")) return 0;
    return wshape_is(we, 4, 1024, 256, 1, 1) && wshape_is(wr, 4, 256, 1024, 1, 1);
}

extern "C" int lt_sel_stem_pool(int32_t dtype, const int32_t x[5], const lt_wshape* w, int32_t stride, int32_t pad, const int32_t pool[3]) {
    return dtype == LT_BF16 && x[1] == 1 && x[4] == 8 && w->nd == 4 && w->s[2] == 7 && w->s[3] == 7 && w->s[0] == 64 && w->s[1] <= 8 && stride == 2 &&
           pad == 3 && pool[0] == 3 && pool[1] == 2 && pool[2] == 1;
}

extern "C" int lt_sel_pwchain(int32_t dtype, const int32_t x[5], int32_t nlayers, const lt_wshape* w) {
    if (dtype != LT_BF16 || nlayers < 1 || nlayers > LT_PWCHAIN_MAX || x[4] != 32) return 0;
    if ((long long)x[0] * x[1] * x[2] * x[3] % 64) return 0;
    int64_t cin = 32;
    for (int i = 0; i < nlayers; ++i) {
        if (!pointwise(&w[i]) || w[i].s[1] != cin || w[i].s[0] > 32 || (i + 1 < nlayers && w[i].s[0] != 32)) return 0;
        cin = w[i].s[0];
    }
    return 1;
}

extern "C" int lt_sel_frag_layout(const lt_conv_desc* d, const lt_wshape* w, int32_t transposed, int32_t has_residual) {
    if (d->dtype != LT_BF16) return 0;
    // ResNet layer3's 3x3 256 -> 256 on 24-wide maps and the 4x4 / stride-2 transposed convolutions 256 -> 256 of the head (four parities of 2 x 2 taps),
    // from 60 tiles of 8 x 24 pixels on (= 5 samples of 4 views; measured with the threshold off: 799.9 -> 811.3 samples/s at 5 samples, 1145 -> 1172 at
    // 10, 1406 -> 1428 at 32 -- a tile is a ~40 us serial chain, so a handful of them loses to the small implicit-GEMM tiles): conv2d_halo_kernel, input
    // halo resident in LDS
    const bool w3x3 = !transposed && wshape_is(w, 4, 256, 256, 3, 3) && d->W == 24;
    const bool w4x4t = transposed && wshape_is(w, 4, 256, 256, 4, 4) && !env_on("LT_DECONV_NO_H2D");
    if ((w3x3 || w4x4t) && d->tile == LT_TILE_AUTO && !has_residual && !env_on("LT_CONV_NO_H2D") && !env_on("LT_CONV_V1") &&
        ((long long)d->N * (d->H / 8) * (d->W / 24) >= 60 || env_on("LT_H2D_ANY_SIZE")) && halo2d_fits(conv_args_of(*d), d->cout_pad, d->nphase))
        return 2;
    // the 288-row layers: fragment order of the 32x32x16 MFMA (conv_igemm7: +1 % end to end over conv_igemm6, 3x3 256->256 90.8 -> 87.4 us, 1x1
    // 1024->256 50.9 -> 48.2 us inside the forward); the short-K pointwise layers stay on the 144-row variant of conv_igemm6 and its 16x16x32 order
    // (measured: conv_igemm7 103.6 vs 85.6 us on 256->1024)
    if (d->cout_pad % 256 == 0 && d->k_pad % 64 == 0) {
        const bool short_pw = pointwise(w) && d->k_pad <= 256 && !transposed;
        return !env_on("LT_CONV_NO_V7") && !short_pw ? 3 : 1;
    }
    // V2V's 3x3x3 64 -> 64, 32 -> 64, 128 -> 128, 16 -> 32: fragments of the transposed product for conv3d_halo_wreg_kernel
    const bool wreg = wshape_is(w, 5, 64, 64, 3, 3, 3) || wshape_is(w, 5, 64, 32, 3, 3, 3) || wshape_is(w, 5, 128, 128, 3, 3, 3) || wshape_is(w, 5, 32, 16, 3, 3, 3);
    if (transposed || !wreg || d->Cin != w->s[1]) return 0;
    for (int i = 0; i < 3; ++i)
        if (d->stride[i] != 1 || d->pad[i] != 1) return 0;
    return 2;
}
