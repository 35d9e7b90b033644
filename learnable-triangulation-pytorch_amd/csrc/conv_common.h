// Shared pieces of the implicit-GEMM and halo convolution kernels: the kernel-side argument block (ConvArgs), the host predicates that say which
// layers a kernel family covers, the MFMA wrappers per operand type and tile shape, and the entry points of every family for the dispatcher in
// conv_igemm.hip (register-staged v1): conv_igemm2 (LDS-DMA staged, LDS-transposed vector epilogue), conv_igemm3 (288-row tiles: v3 / v5 / v6),
// conv_igemm7 (288 x 256 on 32x32x16 MFMAs), conv_pw (single-tap streaming), conv2d_halo and conv3d_halo (input halo resident in LDS).
// The wave-level asm primitives these kernels share live in wave_prims.h, which includes this header.
#pragma once
#include "lt_common.h"

namespace lt {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct PhaseArg {
    const void* w;
    const void* wfrag;   // the same weights in MFMA B-fragment order (lt_conv_pack_weights, layout 1), or null
    const void* wfrag_t; // ... in the order of the transposed product (lt_conv_pack_weights_t32, layout 2), or null
    const void* wfrag32; // ... in B-fragment order of the 32x32x16 MFMA (lt_conv_pack_weights32, layout 3), or null
    const int4* taps;
    int ntaps;
    int ood, ooh, oow;
};

struct ConvArgs {
    const void* x;
    void* y;
    const void* res;
    const float* bias;
    const float* scale;
    const float* shift;
    int N, D, H, W, Cin, log2Cin;
    int Do, Ho, Wo;
    int sd, sh, sw, pd, ph, pw;
    int OD, OH, OW, osd, osh, osw;
    int Cout, ldc, k_pad, flags;
    int M;        // N*Do*Ho*Wo
    int tiles_n;  // cout_pad / BN
    int stages;   // requested LDS-DMA ring depth (0 = auto)
    PhaseArg phase[LT_CONV_MAX_PHASES];
    const void* skip_x;   // lt_conv_skip_fwd: the residual is computed as W_skip . skip_x[voxel] (conv3d_halo_col_kernel only), else null
    const void* skip_w;
    // lt_conv_cat2_fwd (conv_igemm7 MODE 3): a 1x1 convolution over the channel concatenation of TWO tensors -- K steps below Cin / 32 read x, the rest read
    // x2 at pixel (n, oh * s2, ow * s2) of its H2 x W2 map (Cin2 channels per pixel); null = off
    const void* x2;
    int Cin2, H2, W2, s2;
};

// The descriptor's geometry, flags and phases as kernel arguments (tensor pointers, M, log2Cin and the second sources are the caller's).
inline ConvArgs conv_args_of(const lt_conv_desc& d) {
    ConvArgs a = {};
    a.N = d.N; a.D = d.D; a.H = d.H; a.W = d.W; a.Cin = d.Cin;
    a.Do = d.Do; a.Ho = d.Ho; a.Wo = d.Wo;
    a.sd = d.stride[0]; a.sh = d.stride[1]; a.sw = d.stride[2];
    a.pd = d.pad[0]; a.ph = d.pad[1]; a.pw = d.pad[2];
    a.OD = d.OD; a.OH = d.OH; a.OW = d.OW;
    a.osd = d.out_stride[0]; a.osh = d.out_stride[1]; a.osw = d.out_stride[2];
    a.Cout = d.Cout; a.ldc = d.ldc; a.k_pad = d.k_pad; a.flags = d.flags; a.tiles_n = 1; a.stages = d.stages;
    for (int p = 0; p < d.nphase && p < LT_CONV_MAX_PHASES; ++p) {
        const lt_conv_phase& ph = d.phase[p];
        a.phase[p].w = ph.weight;
        a.phase[p].wfrag = ph.weight_frag_layout == 1 ? ph.weight_frag : nullptr;
        a.phase[p].wfrag_t = ph.weight_frag_layout == 2 ? ph.weight_frag : nullptr;
        a.phase[p].wfrag32 = ph.weight_frag_layout == 3 ? ph.weight_frag : nullptr;
        a.phase[p].taps = (const int4*)ph.taps; a.phase[p].ntaps = ph.ntaps;
        a.phase[p].ood = ph.out_off[0]; a.phase[p].ooh = ph.out_off[1]; a.phase[p].oow = ph.out_off[2];
    }
    return a;
}

// The geometry conv3d_halo_col_kernel (the column walk, and with it lt_conv_skip_fwd) covers: tiles of 4 x 8 x 8 voxels, at least 1024 of them in
// multiples of 8 (XCD dealing), and whole columns of >= 2 tiles for every workgroup (>= 256 columns, a multiple of 8).  conv3d_halo_try checks it at
// launch time, lt_sel_conv_skip at plan time for every sample chunk.
inline bool halo_col_fits(long long N, int D, int H, int W) {
    if (D % 4 || H % 8 || W % 8) return false;
    const long long nblk = N * (D / 4) * (H / 8) * (W / 8), cols = N * (H / 8) * (W / 8);
    return nblk >= 1024 && nblk % 8 == 0 && D / 4 >= 2 && cols % 8 == 0 && cols >= 256;
}

// The geometry conv3d_halo7_col_kernel (the column walk of the 7^3 32 -> 16 layer) covers: tiles of 4 x 8 x 8 voxels, columns of >= 2 tiles, and whole
// columns for every workgroup of the persistent grid (>= 256 columns -- the CU count halo_col_fits assumes -- in a multiple of 8 for the XCD dealing).
// conv3d_halo_try checks it at launch time; anything else stays on the one-tile kernel.
inline bool halo7_col_fits(long long N, int D, int H, int W) {
    if (D % 4 || H % 8 || W % 8) return false;
    const long long cols = N * (H / 8) * (W / 8);
    return D / 4 >= 2 && cols % 8 == 0 && cols >= 256 && cols < (1ll << 31);
}

// The "plain pointwise" layer: its one phase has one tap at offset 0, unit strides, no padding, an output grid equal to the input grid, and dense K
// (k_pad == Cin) -- GEMM row m is input pixel m, so the kernels' pointwise modes need no tap table.  (A caller with several phases asks per phase.)
inline bool plain_pointwise(const ConvArgs& a) {
    const PhaseArg& p0 = a.phase[0];
    return p0.ntaps == 1 && a.sd == 1 && a.sh == 1 && a.sw == 1 && a.pd == 0 && a.ph == 0 && a.pw == 0 && a.osd == 1 && a.osh == 1 && a.osw == 1 &&
           p0.ood == 0 && p0.ooh == 0 && p0.oow == 0 && a.OD == a.Do && a.OH == a.Ho && a.OW == a.Wo && a.D == a.Do && a.H == a.Ho && a.W == a.Wo &&
           a.k_pad == a.Cin;
}

// The layers conv2d_halo_kernel covers, whatever the weights and extra sources: 256 -> 256 dense channels, maps whose width is a multiple of 24 and
// whose height is a multiple of 8, iteration space == input grid, plain store; one phase of nine taps (a "same" 3x3 / stride 1 / pad 1) or four
// phases of four taps with output stride 2 (the 2 x 2-tap parities of a 4x4 / stride-2 / pad-1 transposed convolution, recorded with pad 0 and
// signed tap offsets).  conv2d_halo_try checks it at launch time, lt_sel_frag_layout at plan time (a 2D layer packed for it has no other kernel).
inline bool halo2d_fits(const ConvArgs& c, int cout_pad, int nphase) {
    if ((nphase != 1 && nphase != 4) || c.D != 1 || c.Do != 1 || c.OD != 1) return false;
    if (c.sh != 1 || c.sw != 1 || c.H != c.Ho || c.W != c.Wo || c.W % 24 || c.H % 8) return false;
    if (c.Cin != 256 || cout_pad != 256 || c.Cout != 256 || c.ldc % 8 || (c.flags & (LT_EPI_STORE_F32 | LT_EPI_SIGMOID)) || c.pd != 0) return false;
    if (nphase == 1 && (c.osh != 1 || c.osw != 1 || c.OH != c.Ho || c.OW != c.Wo || c.ph != 1 || c.pw != 1)) return false;
    if (nphase == 4 && (c.osh != 2 || c.osw != 2 || c.OH != 2 * c.Ho || c.OW != 2 * c.Wo || c.ph != 0 || c.pw != 0)) return false;
    for (int p = 0; p < nphase; ++p)
        if (c.phase[p].ntaps != (nphase == 1 ? 9 : 4) || c.phase[p].ood) return false;
    return true;
}

// The bf16 MFMA of conv2d_halo_kernel per instantiation (tile rows, phases): 16 = v_mfma_f32_16x16x32_bf16, 32 = 32x32x16.  The same MACs, cycles and
// operand bytes; the chip holds a higher clock on the 16x16x32 form (DESIGN.md "MFMA shape").  LT_H2D_MF32=1 (A/B, read per launch call): 32x32x16.
inline int halo2d_mfma(int tile_rows, int nphase) {
    (void)tile_rows; (void)nphase;
    return env_on("LT_H2D_MF32") ? 32 : 16;
}

// ... and of conv3d_halo_col_kernel per instantiation: kind 0 = bf16 store, 1 = computed skip residual, 2 = fp32 store (training: always 32x32x16).
// LT_HALO_COL_MF32=1 (A/B, read per launch call): 32x32x16.
inline int halo_col_mfma(int kind) {
#ifdef LT_TRACE
    return 32;          // the shader-clock accounting lives in the 32x32x16 form
#endif
    return kind == 2 || env_on("LT_HALO_COL_MF32") ? 32 : 16;
}

union V16 {
    uint4 u;
    f32x4 f;
    bf16x8 h;
};

template <typename T, int MF> struct Mma;
template <> struct Mma<float, 32> {
    typedef f32x16 acc_t;
    static __device__ __forceinline__ void run(acc_t& c, const V16& a, const V16& b) {
#pragma unroll
        for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.f[e], b.f[e], c, 0, 0, 0);
    }
};
template <> struct Mma<float, 16> {
    typedef f32x4 acc_t;
    static __device__ __forceinline__ void run(acc_t& c, const V16& a, const V16& b) {
#pragma unroll
        for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.f[e], b.f[e], c, 0, 0, 0);
    }
};
template <> struct Mma<bf16_t, 32> {
    typedef f32x16 acc_t;
    static __device__ __forceinline__ void run(acc_t& c, const V16& a, const V16& b) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, c, 0, 0, 0);
    }
};
template <> struct Mma<bf16_t, 16> {
    typedef f32x4 acc_t;
    static __device__ __forceinline__ void run(acc_t& c, const V16& a, const V16& b) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, c, 0, 0, 0);
    }
};

// fp8 (e4m3): a 16-byte fragment vector holds 16 K elements = two 8-byte operands of v_mfma_f32_*_fp8_fp8 (K = 16 / 32 per instruction; the K
// order inside a fragment group differs from the bf16 kernels', identically for both operands, which a sum over K does not see)
union V16Q {
    uint4 u;
    long q[2];
};
template <> struct Mma<fp8_t, 32> {
    typedef f32x16 acc_t;
    static __device__ __forceinline__ void run(acc_t& c, const V16& a, const V16& b) {
        V16Q qa, qb;
        qa.u = a.u; qb.u = b.u;
        c = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(qa.q[0], qb.q[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(qa.q[1], qb.q[1], c, 0, 0, 0);
    }
};
template <> struct Mma<fp8_t, 16> {
    typedef f32x4 acc_t;
    static __device__ __forceinline__ void run(acc_t& c, const V16& a, const V16& b) {
        V16Q qa, qb;
        qa.u = a.u; qb.u = b.u;
        c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(qa.q[0], qb.q[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(qa.q[1], qb.q[1], c, 0, 0, 0);
    }
};

// decode a GEMM row into (sample, od, oh, ow)
__device__ __forceinline__ void decode_row(const ConvArgs& a, int m, int& n, int& od, int& oh, int& ow) {
    int hw = a.Ho * a.Wo;
    int dhw = a.Do * hw;
    n = m / dhw;
    int r = m - n * dhw;
    od = r / hw;
    r -= od * hw;
    oh = r / a.Wo;
    ow = r - oh * a.Wo;
}

constexpr int ROW_BYTES = 128;  // K bytes per tile row per step
constexpr int LT_EPI_NO_RES_PREFETCH = 1 << 16;   // internal A/B switch (env LT_CONV_NO_RESPF), not part of the ABI
constexpr int LT_EPI_NO_XCD_REMAP = 1 << 17;      // internal A/B switch (env LT_CONV_NO_XCD)

// launchers implemented in conv_igemm2.hip, used by the dispatcher in conv_igemm.hip
int conv2_dispatch(int dtype, const ConvArgs& a, int cout_pad, int nphase, int max_taps, int tile, hipStream_t s);
// conv_igemm3.hip (288-row tile, 8 waves): 1 = launched, 0 = not applicable (fall back), < 0 = error
int conv3_try(int dtype, const ConvArgs& a, int cout_pad, int nphase, int max_taps, bool forced, hipStream_t s);
// conv_igemm7.hip (288 x 256 tile on 32x32x16 MFMAs, weights in layout 3): 1 / 0 / < 0 as above
int conv7_try(const ConvArgs& a, int cout_pad, int max_taps, bool pw, hipStream_t s);
// conv_pw.hip (streaming kernel for single-tap phases: 1x1x1 convs, 2x2x2 stride-2 deconvs): 1 / 0 / < 0 as above
int conv_pw_try(int dtype, const ConvArgs& a, int cout_pad, int nphase, hipStream_t s);
// conv2d_halo.hip (3x3 256 -> 256 on 24-wide maps, input halo in LDS, weights in layout 2): 1 / 0 / < 0 as above
int conv2d_halo_try(int dtype, const ConvArgs& a, int cout_pad, int nphase, hipStream_t s);
// conv3d_halo.hip (the dispatcher; one unit per kernel family behind it: conv3d_halo_col / _wreg / _tile.hip, conv3d_halo7.hip, declared in
// conv3d_halo.h): 1 = launched, 0 = not applicable (fall back), < 0 = error
int conv3d_halo_try(int dtype, const ConvArgs& a, int cout_pad, int nphase, bool forced, hipStream_t s);

}  // namespace lt
