// Stride-1 "same" 3D convolution (3^3 / 7^3) for the V2V hourglass: the input HALO TILE lives in LDS.
//
// The implicit-GEMM kernels stream one K step of the im2col matrix per barrier, i.e. every input voxel crosses
// L2 -> LDS once per filter tap (27x / 343x).  At the 64^3 / 32^3 levels of V2V the GEMM is narrow (16..64 output
// channels), so that stream -- not the MFMAs -- sets the time (measured: 3^3 32->32 at 64^3 = 350 TF/s, 7^3 = 330 TF/s).
// Here a workgroup owns a TD x TH x TW block of output voxels (256 GEMM rows), DMAs the (T+K-1)^3 input halo into
// LDS ONCE (zero filled outside the volume), and then walks the taps: the A fragment of tap (kd,kh,kw) is the same
// LDS image read at a shifted voxel index, so the per-tap traffic is LDS -> VGPR only.  Weights stream through a
// double-buffered LDS ring, a few taps per barrier.
//
// LDS images (both filled by LDS-DMA, so both are lane-linear and swizzled on the SOURCE side):
//   halo   : voxel-major (row pitch PW voxels), CINB = Cin*sizeof(T) bytes per voxel = NVV 16-byte vectors; vector lv of the
//            voxel at halo position (hd,hh,hw) is stored in slot lv ^ f, f = (FA*hh + FB*hd + ((hw + FC*hh) >> FSH)) % NVV.
//            The constants per (kernel size, CINB, MFMA shape) were found by exhaustive search over all taps and all
//            ds_read_b128 lane groups (tools/halo_bank_search.py): every A-fragment read is bank-conflict free (the
//            linear (hv/VPR)%NVV swizzle of the first version was 3-way conflicted: rows of a lane group are 4 partial
//            lines of the tile, not 16 consecutive voxels);
//   weights: per tap a [cout_pad][CINB] slab, slot lv ^ ((-(col/VPR)) % NVV) (conflict free for both MFMA shapes).
// Weight ring: NBUF chunk buffers, NBUF-1 chunks of DMA in flight (counted vmcnt), one barrier per chunk.
//
// One unit per kernel family, each with its kernels, their launchers and one entry point in namespace lt; conv3d_halo.h has what they share (geometry,
// MFMA step, kernel arguments, staged epilogue).  This unit is the dispatcher:
//   conv3d_halo_col.hip    conv3d_halo_col_kernel, conv3d_halo_persist_kernel     conv3d_halo_col_launch
//   conv3d_halo_wreg.hip   conv3d_halo_wreg_kernel (and lt_conv_pack_weights_t32)  conv3d_halo_wreg_try
//   conv3d_halo7.hip       conv3d_halo7_col_kernel, conv3d_halo7b_kernel          conv3d_halo7_launch
//   conv3d_halo_tile.hip   conv3d_halo_kernel, every row below that names it      conv3d_halo_tile_try
//
// Dispatch (conv3d_halo_try below; the first row that matches launches, and an A/B switch in brackets sends its row's layers on to the rows below):
//   bf16 3^3 32->32, >= 1024 tiles, count % 8 == 0    [LT_HALO_NO_PERSIST]
//     every workgroup gets whole columns of >= 2 tiles  conv3d_halo_col_kernel       column walk, ring of 4-plane halo groups, epilogue under the next
//                                                       [LT_HALO_NO_COL]             tile's MFMAs (also: fp32 store, computed skip residual); 16x16x32 MFMAs
//                                                                                    except for the fp32 store (LT_HALO_COL_MF32=1: 32x32x16, same kernel)
//     else                                              conv3d_halo_persist_kernel   persistent, weights resident, double-buffered halo
//   bf16 3^3 64->64, 16->32, 32->64, 128->128          conv3d_halo_wreg_kernel      halo-only LDS, weights as fragments from global memory
//     with fragment-order weights  [LT_HALO_NO_WREG]
//   fp8  3^3 64->64, 32->32, 32->64                    conv3d_halo_kernel, LDR      one tile per workgroup, weight ring in LDS, waves 4-7 are loaders
//   bf16 3^3 64->64, 32->32, 16->32, 32->64            conv3d_halo_kernel, LDR
//   bf16 7^3 32->16
//     >= 256 whole columns of >= 2 tiles, count % 8 == 0 conv3d_halo7_col_kernel      column walk, ten-plane halo ring, epilogue under the next plane group
//                                                       [LT_HALO_NO_COL7]
//     else                                              conv3d_halo7b_kernel         one tile per workgroup, loader waves, kd-register-blocked
//   bf16 7^3 16->32  [LT_HALO_NO_D7]                   conv3d_halo_kernel, PD 2     fragment ring two taps deep
//   fp32 3^3 32->32  [LT_HALO_F3=1]                    conv3d_halo_kernel, NPH 2    two channel phases of 16, row chunks
//   fp32 3^3 32->32, 16->32                            conv3d_halo_kernel           row chunks / plane chunks
//   fp32 7^3 32->16, 16->32  [LT_HALO_NO_F7]           conv3d_halo_kernel           NPH 2 with the fragment ring / one phase, one-tap lookahead
//   anything else: 0, the caller takes the implicit-GEMM path
#include "conv3d_halo.h"

#ifdef LT_TRACE
// profiling build: conv3d_halo_col.hip and conv3d_halo7.hip have a trace buffer each; lt_trace_read_halo reads the one whose unit launched last
namespace { int g_trace_last = 0; }   // 0: conv3d_halo_col.hip, 1: conv3d_halo7.hip
#define LT_TRACE_LAST(u_) g_trace_last = (u_)
#else
#define LT_TRACE_LAST(u_) (void)0
#endif

namespace lt {

// Returns 1 and launches when the problem matches one of the instantiated halo configurations, 0 when the caller should
// fall back to the implicit-GEMM path, negative on error.
int conv3d_halo_try(int dtype, const ConvArgs& c, int cout_pad, int nphase, bool forced, hipStream_t s) {
    const PhaseArg& p0 = c.phase[0];
    if (nphase != 1 || c.sd != 1 || c.sh != 1 || c.sw != 1 || c.osd != 1 || c.osh != 1 || c.osw != 1) return 0;
    if (p0.ood || p0.ooh || p0.oow || c.D != c.Do || c.H != c.Ho || c.W != c.Wo || c.OD != c.Do || c.OH != c.Ho || c.OW != c.Wo) return 0;
    if (c.flags & LT_EPI_SIGMOID) return 0;
    // fp32 output (LT_EPI_STORE_F32: the mixed-precision training step) exists in the column-walk kernel only, and without a residual (the kernels read
    // the residual in the activation type)
    const bool f32_out = (c.flags & LT_EPI_STORE_F32) != 0;
    if (f32_out && (c.res || dtype != LT_BF16)) return 0;
    int ks = 0;
    if (p0.ntaps == 27 && c.pd == 1 && c.ph == 1 && c.pw == 1) ks = 3;
    else if (p0.ntaps == 343 && c.pd == 3 && c.ph == 3 && c.pw == 3) ks = 7;
    else return 0;
    constexpr int TD = HaloTile::TD, TH = HaloTile::TH, TW = HaloTile::TW;
    if (c.D % TD || c.H % TH || c.W % TW) return 0;
    const long long nblk = (long long)c.N * (c.D / TD) * (c.H / TH) * (c.W / TW);
    if (nblk < 256 && !forced) return 0;   // too few workgroups: the 64x64 implicit-GEMM tile fills the chip better
    HaloArgs a;
    a.x = c.x; a.w = p0.w; a.wfrag = p0.wfrag_t; a.y = c.y; a.res = c.res; a.bias = c.bias; a.scale = c.scale; a.shift = c.shift;
    a.N = c.N; a.D = c.D; a.H = c.H; a.W = c.W; a.Cout = c.Cout; a.ldc = c.ldc; a.k_pad = c.k_pad; a.flags = c.flags;
    a.tiles_d = c.D / TD; a.tiles_h = c.H / TH; a.tiles_w = c.W / TW;
    a.xcd_pin = (c.N % 8 == 0) ? 1 : 0;
    a.skip_x = c.skip_x; a.skip_w = c.skip_w;
    const bool bf = dtype == LT_BF16;
    if (c.skip_x && (f32_out || c.res || (c.flags & LT_EPI_RELU_PRE) || !bf)) return LT_ERR_UNSUPPORTED;
    // persistent variant: needs a few tiles per workgroup to amortise the weight load, and total % 8 == 0 for the XCD dealing
    static const bool no_persist = env_on("LT_HALO_NO_PERSIST");   // A/B
    if (bf && ks == 3 && cout_pad == 32 && c.Cout == 32 && c.ldc % 4 == 0 && c.Cin == 32 && nblk >= 1024 && nblk % 8 == 0 && !no_persist) {
        // column walk (sliding plane window + overlapped epilogue) when every workgroup gets whole columns of >= 2 tiles (LT_HALO_NO_COL: A/B, read per call)
        const bool column_walk = !env_on("LT_HALO_NO_COL") && halo_col_fits(c.N, c.D, c.H, c.W) && c.ldc % 8 == 0;
        if (!column_walk) {
            if (c.skip_x) return LT_ERR_UNSUPPORTED;
            if (f32_out) return 0;
        }
        LT_TRACE_LAST(0);
        int rc = conv3d_halo_col_launch(a, column_walk, s);
        return rc == LT_OK ? 1 : rc;
    }
    if (c.skip_x) return LT_ERR_UNSUPPORTED;             // the computed residual exists in the column-walk kernel only
    if (f32_out) return 0;
    // halo-only LDS, weights as fragments from global memory (lt_conv_pack_weights_t32): 64 -> 64, 16 -> 32, 32 -> 64, 128 -> 128
    if (bf && ks == 3 && c.Cout == cout_pad && c.ldc % 8 == 0 && a.wfrag && !env_on("LT_HALO_NO_WREG")) {
        int rc = conv3d_halo_wreg_try(c.Cin, cout_pad, a, s);
        if (rc) return rc;
    }
    if (bf && ks == 7 && c.Cin == 32 && cout_pad == 16) {
        // column walk (plane ring, epilogue under the next plane group) when every workgroup gets whole columns of >= 2 tiles (LT_HALO_NO_COL7: A/B, read per call)
        LT_TRACE_LAST(1);
        int rc = conv3d_halo7_launch(a, !env_on("LT_HALO_NO_COL7") && halo7_col_fits(c.N, c.D, c.H, c.W), s);
        return rc == LT_OK ? 1 : rc;
    }
    // every other layer: the rows of the one-tile kernel, or none
    return conv3d_halo_tile_try(dtype, ks, c.Cin, cout_pad, a, s);
}

}  // namespace lt

#ifdef LT_TRACE
extern "C" int lt_trace_read_halo(long long* dst, int n) {
    return g_trace_last == 1 ? lt::conv3d_halo7_trace_read(dst, n) : lt::conv3d_halo_col_trace_read(dst, n);
}
#endif
