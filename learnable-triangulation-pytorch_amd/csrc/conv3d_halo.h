// What the units of the 3D halo convolution share (conv3d_halo.hip has the overview and the dispatch table): the tile and LDS geometry, the MFMA step
// of one tap, the kernel arguments, the staged epilogue, and the entry point of every kernel family.  Everything in the unnamed namespaces is per unit
// -- a device symbol cannot span units without relocatable device code, so each unit has its own 64-byte zero page (and, in LT_TRACE builds, its own
// trace buffer).
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "wave_prims.h"

#ifndef LT_ACC64_MASK
#define LT_ACC64_MASK 3          // fp32 (parity) kernels: fp64 flush of the MFMA accumulators every LT_ACC64_MASK + 1 taps / K steps
#endif

using namespace lt;

namespace {

__device__ uint4 g_zero_page_h[4];   // 64 zero bytes: DMA source of padding voxels, and the 'residual' of layers without one

#ifdef LT_TRACE
// profiling build: shader-clock accounting of the persistent kernel's per-tile phases, written by wave 0 of every 8th workgroup:
// [total, top wait+barrier, halo issue, residual issue, tap loop, barrier, epilogue, tiles]
__device__ long long g_trace_h[8 * 64];

// this unit's buffer (the units whose kernels write one export this as their reader; lt_trace_read_halo picks the one that launched last)
inline int halo_trace_read(long long* dst, int n) {
    if (n > 8 * 64) n = 8 * 64;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_trace_h), (size_t)n * sizeof(long long)) != hipSuccess) return -2;
    return n;
}
#endif

// swizzle constants {FA, FB, FC, FSH, pitch multiple}
template <int KS, int CINB, int MF> struct HaloSwz { static constexpr int FA = 0, FB = 0, FC = 0, FSH = 1, PAD = 1; };   // (3, 64 B, 32x32)
template <> struct HaloSwz<7, 64, 16> { static constexpr int FA = 0, FB = 0, FC = 0, FSH = 0, PAD = 1; };
template <> struct HaloSwz<3, 128, 32> { static constexpr int FA = 3, FB = 0, FC = 2, FSH = 1, PAD = 1; };
template <> struct HaloSwz<3, 32, 32> { static constexpr int FA = 0, FB = 0, FC = 0, FSH = 2, PAD = 4; };
// (7, 32 B, 32x32) -- round 6: the input gradient of V2V's 7^3 front layer, 16 -> 32 -- takes the default: the 7^3 tap loop needs a swizzle that depends on kw only,
// and the best of those is 2-way conflicted (tools/halo_bank_search.py: 2.0 for every kw-only candidate; the conflict-free ones mix in kh)

// every 3D halo kernel computes a 4 x 8 x 8 block of output voxels per workgroup tile (256 GEMM rows, one d-plane per compute wave)
struct HaloTile { static constexpr int TD = 4, TH = 8, TW = 8; };

template <typename T, int KS, int CIN, int CP, int TPC, int NBUF>
struct HaloCfg : HaloTile {
    static constexpr int ES = sizeof(T);
    static constexpr int VEC = 16 / ES;
    // outputs / residuals are the operand type, except that fp8 (an operand type only: the 'fp8v2v' training step) stores bf16
    typedef typename std::conditional<sizeof(T) == 1, bf16_t, T>::type OT;
    static constexpr int OVEC = 16 / (int)sizeof(OT);
    static constexpr int CINB = CIN * ES;
    static constexpr int NVV = CINB / 16;          // 16-byte vectors per voxel
    static constexpr int VPR = 16 / NVV;           // voxels per 256-byte bank row
    static constexpr int MF = CP == 16 ? 16 : 32;
    typedef HaloSwz<KS, CINB, MF> SW;
    static constexpr int HD = TD + KS - 1, HH = TH + KS - 1, HW = TW + KS - 1;
    static constexpr int PW = (HW + SW::PAD - 1) / SW::PAD * SW::PAD;       // row pitch in voxels
    static constexpr int HV = HD * HH * PW;        // halo voxel slots
    static constexpr int HALO_BYTES = ((HV * CINB + 1023) / 1024) * 1024;   // whole DMA wave-instructions
    static constexpr int NTAPS = KS * KS * KS;
    static constexpr int NCH = (NTAPS + TPC - 1) / TPC;
    static constexpr int SLAB = CP * CINB;         // bytes of one tap's weights
    static constexpr int WCH = ((TPC * SLAB + 1023) / 1024) * 1024;
    static constexpr int G = MF == 32 ? NVV / 2 : NVV / 4;   // fragment groups per tap (K = Cin)
    static constexpr int SM = 64 / MF;             // sub-tiles per wave along M (wave = 64 rows)
    static constexpr int SN = CP / MF;
    static constexpr int NACC = MF == 32 ? 16 : 4;
    static constexpr int EP_LD = CP + 4;
    static constexpr int EP_BYTES = 4 * 64 * EP_LD * 4;
    static constexpr int MAIN_BYTES = HALO_BYTES + NBUF * WCH;
    static constexpr int LDS_BYTES = MAIN_BYTES > EP_BYTES ? MAIN_BYTES : EP_BYTES;
    static_assert(NVV >= 1 && (MF == 32 ? NVV >= 2 : NVV >= 4), "Cin too small for the MFMA K");
    static_assert((NVV & (NVV - 1)) == 0 && NVV <= 16, "NVV must be a power of two <= 16");
    static_assert(NBUF >= 2 && NBUF <= 4, "2..4 weight chunk buffers");
    static __device__ __forceinline__ int fswz(int hd, int hh, int hw) {
        return (SW::FA * hh + SW::FB * hd + ((hw + SW::FC * hh) >> SW::FSH)) & (NVV - 1);
    }
};

#ifdef LT_ABL_NO_MMA
#define LT_HMMA(c_, a_, b_) (void)0
#else
#define LT_HMMA(c_, a_, b_) Mma<T, MF>::run(c_, a_, b_)
#endif

// All MFMAs of one tap for a wave's SM x SN accumulator blocks over G fragment groups.  bf16: one MFMA per (group, block).  fp32 (round 6): a 16-byte
// fragment is FOUR exact-fp32 MFMAs (K pairs e = 0 .. 3); issued back to back on one accumulator they wait for each other (~10 % below the issue rate,
// measured in conv_igemm2's K loop: 4740 cycles for 64 MFMAs of 64) -- the K pair goes outermost, so that consecutive MFMAs write different blocks.  The
// summation order of every accumulator is unchanged (results are bit-identical).
template <typename T, int MF, int SM, int SN, int G, typename ACC, typename FA, typename FB>
__device__ __forceinline__ void mma_tap_blocks(ACC (&acc)[SM][SN], const FA& fa, const FB& fb) {
#if !defined(LT_ABL_NO_MMA)
    if constexpr (sizeof(T) == 4 && SM * SN > 1) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < SM; ++i)
#pragma unroll
                    for (int j = 0; j < SN; ++j) {
                        if constexpr (MF == 32) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g][i].f[e], fb[g][j].f[e], acc[i][j], 0, 0, 0);
                        else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[g][i].f[e], fb[g][j].f[e], acc[i][j], 0, 0, 0);
                    }
        return;
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < SM; ++i)
#pragma unroll
            for (int j = 0; j < SN; ++j) Mma<T, MF>::run(acc[i][j], fa[g][i], fb[g][j]);
#endif
}

}  // namespace

namespace lt {   // the one type that crosses units (the family entry points below take it)

struct HaloArgs {
    const void* x;
    const void* w;      // [cout_pad][k_pad], k = tap*Cin + ci (the lt_conv_fwd packing)
    const void* wfrag;  // the same weights packed by lt_conv_pack_weights_t32 (conv3d_halo_wreg_kernel), or null
    void* y;
    const void* res;
    const float* bias;
    const float* scale;
    const float* shift;
    int N, D, H, W, Cout, ldc, k_pad, flags;
    int tiles_d, tiles_h, tiles_w;   // per sample
    int xcd_pin;
    const void* skip_x;   // lt_conv_skip_fwd (column-walk kernel only): the residual is W_skip . skip_x[voxel] (16 channels per voxel), or null
    const void* skip_w;   // its weights in lt_conv_pack_weights_t32 order ([32][16] -> one fragment)
};

}  // namespace lt

namespace {

// per-column epilogue constants of the lane (column j*MF + lane % MF), loaded once per kernel, well before they are needed
template <int SN>
struct HaloCst {
    float bi[SN], sc[SN], sf[SN];
    __device__ __forceinline__ void load(const HaloArgs& a, int lane, int MF) {
#pragma unroll
        for (int j = 0; j < SN; ++j) {
            const int colj = j * MF + (lane & (MF - 1));   // < cout_pad: the constant arrays are padded
            bi[j] = a.bias ? a.bias[colj] : 0.f;
            sc[j] = a.scale ? a.scale[colj] : 1.f;
            sf[j] = a.shift ? a.shift[colj] : 0.f;
        }
    }
};

// Epilogue shared by the halo kernels (same scheme as conv_igemm2): (acc + bias)*scale + shift into this wave's fp32 LDS tile
// (64 rows, padded), then 16-byte vectors: optional pre-activation ReLU, residual, ReLU, store.  rp0..rp7: the lane's residual
// vectors when they were prefetched (pre_res), in named registers (an array was kept in scratch memory by hipcc).
template <typename T, int CP, int MF, int SM, int SN, int NACC, bool ACC64, typename ACC, typename DACC>
__device__ __forceinline__ void halo_epilogue(unsigned char* smem, const HaloArgs& a, int wave, int lane, int n, int d0, int h0, int w0,
                                              ACC& acc, DACC& dacc, bool pre_res, uint4 rp0, uint4 rp1, uint4 rp2, uint4 rp3, uint4 rp4,
                                              uint4 rp5, uint4 rp6, uint4 rp7, const HaloCst<SN>& cst) {
    constexpr int EP_LD = CP + 4, TH = HaloTile::TH, TW = HaloTile::TW;
    typedef typename std::conditional<sizeof(T) == 1, bf16_t, T>::type OT;          // fp8 operands: bf16 outputs and residuals
    constexpr int VEC_ = 16 / (int)sizeof(OT);
    // ---- epilogue (same scheme as conv_igemm2: per-wave fp32 LDS tile -> 16-byte vectors) ----
    float* ep = (float*)(smem + wave * (64 * EP_LD * 4));
#pragma unroll
    for (int j = 0; j < SN; ++j) {
        const int colj = j * MF + (lane & (MF - 1));
        const float bi = cst.bi[j], sc = cst.sc[j], sf = cst.sf[j];
#pragma unroll
        for (int i = 0; i < SM; ++i)
#pragma unroll
            for (int e = 0; e < NACC; ++e) {
                const int r = i * MF + ((MF == 32) ? ((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) : ((lane >> 4) * 4 + e));
                float val;
                if (ACC64) val = (float)((dacc[i][j][e] + (double)bi) * (double)sc + (double)sf);
                else val = (acc[i][j][e] + bi) * sc + sf;
                ep[r * EP_LD + colj] = val;
            }
    }
    // (the tile is wave-private and LDS operations of one wave execute in order: no barrier)

    const EpiFloors fl = epi_floors(a.flags);
    const bool has_res = a.res != nullptr;
    auto row_pix = [&](int r) -> size_t {   // r = row inside the workgroup tile
        const int tw = r % TW, th = (r / TW) % TH, td = r / (TW * TH);
        return (((size_t)n * a.D + d0 + td) * a.H + h0 + th) * a.W + w0 + tw;
    };
    constexpr int VECO = VEC_;              // fp32: 4 channels, bf16: 8 channels per 16 bytes
    if ((a.Cout % VECO == 0) && (a.ldc % VECO == 0)) {
        constexpr int LPR = CP / VECO, RPP = 64 / LPR;
        static_assert(RPP % TW == 0 && TW * TH == 64, "a wave owns one d-plane of the tile; an iteration advances whole rows of it");
        const int cq = (lane % LPR) * VECO;
        if (cq < a.Cout) {
            constexpr int NIT = 64 / RPP;
            // the wave's 64 rows are the d-plane td = wave of the tile: row lr + it*RPP -> (th, tw) = (lr / TW + it*RPP/TW, lr % TW),
            // so the element offset of iteration `it` is off0 + it * step (one 64-bit multiply per tile, not per row)
            const int lr = lane / LPR;
            const size_t off0 = ((((size_t)n * a.D + d0 + wave) * a.H + h0 + lr / TW) * a.W + w0 + lr % TW) * a.ldc + cq;
            const size_t step = (size_t)(RPP / TW) * a.W * a.ldc;
            const unsigned no_res = has_res ? 0u : 0x80008000u;   // zeros -> -0.0 pairs: v + -0.0 == v
            auto row = [&](int it, uint4 resv) {      // resv: this row's residual vector (zeros when there is none)
                const size_t off = off0 + it * step;
                const float* src = ep + (lr + it * RPP) * EP_LD + cq;
                uint4 ov;
                if constexpr (sizeof(OT) == 4) {
                    const float4 q = *(const float4*)src;
                    const float nr = has_res ? 0.f : -0.0f;
                    float4 o;
                    o.x = epi_apply(q.x, fl, has_res ? __uint_as_float(resv.x) : nr);
                    o.y = epi_apply(q.y, fl, has_res ? __uint_as_float(resv.y) : nr);
                    o.z = epi_apply(q.z, fl, has_res ? __uint_as_float(resv.z) : nr);
                    o.w = epi_apply(q.w, fl, has_res ? __uint_as_float(resv.w) : nr);
                    ov = make_uint4(__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w));
                } else {
                    const float4 q0 = *(const float4*)src, q1 = *(const float4*)(src + 4);
                    const float vv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                    const unsigned ru[4] = {resv.x | no_res, resv.y | no_res, resv.z | no_res, resv.w | no_res};
                    unsigned ou[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        ou[e] = pack_bf16x2(epi_apply(vv[2 * e], fl, __uint_as_float(ru[e] << 16)),
                                            epi_apply(vv[2 * e + 1], fl, __uint_as_float(ru[e] & 0xffff0000u)));
                    ov = make_uint4(ou[0], ou[1], ou[2], ou[3]);
                }
#ifdef LT_ABL_NO_STORE
                if (a.N < 0)
#endif
                *(uint4*)((OT*)a.y + off) = ov;
            };
            if (pre_res || !has_res) {
                if (NIT > 0) row(0, rp0);
                if (NIT > 1) row(1, rp1);
                if (NIT > 2) row(2, rp2);
                if (NIT > 3) row(3, rp3);
                if (NIT > 4) row(4, rp4);
                if (NIT > 5) row(5, rp5);
                if (NIT > 6) row(6, rp6);
                if (NIT > 7) row(7, rp7);
                if (NIT > 8) {   // fp32 with a narrow tile: no prefetch (PRE_OK false), rows 8.. have no residual here
#pragma unroll
                    for (int it = 8; it < NIT; ++it) row(it, make_uint4(0, 0, 0, 0));
                }
            } else {
                uint4 rv[NIT];
#pragma unroll
                for (int it = 0; it < NIT; ++it)      // all residual loads first: independent HBM round trips
                    rv[it] = *(const uint4*)((const OT*)a.res + off0 + it * step);
#pragma unroll
                for (int it = 0; it < NIT; ++it) row(it, rv[it]);
            }
        }
    } else {
        for (int idx = lane; idx < 64 * CP; idx += 64) {
            const int r = idx / CP, cc = idx - r * CP;
            if (cc >= a.Cout) continue;
            const size_t off = row_pix(64 * wave + r) * a.ldc + cc;
            const float rr = has_res ? elt<OT>::ld((const OT*)a.res + off) : -0.0f;
            elt<OT>::st((OT*)a.y + off, epi_apply(ep[r * EP_LD + cc], fl, rr));
        }
    }
}

}  // namespace

namespace lt {

// The entry point of every kernel family, one per unit.  conv3d_halo_try (conv3d_halo.hip) has checked the geometry, filled the HaloArgs and read the
// A/B switches that choose between families; what is left here is choosing an instantiation and launching it on `s`.
// conv3d_halo_tile.hip, conv3d_halo_kernel: the rows keyed by (dtype, ks, cin, cout_pad).  1 = launched, 0 = no row matches, < 0 = error
int conv3d_halo_tile_try(int dtype, int ks, int cin, int cout_pad, const HaloArgs& a, hipStream_t s);
// conv3d_halo_wreg.hip, conv3d_halo_wreg_kernel (bf16 3^3, a.wfrag set): 1 = launched, 0 = (cin, cout_pad) is not instantiated, < 0 = error
int conv3d_halo_wreg_try(int cin, int cout_pad, const HaloArgs& a, hipStream_t s);
// conv3d_halo_col.hip, bf16 3^3 32 -> 32 with resident weights: conv3d_halo_col_kernel (column_walk) or conv3d_halo_persist_kernel.  LT_OK or an error
int conv3d_halo_col_launch(const HaloArgs& a, bool column_walk, hipStream_t s);
// conv3d_halo7.hip, bf16 7^3 32 -> 16: conv3d_halo7_col_kernel (column_walk) or conv3d_halo7b_kernel.  LT_OK or an error
int conv3d_halo7_launch(const HaloArgs& a, bool column_walk, hipStream_t s);
#ifdef LT_TRACE
// the trace buffers of the two units whose kernels write one (lt_trace_read_halo); the return value of halo_trace_read
int conv3d_halo_col_trace_read(long long* dst, int n);
int conv3d_halo7_trace_read(long long* dst, int n);
#endif

}  // namespace lt
