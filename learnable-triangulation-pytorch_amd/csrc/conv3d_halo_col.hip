// 3D halo convolution, the bf16 3^3 32 -> 32 kernels whose weights stay in LDS while a workgroup walks tiles: the persistent kernel and the column walk
// (with its computed-skip and fp32-store forms, on both MFMA shapes).  Overview, LDS images and the dispatch table: conv3d_halo.hip; the shared parts:
// conv3d_halo.h.
#include "conv3d_halo.h"

namespace {

// ---- persistent 3^3 kernel: weights resident in LDS, halo double-buffered, loader waves -----------------------------------
// The one-tile-per-workgroup kernel (conv3d_halo_tile.hip) spends most of a tile's life NOT in MFMAs at the 32-channel levels: a tile is only
// 27 taps x 4 MFMAs per wave (~3.4k matrix cycles), but its halo DMA round trip, the 27 x 2 KB weight stream with a barrier
// (and an L2 round trip) per chunk, and the epilogue are all serial inside the workgroup (measured 17 us per tile and
// workgroup).  Here a workgroup stays on its CU and walks tiles:
//   * all 27 tap slabs (54 KB at 32->32 bf16) are DMA'd once;
//   * waves 4-7 are LOADERS: they do nothing but request the halo of tile i+1 into the other halo buffer while waves 0-3
//     (CONSUMERS) compute tile i.  Shader-clock accounting of the first version, where the four compute waves also issued the
//     DMAs: 4.4k cycles per tile in the halo issue (the wave sits in the issue stage while the load path queues the requests),
//     3.4k in the tap loop, 5.9k in the epilogue (most of it the wait for that same DMA) -- all serial;
//   * the tap loop has no barrier, and runs a fragment pipeline PDU (k-group) units deep with hand-counted lgkmcnt;
//   * the MFMAs compute the transposed product (weights first): a lane ends up with 16 channels of its own voxel and stores
//     them as 8-byte bf16 groups straight from the accumulators -- no LDS staging tile.
// One workgroup barrier per tile (halo i landed / everybody done with the tap loop of tile i-1).  Tiles are dealt so that
// workgroup b (XCD b % 8) keeps to the samples / raster run of that XCD, as above.
template <typename T, int CIN, int CP>
__global__ __launch_bounds__(512) void conv3d_halo_persist_kernel(const HaloArgs a, const int total_tiles) {
    constexpr int KS = 3;
    typedef HaloCfg<T, KS, CIN, CP, 9, 2> C;
    constexpr int TD = C::TD, TH = C::TH, TW = C::TW;
    static_assert(sizeof(T) == 2, "bf16 only: fp32 slabs do not fit beside two halo buffers");
    constexpr int MF = C::MF, SM = C::SM, SN = C::SN, G = C::G, NACC = C::NACC, NVV = C::NVV, VPR = C::VPR, CINB = C::CINB;
    constexpr int W_BYTES = ((C::NTAPS * C::SLAB + 1023) / 1024) * 1024;
    static_assert(C::SW::FA == 0 && C::SW::FC == 0 && C::SW::FB == 0, "kw-only swizzle");
    static_assert(C::EP_BYTES <= C::HALO_BYTES, "epilogue staging must fit a halo buffer");
    typedef typename Mma<T, MF>::acc_t acc_t;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned lds_halo = lds0 + W_BYTES;            // two halo buffers follow the weights

    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_h;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool loader = wave >= 4;
    const int wl = wave & 3;                             // index inside the role
    constexpr int P = 1;
    const int tps = a.tiles_d * a.tiles_h * a.tiles_w;
    const T* __restrict__ w = (const T*)a.w;

    auto tile_of = [&](int v, int& n, int& d0, int& h0, int& w0) {   // v: virtual workgroup index (v % 8 = XCD of this workgroup)
        int tix;
        if (a.xcd_pin) {
            const int xcd = v & 7, j = v >> 3;
            n = xcd + 8 * (j / tps);
            tix = j % tps;
        } else {
            const int nb = total_tiles, q = nb >> 3, r = nb & 7, xcd = v & 7, j = v >> 3;
            const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
            n = lin / tps;
            tix = lin % tps;
        }
        w0 = (tix % a.tiles_w) * TW;
        h0 = ((tix / a.tiles_w) % a.tiles_h) * TH;
        d0 = (tix / (a.tiles_w * a.tiles_h)) * TD;
    };
    constexpr int NI_H = C::HALO_BYTES / 1024;
    auto issue_halo = [&](int n, int d0, int h0, int w0, int buf) {   // loaders only: piece wl, wl + 4, ...
        const T* __restrict__ x = (const T*)a.x + (size_t)n * a.D * a.H * a.W * CIN;
        for (int i = wl; i < NI_H; i += 4) {
            const int q = i * 64 + lane;
            const int hv = q / NVV, pv = q % NVV;
            const int hw_ = hv % C::PW, hh_ = (hv / C::PW) % C::HH, hd_ = hv / (C::PW * C::HH);
            const int lv = pv ^ C::fswz(hd_, hh_, hw_);
            const int id = d0 - P + hd_, ih = h0 - P + hh_, iw = w0 - P + hw_;
            const bool ok = hv < C::HV && hw_ < C::HW && ((unsigned)id < (unsigned)a.D) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
            const void* src = ok ? (const void*)(x + (((size_t)id * a.H + ih) * a.W + iw) * CIN + lv * C::VEC) : zero_page;
            dma16_uniform(src, lds_halo + buf * C::HALO_BYTES + i * 1024);
        }
    };

    // ---- weights: every tap slab, once (all eight waves) ----
    constexpr int NI_W = W_BYTES / 1024;
    for (int i = wave; i < NI_W; i += 8) {
        const int q = i * 64 + lane;
        const int pv = q % NVV, col = (q / NVV) % CP, tap = q / (NVV * CP);
        const int lv = pv ^ ((-(col / VPR)) & (NVV - 1));
        const void* src = tap < C::NTAPS ? (const void*)(w + (size_t)col * a.k_pad + tap * CIN + lv * C::VEC) : zero_page;
        dma16_uniform(src, lds0 + i * 1024);
    }

    int v = blockIdx.x;
    int n, d0, h0, w0;
    tile_of(v, n, d0, h0, w0);

#ifdef LT_TRACE
    long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
    const long long tr_begin = LT_CLK();
#define LT_TRH(k_) { const long long c_ = LT_CLK(); tr[k_] += c_ - tr_last; tr_last = c_; }
    long long tr_last = tr_begin;
#else
#define LT_TRH(k_)
#endif

    if (loader) {
        // ================================= loader waves =================================
        issue_halo(n, d0, h0, w0, 0);
        for (int it = 0;; ++it) {
            const int vn = v + gridDim.x;
            const bool have_next = vn < total_tiles;
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // A: halo(it) (and the weights) landed
#ifndef LT_ABL_NO_A
            if (have_next) {
                int nn, nd0, nh0, nw0;
                tile_of(vn, nn, nd0, nh0, nw0);
                issue_halo(nn, nd0, nh0, nw0, (it & 1) ^ 1);               // lands while the consumers compute tile it
            }
#endif
            if (!have_next) break;
            v = vn;
        }
        return;
    }

    // ================================= consumer waves =================================
    // ---- per-lane fragment bases (halo part is rebased per tile: the buffer alternates) ----
    const int lvb = (MF == 32) ? (lane >> 5) : (lane >> 4);
    int abase[KS][G][SM];
#pragma unroll
    for (int i = 0; i < SM; ++i) {
        const int r = 64 * wave + i * MF + (lane & (MF - 1));
        const int tw = r % TW, th = (r / TW) % TH, td = r / (TW * TH);
        const int own = ((td * C::HH + th) * C::PW + tw) * CINB;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
            const int f = C::fswz(0, th, tw + kw);
#pragma unroll
            for (int g = 0; g < G; ++g) abase[kw][g][i] = own + (((lvb + ((MF == 32) ? 2 * g : 4 * g)) ^ f) << 4);
        }
    }
    unsigned bbase[G][SN];
#pragma unroll
    for (int j = 0; j < SN; ++j) {
        const int col = j * MF + (lane & (MF - 1));
        const int bsw = (-(col / VPR)) & (NVV - 1);
#pragma unroll
        for (int g = 0; g < G; ++g) bbase[g][j] = lds0 + col * CINB + (((lvb + ((MF == 32) ? 2 * g : 4 * g)) ^ bsw) << 4);
    }

    // fragment pipeline: unit u = tap * G + g (SM voxel-fragment reads + SN weight-fragment reads, SM*SN MFMAs); PDU units of lookahead
    constexpr int RPU = SM + SN;
    constexpr int PDU = 15 / RPU - 1 >= 4 ? 4 : 15 / RPU - 1;
    constexpr int RING = PDU + 1;
    constexpr int NU = C::NTAPS * G;
    static_assert(PDU >= 1 && (PDU + 1) * RPU <= 15, "lookahead exceeds the lgkmcnt counter");

    // ---- epilogue without LDS: the MFMAs compute the TRANSPOSED product D[co][voxel] (weights as the first operand), so lane
    // (voxel v = lane & 31 of fragment i, half h = lane >> 5) ends up with the channels c(e) = (e & 3) + 8 (e >> 2) + 4 h of ITS
    // voxel: four runs of four consecutive channels = four 8-byte bf16 stores (and four 8-byte residual loads) per fragment.
    // No staging tile, no second workgroup barrier per tile.
    static_assert(MF == 32 && SN == 1 && NACC == 16 && CP == 32, "transposed epilogue: one 32-channel column block");
    const int vl = lane & 31, hh = lane >> 5;
    float ebi[16], esc[16], esf[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = (e & 3) + 8 * (e >> 2) + 4 * hh;   // < 32 = cout_pad: the constant arrays are padded
        ebi[e] = a.bias ? a.bias[c] : 0.f;
        esc[e] = a.scale ? a.scale[c] : 1.f;
        esf[e] = a.shift ? a.shift[c] : 0.f;
    }
    const EpiFloors fl = epi_floors(a.flags);
    const bool has_res = a.res != nullptr;
    const unsigned no_res = has_res ? 0u : 0x80008000u;  // zeros -> -0.0 pairs: v + -0.0 == v
    // element offset of the lane's voxel of fragment i inside the tile, relative to the tile origin (td = wave, th = 4 i + v/8, tw = v%8)
    const size_t ldc = (size_t)a.ldc;
    const size_t voff0 = (((size_t)wave * a.H + (vl >> 3)) * a.W + (vl & 7)) * ldc + 4 * hh;
    const size_t vstep = (size_t)4 * a.W * ldc;          // fragment i -> th + 4

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of the weight slabs (and the constants)
    for (int it = 0;; ++it) {
        const int buf = it & 1;
        const int vn = v + gridDim.x;
        const bool have_next = vn < total_tiles;
        // A: halo(it) has landed (the loaders waited for it); every consumer is done with the tap loop of tile it-1 (its stores may still fly)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        LT_TRH(1)
        int nn = 0, nd0 = 0, nh0 = 0, nw0 = 0;
        if (have_next) tile_of(vn, nn, nd0, nh0, nw0);
        LT_TRH(2)
        const size_t tbase = ((((size_t)n * a.D + d0) * a.H + h0) * a.W + w0) * ldc + voff0;
        // residual of this tile: 8-byte pieces in named registers (an array stayed in scratch memory), consumed after the tap loop
        uint2 rq00, rq01, rq02, rq03, rq10, rq11, rq12, rq13;
        rq00 = rq01 = rq02 = rq03 = rq10 = rq11 = rq12 = rq13 = make_uint2(0, 0);
        if (has_res) {
            const T* rb = (const T*)a.res + tbase;
            rq00 = *(const uint2*)(rb + 0); rq01 = *(const uint2*)(rb + 8); rq02 = *(const uint2*)(rb + 16); rq03 = *(const uint2*)(rb + 24);
            rb += vstep;
            rq10 = *(const uint2*)(rb + 0); rq11 = *(const uint2*)(rb + 8); rq12 = *(const uint2*)(rb + 16); rq13 = *(const uint2*)(rb + 24);
        }
        LT_TRH(3)
        acc_t acc[SM];
#pragma unroll
        for (int i = 0; i < SM; ++i)
#pragma unroll
            for (int e = 0; e < NACC; ++e) acc[i][e] = 0.f;

        unsigned ha[KS][G][SM];
        const unsigned hbase = lds_halo + buf * C::HALO_BYTES;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw)
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int i = 0; i < SM; ++i) ha[kw][g][i] = hbase + abase[kw][g][i];

        V16 fa[RING][SM], fb[RING][SN];
        auto load_unit = [&](auto uc) {
            constexpr int u = decltype(uc)::value;
            constexpr int tap = u / G, g = u % G, slot = u % RING;
            constexpr int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            constexpr int imm = ((kd * C::HH + kh) * C::PW + kw) * CINB;
            static_for<0, SM>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                lds_read16<imm>(fa[slot][i], ha[kw][g][i]);
            });
            static_for<0, SN>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                lds_read16<tap * C::SLAB>(fb[slot][j], bbase[g][j]);
            });
        };
#ifndef LT_ABL_NO_MMA
        static_for<0, PDU>([&](auto uc) { load_unit(uc); });
        static_for<0, NU>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            constexpr int slot = u % RING;
            constexpr int ahead = (u + PDU < NU) ? PDU : NU - 1 - u;     // units in flight behind u at the wait
            if constexpr (u + PDU < NU) load_unit(std::integral_constant<int, u + PDU>{});
            lgkm_wait<ahead * RPU>();
#pragma unroll
            for (int i = 0; i < SM; ++i) frag_ready(fa[slot][i]);
            frag_ready(fb[slot][0]);
#pragma unroll
            for (int i = 0; i < SM; ++i) Mma<T, MF>::run(acc[i], fb[slot][0], fa[slot][i]);   // D[co][voxel]: weights first
        });
#endif
        LT_TRH(4)
        LT_TRH(5)
        // ---- epilogue straight from the accumulators ----
#ifdef LT_ABL_NO_EPI
        if (a.N < 0)
#endif
        {
            T* yb = (T*)a.y + tbase;
#define LT_HALO_T_ROW(I_, G_, RQ_)                                                                                  \
            {                                                                                                       \
                const unsigned r0 = RQ_.x | no_res, r1 = RQ_.y | no_res;                                            \
                float v0 = (acc[I_][4 * G_ + 0] + ebi[4 * G_ + 0]) * esc[4 * G_ + 0] + esf[4 * G_ + 0];             \
                float v1 = (acc[I_][4 * G_ + 1] + ebi[4 * G_ + 1]) * esc[4 * G_ + 1] + esf[4 * G_ + 1];             \
                float v2 = (acc[I_][4 * G_ + 2] + ebi[4 * G_ + 2]) * esc[4 * G_ + 2] + esf[4 * G_ + 2];             \
                float v3 = (acc[I_][4 * G_ + 3] + ebi[4 * G_ + 3]) * esc[4 * G_ + 3] + esf[4 * G_ + 3];             \
                v0 = epi_apply(v0, fl, __uint_as_float(r0 << 16));                                                  \
                v1 = epi_apply(v1, fl, __uint_as_float(r0 & 0xffff0000u));                                          \
                v2 = epi_apply(v2, fl, __uint_as_float(r1 << 16));                                                  \
                v3 = epi_apply(v3, fl, __uint_as_float(r1 & 0xffff0000u));                                          \
                *(uint2*)(yb + I_ * vstep + 8 * G_) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));         \
            }
            LT_HALO_T_ROW(0, 0, rq00) LT_HALO_T_ROW(0, 1, rq01) LT_HALO_T_ROW(0, 2, rq02) LT_HALO_T_ROW(0, 3, rq03)
            LT_HALO_T_ROW(1, 0, rq10) LT_HALO_T_ROW(1, 1, rq11) LT_HALO_T_ROW(1, 2, rq12) LT_HALO_T_ROW(1, 3, rq13)
#undef LT_HALO_T_ROW
        }
        LT_TRH(6)
#ifdef LT_TRACE
        tr[0] += 1;
#endif
        if (!have_next) break;
        v = vn; n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
    }
#ifdef LT_TRACE
    if (wave == 0 && lane == 0 && (blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 64) {
        long long* o = g_trace_h + (blockIdx.x >> 3) * 8;
        o[0] = LT_CLK() - tr_begin;
        for (int k = 1; k < 7; ++k) o[k] = tr[k];
        o[7] = tr[0];
    }
#endif
#undef LT_TRH
}

// ---- column-walking 3^3 kernel: sliding window of halo planes, epilogue of tile i under the MFMAs of tile i+1 ------------------
// Shader-clock accounting of the persistent kernel above (32 samples, 64^3): 6.8k cycles per tile = 0.7k waiting for the halo
// + 0.5k tile arithmetic + 0.5k residual issue + 3.6k tap loop (108 MFMAs = 3.5k) + 1.5k epilogue, all serial in the consumer
// waves; and the halo of tile i+1, requested right after the barrier of tile i, lands ~5.8k cycles later: one 38 KB halo in
// flight per CU is what the memory system is given (Little's law: 256 x 38 KB / 2.7 us = 3.6 TB/s, the measured rate).  Here:
//   * a workgroup walks COLUMNS of tiles along d: consecutive tiles share two of their six halo planes, so the halo becomes a
//     stream of 4-plane groups (25 KB per tile instead of 38: -33 % L2->LDS traffic) in a ring of four groups -- two being
//     read, two in flight or landed (51 KB requested ahead per CU);
//   * the epilogue of tile i-1 (affine, ReLU floors, residual, 8-byte stores) is issued in eight pieces between the MFMA
//     units of tile i, out of a copy of the accumulators; the residual of tile i is requested in the middle of its own tap
//     loop, after the pieces have consumed the previous one; tile coordinates advance by a stride (no divisions per tile).
// F32OUT: LT_EPI_STORE_F32 (the mixed-precision training step) as its own instantiation -- the inference kernel keeps its registers and schedule.
// SKIP: the residual is not read but COMPUTED -- the 1x1x1 skip convolution of a Res3DBlock whose channel count changes (v2v.py:33-42, 16 -> 32 at the
// 64^3 level): one more MFMA per fragment on the 16 input channels of the lane's own voxel (a 16-byte load instead of the 32-byte residual), its
// BatchNorm scale folded into the bf16 weights and its shift into `shift` by the caller.  The skip convolution's launch, its 32-channel output and that
// tensor's read here all disappear (lt_conv_skip_fwd).
// MFS: the consumers' bf16 MFMA, 32 = 32x32x16 or 16 = 16x16x32 -- the same tile per wave, LDS image, reads and cycles per tap; the chip holds a higher clock
// on the 16x16x32 form (DESIGN.md "MFMA shape").  The loaders and the LDS layout (C::MF = 32 names the layout) are the same for both.
template <typename T, bool F32OUT, bool SKIP, int MFS>
__global__ __launch_bounds__(512) void conv3d_halo_col_kernel(const HaloArgs a, const int total_cols) {
    constexpr int KS = 3, CIN = 32, CP = 32;
    typedef HaloCfg<T, KS, CIN, CP, 9, 2> C;
    constexpr int TD = C::TD, TH = C::TH, TW = C::TW;
    static_assert(sizeof(T) == 2, "bf16 only");
    constexpr int MF = C::MF, SM = C::SM, SN = C::SN, G = C::G, NACC = C::NACC, NVV = C::NVV, VPR = C::VPR, CINB = C::CINB;
    static_assert(MF == 32 && SM == 2 && SN == 1 && G == 2 && NACC == 16 && NVV == 4, "3^3 32->32 bf16 layout");
    static_assert(C::SW::FA == 0 && C::SW::FC == 0 && C::SW::FB == 0, "the swizzle must not depend on the plane");
    constexpr int W_BYTES = ((C::NTAPS * C::SLAB + 1023) / 1024) * 1024;
    constexpr int PLANE_V = C::HH * C::PW;               // voxel slots of one halo plane
    constexpr int PLANE_B = PLANE_V * CINB;
    constexpr int GROUP_B = TD * PLANE_B;                // one tile step = TD new planes
    constexpr int NI_G = GROUP_B / 1024;
    static_assert(GROUP_B % 1024 == 0, "a plane group must be whole DMA wave-instructions");
    static_assert(W_BYTES + 4 * GROUP_B <= 160 * 1024, "weights + four plane groups must fit LDS");
    typedef typename Mma<T, MF>::acc_t acc_t;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned lds_halo = lds0 + W_BYTES;            // ring of four plane groups

    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_h;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool loader = wave >= 4;
    const int wl = wave & 3;
    const T* __restrict__ w = (const T*)a.w;
    const int tpc = a.tiles_d, ngc = a.tiles_d + 1;      // tiles / plane groups per column
    const int cps = a.tiles_h * a.tiles_w;               // columns per sample
    const int ncol = (total_cols - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

    auto col_of = [&](int v, int& n, int& h0, int& w0) {  // v % 8 = XCD of this workgroup (gridDim.x % 8 == 0)
        const int xcd = v & 7, j = v >> 3;
        int cix;
        if (a.xcd_pin) {
            n = xcd + 8 * (j / cps);
            cix = j % cps;
        } else {
            const int lin = xcd * (total_cols >> 3) + j;     // total_cols % 8 == 0
            n = lin / cps;
            cix = lin % cps;
        }
        w0 = (cix % a.tiles_w) * TW;
        h0 = (cix / a.tiles_w) * TH;
    };

    // ---- weights: every tap slab, once (all eight waves) ----
    constexpr int NI_W = W_BYTES / 1024;
    for (int i = wave; i < NI_W; i += 8) {
        const int q = i * 64 + lane;
        const int pv = q % NVV, col = (q / NVV) % CP, tap = q / (NVV * CP);
        const int lv = pv ^ ((-(col / VPR)) & (NVV - 1));
        const void* src = tap < C::NTAPS ? (const void*)(w + (size_t)col * a.k_pad + tap * CIN + lv * C::VEC) : zero_page;
        dma16_uniform(src, lds0 + i * 1024);
    }

    if (loader) {
        // ================================= loader waves =================================
        // stream of plane groups: column c of this workgroup contributes groups 0..tpc (group g = planes 4g-1 .. 4g+2 of the
        // column), stream index S = c * ngc + g lives in ring slot S & 3; tile (c, k) reads S and S + 1.
        // The (plane, row, column, k-vector) a lane fetches for DMA piece i is the same for every group: decode it ONCE (the
        // divisions below cost ~60 VALU instructions per piece, and the loaders share their SIMDs' issue slots with the
        // consumers' MFMA stream); per group only the plane validity and one base pointer change.
        const int total_groups = ncol * ngc;
        constexpr int MAXP = (NI_G + 3) / 4;              // pieces per wave and group
        int poff[MAXP], pmeta[MAXP];                      // element offset from (plane 4g-1, row h0, column w0); pj << 16 | hh << 8 | hw
#pragma unroll
        for (int m = 0; m < MAXP; ++m) {
            const int q = (wl + 4 * m) * 64 + lane;
            const int pj = q / (PLANE_V * NVV), r = q - pj * (PLANE_V * NVV);
            const int hv = r / NVV, pv = r % NVV;
            const int hh_ = hv / C::PW, hw_ = hv - hh_ * C::PW;
            const int lv = pv ^ C::fswz(0, hh_, hw_);
            poff[m] = ((pj * a.H + hh_ - 1) * a.W + hw_ - 1) * CIN + lv * C::VEC;
            pmeta[m] = (pj << 16) | (hh_ << 8) | hw_;
        }
        int issued = 0, icol = 0, ig = 0, in, ih0, iw0;
        unsigned okhw = 0;                                // bit m: piece m's (row, column) lies inside the sample for this column
        auto enter_col = [&](int v) {
            col_of(v, in, ih0, iw0);
            okhw = 0;
#pragma unroll
            for (int m = 0; m < MAXP; ++m) {
                const int hh_ = (pmeta[m] >> 8) & 255, hw_ = pmeta[m] & 255;
                const bool ok = hw_ < C::HW && ((unsigned)(ih0 - 1 + hh_) < (unsigned)a.H) & ((unsigned)(iw0 - 1 + hw_) < (unsigned)a.W);
                okhw |= ok ? (1u << m) : 0u;
            }
        };
        enter_col(blockIdx.x);
        auto issue_next = [&]() {
            const int d_first = 4 * ig - 1;
            // plane d_first, row h0, column w0 of sample n (outside the tensor for the padding planes: only formed, never read)
            const T* __restrict__ gb = (const T*)a.x + (((ptrdiff_t)in * a.D + d_first) * a.H + ih0) * (ptrdiff_t)a.W * CIN + (ptrdiff_t)iw0 * CIN;
            const unsigned dst = lds_halo + (issued & 3) * GROUP_B;
#pragma unroll
            for (int m = 0; m < MAXP; ++m) {
                if (wl + 4 * m < NI_G) {
                    const bool ok = ((okhw >> m) & 1u) && (unsigned)(d_first + (pmeta[m] >> 16)) < (unsigned)a.D;
                    const void* src = ok ? (const void*)(gb + poff[m]) : zero_page;
#ifdef LT_ABL_NO_A
                    if (a.N < 0)
#endif
                    dma16_uniform(src, dst + (wl + 4 * m) * 1024);
                }
            }
            ++issued;
            if (++ig == ngc) {
                ig = 0;
                if (++icol < ncol) enter_col(blockIdx.x + icol * gridDim.x);
            }
        };
        const int mine = (NI_G - wl + 3) / 4;             // DMA pieces of one group requested by this wave
        for (int k = 0; k < 4 && issued < total_groups; ++k) issue_next();
        int sidx = 0, k = 0;
        const int ntile = ncol * tpc;
        for (int ti = 0; ti < ntile; ++ti) {
            const int ahead = issued - sidx - 2;          // groups requested beyond the two this tile reads: 0, 1 or 2
            wait_vmcnt(ahead > 0 ? ahead * mine : 0);
            asm volatile("s_barrier" ::: "memory");       // A: groups sidx, sidx + 1 landed; the consumers are done with tile ti - 1
            while (issued <= sidx + 3 && issued < total_groups) issue_next();
            ++sidx;
            if (++k == tpc) { k = 0; ++sidx; }
        }
        return;
    }

    if constexpr (MFS == 16) {
        // ================================= consumer waves, v_mfma_f32_16x16x32_bf16 =================================
        // The same 64 voxels x 32 channels per wave, the same LDS image and the same reads per tap (four voxel fragments + two weight fragments, one
        // ds_read_b128 each), eight accumulators of four registers.  A unit is a whole tap (K = 32).  Lane (n = l & 15, q = l >> 4):
        //   voxel fragment f = rows 2 f, 2 f + 1 of the wave's plane: voxel (2 f + (n >> 3), (n & 1) | (n >> 2 & 1) << 1 | (n >> 1 & 1) << 2), k-vector q --
        //     with this column order the four 16-lane groups of the read are conflict-free under the plane's swizzle for every tap (tools/halo_bank_search.py);
        //   weight fragment s = rows chan = 16 (n >> 3) + 8 (n >> 2 & 1) + 4 s + (n & 3) of the tap's slab, k-vector q (conflict-free as stored);
        //   result register reg of (f, s) = channel 8 q + 4 s + reg of the lane's voxel: eight consecutive channels per fragment -- one 16-byte residual load
        //     and one 16-byte store per piece, four pieces per tile under the next tile's taps.
        static_assert(!F32OUT, "the fp32-store instantiation keeps the 32x32x16 form");
        constexpr int NF = 4;
        const int n16 = lane & 15, q = lane >> 4;
        const int vr = n16 >> 3, vc = (n16 & 1) | (((n16 >> 2) & 1) << 1) | (((n16 >> 1) & 1) << 2);
        int abase[KS];                                    // in-plane byte offset of (voxel of fragment 0, k-vector q), per kw; the swizzle does not depend on the row
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) abase[kw] = (vr * C::PW + vc) * CINB + ((q ^ C::fswz(0, vr, vc + kw)) << 4);
        unsigned bbase[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int chan = 16 * (n16 >> 3) + 8 * ((n16 >> 2) & 1) + 4 * s + (n16 & 3);
            bbase[s] = lds0 + chan * CINB + ((q ^ ((-(chan / VPR)) & (NVV - 1))) << 4);
        }
        constexpr int RPU = NF + 2, PDU = 2, RING = PDU + 1, NU = C::NTAPS;
        static_assert(PDU * RPU <= 15, "lookahead exceeds the lgkmcnt counter");
        float esc[8], esf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 8 * q + e;
            const float bi = a.bias ? a.bias[c] : 0.f, sc = a.scale ? a.scale[c] : 1.f, sf = a.shift ? a.shift[c] : 0.f;
            esc[e] = sc;
            esf[e] = bi * sc + sf;
        }
        const EpiFloors fl = epi_floors(a.flags);
        const bool has_res = a.res != nullptr;
        const unsigned no_res = has_res ? 0u : 0x80008000u;  // zeros -> -0.0 pairs: v + -0.0 == v
        const size_t ldc = (size_t)a.ldc;
        const size_t voff0 = (((size_t)wave * a.H + vr) * a.W + vc) * ldc + 8 * q;
        const size_t vstep = (size_t)2 * a.W * ldc;          // fragment f -> two rows on
        const size_t dstep = (size_t)TD * a.H * a.W * ldc;   // next tile of the column
        const size_t rstep = has_res ? vstep : 0;            // without a residual every piece reads the zero page
        constexpr int SKC = 16;                              // channels per voxel of the skip tensor
        const size_t svoff0 = (((size_t)wave * a.H + vr) * a.W + vc) * SKC + 8 * (q & 1);
        const size_t svstep = (size_t)2 * a.W * SKC, sdstep = (size_t)TD * a.H * a.W * SKC;
        // SKIP: a K = 16 product as ONE 16x16x32 MFMA per fragment with the upper half of K zeroed in the WEIGHT operand (lanes q >= 2 hold zeros; the voxel
        // operand of those lanes repeats the lane's own 16 channels, so nothing foreign is multiplied).  Chosen over v_mfma_f32_16x16x16_bf16: that form takes
        // 8-byte operands, i.e. 8-byte scattered loads of the skip tensor; here the loads stay 16 bytes, at 8 more cycles per fragment (32 per tile of ~3.5k)
        V16 wsk[2];
        if constexpr (SKIP) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int r = (n16 & 7) | (s << 3) | ((n16 >> 3) << 4);
                wsk[s].u = *(const uint4*)((const T*)a.skip_w + (size_t)(32 * (q & 1) + r) * 8);
                if (q >= 2) wsk[s].u = make_uint4(0u, 0u, 0u, 0u);
            }
        }

        int n, h0, w0;
        col_of(blockIdx.x, n, h0, w0);
        size_t tbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * ldc + voff0;
        size_t sbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * SKC + svoff0;
        size_t pbase = 0;                                    // output offset of the tile whose epilogue is pending
        f32x4 sacc[2];                                       // SKIP: W_skip . x_skip of the fragment whose piece is being issued
        f32x4 acc[NF][2], pacc[NF][2];
        uint4 rq[NF], rqn[NF];                               // residual (SKIP: skip input) of the pending tile / of the tile being computed
        unsigned ha[KS];
        unsigned hd1 = 0, hd2 = 0;                           // plane base of kd = 1 minus kd = 0, kd = 2 minus kd = 1
        V16 fa[RING][NF], fb[RING][2];

        auto load_unit = [&](auto uc) {
            constexpr int tap = decltype(uc)::value, slot = tap % RING;
            constexpr int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            if constexpr (tap > 0 && tap % 9 == 0) {         // first tap of the next kd: move the fragment bases one plane on
                const unsigned dlt = kd == 1 ? hd1 : hd2;
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) ha[kk] += dlt;
            }
            static_for<0, NF>([&](auto fc) {
                constexpr int f = decltype(fc)::value;
                lds_read16<((kh + 2 * f) * C::PW + kw) * CINB>(fa[slot][f], ha[kw]);
            });
            lds_read16<tap * C::SLAB>(fb[slot][0], bbase[0]);
            lds_read16<tap * C::SLAB>(fb[slot][1], bbase[1]);
        };
        auto skip_mma = [&](auto pc) {                       // SKIP: fragment p of the pending tile (its skip channels are in rq[p])
            constexpr int p = decltype(pc)::value;
            if constexpr (SKIP) {
                V16 xs;
                xs.u = rq[p];
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 2; ++s) sacc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wsk[s].h, xs.h, z, 0, 0, 0);
            }
        };
        auto epi_piece = [&](auto pc) {                      // piece p of the pending tile: fragment p, the lane's eight channels
            constexpr int p = decltype(pc)::value;
            const unsigned rr[4] = {rq[p].x | no_res, rq[p].y | no_res, rq[p].z | no_res, rq[p].w | no_res};
            unsigned o[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int e = 2 * d, s = d >> 1, r = e & 3;
                float v0 = fmaf(pacc[p][s][r], esc[e], esf[e]);
                float v1 = fmaf(pacc[p][s][r + 1], esc[e + 1], esf[e + 1]);
                v0 = epi_apply(v0, fl, SKIP ? sacc[s][r] : __uint_as_float(rr[d] << 16));
                v1 = epi_apply(v1, fl, SKIP ? sacc[s][r + 1] : __uint_as_float(rr[d] & 0xffff0000u));
                o[d] = pack_bf16x2(v0, v1);
            }
            *(uint4*)((T*)a.y + pbase + p * vstep) = make_uint4(o[0], o[1], o[2], o[3]);
        };
        auto tap_loop = [&](auto epi_c) {
            constexpr bool EPI = decltype(epi_c)::value;
            static_for<0, PDU>([&](auto uc) { load_unit(uc); });
            static_for<0, NU>([&](auto uc) {
                constexpr int u = decltype(uc)::value;
                constexpr int slot = u % RING;
                constexpr int ahead = (u + PDU < NU) ? PDU : NU - 1 - u;
                if constexpr (u + PDU < NU) load_unit(std::integral_constant<int, u + PDU>{});
                lgkm_wait<ahead * RPU>();
#pragma unroll
                for (int f = 0; f < NF; ++f) frag_ready(fa[slot][f]);
                frag_ready(fb[slot][0]);
                frag_ready(fb[slot][1]);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int s = 0; s < 2; ++s)               // D[co][voxel]: weights first; eight independent accumulators in rotation
                        acc[f][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[slot][s].h, fa[slot][f].h, acc[f][s], 0, 0, 0);
                // the pending tile's pieces under taps 1, 4, 7, 10 (the units 2, 8, 14, 20 of the 32x32x16 form), each skip product one tap ahead of its piece
                if constexpr (EPI && SKIP && u % 3 == 0 && u < 12) skip_mma(std::integral_constant<int, u / 3>{});
                if constexpr (EPI && u % 3 == 1 && u < 12) epi_piece(std::integral_constant<int, u / 3>{});
                if constexpr (u == 0) {
                    // residual of THIS tile, requested a whole tap loop before the pieces under the next tile consume it; explicitly GLOBAL loads (flat loads
                    // would count in lgkmcnt, which the fragment pipeline counts by hand)
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    typedef const __attribute__((address_space(1))) u32x4* gq_t;
                    const unsigned long long rb = SKIP ? (unsigned long long)(size_t)((const T*)a.skip_x + sbase)
                                                       : has_res ? (unsigned long long)(size_t)((const T*)a.res + tbase) : zp_bits;
                    const size_t st = SKIP ? svstep : rstep;
                    static_for<0, NF>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        const u32x4 rv = *(gq_t)(rb + (p * st) * sizeof(T));
                        rqn[p] = make_uint4(rv[0], rv[1], rv[2], rv[3]);
                    });
                }
            });
        };

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of the weight slabs (and the constants)
        {   // the pointers the tile loop uses, in SGPRs here (see the 32x32x16 form below)
            const void* yp_ = a.y;
            const void* sx_ = SKIP ? a.skip_x : a.res;
            asm volatile("" ::"s"(yp_), "s"(sx_));
        }
        int sidx = 0, k = 0, icol = 0;
        const int ntile = ncol * tpc;
        for (int ti = 0; ti < ntile; ++ti) {
            // A: plane groups sidx, sidx + 1 have landed; every consumer is done with the tap loop of the previous tile
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            {
                const unsigned p0 = lds_halo + ((sidx + (wave >> 2)) & 3) * GROUP_B + (wave & 3) * PLANE_B;
                const unsigned p1 = lds_halo + ((sidx + ((wave + 1) >> 2)) & 3) * GROUP_B + ((wave + 1) & 3) * PLANE_B;
                const unsigned p2 = lds_halo + ((sidx + ((wave + 2) >> 2)) & 3) * GROUP_B + ((wave + 2) & 3) * PLANE_B;
                hd1 = p1 - p0; hd2 = p2 - p1;
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) ha[kw] = p0 + abase[kw];
            }
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[f][0][e] = acc[f][1][e] = 0.f;
            if (ti == 0) tap_loop(std::false_type{});
            else tap_loop(std::true_type{});
#pragma unroll
            for (int f = 0; f < NF; ++f) { pacc[f][0] = acc[f][0]; pacc[f][1] = acc[f][1]; rq[f] = rqn[f]; }
            pbase = tbase;
            ++sidx;
            tbase += dstep;
            sbase += sdstep;
            if (++k == tpc) {                                // next column
                k = 0; ++sidx;
                if (++icol < ncol) {
                    col_of(blockIdx.x + icol * gridDim.x, n, h0, w0);
                    tbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * ldc + voff0;
                    sbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * SKC + svoff0;
                }
            }
        }
        static_for<0, NF>([&](auto pc) {                     // the last tile's epilogue has nothing to hide under
            skip_mma(pc);
            epi_piece(pc);
        });
        return;
    }
    // ================================= consumer waves =================================
    // wave = output plane td of the tile; fragment i covers rows th = 4 i + v / 8, tw = v % 8 of that plane
    const int lvb = lane >> 5;
    int abase[KS][G][SM];                                 // in-plane byte offset of (voxel, k-vector), per kw
#pragma unroll
    for (int i = 0; i < SM; ++i) {
        const int r = i * MF + (lane & (MF - 1));
        const int tw = r % TW, th = r / TW;
        const int own = (th * C::PW + tw) * CINB;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
            const int f = C::fswz(0, th, tw + kw);
#pragma unroll
            for (int g = 0; g < G; ++g) abase[kw][g][i] = own + (((lvb + 2 * g) ^ f) << 4);
        }
    }
    // MFMA row r of the transposed product (= the weight row this lane feeds) carries output channel chan(r), chosen so that
    // the 16 result registers of lane (voxel, h) are channels 8h .. 8h+7 and 16+8h .. 16+8h+7: two 16-byte runs, loaded
    // (residual) and stored as such.  The MFMA's own row order (r = 8q + 4h + j in register 4q + j) would give four 8-byte runs
    // per lane: twice the vector-memory instructions, and their issue (~65 cycles each for 64 scattered lanes) is paid by the
    // wave that also issues the MFMAs.
    unsigned bbase[G][SN];
    {
        const int r = lane & 31;
        const int chan = 16 * (r >> 4) + 8 * ((r >> 2) & 1) + 4 * ((r >> 3) & 1) + (r & 3);
        const int bsw = (-(chan / VPR)) & (NVV - 1);
#pragma unroll
        for (int g = 0; g < G; ++g) bbase[g][0] = lds0 + chan * CINB + (((lvb + 2 * g) ^ bsw) << 4);
    }
    constexpr int RPU = SM + SN;
    constexpr int PDU = 4;
    constexpr int RING = PDU + 1;
    constexpr int NU = C::NTAPS * G;
    static_assert((PDU + 1) * RPU <= 15, "lookahead exceeds the lgkmcnt counter");

    // transposed product D[co][voxel]: lane (voxel v = lane & 31 of fragment i, half h = lane >> 5) holds channels
    // c(e) = 8 h + e (e < 8) and 16 + 8 h + (e - 8) of its voxel; (acc + bias) * scale + shift folded into one fma per value
    const int vl = lane & 31, hh = lane >> 5;
    float esc[16], esf[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = 16 * (e >> 3) + 8 * hh + (e & 7);
        const float bi = a.bias ? a.bias[c] : 0.f, sc = a.scale ? a.scale[c] : 1.f, sf = a.shift ? a.shift[c] : 0.f;
        esc[e] = sc;
        esf[e] = bi * sc + sf;
    }
    const EpiFloors fl = epi_floors(a.flags);
    const bool has_res = a.res != nullptr;
    const unsigned no_res = has_res ? 0u : 0x80008000u;  // zeros -> -0.0 pairs: v + -0.0 == v
    const size_t ldc = (size_t)a.ldc;
    const size_t voff0 = (((size_t)wave * a.H + (vl >> 3)) * a.W + (vl & 7)) * ldc + 8 * hh;
    const size_t vstep = (size_t)4 * a.W * ldc;          // fragment i -> th + 4
    const size_t dstep = (size_t)TD * a.H * a.W * ldc;   // next tile of the column
    const size_t rstep = has_res ? vstep : 0;            // without a residual every piece reads the zero page
    constexpr int SKC = 16;                              // channels per voxel of the skip tensor
    const size_t svoff0 = (((size_t)wave * a.H + (vl >> 3)) * a.W + (vl & 7)) * SKC + 8 * hh;
    const size_t svstep = (size_t)4 * a.W * SKC, sdstep = (size_t)TD * a.H * a.W * SKC;
    V16 wsk;
    if constexpr (SKIP) wsk.u = *(const uint4*)((const T*)a.skip_w + (size_t)lane * 8);

    int n, h0, w0;
    col_of(blockIdx.x, n, h0, w0);
    size_t tbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * ldc + voff0;
    size_t sbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * SKC + svoff0;
    size_t pbase = 0;                                    // output offset of the tile whose epilogue is pending
    acc_t sacc;                                          // SKIP: W_skip . x_skip of the fragment whose pieces are being issued

    acc_t acc[SM], pacc[SM];
    uint4 rq[4], rqn[4];                                  // residual of the pending tile / of the tile being computed
    unsigned ha[KS][G][SM];
    unsigned hd1 = 0, hd2 = 0;                            // plane base of kd = 1 minus kd = 0, kd = 2 minus kd = 1
    V16 fa[RING][SM], fb[RING][SN];

    auto load_unit = [&](auto uc) {
        constexpr int u = decltype(uc)::value;
        constexpr int tap = u / G, g = u % G, slot = u % RING;
        constexpr int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        constexpr int imm = (kh * C::PW + kw) * CINB;
        if constexpr (u > 0 && u % (9 * G) == 0) {       // first unit of the next kd: move the twelve fragment bases one plane on
            const unsigned dlt = kd == 1 ? hd1 : hd2;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk)
#pragma unroll
                for (int gg = 0; gg < G; ++gg)
#pragma unroll
                    for (int ii = 0; ii < SM; ++ii) ha[kk][gg][ii] += dlt;
        }
        static_for<0, SM>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            lds_read16<imm>(fa[slot][i], ha[kw][g][i]);
        });
        lds_read16<tap * C::SLAB>(fb[slot][0], bbase[g][0]);
    };
    auto skip_mma = [&](auto ic) {                        // SKIP: fragment I of the pending tile (its 16 skip channels are in rq[I])
        constexpr int I = decltype(ic)::value;
        if constexpr (SKIP) {
            V16 xs;
            xs.u = rq[I];
            acc_t z;
#pragma unroll
            for (int e = 0; e < NACC; ++e) z[e] = 0.f;
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wsk.h, xs.h, z, 0, 0, 0);
        }
    };
    auto epi_piece = [&](auto pc) {                       // piece p of the pending tile: fragment p / 2, 8-channel run p % 2
        constexpr int p = decltype(pc)::value, I = p >> 1, Q = p & 1;
        const unsigned rr[4] = {rq[SKIP ? 0 : p].x | no_res, rq[SKIP ? 0 : p].y | no_res, rq[SKIP ? 0 : p].z | no_res, rq[SKIP ? 0 : p].w | no_res};
        unsigned o[4];
        float vf[F32OUT ? 8 : 1];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int e = 8 * Q + 2 * d;
            float v0 = fmaf(pacc[I][e], esc[e], esf[e]);
            float v1 = fmaf(pacc[I][e + 1], esc[e + 1], esf[e + 1]);
            v0 = epi_apply(v0, fl, SKIP ? sacc[e] : __uint_as_float(rr[d] << 16));
            v1 = epi_apply(v1, fl, SKIP ? sacc[e + 1] : __uint_as_float(rr[d] & 0xffff0000u));
            if constexpr (F32OUT) { vf[2 * d] = v0; vf[2 * d + 1] = v1; }
            else o[d] = pack_bf16x2(v0, v1);
        }
#ifdef LT_ABL_NO_STORE
        if (a.N < 0)
#endif
        if constexpr (F32OUT) {   // the same eight channels as two float4
            float* yp = (float*)a.y + pbase + I * vstep + 16 * Q;
            *(float4*)yp = make_float4(vf[0], vf[1], vf[2], vf[3]);
            *(float4*)(yp + 4) = make_float4(vf[4], vf[5], vf[6], vf[7]);
        } else {
            *(uint4*)((T*)a.y + pbase + I * vstep + 16 * Q) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    };
    auto tap_loop = [&](auto epi_c) {
        constexpr bool EPI = decltype(epi_c)::value;
        static_for<0, PDU>([&](auto uc) { load_unit(uc); });
        static_for<0, NU>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            constexpr int slot = u % RING;
            constexpr int ahead = (u + PDU < NU) ? PDU : NU - 1 - u;
            if constexpr (u + PDU < NU) load_unit(std::integral_constant<int, u + PDU>{});
            lgkm_wait<ahead * RPU>();
#pragma unroll
            for (int i = 0; i < SM; ++i) frag_ready(fa[slot][i]);
            frag_ready(fb[slot][0]);
#pragma unroll
            for (int i = 0; i < SM; ++i) Mma<T, MF>::run(acc[i], fb[slot][0], fa[slot][i]);   // D[co][voxel]: weights first
#ifndef LT_ABL_NO_EPI
            if constexpr (EPI && SKIP && (u == 0 || u == 12)) skip_mma(std::integral_constant<int, u / 12>{});   // two units in front of the pieces that use it
            if constexpr (EPI && u >= 2 && u < 26 && (u - 2) % 6 == 0) epi_piece(std::integral_constant<int, (u - 2) / 6>{});
#endif
            if constexpr (u == 0) {
                // residual of THIS tile, requested a whole tap loop before the pieces under the next tile consume it (requested
                // at unit 30 it arrived late: the first piece stalled ~1.3k cycles per tile).  Explicitly GLOBAL loads: a
                // pointer selected between the residual and the zero page is a flat pointer to the compiler, and flat loads
                // also count in lgkmcnt, which the fragment pipeline counts by hand
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                typedef const __attribute__((address_space(1))) u32x4* gq_t;
                if constexpr (SKIP) {                            // the lane's own voxel of fragments 0 and 1: 8 of the 16 skip channels each (half hh)
                    const unsigned long long sb = (unsigned long long)(size_t)((const T*)a.skip_x + sbase);
                    static_for<0, 2>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        const u32x4 rv = *(gq_t)(sb + (p * svstep) * sizeof(T));
                        rqn[p] = make_uint4(rv[0], rv[1], rv[2], rv[3]);
                    });
                } else {
                const unsigned long long rb = has_res ? (unsigned long long)(size_t)((const T*)a.res + tbase) : zp_bits;
                static_for<0, 4>([&](auto pc) {
                    constexpr int p = decltype(pc)::value;
                    const u32x4 rv = *(gq_t)(rb + ((p >> 1) * rstep + 16 * (p & 1)) * sizeof(T));
                    rqn[p] = make_uint4(rv[0], rv[1], rv[2], rv[3]);
                });
                }
            }
        });
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of the weight slabs (and the constants)
    {   // the pointers the tile loop uses, in SGPRs HERE: left to itself hipcc fetches a.y from the kernel arguments right in front of the loop and puts the
        // s_waitcnt lgkmcnt(0) for it in front of the first store INSIDE the loop -- where it drains the hand-counted fragment pipeline once per tile
        const void* yp_ = a.y;
        const void* sx_ = SKIP ? a.skip_x : a.res;
        asm volatile("" ::"s"(yp_), "s"(sx_));
    }
#ifdef LT_TRACE
    long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
    const long long tr_begin = LT_CLK();
    long long tr_last = tr_begin;
#define LT_TRC(k_) { const long long c_ = LT_CLK(); tr[k_] += c_ - tr_last; tr_last = c_; }
#else
#define LT_TRC(k_)
#endif
    int sidx = 0, k = 0, icol = 0;
    const int ntile = ncol * tpc;
    for (int ti = 0; ti < ntile; ++ti) {
        // A: plane groups sidx, sidx + 1 have landed; every consumer is done with the tap loop of the previous tile
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        LT_TRC(1)
        {
            const unsigned p0 = lds_halo + ((sidx + (wave >> 2)) & 3) * GROUP_B + (wave & 3) * PLANE_B;
            const unsigned p1 = lds_halo + ((sidx + ((wave + 1) >> 2)) & 3) * GROUP_B + ((wave + 1) & 3) * PLANE_B;
            const unsigned p2 = lds_halo + ((sidx + ((wave + 2) >> 2)) & 3) * GROUP_B + ((wave + 2) & 3) * PLANE_B;
            hd1 = p1 - p0; hd2 = p2 - p1;
#pragma unroll
            for (int kw = 0; kw < KS; ++kw)
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int i = 0; i < SM; ++i) ha[kw][g][i] = p0 + abase[kw][g][i];
        }
#pragma unroll
        for (int i = 0; i < SM; ++i)
#pragma unroll
            for (int e = 0; e < NACC; ++e) acc[i][e] = 0.f;
        LT_TRC(2)
        if (ti == 0) tap_loop(std::false_type{});
        else tap_loop(std::true_type{});
        LT_TRC(4)
#pragma unroll
        for (int i = 0; i < SM; ++i) pacc[i] = acc[i];
#pragma unroll
        for (int p = 0; p < 4; ++p) rq[p] = rqn[p];
        pbase = tbase;
        ++sidx;
        tbase += dstep;
        sbase += sdstep;
        if (++k == tpc) {                                // next column
            k = 0; ++sidx;
            if (++icol < ncol) {
                col_of(blockIdx.x + icol * gridDim.x, n, h0, w0);
                tbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * ldc + voff0;
                sbase = (((size_t)n * a.D * a.H + h0) * a.W + w0) * SKC + svoff0;
            }
        }
        LT_TRC(6)
    }
    static_for<0, 4>([&](auto pc) {                      // the last tile's epilogue has nothing to hide under
        if constexpr ((decltype(pc)::value & 1) == 0) skip_mma(std::integral_constant<int, decltype(pc)::value / 2>{});
        epi_piece(pc);
    });
#ifdef LT_TRACE
    if (wave == 0 && lane == 0 && (blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 64) {   // same record as the persistent kernel
        long long* o = g_trace_h + (blockIdx.x >> 3) * 8;
        o[0] = LT_CLK() - tr_begin;
        for (int q = 1; q < 7; ++q) o[q] = tr[q];
        o[7] = ntile;
    }
#endif
#undef LT_TRC
}

template <typename T, int CIN, int CP>
int launch_halo_persist(const HaloArgs& a, hipStream_t s) {
    typedef HaloCfg<T, 3, CIN, CP, 9, 2> C;
    constexpr int W_BYTES = ((C::NTAPS * C::SLAB + 1023) / 1024) * 1024;
    constexpr int LDS = W_BYTES + 2 * C::HALO_BYTES;
    static_assert(LDS <= 160 * 1024, "weights + two halo buffers do not fit LDS");
    auto kern = conv3d_halo_persist_kernel<T, CIN, CP>;
    LT_OPT_IN_LDS(kern, 160 * 1024);
    const int n_cu = lt::device_cu_count8();
    const long long total = (long long)a.N * a.tiles_d * a.tiles_h * a.tiles_w;
    const int grid = (int)(total < n_cu ? total - total % 8 : n_cu);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), LDS, s, a, (int)total);
    LT_CHECK_LAUNCH("lt_conv_fwd(halo, persistent)");
    return LT_OK;
}

template <typename T, bool F32OUT, bool SKIP, int MFS>
int launch_halo_col_as(const HaloArgs& a, hipStream_t s, int grid, int lds, int total_cols) {
    auto kern = conv3d_halo_col_kernel<T, F32OUT, SKIP, MFS>;
    LT_OPT_IN_LDS(kern, 160 * 1024);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), lds, s, a, total_cols);
    LT_CHECK_LAUNCH("lt_conv_fwd(halo, column walk)");
    return LT_OK;
}

template <typename T>
int launch_halo_col(const HaloArgs& a, hipStream_t s) {
    typedef HaloCfg<T, 3, 32, 32, 9, 2> C;
    constexpr int W_BYTES = ((C::NTAPS * C::SLAB + 1023) / 1024) * 1024;
    constexpr int LDS = W_BYTES + 4 * 4 * C::HH * C::PW * C::CINB;
    const int n_cu = lt::device_cu_count8();
    const int total_cols = a.N * a.tiles_h * a.tiles_w;  // % 8 == 0 (checked by the caller)
    const int grid = total_cols < n_cu ? total_cols : n_cu;
    // the MFMA shape per instantiation: halo_col_mfma (conv_common.h; LT_HALO_COL_MF32 is read here, per launch call)
    const int kind = a.skip_x ? 1 : (a.flags & LT_EPI_STORE_F32) ? 2 : 0;
    const bool mf16 = halo_col_mfma(kind) == 16;
    if (kind == 1) return mf16 ? launch_halo_col_as<T, false, true, 16>(a, s, grid, LDS, total_cols) : launch_halo_col_as<T, false, true, 32>(a, s, grid, LDS, total_cols);
    if (kind == 2) return launch_halo_col_as<T, true, false, 32>(a, s, grid, LDS, total_cols);
    return mf16 ? launch_halo_col_as<T, false, false, 16>(a, s, grid, LDS, total_cols) : launch_halo_col_as<T, false, false, 32>(a, s, grid, LDS, total_cols);
}

}  // namespace

namespace lt {

int conv3d_halo_col_launch(const HaloArgs& a, bool column_walk, hipStream_t s) {
    return column_walk ? launch_halo_col<bf16_t>(a, s) : launch_halo_persist<bf16_t, 32, 32>(a, s);
}

#ifdef LT_TRACE
int conv3d_halo_col_trace_read(long long* dst, int n) { return halo_trace_read(dst, n); }
#endif

}  // namespace lt
