// 3D halo convolution, bf16 3^3 with the weights as fragments from global memory: LDS holds the halo alone.  With it the kernel that packs the weights
// into fragment order (lt_conv_pack_weights_t32).  Overview, LDS images and the dispatch table: conv3d_halo.hip; the shared parts: conv3d_halo.h.
#include "conv3d_halo.h"

namespace {

// ---- 3^3 64 -> 64: halo in LDS, weights from global memory in fragment order, two workgroups per CU ----------------------------
// The loader-wave kernel (conv3d_halo_tile.hip, LDR) spends 37k cycles on a 64 -> 64 tile whose MFMAs take 13.8k: with the 77 KB halo AND a 72 KB weight ring
// in LDS only one workgroup fits a CU, so the halo round trip, the nine weight chunks (a barrier and an L2 round trip each) and
// the epilogue are all exposed.  Here the weights never touch LDS: lt_conv_pack_weights_t32 stores them once in the fragment
// order of the transposed product ([tap][16-channel K block][32-row Cout block][lane] x 16 bytes), a wave reads the one fragment
// it needs per (tap, K block) with a coalesced 1 KB global load (L1/L2 resident: 221 KB shared by every workgroup), and LDS
// holds the halo alone -- 75 KB, TWO workgroups per CU, whose load / MFMA / store phases overlap each other.  Wave = (Cout half,
// pair of output planes): four voxel fragments x one weight fragment per unit = four MFMAs per global load.  Voxel fragments keep
// the 128-byte-voxel swizzle of the other halo kernels (slot ^ f(row, column)); the K block enters the address as XOR (g << 5), one
// v_xor per read instead of 72 precomputed address registers.  Transposed product with permuted weight rows: the epilogue moves
// 16-byte channel runs straight from the accumulators (see conv3d_halo_col_kernel).
// Instantiated for 64 -> 64 (two Cout blocks: wave = (Cout half, pair of output planes), four voxel fragments), 32 -> 64 (same
// roles, two K blocks) and 128 -> 128 (four Cout blocks: wave = Cout block, all eight voxel fragments; 256-byte voxels fill
// LDS with the halo alone, one workgroup per CU with up to 512 registers per wave).
// Round 5: also 16 -> 32 (the first 3^3 layer of V2V at 64^3: one Cout block, wave = output plane, two voxel fragments per weight fragment; a 23 KB halo and
// 110 registers let four workgroups share a CU -- the one-tile loader-wave kernel it replaces there was latency-bound at 0.25 MFMA-busy).
template <typename T, int CIN, int CP>
__global__ __launch_bounds__(256, (CIN == 128 ? 1 : CIN == 16 ? 4 : 2)) void conv3d_halo_wreg_kernel(const HaloArgs a) {
    constexpr int KS = 3, G = CIN / 16, NB = CP / 32;
    typedef HaloCfg<T, KS, CIN, CP, 3, 3> C;
    constexpr int TD = C::TD, TH = C::TH, TW = C::TW;
    static_assert(sizeof(T) == 2 && (NB == 1 || NB == 2 || NB == 4) && (C::CINB == 32 || C::CINB == 64 || C::CINB == 128 || C::CINB == 256),
                  "bf16; 16/32/64/128 -> 32/64/128");
    static_assert(C::SW::FB == 0, "plane-independent swizzle");
    constexpr int PLANE_B = C::HH * C::PW * C::CINB;
    constexpr int NI_H = C::HALO_BYTES / 1024;
    constexpr int FR = NB == 1 ? 2 : NB == 2 ? 4 : 8;     // voxel fragments per wave
    constexpr bool PRE_RES = FR <= 4;                     // residual requested before the tap loop (register budget)
    // swizzle of the 16-byte vectors of a voxel: the searched ones for 64- and 128-byte voxels; 256-byte voxels start at bank 0
    // each, so the 16 lanes of a read phase (2 rows x 8 columns) must use 16 different slots: column & 7 | (row & 1) << 3
    auto wswz = [](int hh_, int hw_) -> int { return C::CINB == 256 ? ((hw_ & 7) | ((hh_ & 1) << 3)) : C::fswz(0, hh_, hw_); };

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_h;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tps = a.tiles_d * a.tiles_h * a.tiles_w;
    int n, tix;
    if (a.xcd_pin) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        n = xcd + 8 * (j / tps);
        tix = j % tps;
    } else {
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
        n = lin / tps;
        tix = lin % tps;
    }
    const int w0 = (tix % a.tiles_w) * TW;
    const int h0 = ((tix / a.tiles_w) % a.tiles_h) * TH;
    const int d0 = (tix / (a.tiles_w * a.tiles_h)) * TD;
    const T* __restrict__ x = (const T*)a.x + (size_t)n * a.D * a.H * a.W * CIN;

    // ---- halo DMA, all four waves ----
    for (int i = wave; i < NI_H; i += 4) {
        const int q = i * 64 + lane;
        const int hv = q / C::NVV, pv = q % C::NVV;
        const int hw_ = hv % C::PW, hh_ = (hv / C::PW) % C::HH, hd_ = hv / (C::PW * C::HH);
        const int lv = pv ^ wswz(hh_, hw_);
        const int id = d0 - 1 + hd_, ih = h0 - 1 + hh_, iw = w0 - 1 + hw_;
        const bool ok = hv < C::HV && ((unsigned)id < (unsigned)a.D) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
        const void* src = ok ? (const void*)(x + (((size_t)id * a.H + ih) * a.W + iw) * CIN + lv * C::VEC) : zero_page;
        dma16_uniform(src, lds0 + i * 1024);
    }

    // ---- roles ----
    const int cb = NB == 1 ? 0 : NB == 2 ? (wave & 1) : wave;             // Cout block of 32
    const int p0 = NB == 1 ? wave : NB == 2 ? 2 * (wave >> 1) : 0;        // first output plane of this wave's fragments
    const int vl = lane & 31, hh = lane >> 5;
    // voxel-fragment addresses: fragment f = (plane p0 + f / 2, rows 4 (f & 1) + vl / 8, column vl % 8); tap (kd, kh, kw), K block g:
    //   (lp[kh*3+kw][f & 1] ^ (g << 5)) + (f / 2 + kd) planes
    unsigned lp[9][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int th = 4 * i + (vl >> 3), tw = vl & 7;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
                lp[kh * 3 + kw][i] = lds0 + ((p0 * C::HH + th + kh) * C::PW + tw + kw) * C::CINB + ((hh ^ wswz(th + kh, tw + kw)) << 4);
    }
    // weight fragments: unit u = tap * G + g -> 1 KB at ((u * NB + cb) * 64 + lane) * 16 bytes
    const T* wl = (const T*)a.wfrag + ((size_t)cb * 64 + lane) * 8;
    auto load_w = [&](int u) -> V16 {
        V16 v;
        v.u = *(const uint4*)(wl + (size_t)u * NB * 64 * 8);
        return v;
    };
    constexpr int NU = 27 * G, WD = 4;
    V16 wf[WD + 1];
#pragma unroll
    for (int u = 0; u < WD; ++u) wf[u] = load_w(u);

    // ---- output offsets; the residual is requested before the tap loop when the register budget allows ----
    const size_t ldc = (size_t)a.ldc;
    const bool has_res = a.res != nullptr;
    auto out_off = [&](int f) -> size_t {
        const int td = p0 + (f >> 1), th = 4 * (f & 1) + (vl >> 3), tw = vl & 7;
        return ((((size_t)n * a.D + d0 + td) * a.H + h0 + th) * a.W + w0 + tw) * ldc + 32 * cb + 8 * hh;
    };
    uint4 rq[PRE_RES ? FR : 1][2];
    if (PRE_RES) {
#pragma unroll
        for (int f = 0; f < FR; ++f)
#pragma unroll
            for (int q = 0; q < 2; ++q)
                rq[PRE_RES ? f : 0][q] = has_res ? *(const uint4*)((const T*)a.res + out_off(f) + 16 * q) : make_uint4(0, 0, 0, 0);
    }

    f32x16 acc[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[f][e] = 0.f;

    // the halo pieces are the oldest vector-memory operations of this wave: wait for everything once (weights and residual are
    // needed soon anyway), then the workgroup barrier publishes the image
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    V16 xa[2][FR];
    auto load_x = [&](auto uc, V16 (&dst)[FR]) {
        constexpr int u = decltype(uc)::value;
        constexpr int tap = u / G, g = u % G;
        constexpr int kd = tap / 9, khkw = tap % 9;
        const unsigned a0 = lp[khkw][0] ^ (g << 5), a1 = lp[khkw][1] ^ (g << 5);
        // planes whose offset does not fit the 16-bit ds_read immediate (256-byte voxels: 25600 B per plane) go through a
        // second base three planes up, so that no read needs its own address register
        constexpr int HI = 3 * PLANE_B;
        const unsigned b0 = a0 + HI, b1 = a1 + HI;
        static_for<0, FR>([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            constexpr int off = ((f >> 1) + kd) * PLANE_B;
            if constexpr (off + 16 <= 65536) dst[f].u = *(const uint4*)((lptr_t)(size_t)(((f & 1) ? a1 : a0) + off));
            else dst[f].u = *(const uint4*)((lptr_t)(size_t)(((f & 1) ? b1 : b0) + (off - HI)));
        });
    };
    load_x(std::integral_constant<int, 0>{}, xa[0]);
    static_for<0, NU>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        if constexpr (u + WD < NU) wf[(u + WD) % (WD + 1)] = load_w(u + WD);
        if constexpr (u + 1 < NU) load_x(std::integral_constant<int, u + 1>{}, xa[(u + 1) & 1]);
#pragma unroll
        for (int f = 0; f < FR; ++f)
            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[u % (WD + 1)].h, xa[u & 1][f].h, acc[f], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);               // keep the prefetch distances (the scheduler sinks the loads otherwise)
    });

    // ---- epilogue from the accumulators: lane (voxel, h) holds channels 32 cb + 8 h + e (e < 8) and 32 cb + 16 + 8 h + (e - 8) ----
    float esc[16], esf[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = 32 * cb + 16 * (e >> 3) + 8 * hh + (e & 7);
        const float bi = a.bias ? a.bias[c] : 0.f, sc = a.scale ? a.scale[c] : 1.f, sf = a.shift ? a.shift[c] : 0.f;
        esc[e] = sc; esf[e] = bi * sc + sf;
    }
    const EpiFloors fl = epi_floors(a.flags);
#pragma unroll
    for (int f = 0; f < FR; ++f) {
        const size_t oo = out_off(f);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint4 rv;
            if (PRE_RES) rv = rq[PRE_RES ? f : 0][q];
            else rv = has_res ? *(const uint4*)((const T*)a.res + oo + 16 * q) : make_uint4(0, 0, 0, 0);
            const unsigned rr[4] = {rv.x, rv.y, rv.z, rv.w};
            unsigned o[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int e = 8 * q + 2 * d;
                const float v0 = epi_apply(fmaf(acc[f][e], esc[e], esf[e]), fl, __uint_as_float(rr[d] << 16));
                const float v1 = epi_apply(fmaf(acc[f][e + 1], esc[e + 1], esf[e + 1]), fl, __uint_as_float(rr[d] & 0xffff0000u));
                o[d] = pack_bf16x2(v0, v1);
            }
            *(uint4*)((T*)a.y + oo + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// lt_conv_fwd packing [cout_pad][k_pad] (k = tap * cin + ci) -> fragments of the transposed product:
// [tap][cin / 16][cout_pad / 32][64 lanes][8]; lane (r = l & 31, h = l >> 5) holds row chan(r) + 32 block, K elements 16 g + 8 h .. + 7
__global__ void conv_pack_t32_kernel(const bf16_t* __restrict__ w, int cout_pad, int k_pad, int cin, int ntaps, bf16_t* __restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nbk = cout_pad / 32, ng = cin / 16;
    if (g >= (long long)ntaps * ng * nbk * 64) return;
    const int l = (int)(g & 63);
    long long ft = g >> 6;
    const int nb = (int)(ft % nbk); ft /= nbk;
    const int kg = (int)(ft % ng);
    const int tap = (int)(ft / ng);
    const int r = l & 31, h = l >> 5;
    const int chan = 32 * nb + 16 * (r >> 4) + 8 * ((r >> 2) & 1) + 4 * ((r >> 3) & 1) + (r & 3);
    *(uint4*)(out + g * 8) = *(const uint4*)(w + (size_t)chan * k_pad + (size_t)tap * cin + 16 * kg + 8 * h);
}

template <typename T, int CIN, int CP>
int launch_halo_wreg(const HaloArgs& a, hipStream_t s) {
    typedef HaloCfg<T, 3, CIN, CP, 3, 3> C;
    static_assert(C::HALO_BYTES <= 160 * 1024, "the halo must fit LDS");
    auto kern = conv3d_halo_wreg_kernel<T, CIN, CP>;
    LT_OPT_IN_LDS(kern, 160 * 1024);
    const long long nblk = (long long)a.N * a.tiles_d * a.tiles_h * a.tiles_w;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), C::HALO_BYTES, s, a);
    LT_CHECK_LAUNCH("lt_conv_fwd(halo, weights from registers)");
    return LT_OK;
}

}  // namespace

namespace lt {

int conv3d_halo_wreg_try(int cin, int cout_pad, const HaloArgs& a, hipStream_t s) {
    int rc;
    if (cin == 64 && cout_pad == 64) rc = launch_halo_wreg<bf16_t, 64, 64>(a, s);
    else if (cin == 16 && cout_pad == 32) rc = launch_halo_wreg<bf16_t, 16, 32>(a, s);
    else if (cin == 32 && cout_pad == 64) rc = launch_halo_wreg<bf16_t, 32, 64>(a, s);
    else if (cin == 128 && cout_pad == 128) rc = launch_halo_wreg<bf16_t, 128, 128>(a, s);
    else return 0;
    return rc == LT_OK ? 1 : rc;
}

}  // namespace lt

extern "C" int lt_conv_pack_weights_t32(const void* weight, int32_t cout_pad, int32_t k_pad, int32_t cin, int32_t ntaps, void* packed,
                                        void* stream) {
    LT_REQUIRE(weight && packed, LT_ERR_INVALID, "lt_conv_pack_weights_t32: null argument");
    LT_REQUIRE(cout_pad >= 32 && cout_pad % 32 == 0 && cin >= 16 && cin % 16 == 0 && ntaps >= 1 && (long long)ntaps * cin <= k_pad && k_pad % 8 == 0,
               LT_ERR_INVALID, "lt_conv_pack_weights_t32: cout_pad %d / cin %d / ntaps %d / k_pad %d", cout_pad, cin, ntaps, k_pad);
    const long long total = (long long)ntaps * (cin / 16) * (cout_pad / 32) * 64;
    hipLaunchKernelGGL(conv_pack_t32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)weight,
                       cout_pad, k_pad, cin, ntaps, (bf16_t*)packed);
    LT_CHECK_LAUNCH("lt_conv_pack_weights_t32");
    return LT_OK;
}
