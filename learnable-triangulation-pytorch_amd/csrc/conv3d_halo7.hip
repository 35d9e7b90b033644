// 3D halo convolution, the bf16 7^3 32 -> 16 kernels of V2V's front layer: the one-tile kernel with loader waves and the column walk, around the tap nest
// they share.  Overview, LDS images and the dispatch table: conv3d_halo.hip; the shared parts: conv3d_halo.h.
#include "conv3d_halo.h"

namespace {

// ---- 7^3 kernel with loader waves -------------------------------------------------------------------------------------------
// PMC on the ring version (conv3d_halo_kernel, PD 2) (7^3 32->16 at 64^3): 3.3 VALU + 3.4 SALU + 1.3 LDS instructions per MFMA and no LDS bank
// conflicts -- with one workgroup per CU (the halo takes 123 KB) and so one compute wave per SIMD, the kernel was bound by
// the INSTRUCTIONS a wave issues between MFMAs (address arithmetic per chunk, the weight DMA and its ~100-cycle issue
// stalls, waitcnt bookkeeping): ~210 cycles per tap against 64 cycles of MFMA.  Here:
//   * waves 4-7 are loaders: halo + the whole weight stream (343 KB per tile, NBUF-deep chunk ring); waves 0-3 never issue
//     a memory instruction inside the tap loop;
//   * a chunk is one (kd, kh) row of 7 taps; kd is the only runtime loop: (kh, kw) offsets are ds_read immediates, the
//     fragment base registers are rebased once per kd (16 v_add per 49 taps), the weight buffer base once per chunk;
//   * fragments: hand-issued reads two taps ahead across chunk boundaries (15 reads in flight = the lgkmcnt counter).
// Measured (B = 16, 64^3): 2261 -> 1550 us (~105 cycles per tap; the LDS fragment reads alone need ~81: 20 ds_read_b128 per
// tap and CU).  Tried and dropped: a 5-deep instead of 4-deep weight ring (no change, kept), walking several tiles per
// workgroup with the next tile's first halo planes prefetched into the planes the tap loop has passed, and separate halo /
// weight loader waves (both ~10 % slower: the plane bursts delay the weight pieces queued behind them).  The next lever is
// LDS traffic: keeping the 7 kd-taps of one (kh, kw) in registers and sweeping the 10 input planes (17 reads per 28 MFMAs).
// (conv3d_halo7_kernel, the tap-major kernel these notes describe, was superseded by the kd-register-blocked variant below and removed
// in round 2; its measurements stay because they motivate that variant.)

// ---- 7^3 kernel, kd-register-blocked variant ------------------------------------------------------------------------------------
// conv3d_halo7_kernel reads five fragments from LDS per four MFMAs (one voxel fragment per output plane + the tap's weights) and
// is bound by those reads (81 of 105 cycles per tap).  Output plane td and tap plane kd meet in halo plane hd = td + kd, so for a
// fixed (kh, kw) ONE voxel fragment of plane hd serves every (td, kd) pair on that diagonal: a compute wave now owns two h rows
// of all four output planes (four accumulator tiles, one per td), keeps the seven kd weight fragments of the current (kh, kw)
// in registers and sweeps the ten halo planes -- 10 + 7 fragment reads per 28 MFMAs instead of 35.  A chunk of the weight ring
// is the seven kd slabs of one (kh, kw); the next chunk's slabs are read into the other register set while this one computes;
// the whole tap nest is unrolled (49 chunks), every LDS offset is an immediate.
constexpr int h7_lpos(int hd) { return hd < 6 ? hd : 2 * hd - 5; }                  // position of A_hd in a chunk's read stream
// global stream position of A_hd of chunk c (49 chunks, 17 entries each but the last, after the 7 entries of B(0)), and how far the
// stream must have been issued before that fragment is waited for
constexpr int h7_gpos(int c, int hd) { return 7 + 17 * c + (c == 48 ? hd : h7_lpos(hd)); }
constexpr int h7_target(int c, int hd, int look, int gend) { return h7_gpos(c, hd) + 1 + look < gend ? h7_gpos(c, hd) + 1 + look : gend; }

// The 49-chunk tap nest of a compute wave, shared by conv3d_halo7b_kernel and conv3d_halo7_col_kernel: one s_barrier per chunk (the loaders have chunks
// <= c+1 in LDS), the hand-issued read stream, the (chunk, hd, td) MFMA order.  Halo plane hd is read at ab[hd / PPB][kw & 3] + (hd % PPB) planes +
// the (kh, kw) immediate: PPB = 5 for the one-tile kernel (planes 0-4 / 5-9 behind two bases, the ds_read offset field holds five planes), PPB = 2 for
// the column walk's plane ring (a pair of planes never straddles the ring's wrap).  after_first_barrier: trace hook (halo and first chunks landed).
template <typename T, int PPB, int NAB, typename ACC, typename F1>
__device__ __forceinline__ void halo7_tap_nest(ACC (&acc)[4], const unsigned (&ab)[NAB][4], const unsigned bbase, F1&& after_first_barrier) {
    constexpr int KS = 7, NBUF = 5;
    typedef HaloCfg<T, KS, 32, 16, 7, 4> C;
    constexpr int TD = C::TD, MF = C::MF, CINB = C::CINB;
    constexpr int NCH = KS * KS;                         // 49 chunks: c = kh*7 + kw, each the 7 kd slabs of that (kh, kw)
    static_assert(NCH == 49, "h7_gpos assumes 49 chunks");
    constexpr int KDSTEP = C::HH * C::PW * CINB;         // bytes per d-plane of the halo image
    constexpr int HDN = TD + KS - 1;                     // 10 halo planes
    static_assert(NAB * PPB == HDN && (PPB - 1) * KDSTEP + ((KS - 1) * C::PW + KS - 1) * CINB < 65536, "plane bases / ds_read offset field");
    // global read stream: [B(0) x 7] + per chunk c < 48: [A0..A5, B'0, A6, B'1, A7, B'2, A8, B'3, A9, B'4, B'5, B'6] (B' = chunk c+1)
    //                                + last chunk: [A0..A9];  LOOK entries of lookahead (the first B' of a chunk sits at position 6,
    //                                so the lookahead out of the previous chunk never reaches weights that may not have landed)
    constexpr int LOOK = 6, SLEN = 17, GEND = 7 + SLEN * (NCH - 1) + HDN;
    V16 fa[HDN], fbk[2][KS];
    auto issue = [&](auto gic) {
        constexpr int gi = decltype(gic)::value;
        if constexpr (gi < 7) {
            lds_read16<gi * 1024>(fbk[0][gi], bbase);                              // chunk 0 lives in ring slot 0
        } else {
            constexpr int c = (gi - 7) / SLEN < NCH - 1 ? (gi - 7) / SLEN : NCH - 1;
            constexpr int q = gi - 7 - c * SLEN;
            constexpr int kh = c / KS, kw = c % KS;
            constexpr bool isA = q < 6 || c == NCH - 1 || (q <= 13 && (q & 1));   // positions 7, 9, 11, 13 are A6..A9
            if constexpr (isA) {
                constexpr int hd = (q < 6 || c == NCH - 1) ? q : (q + 5) / 2;
                constexpr int imm = (hd % PPB) * KDSTEP + (kh * C::PW + kw) * CINB;
                lds_read16<imm>(fa[hd], ab[hd / PPB][kw & 3]);
            } else {
                constexpr int kd = q <= 12 ? (q - 6) / 2 : q - 10;                 // 6,8,10,12 -> 0..3; 14,15,16 -> 4..6
                lds_read16<((c + 1) % NBUF) * C::WCH + kd * 1024>(fbk[(c + 1) & 1][kd], bbase);
            }
        }
    };
    static_for<0, NCH>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        asm volatile("s_barrier" ::: "memory");          // the loaders have chunks <= c+1 (and, the first time, the halo) in LDS
        if constexpr (c == 0) {
            after_first_barrier();
            static_for<0, 7 + LOOK>([&](auto gic) { issue(gic); });   // B(0) and the first LOOK entries of chunk 0
        }
        static_for<0, HDN>([&](auto hc) {
            constexpr int hd = decltype(hc)::value;
            constexpr int gp = h7_gpos(c, hd);
            constexpr int prev_target = (c == 0 && hd == 0) ? 7 + LOOK : (hd == 0 ? h7_target(c - 1, HDN - 1, LOOK, GEND) : h7_target(c, hd - 1, LOOK, GEND));
            constexpr int target = h7_target(c, hd, LOOK, GEND);
            static_for<prev_target, target>([&](auto gic) { issue(gic); });
            lgkm_wait<target - gp - 1>();
            frag_ready(fa[hd]);
            if constexpr (hd == 0) {
#pragma unroll
                for (int kd = 0; kd < KS; ++kd) frag_ready(fbk[c & 1][kd]);
            }
#pragma unroll
            for (int td = 0; td < TD; ++td) {
                if (hd - td >= 0 && hd - td < KS) LT_HMMA(acc[td], fa[hd], fbk[c & 1][hd - td]);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    });
}

#ifdef LT_TRACE
// the 7^3 kernels' record in g_trace_h (wave 0 of up to 64 sampled workgroups): [total, wait for the halo / plane group + first chunks, tile setup,
// -, tap nest, drain / seam barrier, epilogue, tiles]
#define LT_TR7(k_) { const long long c_ = LT_CLK(); tr[k_] += c_ - tr_last; tr_last = c_; }
#else
#define LT_TR7(k_)
#endif

template <typename T>
__global__ __launch_bounds__(512) void conv3d_halo7b_kernel(const HaloArgs a) {
    constexpr int KS = 7, CIN = 32, CP = 16, TPC = 7, NBUF = 5;
    typedef HaloCfg<T, KS, CIN, CP, TPC, 4> C;
    constexpr int TD = C::TD, TH = C::TH, TW = C::TW;
    static_assert(sizeof(T) == 2, "bf16 only");
    constexpr int MF = C::MF, NVV = C::NVV, VPR = C::VPR, CINB = C::CINB;
    static_assert(MF == 16 && NVV == 4 && C::SW::FSH == 0 && C::SW::FA == 0 && C::SW::FC == 0 && C::SLAB == 1024 && C::WCH == TPC * 1024, "7^3 32->16 layout");
    static_assert(C::HALO_BYTES + NBUF * C::WCH <= 160 * 1024, "halo + weight ring must fit LDS");
    typedef typename Mma<T, MF>::acc_t acc_t;
    constexpr int NCH = KS * KS;                         // 49 chunks: c = kh*7 + kw, each the 7 kd slabs of that (kh, kw)
    static_assert(NCH == 49, "h7_gpos assumes 49 chunks");
    constexpr int KDSTEP = C::HH * C::PW * CINB;         // bytes per d-plane of the halo image
    constexpr int NI_H = C::HALO_BYTES / 1024;
#ifdef LT_TRACE
    long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
    const long long tr_begin = LT_CLK();
    long long tr_last = tr_begin;
#endif

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned lds_w = lds0 + C::HALO_BYTES;

    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_h;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool loader = wave >= 4;
    const int wl = wave & 3;
    constexpr int P = KS / 2;

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

    if (loader) {
        // ================================= loader waves =================================
        const T* __restrict__ x = (const T*)a.x + (size_t)n * a.D * a.H * a.W * CIN;
        const T* __restrict__ w = (const T*)a.w;
        for (int i = wl; i < NI_H; i += 4) {
            const int q = i * 64 + lane;
            const int hv = q / NVV, pv = q % NVV;
            const int hw_ = hv % C::PW, hh_ = (hv / C::PW) % C::HH, hd_ = hv / (C::PW * C::HH);
            const int lv = pv ^ C::fswz(hd_, hh_, hw_);
            const int id = d0 - P + hd_, ih = h0 - P + hh_, iw = w0 - P + hw_;
            const bool ok = hv < C::HV && hw_ < C::HW && ((unsigned)id < (unsigned)a.D) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
            const void* src = ok ? (const void*)(x + (((size_t)id * a.H + ih) * a.W + iw) * CIN + lv * C::VEC) : zero_page;
            dma16_uniform(src, lds0 + i * 1024);
        }
        // chunk c = (kh, kw): slab kd is tap kd*49 + c; this loader carries kd = wl (and wl + 4 when < 7)
        const int pv = lane % NVV, col = lane / NVV;
        const int lv = pv ^ ((-(col / VPR)) & (NVV - 1));
        const T* wsrc0 = w + (size_t)col * a.k_pad + (size_t)wl * NCH * CIN + lv * C::VEC;
        const T* wsrc1 = wsrc0 + (size_t)4 * NCH * CIN;
        const bool two = wl + 4 < KS;
        const int dpc = two ? 2 : 1;
        auto stage_w = [&](int c) {
            const unsigned dst = lds_w + (c % NBUF) * C::WCH;
            dma16_uniform(wsrc0 + (size_t)c * CIN, dst + wl * 1024);
            if (two) dma16_uniform(wsrc1 + (size_t)c * CIN, dst + (wl + 4) * 1024);
        };
#pragma unroll
        for (int c = 0; c < NBUF - 1; ++c) stage_w(c);
        for (int c = 0; c < NCH; ++c) {
            // chunks <= c+1 (and, before them, the halo) must have landed; at most NBUF-3 younger chunks stay in flight
            int younger = NCH - 2 - c;
            if (younger > NBUF - 3) younger = NBUF - 3;
            if (younger < 0) younger = 0;
            wait_vmcnt(younger * dpc);
            asm volatile("s_barrier" ::: "memory");
            if (c + NBUF - 1 < NCH) stage_w(c + NBUF - 1);
        }
        asm volatile("s_barrier" ::: "memory");          // the compute waves' "done with the LDS images" barrier
        return;
    }

    // ================================= compute waves =================================
    // wave -> output rows th = 2 wave + (r15 >> 3), tw = r15 & 7 of ALL four planes td (accumulator tile td)
    const int r15 = lane & 15, lvb = lane >> 4;
    const int th = 2 * wave + (r15 >> 3), tw = r15 & 7;
    float cbi, csc, csf;
    cbi = a.bias ? a.bias[r15] : 0.f; csc = a.scale ? a.scale[r15] : 1.f; csf = a.shift ? a.shift[r15] : 0.f;
    constexpr int E_LPR = CP / C::VEC, E_RPP = 64 / E_LPR;   // 2 lanes per output row, 32 rows per iteration, 2 iterations
    const bool vec_epi = (a.Cout % C::VEC == 0) && (a.ldc % C::VEC == 0);
    const int cq = (lane % E_LPR) * C::VEC;
    auto row_off = [&](int row) -> size_t {               // staging row = td*16 + rr  ->  element offset of (voxel, channel cq)
        const int td = row >> 4, rr = row & 15;
        return ((((size_t)n * a.D + d0 + td) * a.H + h0 + 2 * wave + (rr >> 3)) * a.W + w0 + (rr & 7)) * a.ldc + cq;
    };
    const bool has_res = a.res != nullptr;
    uint4 rp0 = make_uint4(0, 0, 0, 0), rp1 = rp0;
    if (vec_epi && has_res && cq < a.Cout) {
        rp0 = *(const uint4*)((const T*)a.res + row_off(lane / E_LPR));
        rp1 = *(const uint4*)((const T*)a.res + row_off(lane / E_LPR + E_RPP));
    }
    unsigned ab[2][4];                                   // halo fragment bases per swizzle variant (kw & 3): planes 0-4 / 5-9
#pragma unroll
    for (int vv = 0; vv < 4; ++vv) {
        ab[0][vv] = lds0 + (th * C::PW + tw) * CINB + ((lvb ^ ((tw + vv) & 3)) << 4);
        ab[1][vv] = ab[0][vv] + 5 * KDSTEP;
    }
    const int bsw = (-(r15 / VPR)) & (NVV - 1);
    const unsigned bbase = lds_w + r15 * CINB + ((lvb ^ bsw) << 4);

    acc_t acc[TD];
#pragma unroll
    for (int i = 0; i < TD; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;

    LT_TR7(2)
    halo7_tap_nest<T, 5, 2>(acc, ab, bbase, [&]() { LT_TR7(1) });
    LT_TR7(4)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave is done with the halo / weight images
    LT_TR7(5)

    // ---- epilogue: this wave's 64 rows (td*16 + rr) x 16 channels through a private fp32 LDS tile ----
    constexpr int EP_LD = CP + 4;
    float* ep = (float*)(smem + wave * (64 * EP_LD * 4));
#pragma unroll
    for (int td = 0; td < TD; ++td)
#pragma unroll
        for (int e = 0; e < 4; ++e) ep[(td * 16 + (lane >> 4) * 4 + e) * EP_LD + r15] = (acc[td][e] + cbi) * csc + csf;
    const EpiFloors fl = epi_floors(a.flags);
    if (vec_epi) {
        if (cq < a.Cout) {
            const unsigned no_res = has_res ? 0u : 0x80008000u;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int row = lane / E_LPR + it * E_RPP;
                const uint4 resv = it == 0 ? rp0 : rp1;
                const float* src = ep + row * EP_LD + cq;
                const float4 q0 = *(const float4*)src, q1 = *(const float4*)(src + 4);
                const float vv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                const unsigned ru[4] = {resv.x | no_res, resv.y | no_res, resv.z | no_res, resv.w | no_res};
                unsigned ou[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    ou[e] = pack_bf16x2(epi_apply(vv[2 * e], fl, __uint_as_float(ru[e] << 16)), epi_apply(vv[2 * e + 1], fl, __uint_as_float(ru[e] & 0xffff0000u)));
                *(uint4*)((T*)a.y + row_off(row)) = make_uint4(ou[0], ou[1], ou[2], ou[3]);
            }
        }
    } else {
        for (int idx = lane; idx < 64 * CP; idx += 64) {
            const int row = idx / CP, cc = idx - row * CP;
            if (cc >= a.Cout) continue;
            const size_t off = row_off(row) - cq + cc;
            const float rr = has_res ? elt<T>::ld((const T*)a.res + off) : -0.0f;
            elt<T>::st((T*)a.y + off, epi_apply(ep[row * EP_LD + cc], fl, rr));
        }
    }
#ifdef LT_TRACE
    {   // 64 workgroups spread evenly over the launch (the first ones start on an idle chip)
        const unsigned every = gridDim.x >= 64 ? gridDim.x / 64 : 1;
        if (wave == 0 && lane == 0 && blockIdx.x % every == 0 && blockIdx.x / every < 64) {
            LT_TR7(6)
            long long* o = g_trace_h + (blockIdx.x / every) * 8;
            o[0] = tr_last - tr_begin;
            for (int k = 1; k < 7; ++k) o[k] = tr[k];
            o[7] = 1;
        }
    }
#endif
}

// ---- 7^3 kernel, column walk --------------------------------------------------------------------------------------------------
// conv3d_halo7b_kernel starts a 512-thread / 158 KB workgroup per tile (one per CU: nothing hides its start), loads the whole ten-plane halo before
// the first MFMA, decodes every DMA piece's address with divisions, primes the weight ring from empty and runs its epilogue after a drain barrier.
// Here a persistent workgroup walks COLUMNS of tiles along d (dealt like conv3d_halo_col_kernel's); the tap nest is the same code (halo7_tap_nest),
// so the output is bit-identical.  Between two nests:
//   * the ten plane slots of the halo image are a RING: column plane p (input d index + 3) lives in slot p % 10, tile i reads planes 4i .. 4i+9 and
//     after its last chunk planes 4i+10 .. 4i+13 overwrite the four oldest (rotation 4i % 10 = 0, 4, 8, 2, 6): 49 KB per tile instead of 123.  A
//     plane is 12.25 DMA pieces, so pieces are cut on the IMAGE (piece j = image bytes 1024 j ..), not on the group: what a lane of piece j fetches
//     (slot, row, column, k-vector, h/w bounds) is decoded once per kernel / column, and per group a lane is active when its slot is one of the
//     group's (the pieces at a group's ends run under a half exec mask; piece 122's upper half is never active);
//   * fragment addresses: a base register per pair of planes and swizzle variant (slots rot + 2j, rot + 2j + 1 never straddle the wrap: rot is
//     even), rebuilt per tile with 20 v_add; the plane inside the pair and (kh, kw) stay ds_read immediates;
//   * the weight ring runs on across tiles and restarts at slot 0 per tile (the nest's slot offsets are immediates): chunks 45 .. 48 sit in
//     slots 0 .. 3, so the next tile's chunk k goes into slot k once chunk 45 + k is consumed -- chunks 0 .. 2 under the last chunks of the nest,
//     chunk 3 at the seam IN FRONT of the plane group (plane bursts queued ahead of weight pieces delay them);
//   * the seam is one barrier (every read of the four oldest planes is done); then the loaders request the plane group and the compute waves run
//     the epilogue of the tile they just finished while it is in flight.  The epilogue stages one output plane at a time (16 rows x 16 channels
//     fp32 per wave) in weight-ring slot 4, which is idle exactly then: its last chunk of a tile is 44, its next one is chunk 4 of the next tile,
//     staged after that tile's first chunk barrier -- which the compute waves reach only after their epilogue.  (The halo image cannot be aliased
//     any more, and the 2 KB LDS left beside image + ring hold no plane of four waves.)  Arithmetic and order are conv3d_halo7b_kernel's.
template <typename T>
__global__ __launch_bounds__(512) void conv3d_halo7_col_kernel(const HaloArgs a, const int total_cols) {
    constexpr int KS = 7, CIN = 32, CP = 16, TPC = 7, NBUF = 5;
    typedef HaloCfg<T, KS, CIN, CP, TPC, 4> C;
    constexpr int TD = C::TD, TH = C::TH, TW = C::TW;
    static_assert(sizeof(T) == 2, "bf16 only");
    constexpr int MF = C::MF, NVV = C::NVV, VPR = C::VPR, CINB = C::CINB;
    static_assert(MF == 16 && NVV == 4 && C::SLAB == 1024 && C::WCH == TPC * 1024, "7^3 32->16 layout");
    static_assert(C::SW::FA == 0 && C::SW::FB == 0 && C::SW::FC == 0 && C::SW::FSH == 0, "the swizzle must not depend on the plane (nor on the row)");
    static_assert(C::HALO_BYTES + NBUF * C::WCH <= 160 * 1024, "halo + weight ring must fit LDS");
    typedef typename Mma<T, MF>::acc_t acc_t;
    constexpr int NCH = KS * KS;                         // 49 weight chunks per tile
    constexpr int HDN = TD + KS - 1;                     // 10 halo planes = ring slots
    constexpr int PLANE_U = C::HH * C::PW * NVV;         // 16-byte units of one plane
    constexpr int KDSTEP = PLANE_U * 16;
    constexpr int NPC = (HDN * KDSTEP + 1023) / 1024;    // DMA pieces of the image (the last one half used)
    constexpr int MAXP = (NPC + 3) / 4;                  // pieces per loader wave
    static_assert(MAXP <= 32, "one bit per piece in okhw");
    constexpr int P = KS / 2;
    constexpr int EP_LD = CP + 4, EP_WAVE = 16 * EP_LD * 4;   // epilogue staging: one output plane of a wave
    static_assert(4 * EP_WAVE <= C::WCH, "the epilogue staging must fit one weight-ring slot");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned lds_w = lds0 + C::HALO_BYTES;

    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_h;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool loader = wave >= 4;
    const int wl = wave & 3;
    const int tpc = a.tiles_d;                           // tiles per column (>= 2)
    const int cps = a.tiles_h * a.tiles_w;               // columns per sample
    const int ncol = (total_cols - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int ntile = ncol * tpc;

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

    if (loader) {
        // ================================= loader waves =================================
        const T* __restrict__ w = (const T*)a.w;
        // chunk c = (kh, kw): slab kd is tap kd*49 + c; this loader carries kd = wl (and wl + 4 when < 7)
        const int wpv = lane % NVV, wcol = lane / NVV;
        const int wlv = wpv ^ ((-(wcol / VPR)) & (NVV - 1));
        const T* wsrc0 = w + (size_t)wcol * a.k_pad + (size_t)wl * NCH * CIN + wlv * C::VEC;
        const T* wsrc1 = wsrc0 + (size_t)4 * NCH * CIN;
        const bool two = wl + 4 < KS;
        const int dpc = two ? 2 : 1;
        auto stage_w = [&](int c) {
            const unsigned dst = lds_w + (c % NBUF) * C::WCH;
            dma16_uniform(wsrc0 + (size_t)c * CIN, dst + wl * 1024);
            if (two) dma16_uniform(wsrc1 + (size_t)c * CIN, dst + (wl + 4) * 1024);
        };
        // image piece wl + 4 m: the (slot, row, column, k-vector) this lane fetches, decoded once
        int poff[MAXP], pmeta[MAXP];                      // element offset from (the slot's plane, row h0, column w0); slot << 16 | hh << 8 | hw
#pragma unroll
        for (int m = 0; m < MAXP; ++m) {
            const int q = (wl + 4 * m) * 64 + lane;
            const int slot = q / PLANE_U, r = q - slot * PLANE_U;
            const int hv = r / NVV, pv = r % NVV;
            const int hh_ = hv / C::PW, hw_ = hv - hh_ * C::PW;
            const int lv = pv ^ C::fswz(0, hh_, hw_);
            poff[m] = ((hh_ - P) * a.W + hw_ - P) * CIN + lv * C::VEC;
            pmeta[m] = ((slot < HDN ? slot : 15) << 16) | (hh_ << 8) | hw_;   // slot 15: past the image, in no group
        }
        int icol = 0, kt = 0, in, ih0, iw0;
        unsigned okhw = 0;                                // bit m: piece m's (row, column) lies inside the sample for this column
        const T* __restrict__ gb = nullptr;               // plane d = 0, row h0, column w0 of the column's sample
        const ptrdiff_t pstep = (ptrdiff_t)a.H * a.W * CIN;
        auto enter_col = [&](int v) {
            col_of(v, in, ih0, iw0);
            okhw = 0;
#pragma unroll
            for (int m = 0; m < MAXP; ++m) {
                const int hh_ = (pmeta[m] >> 8) & 255, hw_ = pmeta[m] & 255;
                const bool ok = ((unsigned)(ih0 - P + hh_) < (unsigned)a.H) & ((unsigned)(iw0 - P + hw_) < (unsigned)a.W);
                okhw |= ok ? (1u << m) : 0u;
            }
            gb = (const T*)a.x + (((ptrdiff_t)in * a.D * a.H + ih0) * a.W + iw0) * CIN;
        };
        // column planes p0 .. p0 + np - 1 into their slots (p0 % 10 = rot); planes outside the volume come from the zero page
        auto issue_planes = [&](int p0, int rot, int np) {
#pragma unroll
            for (int m = 0; m < MAXP; ++m) {
                if (wl + 4 * m < NPC) {
                    int k = (pmeta[m] >> 16) - rot;
                    if (k < 0) k += HDN;
                    if (k < np) {
                        const int d = p0 + k - P;
                        const bool ok = ((okhw >> m) & 1u) && (unsigned)d < (unsigned)a.D;
                        const void* src = ok ? (const void*)(gb + d * pstep + poff[m]) : zero_page;
                        dma16_uniform(src, lds0 + (wl + 4 * m) * 1024);
                    }
                }
            }
        };
        enter_col(blockIdx.x);
#pragma unroll
        for (int c = 0; c < NBUF - 2; ++c) stage_w(c);
        stage_w(NBUF - 2);
        issue_planes(0, 0, HDN);
        for (int ti = 0; ti < ntile; ++ti) {
            const bool has_next = ti + 1 < ntile;
            for (int c = 0; c < NCH; ++c) {
                // chunks <= c+1 must have landed -- and in front of chunk 0 the plane group, requested after the tile's first four chunks: everything.
                // Younger requests that may stay in flight: two chunks in steady state; at the end of the nest the next tile's chunks 0, 1
                int younger = c == 0 ? 0 : NCH - 2 - c < NBUF - 3 ? NCH - 2 - c : NBUF - 3;
                if (c >= NCH - 2) younger = has_next ? c - (NCH - 3) : 0;
                wait_vmcnt(younger * dpc);
                asm volatile("s_barrier" ::: "memory");
                if (c + NBUF - 1 < NCH) stage_w(c + NBUF - 1);
                else if (has_next && c >= NCH - 3) stage_w(c - (NCH - 3));   // the next tile's chunks 0 .. 2 into the slots of chunks 45 .. 47
            }
            asm volatile("s_barrier" ::: "memory");      // seam: the compute waves are done with the tile's planes and with chunk 48
            if (has_next) {
                stage_w(NBUF - 2);
                if (++kt == tpc) {
                    kt = 0;
                    enter_col(blockIdx.x + ++icol * gridDim.x);
                    issue_planes(0, 0, HDN);
                } else {
                    const int p0 = 4 * kt + HDN - TD;    // tile kt reads planes 4 kt .. 4 kt + 9; the first six are there
                    issue_planes(p0, p0 % HDN, TD);
                }
            }
        }
        return;
    }

    // ================================= compute waves =================================
    // wave -> output rows th = 2 wave + (r15 >> 3), tw = r15 & 7 of ALL four planes td (accumulator tile td)
    const int r15 = lane & 15, lvb = lane >> 4;
    const int th = 2 * wave + (r15 >> 3), tw = r15 & 7;
    float cbi, csc, csf;
    cbi = a.bias ? a.bias[r15] : 0.f; csc = a.scale ? a.scale[r15] : 1.f; csf = a.shift ? a.shift[r15] : 0.f;
    // epilogue: lanes 0 .. 31 store the 16 rows of one output plane, two lanes (8 channels each) per row
    const bool vec_epi = (a.Cout % C::VEC == 0) && (a.ldc % C::VEC == 0);
    const int cq = (lane & 1) * C::VEC, er = (lane >> 1) & 15;
    const bool elane = lane < 32 && cq < a.Cout;
    const bool has_res = a.res != nullptr;
    const EpiFloors fl = epi_floors(a.flags);
    const unsigned no_res = has_res ? 0u : 0x80008000u;
    const size_t ldc = (size_t)a.ldc;
    const size_t wrow = (size_t)a.W * ldc, dstep = (size_t)a.H * wrow;    // next row / next plane, in elements
    const size_t voff = (er >> 3) * wrow + (er & 7) * ldc + cq;          // the lane's (row, channel run) inside the wave's two rows of a plane
    float* const ep = (float*)(smem + C::HALO_BYTES + (NBUF - 1) * C::WCH + wave * EP_WAVE);

    unsigned aoff[4];                                    // in-plane fragment offset per swizzle variant (kw & 3)
#pragma unroll
    for (int vv = 0; vv < 4; ++vv) aoff[vv] = (th * C::PW + tw) * CINB + ((lvb ^ ((tw + vv) & 3)) << 4);
    const int bsw = (-(r15 / VPR)) & (NVV - 1);
    const unsigned bbase = lds_w + r15 * CINB + ((lvb ^ bsw) << 4);

#ifdef LT_TRACE
    long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
    const long long tr_begin = LT_CLK();
    long long tr_last = tr_begin;
#endif
    int n, h0, w0, icol = 0, kt = 0;
    col_of(blockIdx.x, n, h0, w0);
    size_t tb = (((size_t)n * a.D * a.H + h0 + 2 * wave) * a.W + w0) * ldc;   // the wave's first row of output plane d0 of the tile
    int rot = 0;                                         // slot of the tile's halo plane 0: (4 kt) % 10
    for (int ti = 0; ti < ntile; ++ti) {
        unsigned ab[HDN / 2][4];
#pragma unroll
        for (int j = 0; j < HDN / 2; ++j) {
            int slot = rot + 2 * j;
            if (slot >= HDN) slot -= HDN;
            const unsigned sb = lds0 + slot * KDSTEP;
#pragma unroll
            for (int vv = 0; vv < 4; ++vv) ab[j][vv] = sb + aoff[vv];
        }
        // residual of this tile: requested here, a whole nest before the epilogue reads it (no memory instruction inside the nest)
        uint4 rp[TD];
#pragma unroll
        for (int td = 0; td < TD; ++td) rp[td] = make_uint4(0, 0, 0, 0);
        if (vec_epi && has_res && elane) {
#pragma unroll
            for (int td = 0; td < TD; ++td) rp[td] = *(const uint4*)((const T*)a.res + tb + td * dstep + voff);
        }
        acc_t acc[TD];
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
        LT_TR7(2)
        halo7_tap_nest<T, 2, HDN / 2>(acc, ab, bbase, [&]() { LT_TR7(1) });
        LT_TR7(4)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // seam: every wave is done with the tile's planes
        LT_TR7(5)

        // ---- epilogue of the tile, under the next plane group's flight: plane td through the wave's private fp32 tile ----
#pragma unroll
        for (int td = 0; td < TD; ++td) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ep[((lane >> 4) * 4 + e) * EP_LD + r15] = (acc[td][e] + cbi) * csc + csf;
            // (the tile is wave-private and LDS operations of one wave execute in order: no barrier)
            if (vec_epi) {
                if (elane) {
                    const float* src = ep + er * EP_LD + cq;
                    const float4 q0 = *(const float4*)src, q1 = *(const float4*)(src + 4);
                    const float vv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                    const unsigned ru[4] = {rp[td].x | no_res, rp[td].y | no_res, rp[td].z | no_res, rp[td].w | no_res};
                    unsigned ou[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        ou[e] = pack_bf16x2(epi_apply(vv[2 * e], fl, __uint_as_float(ru[e] << 16)), epi_apply(vv[2 * e + 1], fl, __uint_as_float(ru[e] & 0xffff0000u)));
                    *(uint4*)((T*)a.y + tb + td * dstep + voff) = make_uint4(ou[0], ou[1], ou[2], ou[3]);
                }
            } else {
                for (int idx = lane; idx < 16 * CP; idx += 64) {
                    const int row = idx / CP, cc = idx - row * CP;
                    if (cc >= a.Cout) continue;
                    const size_t off = tb + td * dstep + (row >> 3) * wrow + (row & 7) * ldc + cc;
                    const float rr = has_res ? elt<T>::ld((const T*)a.res + off) : -0.0f;
                    elt<T>::st((T*)a.y + off, epi_apply(ep[row * EP_LD + cc], fl, rr));
                }
            }
        }
        // next tile of the column (strides, no divisions), or the next column
        tb += TD * dstep;
        rot = rot + TD >= HDN ? rot + TD - HDN : rot + TD;
        if (++kt == tpc && ti + 1 < ntile) {
            kt = 0; rot = 0;
            col_of(blockIdx.x + ++icol * gridDim.x, n, h0, w0);
            tb = (((size_t)n * a.D * a.H + h0 + 2 * wave) * a.W + w0) * ldc;
        }
        LT_TR7(6)
    }
#ifdef LT_TRACE
    if (wave == 0 && lane == 0 && (blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 64) {
        long long* o = g_trace_h + (blockIdx.x >> 3) * 8;
        o[0] = tr_last - tr_begin;
        for (int k = 1; k < 7; ++k) o[k] = tr[k];
        o[7] = ntile;
    }
#endif
}

int launch_halo7_col(const HaloArgs& a, hipStream_t s) {
    typedef HaloCfg<bf16_t, 7, 32, 16, 7, 4> C;
    constexpr int LDS = C::HALO_BYTES + 5 * C::WCH;
    const int n_cu = lt::device_cu_count8();
    const int total_cols = a.N * a.tiles_h * a.tiles_w;  // % 8 == 0 and >= 256 (halo7_col_fits)
    const int grid = total_cols < n_cu ? total_cols : n_cu;
    auto kern = conv3d_halo7_col_kernel<bf16_t>;
    LT_OPT_IN_LDS(kern, 160 * 1024);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), LDS, s, a, total_cols);
    LT_CHECK_LAUNCH("lt_conv_fwd(halo 7^3, column walk)");
    return LT_OK;
}

int launch_halo7(const HaloArgs& a, hipStream_t s) {
    typedef HaloCfg<bf16_t, 7, 32, 16, 7, 4> C;
    constexpr int LDS = C::HALO_BYTES + 5 * C::WCH;
    const long long nblk = (long long)a.N * a.tiles_d * a.tiles_h * a.tiles_w;
    auto kern_b = conv3d_halo7b_kernel<bf16_t>;
    LT_OPT_IN_LDS(kern_b, 160 * 1024);
    hipLaunchKernelGGL(kern_b, dim3((unsigned)nblk), dim3(512), LDS, s, a);
    LT_CHECK_LAUNCH("lt_conv_fwd(halo 7^3, kd-blocked)");
    return LT_OK;
}

}  // namespace

namespace lt {

int conv3d_halo7_launch(const HaloArgs& a, bool column_walk, hipStream_t s) { return column_walk ? launch_halo7_col(a, s) : launch_halo7(a, s); }

#ifdef LT_TRACE
int conv3d_halo7_trace_read(long long* dst, int n) { return halo_trace_read(dst, n); }
#endif

}  // namespace lt
