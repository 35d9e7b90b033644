// 3D halo convolution, the one-tile kernel: a workgroup computes one 4 x 8 x 8 tile from its halo image in LDS, the weights stream through a chunk ring in
// LDS.  Every (operand type, filter, channel) combination without a kernel of its own runs here: thirteen instantiations, chosen by the rows of
// conv3d_halo_tile_try at the end.  Overview, LDS images and the dispatch table: conv3d_halo.hip; the shared parts: conv3d_halo.h.
#include "conv3d_halo.h"

namespace {

// LDR: eight waves, waves 4-7 are loaders (halo + weight chunk ring, nothing else); waves 0-3 then issue no DMA and wait on
// no vmcnt inside the tap loop (same idea as the 7^3 and the persistent kernels; non-ring path only)
// NPH > 1 (round 6, fp32 7^3 32 -> 16): CHANNEL PHASES.  The tensor has CIN * NPH channels per voxel; the halo tile of all of them does not fit LDS
// (10 x 14 x 14 voxels x 128 B = 245 KB), the tile of CIN of them does (123 KB, the byte geometry of the bf16 kernel).  The kernel walks all taps over
// channels [0, CIN), reloads the halo image with channels [CIN, 2 CIN) and walks the taps again; the accumulators live across the phases.  Every input
// voxel enters LDS once per tile and phase -- on the generic 256 x 16 tile it crossed L2 -> LDS once per TAP (343 times), and the eight-piece DMA issue
// per K step cost as much as its 32 MFMAs (51 % of the fp32 MFMA peak).
template <typename T, int KS, int CIN, int CP, int TPC, int NBUF, int PD, bool LDR, int NPH = 1>
__global__ __launch_bounds__(LDR ? 512 : 256) void conv3d_halo_kernel(const HaloArgs a) {
    typedef HaloCfg<T, KS, CIN, CP, TPC, NBUF> C;
    constexpr int TD = C::TD, TH = C::TH, TW = C::TW;
    static_assert(!LDR || PD == 1, "loader waves: non-ring path");
    static_assert(NPH == 1 || !LDR, "channel phases: no loader waves");
    constexpr int XLD = CIN * NPH;                       // channels per voxel of the tensor (and per tap of a weight row)
    // fp64 flush of the fp32 accumulators: every 4 taps of 32 channels = after 128 products; the 16-channel 7^3 and two-phase kernels flush every 8 taps -- the same 128
    // products (the 16 cvt + 16 v_add_f64 of a flush next to the 16 MFMAs of a 16-channel tap cost 10 % at every fourth tap)
    constexpr int AMASK = (sizeof(T) == 4 && CIN <= 16 && (KS == 7 || NPH > 1)) ? 2 * LT_ACC64_MASK + 1 : LT_ACC64_MASK;
    int cph = 0;                                         // the channel phase whose halo / weight images are in LDS (or on their way)
    constexpr bool ACC64 = sizeof(T) == 4;
    constexpr int MF = C::MF, SM = C::SM, SN = C::SN, G = C::G, NACC = C::NACC, NVV = C::NVV, VPR = C::VPR, CINB = C::CINB;
    typedef typename Mma<T, MF>::acc_t acc_t;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    unsigned char* s_halo = smem;
    unsigned char* s_w = smem + C::HALO_BYTES;

    // zero-page address made opaque once (else each use is an s_load from the GOT + s_waitcnt lgkmcnt(0) in the tap loop)
    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_h;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool is_loader = LDR && wave >= 4;
    const bool do_dma = !LDR || is_loader;
    const int dw = wave & 3;                             // index of this wave among the four that issue DMAs

    // ---- workgroup -> (sample, tile); with N % 8 == 0 sample n is pinned to XCD n % 8 (its d-slabs stay in that L2) ----
    const int tps = a.tiles_d * a.tiles_h * a.tiles_w;
    int n, tix;
    if (a.xcd_pin) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        n = xcd + 8 * (j / tps);
        tix = j % tps;
    } else {
        // other batch sizes: every XCD takes one contiguous run of the (sample, tile) raster
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
        n = lin / tps;
        tix = lin % tps;
    }
    const int w0 = (tix % a.tiles_w) * TW;
    const int h0 = ((tix / a.tiles_w) % a.tiles_h) * TH;
    const int d0 = (tix / (a.tiles_w * a.tiles_h)) * TD;
    constexpr int P = KS / 2;

    const T* __restrict__ x = (const T*)a.x + (size_t)n * a.D * a.H * a.W * XLD;
    const T* __restrict__ w = (const T*)a.w;

    // ---- halo DMA: vector q = hv*NVV + pv, wave-instruction i covers q in [64 i, 64 i + 64) ----
    constexpr int NI_H = C::HALO_BYTES / 1024;
    auto issue_halo = [&]() {
#ifndef LT_ABL_NO_A   // -DLT_ABL_*: timing ablations for profiling builds (results are WRONG with any of them)
        for (int i = dw; i < NI_H; i += 4) {
            const int q = i * 64 + lane;
            const int hv = q / NVV, pv = q % NVV;
            const int hw_ = hv % C::PW, hh_ = (hv / C::PW) % C::HH, hd_ = hv / (C::PW * C::HH);
            const int lv = pv ^ C::fswz(hd_, hh_, hw_);
            const int id = d0 - P + hd_, ih = h0 - P + hh_, iw = w0 - P + hw_;
            const bool ok = hv < C::HV && hw_ < C::HW && ((unsigned)id < (unsigned)a.D) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
            const void* src = ok ? (const void*)(x + (((size_t)id * a.H + ih) * a.W + iw) * XLD + cph * CIN + lv * C::VEC) : zero_page;
            dma16_uniform(src, lds0 + i * 1024);
        }
#endif
    };
    if (do_dma) issue_halo();
    // ---- weight chunk DMA: vector q = (tap_in_chunk*CP + col)*NVV + pv ----
    constexpr int NI_W = C::WCH / 1024;
    auto stage_w = [&](int ch, int buf) {
#ifdef LT_ABL_NO_B
        return;
#endif
        for (int i = dw; i < NI_W; i += 4) {
            const int q = i * 64 + lane;
            const int pv = q % NVV, col = (q / NVV) % CP, tj = q / (NVV * CP);
            const int tap = ch * TPC + tj;
            const int lv = pv ^ ((-(col / VPR)) & (NVV - 1));
            const bool ok = tj < TPC && tap < C::NTAPS;
            const void* src = ok ? (const void*)(w + (size_t)col * a.k_pad + tap * XLD + cph * CIN + lv * C::VEC) : zero_page;
            dma16_uniform(src, lds0 + C::HALO_BYTES + buf * C::WCH + i * 1024);
        }
    };
#ifdef LT_ABL_NO_B
    const int dpc = 0;
#else
    const int dpc = (NI_W - dw + 3) / 4;          // weight DMA instructions per chunk issued by this wave (wave-uniform)
#endif
    if (do_dma) {
#pragma unroll
        for (int c = 0; c < NBUF - 1; ++c)
            if (c < C::NCH) stage_w(c, c);
    }
    if (is_loader) {
        // ================================= loader waves: the chunk ring, then out =================================
        for (int ch = 0; ch < C::NCH; ++ch) {
            int younger = C::NCH - 1 - ch;
            if (younger > NBUF - 2) younger = NBUF - 2;
            wait_vmcnt(younger * dpc);
            asm volatile("s_barrier" ::: "memory");
            if (ch + NBUF - 1 < C::NCH) stage_w(ch + NBUF - 1, (ch + NBUF - 1) % NBUF);
        }
        asm volatile("s_barrier" ::: "memory");          // the compute waves' "done with the LDS images" barrier
        return;
    }

    HaloCst<SN> cst;
    cst.load(a, lane, MF);
    // ---- residual prefetch: the lane's 16-byte residual vectors (up to 8) are requested before the tap loop, in named
    // registers (see conv_igemm2.hip for why not an array); they are consumed in the epilogue ----
    constexpr int E_VECO = C::OVEC, E_LPR = CP / E_VECO, E_RPP = 64 / E_LPR, E_NIT = 64 / E_RPP;
    static_assert(E_NIT <= 16, "epilogue rows per lane");
    // (the 64-channel loader-wave configuration is at its 256-VGPR budget: it loads the residual in the epilogue instead)
    constexpr bool PRE_OK = E_NIT <= 8 && !(LDR && CINB == 128);
    const bool vec_epi = (a.Cout % E_VECO == 0) && (a.ldc % E_VECO == 0);
    const bool pre_res = PRE_OK && vec_epi && a.res != nullptr && !(a.flags & LT_EPI_NO_RES_PREFETCH);
    uint4 rp0, rp1, rp2, rp3, rp4, rp5, rp6, rp7;
    rp0 = rp1 = rp2 = rp3 = rp4 = rp5 = rp6 = rp7 = make_uint4(0, 0, 0, 0);
    if (pre_res) {
        const int cqp = (lane % E_LPR) * E_VECO;
        auto pf = [&](int it) -> uint4 {
            const int r = 64 * wave + lane / E_LPR + it * E_RPP;
            const int tw = r % TW, th = (r / TW) % TH, td = r / (TW * TH);
            const size_t pixv = (((size_t)n * a.D + d0 + td) * a.H + h0 + th) * a.W + w0 + tw;
            const void* src = cqp < a.Cout ? (const void*)((const typename C::OT*)a.res + pixv * a.ldc + cqp) : zero_page;
            return *(const uint4*)src;
        };
        if (E_NIT > 0) rp0 = pf(0);
        if (E_NIT > 1) rp1 = pf(1);
        if (E_NIT > 2) rp2 = pf(2);
        if (E_NIT > 3) rp3 = pf(3);
        if (E_NIT > 4) rp4 = pf(4);
        if (E_NIT > 5) rp5 = pf(5);
        if (E_NIT > 6) rp6 = pf(6);
        if (E_NIT > 7) rp7 = pf(7);
    }

    // ---- per-lane fragment addresses, hoisted out of the tap loop ----
    // PMC on the first version: 8.4 VALU + 6 SALU per MFMA (the 7^3 kernel was issue-bound on address arithmetic, not on
    // LDS or MFMA).  Now: A address = abase[kwv][g][i] (per lane: own voxel + swizzle term, which depends on the tap only
    // through kw -- or (kh,kw) for the 128-byte-voxel swizzle) + per-chunk scalar (kd / (kd,kh) plane or row offset)
    // + compile-time immediate (the rest of the tap offset).  The tap loop itself is ds_reads and MFMAs only.
    constexpr bool ROWCH = TPC == KS;                       // a chunk is one (kd,kh) row of taps; else one kd plane (TPC == KS*KS)
    static_assert(TPC == KS || TPC == KS * KS, "chunk = one tap row or one tap plane");
    constexpr bool KW_ONLY = C::SW::FA == 0 && C::SW::FC == 0;   // swizzle term independent of kh
    static_assert(C::SW::FB == 0, "swizzle must not depend on kd");
    static_assert(KW_ONLY || KS == 3, "kh-dependent swizzle only instantiated for 3^3");
    constexpr int NXV = KW_ONLY ? KS : KS * KS;             // swizzle variants
    const int lvb = (MF == 32) ? (lane >> 5) : (lane >> 4);   // logical vector of group 0; group g adds (MF==32 ? 2g : 4g)
    int abase[NXV][G][SM];                                  // bytes: own voxel * CINB + ((lv_g ^ f) << 4)
#pragma unroll
    for (int i = 0; i < SM; ++i) {
        const int r = 64 * wave + i * MF + (lane & (MF - 1));
        const int tw = r % TW, th = (r / TW) % TH, td = r / (TW * TH);
        const int own = ((td * C::HH + th) * C::PW + tw) * CINB;
#pragma unroll
        for (int v = 0; v < NXV; ++v) {
            const int kw = KW_ONLY ? v : v % KS, kh = KW_ONLY ? 0 : v / KS;
            const int f = C::fswz(0, th + kh, tw + kw);
#pragma unroll
            for (int g = 0; g < G; ++g) abase[v][g][i] = own + (((lvb + ((MF == 32) ? 2 * g : 4 * g)) ^ f) << 4);
        }
    }
    int bbase[G][SN];                                       // bytes inside a tap slab
#pragma unroll
    for (int j = 0; j < SN; ++j) {
        const int col = j * MF + (lane & (MF - 1));
        const int bsw = (-(col / VPR)) & (NVV - 1);
#pragma unroll
        for (int g = 0; g < G; ++g) bbase[g][j] = col * CINB + (((lvb + ((MF == 32) ? 2 * g : 4 * g)) ^ bsw) << 4);
    }

    acc_t acc[SM][SN];
    double dacc[ACC64 ? SM : 1][ACC64 ? SN : 1][ACC64 ? NACC : 1];
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < SN; ++j)
#pragma unroll
            for (int e = 0; e < NACC; ++e) {
                acc[i][j][e] = 0.f;
                if (ACC64) dacc[i][j][e] = 0.0;
            }

    if constexpr (PD > 1) {
        // ---- fragment RING (7^3): one workgroup per CU (the halo takes 123 KB) = one wave per SIMD, so nothing but the wave's
        // own lookahead hides the LDS latency; with the one-tap lookahead below the kernel ran at ~290 cycles per tap against
        // 64 cycles of MFMA.  Here the fragments of tap t+PD are requested before the MFMAs of tap t, across chunk boundaries:
        // ring slot = tap index inside the chunk (TPC slots), the halo image is static, and the weight ring runs one chunk
        // further ahead (chunk ch+1 has landed at the barrier of chunk ch) so that its fragments may be read early.
        static_assert(ROWCH && KW_ONLY && PD < TPC && NBUF >= 4, "ring path: row chunks, kw-only swizzle, >= 4 weight buffers");
        V16 fa[TPC][G][SM], fb[TPC][G][SN];
        constexpr int RPT = G * (SM + SN);                  // ds_reads per tap
        static_assert((PD + 1) * RPT <= 15, "lookahead exceeds the lgkmcnt counter");
        const unsigned lds_w = lds0 + C::HALO_BYTES;
        // tap TJ of the chunk whose halo row offset is coff_x and whose weight buffer starts at LDS byte wb_x
        auto load_ring = [&](int coff_x, unsigned wb_x, auto tjc) {
            constexpr int TJ = decltype(tjc)::value;
            static_for<0, G>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                static_for<0, SM>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    lds_read16<TJ * CINB>(fa[TJ][g][i], lds0 + abase[TJ][g][i] + coff_x);
                });
                static_for<0, SN>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    lds_read16<TJ * C::SLAB>(fb[TJ][g][j], wb_x + bbase[g][j]);
                });
            });
        };
        auto mma_tap = [&](auto tjc) {
            constexpr int TJ = decltype(tjc)::value;
#pragma unroll
            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int i = 0; i < SM; ++i) frag_ready(fa[TJ][g][i]);
#pragma unroll
                for (int j = 0; j < SN; ++j) frag_ready(fb[TJ][g][j]);
            }
            mma_tap_blocks<T, MF, SM, SN, G>(acc, fa[TJ], fb[TJ]);
        };
        // LAST_ (compile time): no chunk follows.  Two copies of the chunk body instead of a uniform branch around the
        // cross-chunk loads, so that the number of reads in flight at every wait is a compile-time constant.
#define LT_HALO_RING_CHUNK(LAST_)                                                                                       \
    {                                                                                                                   \
        /* chunks <= ch+1 must have landed; at most NBUF-3 younger chunks stay in flight */                             \
        int younger = C::NCH - 2 - ch;                                                                                  \
        if (younger > NBUF - 3) younger = NBUF - 3;                                                                     \
        if (younger < 0) younger = 0;                                                                                   \
        wait_vmcnt(younger * dpc);                                                                                      \
        asm volatile("s_barrier" ::: "memory"); /* all waves: chunks <= ch+1 landed, chunk ch-1 fully consumed */       \
        if (ch + NBUF - 1 < C::NCH) stage_w(ch + NBUF - 1, (ch + NBUF - 1) % NBUF);                                     \
        const int coff = (((ch / KS) * C::HH + (ch % KS)) * C::PW) * CINB; /* bytes, wave-uniform */                    \
        const int coff_n = ((((ch + 1) / KS) * C::HH + ((ch + 1) % KS)) * C::PW) * CINB;                                \
        const unsigned wb = lds_w + (ch % NBUF) * C::WCH;                                                               \
        const unsigned wb_n = lds_w + ((ch + 1) % NBUF) * C::WCH;                                                       \
        static_for<0, TPC>([&](auto tjc) {                                                                              \
            constexpr int tj = decltype(tjc)::value;                                                                    \
            constexpr int ahead = (tj + PD < TPC) ? PD : (LAST_ ? TPC - 1 - tj : PD); /* taps in flight behind tj */    \
            if constexpr (tj + PD < TPC) load_ring(coff, wb, std::integral_constant<int, tj + PD>{});                   \
            else if constexpr (!LAST_) load_ring(coff_n, wb_n, std::integral_constant<int, (tj + PD) % TPC>{});         \
            lgkm_wait<ahead * RPT>();                                                                                   \
            mma_tap(tjc);                                                                                               \
            if (ACC64 && (((ch * TPC + tj) & AMASK) == AMASK || ch * TPC + tj + 1 == C::NTAPS)) {                                               \
                _Pragma("unroll") for (int i = 0; i < SM; ++i)                                                          \
                    _Pragma("unroll") for (int j = 0; j < SN; ++j)                                                      \
                        _Pragma("unroll") for (int e = 0; e < NACC; ++e) {                                              \
                            dacc[i][j][e] += (double)acc[i][j][e];                                                      \
                            acc[i][j][e] = 0.f;                                                                         \
                        }                                                                                               \
            }                                                                                                           \
        });                                                                                                             \
    }
        for (int phase = 0; phase < NPH; ++phase) {
        if (NPH > 1 && phase) {          // next channel phase: every wave is done with the halo / weight images, then the same start-up as above
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            cph = phase;
            issue_halo();
#pragma unroll
            for (int c = 0; c < NBUF - 1; ++c)
                if (c < C::NCH) stage_w(c, c);
        }
        // prologue: the first PD taps of chunk 0 (needs the halo and chunk 0: same wait as the loop's first barrier)
        {
            int younger = C::NCH - 2;
            if (younger > NBUF - 3) younger = NBUF - 3;
            if (younger < 0) younger = 0;
            wait_vmcnt(younger * dpc);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            static_for<0, PD>([&](auto tjc) { load_ring(0, lds_w, tjc); });
        }
        int ch = 0;
        for (; ch < C::NCH - 1; ++ch) LT_HALO_RING_CHUNK(false)
        LT_HALO_RING_CHUNK(true)
        }
#undef LT_HALO_RING_CHUNK
    } else {
        for (int phase = 0; phase < NPH; ++phase) {
        if (NPH > 1 && phase) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            cph = phase;
            issue_halo();
#pragma unroll
            for (int c = 0; c < NBUF - 1; ++c)
                if (c < C::NCH) stage_w(c, c);
        }
        for (int ch = 0; ch < C::NCH; ++ch) {
            // chunk ch (and, the first time, the halo issued before it) must have landed; up to NBUF-2 younger chunks stay in flight
            int younger = C::NCH - 1 - ch;
            if (younger > NBUF - 2) younger = NBUF - 2;
            if (!LDR) wait_vmcnt(younger * dpc);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // all waves: chunk ch landed, chunk ch-1 fully consumed
            if (!LDR && ch + NBUF - 1 < C::NCH) stage_w(ch + NBUF - 1, (ch + NBUF - 1) % NBUF);
            // per-chunk scalar parts
            const int kd = ROWCH ? ch / KS : ch, kh_row = ROWCH ? ch % KS : 0;
            const int coff = ((kd * C::HH + kh_row) * C::PW) * CINB;           // bytes, wave-uniform
            const unsigned char* wb = s_w + (ch % NBUF) * C::WCH;
            // Fragments of tap tj+1 are requested before the MFMAs of tap tj are issued (register double buffer, order pinned
            // with sched_barrier): with one wave per SIMD nothing else hides the ~100-cycle ds_read latency.
            // kh-dependent swizzle with row chunks: pick this row's variants with a wave-uniform switch (keeps every register
            // index static: a select chain here was turned into a dynamically indexed array = scratch memory)
            int arow[(ROWCH && !KW_ONLY) ? KS : 1][G][SM];
            if (ROWCH && !KW_ONLY) {
                switch (kh_row) {
                    case 0:
    #pragma unroll
                        for (int k = 0; k < KS; ++k)
    #pragma unroll
                            for (int g = 0; g < G; ++g)
    #pragma unroll
                                for (int i = 0; i < SM; ++i) arow[k][g][i] = abase[(0 * KS + k) % NXV][g][i];
                        break;
                    case 1:
    #pragma unroll
                        for (int k = 0; k < KS; ++k)
    #pragma unroll
                            for (int g = 0; g < G; ++g)
    #pragma unroll
                                for (int i = 0; i < SM; ++i) arow[k][g][i] = abase[(1 * KS + k) % NXV][g][i];
                        break;
                    default:
    #pragma unroll
                        for (int k = 0; k < KS; ++k)
    #pragma unroll
                            for (int g = 0; g < G; ++g)
    #pragma unroll
                                for (int i = 0; i < SM; ++i) arow[k][g][i] = abase[(2 * KS + k) % NXV][g][i];
                        break;
                }
            }
            V16 fa[2][G][SM], fb[2][G][SN];
            auto load_tap = [&](int tj, int slot) {     // tj is a compile-time constant after unrolling
                const int kw = ROWCH ? tj : tj % KS, kh = ROWCH ? 0 : tj / KS;
                const int imm = (kh * C::PW + kw) * CINB;                       // compile-time immediate
    #pragma unroll
                for (int g = 0; g < G; ++g) {
    #pragma unroll
                    for (int i = 0; i < SM; ++i) {
                        int ab;
                        if (KW_ONLY) ab = abase[kw][g][i];
                        else if (!ROWCH) ab = abase[kh * KS + kw][g][i];
                        else ab = arow[kw][g][i];
                        fa[slot][g][i].u = *(const uint4*)(s_halo + (ab + coff) + imm);
                    }
    #pragma unroll
                    for (int j = 0; j < SN; ++j) fb[slot][g][j].u = *(const uint4*)(wb + bbase[g][j] + tj * C::SLAB);
                }
            };
            load_tap(0, 0);
    #pragma unroll
            for (int tj = 0; tj < TPC; ++tj) {
                const int tap = ch * TPC + tj;
                if (tap < C::NTAPS) {
                    if (tj + 1 < TPC && tap + 1 < C::NTAPS) load_tap(tj + 1, (tj + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                    mma_tap_blocks<T, MF, SM, SN, G>(acc, fa[tj & 1], fb[tj & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (ACC64 && ((tap & AMASK) == AMASK || tap + 1 == C::NTAPS)) {
    #pragma unroll
                        for (int i = 0; i < SM; ++i)
    #pragma unroll
                            for (int j = 0; j < SN; ++j)
    #pragma unroll
                                for (int e = 0; e < NACC; ++e) {
                                    dacc[i][j][e] += (double)acc[i][j][e];
                                    acc[i][j][e] = 0.f;
                                }
                    }
                }
            }
        }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave is done with the halo / weight images

#ifdef LT_ABL_NO_EPI
    if (a.N < 0)
#endif
    halo_epilogue<T, CP, MF, SM, SN, NACC, ACC64>(smem, a, wave, lane, n, d0, h0, w0, acc, dacc, pre_res, rp0, rp1, rp2, rp3, rp4, rp5,
                                                         rp6, rp7, cst);
}

template <typename T, int KS, int CIN, int CP, int TPC, int NBUF, int PD, bool LDR, int NPH = 1>
int launch_halo(const HaloArgs& a, hipStream_t s) {
    typedef HaloCfg<T, KS, CIN, CP, TPC, NBUF> C;
    static_assert(C::LDS_BYTES <= 160 * 1024, "halo tile does not fit LDS");
    auto kern = conv3d_halo_kernel<T, KS, CIN, CP, TPC, NBUF, PD, LDR, NPH>;
    LT_OPT_IN_LDS(kern, 160 * 1024);
    const long long nblk = (long long)a.N * a.tiles_d * a.tiles_h * a.tiles_w;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(LDR ? 512 : 256), C::LDS_BYTES, s, a);
    LT_CHECK_LAUNCH("lt_conv_fwd(halo)");
    return LT_OK;
}

}  // namespace

namespace lt {

// The rows of the one-tile kernel.  Their keys (dtype, ks, cin, cout_pad) are disjoint -- also from the rows of the other families in conv3d_halo_try --
// except where an A/B switch sends a row's layers on to the row below (LT_HALO_F3).  0: no row matches, the caller takes the implicit-GEMM path.
int conv3d_halo_tile_try(int dtype, int ks, int cin, int cout_pad, const HaloArgs& a, hipStream_t s) {
    // conv3d_halo_kernel<T, KS, CIN, CP, TPC, NBUF, PD, LDR> for a KS^3 layer of CIN -> CP channels
#define HALO_CASE(T_, KS_, CIN_, CP_, ...)                                                       \
    if (ks == KS_ && cin == CIN_ && cout_pad == CP_) {                                          \
        int rc = launch_halo<T_, KS_, CIN_, CP_, __VA_ARGS__>(a, s);                            \
        return rc == LT_OK ? 1 : rc;                                                            \
    }
    if (dtype == LT_FP8) {
        // e4m3 operands (train_precision 'fp8v2v'): the one-tile loader-wave kernel at half the bytes per voxel / per weight slab; bf16 stores.  The byte
        // geometries are the bf16 ones of half the channel count: (64, 64) = bf16 (32 -> 64), (32, 32) = bf16 (16 -> 32)
        if (a.Cout % 8 || a.ldc % 8) return 0;
        HALO_CASE(fp8_t, 3, 64, 64, 9, 2, 1, true)
        HALO_CASE(fp8_t, 3, 32, 32, 9, 2, 1, true)
        HALO_CASE(fp8_t, 3, 32, 64, 9, 2, 1, true)
        return 0;
    }
    if (dtype == LT_BF16) {
        HALO_CASE(bf16_t, 3, 64, 64, 3, 3, 1, true)
        HALO_CASE(bf16_t, 3, 32, 32, 9, 2, 1, true)
        HALO_CASE(bf16_t, 3, 16, 32, 9, 2, 1, true)
        HALO_CASE(bf16_t, 3, 32, 64, 9, 2, 1, true)
        // round 6: 7^3 16 -> 32 = the INPUT GRADIENT of the front layer in the 16-bit training step (the flipped / transposed filter): it ran on the generic
        // 256 x 32 implicit-GEMM tile with four taps per 128-byte K step (1.78 ms at 8 samples, 4.2 % of the step's kernel time); LT_HALO_NO_D7=1: that tile again (A/B)
        if (!env_on("LT_HALO_NO_D7")) { HALO_CASE(bf16_t, 7, 16, 32, 7, 4, 2, false) }
    } else {
        // round 6: 3^3 32 -> 32 (nine layers at 64^3, 23 % of the exact-fp32 forward) in two channel phases of 16: 38 KB of halo + 18 KB of weight ring instead of
        // 77 + 36 KB -> TWO workgroups per CU = two waves per SIMD, so that one tile's halo load, chunk barriers, fp64 flushes and epilogue run under the other
        // tile's MFMAs (with one workgroup per CU all of that was exposed: 59 % of the fp32 MFMA peak).  LT_HALO_F3=1: the one-phase kernel
        {
            const char* f3 = getenv("LT_HALO_F3");
            if (ks == 3 && cin == 32 && cout_pad == 32 && !(f3 && f3[0] == '1')) {
                int rc = launch_halo<float, 3, 16, 32, 3, 3, 1, false, 2>(a, s);
                return rc == LT_OK ? 1 : rc;
            }
        }
        HALO_CASE(float, 3, 32, 32, 3, 3, 1, false)
        HALO_CASE(float, 3, 16, 32, 9, 2, 1, false)
        // round 6: the 7^3 layers of the exact-fp32 kernel set.  32 -> 16 (V2V's front layer, 18 % of the fp32 forward on the generic 256 x 16 tile at 51 % of
        // the fp32 MFMA peak): two channel phases of 16 over a 123 KB halo image (NPH = 2, see the kernel).  16 -> 32 (its input gradient in the fp32
        // training step): one phase, one-tap lookahead, two weight buffers (151 KB).  LT_HALO_NO_F7=1: the generic tiles again (A/B).
        if (ks == 7 && !env_on("LT_HALO_NO_F7")) {
            if (cin == 32 && cout_pad == 16) {
                int rc = launch_halo<float, 7, 16, 16, 7, 4, 2, false, 2>(a, s);
                return rc == LT_OK ? 1 : rc;
            }
            HALO_CASE(float, 7, 16, 32, 7, 2, 1, false)
        }
    }
#undef HALO_CASE
    return 0;
}

}  // namespace lt
