// Wave-level inline-asm primitives of the hand-scheduled MFMA kernels (conv_igemm2/3/7, conv3d_halo, conv2d_halo, xr, bneck): the LDS-DMA, counted
// vmcnt / lgkmcnt waits, hand-issued fragment reads, SGPR-based global loads.  One definition each: a kernel file takes them from here and adds none.
#pragma once
#include <type_traits>

#include "conv_common.h"

namespace lt {

typedef __attribute__((address_space(3))) void* lptr_t;   // (unsigned)(size_t)(lptr_t)smem = LDS byte address of the dynamic region

#ifdef LT_TRACE
// -DLT_TRACE (profiling build, lt_build.build_variant): shader-clock accounting of a kernel's phases; every kernel file has its own trace buffer
#define LT_CLK() ((long long)__builtin_amdgcn_s_memtime())
#endif

// one LDS-DMA wave-instruction: 64 lanes x 16 B -> lds_base .. lds_base + 1 KiB (wave-uniform base).  The base travels in m0, which is saved and
// restored around the load (the compiler does not know that the asm writes it).
__device__ __forceinline__ void dma16(const void* src, unsigned lds_base) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(lds_base)
        : "memory");
}
// the same with a base that is wave-uniform by construction but not provably so (it depends on a loop index or a wave id the compiler keeps in a
// VGPR): readfirstlane makes it provable.  conv3d_halo and conv2d_halo use this form; in the other kernels the base already lives in SGPRs, and the
// extra intrinsic only perturbs their register allocation.
__device__ __forceinline__ void dma16_uniform(const void* src, unsigned lds_base) { dma16(src, __builtin_amdgcn_readfirstlane(lds_base)); }

// s_waitcnt vmcnt(N), N known at compile time: cannot fall through
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// s_waitcnt vmcnt(n) for a wave-uniform run-time n (the immediate must be a literal).  The cases are the union of the counts the kernels ask for;
// any other count waits for everything: correct, but slower.
__device__ __forceinline__ void wait_vmcnt(int n) {
    switch (n) {
        case 0: wait_vmcnt<0>(); break;
        case 1: wait_vmcnt<1>(); break;
        case 2: wait_vmcnt<2>(); break;
        case 3: wait_vmcnt<3>(); break;
        case 4: wait_vmcnt<4>(); break;
        case 5: wait_vmcnt<5>(); break;
        case 6: wait_vmcnt<6>(); break;
        case 7: wait_vmcnt<7>(); break;
        case 8: wait_vmcnt<8>(); break;
        case 9: wait_vmcnt<9>(); break;
        case 10: wait_vmcnt<10>(); break;
        case 11: wait_vmcnt<11>(); break;
        case 12: wait_vmcnt<12>(); break;
        case 14: wait_vmcnt<14>(); break;
        case 15: wait_vmcnt<15>(); break;
        case 18: wait_vmcnt<18>(); break;
        default: wait_vmcnt<0>(); break;   // conservative
    }
}

// ---- hand-scheduled LDS fragment reads -------------------------------------------------------------------------------------
// hipcc's own s_waitcnt insertion degrades to lgkmcnt(0) as soon as more than one group of fragment reads is in flight (seen
// in the ISA: every third tap drained the whole queue).  The deep-lookahead paths therefore issue ds_read_b128 themselves
// and wait with an explicit count; frag_ready() ties the wait to the registers so that no MFMA can be scheduled above it.
template <int IMM>
__device__ __forceinline__ void lds_read16(V16& d, unsigned addr) {
    static_assert(IMM >= 0 && IMM < 65536, "ds_read offset field");
    f32x4 t;   // a native vector (HIP's uint4 is a struct, which inline asm can only take indirectly)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(t) : "v"(addr), "n"(IMM));
    d.f = t;
}
template <int N>
__device__ __forceinline__ void lgkm_wait() {
    static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N));
}
__device__ __forceinline__ void frag_ready(V16& f) {
    f32x4 t = f.f;
    asm volatile("" : "+v"(t));
    f.f = t;
}

// f(integral_constant<int, I>) for I = I0 .. I1 - 1: a loop whose index is a compile-time constant in the body (asm immediates, register arrays)
template <int I0, int I1, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I0>{});
        static_for<I0 + 1, I1>(f);
    }
}

// 16-byte global load: wave-uniform base in SGPRs + 32-bit lane offset + immediate, no 64-bit address arithmetic in VGPRs
template <int IMM = 0>
__device__ __forceinline__ void gload16(V16& d, const void* sbase, unsigned voff) {
    static_assert(IMM >= 0 && IMM < 4096, "global_load immediate offset");
    f32x4 t;
    const unsigned long long b = (unsigned long long)(size_t)sbase;
    const unsigned long long ub = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((int)b);   // uniform by construction; make it provable
    // s_nop: the base may have just been written by v_readfirstlane, and a VALU write of an SGPR needs 5 wait states before a
    // vector-memory instruction reads it -- the hazard recognizer does not look inside inline asm (seen: the load took the
    // stale low dword and faulted)
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(t) : "v"(voff), "s"(ub), "n"(IMM) : "memory");
    d.f = t;
}

// 64-byte LDS rows: a 16-byte slot holds K vector (slot ^ swz64(row)), swz64 = [0,2,3,1][(row >> 2) & 3] -- with that the four 16-lane groups of
// a ds_read_b128 fragment read (rows r, K vector lane >> 4) each touch all 64 banks once (checked by enumeration, comment in DESIGN.md); the DMA
// writes lane-linearly, so the swizzle is applied to the source address.
__device__ __forceinline__ int swz64(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }

}  // namespace lt
