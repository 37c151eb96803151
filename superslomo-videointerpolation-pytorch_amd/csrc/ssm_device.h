// Device-side primitives shared by the kernels of libssm_hip.so (gfx950 only): vector types, the XCD tile order, the LDS-DMA and
// scalar-base store statements (defined here only, each next to the hazard rules it must obey; check_hazard.py fences them on the
// disassembly), vmcnt waits, register pins and the fp8 pack.  Included by the .hip files; the host helpers are in ssm_common.h.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// XCD-aware tile order.  The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own
// L2), so in launch order neighbouring tiles - which share input halos, and for Cout > BN the whole input patch - sit
// on different L2s.  This maps workgroup i to the logical tile index such that every XCD walks one contiguous
// 1/8 of the (cout block, x tile, y tile, batch) sequence.
__device__ __forceinline__ int ssm_xcd_tile(int i, int n) {
    const int xcd = i & 7, local = i >> 3;
    const int per = n >> 3, rem = n & 7;
    return xcd < rem ? xcd * (per + 1) + local : rem * (per + 1) + (xcd - rem) * per + local;
}

// LDS-DMA: every lane copies 16 bytes from sbase + voff_bytes (wave-uniform 64-bit base in SGPRs, 32-bit byte offset per lane) to
// lds_dst + 16 * lane (wave-uniform LDS byte address): 1 KiB per instruction, counted by vmcnt.  The instruction takes its LDS address
// from M0.  M0 is written INSIDE the statement: no asm constraint places an operand in M0, and between two statements the compiler is
// free to use M0 for its own instructions.  s_nop 0 is the wait state between the scalar write of M0 and the DMA that reads it (the
// compiler's hazard recogniser does not look inside a statement).  "m0" in the clobber list tells the compiler its own M0 value is
// gone; clang warns that the register is reserved, which is why the Makefile passes -Wno-inline-asm to the files that issue LDS-DMA.
__device__ __forceinline__ void lds_dma16(const float *sbase, int voff_bytes, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff_bytes), "s"(sbase), "s"(lds_dst) : "memory", "m0");
}
// The per-lane form (64-bit address per lane, through the compiler's builtin, which handles M0 itself): lane l copies 16 bytes from
// gp to lp + 16 * l, lp wave-uniform.  For pieces whose lanes do not share one base.  A macro: as an inline function over void
// pointers it changed the code generated for the fp16 convolution kernels.
#define SSM_GLDS16(gp, lp)                                                                      \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gp),      \
                                     (__attribute__((address_space(3))) void *)(lp), 16, 0, 0)

// Stores with a scalar base: wave-uniform 64-bit base in SGPRs + 32-bit byte offset per lane - one address VGPR per store and no 64-bit
// vector add.  The statements are opaque to the compiler's hazard recogniser; check_hazard.py fences two rules on the disassembly:
//  * a base that the compiler forms with v_readfirstlane_b32 (a wave-uniform value that lived in a vector register) needs 5 wait
//    states before a vector-memory instruction reads it.  The statements carry none: form bases from values that are uniform by
//    construction (kernel arguments, blockIdx, wave ids taken through readfirstlane once at kernel entry), so they stay on the scalar unit;
//  * a store of more than 64 bits followed by a VALU write of its data registers needs 2 wait states.  Where the data registers are
//    rewritten right behind an x4 store (w4_epilogue_shuffle<true>), store_sbase_nop carries them (s_nop 1).
__device__ __forceinline__ void store_sbase(const float *sbase, unsigned off_bytes, float val) {
    asm volatile("global_store_dword %0, %1, %2" ::"v"(off_bytes), "v"(val), "s"(sbase) : "memory");
}
__device__ __forceinline__ void store_sbase(const float *sbase, unsigned off_bytes, f32x2 val) {
    asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"(off_bytes), "v"(val), "s"(sbase) : "memory");
}
__device__ __forceinline__ void store_sbase(const float *sbase, unsigned off_bytes, f32x4 val) {
    asm volatile("global_store_dwordx4 %0, %1, %2" ::"v"(off_bytes), "v"(val), "s"(sbase) : "memory");
}
__device__ __forceinline__ void store_sbase_nop(const float *sbase, unsigned off_bytes, f32x4 val) {
    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(off_bytes), "v"(val), "s"(sbase) : "memory");
}

// At most N vector-memory operations of this wave (LDS-DMA included) are still in flight.  A compiler barrier for memory as well.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Register pin: the value is in a VGPR here and the compiler knows nothing about it afterwards (no rematerialisation or hoisting
// across this point, an array stays scalars in registers).
template <class T>
__device__ __forceinline__ void pin(T &x) {
    asm volatile("" : "+v"(x));
}
template <class T, int N>
__device__ __forceinline__ void pin(T (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(a[i]));
}

// Four floats -> four e4m3fn bytes; clamped first: beyond +-448 the conversion gives NaN.
__device__ __forceinline__ int pack4_fp8(float a, float b, float c, float d) {
    const float lim = 448.0f;
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(a, -lim, lim), __builtin_amdgcn_fmed3f(b, -lim, lim), 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(c, -lim, lim), __builtin_amdgcn_fmed3f(d, -lim, lim), w, true);
}
