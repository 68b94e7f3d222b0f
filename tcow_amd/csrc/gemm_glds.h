// What the bf16 GEMM kernels of both families (NT: gemm_bf16.hip, gemm_nt_c2.hip; TN: gemm_tn_bf16.hip) share: the XCD-aware workgroup order and
// the two direct-to-LDS loads (flat, and bounds-checked through a buffer descriptor).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    // Blocks are dispatched round-robin over the 8 XCDs; give each XCD a contiguous chunk of tile ids.
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, k = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((GLB_PTR(const uint32_t))gsrc, (LDS_PTR(uint32_t))lds_wave_base, 16, 0, 0);
}

// raw buffer descriptor over `bytes` bytes at `base`: a load whose offset passes `bytes` returns zeros and makes no memory request
typedef int i32x4_ __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4_ make_srd(const void* base, long bytes) {
    const uint64_t b = (uint64_t)(uintptr_t)base;
    i32x4_ r; r[0] = (int)(uint32_t)b; r[1] = (int)(uint32_t)((b >> 32) & 0xffffu); r[2] = (int)(uint32_t)bytes; r[3] = 0x00020000;
    return r;
}
// 16 bytes per lane from descriptor `srd` at per-lane byte offset `voff` + scalar byte offset `soff` to the wave's LDS destination `ldsdst`.
// One load = one statement: M0 (LDS destination, wave-uniform) is written in the statement that reads it.  hipcc does not count these loads
// (inline asm): every wait for them is an explicit vmcnt.
#define TCOW_BUFFER_GLDS16(voff, srd, soff, ldsdst) \
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" :: "v"(voff), "s"(srd), "s"(soff), "s"(ldsdst) : "memory")

}  // namespace
