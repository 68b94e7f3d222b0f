// The split-K frame of the skinny-M NT GEMMs (gemm_nt_skinny.hip: the 16-bit modes; gemm_nt_skinny_x3.hip: bf16 x 3 on f32 operands): what the
// two have in common, written once.  Each source keeps its own main loop, LDS image and arithmetic.
//
// Output tiles are 64 x 64 and K is walked in 64-element slices, nk = K / 64 of them.  A workgroup is (tile, slice s of S), 1 <= S <= min(16, nk):
// it walks the k-slices [s nk / S, (s + 1) nk / S).  S == 1: the main kernel applies the epilogue itself.  S > 1: the raw f32 partial goes to slab
// s of the workspace [S, M, N] (S M N 4 bytes, 16-byte aligned) and a second launch, gemm_nt_skinny_reduce_kernel, adds the slabs in slice order
// -- v = slab[0]; v += slab[1]; ... -- and applies the epilogue.  S > 1 is therefore a fixed function of the inputs (no atomics, no arrival
// order).  The kernel boundary makes the slabs visible: workgroups do not communicate inside a launch.
#pragma once
#include "common.h"
#include "internal.h"
#include "gemm_glds.h"

namespace {

constexpr int SK_BM = 64, SK_BN = 64, SK_BK = 64;
constexpr int SK_CT_LD = 68;                  // f32 epilogue tile: 64 rows x 68 floats = 17 KiB (rows 4 apart land 16 banks apart)

struct SkinnySplit {
    int tiles_m, tiles_n;
    int split;            // S
    float* slab;          // [S, M, N] f32 (S > 1)
};

static inline SkinnySplit skinny_split(const tcow_gemm_args* a, int split, float* slab) {
    return SkinnySplit{cdiv(a->M, SK_BM), cdiv(a->N, SK_BN), split, slab};
}
static inline long skinny_blocks(const SkinnySplit& sk) { return (long)sk.tiles_m * sk.tiles_n * sk.split; }

// The work item of this workgroup: output tile at (m0, n0), slice s, its n >= 1 k-slices from k0 on (S <= nk).
struct SkinnyItem { int m0, n0, s, k0, n; };
__device__ __forceinline__ SkinnyItem skinny_item(const SkinnySplit& sk, int K) {
    const int S = sk.split;
    const int nblk = sk.tiles_m * sk.tiles_n * S;
    const int pid = xcd_remap(blockIdx.x, nblk);
    const int tile = pid / S, s = pid - tile * S;
    const int pm = tile / sk.tiles_n, pn = tile - pm * sk.tiles_n;
    const int nk = K / SK_BK;
    const int k0 = (int)((long)s * nk / S), k1 = (int)((long)(s + 1) * nk / S);
    return SkinnyItem{pm * SK_BM, pn * SK_BN, s, k0, k1 - k0};
}

// S > 1 only.  One thread per (row, 4 columns).  P = {p: the main kernel's parameters, sk}; Epi(p, gm, gn) fetches what the epilogue reads of the
// output's own row before the slabs are read (the residual may alias the output), Epi::operator() applies the epilogue and stores.
template <class P, class Epi>
__global__ __launch_bounds__(256) void gemm_nt_skinny_reduce_kernel(P sp) {
    const auto& p = sp.p;
    const int n4 = p.N >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.M * n4) return;
    const int gm = (int)(idx / n4), gn = (int)(idx - (long)gm * n4) * 4;
    const size_t slab_stride = (size_t)p.M * p.N;
    const float* src = sp.sk.slab + (size_t)gm * p.N + gn;
    const Epi epi(p, gm, gn);
    const float4 b4 = p.bias ? ld4(p.bias + gn) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = ld4(src);
    for (int s = 1; s < sp.sk.split; ++s) {
        const float4 t = ld4(src + (size_t)s * slab_stride);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    epi(p, v, b4, gm, gn);
}

// The launches of a validated call (api.cpp): `main` with `lds` bytes on one workgroup per work item, then the reduce if the product is split.
template <class P>
int skinny_launch(const char* who, hipStream_t stream, const P& sp, void (*main)(P), int lds, void (*reduce)(P)) {
    const long blocks = skinny_blocks(sp.sk);
    TCOW_CHECK_ARG(blocks < (1L << 31), "%s: M=%d N=%d split=%d give too many workgroups", who, sp.p.M, sp.p.N, sp.sk.split);
    tcow_ensure_lds(reinterpret_cast<const void*>(main), lds);
    hipLaunchKernelGGL(main, dim3((unsigned)blocks), dim3(256), lds, stream, sp);
    TCOW_CHECK_LAUNCH();
    if (sp.sk.split > 1) {
        const long threads = (long)sp.p.M * (sp.p.N / 4);
        hipLaunchKernelGGL(reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, sp);
        TCOW_CHECK_LAUNCH();
    }
    return TCOW_OK;
}

}  // namespace
