// Skinny-M NT GEMM of the streaming steps (gfx950): C[M,N] = epi(A[M,K] . W[N,K]^T) for a few hundred rows, where the 128 x 128 kernel of
// gemm_bf16.hip starts 18 ... 72 workgroups on 256 CUs and the launch takes one workgroup's serial walk over K.
//
//   gemm_nt_skinny_kernel         64 x 64 output tile, 4 waves as 2 x 2 with one 32 x 32 accumulator each, K in 64-element slices through a ring of
//                                 LDS stages (16 KiB each) filled by direct-to-LDS loads.  A workgroup is (tile, slice s of S): it walks the k-slices
//                                 [s nk / S, (s + 1) nk / S).  S == 1: the shared epilogue (epi_rows<EpiAny>).  S > 1: the raw f32 partial goes to slab
//                                 s of the workspace [S, M, N].
//   gemm_nt_skinny_reduce_kernel  S > 1 only, a second launch: v = slab[0]; v += slab[1]; ... in slice order, then epi_row_apply<EpiAny>.
//
// The arithmetic of an output element is that of gemm_nt_bf16_kernel: the same MFMA, the same k elements per lane half (chunk c = 2 ks + hi), K ascending.
// S == 1 therefore gives the 128 tile's bits; S > 1 is a fixed function of the inputs (no atomics, no arrival order).
// The kernel boundary makes the slabs visible: workgroups do not communicate inside a launch.
#include "common.h"
#include "internal.h"
#include "gemm_nt_common.h"

namespace {

constexpr int SK_BM = 64, SK_BN = 64, SK_BK = 64;
constexpr int SK_TILE = SK_BM * 128;          // 8 KiB per operand per stage
constexpr int SK_STAGE = 2 * SK_TILE;         // 16 KiB
constexpr int SK_CT_LD = 68;                  // f32 epilogue tile: 64 rows x 68 floats = 17 KiB (rows 4 apart land 16 banks apart)

struct SkinnyParams {
    NtParams nt;
    int split;            // S
    float* slab;          // [S, M, N] f32 (S > 1)
};

// Ring of NS stages.  Slice i lives in stage i % NS; NS - 1 slices are in flight in front of the one being multiplied.  Per iteration: a counted
// vmcnt retires this wave's loads of slice kt (4 per slice and wave, in issue order), a raw s_barrier makes every wave's part of it visible and says
// that stage (kt - 1) % NS has been read by all, which the loads of slice kt + NS - 1 then refill.  The fragment reads are inline asm: hipcc does not
// count them against the direct-to-LDS loads (it would drain the ring with vmcnt(0) before every ds_read of its own).
template <int NS>
__global__ __launch_bounds__(256) void gemm_nt_skinny_kernel(SkinnyParams sp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const NtParams& p = sp.nt;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;

    const int S = sp.split;
    const int nblk = p.tiles_m * p.tiles_n * S;
    const int pid = xcd_remap(blockIdx.x, nblk);
    const int tile = pid / S, s = pid - tile * S;
    const int pm = tile / p.tiles_n, pn = tile - pm * p.tiles_n;
    const int m0 = pm * SK_BM, n0 = pn * SK_BN;
    const int nk = p.K / SK_BK;
    const int k0 = (int)((long)s * nk / S), k1 = (int)((long)(s + 1) * nk / S);
    const int n = k1 - k0;                         // >= 1: S <= nk

    const int c4 = (tid & 15) * 4, gn = n0 + c4;   // epilogue: 16 threads x 4 columns per row, 16 rows per pass
    const bool col_ok = gn < p.N;                  // N % 4 == 0
    const float4 b4 = (S == 1 && p.bias && col_ok) ? ld4(p.bias + gn) : make_float4(0.f, 0.f, 0.f, 0.f);

    // wave w issues wave-loads 2w, 2w+1 per operand, each 8 tile rows x 128 B; lane -> (row 8 q + (lane >> 3), LDS chunk position lane & 7)
    const bf16_t* a_src[2];
    const bf16_t* w_src[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (wave * 2 + j) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        int gm = m0 + r; gm = gm < p.M ? gm : p.M - 1;
        int gw = n0 + r; gw = gw < p.N ? gw : p.N - 1;
        a_src[j] = p.A + (size_t)gm * p.lda + (size_t)k0 * SK_BK + c * 8;
        w_src[j] = p.W + (size_t)gw * p.ldw + (size_t)k0 * SK_BK + c * 8;
    }
    auto issue = [&](int i) {
        char* sa = smem + (i % NS) * SK_STAGE;
        char* sw = sa + SK_TILE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            glds16(a_src[j] + (size_t)i * SK_BK, sa + (wave * 2 + j) * 1024);
            glds16(w_src[j] + (size_t)i * SK_BK, sw + (wave * 2 + j) * 1024);
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t lds0 = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    uint32_t a_ad[4], w_ad[4];
    {
        const int ra = wm * 32 + l31, rw = wn * 32 + l31;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            a_ad[ks] = lds0 + ra * 128 + (((2 * ks + hi) ^ ((ra >> 1) & 7)) << 4);
            w_ad[ks] = lds0 + SK_TILE + rw * 128 + (((2 * ks + hi) ^ ((rw >> 1) & 7)) << 4);
        }
    }

#pragma unroll
    for (int i = 0; i < NS - 1; ++i)
        if (i < n) issue(i);
    for (int kt = 0; kt < n; ++kt) {
        // slices kt + 1 .. min(n - 1, kt + NS - 2) may stay in flight: 4 loads each
        const int ahead = n - 1 - kt;
        if (NS >= 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (NS >= 3 && ahead >= 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + NS - 1 < n) issue(kt + NS - 1);
        const uint32_t so = (uint32_t)(kt % NS) * SK_STAGE;
        u32x4 fa[4], fw[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            asm volatile("ds_read_b128 %0, %1" : "=v"(fa[ks]) : "v"(a_ad[ks] + so) : "memory");
            asm volatile("ds_read_b128 %0, %1" : "=v"(fw[ks]) : "v"(w_ad[ks] + so) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            acc = TCOW_MFMA_32x32x16_H16(__builtin_bit_cast(bf16x8, fa[ks]), __builtin_bit_cast(bf16x8, fw[ks]), acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    // (the last iteration waited vmcnt(0): nothing is in flight)  every wave has read its fragments before the f32 tile overwrites the stages
    __syncthreads();
    float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int r = 0; r < 16; ++r) ct[(wm * 32 + crow32(r, hi)) * SK_CT_LD + wn * 32 + l31] = acc[r];
    __syncthreads();
    if (!col_ok) return;
    if (S == 1) {
        epi_rows<4>(p, ct, SK_CT_LD, b4, m0 + (tid >> 4), tid >> 4, 16, c4, gn);
    } else {
        float* dst = sp.slab + (size_t)s * p.M * p.N;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = (tid >> 4) + it * 16, gm = m0 + row;
            if (gm < p.M) st4(dst + (size_t)gm * p.N + gn, *reinterpret_cast<const float4*>(ct + row * SK_CT_LD + c4));
        }
    }
}

// One thread per (row, 4 columns).  The residual may alias the f32 output: a thread reads its residual element (epi_row_fetch) before it stores it.
__global__ __launch_bounds__(256) void gemm_nt_skinny_reduce_kernel(SkinnyParams sp) {
    const NtParams& p = sp.nt;
    const int n4 = p.N >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.M * n4) return;
    const int gm = (int)(idx / n4), gn = (int)(idx - (long)gm * n4) * 4;
    const size_t slab_stride = (size_t)p.M * p.N;
    const float* src = sp.slab + (size_t)gm * p.N + gn;
    const EpiRow o = epi_row_fetch<EpiAny>(p, gm, gn, true);
    const float4 b4 = p.bias ? ld4(p.bias + gn) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = ld4(src);
    for (int s = 1; s < sp.split; ++s) {
        const float4 t = ld4(src + (size_t)s * slab_stride);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    epi_row_apply<EpiAny>(p, o, v, b4, gm, gn);
}

}  // namespace

// (validated by tcow_gemm_nt_skinny, api.cpp)
int tcow_gemm_nt_skinny_bf16(hipStream_t stream, const tcow_gemm_args* a, int split, float* slab) {
    SkinnyParams sp;
    sp.nt = nt_params_from_args(a);
    sp.nt.tiles_m = cdiv(a->M, SK_BM); sp.nt.tiles_n = cdiv(a->N, SK_BN);
    sp.split = split; sp.slab = slab;
    const long blocks = (long)sp.nt.tiles_m * sp.nt.tiles_n * split;
    TCOW_CHECK_ARG(blocks < (1L << 31), "tcow_gemm_nt_skinny: M=%d N=%d split=%d give too many workgroups", a->M, a->N, split);
    // Ring depth (profiles/gemm_skinny.json; the depth does not change the arithmetic).  Up to two workgroups per CU: four stages, the loads of three
    // k-slices in flight per workgroup -- 8.9 -> 6.8 us (qkv), 9.3 -> 7.1 (proj), 9.7 -> 7.8 (fc1) at M = 301 against two stages.  More workgroups
    // than that: two stages (32 KiB, five workgroups per CU), the co-resident workgroups hide the latency and a deep ring only takes their LDS --
    // fc1 at M = 1 201 (912 workgroups) 15.1 us on two stages, 17.1 on three, 18.8 on four.
    typedef void (*Kern)(SkinnyParams);
    const int ns = blocks > 512 ? 2 : 4;
    const Kern k = ns == 2 ? gemm_nt_skinny_kernel<2> : gemm_nt_skinny_kernel<4>;
    const int lds = ns * SK_STAGE;                 // >= 32 KiB: holds the 17 KiB epilogue tile
    tcow_ensure_lds(reinterpret_cast<const void*>(k), lds);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), lds, stream, sp);
    TCOW_CHECK_LAUNCH();
    if (split > 1) {
        const long threads = (long)a->M * (a->N / 4);
        hipLaunchKernelGGL(gemm_nt_skinny_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, sp);
        TCOW_CHECK_LAUNCH();
    }
    return TCOW_OK;
}
