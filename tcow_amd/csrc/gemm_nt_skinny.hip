// Skinny-M NT GEMM of the streaming steps (gfx950): C[M,N] = epi(A[M,K] . W[N,K]^T) for a few hundred rows, where the 128 x 128 kernel of
// gemm_bf16.hip starts 18 ... 72 workgroups on 256 CUs and the launch takes one workgroup's serial walk over K.
//
//   gemm_nt_skinny_kernel         64 x 64 output tile, 4 waves as 2 x 2 with one 32 x 32 accumulator each, K in 64-element slices through a ring of
//                                 LDS stages (16 KiB each) filled by direct-to-LDS loads.  The work items, the split over K, its slabs and the
//                                 reduce launch are those of gemm_nt_skinny.h.  S == 1: the shared epilogue (epi_rows<EpiAny>); the reduce of
//                                 S > 1: epi_row_apply<EpiAny>.
//
// The arithmetic of an output element is that of gemm_nt_bf16_kernel: the same MFMA, the same k elements per lane half (chunk c = 2 ks + hi), K ascending.
// S == 1 therefore gives the 128 tile's bits.
#include "gemm_nt_common.h"
#include "gemm_nt_skinny.h"

namespace {

constexpr int SK_TILE = SK_BM * 128;          // 8 KiB per operand per stage
constexpr int SK_STAGE = 2 * SK_TILE;         // 16 KiB

struct SkinnyParams {
    NtParams p;           // (p.tiles_m / p.tiles_n / p.band unused: the work items are sk's)
    SkinnySplit sk;
};

// Ring of NS stages.  Slice i lives in stage i % NS; NS - 1 slices are in flight in front of the one being multiplied.  Per iteration: a counted
// vmcnt retires this wave's loads of slice kt (4 per slice and wave, in issue order), a raw s_barrier makes every wave's part of it visible and says
// that stage (kt - 1) % NS has been read by all, which the loads of slice kt + NS - 1 then refill.  The fragment reads are inline asm: hipcc does not
// count them against the direct-to-LDS loads (it would drain the ring with vmcnt(0) before every ds_read of its own).
template <int NS>
__global__ __launch_bounds__(256) void gemm_nt_skinny_kernel(SkinnyParams sp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const NtParams& p = sp.p;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;

    const int S = sp.sk.split;
    const SkinnyItem w = skinny_item(sp.sk, p.K);
    const int m0 = w.m0, n0 = w.n0, s = w.s, k0 = w.k0, n = w.n;

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
        float* dst = sp.sk.slab + (size_t)s * p.M * p.N;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = (tid >> 4) + it * 16, gm = m0 + row;
            if (gm < p.M) st4(dst + (size_t)gm * p.N + gn, *reinterpret_cast<const float4*>(ct + row * SK_CT_LD + c4));
        }
    }
}

// The reduce kernel's epilogue.  The residual may alias the f32 output: a thread reads its residual element (epi_row_fetch) before it stores it.
struct SkinnyEpi {
    EpiRow o;
    __device__ SkinnyEpi(const NtParams& p, int gm, int gn) : o(epi_row_fetch<EpiAny>(p, gm, gn, true)) {}
    __device__ void operator()(const NtParams& p, float4 v, float4 b4, int gm, int gn) const { epi_row_apply<EpiAny>(p, o, v, b4, gm, gn); }
};

}  // namespace

// (validated by tcow_gemm_nt_skinny, api.cpp)
int tcow_gemm_nt_skinny_launch_bf16(hipStream_t stream, const tcow_gemm_args* a, int split, float* slab) {
    SkinnyParams sp;
    sp.p = nt_params_from_args(a);
    sp.sk = skinny_split(a, split, slab);
    // Ring depth (profiles/gemm_skinny.json; the depth does not change the arithmetic).  Up to two workgroups per CU: four stages, the loads of three
    // k-slices in flight per workgroup -- 8.9 -> 6.8 us (qkv), 9.3 -> 7.1 (proj), 9.7 -> 7.8 (fc1) at M = 301 against two stages.  More workgroups
    // than that: two stages (32 KiB, five workgroups per CU), the co-resident workgroups hide the latency and a deep ring only takes their LDS --
    // fc1 at M = 1 201 (912 workgroups) 15.1 us on two stages, 17.1 on three, 18.8 on four.
    const int ns = skinny_blocks(sp.sk) > 512 ? 2 : 4;      // (ns * SK_STAGE >= 32 KiB: holds the 17 KiB epilogue tile)
    return skinny_launch("tcow_gemm_nt_skinny", stream, sp, ns == 2 ? gemm_nt_skinny_kernel<2> : gemm_nt_skinny_kernel<4>, ns * SK_STAGE,
                         gemm_nt_skinny_reduce_kernel<SkinnyParams, SkinnyEpi>);
}
