// Skinny-M NT GEMM of the streaming steps in the bf16 x 3 arithmetic (gfx950): C[M,N] = epi(A[M,K] . W[N,K]^T), f32 operands in HBM, for a few
// hundred rows, where the 128 x 128 kernel of gemm_x3.hip starts 18 ... 72 workgroups on 256 CUs and the launch takes one workgroup's serial walk
// over K.  The f32 counterpart of gemm_nt_skinny.hip:
//
//   gemm_nt_skinny_x3_kernel         64 x 64 output tile, 4 waves as 2 x 2 with one 32 x 32 accumulator each, K in 64-element slices through a ring
//                                    of two LDS stages (32 KiB each: 64 rows x 256 B per operand) filled by direct-to-LDS f32 loads.  A lane reads its 8
//                                    consecutive k values as two 16-byte reads and splits them in registers (split2, gemm_f32.h).  The work items, the
//                                    split over K, its slabs and the reduce launch are those of gemm_nt_skinny.h; the epilogue of S == 1 and of the
//                                    reduce is f32_epilogue_store4.
//
// The arithmetic of an output element is that of gemm_x3_body: the same split, per 16-wide k chunk the three MFMAs b_hi a_lo, b_lo a_hi, b_hi a_hi
// in that order (B fragment first: the accumulators hold C^T), the same k elements per lane half (k = 16 ks + 8 hi + e), K ascending from a zero
// accumulator.  S == 1 therefore gives the 128 tile's bits.
#include "gemm_f32.h"
#include "gemm_nt_skinny.h"

namespace {

constexpr int SX_ROW = SK_BK * 4;             // 256 B: an f32 row of a stage is one LDS bank row
constexpr int SX_TILE = SK_BM * SX_ROW;       // 16 KiB per operand per stage
constexpr int SX_STAGE = 2 * SX_TILE;         // 32 KiB
constexpr int SX_NS = 2;                      // ring stages: 64 KiB, two workgroups per CU (a four-stage ring measured no better)

struct SkinnyX3Params {
    F32Params p;          // (p.slab / p.kps unused: the split is sk's)
    SkinnySplit sk;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive f32 (two 16-byte LDS reads) -> the hi and the lo fragment of one lane
__device__ __forceinline__ void split8(u32x4 v0, u32x4 v1, x3_bf16x8& h, x3_bf16x8& l) {
    const f32x4 f0 = __builtin_bit_cast(f32x4, v0), f1 = __builtin_bit_cast(f32x4, v1);
    uint32_t hh[4], ll[4];
    split2(f0[0], f0[1], hh[0], ll[0]);
    split2(f0[2], f0[3], hh[1], ll[1]);
    split2(f1[0], f1[1], hh[2], ll[2]);
    split2(f1[2], f1[3], hh[3], ll[3]);
    h = __builtin_bit_cast(x3_bf16x8, (u32x4){hh[0], hh[1], hh[2], hh[3]});
    l = __builtin_bit_cast(x3_bf16x8, (u32x4){ll[0], ll[1], ll[2], ll[3]});
}

// Ring of SX_NS = 2 stages, as in gemm_nt_skinny_kernel: slice i lives in stage i % 2; one slice is in flight in front of the one being multiplied.
// Per iteration: s_waitcnt vmcnt(0) retires this wave's 8 loads of slice kt (the only ones outstanding at that point: the count is exact), a raw
// s_barrier makes every wave's part of it visible and says that stage (kt - 1) % 2 has been read by all, which the loads of slice kt + 1 then
// refill.  The fragment reads are inline asm: hipcc does not count them against the direct-to-LDS loads.
// LDS image of an operand: row r at r * 256 B, its 16-byte chunk c (4 consecutive k) at position c ^ (r & 15).  A direct-to-LDS load writes lane l
// at base + 16 l, so the XOR is on the SOURCE address; the 16 lanes of a ds_read_b128 group hold rows that differ mod 16 (MFMA row = lane & 31) and
// read the same chunk: 16 different 16-byte slots of the bank row.
__global__ __launch_bounds__(256) void gemm_nt_skinny_x3_kernel(SkinnyX3Params sp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const F32Params& p = sp.p;
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

    // wave w issues wave-loads 4w .. 4w+3 per operand, each 4 tile rows x 256 B; lane -> (row 4 q + (lane >> 4), LDS chunk position lane & 15).
    // Rows >= M and weight rows >= N read the last valid row (never stored).
    const float* a_src[4];
    const float* w_src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (wave * 4 + j) * 4 + (lane >> 4);
        const int c = (lane & 15) ^ (r & 15);
        int gm = m0 + r; gm = gm < p.M ? gm : p.M - 1;
        int gw = n0 + r; gw = gw < p.N ? gw : p.N - 1;
        a_src[j] = p.A + (size_t)gm * p.sai + (size_t)k0 * SK_BK + c * 4;
        w_src[j] = p.B + (size_t)gw * p.sbj + (size_t)k0 * SK_BK + c * 4;
    }
    auto issue = [&](int i) {
        char* sa = smem + (i % SX_NS) * SX_STAGE;
        char* sw = sa + SX_TILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(a_src[j] + (size_t)i * SK_BK, sa + (wave * 4 + j) * 1024);
            glds16(w_src[j] + (size_t)i * SK_BK, sw + (wave * 4 + j) * 1024);
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // fragment of the 16-wide k chunk ks: k = 16 ks + 8 hi + e, e = 0 .. 7 -> the 16-byte chunks 4 ks + 2 hi and 4 ks + 2 hi + 1 of the lane's row
    const uint32_t lds0 = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    uint32_t a_ad[8], w_ad[8];
    {
        const int ra = wm * 32 + l31, rw = wn * 32 + l31;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = 4 * (q >> 1) + 2 * hi + (q & 1);
            a_ad[q] = lds0 + ra * SX_ROW + ((c ^ (ra & 15)) << 4);
            w_ad[q] = lds0 + SX_TILE + rw * SX_ROW + ((c ^ (rw & 15)) << 4);
        }
    }

    issue(0);
    for (int kt = 0; kt < n; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 1 < n) issue(kt + 1);
        const uint32_t so = (uint32_t)(kt % SX_NS) * SX_STAGE;
        u32x4 fa[8], fw[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            asm volatile("ds_read_b128 %0, %1" : "=v"(fa[q]) : "v"(a_ad[q] + so) : "memory");
            asm volatile("ds_read_b128 %0, %1" : "=v"(fw[q]) : "v"(w_ad[q] + so) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            x3_bf16x8 ah, al, bh, bl;
            split8(fa[2 * ks], fa[2 * ks + 1], ah, al);
            split8(fw[2 * ks], fw[2 * ks + 1], bh, bl);
            // (B fragment first: the accumulator holds C^T -- lane = output row, register quads = 4 consecutive columns)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, al, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, ah, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, ah, acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // (the last iteration waited vmcnt(0): nothing is in flight)  every wave has read its fragments before the f32 tile overwrites the stages
    __syncthreads();
    // register 4 g + e of lane (l31, hi): output row l31 of the wave's band, columns 8 g + 4 hi + e
    float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(ct + (wm * 32 + l31) * SK_CT_LD + wn * 32 + 8 * g + 4 * hi) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
    __syncthreads();
    if (!col_ok) return;
    float* dst = S == 1 ? nullptr : sp.sk.slab + (size_t)s * p.M * p.N;
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const int row = (tid >> 4) + it * 16, gm = m0 + row;
        if (gm >= p.M) break;
        const float4 x = *reinterpret_cast<const float4*>(ct + row * SK_CT_LD + c4);
        if (dst) st4(dst + (size_t)gm * p.N + gn, x);
        else f32_epilogue_store4(p, gm, gn, x, b4);
    }
}

// The reduce kernel's epilogue.  The residual may alias the output: f32_epilogue_store4 reads the thread's residual element before it stores it.
struct SkinnyX3Epi {
    __device__ SkinnyX3Epi(const F32Params&, int, int) {}
    __device__ void operator()(const F32Params& p, float4 v, float4 b4, int gm, int gn) const { f32_epilogue_store4(p, gm, gn, v, b4); }
};

}  // namespace

// (validated by tcow_gemm_nt_skinny_x3, api.cpp)  The ring's 64 KiB hold the 17 KiB epilogue tile.
int tcow_gemm_nt_skinny_launch_x3(hipStream_t stream, const tcow_gemm_args* a, int split, float* slab) {
    SkinnyX3Params sp;
    sp.p = f32_params_nt(a, SK_BK);
    sp.sk = skinny_split(a, split, slab);
    return skinny_launch("tcow_gemm_nt_skinny_x3", stream, sp, gemm_nt_skinny_x3_kernel, SX_NS * SX_STAGE, gemm_nt_skinny_reduce_kernel<SkinnyX3Params, SkinnyX3Epi>);
}
