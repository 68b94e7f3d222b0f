// bf16 MFMA GEMMs for the Seeker hot path (gfx950).
//
//   gemm_nt_bf16 : C[M,N] = epi(A[M,K] . W[N,K]^T)  -- every nn.Linear forward and input-gradient on the path
//                  (vit.py:50-61,74-76,111,146; mask_tracker.py:113) with bias / DropPath row-scale / GELU /
//                  GELU' / residual fused in the epilogue.
//   (gemm_tn_bf16, the weight gradients dW[N,K] += dY[M,N]^T . X[M,K], is in gemm_tn_bf16.hip.)
//
// Structure of gemm_nt (per 256-thread workgroup = 4 waves as 2x2):
//   128x128 output tile, K walked in 64-element (128-byte) slices, two LDS stages filled with direct-to-LDS
//   loads (global_load_lds_dwordx4, no VGPR round trip).  Each 16-byte chunk c of tile row r is stored at chunk
//   position c ^ ((r>>1)&7) (applied on the per-lane SOURCE address, the LDS image of a wave-load stays
//   lane-linear), which makes the ds_read_b128 fragment reads of the 32x32x16 MFMA conflict-free.  Accumulators
//   are staged through LDS as f32 so that bias / residual loads and the C stores are full-row coalesced.
//   blockIdx is remapped so that each XCD (private L2) owns a contiguous band of row tiles.
#include <stdlib.h>

#include "common.h"
#include "internal.h"
#include "gemm_nt_common.h"

namespace {

constexpr int BM = 128, BN = 128;
constexpr int BK = 64;                    // bf16 elements per k-slice (128 bytes per tile row)
constexpr int TILE_BYTES = BM * 128;      // 16 KiB per operand per stage
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int NT_LDS_BYTES = 2 * STAGE_BYTES;  // 64 KiB (also holds the 128x128 f32 epilogue tile)

__device__ __forceinline__ void nt_epilogue(const NtParams& p, char* smem, f32x16 (&acc)[2][2], float4 b4, int tid, int wm, int wn, int l31, int hi, int m0, int n0) {
    const int c4 = (tid & 31) * 4, gn = n0 + c4;
    const bool col_ok = gn < p.N;                 // N % 4 == 0: a thread's 4 columns are all in or all out
    float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 64 + i * 32 + crow32(r, hi);
                const int col = wn * 64 + j * 32 + l31;
                ct[row * BN + col] = acc[i][j][r];
            }
    __syncthreads();
    if (!col_ok) return;
    epi_rows(p, ct, BN, b4, m0 + (tid >> 5), tid >> 5, 8, c4, gn);
}

// bias for this thread's 4 epilogue columns, fetched at kernel start (its latency hides behind the whole main loop)
__device__ __forceinline__ float4 epi_bias(const NtParams& p, int tid, int n0) {
    const int gn = n0 + (tid & 31) * 4;
    return (p.bias && gn < p.N) ? ld4(p.bias + gn) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- 256 x 256 tile, 8 waves (2 x 4, 128 x 64 each).  PMC on the 128-tile kernel (profiles/r01_pmc_gemm_units.txt): zero LDS bank
// conflicts, LdsUtil ~22 %, MFMA pipe busy 41-48 %, half of all wave cycles parked in the vmcnt/barrier wait and the texture-address
// path 58-68 % busy -- the 128 x 128 x 64 step pulls 32 KiB per workgroup per 2.1 MFLOP through the global->LDS path and is bound
// by it.  The 256-square tile halves the bytes per FLOP (64 KiB per 8.4 MFLOP; MFMA busy 55 % at 8192^3) and needs 6 instead of 8
// fragment reads per 8 MFMAs.  128 KiB LDS (two stages), one workgroup per CU.
constexpr int B_BM = 256, B_BN = 256;
constexpr int B_TILE = 256 * 128;              // 32 KiB per operand per stage
constexpr int B_STAGE = 2 * B_TILE;
constexpr int B_LDS = 2 * B_STAGE;             // 128 KiB

__global__ __launch_bounds__(512, 2) void gemm_nt_bf16_256_kernel(NtParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int l31 = lane & 31, hi = lane >> 5;
    const int nblk = p.tiles_m * p.tiles_n;
    const int pid = xcd_remap(blockIdx.x, nblk);
    const int pm = pid / p.tiles_n, pn = pid - pm * p.tiles_n;
    const int m0 = pm * B_BM, n0 = pn * B_BN;

    const bf16_t* a_src[4];
    const bf16_t* w_src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (wave * 4 + j) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        int gm = m0 + r; gm = gm < p.M ? gm : p.M - 1;
        int gn = n0 + r; gn = gn < p.N ? gn : p.N - 1;
        a_src[j] = p.A + (size_t)gm * p.lda + c * 8;
        w_src[j] = p.W + (size_t)gn * p.ldw + c * 8;
    }
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.K / BK;
    auto issue = [&](int kt, int stage) {
        char* sa = smem + stage * B_STAGE;
        char* sw = sa + B_TILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(a_src[j] + (size_t)kt * BK, sa + (wave * 4 + j) * 1024);
            glds16(w_src[j] + (size_t)kt * BK, sw + (wave * 4 + j) * 1024);
        }
    };
    // Fragment reads are software-pipelined by hand: left to hipcc, the loop keeps ONE fragment register set and waits lgkmcnt(0)
    // before every group of four MFMAs, exposing the LDS latency eight times per K-slice.  Here the six ds_read_b128 of k-step ks+1
    // are issued (inline asm, so the compiler neither merges nor reorders them) before the eight MFMAs of k-step ks, and a counted
    // s_waitcnt lgkmcnt(6) retires exactly the previous k-step's reads.  All four A (two W) fragments of a k-step share one address
    // register: rows 32 apart have the same swizzle, so they differ by an immediate offset.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t lds0 = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    uint32_t a_ad[4], w_ad[4];
    {
        const int ra = wm * 128 + l31, rw = wn * 64 + l31;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            a_ad[ks] = lds0 + ra * 128 + (((2 * ks + hi) ^ ((ra >> 1) & 7)) << 4);
            w_ad[ks] = lds0 + B_TILE + rw * 128 + (((2 * ks + hi) ^ ((rw >> 1) & 7)) << 4);
        }
    }
    u32x4 fa[2][4], fw[2][2];
#define TCOW_DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr))
#define TCOW_READ_FRAGS(buf, ks, so)                                            \
    do {                                                                        \
        const uint32_t aa = a_ad[ks] + (so), ww = w_ad[ks] + (so);              \
        TCOW_DSR(fw[buf][0], ww, 0); TCOW_DSR(fw[buf][1], ww, 4096);            \
        TCOW_DSR(fa[buf][0], aa, 0); TCOW_DSR(fa[buf][1], aa, 4096);            \
        TCOW_DSR(fa[buf][2], aa, 8192); TCOW_DSR(fa[buf][3], aa, 12288);        \
    } while (0)
#define TCOW_MFMA8(buf)                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                        \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                    \
            acc[i][j] = TCOW_MFMA_32x32x16_H16(__builtin_bit_cast(bf16x8, fa[buf][i]), __builtin_bit_cast(bf16x8, fw[buf][j]), acc[i][j], 0, 0, 0)

    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    TCOW_READ_FRAGS(0, 0, 0u);
    for (int kt = 0; kt < nk; ++kt) {
        const uint32_t so = (uint32_t)(kt & 1) * B_STAGE;
        if (kt + 1 < nk) issue(kt + 1, (kt & 1) ^ 1);
        TCOW_READ_FRAGS(1, 1, so);
        asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        TCOW_MFMA8(0);
        TCOW_READ_FRAGS(0, 2, so);
        asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        TCOW_MFMA8(1);
        TCOW_READ_FRAGS(1, 3, so);
        asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        TCOW_MFMA8(0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        TCOW_MFMA8(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) TCOW_READ_FRAGS(0, 0, so ^ (uint32_t)B_STAGE);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#undef TCOW_DSR
#undef TCOW_READ_FRAGS
#undef TCOW_MFMA8

    // ---- epilogue: every wave stages its own 128 x 64 tile through a private 16 KiB LDS region, 64 rows at a time, and writes
    // full output rows (128 B bf16 / 256 B f32 per row).  No workgroup barrier: a wave's LDS operations execute in order.
    float* ct = reinterpret_cast<float*>(smem + wave * 16384);
    const int c4 = (lane & 15) * 4;
    const int gn = n0 + wn * 64 + c4;
    const bool col_ok = gn < p.N;
    const float4 b4 = (p.bias && col_ok) ? ld4(p.bias + gn) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int mrow0 = m0 + wm * 128 + pass * 64;
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    ct[(ii * 32 + crow32(r, hi)) * 64 + j * 32 + l31] = acc[pass * 2 + ii][j][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (col_ok) epi_rows(p, ct, 64, b4, mrow0 + (lane >> 4), lane >> 4, 4, c4, gn);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of this pass done before the next pass overwrites the region
    }
}

// ---- 320 x 256 tile, 8 waves (2 x 4, 160 x 64 each), one workgroup per CU.  Why this odd shape: the global->LDS stream bounds
// these GEMMs, and (a) 320 x 256 moves (320+256)/(320*256) = 1/142 B per FLOP (256-square 1/128, 128-square 1/64), (b) the path's
// M = 27 090 token rows are 84.7 x 320, so N = 768 / 2304 / 3072 give 255 / 765 / 1020 tiles = 0.996 of 1 / 3 / 4 full rounds
// over the 256 CUs (256-square: 318 tiles = 1.24 rounds for N = 768, which is why those GEMMs had to stay on the 128-square
// kernel).  LDS: (320 + 256) rows x 128 B x 2 stages = 144 KiB.  160 accumulator registers per lane + two fragment sets.
// (A 4-wave version with 160 x 128 per wave needs 320 accumulator registers: hipcc then shuttles accumulators between AGPRs and
// VGPRs around every MFMA -- 480 v_accvgpr moves per K-slice.)
constexpr int C_BM = 320, C_BN = 256;
constexpr int C_ATILE = C_BM * 128;             // 40 KiB
constexpr int C_WTILE = C_BN * 128;             // 32 KiB
constexpr int C_STAGE = C_ATILE + C_WTILE;      // 72 KiB
constexpr int C_LDS = 2 * C_STAGE;              // 144 KiB

// The main loop was first built stand-alone in tools/gemm_p8.hip (16x16x32 MFMAs on 1 KiB subtiles, four phases per K tile, wave rows staggered by a
// barrier): the accumulators sit as [10 row blocks of 16][4 column blocks of 16], the form of the shared epilogue (the round-2 two-stage loop on
// 32x32x16 MFMAs -- 7-12 % slower on every shape, profiles/r03_gemm_shapes.txt -- is gone).
template <typename E>
__global__ __launch_bounds__(512, 2) void gemm_nt_bf16_320_kernel(NtParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int nblk = p.tiles_m * p.tiles_n;
    const int pid = xcd_remap(blockIdx.x, nblk);
    int pm, pn;
    nt_tile_of(pid, p.tiles_m, p.tiles_n, p.band, pm, pn);
    const int m0 = pm * C_BM, n0 = pn * C_BN;
    f32x4 acc16[10][4];
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc16[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // (see tools/gemm_p8.hip for the layout and the ordering argument; BM = 320: 20 row blocks, 5 per wave and phase)
    constexpr int ARB = 20, RBH = 5, A_PLANE = ARB * 1024, KH = A_PLANE + 16 * 1024, KTILE = 2 * KH, NA = 3;
    const int wr = wm, wc = wn;
    const bf16_t* a_base = p.A + (size_t)m0 * p.lda;
    const bf16_t* w_base = p.W + (size_t)n0 * p.ldw;
    uint32_t a_src[NA], w_src[2];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int r = (wave + 8 * j) * 16 + (lane >> 2);
        const int rr = m0 + r < p.M ? r : p.M - 1 - m0;
        a_src[j] = (uint32_t)(rr * p.lda + ((lane & 3) ^ ((lane >> 4) & 3)) * 8);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (wave + 8 * j) * 16 + (lane >> 2);
        const int rr = n0 + r < p.N ? r : p.N - 1 - n0;
        w_src[j] = (uint32_t)(rr * p.ldw + ((lane & 3) ^ ((lane >> 4) & 3)) * 8);
    }
    const bool a_last = wave + 16 < ARB;
    auto load_a = [&](int kt, int kh) {
        char* dst = smem + (kt & 1) * KTILE + kh * KH;
        const bf16_t* g = a_base + (size_t)kt * 64 + kh * 32;
        glds16(g + a_src[0], dst + wave * 1024); glds16(g + a_src[1], dst + (wave + 8) * 1024);
        if (a_last) glds16(g + a_src[2], dst + (wave + 16) * 1024);
    };
    auto load_w = [&](int kt, int kh) {
        char* dst = smem + (kt & 1) * KTILE + kh * KH + A_PLANE;
        const bf16_t* g = w_base + (size_t)kt * 64 + kh * 32;
        glds16(g + w_src[0], dst + wave * 1024); glds16(g + w_src[1], dst + (wave + 8) * 1024);
    };
    typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
    const uint32_t lds0_ = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    const uint32_t frag_off = (uint32_t)((lane & 15) * 64 + (((lane >> 4) ^ (((lane & 15) >> 2) & 3)) << 4));
    const uint32_t a_ad = lds0_ + (wr * (ARB / 2)) * 1024 + frag_off;
    const uint32_t w_ad = lds0_ + A_PLANE + (wc * 4) * 1024 + frag_off;
    u32x4_ fa[2][RBH], fw[2][4];
#define P8_DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))
    auto read_a = [&](u32x4_ (&f)[RBH], uint32_t base, int ri) {
        if (ri == 0) { P8_DSR(f[0], base, 0); P8_DSR(f[1], base, 1024); P8_DSR(f[2], base, 2048); P8_DSR(f[3], base, 3072); P8_DSR(f[4], base, 4096); }
        else { P8_DSR(f[0], base, 5120); P8_DSR(f[1], base, 6144); P8_DSR(f[2], base, 7168); P8_DSR(f[3], base, 8192); P8_DSR(f[4], base, 9216); }
    };
    auto read_w = [&](u32x4_ (&f)[4], uint32_t base) { P8_DSR(f[0], base, 0); P8_DSR(f[1], base, 1024); P8_DSR(f[2], base, 2048); P8_DSR(f[3], base, 3072); };
    auto mfma_block = [&](const u32x4_ (&fA)[RBH], const u32x4_ (&fW)[4], int ri) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < RBH; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc16[ri * RBH + i][j] = TCOW_MFMA_16x16x32_H16(__builtin_bit_cast(bf16x8, fW[j]), __builtin_bit_cast(bf16x8, fA[i]), acc16[ri * RBH + i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    auto wait_vm = [&](bool all) {
        if (all) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (a_last) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    };
#define P8_PHASE_TAIL(set_a, set_w, ri)                                                                   \
    do {                                                                                              \
        __builtin_amdgcn_s_barrier();                                                                 \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                           \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        mfma_block(fa[set_a], fw[set_w], ri);                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        __builtin_amdgcn_s_barrier();                                                                 \
    } while (0)
    const int nk = p.K / 64;
    load_a(0, 0); load_w(0, 0); load_a(0, 1); load_w(0, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
        const uint32_t bo = (uint32_t)(kt & 1) * KTILE;
        const bool more = kt + 1 < nk;
        read_w(fw[0], w_ad + bo); read_a(fa[0], a_ad + bo, 0);
        if (more) load_a(kt + 1, 0);
        P8_PHASE_TAIL(0, 0, 0);
        read_a(fa[1], a_ad + bo, 1);
        if (more) load_w(kt + 1, 0);
        wait_vm(!more);
        P8_PHASE_TAIL(1, 0, 1);
        read_w(fw[1], w_ad + bo + KH); read_a(fa[0], a_ad + bo + KH, 0);
        if (more) load_a(kt + 1, 1);
        P8_PHASE_TAIL(0, 1, 0);
        read_a(fa[1], a_ad + bo + KH, 1);
        if (more) load_w(kt + 1, 1);
        wait_vm(!more);
        P8_PHASE_TAIL(1, 1, 1);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();
#undef P8_DSR
#undef P8_PHASE_TAIL
    wave_tile_epilogue_160x64<E>(p, smem + wave * (64 * 68 * 4), acc16, lane, m0 + wm * 160, n0 + wn * 64);
}

__global__ __launch_bounds__(256, 2) void gemm_nt_bf16_kernel(NtParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;

    const int nblk = p.tiles_m * p.tiles_n;
    const int pid = xcd_remap(blockIdx.x, nblk);
    const int pm = pid / p.tiles_n, pn = pid - pm * p.tiles_n;
    const int m0 = pm * BM, n0 = pn * BN;
    const float4 b4 = epi_bias(p, tid, n0);

    // ---- per-lane source pointers for the direct-to-LDS loads: wave w issues wave-loads 4w..4w+3 per operand,
    // each covering 8 tile rows x 128 B; lane -> (row r = 8*q + (lane>>3), LDS chunk position lane&7).
    const bf16_t* a_src[4];
    const bf16_t* w_src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (wave * 4 + j) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        int gm = m0 + r; gm = gm < p.M ? gm : p.M - 1;
        int gn = n0 + r; gn = gn < p.N ? gn : p.N - 1;
        a_src[j] = p.A + (size_t)gm * p.lda + c * 8;
        w_src[j] = p.W + (size_t)gn * p.ldw + c * 8;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.K / BK;
    auto issue = [&](int kt, int stage) {
        char* sa = smem + stage * STAGE_BYTES;
        char* sw = sa + TILE_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(a_src[j] + (size_t)kt * BK, sa + (wave * 4 + j) * 1024);
            glds16(w_src[j] + (size_t)kt * BK, sw + (wave * 4 + j) * 1024);
        }
    };

    // fragment byte offsets inside a tile (row-dependent part), constant over k
    int a_off[2], w_off[2], a_sw[2], w_sw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ra = wm * 64 + i * 32 + l31, rw = wn * 64 + i * 32 + l31;
        a_off[i] = ra * 128; a_sw[i] = (ra >> 1) & 7;
        w_off[i] = rw * 128; w_sw[i] = (rw >> 1) & 7;
    }

    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int stage = kt & 1;
        if (kt + 1 < nk) issue(kt + 1, stage ^ 1);
        const char* sa = smem + stage * STAGE_BYTES;
        const char* sw = sa + TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c = 2 * ks + hi;
            bf16x8 fa[2], fw[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(sa + a_off[i] + ((c ^ a_sw[i]) << 4)));
                fw[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(sw + w_off[i] + ((c ^ w_sw[i]) << 4)));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = TCOW_MFMA_32x32x16_H16(fa[i], fw[j], acc[i][j], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    nt_epilogue(p, smem, acc, b4, tid, wm, wn, l31, hi, m0, n0);
}

}  // namespace


// Tile order of the wide-output GEMMs (fc1, fc2's input gradient: N = 3072 at K = 768).  Row-major order gives an XCD a band of row tiles with all of W:
// 4.7 MB of W do not stay in a 4 MB L2 beside the A stream, every round of workgroups re-fetches them (FETCH_SIZE 4.4x the algorithmic bytes on the 320
// tile, 7.2x on the 160 tile).  Column bands (nt_tile_of) halve what an XCD keeps of W: measured per launch (profiles/r06_pmc_band.txt) 205 -> 172 MB with
// bands of 6 tiles on the 320 tile, 341 -> 227 MB with bands of 4 on the 160 tile -- and the same time within +-1 % (the refills come from the Infinity
// Cache and the kernel is not bound by them); narrower bands make more XCDs read the same A rows and fetch MORE (band 1: 516 MB).  Kept for the traffic.
int tcow_nt_band_for(const tcow_gemm_args* a, int tiles_n, int tile) {
    if (a->N < 3072) return 0;
    const int band = tile == 320 ? 6 : 4;
    return (tiles_n % band == 0 && tiles_n > band) ? band : 0;
}

int tcow_gemm_nt_bf16(hipStream_t stream, const tcow_gemm_args* a) {
    TCOW_CHECK_ARG(a->K % BK == 0, "tcow_gemm_nt(bf16): K=%d must be a multiple of %d", a->K, BK);
    TCOW_CHECK_ARG(a->lda % 8 == 0 && a->ldw % 8 == 0, "tcow_gemm_nt(bf16): lda/ldw must be multiples of 8 elements");
    TCOW_CHECK_ARG(a->ldc % 4 == 0 && a->N % 4 == 0, "tcow_gemm_nt(bf16): N and ldc must be multiples of 4");
    TCOW_CHECK_ARG((!a->resid || a->ldr % 4 == 0) && (!a->aux || a->ldaux % 4 == 0), "tcow_gemm_nt(bf16): ldr / ldaux must be multiples of 4");
    NtParams p = nt_params_from_args(a);
    p.tiles_m = cdiv(a->M, BM); p.tiles_n = cdiv(a->N, BN);
    TCOW_CHECK_ARG(a->tile == 0 || a->tile == 128 || a->tile == 160 || a->tile == 256 || a->tile == 320, "tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got %d)", a->tile);
    {
        // the 320 x 256 tile runs one workgroup per CU: take it when its tiles fill whole rounds of the 256 CUs
        const long t320 = (long)cdiv(a->M, C_BM) * cdiv(a->N, C_BN);
        const long rounds = (t320 + 255) / 256;
        const bool fills = t320 * 100 >= rounds * 256 * 80;   // (measured: still ahead of the 256 / 128 tiles at 88 % -- configs[3], configs[4])
        // the 160 x 256 tile at two workgroups per CU (gemm_nt_c2.hip): same shapes (its tiles are the wave rows of the 320 tile)
        // It takes the shapes where it measured ahead of the 320 tile at M = 27 090 (profiles/r04_gemm_c2.txt): short-K GEMMs with an f32 residual
        // epilogue (the HBM-bound epilogue hides under the co-resident workgroup's main loop) and plain short-K GEMMs of three rounds.  Same-box A/B
        // of the training step in round 4: 28.05 / 28.10 ms with this routing, 28.24 / 28.30 ms without the kernel.
        // ... and, since round 5, the x GELU' epilogue (fc2's input gradient): with its aux tile read non-temporally the pair fc2-gradient -> fc1-gradient takes
        // 250 us on the 160 tile, 260 on the 320 tile (269 before; profiles/r05_nontemporal.txt)
        const bool c2_pick = a->K <= 1024 && ((a->out_f32 && a->resid) || (a->act == TCOW_ACT_NONE && !a->row_scale && !a->resid && !a->bias2 && a->N >= 2304 && a->N < 3072) ||
                                               (a->act == TCOW_ACT_MUL_AUX && !a->out_f32 && !a->row_scale && !a->resid && !a->bias2));
        if (a->tile == 160 || (a->tile == 0 && c2_pick && fills && t320 >= 200 && tcow_gemm_nt_c2_ok(a))) {
            TCOW_CHECK_ARG(tcow_gemm_nt_c2_ok(a), "tcow_gemm_nt(bf16): tile 160 needs K %% 128 == 0 and operands below 2 GiB");
            return tcow_gemm_nt_bf16_c2(stream, a);
        }
        if (a->tile == 320 || (a->tile == 0 && fills && t320 >= 200)) {
            p.tiles_m = cdiv(a->M, C_BM); p.tiles_n = cdiv(a->N, C_BN);
            p.band = tcow_nt_band_for(a, p.tiles_n, 320);
            typedef void (*Kern)(NtParams);
            Kern k = nullptr;                    // (K % 64 == 0: checked above)
            nt_pick_epilogue(a, [&](auto e) { k = gemm_nt_bf16_320_kernel<decltype(e)>; });
            tcow_ensure_lds(reinterpret_cast<const void*>(k), C_LDS);
            hipLaunchKernelGGL(k, dim3(p.tiles_m * p.tiles_n), dim3(512), C_LDS, stream, p);
            TCOW_CHECK_LAUNCH();
            return TCOW_OK;
        }
    }
    // the 256-square tile runs one workgroup per CU: it only pays when there are several full rounds of tiles (>= ~2.7 per CU)
    if (a->tile == 256 || (a->tile == 0 && (long)cdiv(a->M, B_BM) * cdiv(a->N, B_BN) >= 700)) {
        p.tiles_m = cdiv(a->M, B_BM); p.tiles_n = cdiv(a->N, B_BN);
        tcow_ensure_lds(reinterpret_cast<const void*>(gemm_nt_bf16_256_kernel), B_LDS);
        hipLaunchKernelGGL(gemm_nt_bf16_256_kernel, dim3(p.tiles_m * p.tiles_n), dim3(512), B_LDS, stream, p);
        TCOW_CHECK_LAUNCH();
        return TCOW_OK;
    }
    // (tried and dropped on this tile: a 4-deep BK = 32 ring -- profiles/r01_gemm_variants.txt --, a register-direct epilogue with the swapped MFMA
    // orientation, BK = 32 two-stage and BK = 64 single-stage variants with 4 workgroups per CU: -5 ... -30 %)
    tcow_ensure_lds(reinterpret_cast<const void*>(gemm_nt_bf16_kernel), NT_LDS_BYTES);
    hipLaunchKernelGGL(gemm_nt_bf16_kernel, dim3(p.tiles_m * p.tiles_n), dim3(256), NT_LDS_BYTES, stream, p);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
