// bf16 weight-gradient GEMM (gfx950):  gemm_tn_bf16 : dW[N,K] += dY[M,N]^T . X[M,K], the token dimension split across workgroups.
//
// slab[z][N][K] = sum over token rows of slice z of dY[m][n] * X[m][k].
// Both operands have the contraction index (token row m) as their slow dimension, so the MFMA fragments
// (8 consecutive m for one column) are gathered with the LDS transpose read ds_read_b64_tr_b16:
// within a 16-lane group lane 4r+c supplies the address of row r / 4-element column quad c of a [4][16]
// block and receives column (lane&15), rows 0..3 (verified on hardware, profiles/r01_hw_probe.txt).
// LDS rows are 256 B (128 columns); 16-byte chunk c of row r sits at chunk position c ^ ((r&3)<<2) so the four
// rows a half-wave touches per read fall into four different 64-byte bank segments.
#include <stdlib.h>

#include "common.h"
#include "internal.h"
#include "gemm_glds.h"

namespace {

constexpr int TN_T = 128;                 // output tile edge (n and k)
constexpr int TN_MC = 32;                 // token rows per LDS stage: 32 KiB of LDS, 4 workgroups/CU (64 rows, 2 workgroups/CU: 5-25 % behind, profiles/r01_gemm_tn_ab.txt)

__device__ uint4 g_zero16 = {0u, 0u, 0u, 0u};

struct TnParams {
    int M, N, K;
    const bf16_t* dY; long ldy;
    const bf16_t* X; long ldx;
    float* slab;
    int tiles_n, tiles_k, mps, nz;   // mps: token rows per slice (multiple of TN_MC); nz slices
    float* bias_part;                // optional [nz][tiles_k][2][N] partial column sums of dY (bias gradient)
    int rows_per_pk;                 // LDS rows of each 64-row stage summed by the workgroup with k-tile index pk
};

__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int off0) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tile + off0));
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tile + off0 + 4 * 256));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

__global__ __launch_bounds__(256, 4) void gemm_tn_bf16_kernel(TnParams p) {
    constexpr int MC = TN_MC, TILE_BYTES_ = MC * 256, STAGE_BYTES_ = 2 * TILE_BYTES_;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware placement: blocks are dispatched round-robin over the 8 XCDs (private L2s).  All output tiles of one token
    // slice z read the same dY / X rows, so slice z is pinned to XCD z % 8: its rows are fetched from HBM once per XCD-resident
    // slice instead of once per XCD (measured: FETCH_SIZE 4-8x the algorithmic bytes with the naive order).
    const int ntile = p.tiles_n * p.tiles_k;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int z = xcd + 8 * (idx / ntile), tile = idx % ntile;
    if (z >= p.nz) return;
    const int pn = tile / p.tiles_k, pk = tile - pn * p.tiles_k;
    const int n0 = pn * TN_T, k0 = pk * TN_T;
    const int mbeg = z * p.mps;
    const int mend = (mbeg + p.mps < p.M) ? mbeg + p.mps : p.M;

    // direct-to-LDS loads: wave-load q (16 per operand per stage) covers tile rows 4q..4q+3 x 256 B.
    const int lrow = lane >> 4;
    const int schunk = (lane & 15) ^ (lrow << 2);
    int ncol = n0 + schunk * 8; const bool n_ok = ncol < p.N;     // N, K multiples of 8 -> whole chunk in or out
    int kcol = k0 + schunk * 8; const bool k_ok = kcol < p.K;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(&g_zero16);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto issue = [&](int mt, int stage) {
        char* sy = smem + stage * STAGE_BYTES_;
        char* sx = sy + TILE_BYTES_;
#pragma unroll
        for (int j = 0; j < MC / 16; ++j) {
            const int q = wave * (MC / 16) + j;
            const int gm = mt + q * 4 + lrow;
            const bool ok = gm < mend;
            const bf16_t* ys = (ok && n_ok) ? p.dY + (size_t)gm * p.ldy + ncol : zero;
            const bf16_t* xs = (ok && k_ok) ? p.X + (size_t)gm * p.ldx + kcol : zero;
            glds16(ys, sy + q * 1024);
            glds16(xs, sx + q * 1024);
        }
    };

    // transpose-read addressing (constant over the loop)
    const int q16 = lane & 15, g16 = (lane >> 4) & 1, hi = lane >> 5;
    int y_off[2], x_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cy = wm * 64 + i * 32 + 16 * g16 + 4 * (q16 & 3);
        const int cx = wn * 64 + i * 32 + 16 * g16 + 4 * (q16 & 3);
        const int rr = 8 * hi + (q16 >> 2);
        y_off[i] = rr * 256 + ((((cy >> 3) ^ ((q16 >> 2) << 2))) << 4) + (cy & 7) * 2;
        x_off[i] = rr * 256 + ((((cx >> 3) ^ ((q16 >> 2) << 2))) << 4) + (cx & 7) * 2;
    }

    // column-sum duty of this thread: column cs_col of the dY tile, LDS rows [cs_r0, cs_r1) of every stage
    const int cs_col = tid & 127;
    const int cs_lo = pk * p.rows_per_pk, cs_hi = (cs_lo + p.rows_per_pk < MC) ? cs_lo + p.rows_per_pk : MC;
    const int cs_mid = cs_lo + (cs_hi - cs_lo + 1) / 2;
    const int cs_r0 = (tid >> 7) ? cs_mid : cs_lo, cs_r1 = (tid >> 7) ? cs_hi : (cs_mid < cs_hi ? cs_mid : cs_hi);
    float colsum = 0.f;

    const int nmt = (mend - mbeg + MC - 1) / MC;
    if (nmt > 0) {
        issue(mbeg, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    for (int it = 0; it < nmt; ++it) {
        const int stage = it & 1;
        if (it + 1 < nmt) issue(mbeg + (it + 1) * MC, stage ^ 1);
        const char* sy = smem + stage * STAGE_BYTES_;
        const char* sx = sy + TILE_BYTES_;
#pragma unroll
        for (int ks = 0; ks < MC / 16; ++ks) {
            bf16x8 fy[2], fx[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fy[i] = tr_frag(sy, y_off[i] + ks * 16 * 256);
                fx[i] = tr_frag(sx, x_off[i] + ks * 16 * 256);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = TCOW_MFMA_32x32x16_H16(fy[i], fx[j], acc[i][j], 0, 0, 0);
        }
        if (p.bias_part) {
            // bias gradient = column sums of dY: the dY stage is already in LDS; the tiles_k workgroups that share it split
            // its 64 rows between them (and each between its two thread halves), so the extra work is a few LDS reads each.
#pragma unroll 4
            for (int r = cs_r0; r < cs_r1; ++r) {
                const int off = r * 256 + ((((cs_col >> 3) ^ ((r & 3) << 2))) << 4) + (cs_col & 7) * 2;
                colsum += bf2f(*reinterpret_cast<const bf16_t*>(sy + off));
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (p.bias_part && n0 + cs_col < p.N)
        p.bias_part[(((size_t)z * p.tiles_k + pk) * 2 + (tid >> 7)) * p.N + n0 + cs_col] = colsum;

    float* out = p.slab + (size_t)z * p.N * p.K;
    const int l31 = lane & 31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gk = k0 + wn * 64 + j * 32 + l31;
            if (gk >= p.K) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gn = n0 + wm * 64 + i * 32 + crow32(r, hi);
                if (gn < p.N) out[(size_t)gn * p.K + gk] = acc[i][j][r];
            }
        }
}

// ---- 256 x 256 output tile, 8 waves (2 x 4, 128 x 64 each), 64 token rows per stage, two stages = 128 KiB, one workgroup per CU.
// The 128-tile kernel above is bound by the global->LDS stream (a loads-only build takes 70 % of its time,
// profiles/r01_gemm_variants.txt); this tile moves half the bytes per FLOP.  Workgroups = tiles x slices <= 256 (one round):
// workgroup ids are handed out so that each XCD owns a contiguous range of (slice, tile) pairs, i.e. at most two token slices.
constexpr int T2 = 256;
constexpr int T2_MC = 64;
constexpr int T2_ROWB = T2 * 2;                 // 512 B per LDS row
constexpr int T2_TILE = T2_MC * T2_ROWB;        // 32 KiB per operand per stage
constexpr int T2_STAGE = 2 * T2_TILE;
constexpr int T2_LDS = 2 * T2_STAGE;            // 128 KiB

// one workgroup of the 256-tile weight-gradient GEMM `p`: pid = slice * tiles + tile
// SCHED = 1 (round 4): the stage's ONE wait + barrier sits between the third and the fourth k-step instead of at the stage end: the fourth
// k-step's fragments are in registers by then, so its MFMAs run right behind the barrier while the NEXT stage's first fragments are read and the
// stage after next is requested into the buffer this stage has just released -- no stage boundary at which all eight waves wait for the barrier,
// then for their first transpose reads, with the matrix pipe idle.  (The round-3 order -- wait + barrier at the stage end -- is gone: 553-566 vs 504 us per block.)
// SCHED = 2: the interleaved loop further down, for whole tiles with 32-bit offsets (tn_whole).
template <int SCHED>
__device__ __forceinline__ void tn256_body(const TnParams& p, const int pid, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int ntile = p.tiles_n * p.tiles_k;
    const int z = pid / ntile, tile = pid - z * ntile;
    const int pn = tile / p.tiles_k, pk = tile - pn * p.tiles_k;
    const int n0 = pn * T2, k0 = pk * T2;
    const int mbeg = z * p.mps;
    const int mend = (mbeg + p.mps < p.M) ? mbeg + p.mps : p.M;

    // direct-to-LDS loads: a wave-load covers 2 tile rows x 512 B; wave w issues wave-loads 4w..4w+3 of each operand per stage
    const int lrow = lane >> 5, cl = lane & 31;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(&g_zero16);
    int ycol[2], xcol[2];                                         // source column of this lane for even / odd wave-loads (row & 3 differs)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int r3 = (e << 1) | lrow;                            // (tile row) & 3 for wave-load q with q & 1 == e
        const int sc = cl ^ (r3 << 2);
        ycol[e] = n0 + sc * 8; xcol[e] = k0 + sc * 8;
    }
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto issue = [&](int mt, int stage) {
        char* sy = smem + stage * T2_STAGE;
        char* sx = sy + T2_TILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = wave * 4 + j;
            const int gm = mt + q * 2 + lrow;
            const bool ok = gm < mend;
            const bf16_t* ys = (ok && ycol[j & 1] < p.N) ? p.dY + (size_t)gm * p.ldy + ycol[j & 1] : zero;
            const bf16_t* xs = (ok && xcol[j & 1] < p.K) ? p.X + (size_t)gm * p.ldx + xcol[j & 1] : zero;
            glds16(ys, sy + q * 1024);
            glds16(xs, sx + q * 1024);
        }
    };
    const bool interior = n0 + T2 <= p.N && k0 + T2 <= p.K;
    // The fast path as buffer loads: descriptor + ONE per-lane byte offset per operand and row parity + a scalar row offset -- no vector
    // arithmetic per load, rows past M read as zeros.  (inline asm: hipcc does not count these loads; every wait in the loop is explicit.)
    const i32x4_ srd_y = make_srd(p.dY, ((long)(p.M - 1) * p.ldy + p.N) * 2), srd_x = make_srd(p.X, ((long)(p.M - 1) * p.ldx + p.K) * 2);
    const uint32_t yv0 = (uint32_t)(lrow * p.ldy + ycol[0]) * 2u, yv1 = (uint32_t)(lrow * p.ldy + ycol[1]) * 2u;
    const uint32_t xv0 = (uint32_t)(lrow * p.ldx + xcol[0]) * 2u, xv1 = (uint32_t)(lrow * p.ldx + xcol[1]) * 2u;
    const bool small32 = (long)p.M * p.ldy < (1L << 29) && (long)p.M * p.ldx < (1L << 29);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    auto issue_fast = [&](int mt, int stage) {
        const uint32_t dy = lds_base + stage * T2_STAGE + wave * 4096, dx = dy + T2_TILE;
        const uint32_t sy = (uint32_t)((long)(mt + wave * 8) * p.ldy * 2), sx = (uint32_t)((long)(mt + wave * 8) * p.ldx * 2);
        const uint32_t ry = (uint32_t)(2 * p.ldy * 2), rx = (uint32_t)(2 * p.ldx * 2);
        TCOW_BUFFER_GLDS16(yv0, srd_y, sy, dy); TCOW_BUFFER_GLDS16(xv0, srd_x, sx, dx);
        TCOW_BUFFER_GLDS16(yv1, srd_y, sy + ry, dy + 1024); TCOW_BUFFER_GLDS16(xv1, srd_x, sx + rx, dx + 1024);
        TCOW_BUFFER_GLDS16(yv0, srd_y, sy + 2 * ry, dy + 2048); TCOW_BUFFER_GLDS16(xv0, srd_x, sx + 2 * rx, dx + 2048);
        TCOW_BUFFER_GLDS16(yv1, srd_y, sy + 3 * ry, dy + 3072); TCOW_BUFFER_GLDS16(xv1, srd_x, sx + 3 * rx, dx + 3072);
    };
    // transpose-read addressing (constant over the loop)
    const int q16 = lane & 15, g16 = (lane >> 4) & 1, hi = lane >> 5;
    const int rr = 8 * hi + (q16 >> 2);
    int y_off[4], x_off[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cy = wm * 128 + i * 32 + 16 * g16 + 4 * (q16 & 3);
        y_off[i] = rr * T2_ROWB + ((((cy >> 3) ^ ((q16 >> 2) << 2))) << 4) + (cy & 7) * 2;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cx = wn * 64 + j * 32 + 16 * g16 + 4 * (q16 & 3);
        x_off[j] = rr * T2_ROWB + ((((cx >> 3) ^ ((q16 >> 2) << 2))) << 4) + (cx & 7) * 2;
    }

    // column-sum duty (bias gradient): column cs_col of the dY tile, rows [cs_r0, cs_r1) of every stage; the tiles_k workgroups
    // that share a dY tile split its 64 rows between them, and each between its two thread halves
    // (thread t sums the eight columns of 16-byte chunk t & 31 over rows cs_lo + (t >> 5), + 16, ...: at most four b128 reads per stage instead
    // of up to 32 two-byte ones; the sixteen row groups are folded through LDS once, after the loop)
    const int cs_col = tid & 255;
    const int cs_lo = pk * p.rows_per_pk, cs_hi = (cs_lo + p.rows_per_pk < T2_MC) ? cs_lo + p.rows_per_pk : T2_MC;
    const int cs_chunk = tid & 31, cs_rg = tid >> 5;
    float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // (a macro, expanded in both stage loops: as a lambda the same text compiles to different address arithmetic)
#define TN_COLSUM(sy)                                                                                                              \
    if (p.bias_part) {                                                                                                             \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                            \
            const int r = cs_lo + cs_rg + 16 * u;                                                                                  \
            if (r < cs_hi) {                                                                                                       \
                const uint4 v = *reinterpret_cast<const uint4*>((sy) + r * T2_ROWB + ((cs_chunk ^ ((r & 3) << 2)) << 4));          \
                csum[0] += bflo(v.x); csum[1] += bfhi(v.x); csum[2] += bflo(v.y); csum[3] += bfhi(v.y);                            \
                csum[4] += bflo(v.z); csum[5] += bfhi(v.z); csum[6] += bflo(v.w); csum[7] += bfhi(v.w);                            \
            }                                                                                                                      \
        }                                                                                                                          \
    }

    const int nmt = (mend - mbeg + T2_MC - 1) / T2_MC;
    auto issue_stage = [&](int st_, int buf_) {
        const int mt = mbeg + st_ * T2_MC;
        if (interior && small32 && (mt + T2_MC <= mend || mend == p.M)) issue_fast(mt, buf_); else issue(mt, buf_);
    };
    if constexpr (SCHED == 2) {
        // (every stage through the buffer loads: the host picks this variant for whole tiles and 32-bit offsets only)
        if (nmt > 0) {
            issue_fast(mbeg, 0);
            if (nmt > 1) { issue_fast(mbeg + T2_MC, 1); asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else if (nmt > 0) {
        issue(mbeg, 0);
        if (nmt > 1) { issue_stage(1, 1); asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }      // stage 1 (8 loads per wave) stays in flight
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // Transpose reads software-pipelined by hand, as in the NT kernels: the 12 ds_read_b64_tr_b16 of k-step ks+1 are issued
    // before the 8 MFMAs of k-step ks (inline asm + counted lgkmcnt; hipcc alone waits for each group right before its use).
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t lds0 = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    uint32_t ya[4], xa[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) ya[i] = lds0 + (uint32_t)y_off[i];
#pragma unroll
    for (int j = 0; j < 2; ++j) xa[j] = lds0 + (uint32_t)x_off[j];
    u32x2 fyl[2][4], fyh[2][4], fxl[2][2], fxh[2][2];
#define TCOW_TRR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))
#define TCOW_TN_READ(buf, ks, so)                                                                                          \
    do {                                                                                                                   \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                    \
            TCOW_TRR(fxl[buf][j], xa[j] + (so), T2_TILE + (ks) * 16 * T2_ROWB);                                            \
            TCOW_TRR(fxh[buf][j], xa[j] + (so), T2_TILE + (ks) * 16 * T2_ROWB + 4 * T2_ROWB);                              \
        }                                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                    \
            TCOW_TRR(fyl[buf][i], ya[i] + (so), (ks) * 16 * T2_ROWB);                                                      \
            TCOW_TRR(fyh[buf][i], ya[i] + (so), (ks) * 16 * T2_ROWB + 4 * T2_ROWB);                                        \
        }                                                                                                                  \
    } while (0)
#define TCOW_TN_FRAG(lo, hi) __builtin_bit_cast(bf16x8, (u32x4){(lo).x, (lo).y, (hi).x, (hi).y})
#define TCOW_TN_MFMA8(buf)                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                          \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                      \
            acc[i][j] = TCOW_MFMA_32x32x16_H16(TCOW_TN_FRAG(fyl[buf][i], fyh[buf][i]), TCOW_TN_FRAG(fxl[buf][j], fxh[buf][j]), acc[i][j], 0, 0, 0)

    if (nmt > 0) TCOW_TN_READ(0, 0, 0u);
    if constexpr (SCHED == 2) {
        // Every k-step as ONE block: its 8 MFMAs with the NEXT k-step's 12 transpose reads behind the first six of them (two each), the waits
        // counted per fragment -- issued as a burst before the MFMAs, the reads of all 8 waves queue up at the LDS while the MFMA pipe idles,
        // and then the LDS idles under the MFMAs: reads-only 30 us + MFMAs-only 60 us = 92 us measured with the loads off, no overlap at all
        // (profiles/r04_ubench_tn_ab.txt).  The fourth k-step also carries the 8 buffer loads of stage it+2, one behind each MFMA.
#define TN_NOP do { } while (0)
#define TN_MF(cur, i, j) acc[i][j] = TCOW_MFMA_32x32x16_H16(TCOW_TN_FRAG(fyl[cur][i], fyh[cur][i]), TCOW_TN_FRAG(fxl[cur][j], fxh[cur][j]), acc[i][j], 0, 0, 0); \
                    __builtin_amdgcn_sched_barrier(0)
#define TN_BLK(cur, nxt, OFFK, son, W0, B0, B1, B2, B3, B4, B5, B6, B7)                                                                  \
    do {                                                                                                                                 \
        asm volatile("s_waitcnt lgkmcnt(" #W0 ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0);                     \
        TN_MF(cur, 0, 0); TCOW_TRR(fxl[nxt][0], xa[0] + (son), T2_TILE + (OFFK)); TCOW_TRR(fxh[nxt][0], xa[0] + (son), T2_TILE + (OFFK) + 4 * T2_ROWB); B0; \
        TN_MF(cur, 0, 1); TCOW_TRR(fxl[nxt][1], xa[1] + (son), T2_TILE + (OFFK)); TCOW_TRR(fxh[nxt][1], xa[1] + (son), T2_TILE + (OFFK) + 4 * T2_ROWB); B1; \
        TN_MF(cur, 1, 0); TCOW_TRR(fyl[nxt][0], ya[0] + (son), (OFFK)); TCOW_TRR(fyh[nxt][0], ya[0] + (son), (OFFK) + 4 * T2_ROWB); B2;              \
        TN_MF(cur, 1, 1); TCOW_TRR(fyl[nxt][1], ya[1] + (son), (OFFK)); TCOW_TRR(fyh[nxt][1], ya[1] + (son), (OFFK) + 4 * T2_ROWB); B3;              \
        asm volatile("s_waitcnt lgkmcnt(10)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);    /* the previous block's fy[2] */ \
        TN_MF(cur, 2, 0); TCOW_TRR(fyl[nxt][2], ya[2] + (son), (OFFK)); TCOW_TRR(fyh[nxt][2], ya[2] + (son), (OFFK) + 4 * T2_ROWB); B4;              \
        TN_MF(cur, 2, 1); TCOW_TRR(fyl[nxt][3], ya[3] + (son), (OFFK)); TCOW_TRR(fyh[nxt][3], ya[3] + (son), (OFFK) + 4 * T2_ROWB); B5;              \
        asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);    /* ... and its fy[3] */  \
        TN_MF(cur, 3, 0); B6;                                                                                                            \
        TN_MF(cur, 3, 1); B7;                                                                                                            \
    } while (0)
        for (int it = 0; it < nmt; ++it) {
            const int stage = it & 1;
            const uint32_t so = (uint32_t)stage * T2_STAGE;
            const char* sy = smem + stage * T2_STAGE;
            TN_BLK(0, 1, 1 * 16 * T2_ROWB, so, 4, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP);
            TN_BLK(1, 0, 2 * 16 * T2_ROWB, so, 4, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP);
            TN_BLK(0, 1, 3 * 16 * T2_ROWB, so, 4, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP);
            TN_COLSUM(sy)
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __syncthreads();
            {
                const int mt2 = mbeg + (it + 2) * T2_MC;
                const bool more = it + 2 < nmt;
                const uint32_t dy = lds_base + so + wave * 4096, dx = dy + T2_TILE;
                const uint32_t by = (uint32_t)((long)(mt2 + wave * 8) * p.ldy * 2), bx = (uint32_t)((long)(mt2 + wave * 8) * p.ldx * 2);
                const uint32_t yw0 = more ? yv0 : 0x80000000u, yw1 = more ? yv1 : 0x80000000u;     // (the per-lane offset is the range-checked one)
                const uint32_t xw0 = more ? xv0 : 0x80000000u, xw1 = more ? xv1 : 0x80000000u;
                const uint32_t ry = (uint32_t)(2 * p.ldy * 2), rx = (uint32_t)(2 * p.ldx * 2);
                const uint32_t sn = so ^ (uint32_t)T2_STAGE;
                TN_BLK(1, 0, 0, sn, 0, TCOW_BUFFER_GLDS16(yw0, srd_y, by, dy), TCOW_BUFFER_GLDS16(xw0, srd_x, bx, dx), TCOW_BUFFER_GLDS16(yw1, srd_y, by + ry, dy + 1024),
                       TCOW_BUFFER_GLDS16(xw1, srd_x, bx + rx, dx + 1024), TCOW_BUFFER_GLDS16(yw0, srd_y, by + 2 * ry, dy + 2048), TCOW_BUFFER_GLDS16(xw0, srd_x, bx + 2 * rx, dx + 2048),
                       TCOW_BUFFER_GLDS16(yw1, srd_y, by + 3 * ry, dy + 3072), TCOW_BUFFER_GLDS16(xw1, srd_x, bx + 3 * rx, dx + 3072));
            }
        }
#undef TN_BLK
#undef TN_MF
#undef TN_NOP
    } else
    if constexpr (SCHED == 1) {
        for (int it = 0; it < nmt; ++it) {
            const int stage = it & 1;
            const uint32_t so = (uint32_t)stage * T2_STAGE;
            const char* sy = smem + stage * T2_STAGE;
            TCOW_TN_READ(1, 1, so);
            asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            TCOW_TN_MFMA8(0);
            TCOW_TN_READ(0, 2, so);
            asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            TCOW_TN_MFMA8(1);
            TCOW_TN_READ(1, 3, so);
            asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            TCOW_TN_MFMA8(0);
            TN_COLSUM(sy)
            // this wave's loads of stage it+1 (requested a whole stage ago) have landed, its reads of this stage are back (the fourth k-step's
            // fragments are in registers): behind the barrier the buffer of this stage is free and stage it+1 is visible
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __syncthreads();
            if (it + 2 < nmt) issue_stage(it + 2, stage);
            if (it + 1 < nmt) TCOW_TN_READ(0, 0, so ^ (uint32_t)T2_STAGE);
            __builtin_amdgcn_sched_barrier(0);
            TCOW_TN_MFMA8(1);
        }
    }
    // (SCHED = 2: the last stage's fourth k-step has requested fragments of a stage that does not exist into set 0.  The wait re-defines those
    // registers, so that hipcc -- which knows nothing of reads issued by asm statements -- cannot hand them to the code behind the loop before the
    // data is in: see the same note in gemm_nt_c2.hip, where exactly that corrupted tiles)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(fxl[0][0]), "+v"(fxl[0][1]), "+v"(fxh[0][0]), "+v"(fxh[0][1]), "+v"(fyl[0][0]), "+v"(fyl[0][1]), "+v"(fyl[0][2]), "+v"(fyl[0][3]),
                   "+v"(fyh[0][0]), "+v"(fyh[0][1]), "+v"(fyh[0][2]), "+v"(fyh[0][3])
                 :: "memory");
    __builtin_amdgcn_sched_barrier(0);
#undef TCOW_TRR
#undef TN_COLSUM
#undef TCOW_TN_READ
#undef TCOW_TN_FRAG
#undef TCOW_TN_MFMA8
    if (p.bias_part) {
        // fold the sixteen row groups (the operand stages are dead: the loop ended on a barrier): red[rg][256 columns]
        float* red = reinterpret_cast<float*>(smem);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[cs_rg * 256 + cs_chunk * 8 + e] = csum[e];
        __syncthreads();
        if (n0 + cs_col < p.N) {
            float t = 0.f;
            if (tid < 256) {
#pragma unroll
                for (int g = 0; g < 16; ++g) t += red[g * 256 + cs_col];
            }
            p.bias_part[(((size_t)z * p.tiles_k + pk) * 2 + (tid >> 8)) * p.N + n0 + cs_col] = t;      // (the second half-row of the table stays zero)
        }
        __syncthreads();
    }

    float* out = p.slab + (size_t)z * p.N * p.K;
    const int l31 = lane & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gk = k0 + wn * 64 + j * 32 + l31;
            if (gk >= p.K) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gn = n0 + wm * 128 + i * 32 + crow32(r, hi);
                if (gn < p.N) out[(size_t)gn * p.K + gk] = acc[i][j][r];
            }
        }
}

template <int SCHED>
__global__ __launch_bounds__(512, 2) void gemm_tn_bf16_256_kernel(TnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    tn256_body<SCHED>(p, xcd_remap(blockIdx.x, gridDim.x), smem);
}

// Grouped launch: the weight gradients of ONE transformer block (7 Linear layers, 153 tiles of 256 x 256 at ViT-B) as one grid.  Launched
// one by one, a 768 x 768 weight has 9 tiles and needs 28 token slices to fill the chip -- 66 MB of f32 partials written and read back per
// GEMM (11.5 GB per training step), a fold launch each, and a ramp / tail per launch.  Together the tiles fill three rounds with FIVE slices:
// every workgroup walks 5 418 token rows, the partials shrink 5x and one launch replaces seven.
struct TnGroup { int n; int first[TCOW_TN_GROUP_MAX + 1]; TnParams p[TCOW_TN_GROUP_MAX]; };
template <int SCHED>
__global__ __launch_bounds__(512, 2) void gemm_tn_bf16_256_group_kernel(TnGroup g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int pid = xcd_remap(blockIdx.x, gridDim.x);
    int k = 0;
    while (k + 1 < g.n && pid >= g.first[k + 1]) ++k;           // workgroup-uniform
    const TnParams p = g.p[k];
    tn256_body<SCHED>(p, pid - g.first[k], smem);
}

}  // namespace

// slices for the 256-tile kernel: as many as fit one round of workgroups (<= 256), at least 256 token rows each
int tcow_tn_splits_256(int M, int N, int K) {
    const int tiles = cdiv(N, T2) * cdiv(K, T2);
    int s = 256 / tiles;
    const int max_s = M / 256;
    if (s > max_s) s = max_s;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    return s;
}
bool tcow_tn_use_256(int M, int N, int K) {
    const int tiles = cdiv(N, T2) * cdiv(K, T2);
    // (a 768 x 768 weight = 9 tiles x 28 slices still wins 12 % over the 128-tile kernel despite the larger slab fold)
    return M >= 4096 && N >= 256 && K >= 256 && tiles >= 9 && tiles <= 256;
}

// Stage loop of the 256-tile weight-gradient kernel (tn256_body): whole 256-tiles with 32-bit byte offsets take the interleaved loop (SCHED = 2 --
// the transpose reads of the next k-step and the next stage's requests spread between the MFMAs of every k-step, the loads as buffer loads with
// scalar row offsets), anything else the general one (SCHED = 1: the same wait / barrier placement, general addressing).
static bool tn_whole(int M, int N, int K, long ldy, long ldx) { return N % T2 == 0 && K % T2 == 0 && (long)M * ldy < (1L << 29) && (long)M * ldx < (1L << 29); }

// launch parameters of one weight gradient on output tiles of `tile` (TN_T with mc = TN_MC token rows per stage, or T2 with T2_MC), `splits` token slices requested
static TnParams tn_params(int M, int N, int K, const bf16_t* dY, long ldy, const bf16_t* X, long ldx, float* slab, float* bias_part, int splits, int tile, int mc) {
    TnParams p;
    p.M = M; p.N = N; p.K = K; p.dY = dY; p.ldy = ldy; p.X = X; p.ldx = ldx; p.slab = slab;
    p.tiles_n = cdiv(N, tile); p.tiles_k = cdiv(K, tile);
    p.mps = ((cdiv(M, splits) + 63) / 64) * 64;
    p.nz = cdiv(M, p.mps);
    p.bias_part = bias_part;
    p.rows_per_pk = cdiv(mc, p.tiles_k);
    return p;
}
template <typename P>
static void tn_launch_256(void (*kernel)(P), int grid, hipStream_t stream, const P& p) {
    tcow_ensure_lds(reinterpret_cast<const void*>(kernel), T2_LDS);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), T2_LDS, stream, p);
}

int tcow_gemm_tn_bf16(hipStream_t stream, int M, int N, int K, const bf16_t* dY, long ldy, const bf16_t* X, long ldx, float* slab, int splits,
                      int* nz_out, float* bias_part, int* bias_parts_out) {
    TCOW_CHECK_ARG(N % 8 == 0 && K % 8 == 0 && ldy % 8 == 0 && ldx % 8 == 0, "tcow_gemm_tn(bf16): N, K, ldy, ldx must be multiples of 8");
    const bool big = tcow_tn_use_256(M, N, K);
    const TnParams p = big ? tn_params(M, N, K, dY, ldy, X, ldx, slab, bias_part, splits, T2, T2_MC) : tn_params(M, N, K, dY, ldy, X, ldx, slab, bias_part, splits, TN_T, TN_MC);
    *nz_out = p.nz;
    if (bias_parts_out) *bias_parts_out = p.nz * p.tiles_k * 2;
    if (big) {
        tn_launch_256(tn_whole(M, N, K, ldy, ldx) ? gemm_tn_bf16_256_kernel<2> : gemm_tn_bf16_256_kernel<1>, p.nz * p.tiles_n * p.tiles_k, stream, p);
    } else {
        const dim3 grid(8 * cdiv(p.nz, 8) * p.tiles_n * p.tiles_k);
        hipLaunchKernelGGL(gemm_tn_bf16_kernel, grid, dim3(256), 2 * 2 * TN_MC * 256, stream, p);
    }
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// ---- grouped weight-gradient launch (see gemm_tn_bf16_256_group_kernel).  All problems share M and the slice count nz.
bool tcow_tn_group_ok(int n, const tcow_tn_problem* pr) {
    if (n < 2 || n > TCOW_TN_GROUP_MAX) return false;
    for (int i = 0; i < n; ++i) {
        if (pr[i].M != pr[0].M || !tcow_tn_use_256(pr[i].M, pr[i].N, pr[i].K)) return false;
        if (pr[i].N % 8 || pr[i].K % 8 || pr[i].ldy % 8 || pr[i].ldx % 8) return false;
    }
    return true;
}
// common slice count: the cheapest one under  cost(s) = 1 / (fill of whole rounds of 256 workgroups) + 0.044 s  -- every slice writes and re-reads
// one f32 image of all the group's weights: slab store + fold measured at 22 % of the loop time with five slices (profiles/r04_ubench_tn_ab.txt,
// r04_step_kernel_stats.txt).  One ViT-B block (153 tiles): 5 slices (765 workgroups = 2.99 rounds); four blocks (612 tiles): 2 slices
// (1224 workgroups = 4.78 rounds, 60 % less slab traffic for 4 % more tail).  >= 256 token rows per slice.
int tcow_tn_group_slices(int n, const tcow_tn_problem* pr) {
    int tiles = 0;
    for (int i = 0; i < n; ++i) tiles += cdiv(pr[i].N, T2) * cdiv(pr[i].K, T2);
    int max_s = pr[0].M / 256; if (max_s > 64) max_s = 64; if (max_s < 1) max_s = 1;
    int best = 1; double best_cost = 1e30;
    for (int s = 1; s <= max_s; ++s) {
        const int wg = s * tiles, rounds = cdiv(wg, 256);
        const double cost = (rounds * 256.0) / (double)wg + 0.044 * s;
        if (cost < best_cost - 1e-9) { best_cost = cost; best = s; }
    }
    return best;
}
int tcow_gemm_tn_bf16_group(hipStream_t stream, int n, const tcow_tn_problem* pr, int nz_req, float* const* slabs, float* const* bias_parts, int* nz_out,
                            int* bias_nparts) {
    TnGroup g;
    g.n = n;
    int first = 0, nz = 0;
    for (int i = 0; i < n; ++i) {
        TnParams& p = g.p[i];
        p = tn_params(pr[i].M, pr[i].N, pr[i].K, (const bf16_t*)pr[i].dY, pr[i].ldy, (const bf16_t*)pr[i].X, pr[i].ldx, slabs[i], bias_parts[i], nz_req, T2, T2_MC);
        nz = p.nz;
        bias_nparts[i] = p.nz * p.tiles_k * 2;
        g.first[i] = first;
        first += p.nz * p.tiles_n * p.tiles_k;
    }
    g.first[n] = first;
    for (int i = n + 1; i <= TCOW_TN_GROUP_MAX; ++i) g.first[i] = first;
    *nz_out = nz;
    bool whole = true;
    for (int i = 0; i < n; ++i) whole = whole && tn_whole(pr[i].M, pr[i].N, pr[i].K, pr[i].ldy, pr[i].ldx);
    tn_launch_256(whole ? gemm_tn_bf16_256_group_kernel<2> : gemm_tn_bf16_256_group_kernel<1>, first, stream, g);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
