// 256-tile kernels of the 16-bit weight-gradient GEMM (included by gemm_tn_bf16.hip; every weight of the training step): 256 x 256 output tile on 8 waves
// (2 x 4, 128 x 64 each), TNL_ROWS = 64 token rows per stage, two stages = 128 KiB of LDS, one workgroup per CU.  The 128-tile kernel is bound by the
// global->LDS stream (a loads-only build takes 70 % of its time, profiles/r01_gemm_variants.txt); this tile moves half the bytes per FLOP.
// 16x16x32 MFMAs with X as the A and dY as the B operand: a fragment is 16 columns x 32 tokens (lane l: column l & 15, tokens 8 (l >> 4) ... + 7), one
// "lo" + one "hi" transpose read each.  A half-wave then touches EIGHT rows, {b ... b+3, b+8 ... b+11}, 32 bytes of each: the image of the 512-byte
// rows is c ^ ((r&3)<<2) ^ (((r>>3)&1)<<1), eight different 32-byte bank segments (gemm_tn_layout.h: the image, the loads' source permutation, the
// read addresses; checked lane by lane on the CPU by tools/tn_layout_check.cpp).  A lane's four accumulators of a 16 x 16 block are four consecutive
// k of one n: the slab store is one 16-byte store per block.
// Workgroups = tiles x slices <= 256 (one round) for a single problem: workgroup ids are handed out so that each XCD owns a contiguous range of
// (slice, tile) pairs, i.e. at most two token slices.
namespace {
constexpr int T2 = TNL_COLS;                    // output tile edge
constexpr int T2_MC = TNL_ROWS;                 // token rows per stage
constexpr int T2_STAGE = 2 * TNL_TILE;          // dY + X: 64 KiB
constexpr int T2_LDS = 2 * T2_STAGE;            // 128 KiB

// one workgroup of the 256-tile weight-gradient GEMM `p`: pid = slice * tiles + tile.  Both SCHED values run ONE stage loop (described further down).
// SCHED = 2, for whole tiles with 32-bit offsets (tcow_tn_whole): every stage by buffer loads, issued one behind every second MFMA of the fourth block.
// SCHED = 1: the general addressing (edge tiles, 64-bit offsets); the stage after next is requested in one piece behind the barrier.
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
    const int lrow = lane >> 5;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(&g_zero16);
    int ycol[2], xcol[2];                                         // source column of this lane for even / odd wave-loads (the row's swizzle differs)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int sc = tnl_load_chunk(wave, e, lane);              // rows 8 wave + 2 j + lrow: the swizzle depends on j through j & 1 only
        ycol[e] = n0 + sc * 8; xcol[e] = k0 + sc * 8;
    }
    // accumulators of 16x16x32 MFMAs with X as the A and dY as the B operand: acc[i][j] is the block of columns n = 16 i ... + 15 and
    // k = 16 j ... + 15 of the wave's 128 x 64, lane l holding n = l & 15 and the FOUR CONSECUTIVE k = 4 (l >> 4) ... + 3 -- one 16-byte store each
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

    auto issue = [&](int mt, int stage) {
        char* sy = smem + stage * T2_STAGE;
        char* sx = sy + TNL_TILE;
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
        const uint32_t dy = lds_base + stage * T2_STAGE + wave * 4096, dx = dy + TNL_TILE;
        const uint32_t sy = (uint32_t)((long)(mt + wave * 8) * p.ldy * 2), sx = (uint32_t)((long)(mt + wave * 8) * p.ldx * 2);
        const uint32_t ry = (uint32_t)(2 * p.ldy * 2), rx = (uint32_t)(2 * p.ldx * 2);
        TCOW_BUFFER_GLDS16(yv0, srd_y, sy, dy); TCOW_BUFFER_GLDS16(xv0, srd_x, sx, dx);
        TCOW_BUFFER_GLDS16(yv1, srd_y, sy + ry, dy + 1024); TCOW_BUFFER_GLDS16(xv1, srd_x, sx + rx, dx + 1024);
        TCOW_BUFFER_GLDS16(yv0, srd_y, sy + 2 * ry, dy + 2048); TCOW_BUFFER_GLDS16(xv0, srd_x, sx + 2 * rx, dx + 2048);
        TCOW_BUFFER_GLDS16(yv1, srd_y, sy + 3 * ry, dy + 3072); TCOW_BUFFER_GLDS16(xv1, srd_x, sx + 3 * rx, dx + 3072);
    };
    // transpose-read addressing (constant over the loop)
    // (gemm_tn_layout.h: the "lo" read of the fragment of 16 columns, first MFMA step; "hi" and the second step are immediate offsets)
    int y_off[8], x_off[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) y_off[i] = tnl_read_off(lane, wm * 128 + i * 16, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) x_off[j] = tnl_read_off(lane, wn * 64 + j * 16, 0);

    // column-sum duty (bias gradient): column cs_col of the dY tile, rows [cs_r0, cs_r1) of every stage; the tiles_k workgroups
    // that share a dY tile split its 64 rows between them, and each between its two thread halves
    // (thread t sums the eight columns of 16-byte chunk t & 31 over rows cs_lo + (t >> 5), + 16, ...: at most four b128 reads per stage instead
    // of up to 32 two-byte ones; the sixteen row groups are folded through LDS once, after the loop)
    const int cs_col = tid & 255;
    const int cs_lo = pk * p.rows_per_pk, cs_hi = (cs_lo + p.rows_per_pk < T2_MC) ? cs_lo + p.rows_per_pk : T2_MC;
    const int cs_chunk = tid & 31, cs_rg = tid >> 5;
    float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // (a macro: as a lambda the same text compiles to different address arithmetic)
#define TN_COLSUM(sy)                                                                                                              \
    if (p.bias_part) {                                                                                                             \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                            \
            const int r = cs_lo + cs_rg + 16 * u;                                                                                  \
            if (r < cs_hi) {                                                                                                       \
                const uint4 v = *reinterpret_cast<const uint4*>((sy) + tnl_colsum_off(r, cs_chunk));                               \
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
    // The stage loop.  A stage (64 token rows) is two MFMA steps of 32 tokens; a step is 8 dY x 4 X fragments = 32 MFMAs, issued as two blocks of
    // 16: block P multiplies the step's dY fragments 0-3 (set FY[0]), block Q its fragments 4-7 (FY[1]), both with the step's four X fragments
    // (FX[xb], double-buffered over steps).  A block's MFMAs run X-fragment-major, so its first four need one X fragment and its dY set.
    // The four blocks of a stage share ONE wait + barrier, between the third and the fourth block instead of at the stage end: the fourth block's fragments
    // are in registers by then, so its MFMAs run right behind the barrier -- no stage boundary at which all eight waves wait for the barrier, then for their
    // first transpose reads, with the matrix pipe idle -- while it carries the 8 buffer loads of the stage after next (into the buffer the barrier has
    // released) and reads its fragments from the NEXT stage.
    // Transpose reads (inline asm, counted lgkmcnt: hipcc knows nothing of them): ONE behind each of the first 12 MFMAs of a block, 24 per step.
    //   P issues   X2 X3 (this step, used by its own MFMAs 8.. and 12..), then FY[1] 0-3 (this step, for Q)
    //   Q issues   X0 of the next step (other FX set), FY[0] 0-3 of the next step, X1 of the next step
    // each as a "lo" and a "hi" read.  Reads return in order, so "at most n outstanding" names the fragment an MFMA is about to use; the n below
    // are (reads issued so far) - (reads up to and including that fragment).
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    uint32_t ya[8], xa[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) ya[i] = lds_base + (uint32_t)y_off[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) xa[j] = lds_base + (uint32_t)(TNL_TILE + x_off[j]);
    u32x2 fyl[2][4], fyh[2][4], fxl[2][4], fxh[2][4];
    constexpr int STEPB = TNL_STEP * TNL_ROWB;                        // bytes from the first MFMA step of a stage to the second
#define TN_SB __builtin_amdgcn_sched_barrier(0)
#define TN_TRR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off)); TN_SB
#define TN_RXL(xb, j, OFF) TN_TRR(fxl[xb][j], xa[j], (OFF))
#define TN_RXH(xb, j, OFF) TN_TRR(fxh[xb][j], xa[j], (OFF) + TNL_HI)
#define TN_RYL(h, i, OFF) TN_TRR(fyl[h][i], ya[4 * (h) + (i)], (OFF))
#define TN_RYH(h, i, OFF) TN_TRR(fyh[h][i], ya[4 * (h) + (i)], (OFF) + TNL_HI)
#define TN_FRAG(lo, hi) __builtin_bit_cast(bf16x8, (u32x4){(lo).x, (lo).y, (hi).x, (hi).y})
#define TN_WAIT(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); TN_SB
#define TN_MF(h, xb, i, j)                                                                                                                  \
    acc[4 * (h) + (i)][j] = TCOW_MFMA_16x16x32_H16(TN_FRAG(fxl[xb][j], fxh[xb][j]), TN_FRAG(fyl[h][i], fyh[h][i]), acc[4 * (h) + (i)][j], 0, 0, 0); TN_SB
#define TN_NOP do { } while (0)
    // block P of the step at byte offset OFF of the stage: 12 reads of block Q (X0, Y0 Y1 Y2 Y3, X1) are outstanding at most on entry
#define TN_BLK_P(xb, OFF)                                                                                                                   \
    do {                                                                                                                                    \
        TN_WAIT(8); TN_MF(0, xb, 0, 0); TN_RXL(xb, 2, OFF);                              /* X0, Y0 */                                        \
        TN_WAIT(7); TN_MF(0, xb, 1, 0); TN_RXH(xb, 2, OFF);                              /* Y1 */                                            \
        TN_WAIT(6); TN_MF(0, xb, 2, 0); TN_RXL(xb, 3, OFF);                              /* Y2 */                                            \
        TN_WAIT(5); TN_MF(0, xb, 3, 0); TN_RXH(xb, 3, OFF);                              /* Y3 */                                            \
        TN_WAIT(4); TN_MF(0, xb, 0, 1); TN_RYL(1, 0, OFF);                               /* X1: all of block Q's */                          \
        TN_MF(0, xb, 1, 1); TN_RYH(1, 0, OFF);                                                                                              \
        TN_MF(0, xb, 2, 1); TN_RYL(1, 1, OFF);                                                                                              \
        TN_MF(0, xb, 3, 1); TN_RYH(1, 1, OFF);                                                                                              \
        TN_WAIT(6); TN_MF(0, xb, 0, 2); TN_RYL(1, 2, OFF);                               /* X2: 2 of this block's 8 */                       \
        TN_MF(0, xb, 1, 2); TN_RYH(1, 2, OFF);                                                                                              \
        TN_MF(0, xb, 2, 2); TN_RYL(1, 3, OFF);                                                                                              \
        TN_MF(0, xb, 3, 2); TN_RYH(1, 3, OFF);                                                                                              \
        TN_WAIT(8); TN_MF(0, xb, 0, 3);                                                  /* X3: 4 of this block's 12 */                      \
        TN_MF(0, xb, 1, 3); TN_MF(0, xb, 2, 3); TN_MF(0, xb, 3, 3);                                                                         \
    } while (0)
    // block Q: block P's 12 reads (X2, X3, Y0 Y1 Y2 Y3 of FY[1]) are outstanding at most on entry.  NOFF: byte offset of the NEXT step from the
    // stage that ya / xa point to; nb: the FX set of that step; L0 ... L7: the load slots, behind every second MFMA.
#define TN_BLK_Q(xb, nb, NOFF, L0, L1, L2, L3, L4, L5, L6, L7)                                                                              \
    do {                                                                                                                                    \
        TN_WAIT(6); TN_MF(1, xb, 0, 0); TN_RXL(nb, 0, NOFF);                             /* X2, X3, Y0 */                                    \
        TN_WAIT(5); TN_MF(1, xb, 1, 0); TN_RXH(nb, 0, NOFF); L0; TN_SB;                  /* Y1 */                                            \
        TN_WAIT(4); TN_MF(1, xb, 2, 0); TN_RYL(0, 0, NOFF);                              /* Y2 */                                            \
        TN_WAIT(3); TN_MF(1, xb, 3, 0); TN_RYH(0, 0, NOFF); L1; TN_SB;                   /* Y3: all of block P's */                          \
        TN_MF(1, xb, 0, 1); TN_RYL(0, 1, NOFF);                                                                                             \
        TN_MF(1, xb, 1, 1); TN_RYH(0, 1, NOFF); L2; TN_SB;                                                                                  \
        TN_MF(1, xb, 2, 1); TN_RYL(0, 2, NOFF);                                                                                             \
        TN_MF(1, xb, 3, 1); TN_RYH(0, 2, NOFF); L3; TN_SB;                                                                                  \
        TN_MF(1, xb, 0, 2); TN_RYL(0, 3, NOFF);                                                                                             \
        TN_MF(1, xb, 1, 2); TN_RYH(0, 3, NOFF); L4; TN_SB;                                                                                  \
        TN_MF(1, xb, 2, 2); TN_RXL(nb, 1, NOFF);                                                                                            \
        TN_MF(1, xb, 3, 2); TN_RXH(nb, 1, NOFF); L5; TN_SB;                                                                                 \
        TN_MF(1, xb, 0, 3); TN_MF(1, xb, 1, 3); L6; TN_SB;                                                                                  \
        TN_MF(1, xb, 2, 3); TN_MF(1, xb, 3, 3); L7; TN_SB;                                                                                  \
    } while (0)

    if (nmt > 0) {       // what block Q of a stage before the first would have issued
        TN_RXL(0, 0, 0); TN_RXH(0, 0, 0);
        TN_RYL(0, 0, 0); TN_RYH(0, 0, 0); TN_RYL(0, 1, 0); TN_RYH(0, 1, 0); TN_RYL(0, 2, 0); TN_RYH(0, 2, 0); TN_RYL(0, 3, 0); TN_RYH(0, 3, 0);
        TN_RXL(0, 1, 0); TN_RXH(0, 1, 0);
    }
    for (int it = 0; it < nmt; ++it) {
        const int stage = it & 1;
        const uint32_t so = (uint32_t)stage * T2_STAGE;
        const char* sy = smem + stage * T2_STAGE;
        TN_BLK_P(0, 0);
        TN_BLK_Q(0, 1, STEPB, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP);
        TN_BLK_P(1, STEPB);
        TN_COLSUM(sy)
        // this wave's loads of stage it+1 (requested a whole stage ago) have landed, its reads of this stage are back (the fourth block's
        // fragments are in registers): behind the barrier the buffer of this stage is free and stage it+1 is visible
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        {
            const uint32_t flip = stage ? (uint32_t)(-T2_STAGE) : (uint32_t)T2_STAGE;       // the read addresses move to the next stage
#pragma unroll
            for (int i = 0; i < 8; ++i) ya[i] += flip;
#pragma unroll
            for (int j = 0; j < 4; ++j) xa[j] += flip;
        }
        TN_SB;
        if constexpr (SCHED == 2) {
            const int mt2 = mbeg + (it + 2) * T2_MC;
            const bool more = it + 2 < nmt;
            const uint32_t dy = lds_base + so + wave * 4096, dx = dy + TNL_TILE;
            const uint32_t by = (uint32_t)((long)(mt2 + wave * 8) * p.ldy * 2), bx = (uint32_t)((long)(mt2 + wave * 8) * p.ldx * 2);
            const uint32_t yw0 = more ? yv0 : 0x80000000u, yw1 = more ? yv1 : 0x80000000u;     // (the per-lane offset is the range-checked one)
            const uint32_t xw0 = more ? xv0 : 0x80000000u, xw1 = more ? xv1 : 0x80000000u;
            const uint32_t ry = (uint32_t)(2 * p.ldy * 2), rx = (uint32_t)(2 * p.ldx * 2);
            TN_BLK_Q(1, 0, 0, TCOW_BUFFER_GLDS16(yw0, srd_y, by, dy), TCOW_BUFFER_GLDS16(xw0, srd_x, bx, dx), TCOW_BUFFER_GLDS16(yw1, srd_y, by + ry, dy + 1024),
                     TCOW_BUFFER_GLDS16(xw1, srd_x, bx + rx, dx + 1024), TCOW_BUFFER_GLDS16(yw0, srd_y, by + 2 * ry, dy + 2048), TCOW_BUFFER_GLDS16(xw0, srd_x, bx + 2 * rx, dx + 2048),
                     TCOW_BUFFER_GLDS16(yw1, srd_y, by + 3 * ry, dy + 3072), TCOW_BUFFER_GLDS16(xw1, srd_x, bx + 3 * rx, dx + 3072));
        } else {
            if (it + 2 < nmt) issue_stage(it + 2, stage);
            TN_SB;
            TN_BLK_Q(1, 0, 0, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP, TN_NOP);
        }
    }
    // (The last stage's fourth block has requested fragments of a stage that does not exist into X0, X1 of set 0 and FY[0].  The wait re-defines those
    // registers, so that hipcc -- which knows nothing of reads issued by asm statements -- cannot hand them to the code behind the loop before the
    // data is in: see the same note in gemm_nt_c2.hip, where exactly that corrupted tiles)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(fxl[0][0]), "+v"(fxl[0][1]), "+v"(fxh[0][0]), "+v"(fxh[0][1]), "+v"(fyl[0][0]), "+v"(fyl[0][1]), "+v"(fyl[0][2]), "+v"(fyl[0][3]),
                   "+v"(fyh[0][0]), "+v"(fyh[0][1]), "+v"(fyh[0][2]), "+v"(fyh[0][3])
                 :: "memory");
    __builtin_amdgcn_sched_barrier(0);
#undef TN_BLK_Q
#undef TN_BLK_P
#undef TN_NOP
#undef TN_MF
#undef TN_WAIT
#undef TN_FRAG
#undef TN_RYH
#undef TN_RYL
#undef TN_RXH
#undef TN_RXL
#undef TN_TRR
#undef TN_SB
#undef TN_COLSUM
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

    // slab store: a lane's four accumulators of a block are four consecutive k of one n -- 16 bytes, 32 stores per wave.  (K is a multiple of 8,
    // so a piece of four is whole or absent; SCHED = 2 has whole tiles only.  A slab that is not 16-byte aligned gets the same values one by one.)
    float* out = p.slab + (size_t)z * p.N * p.K;
    const int ln = lane & 15, lk = 4 * (lane >> 4);
    auto store = [&](auto vec) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gn = n0 + wm * 128 + i * 16 + ln;
            if (SCHED != 2 && gn >= p.N) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gk = k0 + wn * 64 + j * 16 + lk;
                if (SCHED != 2 && gk >= p.K) continue;
                float* dst = out + (size_t)gn * p.K + gk;
                if constexpr (decltype(vec)::value) *reinterpret_cast<f32x4*>(dst) = acc[i][j];
                else { dst[0] = acc[i][j][0]; dst[1] = acc[i][j][1]; dst[2] = acc[i][j][2]; dst[3] = acc[i][j][3]; }
            }
        }
    };
    if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) store(std::true_type{}); else store(std::false_type{});
}

template <int SCHED>
__global__ __launch_bounds__(512, 2) void gemm_tn_bf16_256_kernel(TnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    tn256_body<SCHED>(p, xcd_remap(blockIdx.x, gridDim.x), smem);
}

// Grouped launch: the weight gradients of ONE transformer block (7 Linear layers, 153 tiles of 256 x 256 at ViT-B) or of several as one grid.  Launched
// one by one, a 768 x 768 weight has 9 tiles and needs 28 token slices to fill the chip -- 66 MB of f32 partials written and read back per GEMM (11.5 GB
// per training step), a fold launch each, and a ramp / tail per launch; together a block's tiles fill three rounds with FIVE slices (gemm_tn_plan.h).
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
