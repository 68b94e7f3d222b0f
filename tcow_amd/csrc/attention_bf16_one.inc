// 16-bit MFMA attention, one-kernel spatial backward (workgroup-shared sequences of four to ten tiles; overview in attention_bf16.hip).
// Part of the translation unit attention_bf16.hip, which includes this file after attention_common.h and attention_tiles.h.
namespace {

// ONE kernel per (frame, head) (S <= 320).
// The two chunked backward kernels (attention_bf16_chunked.inc) visit every (query tile, key tile) pair twice -- once for dQ, once for dK / dV: 28 MFMAs per pair, the
// scores and dP recomputed, Q / K / V / dO read twice (HBM floor 82 us at configs[1]).  Here ONE 10-wave workgroup owns a (frame, head):
//   * wave w owns key tile w: K_w, V_w fragments from the LDS copies, dK_w / dV_w in 64 accumulator registers, for the whole kernel;
//   * the query side streams: Q_i / dO_i tiles through a double buffer (8 KiB per step, brought in by waves 0-7 one 1 KiB piece each);
//   * per query tile i every wave runs the dK / dV step (dkv_tile: S, dP, P, dS, dV += P^T dO, dK += dS^T Q -- 16 MFMAs) and writes its
//     32 x 32 dS block (bf16) into a [320 keys][32 queries] strip in LDS; after ONE barrier waves 0-7 form dQ_i^T = K^T dS_i in eight
//     16 x 16 output blocks, each a chain of nt v_mfma_16x16x32 over ALL keys (operands by transpose reads: K from its LDS copy, dS from the
//     strip) -- no partial sums across waves, no atomics; 20 MFMA-equivalents per pair instead of 28, every operand read once (floor 53 us).
//   The strip and the Q / dO buffers are double-buffered, so the dQ phase of step i runs while other waves are already in step i+1: one
//   barrier per step.  delta = rowsum(dO * O) and the log-sum-exp go into an LDS table in the prologue (wave w: query tile w).
// LDS: K 40 + V 40 + Q/dO 16 + strip 40 + table 2.5 = 138.5 KiB, one workgroup per CU; 168 VGPRs (three waves on two of the SIMDs).
constexpr int ONE_MAX_NT = 10;
constexpr int ONE_K = 0, ONE_V = ONE_MAX_NT * TILE_B, ONE_QDO = 2 * ONE_MAX_NT * TILE_B, ONE_STRIP = ONE_QDO + 4 * TILE_B;
constexpr int ONE_STRIP_B = ONE_MAX_NT * 32 * 64;                       // [320 keys][32 queries] bf16
constexpr int ONE_TAB = ONE_STRIP + 2 * ONE_STRIP_B, ONE_DQ = ONE_TAB + ONE_MAX_NT * 32 * 8, ONE_LDS = ONE_DQ + 2 * TILE_B;      // + two dQ staging tiles

__global__ __launch_bounds__(768) void attn_bwd_one_kernel(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
                                                           const float* __restrict__ lse, bf16_t* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int pair = blockIdx.x;
    const int item = pair / sd.heads, head = pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const bf16_t* qh = qkv + base * ld3 + head * ATT_HD;
    const bf16_t* doh = dout + base * sd.D + head * ATT_HD;
    const bf16_t* oh = o + base * sd.D + head * ATT_HD;
    char* ktiles = smem + ONE_K; char* vtiles = smem + ONE_V;
    float2* tab = reinterpret_cast<float2*>(smem + ONE_TAB);
    const bool owner = wave < nt;
    // (the third tile wave of a SIMD -- waves 8, 9 -- gets the issue slots last and is the one everybody waits for at the step barrier: priorities 2 / 1 / 0 for
    // waves 8-9 / 4-7 / 0-3 and the chain waves)
    if (wave >= 8 && wave < 10) __builtin_amdgcn_s_setprio(2); else if (wave >= 4 && wave < 8) __builtin_amdgcn_s_setprio(1);
    // ---- prologue: K_w / V_w tiles, the first two Q / dO tiles (a 1 KiB quarter per wave 0-7), the (lse, delta) table of query tile w
    if (owner) {
        load_tile<LD_NT>(qh + sd.D, pse, 32 * wave, sd.L, ktiles + wave * TILE_B, lane);
        load_tile<LD_NT>(qh + 2 * sd.D, pse, 32 * wave, sd.L, vtiles + wave * TILE_B, lane);
    }
    auto load_qdo = [&](int i, int buf) {                     // waves 0-3: quarter `wave` of Q_i, waves 4-7: quarter `wave - 4` of dO_i
        char* dst = smem + ONE_QDO + buf * (2 * TILE_B);
        if (wave < 4) load_tile_chunk<LD_NT>(qh, pse, 32 * i, sd.L, dst, wave, lane);
        else if (wave < 8) load_tile_chunk<LD_NT>(doh, pso, 32 * i, sd.L, dst + TILE_B, wave - 4, lane);
    };
    load_qdo(0, 0);
    if (nt > 1) load_qdo(1, 1);
    if (owner) {
        // delta_q = sum_d dO * O, 8 lanes per row (one 16-byte piece each: every load instruction takes 8 whole rows), three butterfly steps.
        // All nine loads of the wave are issued before the first use (in a loop hipcc waits for each row group's loads in turn: four
        // dependent round trips, 26 000 cycles of the prologue in the first timeline of this kernel).
        uint4 xo[4], yo[4]; float ls4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int q = 32 * wave + 8 * j + (lane >> 3); q = q < sd.L ? q : sd.L - 1;
            xo[j] = *reinterpret_cast<const uint4*>(oh + (long)q * pso + (lane & 7) * 8); yo[j] = *reinterpret_cast<const uint4*>(doh + (long)q * pso + (lane & 7) * 8);
            ls4[j] = lse[(base + (long)q * sd.pos_stride) * sd.heads + head];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = 32 * wave + 8 * j + (lane >> 3);
            const uint4 x = xo[j], y = yo[j];
            float part = bflo(x.x) * bflo(y.x) + bfhi(x.x) * bfhi(y.x) + bflo(x.y) * bflo(y.y) + bfhi(x.y) * bfhi(y.y)
                       + bflo(x.z) * bflo(y.z) + bfhi(x.z) * bfhi(y.z) + bflo(x.w) * bflo(y.w) + bfhi(x.w) * bfhi(y.w);
            part += __shfl_xor(part, 1, 64); part += __shfl_xor(part, 2, 64); part += __shfl_xor(part, 4, 64);
            if ((lane & 7) == 0) tab[q] = q < sd.L ? make_float2(ls4[j] * kLog2e, part) : make_float2(0.f, 0.f);
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();

    f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
    const int key = 32 * wave + l31;
    // dQ phase (waves 0-7): output block = queries 16 qb .. +15 x channels 16 db .. +15 of the step's tile, as dQ^T (lane: query l & 15,
    // channels 16 db + 4 (l >> 4) .. + 3).  Transpose-read addressing: in its 16-lane group lane 4 r + c supplies row r / 4-element quad c.
    // dQ phase: TWO MORE WAVES (10, 11 -- they land on the two SIMDs that host two key-tile waves, wave w sits on SIMD w % 4) do nothing else: behind
    // the barrier of step i they turn the strip into dQ_i^T while waves 0-9 are already in step i+1 -- the chains no longer sit between two tile
    // steps of the same wave (timeline in profiles/r04_ubench_valu.txt part F: a step cost tile arithmetic 2 700 + chains 2 600 + barrier wait).
    // Chain wave c = wave - 10 owns channel blocks 2c, 2c + 1 (16 channels each) x both query halves: four independent accumulate chains of nt
    // 16x16x32 MFMAs over all key tiles; K and strip fragments by transpose reads (in its 16-lane group lane 4 r + q supplies row r / quad q).
    // Output lane: query l & 15 (+ 16 for the second half), channels 16 db + 4 (l >> 4) .. + 3.
    const bool chain_wave = wave >= 10;
    const int cw = wave - 10;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(LDS_PTR(char))smem;
    // strip write of this wave's dS block: lane (key l31, hi) holds queries 4 hi + {0..3}, 8 + .., 16 + .., 24 + ..: four 8-byte quads (slots
    // hi, 2 + hi, 4 + hi, 6 + hi of the key's 64-byte row; slot s of key row k sits at s ^ ((k >> 1) & 7): a ds_write_b64 is served in groups of 16
    // consecutive lanes over 32 banks -- rows of equal parity share their banks, so the eight of a group must differ in the slot --, and the chain
    // waves' transpose reads in groups of 32 lanes over 64 banks: rows 8 g4 + tr, g4 = 0 / 1, must differ in bit 2 of the slot.  With k & 7, as in
    // round 4, rows k and k + 8 met on one bank in both: SQ_LDS_BANK_CONFLICT = 17 % of the LDS cycles, profiles/r04_pmc_attn.txt.)
    const uint32_t sw = lds0 + ONE_STRIP + (32 * wave + l31) * 64;
    const int k7 = (l31 >> 1) & 7;

    if (chain_wave) {
        // ---- the chain waves' own loop (a separate one: their 80 registers of K^T fragments must not be live across the tile-step code)
        typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
        typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
        const int g4 = lane >> 4, tr = (lane & 15) >> 2, tc = lane & 3;
        const int krow = 8 * g4 + tr;                                                        // key row inside a 32-key tile (second read: + 4)
        const int kchunk = 4 * cw + (tc >> 1);                                               // channel block 2 cw; block 2 cw + 1 = chunk + 2 = offset ^ 32
        const uint32_t ko0 = ONE_K + krow * 128 + ((kchunk ^ swz_g(krow)) << 4) + (tc & 1) * 8, ko1 = ONE_K + (krow + 4) * 128 + ((kchunk ^ swz_g(krow + 4)) << 4) + (tc & 1) * 8;
        const uint32_t so0 = ONE_STRIP + krow * 64 + ((tc ^ ((krow >> 1) & 7)) << 3);        // query half 0; half 1 = slot ^ 4 = offset ^ 32
        const uint32_t so1 = ONE_STRIP + (krow + 4) * 64 + ((tc ^ (((krow + 4) >> 1) & 7)) << 3);
        // K^T fragments of ALL key tiles, once: they are the same in every step (80 registers the tile-step waves do not have to spare)
        u32x2_ kfr[ONE_MAX_NT][4];
#pragma unroll
        for (int kt = 0; kt < ONE_MAX_NT; ++kt) {
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(kfr[kt][0]) : "v"(lds0 + ko0 + kt * TILE_B));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(kfr[kt][1]) : "v"(lds0 + ko1 + kt * TILE_B));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(kfr[kt][2]) : "v"(lds0 + (ko0 ^ 32u) + kt * TILE_B));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(kfr[kt][3]) : "v"(lds0 + (ko1 ^ 32u) + kt * TILE_B));
            if ((kt & 1) == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint32_t stg = lds0 + ONE_DQ + cw * TILE_B;
        for (int i = 0; i < nt; ++i) {
            const int buf = i & 1;
            __syncthreads();                                            // barrier of step i: the strip of step i is complete
            f32x4 acc[2][2];                                            // [channel block][query half]
#pragma unroll
            for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
                for (int b_ = 0; b_ < 2; ++b_) acc[a_][b_] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const uint32_t sa0 = lds0 + so0 + buf * ONE_STRIP_B, sa1 = lds0 + so1 + buf * ONE_STRIP_B;
            const uint32_t sb0 = lds0 + (so0 ^ 32u) + buf * ONE_STRIP_B, sb1 = lds0 + (so1 ^ 32u) + buf * ONE_STRIP_B;
            u32x2_ fr[3][4];                                            // per set: strip half 0 (2 reads), half 1 (2)
#define ONE_RD(set, kt_)                                                                                               \
            do {                                                                                                       \
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fr[set][0]) : "v"(sa0 + (kt_) * 2048));                \
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fr[set][1]) : "v"(sa1 + (kt_) * 2048));                \
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fr[set][2]) : "v"(sb0 + (kt_) * 2048));                \
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fr[set][3]) : "v"(sb1 + (kt_) * 2048));                \
            } while (0)
#define ONE_KF(kt_, j) __builtin_bit_cast(bf16x8, (u32x4_){kfr[kt_][2 * (j)].x, kfr[kt_][2 * (j)].y, kfr[kt_][2 * (j) + 1].x, kfr[kt_][2 * (j) + 1].y})
#define ONE_SF(set, j) __builtin_bit_cast(bf16x8, (u32x4_){fr[set][2 * (j)].x, fr[set][2 * (j)].y, fr[set][2 * (j) + 1].x, fr[set][2 * (j) + 1].y})
#define ONE_MF(set, kt_)                                                                                               \
            do {                                                                                                       \
                acc[0][0] = TCOW_MFMA_16x16x32_H16(ONE_KF(kt_, 0), ONE_SF(set, 0), acc[0][0], 0, 0, 0);                \
                acc[1][0] = TCOW_MFMA_16x16x32_H16(ONE_KF(kt_, 1), ONE_SF(set, 0), acc[1][0], 0, 0, 0);                \
                acc[0][1] = TCOW_MFMA_16x16x32_H16(ONE_KF(kt_, 0), ONE_SF(set, 1), acc[0][1], 0, 0, 0);                \
                acc[1][1] = TCOW_MFMA_16x16x32_H16(ONE_KF(kt_, 1), ONE_SF(set, 1), acc[1][1], 0, 0, 0);                \
            } while (0)
#define ONE_WAIT(set, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(fr[set][0]), "+v"(fr[set][1]), "+v"(fr[set][2]), "+v"(fr[set][3]) :: "memory")
            // (fully unrolled over the ten key tiles: the K fragments are register arrays; tiles past nt - 1 are skipped)
            ONE_RD(0, 0); ONE_RD(1, 1);
#pragma unroll
            for (int kt = 0; kt < ONE_MAX_NT; ++kt) {
                if (kt < nt) {
                    if (kt % 3 == 0) { ONE_RD(2, kt + 2); ONE_WAIT(0, 8); ONE_MF(0, kt); }
                    else if (kt % 3 == 1) { ONE_RD(0, kt + 2); ONE_WAIT(1, 8); ONE_MF(1, kt); }
                    else { ONE_RD(1, kt + 2); ONE_WAIT(2, 8); ONE_MF(2, kt); }
                }
            }
            // (the last key tiles have requested strip fragments two tiles past the end into the three sets: the wait re-defines them, so that hipcc -- which
            // knows nothing of reads issued by asm statements -- cannot reuse a register the late data will still land on; cf. gemm_nt_c2.hip)
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(fr[0][0]), "+v"(fr[0][1]), "+v"(fr[0][2]), "+v"(fr[0][3]), "+v"(fr[1][0]), "+v"(fr[1][1]), "+v"(fr[1][2]), "+v"(fr[1][3]),
                           "+v"(fr[2][0]), "+v"(fr[2][1]), "+v"(fr[2][2]), "+v"(fr[2][3])
                         :: "memory");
#undef ONE_WAIT
#undef ONE_RD
#undef ONE_MF
#undef ONE_KF
#undef ONE_SF
            // the wave's half of the dQ tile ([32 q][channels 32 cw .. + 31]) through its PRIVATE staging tile (a wave's LDS operations complete in
            // order: no barrier), then out as 64-byte row pieces: 16-byte chunk c of row q sits at position c ^ (q & 7) of the row's 128 bytes
#pragma unroll
            for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
                for (int b_ = 0; b_ < 2; ++b_) {
                    const int ql = 16 * b_ + (lane & 15), slot = 4 * (2 * cw + a_) + g4;      // 8-byte slot of the row: channels 4 slot .. + 3
                    const uint32_t da = stg + ql * 128 + (((slot >> 1) ^ (ql & 7)) << 4) + ((slot & 1) << 3);
                    const u32x2_ pk = {pack_bf2(acc[a_][b_][0] * kScale, acc[a_][b_][1] * kScale), pack_bf2(acc[a_][b_][2] * kScale, acc[a_][b_][3] * kScale)};
                    asm volatile("ds_write_b64 %0, %1" :: "v"(da), "v"(pk) : "memory");
                }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int r = 16 * j + (lane >> 2), c = 4 * cw + (lane & 3);
                u32x4_ v;
                asm volatile("s_waitcnt lgkmcnt(0)\n\tds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(stg + r * 128 + ((c ^ (r & 7)) << 4)) : "memory");
                const int q = 32 * i + r;
                if (q < sd.L) *reinterpret_cast<u32x4_*>(dqkv + (base + (long)q * sd.pos_stride) * ld3 + head * ATT_HD + c * 8) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();                                                // (the owners' final barrier: the K / V tiles become their staging space)
        return;
    }

    for (int i = 0; i < nt; ++i) {
        const int buf = i & 1;
        const char* qtile = smem + ONE_QDO + buf * (2 * TILE_B);
        const char* dotile = qtile + TILE_B;
        if (owner) {
            bf16x8 kf[4], vf[4], dsb[2];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) { kf[ks] = frag_row(ktiles + wave * TILE_B, l31, ks, hi); vf[ks] = frag_row(vtiles + wave * TILE_B, l31, ks, hi); }
            dkv_tile(sd, qtile, dotile, tab, i, key, kf, vf, l31, hi, lane, dk0, dk1, dv0, dv1, dsb);
            typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
            typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
            const u32x4_ w0 = __builtin_bit_cast(u32x4_, dsb[0]), w1 = __builtin_bit_cast(u32x4_, dsb[1]);
            const uint32_t sb = sw + buf * ONE_STRIP_B;
            asm volatile("ds_write_b64 %0, %1" :: "v"(sb + ((hi ^ k7) << 3)), "v"((u32x2_){w0.x, w0.y}) : "memory");
            asm volatile("ds_write_b64 %0, %1" :: "v"(sb + (((2 + hi) ^ k7) << 3)), "v"((u32x2_){w0.z, w0.w}) : "memory");
            asm volatile("ds_write_b64 %0, %1" :: "v"(sb + (((4 + hi) ^ k7) << 3)), "v"((u32x2_){w1.x, w1.y}) : "memory");
            asm volatile("ds_write_b64 %0, %1" :: "v"(sb + (((6 + hi) ^ k7) << 3)), "v"((u32x2_){w1.z, w1.w}) : "memory");
        }
        // this wave's piece of tile i+1 has landed, its LDS traffic of this step is done: behind the barrier the strip of step i is complete,
        // tile i+1 is visible and buffer `buf` may take tile i+2
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (i + 2 < nt) load_qdo(i + 2, buf);
    }
    // dK / dV as whole rows through the waves' own K / V tiles (dead once the chain waves have passed this barrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (owner) {
        bf16_t* drow0 = dqkv + (base + (long)(32 * wave) * sd.pos_stride) * ld3 + head * ATT_HD;
        store_tile_staged(lds0 + ONE_K + wave * TILE_B, lane, kScale, dk0, dk1, drow0 + sd.D, pse, sd.L - 32 * wave);      // dS was accumulated without its 1/sqrt(d) factor
        store_tile_staged(lds0 + ONE_V + wave * TILE_B, lane, 1.0f, dv0, dv1, drow0 + 2 * sd.D, pse, sd.L - 32 * wave);
    }
}

}  // namespace

int tcow_attn_one_bwd(hipStream_t st, const SeqDesc& d, int nt, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv) {
    tcow_ensure_lds((const void*)attn_bwd_one_kernel, ONE_LDS);
    hipLaunchKernelGGL(attn_bwd_one_kernel, dim3(d.n_outer * d.n_inner * d.heads), dim3(768), ONE_LDS, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
