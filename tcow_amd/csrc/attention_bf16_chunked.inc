// 16-bit MFMA attention, chunked family (sequences of ANY length; overview in attention_bf16.hip): a 256-thread workgroup owns 4 query tiles
// (forward, dQ) or 4 key tiles (dK / dV) of one (sequence, head), one per wave, and walks the other side in chunks of CH tiles staged in LDS.
// The kernels keep the name *_stream of their first version; the streaming-INFERENCE cache kernels are attention_stream.hip.
// Part of the translation unit attention_bf16.hip, which includes this file after attention_common.h and attention_tiles.h.
namespace {

// ------------------------------------------------------------------------------------------------ forward
// Wave w loads K/V tile 4c+w of chunk c; 32 KiB of LDS -> 4 workgroups per CU.  K/V are re-read from L2 by the ceil(nt/4) workgroups of a
// sequence (placement: stream_work, attention_common.h).
template <int CH>
__global__ __launch_bounds__(256, 2) void attn_fwd_stream(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) char smem[2 * CH * TILE_B];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const StreamWork sw_ = stream_work(sd.n_outer * sd.n_inner * sd.heads, (nt + 3) / 4);
    if (!sw_.valid) return;
    const int item = sw_.pair / sd.heads, head = sw_.pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3;
    const bf16_t* qh = qkv + base * ld3 + head * ATT_HD;
    char* kt = smem;
    char* vt = smem + CH * TILE_B;
    // the first K / V chunk is requested before anything else: its flight covers the query-fragment loads below
    load_chunk2<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, 0, nt, sd.L, kt, vt, wave, lane);
    const int qt = sw_.chunk * 4 + wave;
    const bool active = qt < nt;
    const int q = 32 * qt + l31;
    const int qc = q < sd.L ? q : sd.L - 1;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = frag_row_global(qh, pse, qc, ks, hi);
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m = -1e30f, l = 0.f;
    const int kt_end = (!active) ? 0 : causal_key_tiles(sd, nt, qt);
    const int kt_end_wg = causal_key_tiles(sd, nt, sw_.chunk * 4 + 3);          // key tiles any wave of this workgroup needs
    for (int c0 = 0; c0 < kt_end_wg; c0 += CH) {
        if (c0) {
            __syncthreads();                               // previous chunk fully consumed
            load_chunk2<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, c0, nt, sd.L, kt, vt, wave, lane);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int jend = (c0 + CH < kt_end) ? c0 + CH : kt_end;
        for (int j = c0; j < jend; ++j) fwd_tile(sd, kt + (j - c0) * TILE_B, vt + (j - c0) * TILE_B, qf, j, qt, q, l31, hi, lane, m, l, o0, o1);
    }
    if (active) fwd_store(sd, base, head, q, hi, m, l, o0, o1, out, lse);
}

// The streaming forward for sequences WITHOUT a causal mask (spatial / joint attention: every call of the training step), on a VALU diet.  The
// streaming kernel above is VALU-throughput-bound at its 2.6-4 waves per SIMD (profiles/r05_attn_fwd_p4.txt: at d = 64 a tile step's softmax
// costs more issue cycles than its 8 MFMAs), so what counts is the number of vector instructions per step -- 87 in fwd_tile:
//   * Q is multiplied by 0.125 log2(e) ONCE, when its fragments are loaded (16-bit result: the scores see one more rounding of q, the saved
//     log-sum-exp stays consistent with the probabilities the forward used), so the exponent needs no scaling;
//   * the running reference maximum sits in the C operand of the first S MFMA -- S' = K Q'^T - m comes out of the matrix pipe and
//     p = exp2(S') is one instruction per element (fwd_tile: one fma + one exp);
//   * no mask arithmetic except on the sequence's last key tile (padding keys).
// (Walking a chunk's tiles by an unrolled loop -- fragment addresses as lane constant + immediate -- was tried: hipcc then carries the accumulators through
// 50 register copies per step and needs 202 registers, one wave per SIMD less.)
// The lazy maximum is fwd_tile's: the reference moves only when some row grew by more than 2^8, and the first key tile always sets it.
__device__ __forceinline__ void fwd_tile_pre(const char* ktile, const char* vtile, const bf16x8 (&qf)[4], bool first, bool pad, bool half, int lr, int l31, int hi, int lane,
                                             float& m, float& l, f32x16& negm, f32x16& o0, f32x16& o1) {
    f32x16 s = TCOW_MFMA_32x32x16_H16(frag_row(ktile, l31, 0, hi), qf[0], negm, 0, 0, 0);      // (negm = 0 until the first key tile has set the reference)
#pragma unroll
    for (int ks = 1; ks < 4; ++ks) s = TCOW_MFMA_32x32x16_H16(frag_row(ktile, l31, ks, hi), qf[ks], s, 0, 0, 0);
    if (pad) {                                              // the sequence's last key tile: padding keys underflow to probability 0
        TCOW_NO_IFCVT();
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = (crow32(r, hi) >= lr) ? -1e30f : s[r];
    }
    float mx = fmaxf(fmaxf(s[0], s[1]), s[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, s[r]), s[r + 1]);
    mx = half_max(fmaxf(mx, s[15]));                        // row maximum of this tile, relative to the reference
    if (first || __any(mx > 8.0f)) {
        TCOW_NO_IFCVT();
        const float delta = first ? mx : fmaxf(mx, 0.0f);   // (the first tile SETS the reference, later ones only raise it)
        const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);       // (first tile: l = O = 0)
        m += delta;
        l *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; s[r] -= delta; negm[r] = -m; }
    }
    // `half`: the sequence's last key tile when at most 16 of its keys exist (S = 301: 13).  Keys 0..15 of a tile are registers 0..7 of the S^T
    // accumulator (crow32(r, hi) = 8 (r >> 2) + 4 hi + (r & 3)) and contraction slots 0..15 of the P V product: registers 8..15 are padding (probability
    // exactly 0), so their exponentials and the second k-step of both P V MFMAs are skipped -- half the softmax arithmetic and 6 instead of 8 MFMAs.
    float p[16];
    float pa = 0.f, pb = 0.f;
#pragma unroll
    for (int r = 0; r < 8; r += 2) { p[r] = __builtin_amdgcn_exp2f(s[r]); p[r + 1] = __builtin_amdgcn_exp2f(s[r + 1]); pa += p[r]; pb += p[r + 1]; }
    const bf16x8 pb0 = pack8(p);
    o0 = TCOW_MFMA_32x32x16_H16(frag_tr(vtile, 0, 0, lane), pb0, o0, 0, 0, 0);
    o1 = TCOW_MFMA_32x32x16_H16(frag_tr(vtile, 0, 1, lane), pb0, o1, 0, 0, 0);
    if (!half) {
        TCOW_NO_IFCVT();
#pragma unroll
        for (int r = 8; r < 16; r += 2) { p[r] = __builtin_amdgcn_exp2f(s[r]); p[r + 1] = __builtin_amdgcn_exp2f(s[r + 1]); pa += p[r]; pb += p[r + 1]; }
        const bf16x8 pb1 = pack8(p + 8);
        o0 = TCOW_MFMA_32x32x16_H16(frag_tr(vtile, 1, 0, lane), pb1, o0, 0, 0, 0);
        o1 = TCOW_MFMA_32x32x16_H16(frag_tr(vtile, 1, 1, lane), pb1, o1, 0, 0, 0);
    }
    l += pa + pb;
}

// Work placement of attn_fwd_stream_nc.  PACK = false: stream_work (a sequence's ceil(nt / 4) workgroups back to back on one XCD).  PACK = true, for
// nt % 4 == 2 (S = 301: ten query tiles = 4 + 4 + 2): the third workgroup of a (frame, head) would run with two idle waves -- a sixth of the wave
// slots of a kernel whose throughput is set by how many waves a SIMD has to switch between.  Two sequences that follow each other on an XCD (pairs p
// and p + 8) form a group of 2 (nt / 4) + 1 workgroups: the full ones of each, and ONE mixed workgroup whose waves 0-1 take the two remaining query
// tiles of the first sequence and waves 2-3 those of the second; it walks the keys two tiles at a time (wave w stages tile c0 + (w & 1) of ITS
// sequence: the same 32 KiB of LDS).  An odd sequence out at the end of an XCD's list keeps the ordinary mapping.
struct NcWork { int pair, qt; bool mixed, valid; };
template <bool PACK>
__device__ __forceinline__ NcWork nc_work(int pairs, int nt, int wave) {
    NcWork w; w.mixed = false;
    if (!PACK) {
        const StreamWork sw_ = stream_work(pairs, (nt + 3) / 4);
        w.pair = sw_.pair; w.qt = sw_.chunk * 4 + wave; w.valid = sw_.valid;
        return w;
    }
    const int nfull = nt >> 2, G = 2 * nfull + 1;
    const int x = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int ngr = ((pairs + 7) >> 3) >> 1;                 // groups of two per XCD list
    int lp, chunk;
    if (k < ngr * G) {
        const int g = k / G, slot = k - g * G;
        if (slot < nfull) { lp = 2 * g; chunk = slot; }
        else if (slot < 2 * nfull) { lp = 2 * g + 1; chunk = slot - nfull; }
        else { w.mixed = true; lp = 2 * g + (wave >> 1); chunk = nfull; }
    } else { lp = 2 * ngr; chunk = k - ngr * G; }
    w.pair = 8 * lp + x; w.valid = w.pair < pairs;
    w.qt = w.mixed ? 4 * nfull + (wave & 1) : 4 * chunk + wave;
    return w;
}
static inline int nc_grid(int pairs, int nt, bool pack) {
    if (!pack) return stream_grid(pairs, (nt + 3) / 4);
    const int npl = (pairs + 7) >> 3, nfull = nt >> 2;
    return 8 * ((npl >> 1) * (2 * nfull + 1) + (npl & 1) * (nfull + 1));
}

template <int CH, bool PACK>
__global__ __launch_bounds__(256, 2) void attn_fwd_stream_nc(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) char smem[2 * CH * TILE_B];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const NcWork nw = nc_work<PACK>(sd.n_outer * sd.n_inner * sd.heads, nt, wave);
    if (!nw.mixed && !nw.valid) return;                    // (a mixed workgroup whose second sequence does not exist keeps its waves for the barriers ...
    const int pair = nw.valid ? nw.pair : 0;               //  ... and must not form addresses from a sequence index past the end: it reads sequence 0's query rows, no more)
    const int item = pair / sd.heads, head = pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3;
    const bf16_t* qh = qkv + base * ld3 + head * ATT_HD;
    char* kt = smem;
    char* vt = smem + CH * TILE_B;
    const bool mixed = PACK && nw.mixed;
    auto load_pair_tiles = [&](int c0) {                   // mixed workgroup: K / V tile c0 + (wave & 1) of this wave's sequence into slot `wave`
        if (nw.valid) {
            load_tile(qh + sd.D, pse, 32 * (c0 + (wave & 1)), sd.L, kt + wave * TILE_B, lane);
            load_tile(qh + 2 * sd.D, pse, 32 * (c0 + (wave & 1)), sd.L, vt + wave * TILE_B, lane);
        }
    };
    if (mixed) load_pair_tiles(0);
    else load_chunk2<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, 0, nt, sd.L, kt, vt, wave, lane);
    const int qt = nw.qt;
    const bool active = nw.valid && qt < nt;
    const int q = 32 * qt + l31;
    const int qc = q < sd.L ? q : sd.L - 1;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        typedef __attribute__((ext_vector_type(8))) float f32x8;
        qf[ks] = __builtin_convertvector(__builtin_convertvector(frag_row_global(qh, pse, qc, ks, hi), f32x8) * (kScale * kLog2e), bf16x8);
    }
    f32x16 o0, o1, negm;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; negm[r] = 0.f; }
    float m = 0.f, l = 0.f;
    const int lr = sd.L - 32 * (nt - 1);                    // valid keys of the last tile
    const bool pad = lr < 32, half_last = lr <= 16;
    const int step = mixed ? 2 : CH, slot0 = mixed ? (wave & 2) : 0;
    for (int c0 = 0; c0 < nt; c0 += step) {
        if (c0) {
            __syncthreads();                               // previous chunk fully consumed
            if (mixed) load_pair_tiles(c0);
            else load_chunk2<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, c0, nt, sd.L, kt, vt, wave, lane);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int jend = (c0 + step < nt) ? c0 + step : nt;
        if (active)
            for (int j = c0; j < jend; ++j)
                fwd_tile_pre(kt + (slot0 + j - c0) * TILE_B, vt + (slot0 + j - c0) * TILE_B, qf, j == 0, pad && j == nt - 1, half_last && j == nt - 1, lr, l31, hi, lane, m, l, negm,
                             o0, o1);
    }
    if (active) fwd_store(sd, base, head, q, hi, m, l, o0, o1, out, lse);
}

// ------------------------------------------------------------------------------------------------ backward
// Chunks of CH = 4 or 5 tiles in 32 / 40 KiB of LDS (load_chunk2: wave w loads tile 4c+w of the chunk, a fifth tile comes in quarters).
template <int CH>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_stream(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                           const float2* __restrict__ ld, bf16_t* __restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) char smem[2 * CH * TILE_B];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const StreamWork sw_ = stream_work(sd.n_outer * sd.n_inner * sd.heads, (nt + 3) / 4);
    if (!sw_.valid) return;
    const int item = sw_.pair / sd.heads, head = sw_.pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const bf16_t* qh = qkv + base * ld3 + head * ATT_HD;
    const bf16_t* doh = dout + base * sd.D + head * ATT_HD;
    const float2* ldh = ld + ((size_t)item * sd.heads + head) * (nt * 32);
    char* qt_ = smem;
    char* dot_ = smem + CH * TILE_B;
    const int j = sw_.chunk * 4 + wave;
    const bool active = j < nt;
    const int i0 = causal_first_query_tile(sd, j);                                // first query tile that can see this wave's keys
    const int c_start = (causal_first_query_tile(sd, sw_.chunk * 4) / CH) * CH;   // ... and the chunk of the first that sees any key of this workgroup
    // the first Q / dO chunk is requested before the K / V fragment loads: both latencies run together
    load_chunk2<CH>(qh, pse, doh, pso, c_start, nt, sd.L, qt_, dot_, wave, lane);
    const int key = 32 * j + l31;
    const int kc = key < sd.L ? key : sd.L - 1;
    bf16x8 kf[4], vf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { kf[ks] = frag_row_global(qh + sd.D, pse, kc, ks, hi); vf[ks] = frag_row_global(qh + 2 * sd.D, pse, kc, ks, hi); }
    f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
    for (int c0 = c_start; c0 < nt; c0 += CH) {
        if (c0 != c_start) {
            __syncthreads();
            load_chunk2<CH>(qh, pse, doh, pso, c0, nt, sd.L, qt_, dot_, wave, lane);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (active) {
            const int ib = c0 > i0 ? c0 : i0, ie = c0 + CH < nt ? c0 + CH : nt;
            for (int i = ib; i < ie; ++i) dkv_tile(sd, qt_ + (i - c0) * TILE_B, dot_ + (i - c0) * TILE_B, ldh, i, key, kf, vf, l31, hi, lane, dk0, dk1, dv0, dv1);
        }
    }
    if (active) dkv_store(sd, base, ld3, head, j, l31, hi, dk0, dk1, dv0, dv1, dqkv);
}

// (This kernel runs FIRST in the streaming backward: every wave owns a query tile, so it also computes delta = rowsum(dO * O) of
// its queries and publishes the packed (lse, delta) table that the dK / dV kernel reads -- no separate preparation launch.)
template <int CH>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_stream(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
                                                          const float* __restrict__ lse, float2* __restrict__ ld, bf16_t* __restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) char smem[2 * CH * TILE_B];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const StreamWork sw_ = stream_work(sd.n_outer * sd.n_inner * sd.heads, (nt + 3) / 4);
    if (!sw_.valid) return;
    const int item = sw_.pair / sd.heads, head = sw_.pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const bf16_t* qh = qkv + base * ld3 + head * ATT_HD;
    const bf16_t* doh = dout + base * sd.D + head * ATT_HD;
    float2* ldh = ld + ((size_t)item * sd.heads + head) * (nt * 32);
    char* kt = smem;
    char* vt = smem + CH * TILE_B;
    // the first K / V chunk is requested before the Q / dO / O fragment loads and the delta sums: both latencies run together
    load_chunk2<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, 0, nt, sd.L, kt, vt, wave, lane);
    const int qt = sw_.chunk * 4 + wave;
    const bool active = qt < nt;
    const int q = 32 * qt + l31;
    const int qc = q < sd.L ? q : sd.L - 1;
    bf16x8 qf[4], dof[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { qf[ks] = frag_row_global(qh, pse, qc, ks, hi); dof[ks] = frag_row_global(doh, pso, qc, ks, hi); }
    // delta of row q = sum_d dO * O: the dO fragments are already in registers (this half-wave's 32 of the 64 channels); O is
    // fetched with the same fragment pattern
    const bf16_t* oh = o + base * sd.D + head * ATT_HD;
    float part = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 of = frag_row_global(oh, pso, qc, ks, hi);
#pragma unroll
        for (int e = 0; e < 8; ++e) part = fmaf((float)of[e], (float)dof[ks][e], part);
    }
    const float dl = half_sum(part);
    const float lsn = lse[(base + (long)qc * sd.pos_stride) * sd.heads + head];
    if (active && hi == 0) ldh[32 * qt + l31] = q < sd.L ? make_float2(lsn * kLog2e, dl) : make_float2(0.f, 0.f);
    const float ls = lsn * kLog2e;
    f32x16 dq0, dq1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq0[r] = 0.f; dq1[r] = 0.f; }
    const int kt_end = (!active) ? 0 : causal_key_tiles(sd, nt, qt);
    const int kt_end_wg = causal_key_tiles(sd, nt, sw_.chunk * 4 + 3);
    for (int c0 = 0; c0 < kt_end_wg; c0 += CH) {
        if (c0) {
            __syncthreads();
            load_chunk2<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, c0, nt, sd.L, kt, vt, wave, lane);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int jend = (c0 + CH < kt_end) ? c0 + CH : kt_end;
        for (int j = c0; j < jend; ++j) dq_tile(sd, kt + (j - c0) * TILE_B, vt + (j - c0) * TILE_B, j, q, qf, dof, ls, dl, l31, hi, lane, dq0, dq1);
    }
    if (active) dq_store(sd, base, ld3, head, qt, l31, hi, dq0, dq1, dqkv);
}

}  // namespace

int tcow_attn_chunked_fwd(hipStream_t st, const SeqDesc& d, int nt, const void* qkv, void* out, float* lse) {
    const int pairs = d.n_outer * d.n_inner * d.heads;
    // (forward: four tiles per chunk -- with five, 40 KiB per workgroup, the fourth workgroup of a CU no longer fits and 56 us become 60)
    if (d.diag >= (1 << 27) && nt >= 2) {
        if (nt % 4 == 2) hipLaunchKernelGGL((attn_fwd_stream_nc<4, true>), dim3(nc_grid(pairs, nt, true)), dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (bf16_t*)out, lse);
        else hipLaunchKernelGGL((attn_fwd_stream_nc<4, false>), dim3(nc_grid(pairs, nt, false)), dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (bf16_t*)out, lse);
    }
    else hipLaunchKernelGGL(attn_fwd_stream<4>, dim3(stream_grid(pairs, cdiv(nt, 4))), dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (bf16_t*)out, lse);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// ch5: five tiles per LDS chunk instead of four.  ws: the (lse, delta) table that the dQ kernel writes for the dK / dV kernel
int tcow_attn_chunked_bwd(hipStream_t st, const SeqDesc& d, int nt, bool ch5, const void* qkv, const void* out, const void* dout, const float* lse, void* ws, void* dqkv) {
    float2* ld = (float2*)ws;
    const dim3 sg(stream_grid(d.n_outer * d.n_inner * d.heads, cdiv(nt, 4)));
    if (ch5) {
        hipLaunchKernelGGL(attn_bwd_dq_stream<5>, sg, dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, ld, (bf16_t*)dqkv);
        TCOW_CHECK_LAUNCH();
        hipLaunchKernelGGL(attn_bwd_dkv_stream<5>, sg, dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)dout, ld, (bf16_t*)dqkv);
    } else {
        hipLaunchKernelGGL(attn_bwd_dq_stream<4>, sg, dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, ld, (bf16_t*)dqkv);
        TCOW_CHECK_LAUNCH();
        hipLaunchKernelGGL(attn_bwd_dkv_stream<4>, sg, dim3(256), 0, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)dout, ld, (bf16_t*)dqkv);
    }
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
