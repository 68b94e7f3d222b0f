// Flash attention of the f32-storage mode precision='bf16x3' on the bf16 matrix cores: softmax(q k^T * d^-0.5 [causal mask]) v (vit.py:88-109) with every
// matrix product formed as THREE bf16 MFMAs on hi / lo operand splits, exactly as gemm_x3.hip does for the Linear layers (attention_tiles.h, SplitOp).
// Until round 6 the mode ran its attention on the exact-f32 MFMA (attention_f32.hip: 1/16 of the bf16 rate): 1 499 us per spatial forward at configs[1], a fifth
// of that mode's step.  Same contract as attention_f32.hip (f32 qkv [rows, 3D] in, f32 out / dqkv, natural-log LSE, delta workspace in the lse layout).
//
// Structure = the kernels of attention_bf16_chunked.inc: a 256-thread workgroup owns 4 query (forward, dQ) or 4 key (dK / dV) tiles of one (sequence, head),
// one per wave, and walks the other side in chunks of CH tiles.  The forward step of one tile against another IS attention_tiles.h's fwd_tile, called with
// the split operand policy: softmax statistics, masks, the lazy running maximum and the accumulation order are stated there, once.  The two backward
// steps stand here, written on that header's helpers (fragments, split, product, half-wave exchange, row store): see the comment above attn_x3_bwd_dkv.
// What this file holds is what the f32 storage needs around those steps:
//   staging     a chunk is read as f32 by all 256 threads (one 8-element piece of a row per thread and tile: two 16-byte loads), split ONCE in registers and
//               stored as two [32][64] bf16 LDS tiles (hi, lo) in the layout of attention_tiles.h; arrays [a hi][a lo][b hi][b lo], CH tiles each (x_stage),
//               or one such set per wave in the one-tile SOLO kernels (x_stage_wave)
//   xfrag_global  the wave's own rows (Q, dO or K, V), split when their fragments are loaded
//   delta       rowsum(dO * O) in f32, from the unsplit dO
//   the launchers with the CH / SOLO choices and what they measured.
// MFMAs per (query tile, key tile) pair: forward 24, dQ 36, dK / dV 48 (bf16 mode: 8 / 12 / 16).
#include <stdlib.h>

#include "attention_tiles.h"

namespace {

constexpr float kLn2 = 0.6931471805599453f;
typedef SplitOp P;          // the operand policy of every kernel here

// tile t of a staged source whose hi plane starts at `hi_plane`; the lo plane follows CH tiles later
template <int CH>
__device__ __forceinline__ SplitOp::Tile x_tile(const char* hi_plane, int t) { return {hi_plane + t * TILE_B, hi_plane + (CH + t) * TILE_B}; }

// ---- staging: tile = rows p0 .. p0+31 (clamped to L-1: padding rows hold finite data, masks / zero probabilities keep them out) of a 64-column f32 block.
// Thread t of the 256: row t >> 3, columns 8 (t & 7) .. + 7.
struct XItem { f32x4 a, b; };
__device__ __forceinline__ XItem x_load(const float* __restrict__ src, long stride, int p0, int L, int tid) {
    int pos = p0 + (tid >> 3); pos = pos < L ? pos : L - 1;
    const float* p = src + (size_t)pos * stride + 8 * (tid & 7);
    XItem it; it.a = *reinterpret_cast<const f32x4*>(p); it.b = *reinterpret_cast<const f32x4*>(p + 4);
    return it;
}
__device__ __forceinline__ void x_store_rc(const XItem& it, char* hi_tile, char* lo_tile, int r, int c);
__device__ __forceinline__ void x_store(const XItem& it, char* hi_tile, char* lo_tile, int tid) { x_store_rc(it, hi_tile, lo_tile, tid >> 3, tid & 7); }
__device__ __forceinline__ void x_store_rc(const XItem& it, char* hi_tile, char* lo_tile, int r, int c) {
    xu4 h, l;
    const float v[8] = {it.a[0], it.a[1], it.a[2], it.a[3], it.b[0], it.b[1], it.b[2], it.b[3]};
    xsplit8u(v, h, l);
    const int off = r * 128 + ((c ^ swz_g(r)) << 4);
    *reinterpret_cast<xu4*>(hi_tile + off) = h;
    *reinterpret_cast<xu4*>(lo_tile + off) = l;
}
// tiles c0 .. c0+CH-1 (those below `nt_end`) of two row sources a, b -> LDS arrays [a hi][a lo][b hi][b lo], CH tiles each.  All loads are issued before the
// first split (16 CH registers in flight).
template <int CH>
__device__ __forceinline__ void x_stage(const float* __restrict__ a, long sa, const float* __restrict__ b, long sb, int c0, int nt_end, int L, char* smem, int tid) {
    XItem ia[CH], ib[CH];
#pragma unroll
    for (int t = 0; t < CH; ++t)
        if (c0 + t < nt_end) { ia[t] = x_load(a, sa, 32 * (c0 + t), L, tid); ib[t] = x_load(b, sb, 32 * (c0 + t), L, tid); }
#pragma unroll
    for (int t = 0; t < CH; ++t)
        if (c0 + t < nt_end) {
            x_store(ia[t], smem + t * TILE_B, smem + (CH + t) * TILE_B, tid);
            x_store(ib[t], smem + (2 * CH + t) * TILE_B, smem + (3 * CH + t) * TILE_B, tid);
        }
}

// SOLO kernels (one-tile sequences, temporal attention): every WAVE owns its own (sequence, head) and stages the one tile of each source itself -- row (lane >> 3) + 8 pass,
// columns 8 (lane & 7) .. + 7, four passes per tile -- into wave-private LDS; no workgroup barrier (a wave's LDS operations execute in order).
__device__ __forceinline__ void x_stage_wave(const float* __restrict__ a, long sa, const float* __restrict__ b, long sb, int L, char* wsm, int lane) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {               // two rounds of 16 rows: 32 registers of loads in flight instead of 64 (the SOLO kernels hold their own fragments too)
        XItem ia[2], ib[2];
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) { ia[ps] = x_load(a, sa, 16 * half + 8 * ps, L, lane); ib[ps] = x_load(b, sb, 16 * half + 8 * ps, L, lane); }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            x_store_rc(ia[ps], wsm, wsm + TILE_B, 16 * half + 8 * ps + (lane >> 3), lane & 7);
            x_store_rc(ib[ps], wsm + 2 * TILE_B, wsm + 3 * TILE_B, 16 * half + 8 * ps + (lane >> 3), lane & 7);
        }
        asm volatile("" ::: "memory");                   // (keeps hipcc from issuing the second round's loads with the first)
    }
}

// the wave's own row (position pos of a 64-column f32 block), split: fragment ks = columns 16 ks + 8 hi .. + 7
__device__ __forceinline__ void xfrag_global(const float* __restrict__ row, int hi, SplitOp::Frag (&f)[4], float* keep = nullptr) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(row + 16 * ks + 8 * hi), b = *reinterpret_cast<const f32x4*>(row + 16 * ks + 8 * hi + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        f[ks] = SplitOp::pack(v);
        if (keep) {
#pragma unroll
            for (int e = 0; e < 8; ++e) keep[8 * ks + e] = v[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int CH, bool SOLO = false>
__global__ __launch_bounds__(256, 2) void attn_x3_fwd(SeqDesc sd, int nt, const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) char smem_[];          // [K hi][K lo][V hi][V lo], CH tiles each (SOLO: one such set per wave)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    StreamWork w = stream_work(sd.n_outer * sd.n_inner * sd.heads, (nt + 3) / 4);
    if (SOLO) { w.pair = blockIdx.x * 4 + wave; w.chunk = 0; w.valid = w.pair < sd.n_outer * sd.n_inner * sd.heads; }
    if (!w.valid) return;
    char* smem = SOLO ? smem_ + wave * (4 * TILE_B) : smem_;
    const int item = w.pair / sd.heads, head = w.pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3;
    const float* qh = qkv + base * ld3 + head * ATT_HD;
    const int qt = SOLO ? 0 : w.chunk * 4 + wave;
    const bool active = qt < nt;
    const int q = 32 * qt + l31, qc = q < sd.L ? q : sd.L - 1;
    if (SOLO) x_stage_wave(qh + sd.D, pse, qh + 2 * sd.D, pse, sd.L, smem, lane);      // (before the wave's own fragments are loaded: the staging registers are dead by then)
    SplitOp::Frag qf[4];
    xfrag_global(qh + (size_t)qc * pse, hi, qf);
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m = -1e30f, l = 0.f;
    const int kt_end = (!active) ? 0 : causal_key_tiles(sd, nt, qt);
    const int kt_end_wg = causal_key_tiles(sd, nt, w.chunk * 4 + 3);          // key tiles any wave of this workgroup needs
    for (int c0 = 0; c0 < kt_end_wg; c0 += CH) {
        if (!SOLO) {
            __syncthreads();                                               // previous chunk fully consumed
            x_stage<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, c0, kt_end_wg, sd.L, smem, tid);
            __syncthreads();
        }
        const int jend = (c0 + CH < kt_end) ? c0 + CH : kt_end;
        for (int j = c0; j < jend; ++j)
            fwd_tile<SplitOp>(sd, x_tile<CH>(smem, j - c0), x_tile<CH>(smem + 2 * CH * TILE_B, j - c0), qf, j, qt, q, l31, hi, lane, m, l, o0, o1);
    }
    if (!active) return;
    l = half_sum(l);
    if (q < sd.L) {
        const long row = base + (long)q * sd.pos_stride;
        store_rowT(out + row * sd.D + head * ATT_HD, hi, o0, o1, 1.0f / l);
        if (lse && hi == 0) lse[row * sd.heads + head] = (m + log2f(l)) * kLn2;          // natural-log LSE of the scaled scores
    }
}

// ------------------------------------------------------------------------------------------------ backward: dQ (+ delta)
template <int CH, bool SOLO = false>
__global__ __launch_bounds__(256, 2) void attn_x3_bwd_dq(SeqDesc sd, int nt, const float* __restrict__ qkv, const float* __restrict__ o, const float* __restrict__ dout,
                                                         const float* __restrict__ lse, float* __restrict__ delta, float* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) char smem_[];          // [K hi][K lo][V hi][V lo] (SOLO: one set per wave)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    StreamWork w = stream_work(sd.n_outer * sd.n_inner * sd.heads, (nt + 3) / 4);
    if (SOLO) { w.pair = blockIdx.x * 4 + wave; w.chunk = 0; w.valid = w.pair < sd.n_outer * sd.n_inner * sd.heads; }
    if (!w.valid) return;
    char* smem = SOLO ? smem_ + wave * (4 * TILE_B) : smem_;
    const int item = w.pair / sd.heads, head = w.pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3;
    const float* qh = qkv + base * ld3 + head * ATT_HD;
    const int qt = SOLO ? 0 : w.chunk * 4 + wave;
    const bool active = qt < nt;
    const int q = 32 * qt + l31, qc = q < sd.L ? q : sd.L - 1;
    const long row = base + (long)qc * sd.pos_stride;
    if (SOLO) x_stage_wave(qh + sd.D, pse, qh + 2 * sd.D, pse, sd.L, smem, lane);
    SplitOp::Frag qf[4], dof[4];
    xfrag_global(qh + (size_t)qc * pse, hi, qf);
    // delta = rowsum(dO * O) of this lane's query in f32 (this half-wave's 32 channels + the other's): published for the dK / dV kernel, which runs after this one
    float dl;
    {
        float dov[32];
        xfrag_global(dout + row * sd.D + head * ATT_HD, hi, dof, dov);
        const float* orow = o + row * sd.D + head * ATT_HD;
        float part = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(orow + 16 * ks + 8 * hi), b = *reinterpret_cast<const f32x4*>(orow + 16 * ks + 8 * hi + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { part = fmaf(dov[8 * ks + e], a[e], part); part = fmaf(dov[8 * ks + 4 + e], b[e], part); }
        }
        dl = half_sum(part);
        if (active && q < sd.L && hi == 0) delta[row * sd.heads + head] = dl;
    }
    const float ls = lse[row * sd.heads + head] * kLog2e;
    const float sc = kScale * kLog2e;
    f32x16 dq0, dq1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq0[r] = 0.f; dq1[r] = 0.f; }
    const int kt_end = (!active) ? 0 : causal_key_tiles(sd, nt, qt);
    const int kt_end_wg = causal_key_tiles(sd, nt, w.chunk * 4 + 3);
    for (int c0 = 0; c0 < kt_end_wg; c0 += CH) {
        if (!SOLO) {
            __syncthreads();
            x_stage<CH>(qh + sd.D, pse, qh + 2 * sd.D, pse, c0, kt_end_wg, sd.L, smem, tid);
            __syncthreads();
        }
        const int jend = (c0 + CH < kt_end) ? c0 + CH : kt_end;
        for (int j = c0; j < jend; ++j) {
            // dq_tile on its helpers, written out (see the comment above attn_x3_bwd_dkv)
            const P::Tile kt = x_tile<CH>(smem, j - c0), vt = x_tile<CH>(smem + 2 * CH * TILE_B, j - c0);
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = P::mm(frag_row<P>(kt, l31, ks, hi), qf[ks], s);                 // S^T[key][query]
                dp = P::mm(frag_row<P>(vt, l31, ks, hi), dof[ks], dp);              // dP^T[key][query] = V dO^T
            }
            const bool need_mask = (32 * j + 31 >= sd.L) || (q - l31 + 31 >= sd.L) || ((long)32 * j + 31 > (long)(q - l31) + sd.diag);
            float dsv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sc, -ls));
                dsv[r] = p * (dp[r] - dl);
            }
            if (need_mask) {
                TCOW_NO_IFCVT();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = 32 * j + crow32(r, hi);
                    if (!(q < sd.L && key < sd.L && (long)key <= (long)q + sd.diag)) dsv[r] = 0.f;
                }
            }
            const P::Frag d0 = P::pack(dsv), d1 = P::pack(dsv + 8);
            dq0 = P::mm(frag_tr<P>(kt, 0, 0, lane), d0, dq0);                       // dQ^T += K^T dS^T
            dq1 = P::mm(frag_tr<P>(kt, 0, 1, lane), d0, dq1);
            dq0 = P::mm(frag_tr<P>(kt, 1, 0, lane), d1, dq0);
            dq1 = P::mm(frag_tr<P>(kt, 1, 1, lane), d1, dq1);
        }
    }
    if (!active || q >= sd.L) return;
    store_rowT(dqkv + row * ld3 + head * ATT_HD, hi, dq0, dq1, kScale);        // dS was accumulated without its 1/sqrt(d) factor
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// The steps of the two backward kernels are dq_tile / dkv_tile of attention_tiles.h written out on that header's helpers (P = SplitOp), not calls of them, for
// two measured reasons.  (1) dkv_tile pushes masked scores to -1e30 before the exp2; in the code hipcc generates that keeps a second copy of the 16 score
// registers across the mask branch, and with split operands (64 registers of K / V fragments, 64 of accumulators) the chunked dK / dV kernel then needs 256
// registers plus 64 bytes of scratch.  (2) Through dq_tile (and through a dK / dV step in the header's MFMA order) the chunked kernels ran 1.7 % and 3 % slower than
// with the loops below, more than the run-to-run spread (profiles/attn_tile_policy_ab.json).  So here P and dS are zeroed AFTER the exp2, the accumulators
// alternate (dq0, dq1, dq0, dq1), and dkv_tile's key-padding fast path is not taken.  Same values: a masked score gives P = 0 there, P is set to 0 here.
template <int CH, bool SOLO = false>
__global__ __launch_bounds__(256, 2) void attn_x3_bwd_dkv(SeqDesc sd, int nt, const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, float* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) char smem_[];          // [Q hi][Q lo][dO hi][dO lo], CH tiles each, + the chunk's (lse log2e, delta) table (SOLO: per wave)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    StreamWork w = stream_work(sd.n_outer * sd.n_inner * sd.heads, (nt + 3) / 4);
    if (SOLO) { w.pair = blockIdx.x * 4 + wave; w.chunk = 0; w.valid = w.pair < sd.n_outer * sd.n_inner * sd.heads; }
    if (!w.valid) return;
    char* smem = SOLO ? smem_ + wave * (4 * TILE_B + 256) : smem_;
    float2* tab = reinterpret_cast<float2*>(smem + 4 * CH * TILE_B);
    const int item = w.pair / sd.heads, head = w.pair - item * sd.heads;
    const long base = seq_base(sd, item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const float* qh = qkv + base * ld3 + head * ATT_HD;
    const float* doh = dout + base * sd.D + head * ATT_HD;
    const int jt = SOLO ? 0 : w.chunk * 4 + wave;
    const bool active = jt < nt;
    const int key = 32 * jt + l31, kc = key < sd.L ? key : sd.L - 1;
    if (SOLO) {
        x_stage_wave(qh, pse, doh, pso, sd.L, smem, lane);
        if (lane < 32) {
            const long row = base + (long)(lane < sd.L ? lane : sd.L - 1) * sd.pos_stride;
            tab[lane] = make_float2(lse[row * sd.heads + head] * kLog2e, delta[row * sd.heads + head]);
        }
    }
    SplitOp::Frag kf[4], vf[4];
    xfrag_global(qh + (size_t)kc * pse + sd.D, hi, kf);
    xfrag_global(qh + (size_t)kc * pse + 2 * sd.D, hi, vf);
    // lanes 0..31 wrote the table through a float2*, the tile step reads it in every lane through a float4*: keep hipcc from moving those reads up
    // (placed after the K / V loads are issued, so that they still go out together with the table's lse / delta loads)
    if (SOLO) TCOW_WAVE_LDS_ORDER();
    f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
    const float sc = kScale * kLog2e;
    // first query tile that can see any key of this wave / of this workgroup
    // (i0 = causal_first_query_tile(sd, jt), written out: with jt = 0 in the SOLO instantiation hipcc folds this form to a 32-bit value that it knows
    // to be non-negative and drops the max(c0, i0) of the loop below; through the function that kernel needed 8 registers more)
    const long qlo = (long)32 * jt - sd.diag;
    const int i0 = qlo > 0 ? (int)(qlo / 32) : 0;
    const int c_start = (causal_first_query_tile(sd, w.chunk * 4) / CH) * CH;
    for (int c0 = c_start; c0 < nt; c0 += CH) {
        if (!SOLO) {
            __syncthreads();
            x_stage<CH>(qh, pse, doh, pso, c0, nt, sd.L, smem, tid);
            if (tid < CH * 32) {
                const int qi = 32 * c0 + tid;
                const long row = base + (long)(qi < sd.L ? qi : sd.L - 1) * sd.pos_stride;
                tab[tid] = make_float2(lse[row * sd.heads + head] * kLog2e, delta[row * sd.heads + head]);
            }
            __syncthreads();
        }
        if (!active) continue;
        const int ib = c0 > i0 ? c0 : i0, ie = c0 + CH < nt ? c0 + CH : nt;
        for (int i = ib; i < ie; ++i) {
            const P::Tile qt_ = x_tile<CH>(smem, i - c0), dot_ = x_tile<CH>(smem + 2 * CH * TILE_B, i - c0);
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = P::mm(frag_row<P>(qt_, l31, ks, hi), kf[ks], s);                // S[query crow32(r, hi)][key l31]
                dp = P::mm(frag_row<P>(dot_, l31, ks, hi), vf[ks], dp);             // dP[query][key] = dO V^T
            }
            const bool need_mask = (32 * i + 31 >= sd.L) || (key - l31 + 31 >= sd.L) || ((long)(key - l31) + 31 > (long)32 * i + sd.diag);
            float pv[16], dsv[16];
            const float4* t4 = reinterpret_cast<const float4*>(tab + 32 * (i - c0) + 4 * hi);                      // (lse2, delta) of queries 8 gq + 4 hi + e
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 a = t4[4 * gq], b = t4[4 * gq + 1];
                const float lsq[4] = {a.x, a.z, b.x, b.z}, dlq[4] = {a.y, a.w, b.y, b.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * gq + e;
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sc, -lsq[e]));
                    pv[r] = p;
                    dsv[r] = p * (dp[r] - dlq[e]);
                }
            }
            if (need_mask) {
                TCOW_NO_IFCVT();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qi = 32 * i + crow32(r, hi);
                    if (!(qi < sd.L && key < sd.L && (long)key <= (long)qi + sd.diag)) { pv[r] = 0.f; dsv[r] = 0.f; }
                }
            }
            const P::Frag p0 = P::pack(pv), p1 = P::pack(pv + 8), d0 = P::pack(dsv), d1 = P::pack(dsv + 8);
            dv0 = P::mm(frag_tr<P>(dot_, 0, 0, lane), p0, dv0);                     // dV^T += dO^T P
            dv1 = P::mm(frag_tr<P>(dot_, 0, 1, lane), p0, dv1);
            dv0 = P::mm(frag_tr<P>(dot_, 1, 0, lane), p1, dv0);
            dv1 = P::mm(frag_tr<P>(dot_, 1, 1, lane), p1, dv1);
            dk0 = P::mm(frag_tr<P>(qt_, 0, 0, lane), d0, dk0);                      // dK^T += Q^T dS
            dk1 = P::mm(frag_tr<P>(qt_, 0, 1, lane), d0, dk1);
            dk0 = P::mm(frag_tr<P>(qt_, 1, 0, lane), d1, dk0);
            dk1 = P::mm(frag_tr<P>(qt_, 1, 1, lane), d1, dk1);
        }
    }
    if (!active || key >= sd.L) return;
    const long row = base + (long)key * sd.pos_stride;
    store_rowT(dqkv + row * ld3 + sd.D + head * ATT_HD, hi, dk0, dk1, kScale);
    store_rowT(dqkv + row * ld3 + 2 * sd.D + head * ATT_HD, hi, dv0, dv1, 1.0f);
}

constexpr int X3_CH = 4;
template <int CH> constexpr int x3_lds() { return 4 * CH * TILE_B; }
template <int CH> constexpr int x3_lds_dkv() { return 4 * CH * TILE_B + CH * 32 * 8; }

template <int CH>
int x3_fwd_launch(hipStream_t st, const SeqDesc& d, int nt, int grid, const void* qkv, void* out, float* lse) {
    tcow_ensure_lds((const void*)attn_x3_fwd<CH>, x3_lds<CH>());
    hipLaunchKernelGGL(attn_x3_fwd<CH>, dim3(grid), dim3(256), x3_lds<CH>(), st, d, nt, (const float*)qkv, (float*)out, lse);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
template <int CH>
int x3_bwd_launch(hipStream_t st, const SeqDesc& d, int nt, int grid, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv) {
    tcow_ensure_lds((const void*)attn_x3_bwd_dq<CH>, x3_lds<CH>());
    tcow_ensure_lds((const void*)attn_x3_bwd_dkv<CH>, x3_lds_dkv<CH>());
    hipLaunchKernelGGL(attn_x3_bwd_dq<CH>, dim3(grid), dim3(256), x3_lds<CH>(), st, d, nt, (const float*)qkv, (const float*)out, (const float*)dout, lse, delta, (float*)dqkv);
    TCOW_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_x3_bwd_dkv<CH>, dim3(grid), dim3(256), x3_lds_dkv<CH>(), st, d, nt, (const float*)qkv, (const float*)dout, lse, (const float*)delta, (float*)dqkv);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // namespace

// Every length.  One-tile sequences (temporal attention, T <= 32) run the SOLO instantiations: a wave per (sequence, head) with wave-private LDS tiles, no barriers
// (the same kernels with one tile per chunk and one active wave per workgroup measured 84 / 302 us forward / backward at configs[1], attention_f32.hip's wave-private
// exact-f32 kernels 127 / 407 us).
int tcow_attn_x3_fwd(hipStream_t st, const SeqDesc& d, const void* qkv, void* out, float* lse) {
    const int nt = cdiv(d.L, 32), pairs = d.n_outer * d.n_inner * d.heads, grid = stream_grid(pairs, cdiv(nt, 4));
    if (nt == 1) {                       // one-tile sequences: a wave per (sequence, head), wave-private 16 KiB
        constexpr int lds = 4 * 4 * TILE_B;
        tcow_ensure_lds((const void*)attn_x3_fwd<1, true>, lds);
        hipLaunchKernelGGL((attn_x3_fwd<1, true>), dim3(cdiv(pairs, 4)), dim3(256), lds, st, d, nt, (const float*)qkv, (float*)out, lse);
        TCOW_CHECK_LAUNCH();
        return TCOW_OK;
    }
    return x3_fwd_launch<2>(st, d, nt, grid, qkv, out, lse);      // forward: two tiles per chunk (32 KiB, 146 registers: three workgroups per CU) -- 132-142 us against 158-163 with four
}

// `delta` = rows * heads floats of workspace (the layout of lse)
int tcow_attn_x3_bwd(hipStream_t st, const SeqDesc& d, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv) {
    const int nt = cdiv(d.L, 32), pairs = d.n_outer * d.n_inner * d.heads, grid = stream_grid(pairs, cdiv(nt, 4));
    if (nt == 1) {
        constexpr int lds = 4 * 4 * TILE_B, lds_dkv = 4 * (4 * TILE_B + 256);
        tcow_ensure_lds((const void*)attn_x3_bwd_dq<1, true>, lds);
        tcow_ensure_lds((const void*)attn_x3_bwd_dkv<1, true>, lds_dkv);
        hipLaunchKernelGGL((attn_x3_bwd_dq<1, true>), dim3(cdiv(pairs, 4)), dim3(256), lds, st, d, nt, (const float*)qkv, (const float*)out, (const float*)dout, lse, delta, (float*)dqkv);
        TCOW_CHECK_LAUNCH();
        hipLaunchKernelGGL((attn_x3_bwd_dkv<1, true>), dim3(cdiv(pairs, 4)), dim3(256), lds_dkv, st, d, nt, (const float*)qkv, (const float*)dout, lse, (const float*)delta, (float*)dqkv);
        TCOW_CHECK_LAUNCH();
        return TCOW_OK;
    }
    return x3_bwd_launch<X3_CH>(st, d, nt, grid, qkv, out, dout, lse, delta, dqkv);      // (two tiles per chunk measured 437-449 vs 426-439 us: the backward kernels stay at two waves per SIMD either way)
}
