// 16-bit MFMA attention, wave-private family (temporal sequences of at most 64 positions; overview in attention_bf16.hip): one WAVE per
// (clip, slot, head).  The whole sequence -- one or two 32-position tiles of each operand -- sits in LDS tiles that only this wave touches, so
// the kernels have no barriers; four waves of a workgroup take four consecutive (sequence, head) pairs.
// Part of the translation unit attention_bf16.hip, which includes this file after attention_common.h and attention_tiles.h.
namespace {

// Temporal sequences skip slot 0 of every frame (the cls replica: SeqDesc.offset = 1, inner_stride = 1), but the GEMMs that consume the attention
// output / produce dqkv read all rows: the wave that owns slot 1 of a clip also defines the slot-0 rows of its head as zero (`sections` blocks of
// 64 columns, D apart) -- this used to be a separate launch per attention call.
__device__ __forceinline__ void zero_prev_slot(const SeqDesc& sd, const WorkId& w, long base, bf16_t* __restrict__ dst, long ld, int sections, int lane) {
    if (w.item % sd.n_inner != 0) return;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int p0 = 0; p0 < sd.L; p0 += 8) {
        const int p = p0 + (lane >> 3);
        if (p < sd.L)
            for (int sec = 0; sec < sections; ++sec)
                *reinterpret_cast<uint4*>(dst + (base - 1 + (long)p * sd.pos_stride) * ld + (long)sec * sd.D + w.head * ATT_HD + (lane & 7) * 8) = z;
    }
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256, 2) void attn_fwd_mfma(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse, int zero0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkId w = work_id(sd, wave);
    if (!w.valid) return;
    const long base = seq_base(sd, w.item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3;
    const bf16_t* qh = qkv + base * ld3 + w.head * ATT_HD;
    if (zero0) zero_prev_slot(sd, w, base, out, sd.D, 1, lane);
    // K, V AND Q tiles of the sequence in LDS.  Q used to be fetched as MFMA fragments straight from
    // global memory -- 16 bytes per lane from 32 different rows per instruction, a quarter of every cache line per request -- and the
    // result went out as 8-byte pieces per lane; both now move as whole 128-byte rows (direct-to-LDS loads in, store_tile_staged out
    // through the Q tile's space once its fragments are in registers).
    char* kt = smem + wave * (3 * nt * TILE_B);
    char* vt = kt + nt * TILE_B;
    char* qt_ = vt + nt * TILE_B;
    for (int t = 0; t < nt; ++t) {
        load_tile(qh, pse, 32 * t, sd.L, qt_ + t * TILE_B, lane);
        load_tile(qh + sd.D, pse, 32 * t, sd.L, kt + t * TILE_B, lane);
        load_tile(qh + 2 * sd.D, pse, 32 * t, sd.L, vt + t * TILE_B, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int qt = 0; qt < nt; ++qt) {
        const int q = 32 * qt + l31;
        bf16x8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = frag_row(qt_ + qt * TILE_B, l31, ks, hi);
        f32x16 o0, o1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
        float m = -1e30f, l = 0.f;
        const int kt_end = causal_key_tiles(sd, nt, qt);
        for (int j = 0; j < kt_end; ++j) fwd_tile(sd, kt + j * TILE_B, vt + j * TILE_B, qf, j, qt, q, l31, hi, lane, m, l, o0, o1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        fwd_store_rows(sd, base, w.head, 32 * qt, lane, m, l, o0, o1, (uint32_t)(uintptr_t)(LDS_PTR(char))(qt_ + qt * TILE_B), out, lse);
    }
}

// ------------------------------------------------------------------------------------------------ backward prep
// ld[(item*heads + h)*Lp + q] = (lse, delta), delta = sum_d dO*O  -- packed per sequence so the kernels read it contiguously
__global__ void attn_bwd_prep_kernel(SeqDesc sd, int Lp, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                     float2* __restrict__ ld) {
    const int items = sd.n_outer * sd.n_inner;
    const long total = (long)items * sd.heads * Lp;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int q = (int)(i % Lp); const long ih = i / Lp; const int h = (int)(ih % sd.heads); const int item = (int)(ih / sd.heads);
        float2 v = make_float2(0.f, 0.f);
        if (q < sd.L) {
            const long row = seq_base(sd, item) + (long)q * sd.pos_stride;
            const bf16_t* a = o + row * sd.D + h * ATT_HD; const bf16_t* b = dout + row * sd.D + h * ATT_HD;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < ATT_HD; d += 4) { const float4 x = ld4(a + d), y = ld4(b + d); s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w; }
            v = make_float2(lse[row * sd.heads + h] * kLog2e, s);      // (lse in log2 units: the consumers feed it to exp2)
        }
        ld[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_mfma(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                         const float2* __restrict__ ld, bf16_t* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkId w = work_id(sd, wave);
    if (!w.valid) return;
    const long base = seq_base(sd, w.item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const bf16_t* qh = qkv + base * ld3 + w.head * ATT_HD;
    const bf16_t* doh = dout + base * sd.D + w.head * ATT_HD;
    const float2* ldh = ld + ((size_t)w.item * sd.heads + w.head) * (nt * 32);
    char* qt_ = smem + wave * (2 * nt * TILE_B);
    char* dot_ = qt_ + nt * TILE_B;
    for (int t = 0; t < nt; ++t) {
        load_tile(qh, pse, 32 * t, sd.L, qt_ + t * TILE_B, lane);
        load_tile(doh, pso, 32 * t, sd.L, dot_ + t * TILE_B, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int j = 0; j < nt; ++j) {
        const int key = 32 * j + l31;
        const int kc = key < sd.L ? key : sd.L - 1;
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { kf[ks] = frag_row_global(qh + sd.D, pse, kc, ks, hi); vf[ks] = frag_row_global(qh + 2 * sd.D, pse, kc, ks, hi); }
        f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
        for (int i = causal_first_query_tile(sd, j); i < nt; ++i) dkv_tile(sd, qt_ + i * TILE_B, dot_ + i * TILE_B, ldh, i, key, kf, vf, l31, hi, lane, dk0, dk1, dv0, dv1);
        dkv_store(sd, base, ld3, w.head, j, l31, hi, dk0, dk1, dv0, dv1, dqkv);
    }
}

// ------------------------------------------------------------------------------------------------ backward: dQ
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_mfma(SeqDesc sd, int nt, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                        const float2* __restrict__ ld, bf16_t* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkId w = work_id(sd, wave);
    if (!w.valid) return;
    const long base = seq_base(sd, w.item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const bf16_t* qh = qkv + base * ld3 + w.head * ATT_HD;
    const bf16_t* doh = dout + base * sd.D + w.head * ATT_HD;
    const float2* ldh = ld + ((size_t)w.item * sd.heads + w.head) * (nt * 32);
    char* kt = smem + wave * (2 * nt * TILE_B);
    char* vt = kt + nt * TILE_B;
    for (int t = 0; t < nt; ++t) {
        load_tile(qh + sd.D, pse, 32 * t, sd.L, kt + t * TILE_B, lane);
        load_tile(qh + 2 * sd.D, pse, 32 * t, sd.L, vt + t * TILE_B, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int qt = 0; qt < nt; ++qt) {
        const int q = 32 * qt + l31;
        const int qc = q < sd.L ? q : sd.L - 1;
        bf16x8 qf[4], dof[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { qf[ks] = frag_row_global(qh, pse, qc, ks, hi); dof[ks] = frag_row_global(doh, pso, qc, ks, hi); }
        const float2 lq = ldh[32 * qt + l31];
        const float ls = lq.x, dl = lq.y;
        f32x16 dq0, dq1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dq0[r] = 0.f; dq1[r] = 0.f; }
        const int kt_end = causal_key_tiles(sd, nt, qt);
        for (int j = 0; j < kt_end; ++j) dq_tile(sd, kt + j * TILE_B, vt + j * TILE_B, j, q, qf, dof, ls, dl, l31, hi, lane, dq0, dq1);
        dq_store(sd, base, ld3, w.head, qt, l31, hi, dq0, dq1, dqkv);
    }
}

// ------------------------------------------------------------------------------------------------ backward, one tile (L <= 32)
// Temporal attention at T <= 32: the whole sequence of a (site, head) is one 32-position tile, so one wave produces dQ, dK and dV
// from a single visit of Q, K, V, dO (wave-private LDS tiles): one launch and one read of every operand instead of prep + dK/dV + dQ
// kernels (three launches, Q/K/V/dO read twice).  delta = rowsum(dO * O) is NOT read from O: with the whole row of P in one tile,
// rowsum(dO * O) = sum_j P_ij (dO_i . V_j) = sum_j P_ij dP_ij comes out of the accumulators the dQ pass holds anyway (lane = query: 16
// multiply-adds + one half-wave exchange, in f32) -- the O tensor (a sixth of the kernel's bytes, read as 8-byte pieces per lane) is not touched.
__global__ __launch_bounds__(256, 2) void attn_bwd_one_tile(SeqDesc sd, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                         const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int zero0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkId w = work_id(sd, wave);
    if (!w.valid) return;
    const long base = seq_base(sd, w.item);
    const long ld3 = 3L * sd.D, pse = sd.pos_stride * ld3, pso = sd.pos_stride * sd.D;
    const bf16_t* qh = qkv + base * ld3 + w.head * ATT_HD;
    const bf16_t* doh = dout + base * sd.D + w.head * ATT_HD;
    if (zero0) zero_prev_slot(sd, w, base, dqkv, ld3, 3, lane);
    char* qt_ = smem + wave * (4 * TILE_B + 256);
    char* kt = qt_ + TILE_B; char* vt = kt + TILE_B; char* dot_ = vt + TILE_B;
    float2* ldw = reinterpret_cast<float2*>(dot_ + TILE_B);
    load_tile<LD_NT>(qh, pse, 0, sd.L, qt_, lane);
    load_tile<LD_NT>(qh + sd.D, pse, 0, sd.L, kt, lane);
    load_tile<LD_NT>(qh + 2 * sd.D, pse, 0, sd.L, vt, lane);
    load_tile<LD_NT>(doh, pso, 0, sd.L, dot_, lane);
    const int qc = l31 < sd.L ? l31 : sd.L - 1;
    const float ls = lse[(base + (long)qc * sd.pos_stride) * sd.heads + w.head] * kLog2e;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- dQ (this wave's queries against its keys), which also yields delta
    {
        bf16x8 qf[4], dof[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { qf[ks] = frag_row(qt_, l31, ks, hi); dof[ks] = frag_row(dot_, l31, ks, hi); }
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = TCOW_MFMA_32x32x16_H16(frag_row(kt, l31, ks, hi), qf[ks], s, 0, 0, 0);
            dp = TCOW_MFMA_32x32x16_H16(frag_row(vt, l31, ks, hi), dof[ks], dp, 0, 0, 0);
        }
        // (one tile = the whole sequence: always a boundary tile.  Lane (q = l31, hi) holds the keys crow32(r, hi).)
        float pv[16];
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = crow32(r, hi);
            const bool ok = l31 < sd.L && key < sd.L && (long)key <= (long)l31 + sd.diag;
            const float p = ok ? __builtin_amdgcn_exp2f(fmaf(s[r], kScale * kLog2e, -ls)) : 0.f;
            pv[r] = p;
            part = fmaf(p, dp[r], part);
        }
        const float dl = half_sum(part);                     // delta_q = sum over ALL keys of P dP
        if (hi == 0) ldw[l31] = l31 < sd.L ? make_float2(ls, dl) : make_float2(0.f, 0.f);
        float dsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dsv[r] = pv[r] * (dp[r] - dl);
        const bf16x8 da0 = pack8(dsv), da1 = pack8(dsv + 8);
        f32x16 dq0, dq1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dq0[r] = 0.f; dq1[r] = 0.f; }
        dq0 = TCOW_MFMA_32x32x16_H16(frag_tr(kt, 0, 0, lane), da0, dq0, 0, 0, 0);
        dq0 = TCOW_MFMA_32x32x16_H16(frag_tr(kt, 1, 0, lane), da1, dq0, 0, 0, 0);
        dq1 = TCOW_MFMA_32x32x16_H16(frag_tr(kt, 0, 1, lane), da0, dq1, 0, 0, 0);
        dq1 = TCOW_MFMA_32x32x16_H16(frag_tr(kt, 1, 1, lane), da1, dq1, 0, 0, 0);
        // K and V fragments of the second pass are taken BEFORE the gradient tiles go out through the K / V tiles' LDS space (whole-row stores)
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { kf[ks] = frag_row(kt, l31, ks, hi); vf[ks] = frag_row(vt, l31, ks, hi); }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (also: the (lse, delta) table is in LDS; wave-private, no barrier)
        bf16_t* drow0 = dqkv + base * ld3 + w.head * ATT_HD;
        const uint32_t lds_k = (uint32_t)(uintptr_t)(LDS_PTR(char))kt, lds_v = (uint32_t)(uintptr_t)(LDS_PTR(char))vt;
        store_tile_staged(lds_k, lane, kScale, dq0, dq1, drow0, pse, sd.L);
        // ---- dK, dV (this wave's keys against its queries)
        f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
        dkv_tile(sd, qt_, dot_, ldw, 0, l31, kf, vf, l31, hi, lane, dk0, dk1, dv0, dv1);
        store_tile_staged(lds_k, lane, kScale, dk0, dk1, drow0 + sd.D, pse, sd.L);        // dS was accumulated without its 1/sqrt(d) factor
        store_tile_staged(lds_v, lane, 1.0f, dv0, dv1, drow0 + 2 * sd.D, pse, sd.L);
    }
}

}  // namespace

// nt = number of 32-position tiles of the sequence (1 or 2); zero0: the kernel also writes the zero rows of the skipped slot 0
int tcow_attn_private_fwd(hipStream_t st, const SeqDesc& d, int nt, const void* qkv, void* out, float* lse, int zero0) {
    const int pairs = d.n_outer * d.n_inner * d.heads, lds = 4 * 3 * nt * TILE_B;
    tcow_ensure_lds((const void*)attn_fwd_mfma, lds);
    hipLaunchKernelGGL(attn_fwd_mfma, dim3(cdiv(pairs, 4)), dim3(256), lds, st, d, nt, (const bf16_t*)qkv, (bf16_t*)out, lse, zero0);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_attn_private_bwd_one_tile(hipStream_t st, const SeqDesc& d, const void* qkv, const void* dout, const float* lse, void* dqkv, int zero0) {
    const int pairs = d.n_outer * d.n_inner * d.heads, lds = 4 * (4 * TILE_B + 256);
    tcow_ensure_lds((const void*)attn_bwd_one_tile, lds);
    hipLaunchKernelGGL(attn_bwd_one_tile, dim3(cdiv(pairs, 4)), dim3(256), lds, st, d, (const bf16_t*)qkv, (const bf16_t*)dout, lse, (bf16_t*)dqkv, zero0);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// ws: the (lse, delta) table, tcow_attn_mfma_bwd_workspace_bytes
int tcow_attn_private_bwd(hipStream_t st, const SeqDesc& d, int nt, const void* qkv, const void* out, const void* dout, const float* lse, void* ws, void* dqkv) {
    const int pairs = d.n_outer * d.n_inner * d.heads, lds = 4 * 2 * nt * TILE_B;
    float2* ld = (float2*)ws;
    const long total = (long)pairs * nt * 32;
    int blocks = cdiv(total, 256); if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(attn_bwd_prep_kernel, dim3(blocks), dim3(256), 0, st, d, nt * 32, (const bf16_t*)out, (const bf16_t*)dout, lse, ld);
    TCOW_CHECK_LAUNCH();
    tcow_ensure_lds((const void*)attn_bwd_dkv_mfma, lds); tcow_ensure_lds((const void*)attn_bwd_dq_mfma, lds);
    hipLaunchKernelGGL(attn_bwd_dkv_mfma, dim3(cdiv(pairs, 4)), dim3(256), lds, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)dout, ld, (bf16_t*)dqkv);
    TCOW_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_bwd_dq_mfma, dim3(cdiv(pairs, 4)), dim3(256), lds, st, d, nt, (const bf16_t*)qkv, (const bf16_t*)dout, ld, (bf16_t*)dqkv);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
