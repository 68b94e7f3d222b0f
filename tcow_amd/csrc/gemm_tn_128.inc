// 128-tile kernel of the 16-bit weight-gradient GEMM (included by gemm_tn_bf16.hip; small shapes): 128 x 128 output tile on four waves of 64 x 64,
// 32x32x16 MFMAs, TN_MC = 32 token rows per stage, two stages = 32 KiB of LDS, four workgroups per CU.  A fragment is 32 columns x 16 tokens
// (lane l: column l & 31, tokens 8 (l >> 5) ... + 7), gathered by one "lo" + one "hi" transpose read.  LDS rows are 256 B (128 columns); 16-byte chunk c
// of row r sits at chunk position c ^ ((r&3)<<2), so the four rows a half-wave touches per read fall into four different 64-byte bank segments.
namespace {
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
}  // namespace
