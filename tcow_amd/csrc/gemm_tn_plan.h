// Host plan of the weight-gradient GEMMs (tcow_gemm_tn, tcow_gemm_tn_grouped): which kernel, how many token slices of how many rows, how the bias gradient is
// produced, and where everything lies in the caller's workspace.  Plain C++17 functions of integers (no HIP types), shared by the library (api.cpp reads a plan and
// nothing else; the back ends launch what it says) and by tools/tn_plan_check.cpp, which sweeps shapes and asserts what the launches rely on (tests/test_gemm_tn_plan_host.py).
// Workspace of one problem, the same for every dtype so that one buffer serves a module in any precision: from byte 0 the slab[nz][N][K] f32, one image
// of dW per token slice, with room for one slice more than any dtype's kernel requests; 224 bytes behind it the bias table, TN_TABLE_ROWS x N f32 partial
// column sums of dY that are folded with the slab (or the scratch of the column-sum launch); 32 unused bytes (the total the library has always asked for).
// Workspace of a group that runs as one grid: per problem a slab of (slices + 1) images, then its table of (slices + 1) x tiles_k x 2 rows + 64 bytes,
// 256 bytes behind the last; never below the total of any member alone, since a group that does not group runs its problems one by one in the same buffer.
#pragma once
#include <stdint.h>
#include <initializer_list>
#include "../../include/tcow_hip.h"
#include "gemm_tile_sizes.h"
#include "gemm_tn_layout.h"

constexpr int TCOW_TN_GROUP_MAX = 40;     // problems of one grouped weight-gradient launch (five divided space-time blocks: 35-40 problems; TnGroup = 3.7 KiB, below the 4 KiB kernel-argument limit)
constexpr int TN_TABLE_ROWS = 64 * 24 * 2;   // rows of the bias table: >= nz * tiles_k * 2 partial rows of the fused bias gradient for nz <= 64, K <= 3072
constexpr int TN_COLSUM_PARTS = 64;       // row slices of the column-sum launches (5.4 TB/s averaged over the step's shapes; 256 slices measured the same and a dearer fold)

enum { TN_KNONE = -1, TN_K128, TN_K256_S1, TN_K256_S2, TN_KF32, TN_KX3 };      // gemm_tn_bf16_kernel, gemm_tn_bf16_256(_group)_kernel<1> / <2>, gemm_f32_kernel, gemm_x3_kernel
// How the bias gradient (column sums of dY) is produced.  FUSED: the 16-bit kernels sum the dY stages they hold in LDS into the table, which the slab fold's
// launch folds.  PARTIALS (f32 storage): a column-sum launch writes <= TN_COLSUM_PARTS partial rows first and their fold rides on the slab fold (one launch
// instead of two per Linear).  COLSUM (16-bit, table too small by the fuse rule): a separate column-sum launch behind the fold.
enum { TN_BIAS_NONE, TN_BIAS_FUSED, TN_BIAS_PARTIALS, TN_BIAS_COLSUM };

struct TnPlan {
    int kernel, splits, stage;            // TN_K*; token slices requested; token rows per stage of the kernel
    int mps, nz;                          // token rows per slice (a multiple of the stage); slices that hold rows (<= splits)
    int tiles_n, tiles_k;
    int rows_per_pk;                      // 16-bit: LDS rows of each stage summed by the workgroup with k-tile index pk
    int bias, table_rows;                 // TN_BIAS_*; bias-table rows the kernel writes (FUSED)
    long slab_off, table_off, total;      // bytes
    int first; bool in_place;             // member of a group: its first workgroup; the kernel writes dW itself (slab_off is unused)
};
struct TnGroupPlan {
    bool grouped;                         // one grid; otherwise the problems run one by one (tcow_tn_plan) in the same workspace
    int kernel, splits, mps, nz, workgroups;      // common to the group; TN_K256_S2 if every problem has whole tiles and 32-bit offsets
    long total;
    TnPlan p[TCOW_TN_GROUP_MAX];          // tiles, rows_per_pk, table_rows, offsets, first, in_place of each problem
};

inline constexpr int tnp_cdiv(int a, int b) { return (a + b - 1) / b; }
inline int tnp_clamp(int s, int M) { s = s > M / 256 ? M / 256 : s; return s > 64 ? 64 : s < 1 ? 1 : s; }      // at most 64 slices of at least 256 token rows, at least one

// ---- slices requested
// 128-tile 16-bit kernel and the exact-f32 kernel: ~2 workgroups per CU, a multiple of 8 so that every XCD owns the same number of slices
// (gemm_tn_bf16_kernel pins slice z to XCD z % 8), >= 256 tokens each.
inline int tcow_tn_splits(int M, int N, int K, int tile) {
    int s = ((tnp_cdiv(512, tnp_cdiv(N, tile) * tnp_cdiv(K, tile)) + 7) / 8) * 8;
    const int max_s = M / 256;
    if (s > max_s) s = max_s >= 8 ? (max_s / 8) * 8 : max_s;
    return s < 1 ? 1 : s > 64 ? 64 : s;
}
// 256-tile kernel: as many as fit one round of workgroups (<= 256), at least 256 token rows each
inline int tcow_tn_splits_256(int M, int N, int K) { return tnp_clamp(256 / (tnp_cdiv(N, TNL_COLS) * tnp_cdiv(K, TNL_COLS)), M); }
// bf16 x 3: as many as keep tiles x slices within ONE round of 3 workgroups per CU (the vector loaders fit 168 registers and 40 KiB of LDS), at least 256 tokens each
inline int tcow_tn_splits_x3(int M, int N, int K) { return tnp_clamp((3 * 256) / (tnp_cdiv(N, XT) * tnp_cdiv(K, XT)), M); }

// ---- kernel of the 16-bit mode.  (a 768 x 768 weight = 9 tiles x 28 slices still wins 12 % over the 128-tile kernel despite the larger slab fold)
inline bool tcow_tn_use_256(int M, int N, int K) {
    const int tiles = tnp_cdiv(N, TNL_COLS) * tnp_cdiv(K, TNL_COLS);
    return M >= 4096 && N >= 256 && K >= 256 && tiles >= 9 && tiles <= 256;
}
// Loads of the 256-tile kernel (tn256_body): whole 256-tiles with 32-bit byte offsets take SCHED = 2 (the next stage's requests spread between the MFMAs
// of the stage's fourth block, as buffer loads with scalar row offsets), anything else the general SCHED = 1 (the same stage loop, general addressing).
inline bool tcow_tn_whole(int M, int N, int K, long ldy, long ldx) {
    return N % TNL_COLS == 0 && K % TNL_COLS == 0 && (long)M * ldy < (1L << 29) && (long)M * ldx < (1L << 29);
}

// rows per slice: the even share rounded up to `granule` rows; slices that then hold rows
inline void tnp_slices(int M, int splits, int granule, int* mps, int* nz) {
    *mps = tnp_cdiv(tnp_cdiv(M, splits), granule) * granule;
    *nz = tnp_cdiv(M, *mps);
}

// ---- workspace of one problem (the head comment)
inline long tcow_tn_table_off(int M, int N, int K) {
    int s = tcow_tn_splits(M, N, K, TN_T);
    for (int t : {tcow_tn_splits(M, N, K, FT), tcow_tn_splits_256(M, N, K), tcow_tn_splits_x3(M, N, K)}) s = t > s ? t : s;
    return (long)(s + 1) * N * K * 4 + 224;
}
inline long tnp_table_bytes(int N) { return (long)TN_TABLE_ROWS * N * 4 + 32; }
inline long tcow_tn_workspace_total(int M, int N, int K) { return tcow_tn_table_off(M, N, K) + tnp_table_bytes(N); }

inline TnPlan tcow_tn_plan(int dtype, int M, int N, int K, long ldy, long ldx, bool bias_grad) {
    TnPlan p = {};
    p.table_off = tcow_tn_table_off(M, N, K);
    p.total = p.table_off + tnp_table_bytes(N);
    const bool h16 = dtype == TCOW_BF16, big = h16 && tcow_tn_use_256(M, N, K);
    int tile = TNL_COLS;
    if (big) { p.kernel = tcow_tn_whole(M, N, K, ldy, ldx) ? TN_K256_S2 : TN_K256_S1; p.splits = tcow_tn_splits_256(M, N, K); p.stage = TNL_ROWS; }
    else if (h16) { p.kernel = TN_K128; p.splits = tcow_tn_splits(M, N, K, tile = TN_T); p.stage = TN_MC; }
    else if (dtype == TCOW_F32) { p.kernel = TN_KF32; p.splits = tcow_tn_splits(M, N, K, tile = FT); p.stage = FK; }
    else if (dtype == TCOW_F32X3) { p.kernel = TN_KX3; tile = XT; p.splits = tcow_tn_splits_x3(M, N, K); p.stage = XK; }
    else { p.kernel = TN_KNONE; return p; }
    p.tiles_n = tnp_cdiv(N, tile); p.tiles_k = tnp_cdiv(K, tile);
    tnp_slices(M, p.splits, h16 ? TNL_ROWS : p.stage, &p.mps, &p.nz);      // (both 16-bit kernels round to the 256-tile kernel's stage, two of the 128-tile kernel's)
    if (h16) p.rows_per_pk = tnp_cdiv(p.stage, p.tiles_k);
    // The fuse rule: the table must hold two rows per slice REQUESTED and k-tile of 128, whichever kernel runs.  Conservative for the 256-tile kernel, which
    // writes two rows per slice that holds rows and k-tile of 256 (at most half as many).
    if (bias_grad) p.bias = !h16 ? TN_BIAS_PARTIALS : (long)p.splits * tnp_cdiv(K, TN_T) * 2 <= TN_TABLE_ROWS ? TN_BIAS_FUSED : TN_BIAS_COLSUM;
    p.table_rows = p.bias == TN_BIAS_FUSED ? p.nz * p.tiles_k * 2 : 0;
    return p;
}

// ---- groups: 16-bit problems of the 256-tile kernel that share M run as one grid with a common slice count
inline bool tcow_tn_group_ok(int dtype, int n, const tcow_tn_problem* pr) {
    if (dtype != TCOW_BF16 || n < 2 || n > TCOW_TN_GROUP_MAX) return false;
    for (int i = 0; i < n; ++i) {
        if (pr[i].M != pr[0].M || !tcow_tn_use_256(pr[i].M, pr[i].N, pr[i].K) || pr[i].N % 8 || pr[i].K % 8 || pr[i].ldy % 8 || pr[i].ldx % 8) return false;
    }
    return true;
}
// common slice count: the cheapest one under  cost(s) = 1 / (fill of whole rounds of 256 workgroups) + 0.044 s  -- every slice writes and re-reads
// one f32 image of all the group's weights: slab store + fold measured at 22 % of the loop time with five slices (profiles/r04_ubench_tn_ab.txt,
// r04_step_kernel_stats.txt).  One ViT-B block (153 tiles): 5 slices (765 workgroups = 2.99 rounds); four blocks (612 tiles): 2 slices
// (1224 workgroups = 4.78 rounds, 60 % less slab traffic for 4 % more tail).  >= 256 token rows per slice.
inline int tcow_tn_group_slices(int n, const tcow_tn_problem* pr) {
    int tiles = 0, best = 1;
    for (int i = 0; i < n; ++i) tiles += tnp_cdiv(pr[i].N, TNL_COLS) * tnp_cdiv(pr[i].K, TNL_COLS);
    double best_cost = 1e30;
    for (int s = 1; s <= tnp_clamp(64, pr[0].M); ++s) {
        const int wg = s * tiles, rounds = tnp_cdiv(wg, 256);
        const double cost = (rounds * 256.0) / (double)wg + 0.044 * s;
        if (cost < best_cost - 1e-9) { best_cost = cost; best = s; }
    }
    return best;
}

inline TnGroupPlan tcow_tn_group_plan(int dtype, int n, const tcow_tn_problem* pr) {
    TnGroupPlan g = {};
    for (int i = 0; i < n; ++i) { const long b = tcow_tn_workspace_total(pr[i].M, pr[i].N, pr[i].K); if (b > g.total) g.total = b; }
    g.grouped = tcow_tn_group_ok(dtype, n, pr);
    if (!g.grouped) return g;
    g.splits = tcow_tn_group_slices(n, pr);
    tnp_slices(pr[0].M, g.splits, TNL_ROWS, &g.mps, &g.nz);
    g.kernel = TN_K256_S2;      // until a problem says otherwise
    long w = 0;
    for (int i = 0; i < n; ++i) {
        TnPlan& p = g.p[i];
        const int N = pr[i].N, K = pr[i].K;
        if (!tcow_tn_whole(pr[i].M, N, K, pr[i].ldy, pr[i].ldx)) g.kernel = TN_K256_S1;
        p.mps = g.mps; p.nz = g.nz; p.tiles_n = tnp_cdiv(N, TNL_COLS); p.tiles_k = tnp_cdiv(K, TNL_COLS);
        p.rows_per_pk = tnp_cdiv(TNL_ROWS, p.tiles_k);
        p.table_rows = pr[i].bias_grad ? g.nz * p.tiles_k * 2 : 0;
        p.first = g.workgroups; g.workgroups += g.nz * p.tiles_n * p.tiles_k;
        p.slab_off = w; w += (long)(g.splits + 1) * N * K * 4;
        p.table_off = w; w += (long)(g.splits + 1) * p.tiles_k * 2 * N * 4 + 64;
        // ONE token slice (a group whose tiles fill whole rounds of the chip by themselves: five ViT-B blocks = 765 tiles): nothing to fold, so the
        // kernel writes a dense, non-accumulating weight gradient straight into its destination -- no slab image written, re-read and copied
        // (2 x 177 MB per five-block group); only the bias-gradient partials still go through the fold launch.  (K % 8 == 0 and lddw == K: of the
        // fold's vector rule, tcow_fold_vec_ok, only the pointer's alignment is left to ask.)
        p.in_place = g.splits == 1 && !pr[i].accumulate && pr[i].lddw == K && ((uintptr_t)pr[i].dW & 15) == 0;
    }
    if (w + 256 > g.total) g.total = w + 256;
    return g;
}
