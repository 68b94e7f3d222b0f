// 16-bit weight-gradient GEMM (gfx950):  dW[N,K] += dY[M,N]^T . X[M,K], the token dimension split across workgroups:
// slab[z][N][K] = sum over token rows of slice z of dY[m][n] * X[m][k];  the slabs are folded by reduce.hip.
// Both operands have the contraction index (token row m) as their slow dimension, so the MFMA fragments (consecutive m for one column) are
// gathered with the LDS transpose read ds_read_b64_tr_b16: within a 16-lane group lane 4r+c supplies the address of row r / 4-element column
// quad c of a [4][16] block and receives column (lane&15), rows 0..3 (verified on hardware, profiles/r01_hw_probe.txt).
// Two kernels with two fragment shapes, one included file each, compiled as ONE translation unit: gemm_tn_128.inc (gemm_tn_bf16_kernel, small shapes)
// and gemm_tn_256.inc (tn256_body: gemm_tn_bf16_256_kernel<SCHED> for one problem, gemm_tn_bf16_256_group_kernel<SCHED> for a group in one grid).
// Which kernel runs on how many token slices, and where slab and bias table lie, is the host plan's to say (gemm_tn_plan.h); the launchers below
// turn a plan into kernel parameters and a grid.
#include <stdlib.h>
#include <type_traits>

#include "common.h"
#include "internal.h"
#include "gemm_glds.h"
#include "gemm_tn_layout.h"

namespace {

__device__ uint4 g_zero16 = {0u, 0u, 0u, 0u};

struct TnParams {
    int M, N, K;
    const bf16_t* dY; long ldy;
    const bf16_t* X; long ldx;
    float* slab;
    int tiles_n, tiles_k, mps, nz;   // mps: token rows per slice (multiple of the stage); nz slices
    float* bias_part;                // optional [nz][tiles_k][2][N] partial column sums of dY (bias gradient)
    int rows_per_pk;                 // LDS rows of each stage summed by the workgroup with k-tile index pk
};

}  // namespace

#include "gemm_tn_128.inc"
#include "gemm_tn_256.inc"

static TnParams tn_params(const TnPlan& pl, int M, int N, int K, const void* dY, long ldy, const void* X, long ldx, float* slab, float* bias_part) {
    TnParams p;
    p.M = M; p.N = N; p.K = K; p.dY = (const bf16_t*)dY; p.ldy = ldy; p.X = (const bf16_t*)X; p.ldx = ldx; p.slab = slab;
    p.tiles_n = pl.tiles_n; p.tiles_k = pl.tiles_k; p.mps = pl.mps; p.nz = pl.nz;
    p.bias_part = bias_part; p.rows_per_pk = pl.rows_per_pk;
    return p;
}
template <typename P>
static void tn_launch_256(void (*kernel)(P), int grid, hipStream_t stream, const P& p) {
    tcow_ensure_lds(reinterpret_cast<const void*>(kernel), T2_LDS);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), T2_LDS, stream, p);
}

int tcow_gemm_tn_bf16(hipStream_t stream, const TnPlan& pl, int M, int N, int K, const bf16_t* dY, long ldy, const bf16_t* X, long ldx, float* slab, float* bias_part) {
    TCOW_CHECK_ARG(N % 8 == 0 && K % 8 == 0 && ldy % 8 == 0 && ldx % 8 == 0, "tcow_gemm_tn(bf16): N, K, ldy, ldx must be multiples of 8");
    const TnParams p = tn_params(pl, M, N, K, dY, ldy, X, ldx, slab, bias_part);
    if (pl.kernel == TN_K128) hipLaunchKernelGGL(gemm_tn_bf16_kernel, dim3(8 * cdiv(p.nz, 8) * p.tiles_n * p.tiles_k), dim3(256), 2 * 2 * TN_MC * 256, stream, p);
    else tn_launch_256(pl.kernel == TN_K256_S2 ? gemm_tn_bf16_256_kernel<2> : gemm_tn_bf16_256_kernel<1>, p.nz * p.tiles_n * p.tiles_k, stream, p);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// grouped launch (gemm_tn_bf16_256_group_kernel): all problems share M and the slice count
int tcow_gemm_tn_bf16_group(hipStream_t stream, const TnGroupPlan& pl, int n, const tcow_tn_problem* pr, float* const* slabs, float* const* bias_parts) {
    TnGroup g;
    g.n = n;
    for (int i = 0; i < n; ++i) {
        g.p[i] = tn_params(pl.p[i], pr[i].M, pr[i].N, pr[i].K, pr[i].dY, pr[i].ldy, pr[i].X, pr[i].ldx, slabs[i], bias_parts[i]);
        g.first[i] = pl.p[i].first;
    }
    for (int i = n; i <= TCOW_TN_GROUP_MAX; ++i) g.first[i] = pl.workgroups;
    tn_launch_256(pl.kernel == TN_K256_S2 ? gemm_tn_bf16_256_group_kernel<2> : gemm_tn_bf16_256_group_kernel<1>, pl.workgroups, stream, g);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
