// Exact-f32 GEMMs (parity mode) on the f32-input MFMA (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain).
// One stride-generic kernel serves the NT form (forward / input-gradient) and the TN form (weight gradient):
//   C[i,j] = sum_k A(i,k) * B(j,k),  A(i,k) = A[i*sai + k*sak],  B(j,k) = B[j*sbj + k*sbk].
// 64x64 tile per 256-thread workgroup (4 waves, one 32x32 MFMA tile each), k walked 16 at a time through LDS
// stored k-major so that fragment reads are conflict-free ds_read_b32.  Speed is secondary here: this path
// exists so that the HIP pipeline can be compared with the fp32 reference below 1e-3.
#include "gemm_f32.h"

namespace {

// (FT = 64: tile edge, FK = 16: k-slice -- gemm_tile_sizes.h)
constexpr int FLD = FT + 4;

__device__ __forceinline__ void load_tile(const float* __restrict__ P, long s_row, long s_k, int row0, int nrows, int k0, int kend,
                                          float (*dst)[FLD], int tid) {
    // 64 rows x 16 k = 1024 elements, 4 per thread, vectorised along whichever index is contiguous.
    if (s_k == 1) {
        const int r = tid >> 2, kk = (tid & 3) * 4;
        const int gr = row0 + r;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (gr < nrows) {
            const float* src = P + (size_t)gr * s_row + k0 + kk;
            if (k0 + kk + 3 < kend && ((reinterpret_cast<uintptr_t>(src) & 15) == 0)) {
                float4 t = *reinterpret_cast<const float4*>(src); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                for (int e = 0; e < 4; ++e) if (k0 + kk + e < kend) v[e] = src[e];
            }
        }
        for (int e = 0; e < 4; ++e) dst[kk + e][r] = v[e];
    } else {
        const int kk = tid >> 4, r = (tid & 15) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (k0 + kk < kend) {
            const float* src = P + (size_t)(k0 + kk) * s_k;
            if (s_row == 1 && row0 + r + 3 < nrows && ((reinterpret_cast<uintptr_t>(src + row0 + r) & 15) == 0)) {
                float4 t = *reinterpret_cast<const float4*>(src + row0 + r); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                for (int e = 0; e < 4; ++e) if (row0 + r + e < nrows) v[e] = src[(size_t)(row0 + r + e) * s_row];
            }
        }
        *reinterpret_cast<float4*>(&dst[kk][r]) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

__global__ __launch_bounds__(256) void gemm_f32_kernel(F32Params p) {
    __shared__ __attribute__((aligned(16))) float As[FK][FLD];
    __shared__ __attribute__((aligned(16))) float Bs[FK][FLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hi = lane >> 5;
    const int m0 = blockIdx.y * FT, n0 = blockIdx.x * FT;
    const int kbeg = blockIdx.z * p.kps;
    const int kend = (kbeg + p.kps < p.K) ? kbeg + p.kps : p.K;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += FK) {
        load_tile(p.A, p.sai, p.sak, m0, p.M, k0, kend, As, tid);
        load_tile(p.B, p.sbj, p.sbk, n0, p.N, k0, kend, Bs, tid);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < FK / 2; ++s) {
            const float a = As[2 * s + hi][wm * 32 + l31];
            const float b = Bs[2 * s + hi][wn * 32 + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int gn = n0 + wn * 32 + l31;
    if (gn >= p.N) return;
    if (p.slab) {
        float* out = p.slab + (size_t)blockIdx.z * p.M * p.N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gm = m0 + wm * 32 + crow32(r, hi);
            if (gm < p.M) out[(size_t)gm * p.N + gn] = acc[r];
        }
        return;
    }
    const float bv = p.bias ? p.bias[gn] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 32 + crow32(r, hi);
        if (gm < p.M) f32_epilogue_store(p, gm, gn, acc[r], bv);
    }
}

}  // namespace

int tcow_gemm_nt_f32(hipStream_t stream, const tcow_gemm_args* a) {
    const F32Params p = f32_params_nt(a, FK);
    hipLaunchKernelGGL(gemm_f32_kernel, dim3(cdiv(a->N, FT), cdiv(a->M, FT), 1), dim3(256), 0, stream, p);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_gemm_tn_f32(hipStream_t stream, const TnPlan& pl, int M, int N, int K, const float* dY, long ldy, const float* X, long ldx, float* slab) {
    const F32Params p = f32_params_plain(N, K, M, dY, 1, ldy, X, 1, ldx, pl.mps, slab);      // output [N,K], contraction over tokens
    hipLaunchKernelGGL(gemm_f32_kernel, dim3(pl.tiles_k, pl.tiles_n, pl.nz), dim3(256), 0, stream, p);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
