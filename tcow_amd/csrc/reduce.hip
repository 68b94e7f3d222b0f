// The reduction layer behind every precision mode's backward: the split-K slab folds of the weight-gradient GEMMs (gemm_tn_bf16.hip,
// gemm_f32.hip, gemm_x3.hip), the row folds of LayerNorm's dgamma | dbeta | bias-gradient partial tables (layernorm.hip) and the column
// sums of the bias gradients.  All sums are taken in a fixed order: the results do not depend on the launch.
#include "internal.h"

namespace {

// out[i] (+)= sum_z slab[z][i]  (float4 lanes; cols, ldo and slab_stride multiples of 4 on the vector path)
__global__ void slab_reduce_kernel(const float* __restrict__ slab, int nz, long slab_stride, long n, float* __restrict__ out, long rows, long cols, long ldo, int accumulate) {
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float s = 0.f;
        for (int z = 0; z < nz; ++z) s += slab[(size_t)z * slab_stride + i];
        const long r = i / cols, c = i - r * cols;
        float* o = out + r * ldo + c;
        *o = accumulate ? (*o + s) : s;
    }
}
// Workgroups [0, slab_blocks) fold the split-K slabs; the optional tail workgroups fold the bias-gradient partial table of the same
// weight-gradient GEMM (4 columns x 16 row groups per 64-thread workgroup), so one launch finishes both.
__device__ __forceinline__ void slab_reduce4_body(const int bx, const float* __restrict__ slab, int nz, long slab_stride, long n4, float* __restrict__ out, long cols4, long ldo, int accumulate,
                                                          int slab_blocks, const float* __restrict__ part, int nparts, int N, float* __restrict__ bias_out) {
    if (bx >= slab_blocks) {
        __shared__ float red[16][4];
        const int cq = threadIdx.x & 3, g = threadIdx.x >> 2;
        const int c = (bx - slab_blocks) * 4 + cq;
        float a = 0.f;
        if (c < N)
            for (int r = g; r < nparts; r += 16) a += part[(size_t)r * N + c];
        red[g][cq] = a;
        __syncthreads();
        if (g == 0 && c < N) {
            for (int k = 1; k < 16; ++k) a += red[k][cq];
            bias_out[c] = accumulate ? bias_out[c] + a : a;
        }
        return;
    }
    long i = bx * (long)blockDim.x + threadIdx.x;
    const long stride = (long)slab_blocks * blockDim.x;
    for (; i < n4; i += stride) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        // 8 independent loads in flight per thread: the slabs are streamed once, latency not bandwidth is the enemy
        for (int z0 = 0; z0 < nz; z0 += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (z0 + u < nz) ? ld4(slab + (size_t)(z0 + u) * slab_stride + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        const long r = i / cols4, c = (i - r * cols4) * 4;
        float* o = out + r * ldo + c;
        if (accumulate) { const float4 p = ld4(o); s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w; }
        st4(o, s);
    }
}

__global__ __launch_bounds__(64) void slab_reduce4_kernel(const float* __restrict__ slab, int nz, long slab_stride, long n4, float* __restrict__ out, long cols4, long ldo, int accumulate,
                                                          int slab_blocks, const float* __restrict__ part, int nparts, int N, float* __restrict__ bias_out) {
    slab_reduce4_body(blockIdx.x, slab, nz, slab_stride, n4, out, cols4, ldo, accumulate, slab_blocks, part, nparts, N, bias_out);
}
// The folds of a grouped weight-gradient launch (tcow_gemm_tn_grouped) as ONE flat grid of 256-thread workgroups: job k owns workgroups
// [first[k], first[k + 1]) -- its slab workgroups (512 float4 columns each: two per thread, 2 x nz independent 16-byte loads in flight, the
// slabs read once and not kept in cache) followed by its bias-table workgroups (16 columns x 16 row groups each).
// (The first version was a (max blocks, jobs) grid of one-wave workgroups with one float4 per thread: 52 us for the 170 MB of a ViT-B block's
// seven weights = 3.3 TB/s, a third of its workgroups empty.)
// (measured equal: non-temporal vs plain loads, one vs two float4 columns per thread, 64-bit vs 32-bit row / column split: the launch moves its
// 198-226 MB at 4.1-4.4 TB/s either way)
constexpr int FOLD_BLK = 512;
struct FoldJob { const float* slab; long slab_stride, n4, cols4, ldo; float* out; const float* part; float* bias_out; int nz, accumulate, slab_blocks, nparts, N, blocks; };
struct FoldGroup { int n; int first[TCOW_TN_GROUP_MAX + 1]; FoldJob j[TCOW_TN_GROUP_MAX]; };       // (as many jobs as a grouped weight-gradient launch has problems)
__global__ __launch_bounds__(256) void slab_reduce4_group_kernel(FoldGroup g) {
    int k = 0;
    while (k + 1 < g.n && (int)blockIdx.x >= g.first[k + 1]) ++k;          // workgroup-uniform
    const FoldJob& j = g.j[k];
    const int bx = (int)blockIdx.x - g.first[k];
    const int tid = threadIdx.x;
    if (bx >= j.slab_blocks) {
        __shared__ float red[16][17];
        const int cq = tid & 15, rg = tid >> 4;
        const int c = (bx - j.slab_blocks) * 16 + cq;
        float a = 0.f;
        if (c < j.N)
            for (int r = rg; r < j.nparts; r += 16) a += j.part[(size_t)r * j.N + c];
        red[rg][cq] = a;
        __syncthreads();
        if (rg == 0 && c < j.N) {
            for (int q = 1; q < 16; ++q) a += red[q][cq];
            j.bias_out[c] = j.accumulate ? j.bias_out[c] + a : a;
        }
        return;
    }
    const long i0 = (long)bx * FOLD_BLK + tid, i1 = i0 + 256;
    const bool ok0 = i0 < j.n4, ok1 = i1 < j.n4;
    const int nz = j.nz;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    for (int z0 = 0; z0 < nz; z0 += 8) {
        float4 v0[8], v1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (z0 + u < nz) {                  // (uniform: no load is issued for an absent slice)
                const float* b = j.slab + (size_t)(z0 + u) * j.slab_stride;
                v0[u] = ok0 ? ld4(b + i0 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                v1[u] = ok1 ? ld4(b + i1 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                v0[u] = make_float4(0.f, 0.f, 0.f, 0.f); v1[u] = v0[u];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {          // (slice order 0, 1, 2, ...: the same sum as the one-weight kernel)
            s0.x += v0[u].x; s0.y += v0[u].y; s0.z += v0[u].z; s0.w += v0[u].w;
            s1.x += v1[u].x; s1.y += v1[u].y; s1.z += v1[u].z; s1.w += v1[u].w;
        }
    }
    // (dense outputs need no row / column split; otherwise 32-bit division: the 64-bit one is ~100 instructions, twice per thread = 9 us of a 49 us launch)
    const bool dense = j.ldo == j.cols4 * 4;
    if (ok0) {
        const unsigned r = dense ? 0u : (unsigned)i0 / (unsigned)j.cols4;
        float* o = dense ? j.out + i0 * 4 : j.out + (long)r * j.ldo + ((unsigned)i0 - r * (unsigned)j.cols4) * 4;
        if (j.accumulate) { const float4 p = ld4(o); s0.x += p.x; s0.y += p.y; s0.z += p.z; s0.w += p.w; }
        st4(o, s0);
    }
    if (ok1) {
        const unsigned r = dense ? 0u : (unsigned)i1 / (unsigned)j.cols4;
        float* o = dense ? j.out + i1 * 4 : j.out + (long)r * j.ldo + ((unsigned)i1 - r * (unsigned)j.cols4) * 4;
        if (j.accumulate) { const float4 p = ld4(o); s1.x += p.x; s1.y += p.y; s1.z += p.z; s1.w += p.w; }
        st4(o, s1);
    }
}

// out[c] (+)= sum_r part[r][c] for a tall-skinny partial table (many rows, few columns): 16 columns x 16 row groups per block
// (columns >= N1 go to out2[c - N1]: LayerNorm's dgamma | dbeta table is folded by one launch)
__device__ __forceinline__ void row_reduce_body(int bx, const float* __restrict__ part, int nrows, long ld, int N, float* __restrict__ out, int accumulate,
                                                int N1, float* __restrict__ out2, int N12, float* __restrict__ out3) {
    __shared__ float red[16][17];
    const int c = bx * 16 + (threadIdx.x & 15), g = threadIdx.x >> 4;
    float s = 0.f;
    if (c < N) {
        // 8 independent loads in flight per thread: the table is small (a few MB), the kernel is pure load latency
        int r = g;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (; r + 7 * 16 < nrows; r += 8 * 16) {
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += part[(size_t)(r + 16 * u) * ld + c];
        }
        for (; r < nrows; r += 16) a[0] += part[(size_t)r * ld + c];
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    red[g][threadIdx.x & 15] = s;
    __syncthreads();
    if (g == 0 && c < N) {
        for (int k = 1; k < 16; ++k) s += red[k][threadIdx.x & 15];
        float* o = c < N1 ? out + c : (c < N12 ? out2 + (c - N1) : out3 + (c - N12));      // (columns >= N12: a third table, LayerNorm's fused bias gradient)
        *o = accumulate ? *o + s : s;
    }
}
__global__ __launch_bounds__(256) void row_reduce_kernel(const float* __restrict__ part, int nrows, long ld, int N, float* __restrict__ out, int accumulate,
                                                         int N1, float* __restrict__ out2, int N12, float* __restrict__ out3) {
    row_reduce_body(blockIdx.x, part, nrows, ld, N, out, accumulate, N1, out2, N12, out3);
}
// several such folds in one launch (blockIdx.y = job): the dgamma | dbeta (| bias) tables of all LayerNorm backward calls of a group of blocks
struct RowReduceJob { const float* part; float* out; float* out2; float* out3; long ld; int nrows, N, N1, N12, accumulate; };
struct RowReduceGroup { RowReduceJob j[TCOW_LN_FOLD_MAX]; };
__global__ __launch_bounds__(256) void row_reduce_group_kernel(RowReduceGroup g) {
    const RowReduceJob& j = g.j[blockIdx.y];
    if ((int)blockIdx.x * 16 >= j.N) return;
    row_reduce_body(blockIdx.x, j.part, j.nrows, j.ld, j.N, j.out, j.accumulate, j.N1, j.out2, j.N12, j.out3);
}

// VW consecutive elements of a row as floats: ld4 (VW = 4), or one 16-byte load of eight 16-bit elements (VW = 8)
template <int VW, typename T> __device__ __forceinline__ void ld_cols(const T* p, float (&v)[VW]) {
    if constexpr (VW == 4) {
        const float4 t = ld4(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        static_assert(VW == 8 && sizeof(T) == 2, "eight 16-bit elements or four of any type");
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        v[0] = bflo(u.x); v[1] = bfhi(u.x); v[2] = bflo(u.y); v[3] = bfhi(u.y); v[4] = bflo(u.z); v[5] = bfhi(u.z); v[6] = bflo(u.w); v[7] = bfhi(u.w);
    }
}

// column sums of Y[M,N] (bias gradient): thread = VW consecutive columns, workgroup (bx, by) covers 32 * VW columns x a row slice with
// 8 row groups folded through LDS; partial rows go to `part` and tcow_launch_slab_reduce / a row fold finishes.
template <typename T, int VW>
__device__ __forceinline__ void colsum_partial_body(const int bx, const int by, const T* __restrict__ Y, long ldy, int M, int N, int rows_per_blk, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[8][32][VW];
    const int cq = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = bx * (32 * VW) + cq * VW;
    const int r0 = by * rows_per_blk;
    const int r1 = (r0 + rows_per_blk < M) ? r0 + rows_per_blk : M;
    float s[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) s[k] = 0.f;
    if (c + VW - 1 < N) {
        // four row groups in flight per trip (one load per trip ran at the memory latency: 2.7 TB/s at N = 768 in the f32-storage modes' step)
        int r = r0 + rg;
        for (; r + 24 < r1; r += 32) {
            float v0[VW], v1[VW], v2[VW], v3[VW];
            ld_cols<VW>(Y + (size_t)r * ldy + c, v0); ld_cols<VW>(Y + (size_t)(r + 8) * ldy + c, v1);
            ld_cols<VW>(Y + (size_t)(r + 16) * ldy + c, v2); ld_cols<VW>(Y + (size_t)(r + 24) * ldy + c, v3);
#pragma unroll
            for (int k = 0; k < VW; ++k) s[k] += (v0[k] + v1[k]) + (v2[k] + v3[k]);
        }
        for (; r < r1; r += 8) {
            float v[VW];
            ld_cols<VW>(Y + (size_t)r * ldy + c, v);
#pragma unroll
            for (int k = 0; k < VW; ++k) s[k] += v[k];
        }
    } else if (c < N) {
        for (int r = r0 + rg; r < r1; r += 8) {
            const T* p = Y + (size_t)r * ldy + c;
#pragma unroll
            for (int k = 0; k < VW; ++k)
                if (c + k < N) s[k] += Elem<T>::ld(p + k);
        }
    }
#pragma unroll
    for (int k = 0; k < VW; ++k) red[rg][cq][k] = s[k];
    __syncthreads();
    if (rg == 0 && c < N) {
        for (int g = 1; g < 8; ++g) {
#pragma unroll
            for (int k = 0; k < VW; ++k) s[k] += red[g][cq][k];
        }
        float* o = part + (size_t)by * N + c;
#pragma unroll
        for (int k = 0; k < VW; ++k)
            if (c + k < N) o[k] = s[k];
    }
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ Y, long ldy, int M, int N, int rows_per_blk, float* __restrict__ part) {
    colsum_partial_body<T, 4>(blockIdx.x, blockIdx.y, Y, ldy, M, N, rows_per_blk, part);
}
// the same for several matrices as ONE flat grid (tcow_colsum_grouped): job k owns workgroups [first[k], first[k + 1]), column blocks fastest;
// every thread loads 16 bytes (the entry point has checked what that needs of N, ldy and the pointers)
struct ColsumJob { const void* Y; float* part; long ldy; int M, N, rows_per_blk, nbx; };
struct ColsumGroup { int n; int first[TCOW_COLSUM_GROUP_MAX + 1]; ColsumJob j[TCOW_COLSUM_GROUP_MAX]; };
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_group_kernel(ColsumGroup g) {
    int k = 0;
    while (k + 1 < g.n && (int)blockIdx.x >= g.first[k + 1]) ++k;          // workgroup-uniform
    const ColsumJob& j = g.j[k];
    const int b = (int)blockIdx.x - g.first[k];
    colsum_partial_body<T, 16 / (int)sizeof(T)>(b % j.nbx, b / j.nbx, (const T*)j.Y, j.ldy, j.M, j.N, j.rows_per_blk, j.part);
}

// row slices of a column sum over M rows: one per 256 rows, at most max_parts, none of them empty
inline int colsum_parts(int M, int max_parts, int* rows_per_blk) {
    int parts = cdiv(M, 256); if (parts > max_parts) parts = max_parts; if (parts < 1) parts = 1;
    *rows_per_blk = cdiv(M, parts);
    return cdiv(M, *rows_per_blk);
}
// (the row slices of the f32-storage weight-gradient GEMM's own column-sum launch: with them the partial rows, and so a bias gradient, are the
// same bits whether its Linear's weight gradient is computed or not; up to 112 rows tcow_launch_row_reduce_group adds them in that fold's order)
constexpr int kColsumGroupMaxParts = TN_COLSUM_PARTS;
// f32 elements of a problem's partial table inside the group's workspace (tables start on 16-byte boundaries)
inline long colsum_table_floats(const tcow_colsum_problem& p) {
    if (p.M < 1 || p.N < 1) return 0;
    int rpb;
    return ((long)colsum_parts(p.M, kColsumGroupMaxParts, &rpb) * p.N + 3) & ~3L;
}

}  // namespace

// the vector fold's alignment rules (a group launch needs them of every job: the caller checks)
bool tcow_fold_vec_ok(const float* slab, long slab_stride, long cols, float* out, long ldo) {
    return (cols % 4 == 0) && (ldo % 4 == 0) && (slab_stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(slab) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
}

int tcow_launch_slab_reduce(hipStream_t stream, const float* slab, int nz, long slab_stride, long rows, long cols, float* out, long ldo, int accumulate,
                            const float* bias_part, int bias_nparts, int bias_n, float* bias_out) {
    const long n = rows * cols;
    if (tcow_fold_vec_ok(slab, slab_stride, cols, out, ldo)) {
        int blocks = cdiv(n / 4, 64); if (blocks > 8192) blocks = 8192;
        const int tail = bias_part ? cdiv(bias_n, 4) : 0;
        hipLaunchKernelGGL(slab_reduce4_kernel, dim3(blocks + tail), dim3(64), 0, stream, slab, nz, slab_stride, n / 4, out, cols / 4, ldo, accumulate,
                           blocks, bias_part, bias_nparts, bias_n, bias_out);
    } else {
        if (bias_part) { const int rc = tcow_launch_row_reduce(stream, bias_part, bias_nparts, bias_n, bias_n, bias_out, 0, nullptr, 0, nullptr, accumulate); if (rc) return rc; }
        int blocks = cdiv(n, 256); if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks), dim3(256), 0, stream, slab, nz, slab_stride, n, out, rows, cols, ldo, accumulate);
    }
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// n <= TCOW_TN_GROUP_MAX folds in one launch; every job must satisfy the vector path's alignment rules (the caller checks with tcow_fold_vec_ok)
int tcow_launch_slab_reduce_group(hipStream_t stream, int n, const float* const* slab, int nz, const long* rows, const long* cols, float* const* out, const long* ldo,
                                  const int* accumulate, const float* const* bias_part, const int* bias_nparts, float* const* bias_out) {
    FoldGroup g;
    g.n = n;
    int first = 0;
    for (int i = 0; i < n; ++i) {
        FoldJob& j = g.j[i];
        const long nel = rows[i] * cols[i];
        j.slab = slab[i]; j.slab_stride = nel; j.n4 = nel / 4; j.cols4 = cols[i] / 4; j.ldo = ldo[i]; j.out = out[i];
        j.part = bias_part[i]; j.bias_out = bias_out[i]; j.nz = nz; j.accumulate = accumulate[i];
        j.slab_blocks = slab[i] == out[i] ? 0 : (int)cdiv(nel / 4, FOLD_BLK);       // (slab == destination: the GEMM wrote its single slice in place)
        j.nparts = bias_nparts[i]; j.N = (int)rows[i];
        j.blocks = j.slab_blocks + (bias_part[i] ? cdiv(rows[i], 16) : 0);
        g.first[i] = first;
        first += j.blocks;
    }
    for (int i = n; i < TCOW_TN_GROUP_MAX; ++i) { g.j[i] = g.j[0]; }
    for (int i = n; i <= TCOW_TN_GROUP_MAX; ++i) g.first[i] = first;
    if (first == 0) return TCOW_OK;
    hipLaunchKernelGGL(slab_reduce4_group_kernel, dim3(first), dim3(256), 0, stream, g);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// out1[c] (+)= column sums of part[:, c] for c < N1, out2[c - N1] for N1 <= c < N1 + N2, out3[c - N1 - N2] for the N3 columns after them
// (one table: N2 = N3 = 0, out2 = out3 = NULL; two tables: N3 = 0, out3 = NULL)
int tcow_launch_row_reduce(hipStream_t stream, const float* part, int nrows, long ld, int N1, float* out1, int N2, float* out2, int N3, float* out3, int accumulate) {
    const int N = N1 + N2 + N3;
    hipLaunchKernelGGL(row_reduce_kernel, dim3(cdiv(N, 16)), dim3(256), 0, stream, part, nrows, ld, N, out1, accumulate, N1, out2, out3 ? N1 + N2 : 1 << 30, out3);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// n <= TCOW_LN_FOLD_MAX three-way folds (out | out2 | out3 = columns [0, N1) | [N1, N12) | [N12, N)) in one launch
int tcow_launch_row_reduce_group(hipStream_t stream, int n, const float* const* part, const int* nrows, const long* ld, const int* N1, float* const* out1, const int* N2,
                                 float* const* out2, const int* N3, float* const* out3, const int* accumulate) {
    RowReduceGroup g;
    int gx = 0;
    for (int i = 0; i < n; ++i) {
        RowReduceJob& j = g.j[i];
        j.part = part[i]; j.out = out1[i]; j.out2 = out2[i]; j.out3 = out3[i]; j.ld = ld[i]; j.nrows = nrows[i];
        j.N = N1[i] + N2[i] + (out3[i] ? N3[i] : 0); j.N1 = N1[i]; j.N12 = out3[i] ? N1[i] + N2[i] : (1 << 30); j.accumulate = accumulate[i];
        const int b = cdiv(j.N, 16); if (b > gx) gx = b;
    }
    for (int i = n; i < TCOW_LN_FOLD_MAX; ++i) g.j[i] = g.j[0];
    hipLaunchKernelGGL(row_reduce_group_kernel, dim3(gx, n), dim3(256), 0, stream, g);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

// the partial sums only: `part` [parts][N], returns the number of parts (the caller folds them -- with the weight-gradient slabs, in one launch)
int tcow_launch_colsum_partials(hipStream_t stream, int dtype, const void* Y, long ldy, int M, int N, float* part, int max_parts, int* nparts) {
    int rpb;
    const int parts = colsum_parts(M, max_parts, &rpb);
    if (dtype == TCOW_BF16)
        hipLaunchKernelGGL(colsum_partial_kernel<bf16_t>, dim3(cdiv(N, 128), parts), dim3(256), 0, stream, (const bf16_t*)Y, ldy, M, N, rpb, part);
    else
        hipLaunchKernelGGL(colsum_partial_kernel<float>, dim3(cdiv(N, 128), parts), dim3(256), 0, stream, (const float*)Y, ldy, M, N, rpb, part);
    TCOW_CHECK_LAUNCH();
    *nparts = parts;
    return TCOW_OK;
}

// the partial sums and their fold: out[c] (+)= sum_r Y[r][c]
int tcow_launch_colsum(hipStream_t stream, int dtype, const void* Y, long ldy, int M, int N, float* out, int accumulate, float* part, int max_parts) {
    int parts = 0;
    const int rc = tcow_launch_colsum_partials(stream, dtype, Y, ldy, M, N, part, max_parts, &parts);
    if (rc) return rc;
    return tcow_launch_slab_reduce(stream, part, parts, N, 1, N, out, N, accumulate, nullptr, 0, 0, nullptr);
}

extern "C" {

int tcow_colsum_group_max(void) { return TCOW_COLSUM_GROUP_MAX; }

long tcow_colsum_grouped_workspace_bytes(int dtype, int n, const tcow_colsum_problem* pr) {
    (void)dtype;                    // (partial sums are f32 whatever the storage)
    long total = 0;
    for (int i = 0; pr && i < n; ++i) total += colsum_table_floats(pr[i]);
    return total * 4;
}

int tcow_colsum_grouped(void* stream, int dtype, int n, const tcow_colsum_problem* pr, void* workspace, long workspace_bytes) {
    constexpr int G = TCOW_COLSUM_GROUP_MAX;
    TCOW_CHECK_ARG(dtype == TCOW_BF16 || dtype == TCOW_F32, "tcow_colsum_grouped: unknown dtype %d", dtype);
    TCOW_CHECK_ARG(n >= 1 && n <= G, "tcow_colsum_grouped: 1 .. %d problems per call (got %d)", G, n);
    TCOW_CHECK_ARG(pr && workspace, "tcow_colsum_grouped: null pointer (problems or workspace)");
    const int vw = dtype == TCOW_BF16 ? 8 : 4;              // elements of one 16-byte load
    for (int i = 0; i < n; ++i) {
        const tcow_colsum_problem& p = pr[i];
        TCOW_CHECK_ARG(p.dY && p.out, "tcow_colsum_grouped: null pointer in problem %d (dY or out)", i);
        TCOW_CHECK_ARG(p.M >= 1, "tcow_colsum_grouped: problem %d has M=%d rows, at least 1 is needed", i, p.M);
        TCOW_CHECK_ARG(p.N >= 1 && p.N % vw == 0, "tcow_colsum_grouped: N=%d of problem %d must be a multiple of %d", p.N, i, vw);
        TCOW_CHECK_ARG(p.lddy >= p.N, "tcow_colsum_grouped: lddy=%ld of problem %d is below N=%d", p.lddy, i, p.N);
        TCOW_CHECK_ARG(p.lddy % vw == 0 && reinterpret_cast<uintptr_t>(p.dY) % 16 == 0,
                       "tcow_colsum_grouped: dY of problem %d must be 16-byte aligned with lddy a multiple of %d", i, vw);
    }
    const long need = tcow_colsum_grouped_workspace_bytes(dtype, n, pr);
    TCOW_CHECK_ARG(workspace_bytes >= need, "tcow_colsum_grouped: workspace too small (%ld < %ld)", workspace_bytes, need);
    ColsumGroup g;
    g.n = n;
    const float* part[G]; int nrows[G]; long ld[G]; int N1[G], zero[G], acc[G]; float* out[G]; float* none[G];
    float* table = static_cast<float*>(workspace);
    int first = 0;
    for (int i = 0; i < n; ++i) {
        const tcow_colsum_problem& p = pr[i];
        ColsumJob& j = g.j[i];
        j.Y = p.dY; j.part = table; j.ldy = p.lddy; j.M = p.M; j.N = p.N;
        nrows[i] = colsum_parts(p.M, kColsumGroupMaxParts, &j.rows_per_blk);
        j.nbx = cdiv(p.N, 32 * vw);
        g.first[i] = first;
        first += j.nbx * nrows[i];
        part[i] = table; ld[i] = p.N; N1[i] = p.N; zero[i] = 0; acc[i] = p.accumulate ? 1 : 0; out[i] = p.out; none[i] = nullptr;
        table += colsum_table_floats(p);
    }
    for (int i = n; i < G; ++i) g.j[i] = g.j[0];
    for (int i = n; i <= G; ++i) g.first[i] = first;
    if (dtype == TCOW_BF16) hipLaunchKernelGGL(colsum_partial_group_kernel<bf16_t>, dim3(first), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(colsum_partial_group_kernel<float>, dim3(first), dim3(256), 0, (hipStream_t)stream, g);
    TCOW_CHECK_LAUNCH();
    return tcow_launch_row_reduce_group((hipStream_t)stream, n, part, nrows, ld, N1, out, zero, none, zero, none, acc);
}

}  // extern "C"
