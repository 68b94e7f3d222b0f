// Operand casts and row scales of the Seeker step: the f32 -> storage-type copies the GEMMs read (weights and their transposes, one at a time or all of a
// step's in one launch; gradients times a row scale), the in-place upstream-gradient scale, and caller row K9b: the
// DropPath row scales of vit_utils.py:139-154 as applied at vit.py:172-186.  Bandwidth-bound glue kernels: 8-16 byte vector accesses along the contiguous
// dimension.
#include "common.h"

namespace {

// All operand copies of a step in ONE launch: a device-resident table of (W, Wc, Wt, N, K, first tile) records, one tile per workgroup; the
// workgroup finds its record by bisection on the first-tile column (86 weights -> 7 steps).  Tile edge = record.tile (32 or 64): the caller
// counts 64 x 64 tiles when every N and K is a multiple of 64 (all GEMM weights of the reference geometries) -- 16-byte loads and 8-byte
// (16-bit) / 16-byte (f32) stores instead of one element per thread (389 -> ~200 us for the 120 M weights of ViT-B).
struct CastDesc { const float* W; void* Wc; void* Wt; int N, K, tile_begin, tile; };
template <typename T>
__global__ __launch_bounds__(256) void cast_transpose_batched_kernel(const CastDesc* __restrict__ tab, int n) {
    __shared__ float tile[64][65];
    int lo = 0, hi = n - 1;
    const int b = blockIdx.x;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid].tile_begin <= b) lo = mid; else hi = mid - 1; }
    const CastDesc d = tab[lo];
    T* Wc = reinterpret_cast<T*>(d.Wc); T* Wt = reinterpret_cast<T*>(d.Wt);
    if (d.tile == 64) {                                   // N % 64 == 0 and K % 64 == 0: no edge handling
        const int t = b - d.tile_begin, tiles_k = d.K >> 6;
        const int n0 = (t / tiles_k) * 64, k0 = (t - (t / tiles_k) * tiles_k) * 64;
        const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 16 * i;
            const float4 v = ld4(d.W + (size_t)(n0 + r) * d.K + k0 + c4);
            if (Wc) st4(Wc + (size_t)(n0 + r) * d.K + k0 + c4, v);
            tile[r][c4] = v.x; tile[r][c4 + 1] = v.y; tile[r][c4 + 2] = v.z; tile[r][c4 + 3] = v.w;
        }
        __syncthreads();
        if (Wt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = r0 + 16 * i;
                st4(Wt + (size_t)(k0 + k) * d.N + n0 + c4, make_float4(tile[c4][k], tile[c4 + 1][k], tile[c4 + 2][k], tile[c4 + 3][k]));
            }
        }
        return;
    }
    const int t = b - d.tile_begin, tiles_k = (d.K + 31) / 32;
    const int n0 = (t / tiles_k) * 32, k0 = (t - (t / tiles_k) * tiles_k) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int nn = n0 + r, k = k0 + tx;
        float v = 0.f;
        if (nn < d.N && k < d.K) { v = d.W[(size_t)nn * d.K + k]; if (Wc) Elem<T>::st(Wc + (size_t)nn * d.K + k, v); }
        tile[r][tx] = v;
    }
    __syncthreads();
    if (Wt)
        for (int r = ty; r < 32; r += 8) {
            const int k = k0 + r, nn = n0 + tx;
            if (k < d.K && nn < d.N) Elem<T>::st(Wt + (size_t)k * d.N + nn, tile[tx][r]);
        }
}

// ------------------------------------------------------------------------------------------ casts
// dst = T(src * row_scale[row])  (f32 -> T), used to turn residual-stream gradients into GEMM operands
template <typename T>
__global__ void scale_cast_kernel(long rows, int D, const float* __restrict__ src, long lds_, const float* __restrict__ row_scale, T* __restrict__ dst, long ldd) {
    const int d4 = D / 4;
    const long total = rows * d4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / d4; const int c = (int)(i - row * d4) * 4;
        float4 v = ld4(src + row * lds_ + c);
        if (row_scale) { const float s = row_scale[row]; v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
        st4(dst + row * ldd + c, v);
    }
}
// W [N,K] f32 -> Wc [N,K] (T, optional) and Wt [K,N] (T, optional): 32x32 tile transpose through LDS
template <typename T>
__global__ __launch_bounds__(256) void cast_transpose_kernel(int N, int K, const float* __restrict__ Wsrc, T* __restrict__ Wc, T* __restrict__ Wt) {
    __shared__ float tile[32][33];
    const int n0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, k = k0 + tx;
        float v = 0.f;
        if (n < N && k < K) { v = Wsrc[(size_t)n * K + k]; if (Wc) Elem<T>::st(Wc + (size_t)n * K + k, v); }
        tile[r][tx] = v;
    }
    __syncthreads();
    if (Wt)
        for (int r = ty; r < 32; r += 8) {
            const int k = k0 + r, n = n0 + tx;
            if (n < N && k < K) Elem<T>::st(Wt + (size_t)k * N + n, tile[tx][r]);
        }
}

// x *= *scale unless *scale == 1 (then no memory is touched): the upstream gradient of a scalar loss is 1 in the plain training step, and a
// device-side branch is cheaper than a pass over an 83 MB gradient for it (the host cannot look at a device scalar without a synchronisation).
__global__ __launch_bounds__(256) void scale_unless_one_kernel(float* __restrict__ x, long n4, long n, const float* __restrict__ scale) {
    const float s = scale[0];
    if (s == 1.0f) return;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 v = ld4(x + i * 4); v.x *= s; v.y *= s; v.z *= s; v.w *= s; st4(x + i * 4, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) x[n4 * 4 + threadIdx.x] *= s;
}

// DropPath row scales of every block of a divided space-time step (vit_utils.py:139-154 applied at vit.py:172-186): keep = floor(u + keep_p),
// scale = keep / keep_p, one draw per (clip, spatial position) for the temporal branch, per (clip, frame) for the spatial one, per clip for the
// MLP.  out [4][depth][B*T*S]: temporal | spatial | MLP | temporal x mask0 (the row scale of the folded temporal projection).
__global__ void __launch_bounds__(256) droppath_rows_kernel(int depth, int B, int T, int S, const float* __restrict__ u, const float* __restrict__ keep_p,
                                                            const float* __restrict__ mask0, float* __restrict__ out) {
    const long M = (long)B * T * S, n = (long)depth * M;
    const int N = S - 1, per = B * N + B * T + B;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int l = (int)(i / M); const long r = i - (long)l * M;
        const int b = (int)(r / ((long)T * S)), ts = (int)(r - (long)b * T * S), t = ts / S, sp = ts - t * S;
        const float kp = keep_p[l];
        const float* ul = u + (long)l * per;
        const float st = sp == 0 ? 1.0f : floorf(ul[b * N + sp - 1] + kp) / kp;
        const float ss = floorf(ul[B * N + b * T + t] + kp) / kp;
        const float sm = floorf(ul[B * N + B * T + b] + kp) / kp;
        out[i] = st; out[n + i] = ss; out[2 * n + i] = sm; out[3 * n + i] = st * mask0[r];
    }
}

}  // namespace

extern "C" {

int tcow_scale_unless_one(void* stream, float* x, long n, const float* scale) {
    TCOW_CHECK_ARG(x && scale && n > 0 && ((uintptr_t)x & 15) == 0, "tcow_scale_unless_one: bad arguments");
    hipLaunchKernelGGL(scale_unless_one_kernel, dim3(gs_blocks(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, x, n / 4, n, scale);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_scale_cast(void* stream, int dtype, long rows, int D, const float* src, long ld_src, const float* row_scale, void* dst, long ld_dst) {
    TCOW_CHECK_ARG(rows > 0 && D > 0 && D % 4 == 0 && src && dst && ld_src % 4 == 0 && ld_dst % 4 == 0, "tcow_scale_cast: bad arguments");
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(scale_cast_kernel<T>, dim3(gs_blocks(rows * D / 4)), dim3(256), 0, (hipStream_t)stream, rows, D, src, ld_src, row_scale, (T*)dst, ld_dst); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_cast_transpose(void* stream, int dtype, int N, int K, const float* W, void* Wc, void* Wt) {
    TCOW_CHECK_ARG(N > 0 && K > 0 && W && (Wc || Wt), "tcow_cast_transpose: bad arguments");
    const dim3 grid(cdiv(K, 32), cdiv(N, 32));
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(cast_transpose_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, N, K, W, (T*)Wc, (T*)Wt); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

long tcow_cast_desc_bytes(void) { return (long)sizeof(CastDesc); }

int tcow_cast_transpose_batched(void* stream, int dtype, const void* table, int n, int total_tiles) {
    TCOW_CHECK_ARG(table && n > 0 && total_tiles > 0, "tcow_cast_transpose_batched: bad arguments");
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(cast_transpose_batched_kernel<T>, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, (const CastDesc*)table, n); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_droppath_rows(void* stream, int depth, int B, int T, int S, const float* u, const float* keep_p, const float* mask0, float* out) {
    TCOW_CHECK_ARG(depth > 0 && B > 0 && T > 0 && S > 1 && u && keep_p && mask0 && out, "tcow_droppath_rows: bad arguments");
    const long n = (long)depth * B * T * S;
    hipLaunchKernelGGL(droppath_rows_kernel, dim3(gs_blocks(n)), dim3(256), 0, (hipStream_t)stream, depth, B, T, S, u, keep_p, mask0, out);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // extern "C"
