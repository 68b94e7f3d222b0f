// Fused gradient clipping + AdamW over all parameters of the Seeker in three launches (train.py:99-102:
// clip_grad_norm_(seeker.parameters(), 0.3) then AdamW.step(); torch defaults betas (0.9, 0.999), eps 1e-8, weight_decay 0.01 on
// every parameter).  The reference's foreach implementation walks ~250 tensors from Python / ATen per step;
// here a device-resident chunk table (<= 65536 elements per chunk) lets one grid cover every tensor.
//   1. sumsq_kernel   : per-chunk sum of squares of the gradient
//   2. clipcoef_kernel: total norm -> clip coefficient min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); NaN / infinite -> -1 = "skip this step"
//   3. adamw_kernel   : p, m, v update with the clipped gradient (decoupled weight decay, bias correction as torch.optim.AdamW)
#include "common.h"

namespace {

struct Chunk { float* p; const float* g; float* m; float* v; long n; };

__global__ __launch_bounds__(256) void sumsq_kernel(const Chunk* __restrict__ chunks, float* __restrict__ partial) {
    __shared__ float red[4];
    const Chunk c = chunks[blockIdx.x];
    float s = 0.f;
    const long n4 = c.n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) { const float4 g = ld4(c.g + i * 4); s += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w; }
    for (long i = (n4 << 2) + threadIdx.x; i < c.n; i += 256) s += c.g[i] * c.g[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// gscale (may be NULL): the gradients in memory are g_true / *gscale' -- i.e. still multiplied by a loss scale whose INVERSE is *gscale (a power of two).
// The norm is taken of the true gradients and the coefficient handed to the update kernel carries the inverse scale, so the update kernel's
// g * coef is clip(g_true) exactly (powers of two commute with every rounding here): the binary16 mode's unscaling pass over all gradients
// (488 MB read + written per step) disappears into this one-workgroup kernel.
__global__ __launch_bounds__(256) void clipcoef_kernel(const float* __restrict__ partial, int n, float max_norm, float* __restrict__ out /* [0]=coef, [1]=norm, [2]+=skipped */,
                                                       const float* __restrict__ gscale) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float gs = gscale ? gscale[0] : 1.0f;
        const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3])) * gs;
        float coef = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.0f;
        // a non-finite gradient norm (an overflow in a 16-bit backward) marks the step as skipped: coefficient -1
        const bool skip = !(norm <= 3.0e38f);
        out[0] = skip ? -1.0f : (coef < 1.0f ? coef : 1.0f) * gs;
        out[1] = norm;
        if (skip) out[2] += 1.0f;                  // steps skipped so far (every precision): the update kernel counts them out of its bias correction
    }
}

// One element's update, and what of it is the same for every element of a step; both update kernels build it after their early return.  The bias correction
// runs with the number of updates actually APPLIED: the caller counts calls, skipped ones (coef_ptr[2]) are subtracted here, so the moments and their
// correction stay in step after an overflow (torch's GradScaler does not advance the optimizer on a skipped step either).
struct AdamwUpdate {
    float coef, beta1, beta2, eps, bc2_sqrt, decay, step_size;
    __device__ __forceinline__ AdamwUpdate(float coef, const float* coef_ptr, float lr, float beta1, float beta2, float eps, float weight_decay, int step)
        : coef(coef), beta1(beta1), beta2(beta2), eps(eps) {
        const float eff = fmaxf((float)step - coef_ptr[2], 1.0f);
        const float bc1 = 1.0f - powf(beta1, eff);
        bc2_sqrt = sqrtf(1.0f - powf(beta2, eff)), decay = 1.0f - lr * weight_decay, step_size = lr / bc1;
    }
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
        g *= coef;
        p *= decay;
        m = beta1 * m + (1.0f - beta1) * g;
        v = beta2 * v + (1.0f - beta2) * g * g;
        p -= step_size * m / (sqrtf(v) / bc2_sqrt + eps);
    }
};

__global__ __launch_bounds__(256) void adamw_kernel(const Chunk* __restrict__ chunks, const float* __restrict__ coef_ptr, float lr, float beta1, float beta2, float eps,
                                                    float weight_decay, int step) {
    const Chunk c = chunks[blockIdx.x];
    const float coef = coef_ptr[0];
    if (coef < 0.f) return;                        // non-finite gradients: parameters and moments stay as they are (like a GradScaler skip)
    const AdamwUpdate upd(coef, coef_ptr, lr, beta1, beta2, eps, weight_decay, step);
    const long n4 = c.n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
        float4 p = ld4(c.p + i * 4), m = ld4(c.m + i * 4), v = ld4(c.v + i * 4);
        const float4 g = ld4(c.g + i * 4);
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        st4(c.p + i * 4, p); st4(c.m + i * 4, m); st4(c.v + i * 4, v);
    }
    for (long i = (n4 << 2) + threadIdx.x; i < c.n; i += 256) upd(c.p[i], c.g[i], c.m[i], c.v[i]);
}

// The same update for one 64 x 64 tile of a GEMM weight [N, K] -- and, while the new values are in registers, the two 16-bit operand copies the GEMMs read
// (W [N, K] and W^T [K, N] in the library's 16-bit format): the separate re-cast pass (tcow_cast_transpose_batched: 488 MB of f32 read again + the same
// 488 MB of copies written) shrinks to the weights this kernel does not own (the folded products).  Same arithmetic, same operation order as adamw_kernel:
// parameters and moments are bit-identical; the copies equal a cast of the stored f32 value.  Tile pointers are the tile's ORIGIN in each array.
struct CastTile { float* p; const float* g; float* m; float* v; bf16_t* wc; bf16_t* wt; int K, N; };

__global__ __launch_bounds__(256) void adamw_cast_kernel(const CastTile* __restrict__ tiles, const float* __restrict__ coef_ptr, float lr, float beta1, float beta2, float eps,
                                                         float weight_decay, int step) {
    __shared__ float tile[64][65];
    const float coef = coef_ptr[0];
    if (coef < 0.f) return;                        // skipped step: parameters unchanged, the copies stay valid
    const CastTile d = tiles[blockIdx.x];
    const AdamwUpdate upd(coef, coef_ptr, lr, beta1, beta2, eps, weight_decay, step);
    const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + 16 * i;
        const size_t o = (size_t)r * d.K + c4;
        float4 p = ld4(d.p + o), m = ld4(d.m + o), v = ld4(d.v + o);
        const float4 g = ld4(d.g + o);
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        st4(d.p + o, p); st4(d.m + o, m); st4(d.v + o, v);
        st4(d.wc + o, p);
        tile[r][c4] = p.x; tile[r][c4 + 1] = p.y; tile[r][c4 + 2] = p.z; tile[r][c4 + 3] = p.w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = r0 + 16 * i;
        st4(d.wt + (size_t)k * d.N + c4, make_float4(tile[c4][k], tile[c4 + 1][k], tile[c4 + 2][k], tile[c4 + 3][k]));
    }
}

}  // namespace

extern "C" {

long tcow_adamw_chunk_bytes(void) { return (long)sizeof(Chunk); }
long tcow_adamw_tile_bytes(void) { return (long)sizeof(CastTile); }

// Arguments: include/tcow_hip.h.  One launch sequence: the flat table is the chunk table when nothing is tiled; a kernel whose table is empty is not launched.
int tcow_adamw_clip_step(void* stream, const tcow_adamw_args* args) {
    TCOW_CHECK_ARG(args, "tcow_adamw_clip_step: args is NULL");
    const tcow_adamw_args& a = *args;
    TCOW_CHECK_ARG(a.chunks, "tcow_adamw_clip_step: chunks is NULL");
    TCOW_CHECK_ARG(a.scratch, "tcow_adamw_clip_step: scratch is NULL");
    TCOW_CHECK_ARG(a.n_chunks >= 1, "tcow_adamw_clip_step: n_chunks = %d, must be >= 1", a.n_chunks);
    TCOW_CHECK_ARG(a.step >= 1, "tcow_adamw_clip_step: step = %d, must be >= 1", a.step);
    TCOW_CHECK_ARG(a.n_flat >= 0, "tcow_adamw_clip_step: n_flat = %d, must be >= 0", a.n_flat);
    TCOW_CHECK_ARG(a.n_tiles >= 0, "tcow_adamw_clip_step: n_tiles = %d, must be >= 0", a.n_tiles);
    TCOW_CHECK_ARG(a.flat_chunks || a.n_flat == 0, "tcow_adamw_clip_step: flat_chunks is NULL with n_flat = %d", a.n_flat);
    TCOW_CHECK_ARG(a.tiles || a.n_tiles == 0, "tcow_adamw_clip_step: tiles is NULL with n_tiles = %d", a.n_tiles);
    hipStream_t s = (hipStream_t)stream;
    float* tail = a.scratch + a.n_chunks;          // coefficient, norm, skipped count
    hipLaunchKernelGGL(sumsq_kernel, dim3(a.n_chunks), dim3(256), 0, s, (const Chunk*)a.chunks, a.scratch);
    TCOW_CHECK_LAUNCH();
    hipLaunchKernelGGL(clipcoef_kernel, dim3(1), dim3(256), 0, s, a.scratch, a.n_chunks, a.max_norm, tail, a.grad_inv_scale);
    TCOW_CHECK_LAUNCH();
    if (a.n_flat > 0) {
        hipLaunchKernelGGL(adamw_kernel, dim3(a.n_flat), dim3(256), 0, s, (const Chunk*)a.flat_chunks, tail, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step);
        TCOW_CHECK_LAUNCH();
    }
    if (a.n_tiles > 0) {
        hipLaunchKernelGGL(adamw_cast_kernel, dim3(a.n_tiles), dim3(256), 0, s, (const CastTile*)a.tiles, tail, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step);
        TCOW_CHECK_LAUNCH();
    }
    return TCOW_OK;
}

}  // extern "C"
