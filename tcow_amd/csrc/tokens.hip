// Caller rows K0-K2 and the cls handling of K3-K9: input assembly into patch rows, the embeddings, the one-cls-per-clip
// merge.  Replaces vit.py:233-240 + mask_tracker.py:107-108 + vision_tf.py:81-89 (im2col), vision_tf.py:99-138 (embeddings), vit.py:189-198,215 (cls).
// Bandwidth-bound glue kernels of the Seeker path: simple grid-stride kernels with 8-16 byte vector accesses along the contiguous dimension.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------ im2col
// rows (b,t,s): s = 0 -> zeros, s = 1+n -> flattened patch n of frame (b,t) of cat([rgb, query]) in the order
// c*P*P + py*P + px (Conv2d weight flattening, vit.py:233-240; cat at mask_tracker.py:107-108).  Optional
// (x-0.45)/0.225 on the rgb channels only (vision_tf.py:81-89).
template <typename T>
__global__ void im2col_kernel(int B, int T_, int H, int W, int P, int Crgb, int Cq, const float* __restrict__ rgb, const float* __restrict__ qm, int norm,
                              T* __restrict__ out) {
    const int Hp = H / P, Wp = W / P, N = Hp * Wp, S = N + 1, C = Crgb + Cq;
    const int Kc = C * P * P, q4 = Kc / 4;
    const long total = (long)B * T_ * S * q4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / q4; const int k = (int)(i - row * q4) * 4;
        const int s = (int)(row % S); const long bt = row / S; const int t = (int)(bt % T_); const int b = (int)(bt / T_);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s > 0) {
            const int n = s - 1, hp = n / Wp, wp = n - hp * Wp;
            const int c = k / (P * P), rem = k - c * P * P, py = rem / P, px = rem - py * P;
            const int y = hp * P + py, x = wp * P + px;
            if (c < Crgb) {
                v = ld4(rgb + ((((size_t)b * Crgb + c) * T_ + t) * H + y) * W + x);
                if (norm) { v.x = (v.x - 0.45f) / 0.225f; v.y = (v.y - 0.45f) / 0.225f; v.z = (v.z - 0.45f) / 0.225f; v.w = (v.w - 0.45f) / 0.225f; }
            } else {
                v = ld4(qm + ((((size_t)b * Cq + (c - Crgb)) * T_ + t) * H + y) * W + x);
            }
        }
        st4(out + row * Kc + k, v);
    }
}

// ------------------------------------------------------------------------------------------ col2im
// The adjoint of im2col_kernel.  The patch stride is the patch size, so every pixel sits in exactly one (row, column) of the patch matrix: a permutation
// with a scale, no sums.  Walks the matrix side in order, as im2col_kernel does (16 bytes per thread, whole rows of 4 * (c1 - c0) * P * P bytes
// contiguous), and writes the images in pieces of P * 4 bytes.  Channels c0 <= c < c1 only: c < Crgb goes to channel c of d_rgb (B,Crgb,T,H,W), the rest to
// channel c - Crgb of d_qm (B,Cq,T,H,W); the slot-0 rows of dA are never read.  Channels below Cnorm take the 1 / 0.225 of the forward's normalisation (an
// f32 division, as there); *inv_scale (device scalar, may be NULL) undoes a power-of-two loss scale on the way.
__global__ void col2im_kernel(int B, int T_, int H, int W, int P, int Crgb, int Cq, int c0, int c1, int Cnorm, const float* __restrict__ dA, long lda,
                              const float* __restrict__ inv_scale, float* __restrict__ d_rgb, float* __restrict__ d_qm) {
    const int Hp = H / P, Wp = W / P, N = Hp * Wp, S = N + 1, PP = P * P;
    const int q4 = (c1 - c0) * PP / 4;
    const long total = (long)B * T_ * N * q4;
    const float s = inv_scale ? *inv_scale : 1.0f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long prow = i / q4; const int k = c0 * PP + (int)(i - prow * q4) * 4;
        const int n = (int)(prow % N); const long bt = prow / N; const int t = (int)(bt % T_); const int b = (int)(bt / T_);
        const int hp = n / Wp, wp = n - hp * Wp;
        const int c = k / PP, rem = k - c * PP, py = rem / P, px = rem - py * P;
        const int y = hp * P + py, x = wp * P + px;
        float4 v = ld4(dA + (bt * S + 1 + n) * lda + k);
        v.x *= s; v.y *= s; v.z *= s; v.w *= s;
        if (c < Cnorm) { v.x /= 0.225f; v.y /= 0.225f; v.z /= 0.225f; v.w /= 0.225f; }
        if (c < Crgb) st4(d_rgb + ((((size_t)b * Crgb + c) * T_ + t) * H + y) * W + x, v);
        else st4(d_qm + ((((size_t)b * Cq + (c - Crgb)) * T_ + t) * H + y) * W + x, v);
    }
}

// ------------------------------------------------------------------------------------------ embeddings
// x[b,t,s,:] = (s == 0) ? cls + pos[0] : x + pos[s] + time[t]      (vision_tf.py:99-138; f32 residual stream)
__global__ void embed_fwd_kernel(int B, int T_, int S, int D, float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos,
                                 const float* __restrict__ time) {
    const int d4 = D / 4;
    const long total = (long)B * T_ * S * d4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / d4; const int c = (int)(i - row * d4) * 4;
        const int s = (int)(row % S); const int t = (int)((row / S) % T_);
        const float4 p = ld4(pos + (size_t)s * D + c);
        float4 o;
        if (s == 0) { const float4 cv = ld4(cls + c); o = make_float4(cv.x + p.x, cv.y + p.y, cv.z + p.z, cv.w + p.w); }
        else {
            const float4 v = ld4(x + row * D + c), te = ld4(time + (size_t)t * D + c);
            o = make_float4(v.x + p.x + te.x, v.y + p.y + te.y, v.z + p.z + te.z, v.w + p.w + te.w);
        }
        st4(x + row * D + c, o);
    }
}
// dpos[s] = sum_{b,t} g[b,t,s];  one workgroup per (s, 64 channel quads = 1 KiB of the row): four thread rows split the B T frames (frame bt goes to row
// bt & 3), six loads in flight per thread, partial sums folded in LDS in a fixed order.  (One thread per (s, quad) walking all B T frames alone kept 58 000
// x 16 bytes in flight: 43 us for the 83 MB of configs[1].)
__global__ __launch_bounds__(256) void embed_bwd_pos_kernel(int B, int T_, int S, int D, const float* __restrict__ g, float* __restrict__ dpos, int accumulate) {
    __shared__ float4 red[256];
    const int d4 = D / 4, s = blockIdx.x, q = blockIdx.y * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6, BT = B * T_;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < d4) {
        const float* src = g + (size_t)s * D + q * 4;
        const size_t fs = (size_t)S * D;
        int bt = part;
        for (; bt + 20 < BT; bt += 24) {
            float4 v[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) v[u] = ld4(src + (size_t)(bt + 4 * u) * fs);
#pragma unroll
            for (int u = 0; u < 6; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
        }
        for (; bt < BT; bt += 4) { const float4 v = ld4(src + (size_t)bt * fs); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (part == 0 && q < d4) {
#pragma unroll
        for (int p = 1; p < 4; ++p) { const float4 v = red[p * 64 + threadIdx.x]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
        float* o = dpos + (size_t)s * D + q * 4;
        if (accumulate) { const float4 p = ld4(o); a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w; }
        st4(o, a);
    }
}
// dtime[t] = sum_{b, s>=1} g[b,t,s];  one workgroup per (t, 64-channel-quad group): threads split s, reduce in LDS
__global__ __launch_bounds__(256) void embed_bwd_time_kernel(int B, int T_, int S, int D, const float* __restrict__ g, float* __restrict__ dtime, int accumulate) {
    __shared__ float4 red[256];
    const int t = blockIdx.x, cq = blockIdx.y * 16 + (threadIdx.x & 15), part = threadIdx.x >> 4;  // 16 channel quads x 16 row slices
    const int d4 = D / 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cq < d4) {
        for (int b = 0; b < B; ++b)
            for (int s = 1 + part; s < S; s += 16) {
                const float4 v = ld4(g + (((size_t)b * T_ + t) * S + s) * D + cq * 4); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (part == 0 && cq < d4) {
        for (int p = 1; p < 16; ++p) { const float4 v = red[p * 16 + (threadIdx.x & 15)]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
        float* o = dtime + (size_t)t * D + cq * 4;
        if (accumulate) { const float4 p = ld4(o); a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w; }
        st4(o, a);
    }
}

// ------------------------------------------------------------------------------------------ cls merge
// After the spatial projection every frame's slot 0 holds cls + attn_out(frame).  The reference keeps ONE cls per
// clip: frame 0's row for causal_attention == 1, the mean over frames for 0 (vit.py:189-198,215).  Write that row
// back to every frame's slot 0.  mode: 1 -> frame 0, 0 -> mean.  Backward: sum of the replicas' gradients goes to
// frame 0 (mode 1, others get zero) or is spread as mean (mode 0).
// CT* cast_out (backward only, may be NULL): the 16-bit operand copy of the gradient (cast_scale[row] * x[row], what the LayerNorm backward
// in front of this call wrote for every row) is refreshed for the slot-0 rows this kernel changes, so no separate cast pass is needed.
// sum over the T frames' slot-0 rows in frame order, eight independent loads in flight (one thread per 4 columns of one clip: the loop was
// T dependent-latency loads, 20 us for 276 KB)
__device__ __forceinline__ float4 sum_frames(const float* base, size_t fs, int T_) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < T_; t0 += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = t0 + u < T_ ? ld4(base + (t0 + u) * fs) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
    }
    return a;
}
template <typename CT>
__global__ void cls_merge_kernel(int B, int T_, int S, int D, float* __restrict__ x, int mode, int backward, CT* __restrict__ cast_out, long ldc,
                                 const float* __restrict__ cast_scale) {
    const int d4 = D / 4;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)B * d4) return;
    const int b = (int)(i / d4), c = (int)(i - (long)b * d4) * 4;
    float* base = x + (size_t)b * T_ * S * D + c;
    const size_t fs = (size_t)S * D;
    if (!backward) {
        float4 a;
        if (mode == 1) a = ld4(base);
        else {
            a = sum_frames(base, fs, T_);
            const float inv = 1.0f / (float)T_; a.x *= inv; a.y *= inv; a.z *= inv; a.w *= inv;
        }
        for (int t = 0; t < T_; ++t) st4(base + t * fs, a);
    } else {
        float4 a = sum_frames(base, fs, T_);
        if (mode == 1) {
            st4(base, a);
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 1; t < T_; ++t) st4(base + t * fs, z);
        } else {
            const float inv = 1.0f / (float)T_; a.x *= inv; a.y *= inv; a.z *= inv; a.w *= inv;
            for (int t = 0; t < T_; ++t) st4(base + t * fs, a);
        }
        if (cast_out) {
            for (int t0 = 0; t0 < T_; t0 += 8) {                 // (the row scales eight at a time: the loads used to wait for each other)
                float cs[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) cs[u] = (cast_scale && t0 + u < T_ && !(mode == 1 && t0 + u > 0)) ? cast_scale[((long)b * T_ + t0 + u) * S] : 1.0f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int t = t0 + u;
                    if (t < T_) {
                        const float4 v = (mode == 1 && t > 0) ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(a.x * cs[u], a.y * cs[u], a.z * cs[u], a.w * cs[u]);
                        st4(cast_out + ((long)b * T_ + t) * S * ldc + c, v);
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int tcow_im2col(void* stream, int dtype, int B, int T_, int H, int W, int P, const float* rgb, const float* query, int pretrained_norm, void* out) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && P > 0 && P % 4 == 0 && H % P == 0 && W % P == 0, "tcow_im2col: bad geometry B=%d T=%d H=%d W=%d P=%d", B, T_, H, W, P);
    TCOW_CHECK_ARG(rgb && query && out, "tcow_im2col: null pointer");
    const long total = (long)B * T_ * ((H / P) * (W / P) + 1) * (4 * P * P / 4);
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(im2col_kernel<T>, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, B, T_, H, W, P, 3, 1, rgb, query, pretrained_norm, (T*)out); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_im2col_channels(void* stream, int dtype, int B, int T_, int H, int W, int P, int C, const float* src, int normalise, void* out) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && C > 0 && P > 0 && P % 4 == 0 && H % P == 0 && W % P == 0, "tcow_im2col_channels: bad geometry B=%d T=%d H=%d W=%d P=%d C=%d", B, T_, H, W, P, C);
    TCOW_CHECK_ARG(src && out, "tcow_im2col_channels: null pointer");
    const long total = (long)B * T_ * ((H / P) * (W / P) + 1) * (C * P * P / 4);
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(im2col_kernel<T>, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, B, T_, H, W, P, C, 0, src, src, normalise, (T*)out); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_col2im(void* stream, int B, int T_, int H, int W, int P, const float* dA, long lda, float* d_rgb, float* d_query, int pretrained_norm,
                const float* inv_scale) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && H > 0 && W > 0 && P > 0 && P % 4 == 0 && H % P == 0 && W % P == 0, "tcow_col2im: bad geometry B=%d T=%d H=%d W=%d P=%d", B, T_, H, W, P);
    TCOW_CHECK_ARG(lda >= 4L * P * P && lda % 4 == 0, "tcow_col2im: lda=%ld must be a multiple of 4 and at least 4 * P * P = %d", lda, 4 * P * P);
    TCOW_CHECK_ARG(dA && (d_rgb || d_query), "tcow_col2im: null pointer (dA, or both outputs)");
    const int c0 = d_rgb ? 0 : 3, c1 = d_query ? 4 : 3;
    const long total = (long)B * T_ * ((H / P) * (W / P)) * ((c1 - c0) * P * P / 4);
    hipLaunchKernelGGL(col2im_kernel, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, B, T_, H, W, P, 3, 1, c0, c1, pretrained_norm ? 3 : 0, dA, lda, inv_scale,
                       d_rgb, d_query);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_col2im_channels(void* stream, int B, int T_, int H, int W, int P, int C, const float* dA, long lda, int normalise, const float* inv_scale, float* dst) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && C > 0 && H > 0 && W > 0 && P > 0 && P % 4 == 0 && H % P == 0 && W % P == 0,
                   "tcow_col2im_channels: bad geometry B=%d T=%d H=%d W=%d P=%d C=%d", B, T_, H, W, P, C);
    TCOW_CHECK_ARG(lda >= (long)C * P * P && lda % 4 == 0, "tcow_col2im_channels: lda=%ld must be a multiple of 4 and at least C * P * P = %ld", lda, (long)C * P * P);
    TCOW_CHECK_ARG(dA && dst, "tcow_col2im_channels: null pointer");
    const long total = (long)B * T_ * ((H / P) * (W / P)) * (C * P * P / 4);
    hipLaunchKernelGGL(col2im_kernel, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, B, T_, H, W, P, C, 0, 0, C, normalise ? C : 0, dA, lda, inv_scale, dst, dst);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_embed_fwd(void* stream, int B, int T_, int S, int D, float* x,const float* cls, const float* pos, const float* time_embed) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && S > 1 && D % 4 == 0 && x && cls && pos && time_embed, "tcow_embed_fwd: bad arguments");
    hipLaunchKernelGGL(embed_fwd_kernel, dim3(gs_blocks((long)B * T_ * S * D / 4)), dim3(256), 0, (hipStream_t)stream, B, T_, S, D, x, cls, pos, time_embed);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_embed_bwd(void* stream, int B, int T_, int S, int D, const float* g, float* dpos, float* dtime, int accumulate) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && S > 1 && D % 4 == 0 && g && dpos && dtime, "tcow_embed_bwd: bad arguments");
    hipLaunchKernelGGL(embed_bwd_pos_kernel, dim3(S, cdiv(D / 4, 64)), dim3(256), 0, (hipStream_t)stream, B, T_, S, D, g, dpos, accumulate);
    TCOW_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_bwd_time_kernel, dim3(T_, cdiv(D / 4, 16)), dim3(256), 0, (hipStream_t)stream, B, T_, S, D, g, dtime, accumulate);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_cls_merge(void* stream, int B, int T_, int S, int D, float* x, int mode, int backward) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && S > 1 && D % 4 == 0 && x && (mode == 0 || mode == 1), "tcow_cls_merge: bad arguments");
    hipLaunchKernelGGL(cls_merge_kernel<float>, dim3(cdiv((long)B * D / 4, 64)), dim3(64), 0, (hipStream_t)stream, B, T_, S, D, x, mode, backward, (float*)nullptr, 0L, (const float*)nullptr);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_cls_merge_bwd_cast(void* stream, int dtype, int B, int T_, int S, int D, float* x, int mode, void* cast_out, long ldc, const float* cast_scale) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && S > 1 && D % 4 == 0 && x && (mode == 0 || mode == 1) && cast_out && ldc % 4 == 0, "tcow_cls_merge_bwd_cast: bad arguments");
    const dim3 grid(cdiv((long)B * D / 4, 64));      // (one wave per workgroup: 576 threads of latency-bound work over 9 CUs rather than 3)
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(cls_merge_kernel<T>, grid, dim3(64), 0, (hipStream_t)stream, B, T_, S, D, x, mode, 1, (T*)cast_out, ldc, cast_scale); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // extern "C"
