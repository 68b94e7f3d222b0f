// Caller rows K10-K12: the mask head's re-layout + avg-pool (un-patchify), coarsening (bilinear / nearest upsample,
// with the loss scale's max |dout| statistic) and the flags head.  Replaces mask_tracker.py:114-137.  Bandwidth-bound glue kernels: grid-stride, 8-16 byte
// vector accesses along the contiguous dimension.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------ mask head re-layout + avg-pool
// pm rows (b,t,1+n) hold C*P*P outputs in (c, py, px) order (mask_tracker.py:114-115); pooled[bt][c][Y][X] is the
// mean over the st x st pixel block (mask_tracker.py:121-122), Y = hp*(P/st) + py/st.
template <typename T>
__global__ void unpatchify_pool_fwd_kernel(int BT, int Hp, int Wp, int P, int C, int st, const T* __restrict__ pm, float* __restrict__ pooled) {
    const int S = Hp * Wp + 1, Ps = P / st, Ho = Hp * Ps, Wo = Wp * Ps, K = C * P * P;
    const long total = (long)BT * C * Ho * Wo;
    const float inv = 1.0f / (float)(st * st);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int X = (int)(i % Wo); const int Y = (int)((i / Wo) % Ho); const int c = (int)((i / ((long)Wo * Ho)) % C); const long bt = i / ((long)Wo * Ho * C);
        const int hp = Y / Ps, py0 = (Y - hp * Ps) * st, wp = X / Ps, px0 = (X - wp * Ps) * st;
        const T* src = pm + ((size_t)bt * S + 1 + hp * Wp + wp) * K + (size_t)c * P * P;
        float a = 0.f;
        for (int dy = 0; dy < st; ++dy)
            for (int dx = 0; dx < st; ++dx) a += Elem<T>::ld(src + (py0 + dy) * P + px0 + dx);
        pooled[i] = a * inv;
    }
}
// The same for stride 4 and P % 8 == 0 (the path's head: P = 16) with 16-byte loads: one thread takes 8 consecutive patch pixels of FOUR consecutive
// patch rows (a 4 x 8 block of one channel of one token = two pooled outputs), i.e. four loads 2 P elements apart and one 8-byte store -- the
// one-output version reads its 4 x 4 window as sixteen 2-byte loads (48 us for 41 MB at configs[1]).
template <typename T>
__global__ __launch_bounds__(256) void unpatchify_pool4_fwd_kernel(int BT, int Hp, int Wp, int P, int C, const T* __restrict__ pm, float* __restrict__ pooled) {
    const int S = Hp * Wp + 1, Ps = P / 4, Ho = Hp * Ps, Wo = Wp * Ps, K = C * P * P, P8 = P / 8;
    const int per_tok = C * Ps * P8;                         // threads per token: channel x pooled row x 8-pixel piece
    const long total = (long)BT * (S - 1) * per_tok;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int tok = (int)(i / per_tok), r = (int)(i - (long)tok * per_tok);
        const int piece = r % P8, yb = (r / P8) % Ps, c = r / (P8 * Ps);
        const int bt = tok / (S - 1), n = tok - bt * (S - 1), hp = n / Wp, wp = n - hp * Wp;
        const T* src = pm + ((size_t)bt * S + 1 + n) * K + (size_t)c * P * P + (4 * yb) * P + piece * 8;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const float4 u = ld4(src + dy * P), v = ld4(src + dy * P + 4);
            a0 += (u.x + u.y) + (u.z + u.w); a1 += (v.x + v.y) + (v.z + v.w);
        }
        float* o = pooled + (((size_t)bt * C + c) * Ho + hp * Ps + yb) * Wo + wp * Ps + piece * 2;
        *reinterpret_cast<float2*>(o) = make_float2(a0 * 0.0625f, a1 * 0.0625f);
    }
}

template <typename T>
__global__ void unpatchify_pool_bwd_kernel(int BT, int Hp, int Wp, int P, int C, int st, const float* __restrict__ dpooled, T* __restrict__ dpm) {
    const int S = Hp * Wp + 1, Ps = P / st, Ho = Hp * Ps, Wo = Wp * Ps, K = C * P * P;
    const long total = (long)BT * S * K;
    const float inv = 1.0f / (float)(st * st);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K); const long row = i / K; const int s = (int)(row % S); const long bt = row / S;
        float v = 0.f;
        if (s > 0) {
            const int n = s - 1, hp = n / Wp, wp = n - hp * Wp;
            const int c = k / (P * P), rem = k - c * P * P, py = rem / P, px = rem - py * P;
            const int Y = hp * Ps + py / st, X = wp * Ps + px / st;
            v = dpooled[(((size_t)bt * C + c) * Ho + Y) * Wo + X] * inv;
        }
        Elem<T>::st(dpm + i, v);
    }
}

// The same with 8 consecutive patch pixels per thread (P % 8 == 0): 32-bit index arithmetic once per 8 outputs and one 16-byte (16-bit) /
// two 16-byte (f32) stores -- the one-element version spends its time in 64-bit divisions (98 us for 20.8 M elements at configs[1]).
template <typename T>
__global__ __launch_bounds__(256) void unpatchify_pool_bwd8_kernel(int rows, int Hp, int Wp, int P, int C, int st, const float* __restrict__ dpooled, T* __restrict__ dpm) {
    const int S = Hp * Wp + 1, Ps = P / st, Ho = Hp * Ps, Wo = Wp * Ps, K = C * P * P, K8 = K >> 3;
    const float inv = 1.0f / (float)(st * st);
    const long total = (long)rows * K8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int row = (int)(i / K8), k = (int)(i - (long)row * K8) * 8;
        const int bt = row / S, s = row - bt * S;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            const int n = s - 1, hp = n / Wp, wp = n - hp * Wp;
            const int c = k / (P * P), rem = k - c * P * P, py = rem / P, px = rem - py * P;
            const float* src = dpooled + (((size_t)bt * C + c) * Ho + hp * Ps + py / st) * Wo + wp * Ps;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = src[(px + e) / st] * inv;
        }
        T* dst = dpm + (size_t)row * K + k;
        st4(dst, make_float4(v[0], v[1], v[2], v[3]));
        st4(dst + 4, make_float4(v[4], v[5], v[6], v[7]));
    }
}

// ------------------------------------------------------------------------------------------ upsample
// F.interpolate(scale_factor=st, mode='bilinear', align_corners=True) or 'nearest' (mask_tracker.py:124-130),
// fused with the '(B T) C H W -> B C T H W' re-layout (mask_tracker.py:132).  Source index rule of ATen:
// align_corners: src = dst * (in-1)/(out-1); i0 = (int)src; i1 = i0 + (i0 < in-1); w1 = src - i0.
__device__ __forceinline__ void bil_src(int dst, int in, int out, int& i0, int& i1, float& w0, float& w1) {
    const float scale = (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f;
    const float src = scale * (float)dst;
    i0 = (int)src; if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    w1 = src - (float)i0; w0 = 1.0f - w1;
}
// one workgroup column per (b, c, t) frame (blockIdx.y), 4 consecutive output pixels per thread (W is a multiple of st; a 16-byte
// store when W % 4 == 0), 32-bit index arithmetic only
__global__ void upsample_fwd_kernel(int B, int T_, int C, int h, int w, int st, int bilinear, const float* __restrict__ pooled, float* __restrict__ out) {
    const int H = h * st, W = w * st;
    const int f = blockIdx.y;                                   // (b*C + c)*T_ + t  (output layout B,C,T,H,W)
    const int t = f % T_, bc = f / T_, c = bc % C, b = bc / C;
    const float* src = pooled + (((size_t)(b * T_ + t)) * C + c) * h * w;
    float* dst = out + (size_t)f * H * W;
    const int Wq = (W + 3) / 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * Wq; i += gridDim.x * blockDim.x) {
        const int y = i / Wq, x0q = (i - y * Wq) * 4;
        float v[4];
        int y0, y1; float wy0, wy1;
        if (bilinear) bil_src(y, h, H, y0, y1, wy0, wy1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = x0q + e < W ? x0q + e : W - 1;
            if (bilinear) {
                int x0, x1; float wx0, wx1;
                bil_src(x, w, W, x0, x1, wx0, wx1);
                v[e] = wy0 * (wx0 * src[y0 * w + x0] + wx1 * src[y0 * w + x1]) + wy1 * (wx0 * src[y1 * w + x0] + wx1 * src[y1 * w + x1]);
            } else {
                v[e] = src[(y / st) * w + (x / st)];
            }
        }
        float* o = dst + (size_t)y * W + x0q;
        if ((W & 3) == 0) st4(o, make_float4(v[0], v[1], v[2], v[3]));
        else for (int e = 0; e < 4 && x0q + e < W; ++e) o[e] = v[e];
    }
}
// gather-form backward: one thread per pooled pixel sums the output pixels that read it
// amax_bits (may be NULL): atomic maximum of the bit patterns of |dout| over everything the fast path reads = max |dout| (every pixel is read by some
// window; the maximum is idempotent) -- the statistic the binary16 mode's loss scale needs, without two more passes over dout.
__global__ void upsample_bwd_kernel(int B, int T_, int C, int h, int w, int st, int bilinear, const float* __restrict__ dout, float* __restrict__ dpooled,
                                    unsigned* __restrict__ amax_bits) {
    const int H = h * st, W = w * st;
    const long total = (long)B * T_ * C * h * w;
    float amax = 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int X = (int)(i % w); const int Y = (int)((i / w) % h); const int c = (int)((i / ((long)w * h)) % C); const long bt = i / ((long)w * h * C);
        const int b = (int)(bt / T_), t = (int)(bt - (long)b * T_);
        const float* g = dout + (((size_t)b * C + c) * T_ + t) * H * W;
        float a = 0.f;
        if (bilinear && st == 4 && h > 4 && w > 4) {
            // stride 4 (the path's head): output column x reads pooled columns floor(s x), floor(s x) + 1 with 1 / s = 4 + 3 / (w - 1), so X is
            // read by columns inside [4X - 4, 4X + 8) only (same for rows): twelve column weights once per thread, then per candidate row one
            // row weight and three aligned float4 loads -- instead of ~100 per-pixel weight evaluations and scalar loads (122 us -> see HISTORY)
            float wx[12];
            const int xa = 4 * X - 4, ya = 4 * Y - 4;
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int x = xa + e;
                wx[e] = 0.f;
                if (x >= 0 && x < W) { int x0, x1; float wx0, wx1; bil_src(x, w, W, x0, x1, wx0, wx1); if (x0 == X) wx[e] += wx0; if (x1 == X) wx[e] += wx1; }
            }
            for (int e = 0; e < 12; ++e) {
                const int y = ya + e;
                if (y < 0 || y >= H) continue;
                int y0, y1; float wy0, wy1; bil_src(y, h, H, y0, y1, wy0, wy1);
                float wy = 0.f; if (y0 == Y) wy += wy0; if (y1 == Y) wy += wy1;
                if (wy == 0.f) continue;
                const float* row = g + (size_t)y * W + xa;
                float r = 0.f;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (xa + 4 * q >= 0 && xa + 4 * q + 3 < W) {
                        const float4 v = ld4(row + 4 * q);
                        r += wx[4 * q] * v.x + wx[4 * q + 1] * v.y + wx[4 * q + 2] * v.z + wx[4 * q + 3] * v.w;
                        if (amax_bits && q == 1) amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));   // (columns 4X .. 4X+3: each pixel once per row window)
                    }
                }
                a += wy * r;
            }
        } else if (bilinear) {
            // candidate output rows: those whose i0 or i1 can equal Y
            // an output row y reads pooled rows floor(s*y) and floor(s*y)+1, s = (h-1)/(H-1): Y is among them only for
            // (Y-1)/s < y < (Y+1)/s -- about 2/s + 1 rows (9 at stride 4) instead of the 4*st + 1 of the safe bound
            const float isy = (h > 1) ? (float)(H - 1) / (float)(h - 1) : 0.f, isx = (w > 1) ? (float)(W - 1) / (float)(w - 1) : 0.f;
            int ylo = (int)((float)(Y - 1) * isy) - 1, yhi = (int)((float)(Y + 1) * isy) + 2; if (ylo < 0) ylo = 0; if (yhi > H - 1) yhi = H - 1;
            int xlo = (int)((float)(X - 1) * isx) - 1, xhi = (int)((float)(X + 1) * isx) + 2; if (xlo < 0) xlo = 0; if (xhi > W - 1) xhi = W - 1;
            if (h <= 1) { ylo = 0; yhi = H - 1; }
            if (w <= 1) { xlo = 0; xhi = W - 1; }
            for (int y = ylo; y <= yhi; ++y) {
                int y0, y1; float wy0, wy1; bil_src(y, h, H, y0, y1, wy0, wy1);
                float wy = 0.f; if (y0 == Y) wy += wy0; if (y1 == Y) wy += wy1;
                if (wy == 0.f) continue;
                for (int x = xlo; x <= xhi; ++x) {
                    int x0, x1; float wx0, wx1; bil_src(x, w, W, x0, x1, wx0, wx1);
                    float wx = 0.f; if (x0 == X) wx += wx0; if (x1 == X) wx += wx1;
                    if (wx != 0.f) a += wy * wx * g[(size_t)y * W + x];
                }
            }
        } else {
            for (int dy = 0; dy < st; ++dy)
                for (int dx = 0; dx < st; ++dx) a += g[(size_t)(Y * st + dy) * W + X * st + dx];
        }
        dpooled[i] = a;
    }
    if (amax_bits) {
        // one atomic per WORKGROUP, spread over TCOW_AMAX_SLOTS words (the caller takes the maximum of the slots): device-scope atomics on ONE word are
        // served one after the other (~10 ns each) -- with one per wave on one word the 16 000 of them were 160 us of a 200 us kernel
        __shared__ float wmax[4];
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
            if (m > 0.f) atomicMax(amax_bits + (blockIdx.x & (TCOW_AMAX_SLOTS - 1)), __builtin_bit_cast(unsigned, m));      // (non-negative floats order as their bit patterns)
        }
    }
}

// ------------------------------------------------------------------------------------------ flags
// flags[b,t,f] = mean_n (Wf . x[b,t,1+n] + bf) = Wf . mean_n x + bf   (mask_tracker.py:135-137)
// One workgroup of 1024 threads per (b,t): thread (g, c) sums rows 1+g, 1+g+G, ... of float4 column c (G = 1024 / (D/4) row
// groups run in parallel; a single thread per column would walk all S rows serially and leave the load pipe empty).
__global__ __launch_bounds__(1024) void flags_fwd_kernel(int S, int D, int F, const float* __restrict__ x, const float* __restrict__ Wf, const float* __restrict__ bf,
                                                         float* __restrict__ flags) {
    extern __shared__ float4 part[];  // [G][D/4]; row 0 ends up holding the mean
    const int bt = blockIdx.x;
    const int D4 = D >> 2;
    const int G = 1024 / D4 > 0 ? 1024 / D4 : 1;
    const float4* xb = reinterpret_cast<const float4*>(x + (size_t)bt * S * D);
    for (int idx = threadIdx.x; idx < G * D4; idx += 1024) {
        const int g = idx / D4, c = idx - g * D4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int s = 1 + g; s < S; s += G) {
            const float4 v = xb[(size_t)s * D4 + c];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        part[idx] = a;
    }
    __syncthreads();
    const float inv = 1.0f / (float)(S - 1);
    for (int c = threadIdx.x; c < D4; c += 1024) {
        float4 a = part[c];
        for (int g = 1; g < G; ++g) { const float4 v = part[g * D4 + c]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
        part[c] = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
    }
    __syncthreads();
    const float* mean = reinterpret_cast<const float*>(part);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int f = wave; f < F; f += 16) {
        float a = 0.f;
        for (int d = lane; d < D; d += 64) a += mean[d] * Wf[(size_t)f * D + d];
        a = wave_sum(a);
        if (lane == 0) flags[(size_t)bt * F + f] = a + bf[f];
    }
}

}  // namespace

extern "C" {

int tcow_unpatchify_pool_fwd(void* stream, int dtype, int BT, int Hp, int Wp, int P, int C, int st, const void* pm, float* pooled) {
    TCOW_CHECK_ARG(BT > 0 && Hp > 0 && Wp > 0 && P > 0 && C > 0 && st > 0 && P % st == 0 && pm && pooled, "tcow_unpatchify_pool_fwd: bad arguments");
    const long total = (long)BT * C * Hp * Wp * (P / st) * (P / st);
    if (st == 4 && P % 8 == 0 && ((P / 4) * Wp) % 2 == 0 && (dtype == TCOW_BF16 || dtype == TCOW_F32)) {      // the path's head: 16-byte loads (see the kernel)
        const long nthr = (long)BT * Hp * Wp * C * (P / 4) * (P / 8);
        TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(unpatchify_pool4_fwd_kernel<T>, dim3(gs_blocks(nthr)), dim3(256), 0, (hipStream_t)stream, BT, Hp, Wp, P, C, (const T*)pm, pooled); });
        TCOW_CHECK_LAUNCH();
        return TCOW_OK;
    }
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(unpatchify_pool_fwd_kernel<T>, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, BT, Hp, Wp, P, C, st, (const T*)pm, pooled); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_unpatchify_pool_bwd(void* stream, int dtype, int BT, int Hp, int Wp, int P, int C, int st, const float* dpooled, void* dpm) {
    TCOW_CHECK_ARG(BT > 0 && Hp > 0 && Wp > 0 && P > 0 && C > 0 && st > 0 && P % st == 0 && dpooled && dpm, "tcow_unpatchify_pool_bwd: bad arguments");
    const long total = (long)BT * (Hp * Wp + 1) * C * P * P;
    if (P % 8 == 0 && (dtype == TCOW_BF16 || dtype == TCOW_F32) && (reinterpret_cast<uintptr_t>(dpm) & 15) == 0) {
        const int rows = BT * (Hp * Wp + 1);
        TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(unpatchify_pool_bwd8_kernel<T>, dim3(gs_blocks(total / 8)), dim3(256), 0, (hipStream_t)stream, rows, Hp, Wp, P, C, st, dpooled, (T*)dpm); });
        TCOW_CHECK_LAUNCH();
        return TCOW_OK;
    }
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(unpatchify_pool_bwd_kernel<T>, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, BT, Hp, Wp, P, C, st, dpooled, (T*)dpm); });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_upsample_fwd(void* stream, int B, int T_, int C, int h, int w, int st, int bilinear, const float* pooled, float* out) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && C > 0 && h > 0 && w > 0 && st > 0 && pooled && out, "tcow_upsample_fwd: bad arguments");
    TCOW_CHECK_ARG((long)B * C * T_ < 65536, "tcow_upsample_fwd: too many frames for one call");
    { const int per = h * st * ((w * st + 3) / 4); int gx = cdiv(per, 256); if (gx > 64) gx = 64;
      hipLaunchKernelGGL(upsample_fwd_kernel, dim3(gx, B * C * T_), dim3(256), 0, (hipStream_t)stream, B, T_, C, h, w, st, bilinear, pooled, out); }
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_upsample_bwd(void* stream, int B, int T_, int C, int h, int w, int st, int bilinear, const float* dout, float* dpooled) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && C > 0 && h > 0 && w > 0 && st > 0 && dout && dpooled, "tcow_upsample_bwd: bad arguments");
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3(gs_blocks((long)B * C * T_ * h * w)), dim3(256), 0, (hipStream_t)stream, B, T_, C, h, w, st, bilinear, dout, dpooled, (unsigned*)nullptr);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_upsample_bwd_amax(void* stream, int B, int T_, int C, int h, int w, int st, const float* dout, float* dpooled, unsigned* amax_bits, int n_slots) {
    TCOW_CHECK_ARG(B > 0 && T_ > 0 && C > 0 && h > 4 && w > 4 && st == 4 && dout && dpooled && amax_bits, "tcow_upsample_bwd_amax: bilinear stride 4 with h, w > 4 only");
    TCOW_CHECK_ARG(n_slots == TCOW_AMAX_SLOTS, "tcow_upsample_bwd_amax: amax_bits must hold TCOW_AMAX_SLOTS = %d words (got %d)", TCOW_AMAX_SLOTS, n_slots);
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3(gs_blocks((long)B * C * T_ * h * w)), dim3(256), 0, (hipStream_t)stream, B, T_, C, h, w, st, 1, dout, dpooled, amax_bits);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_flags_fwd(void* stream, int BT, int S, int D, int F, const float* x, const float* Wf, const float* bf, float* flags) {
    TCOW_CHECK_ARG(BT > 0 && S > 1 && D > 0 && F > 0 && x && Wf && bf && flags, "tcow_flags_fwd: bad arguments");
    TCOW_CHECK_ARG(D % 4 == 0, "tcow_flags_fwd: D %d must be a multiple of 4", D);
    const int D4 = D / 4, G = 1024 / D4 > 0 ? 1024 / D4 : 1;
    hipLaunchKernelGGL(flags_fwd_kernel, dim3(BT), dim3(1024), (size_t)G * D4 * 16, (hipStream_t)stream, S, D, F, x, Wf, bf, flags);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // extern "C"
