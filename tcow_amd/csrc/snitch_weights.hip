// Caller row L, the pixel weights of the track (snitch) channel: class balancing, the occluded-pixel factor and the
// hard-negative band of loss.py:85-148 times the frame weights of loss.py:55-83.  (The objective that consumes them is mask_loss.hip.)
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------ snitch pixel weights (caller row L)
// loss.py:85-148 times the frame weights of loss.py:55-83: class balancing (powers 0.7 / -0.3 of the rarer / commoner class
// fraction, 5 % floor), x2 on occluded snitch pixels, x hard_negative_factor on the band = (k x k box dilation of the target) minus
// the target, k = odd(int(sqrt(HW) / 12)) -- the reference's gaussian_blur(target, k, sigma=k) > 0.  Separable dilation: rows here,
// columns inside the weight kernel.
__global__ void __launch_bounds__(256) dilate_rows_kernel(const float* __restrict__ target, long frame_stride_t, int frames_per_seq, long seq_stride_t, int H, int W, int r,
                                                          uint8_t* __restrict__ tmp) {
    const int f = blockIdx.y;
    const int s = f / frames_per_seq, ft = f - s * frames_per_seq;
    const float* src = target + (size_t)s * seq_stride_t + (size_t)ft * frame_stride_t;
    uint8_t* dst = tmp + (size_t)f * H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
        const int y = i / W, x = i - y * W;
        const int x0 = x - r > 0 ? x - r : 0, x1 = x + r < W - 1 ? x + r : W - 1;
        int any = 0;
        for (int xx = x0; xx <= x1; ++xx) any |= src[y * W + xx] > 0.f;
        dst[i] = (uint8_t)any;
    }
}
// The same row dilation as 64-bit masks (W a multiple of 64, r <= 63): one wave per row; ballots give the row's set pixels, every lane tests
// its window [x - r, x + r] against the three words around it, a second ballot is the dilated word.  4 B read + 1 bit written per pixel
// (the byte version walks 2r + 1 = 23 floats per pixel at 240 x 320: 68 us per step); the weight kernel ORs 2r + 1 of these words per 64
// pixels instead of reading 2r + 1 bytes per pixel.
__device__ __forceinline__ unsigned long long bit_range(int a, int b) {            // bits a..b (0 <= a <= b <= 63)
    return ((~0ull) >> (63 - (b - a))) << a;
}
__global__ void __launch_bounds__(256) dilate_rows_bits_kernel(const float* __restrict__ target, long frame_stride_t, int frames_per_seq, long seq_stride_t, int H, int W, int r,
                                                               unsigned long long* __restrict__ bits) {
    const int f = blockIdx.y;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;
    const int s = f / frames_per_seq, ft = f - s * frames_per_seq;
    const float* src = target + (size_t)s * seq_stride_t + (size_t)ft * frame_stride_t + (size_t)y * W;
    const int nw = W >> 6;
    unsigned long long* dst = bits + ((size_t)f * H + y) * nw;
    unsigned long long prev = 0ull, cur = __ballot(src[lane] > 0.f);
    for (int c = 0; c < nw; ++c) {
        const unsigned long long next = c + 1 < nw ? __ballot(src[(c + 1) * 64 + lane] > 0.f) : 0ull;
        const int lo = lane - r, hi = lane + r;
        bool any = (cur & bit_range(lo > 0 ? lo : 0, hi < 63 ? hi : 63)) != 0ull;
        if (lo < 0) any = any || (prev & bit_range(64 + lo, 63)) != 0ull;
        if (hi > 63) any = any || (next & bit_range(0, hi - 64)) != 0ull;
        const unsigned long long d = __ballot(any);
        if (lane == 0) dst[c] = d;
        prev = cur; cur = next;
    }
}
struct WeightsArgs {
    const float* target; long frame_stride_t; int frames_per_seq; long seq_stride_t;   // channel 0 of (BQ,3,T,H,W)
    const uint8_t* ptr; const uint8_t* rowdil; const unsigned long long* rowbits; const float* frame_w; const int* pos_count;   // rowbits != NULL: bit-mask rows (W % 64 == 0)
    float* out; int H, W, r; long n_pixels; int class_balancing; float hard_negative_factor;
};
__global__ void __launch_bounds__(256) snitch_weights_kernel(WeightsArgs a) {
    __shared__ float corr[2];
    if (threadIdx.x == 0) {
        float pc = 1.f, nc = 1.f;
        if (a.class_balancing) {                                            // loss.py:100-119 (host float64 arithmetic there, double here)
            const long pos = *a.pos_count, neg = a.n_pixels - pos;
            float pf = (float)pos / (float)a.n_pixels, nf = (float)neg / (float)a.n_pixels;
            pf = pf < 0.05f ? 0.05f : pf; nf = nf < 0.05f ? 0.05f : nf;
            const double p = pf, n = nf;
            if (p > n) { pc = (float)pow(n / p, 0.7); nc = (float)pow(n / p, -0.3); }
            else { pc = (float)pow(p / n, -0.3); nc = (float)pow(p / n, 0.7); }
        }
        corr[0] = nc; corr[1] = pc;
    }
    __syncthreads();
    const int f = blockIdx.y;
    const int s = f / a.frames_per_seq, ft = f - s * a.frames_per_seq;
    const float* tg = a.target + (size_t)s * a.seq_stride_t + (size_t)ft * a.frame_stride_t;
    const size_t fo = (size_t)f * a.H * a.W;
    const float fw = a.frame_w[f];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.H * a.W; i += gridDim.x * 256) {
        const int y = i / a.W, x = i - y * a.W;
        const float t = tg[i];
        float w = 1.f;
        if (a.class_balancing) { if (t == 0.f) w *= corr[0]; if (t == 1.f) w *= corr[1]; }
        if (a.ptr[fo + i] != 0) w *= 2.f;
        if (a.hard_negative_factor > 1.f && a.rowbits) {
            // the wave's 64 pixels share one word per row (W % 64 == 0, i % 64 == lane): lane j fetches row y - r + j's word, an OR butterfly
            // over the wave gives the column-dilated word, every lane takes its bit
            const int y0 = y - a.r, nw = a.W >> 6, lane = threadIdx.x & 63;
            const int yy = y0 + lane;
            unsigned long long m = (lane <= 2 * a.r && yy >= 0 && yy < a.H) ? a.rowbits[((size_t)f * a.H + yy) * nw + (x >> 6)] : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o, 64);
            if (!(t >= 0.5f) && ((m >> (x & 63)) & 1ull)) w *= a.hard_negative_factor;
        } else if (a.hard_negative_factor > 1.f && !(t >= 0.5f)) {
            const int y0 = y - a.r > 0 ? y - a.r : 0, y1 = y + a.r < a.H - 1 ? y + a.r : a.H - 1;
            int any = 0;
            for (int yy = y0; yy <= y1; ++yy) any |= a.rowdil[fo + (size_t)yy * a.W + x];
            if (any) w *= a.hard_negative_factor;
        }
        a.out[fo + i] = fw * w;
    }
}

}  // namespace

extern "C" size_t tcow_snitch_weights_workspace_bytes(long n_frames, int H, int W) { return (size_t)n_frames * H * W + 256; }

extern "C" int tcow_snitch_weights(void* stream, long n_seq, int T, int H, int W, const float* target_ch0, long target_seq_stride, const uint8_t* snitch_occl_by_ptr,
                                   const float* frame_w, const int* pos_count, int class_balancing, float hard_negative_factor, float* weights, void* ws,
                                   size_t ws_bytes) {
    TCOW_CHECK_ARG(n_seq > 0 && T > 0 && H > 0 && W > 0 && target_ch0 && snitch_occl_by_ptr && frame_w && weights, "tcow_snitch_weights: bad arguments");
    TCOW_CHECK_ARG(!class_balancing || pos_count, "tcow_snitch_weights: class balancing needs the positive-pixel count");
    const long frames = n_seq * T;
    TCOW_CHECK_ARG(frames < 65536, "tcow_snitch_weights: too many frames for one call");
    hipStream_t st = (hipStream_t)stream;
    int k = (int)(sqrt((double)H * (double)W) / 12.0);                       // loss.py:138-140
    if (k % 2 == 0) k += 1;
    const int r = k / 2;
    uint8_t* tmp = (uint8_t*)ws;
    const int gx = cdiv((long)H * W, 256 * 8) < 1 ? 1 : cdiv((long)H * W, 256 * 8);
    const bool band = hard_negative_factor > 1.f;
    const bool bitrows = band && W % 64 == 0 && r <= 31 && ((long)H * W) % 256 == 0;     // (2r + 1 <= 64 rows in one wave; whole waves inside the frame)
    if (band) {
        TCOW_CHECK_ARG(ws && ws_bytes >= tcow_snitch_weights_workspace_bytes(frames, H, W), "tcow_snitch_weights: workspace too small");
        if (bitrows) hipLaunchKernelGGL(dilate_rows_bits_kernel, dim3(cdiv(H, 4), (unsigned)frames), dim3(256), 0, st, target_ch0, (long)H * W, T, target_seq_stride, H, W, r,
                                        (unsigned long long*)ws);
        else hipLaunchKernelGGL(dilate_rows_kernel, dim3(gx, (unsigned)frames), dim3(256), 0, st, target_ch0, (long)H * W, T, target_seq_stride, H, W, r, tmp);
        TCOW_CHECK_LAUNCH();
    }
    WeightsArgs a;
    a.target = target_ch0; a.frame_stride_t = (long)H * W; a.frames_per_seq = T; a.seq_stride_t = target_seq_stride; a.ptr = snitch_occl_by_ptr; a.rowdil = tmp; a.rowbits = bitrows ? (const unsigned long long*)ws : nullptr;
    a.frame_w = frame_w; a.pos_count = pos_count; a.out = weights; a.H = H; a.W = W; a.r = r; a.n_pixels = frames * H * W; a.class_balancing = class_balancing;
    a.hard_negative_factor = band ? hard_negative_factor : 1.f;
    hipLaunchKernelGGL(snitch_weights_kernel, dim3(gx, (unsigned)frames), dim3(256), 0, st, a);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
