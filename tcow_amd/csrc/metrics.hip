// Caller row M: the IoU metrics of eval/metrics.py:19-20,55-113 -- per-frame area counts in one pass over logits and
// targets, then the six masked IoU means and their frame counts from those tables.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------ IoU area counts (caller row M)
// eval/metrics.py:19-20,55-66: per frame, |target|, |output & target|, |output | target| with output = logit > 0 and
// target = value > 0.5.  One pass over both tensors; integer counts, so the result is exact and order-independent.
__global__ void __launch_bounds__(256) iou_counts_kernel(const float* __restrict__ logits, const float* __restrict__ target, int L4, int* __restrict__ counts) {
    __shared__ int red[3][4];
    const int f = blockIdx.x;
    const float4* x = reinterpret_cast<const float4*>(logits) + (size_t)f * L4;
    const float4* t = reinterpret_cast<const float4*>(target) + (size_t)f * L4;
    int ta = 0, in = 0, un = 0;
    for (int i = threadIdx.x; i < L4; i += 256) {
        const float4 xv = x[i], tv = t[i];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ts[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = xs[e] > 0.0f, g = ts[e] > 0.5f;
            ta += g; in += o & g; un += o | g;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { ta += __shfl_xor(ta, o, 64); in += __shfl_xor(in, o, 64); un += __shfl_xor(un, o, 64); }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = ta; red[1][w] = in; red[2][w] = un; }
    __syncthreads();
    if (threadIdx.x < 3) counts[f * 3 + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// eval/metrics.py:55-113 from the per-frame area tables of tcow_iou_counts: the six masked IoU means and their frame counts
__global__ void __launch_bounds__(256) iou_means_kernel(const int* __restrict__ counts, int n_seq, int C, int T, float* __restrict__ mean, int* __restrict__ count) {
    __shared__ double ssum[6][4];
    __shared__ int scnt[6][4];
    double sum[6] = {0., 0., 0., 0., 0., 0.};
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n_seq * T; i += 256) {
        const int sq = i / T, t = i - sq * T;
        double iou[3] = {0., 0., 0.}; bool has[3] = {false, false, false};
        for (int c = 0; c < C && c < 3; ++c) {
            const int* k = counts + (((size_t)sq * C + c) * T + t) * 3;
            iou[c] = (double)k[1] / ((double)k[2] + 1e-7);                 // metrics.py:55-66
            has[c] = k[0] > 0;
        }
        const bool sel[6] = {has[0], has[1], has[2], has[0] && !has[1] && C >= 2, has[0] && has[1], has[0] && has[2]};
        const double val[6] = {iou[0], iou[1], iou[2], iou[0], iou[0], iou[0]};
#pragma unroll
        for (int k = 0; k < 6; ++k) if (sel[k]) { sum[k] += val[k]; ++cnt[k]; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = sum[k]; int c = cnt[k];
        for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
        if ((threadIdx.x & 63) == 0) { ssum[k][threadIdx.x >> 6] = s; scnt[k][threadIdx.x >> 6] = c; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        const double s = (ssum[k][0] + ssum[k][1]) + (ssum[k][2] + ssum[k][3]);
        const int c = scnt[k][0] + scnt[k][1] + scnt[k][2] + scnt[k][3];
        mean[k] = c > 0 ? (float)(s / (double)c) : -1.0f;
        count[k] = c;
    }
}

}  // namespace

extern "C" int tcow_iou_counts(void* stream, const float* logits, const float* target, long n_frames, long frame_len, int* counts) {
    TCOW_CHECK_ARG(logits && target && counts && n_frames > 0 && frame_len > 0, "tcow_iou_counts: bad arguments");
    TCOW_CHECK_ARG(frame_len % 4 == 0 && frame_len / 4 < (1L << 31) && n_frames < (1L << 31), "tcow_iou_counts: frame_len %ld must be a multiple of 4", frame_len);
    hipLaunchKernelGGL(iou_counts_kernel, dim3((unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, logits, target, (int)(frame_len / 4), counts);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

extern "C" int tcow_iou_means(void* stream, const int* counts, int n_seq, int C, int T, float* mean, int* count) {
    TCOW_CHECK_ARG(counts && mean && count && n_seq > 0 && C >= 1 && T > 0, "tcow_iou_means: bad arguments");
    hipLaunchKernelGGL(iou_means_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, n_seq, C, T, mean, count);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
