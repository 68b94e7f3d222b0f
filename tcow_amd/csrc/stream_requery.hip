// Hand-off of a rollover stream pool (tcow_amd/stream.py): the query mask of a session's next window is the model's own
// prediction at the frame where that window starts, binarised as eval/metrics.py:18 does (output_mask > threshold).  One launch turns the
// mask-logit planes of all hand-offs of a step into 0.0 / 1.0 planes and counts their ones, so nothing is read back to the host.
#include "common.h"
#include "internal.h"

namespace {

constexpr int RQ_THREADS = 1024;      // one workgroup per plane: the count is one integer tree, the same for every run

// Workgroup i: mask[dst_rows[i]][e] = logits[src_off[i] + e] > thr ? 1 : 0 for e < plane (NaN and equality give 0), pixels[dst_rows[i]] = the
// number of ones.  A dst row outside [0, n_dst) or a plane outside [0, logits_len) writes nothing.  16-byte loads and stores where both the
// source plane and the destination row start on a 16-byte boundary; any other plane, and the last plane % 4 elements, go element by element.
__global__ void __launch_bounds__(RQ_THREADS) requery_mask_kernel(long plane, const float* __restrict__ logits, long logits_len, const long* __restrict__ src_off,
                                                                  float thr, float* __restrict__ mask, const int* __restrict__ dst_rows, int n_dst,
                                                                  int* __restrict__ pixels) {
    __shared__ int red[RQ_THREADS / 64];
    const int i = blockIdx.x;
    const long off = src_off[i];
    const int row = dst_rows[i];
    if (row < 0 || row >= n_dst || off < 0 || off > logits_len - plane) return;       // (uniform over the workgroup)
    const float* x = logits + off;
    float* y = mask + (long)row * plane;
    int ones = 0;
    long done = 0;                                                                  // elements the vector body covers
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
        const long n4 = plane >> 2;
        for (long q = threadIdx.x; q < n4; q += RQ_THREADS) {
            const float4 v = ld4(x + 4 * q);
            const int a = v.x > thr, b = v.y > thr, c = v.z > thr, d = v.w > thr;
            ones += a + b + c + d;
            st4(y + 4 * q, make_float4((float)a, (float)b, (float)c, (float)d));
        }
        done = n4 << 2;
    }
    for (long e = done + threadIdx.x; e < plane; e += RQ_THREADS) {
        const int a = x[e] > thr;
        ones += a;
        y[e] = (float)a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ones;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < RQ_THREADS / 64; ++w) total += red[w];
        pixels[row] = total;
    }
}

}  // namespace

int tcow_launch_requery_mask(hipStream_t stream, int n, long plane, const float* logits, long logits_len, const long* src_off, float threshold, float* mask,
                             const int* dst_rows, int n_dst, int* pixels) {
    hipLaunchKernelGGL(requery_mask_kernel, dim3((unsigned)n), dim3(RQ_THREADS), 0, stream, plane, logits, logits_len, src_off, threshold, mask, dst_rows, n_dst, pixels);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}
