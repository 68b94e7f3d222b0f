// Caller row L: the per-channel mask objective of loss.py:164-225 as one forward+backward pass family.
//
//   loss = [ aot * (boot + jac) / 2 + (1 - aot) * mean(w * bce) ] * sqrt(n_sel / n)           loss.py:196-222
//   boot = mean(top-k of (w *) bce), k = int(topk_frac * n_sel)                               loss.py:13-17
//   jac  = 1 - sum(p g) / (sum(p g) + sum(p (1-g)) + sum((1-p) g) + 0.1)   (or = boot)        loss.py:20-32
//
// Everything the reference decides on the host (which frames carry weight, mean weight >= 1e-4, empty target, k == n)
// is decided on the device from a control block, so the step has no host synchronisation.  The k-th largest loss value
// is found exactly by an 11/11/9-bit radix select over the float bit pattern (loss values are >= 0, so the unsigned
// pattern orders like the value); elements equal to the k-th value share the remaining weight equally (a valid
// sub-gradient where torch.topk picks an arbitrary subset of the ties).
// Pass A and the gradient pass stream x, t, w once (12 B/pixel; + 4 B/pixel written: the loss values' bit patterns / the gradient); the two
// radix passes in between read only those bit patterns (4 B/pixel, no arithmetic -- round 5: they recomputed the loss from x, t, w before).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVecPerBlock = 1024;          // float4 groups per workgroup (4 per thread)
constexpr int kBins12 = 2048, kBins3 = 512;
constexpr int kNPart = 6;

struct MlView {
    const float* x; long xs;
    const float* t; long ts;
    const float* pw;                        // dense [n_frames * frame_len] or null
    const float* fw;                        // [n_frames] or null
    float* dx; long dxs;
    int T; int L4; int n_frames; int weighted;
    int focal;                              // loss.py:49-51: sigmoid focal loss (alpha 0.25, gamma 2) in place of the plain BCE term
};

struct MlCtl {
    long n_sel, n_all, k, above, cnt_eq, r;
    int valid, mode_all, jac_valid, pad;
    unsigned b1, b2, tau, pad2;
    double S[kNPart];
    double topk_sum;
};

struct MlWs {
    int* fsel; double* fwsum; double* part; unsigned* hist; MlCtl* ctl; int nblk;
    unsigned* vb;                           // [n_frames * frame_len] bit patterns of the (weighted) loss values: written by pass A, read by the radix passes
};

// Up to kMaxJobs channels of the objective as ONE set of launches (round 5: the three channels of a step were 30 launches of 2-40 us each; the
// workgroups of a pass now carry their job in blockIdx.z, the one-workgroup kernels run one workgroup per job): job = one tcow_mask_loss call.
constexpr int kMaxJobs = 4;
struct MlJob { MlView v; MlWs ws; float aot, lw; double topk_frac; float* loss; int radix; };
struct MlBatch { int n; float* total; MlJob j[kMaxJobs]; };

// bce-with-logits and sigmoid of one pixel; identical instruction sequence in every pass (the radix passes rely on it)
__device__ __forceinline__ void bce_sig(float x, float t, float& bce, float& p) {
    const float e = expf(-fabsf(x));
    const float inv = 1.0f / (1.0f + e);
    p = x >= 0.0f ? inv : e * inv;
    bce = fmaxf(x, 0.0f) - x * t + log1pf(e);
}

// The per-pixel loss value and its derivative d(value)/d(logit).  focal = 0: BCE, derivative p - t.  focal = 1 (train_args.focal_loss, loss.py:49-51 =
// torchvision.ops.sigmoid_focal_loss with its defaults alpha = 0.25, gamma = 2, reduction 'none'): value = a_t (1 - p_t)^2 bce with
// p_t = p t + (1 - p)(1 - t), a_t = 0.25 t + 0.75 (1 - t); derivative a_t (1 - p_t) [(1 - p_t)(p - t) - 2 p (1 - p)(2 t - 1) bce].  One instruction
// sequence for every pass (the radix select compares bit patterns of the value across passes).
__device__ __forceinline__ void pix_loss(float x, float t, int focal, float& val, float& dval, float& p) {
    float bce; bce_sig(x, t, bce, p);
    if (!focal) { val = bce; dval = p - t; return; }
    const float pt = p * t + (1.0f - p) * (1.0f - t), at = 0.25f * t + 0.75f * (1.0f - t), q = 1.0f - pt;
    val = at * bce * (q * q);
    dval = at * q * (q * (p - t) - 2.0f * p * (1.0f - p) * (2.0f * t - 1.0f) * bce);
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) s += red[i];
    return s;
}

__device__ __forceinline__ long elem_off(const MlView& v, int f, long stride) {
    const int s = f / v.T;
    return (long)s * stride + (long)(f - s * v.T) * v.L4 * 4;
}

// ---- pass 0: which frames carry weight (loss.py:176-181) and the sum of the weights (loss.py:184)
__device__ __forceinline__ void ml_frames_body(const MlView& v, const MlWs& ws) {
    __shared__ double red[kThreads / 64];
    const int f = blockIdx.x;
    const float fwv = v.fw ? v.fw[f] : 1.0f;
    double sum = 0.0; int any = 0;
    if (v.pw) {
        const float4* pw = reinterpret_cast<const float4*>(v.pw + (long)f * v.L4 * 4);
        float s = 0.f;
        for (int i = threadIdx.x; i < v.L4; i += kThreads) {
            float4 w = pw[i];
            w.x *= fwv; w.y *= fwv; w.z *= fwv; w.w *= fwv;
            any |= (w.x != 0.f) | (w.y != 0.f) | (w.z != 0.f) | (w.w != 0.f);
            s += (w.x + w.y) + (w.z + w.w);
        }
        sum = s;
    } else if (threadIdx.x == 0) {
        any = fwv != 0.f; sum = (double)fwv * (v.L4 * 4.0);
    }
    sum = block_sum(sum, red);
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) { ws.fsel[f] = any; ws.fwsum[f] = sum; }
}

// ---- control: n_sel, validity, k; clears the histograms
__device__ __forceinline__ void ml_ctl_body(const MlView& v, const MlWs& ws, double topk_frac) {
    __shared__ double red[kThreads / 64];
    double nf = 0.0, wsum = 0.0;
    for (int f = threadIdx.x; f < v.n_frames; f += kThreads) { nf += ws.fsel[f] ? 1.0 : 0.0; wsum += ws.fwsum[f]; }
    nf = block_sum(nf, red); wsum = block_sum(wsum, red);
    for (int i = threadIdx.x; i < 2 * kBins12 + kBins3; i += kThreads) ws.hist[i] = 0u;
    if (threadIdx.x == 0) {
        MlCtl c = {};
        c.n_all = (long)v.n_frames * v.L4 * 4;
        c.n_sel = (long)nf * v.L4 * 4;
        const float wmean = (float)(wsum / (double)c.n_all);
        c.valid = c.n_sel > 0 && wmean >= 1e-4f;                           // loss.py:184
        c.k = (long)(topk_frac * (double)c.n_sel);                         // loss.py:14
        c.mode_all = c.k >= c.n_sel;
        *ws.ctl = c;
    }
}

// Iterates this workgroup's float4 groups of frame blockIdx.y; F(x4, t4, w4, offset into the frame in elements)
template <typename F> __device__ __forceinline__ void for_each_vec(const MlView& v, int f, F&& fn) {
    const float4* x = reinterpret_cast<const float4*>(v.x + elem_off(v, f, v.xs));
    const float4* t = reinterpret_cast<const float4*>(v.t + elem_off(v, f, v.ts));
    const float4* pw = v.pw ? reinterpret_cast<const float4*>(v.pw + (long)f * v.L4 * 4) : nullptr;
    const float fwv = v.fw ? v.fw[f] : 1.0f;
    const int base = blockIdx.x * kVecPerBlock;
#pragma unroll
    for (int j = 0; j < kVecPerBlock / kThreads; ++j) {
        const int i = base + j * kThreads + threadIdx.x;
        if (i < v.L4) {
            float4 w = pw ? pw[i] : make_float4(1.f, 1.f, 1.f, 1.f);
            w.x *= fwv; w.y *= fwv; w.z *= fwv; w.w *= fwv;
            fn(x[i], t[i], w, i);
        }
    }
}

__device__ __forceinline__ unsigned vbits(float bce, float w, int weighted) {
    const unsigned u = __builtin_bit_cast(unsigned, weighted ? bce * w : bce);
    return (int)u < 0 ? 0u : u;                 // (-0 / rounding below zero with soft targets) orders as zero
}

// ---- pass A: sums for the three terms + level-1 histogram of the loss values
__device__ __forceinline__ void ml_stats_body(const MlView& v, const MlWs& ws, int radix) {
    __shared__ unsigned hist[kBins12];
    __shared__ double red[kThreads / 64];
    const int f = blockIdx.y;
    const MlCtl* c = ws.ctl;
    const bool live = c->valid && ws.fsel[f];
    const bool need_hist = live && !c->mode_all && radix;      // (no radix select -- topk_frac = 1 or aot_loss = 0 --: no histogram, and the workspace has no bit-pattern image)
    if (need_hist) { for (int i = threadIdx.x; i < kBins12; i += kThreads) hist[i] = 0u; }
    __syncthreads();
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        uint4* vbo = need_hist ? reinterpret_cast<uint4*>(ws.vb + (long)f * v.L4 * 4) : nullptr;
        for_each_vec(v, f, [&](float4 x, float4 t, float4 w, int i) {
            const float xs[4] = {x.x, x.y, x.z, x.w}, ts[4] = {t.x, t.y, t.z, t.w}, wv[4] = {w.x, w.y, w.z, w.w};
            unsigned vbs[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float bce, dval, p; pix_loss(xs[e], ts[e], v.focal, bce, dval, p);
                const unsigned vb = vbits(bce, wv[e], v.weighted);
                vbs[e] = vb;
                s[0] += bce * wv[e]; s[1] += __builtin_bit_cast(float, vb);
                s[2] += p * ts[e]; s[3] += p; s[4] += ts[e];
                if (need_hist) atomicAdd(&hist[vb >> 20], 1u);
            }
            // the radix passes that follow only need the bit patterns: 4 B/pixel instead of x, t, w again (12 B/pixel) and no arithmetic
            if (vbo) vbo[i] = make_uint4(vbs[0], vbs[1], vbs[2], vbs[3]);
        });
    }
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    for (int q = 0; q < 5; ++q) {
        const double tot = block_sum((double)s[q], red);
        if (threadIdx.x == 0) ws.part[(long)blk * kNPart + q] = tot;
    }
    if (need_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < kBins12; i += kThreads)
            if (hist[i]) atomicAdd(&ws.hist[i], hist[i]);
    }
}

// ---- levels 2 and 3 of the radix select: histogram the next digit of the values that share the known prefix
template <int LEVEL> __device__ __forceinline__ void ml_hist_body(const MlView& v, const MlWs& ws) {
    __shared__ unsigned hist[kBins12];
    const int f = blockIdx.y;
    const MlCtl* c = ws.ctl;
    if (!(c->valid && ws.fsel[f]) || c->mode_all) return;
    constexpr int NB = LEVEL == 2 ? kBins12 : kBins3;
    for (int i = threadIdx.x; i < NB; i += kThreads) hist[i] = 0u;
    __syncthreads();
    const unsigned prefix = LEVEL == 2 ? c->b1 : ((c->b1 << 11) | c->b2);
    const uint4* vbi = reinterpret_cast<const uint4*>(ws.vb + (long)f * v.L4 * 4);          // pass A's bit patterns of this frame
    const int base = blockIdx.x * kVecPerBlock;
#pragma unroll
    for (int j = 0; j < kVecPerBlock / kThreads; ++j) {
        const int i = base + j * kThreads + threadIdx.x;
        if (i >= v.L4) continue;
        const uint4 q = vbi[i];
        const unsigned vbs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned vb = vbs[e];
            if (LEVEL == 2) { if ((vb >> 20) == prefix) atomicAdd(&hist[(vb >> 9) & 2047u], 1u); }
            else            { if ((vb >> 9) == prefix) atomicAdd(&hist[vb & 511u], 1u); }
        }
    }
    __syncthreads();
    unsigned* gh = ws.hist + (LEVEL == 2 ? kBins12 : 2 * kBins12);
    for (int i = threadIdx.x; i < NB; i += kThreads)
        if (hist[i]) atomicAdd(&gh[i], hist[i]);
}

// ---- one wave walks a histogram from the top for the bin holding the (k - above)-th largest value;
//      level 1 also folds the pass-A partial sums (fixed order: deterministic)
template <int LEVEL> __device__ __forceinline__ void ml_scan_body(const MlView& v, const MlWs& ws) {
    __shared__ double red[kThreads / 64];
    MlCtl* c = ws.ctl;
    if (LEVEL == 1) {
        for (int q = 0; q < 5; ++q) {
            double s = 0.0;
            for (int b = threadIdx.x; b < ws.nblk; b += kThreads) s += ws.part[(long)b * kNPart + q];
            s = block_sum(s, red);
            if (threadIdx.x == 0) c->S[q] = s;
        }
        if (threadIdx.x == 0) {
            const float tmean = c->n_sel > 0 ? (float)(c->S[4] / (double)c->n_sel) : 0.f;
            c->jac_valid = !v.weighted && tmean >= 1e-6f;                  // loss.py:21
        }
    }
    if (!c->valid || c->mode_all || threadIdx.x >= 64) return;
    constexpr int NB = LEVEL == 3 ? kBins3 : kBins12;
    constexpr int PER = NB / 64;
    const unsigned* h = ws.hist + (LEVEL == 1 ? 0 : LEVEL == 2 ? kBins12 : 2 * kBins12);
    const long krem = c->k - (LEVEL == 1 ? 0 : c->above);
    const int lane = threadIdx.x;
    long mine = 0;
    for (int i = 0; i < PER; ++i) mine += h[lane * PER + i];
    long incl = mine;                                                     // inclusive suffix sum over lanes >= lane
    for (int o = 1; o < 64; o <<= 1) {
        const long up = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl += up;
    }
    const long above_lane = incl - mine;
    if (above_lane < krem && krem <= incl) {                               // exactly one lane
        long acc = above_lane;
        for (int b = lane * PER + PER - 1; b >= lane * PER; --b) {
            const long hb = h[b];
            if (acc + hb >= krem) {
                const long above = (LEVEL == 1 ? 0 : c->above) + acc;
                c->above = above;
                if (LEVEL == 1) c->b1 = (unsigned)b;
                else if (LEVEL == 2) c->b2 = (unsigned)b;
                else { c->tau = (c->b1 << 20) | (c->b2 << 9) | (unsigned)b; c->cnt_eq = hb; c->r = c->k - above; }
                break;
            }
            acc += hb;
        }
    }
}

// ---- pass E: gradient of the channel loss w.r.t. the logits + the top-k sum
__device__ __forceinline__ void ml_grad_body(const MlView& v, const MlWs& ws, float aot, float lw) {
    __shared__ double red[kThreads / 64];
    const int f = blockIdx.y;
    const MlCtl* c = ws.ctl;
    const bool live = c->valid && ws.fsel[f];
    float4* dx = v.dx ? reinterpret_cast<float4*>(v.dx + elem_off(v, f, v.dxs)) : nullptr;
    float tk = 0.f;
    if (!live) {
        if (dx) {
            const int base = blockIdx.x * kVecPerBlock;
            for (int j = 0; j < kVecPerBlock / kThreads; ++j) {
                const int i = base + j * kThreads + threadIdx.x;
                if (i < v.L4) dx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    } else {
        const float sf = lw * sqrtf((float)((double)c->n_sel / (double)c->n_all));     // loss.py:222
        const float inv_n = (float)(1.0 / (double)c->n_sel);
        const float inv_k = c->k > 0 ? (float)(1.0 / (double)c->k) : 0.f;
        const float c_custom = aot > 0.f ? sf * (1.f - aot) * inv_n : sf * inv_n;
        const float c_boot = aot > 0.f ? sf * aot * (v.weighted ? 1.f : 0.5f) * inv_k : 0.f;
        const float c_jac = (aot > 0.f && c->jac_valid) ? sf * aot * 0.5f : 0.f;
        const float num = (float)c->S[2];
        const float D = (float)(c->S[3] + c->S[4] - c->S[2]) + 0.1f;                  // num + sum p(1-g) + sum (1-p)g + eps
        const float invD2 = 1.f / (D * D);
        const int mode_all = c->mode_all || aot <= 0.f;
        const unsigned tau = c->tau;
        const float tie = (mode_all || c->cnt_eq <= 0) ? 1.f : (float)((double)c->r / (double)c->cnt_eq);
        for_each_vec(v, f, [&](float4 x, float4 t, float4 w, int i) {
            const float xs[4] = {x.x, x.y, x.z, x.w}, ts[4] = {t.x, t.y, t.z, t.w}, wv[4] = {w.x, w.y, w.z, w.w};
            float g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float bce, d, p; pix_loss(xs[e], ts[e], v.focal, bce, d, p);
                const unsigned vb = vbits(bce, wv[e], v.weighted);
                const float sel = mode_all ? 1.f : (vb > tau ? 1.f : (vb == tau ? tie : 0.f));
                tk += sel * __builtin_bit_cast(float, vb);
                float gr = c_custom * wv[e] * d + c_boot * sel * (v.weighted ? wv[e] : 1.f) * d;
                const float dJ = -(ts[e] * D - num * (1.f - ts[e])) * invD2;
                gr += c_jac * dJ * p * (1.f - p);
                g[e] = gr;
            }
            if (dx) dx[i] = make_float4(g[0], g[1], g[2], g[3]);
        });
    }
    const double tot = block_sum((double)tk, red);
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) ws.part[(long)blk * kNPart + 5] = tot;
}

// ---- final: the scalar
__device__ __forceinline__ void ml_final_body(const MlView& v, const MlWs& ws, float aot, float loss_weight, float* loss, float* total) {
    __shared__ double red[kThreads / 64];
    MlCtl* c = ws.ctl;
    double s = 0.0;
    for (int b = threadIdx.x; b < ws.nblk; b += kThreads) s += ws.part[(long)b * kNPart + 5];
    s = block_sum(s, red);
    if (threadIdx.x != 0) return;
    c->topk_sum = s;
    float L = 0.f;
    if (c->valid) {
        const double n = (double)c->n_sel;
        const float custom = (float)(c->S[0] / n);
        if (aot > 0.f) {
            const float boot = c->mode_all ? (float)(c->S[1] / n) : (float)(s / (double)c->k);
            float jac = boot;
            if (!v.weighted) {
                const float num = (float)c->S[2];
                const float den = (float)(c->S[3] + c->S[4] - c->S[2]);
                jac = c->jac_valid ? 1.f - num / (den + 0.1f) : 0.f;
            }
            L = (boot + jac) / 2.f * aot + custom * (1.f - aot);
        } else {
            L = custom;
        }
        L *= sqrtf((float)(n / (double)c->n_all));
    }
    *loss = L;
    if (total) *total += loss_weight * L;
}

// ---- the launches: one per pass for all jobs of a batch
__global__ void __launch_bounds__(kThreads) ml_frames_kernel(MlBatch b) { const MlJob& J = b.j[blockIdx.y]; ml_frames_body(J.v, J.ws); }
__global__ void __launch_bounds__(kThreads) ml_ctl_kernel(MlBatch b) { const MlJob& J = b.j[blockIdx.x]; ml_ctl_body(J.v, J.ws, J.topk_frac); }
__global__ void __launch_bounds__(kThreads) ml_stats_kernel(MlBatch b) { const MlJob& J = b.j[blockIdx.z]; ml_stats_body(J.v, J.ws, J.radix); }
template <int LEVEL> __global__ void __launch_bounds__(kThreads) ml_hist_kernel(MlBatch b) { const MlJob& J = b.j[blockIdx.z]; if (J.radix) ml_hist_body<LEVEL>(J.v, J.ws); }
template <int LEVEL> __global__ void __launch_bounds__(kThreads) ml_scan_kernel(MlBatch b) { const MlJob& J = b.j[blockIdx.x]; if (LEVEL == 1 || J.radix) ml_scan_body<LEVEL>(J.v, J.ws); }
__global__ void __launch_bounds__(kThreads) ml_grad_kernel(MlBatch b) { const MlJob& J = b.j[blockIdx.z]; ml_grad_body(J.v, J.ws, J.aot, J.lw); }
// (one workgroup walks the jobs in order: `total` is accumulated in job order, as the one-launch-per-channel form did)
__global__ void __launch_bounds__(kThreads) ml_final_kernel(MlBatch b) {
    for (int i = 0; i < b.n; ++i) { const MlJob& J = b.j[i]; ml_final_body(J.v, J.ws, J.aot, J.lw, J.loss, b.total); __syncthreads(); }
}

static int ml_nblk(long n_frames, long frame_len) { return (int)(n_frames * ((frame_len / 4 + kVecPerBlock - 1) / kVecPerBlock)); }

// The workspace of one job: byte offset of every region of MlWs and the total.  The one place that knows the layout -- the size functions return
// `total`, ml_make_job carves by the offsets.
struct MlLayout { size_t fsel, fwsum, part, hist, ctl, vb, total; };
static MlLayout ml_layout(long n_frames, long frame_len, bool radix) {
    const auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    MlLayout o = {};
    o.fwsum = o.fsel + pad((size_t)n_frames * sizeof(int));
    o.part = o.fwsum + pad((size_t)n_frames * sizeof(double));
    o.hist = o.part + pad((size_t)ml_nblk(n_frames, frame_len) * kNPart * sizeof(double));
    o.ctl = o.hist + (2 * kBins12 + kBins3) * sizeof(unsigned);
    static_assert(sizeof(MlCtl) <= 512, "control block");
    o.vb = o.ctl + 512;
    o.total = o.vb + (radix ? (size_t)n_frames * (size_t)frame_len * sizeof(unsigned) : 0);      // the loss values' bit patterns between pass A and the radix passes
    return o;
}
static size_t ml_ws_bytes(long n_frames, long frame_len, bool radix) { return n_frames <= 0 || frame_len <= 0 ? 0 : ml_layout(n_frames, frame_len, radix).total; }

}  // namespace

extern "C" {

size_t tcow_mask_loss_workspace_bytes(long n_frames, long frame_len) { return ml_ws_bytes(n_frames, frame_len, true); }
size_t tcow_mask_loss_workspace_bytes_for(long n_frames, long frame_len, double topk_frac, float aot_loss) { return ml_ws_bytes(n_frames, frame_len, topk_frac < 1.0 && aot_loss > 0.f); }

static int ml_make_job(const tcow_mask_loss_args* a, MlJob& J) {
    TCOW_CHECK_ARG(a && a->logits && a->target && a->loss && a->ws, "tcow_mask_loss: null argument");
    TCOW_CHECK_ARG(a->n_frames > 0 && a->frame_len > 0 && a->frames_per_seq > 0 && a->n_frames % a->frames_per_seq == 0,
                   "tcow_mask_loss: bad frame counts");
    TCOW_CHECK_ARG(a->frame_len % 4 == 0, "tcow_mask_loss: frame_len %ld must be a multiple of 4", a->frame_len);
    TCOW_CHECK_ARG(a->logits_seq_stride % 4 == 0 && a->target_seq_stride % 4 == 0 && a->dlogits_seq_stride % 4 == 0,
                   "tcow_mask_loss: sequence strides must be multiples of 4 elements");
    TCOW_CHECK_ARG(a->n_frames * (a->frame_len / 4) < (1L << 31) && a->n_frames < 65536, "tcow_mask_loss: too many pixels for one call");
    TCOW_CHECK_ARG(a->topk_frac > 0.0 && a->topk_frac <= 1.0, "tcow_mask_loss: topk_frac %g outside (0, 1]", a->topk_frac);
    TCOW_CHECK_ARG(a->ws_bytes >= tcow_mask_loss_workspace_bytes_for(a->n_frames, a->frame_len, a->topk_frac, a->aot_loss), "tcow_mask_loss: workspace too small");
    MlView& v = J.v;
    v.x = a->logits; v.xs = a->logits_seq_stride; v.t = a->target; v.ts = a->target_seq_stride;
    v.pw = a->pixel_w; v.fw = a->frame_w; v.dx = a->dlogits; v.dxs = a->dlogits_seq_stride;
    v.T = (int)a->frames_per_seq; v.L4 = (int)(a->frame_len / 4); v.n_frames = (int)a->n_frames; v.weighted = a->weighted_aot ? 1 : 0; v.focal = a->focal ? 1 : 0;
    J.aot = a->aot_loss; J.lw = a->loss_weight; J.topk_frac = a->topk_frac; J.loss = a->loss;
    J.radix = (a->topk_frac < 1.0 && a->aot_loss > 0.f) ? 1 : 0;
    const MlLayout o = ml_layout(a->n_frames, a->frame_len, J.radix);
    MlWs& ws = J.ws; char* p = (char*)a->ws;
    ws.fsel = (int*)(p + o.fsel); ws.fwsum = (double*)(p + o.fwsum); ws.part = (double*)(p + o.part); ws.hist = (unsigned*)(p + o.hist);
    ws.ctl = (MlCtl*)(p + o.ctl); ws.vb = (unsigned*)(p + o.vb); ws.nblk = ml_nblk(a->n_frames, a->frame_len);
    return TCOW_OK;
}

// n <= 4 channels of one objective in one set of launches: the same frame geometry, the same `total` (may be NULL) -- accumulated in argument
// order --, separate workspaces.
int tcow_mask_loss_batch(void* stream, const tcow_mask_loss_args* a, int n) {
    TCOW_CHECK_ARG(a && n >= 1 && n <= kMaxJobs, "tcow_mask_loss_batch: 1 .. %d jobs (got %d)", kMaxJobs, n);
    MlBatch b; b.n = n; b.total = a[0].total;
    int any_radix = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = ml_make_job(a + i, b.j[i]);
        if (rc != TCOW_OK) return rc;
        TCOW_CHECK_ARG(a[i].n_frames == a[0].n_frames && a[i].frame_len == a[0].frame_len && a[i].total == a[0].total,
                       "tcow_mask_loss_batch: the jobs of a batch share n_frames, frame_len and total");
        for (int k = 0; k < i; ++k) TCOW_CHECK_ARG(a[k].ws != a[i].ws, "tcow_mask_loss_batch: every job needs its own workspace");
        any_radix |= b.j[i].radix;
    }
    for (int i = n; i < kMaxJobs; ++i) b.j[i] = b.j[0];
    hipStream_t st = (hipStream_t)stream;
    const MlView& v = b.j[0].v;
    const dim3 grid((v.L4 + kVecPerBlock - 1) / kVecPerBlock, v.n_frames, n);
    ml_frames_kernel<<<dim3(v.n_frames, n), kThreads, 0, st>>>(b);
    ml_ctl_kernel<<<n, kThreads, 0, st>>>(b);
    ml_stats_kernel<<<grid, kThreads, 0, st>>>(b);
    ml_scan_kernel<1><<<n, kThreads, 0, st>>>(b);
    if (any_radix) {
        ml_hist_kernel<2><<<grid, kThreads, 0, st>>>(b);
        ml_scan_kernel<2><<<n, kThreads, 0, st>>>(b);
        ml_hist_kernel<3><<<grid, kThreads, 0, st>>>(b);
        ml_scan_kernel<3><<<n, kThreads, 0, st>>>(b);
    }
    ml_grad_kernel<<<grid, kThreads, 0, st>>>(b);
    ml_final_kernel<<<1, kThreads, 0, st>>>(b);
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_mask_loss(void* stream, const tcow_mask_loss_args* a) { return tcow_mask_loss_batch(stream, a, 1); }

}  // extern "C"
