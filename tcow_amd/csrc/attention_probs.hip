// Attention maps (tcow_attn_probs): the softmax rows that the flash kernels never store, recomputed from a block's stored q and k.  The qkv
// GEMM output [rows, 3D] is read as it is (the 16-bit type of the build, or f32); products, sums, maximum, exp and normalisation are f32 in a
// fixed order, nothing is atomic: the output is a fixed function of the inputs.  This is "the softmax of the q and k the model computed", not a
// replay of a flash kernel's own score rounding (include/tcow_hip.h).  Replaces, for inspection, attn.softmax(dim=-1) of vit.py:88-101.
//
// probs_temporal_kernel: one wave per (clip b, slot s >= 1, head h), AP_WAVES waves per workgroup, no LDS.  LANE = KEY: in a trip of AP_TKEYS = 64
// keys lane l owns key frame k0 + l and holds its 64 channels in registers (16-byte loads of its own K row, rows S * 3D elements apart), so with
// T <= 64 -- one trip, the workload's T = 30 -- K is read once per (b, s, h) and every query frame reuses the registers.  A query row is the same
// address in every lane (a broadcast load).  The wave's maximum and sum are xor-shuffle trees.  A longer T loops over trips: pass one leaves the
// raw scaled scores in the wave's own output row while every lane keeps an online (max, sum) of its keys, pass two re-reads them (each lane the
// addresses it wrote) and normalises.  Rows of T % 4 == 0 floats on a 16-byte aligned `out` leave in 16-byte stores (four lanes' values
// gathered by shuffles), the others in coalesced 4-byte stores.  A masked entry is stored as +0.0.
// probs_rows_kernel: one wave per (sequence g, table entry i, head h): a GEMV of one query against the S slots of its frame (or the 1 + N T
// tokens of a joint sequence), on the lane groups of temporal_cached_kernel (attention_stream.hip): LPR lanes read one head line with a 16-byte
// load each, G = 64 / LPR keys per load, AP_U batches in flight, scores reduced over a group's lanes by xor shuffles.  After the reduction every
// lane of a group holds the score, so lane `u` of the group stores that of batch u: pass two (exp, scale, in place) then runs on AP_U lanes per
// group, each re-reading only what it wrote itself -- no fence, no barrier.
#include <math.h>

#include "attention_stream_cache.h"

namespace {

constexpr int AP_WAVES = 4;      // waves (items) per workgroup
constexpr int AP_TKEYS = 64;     // temporal form: keys per trip (one per lane)
constexpr int AP_U = 4;          // rows form: batches of G keys loaded before they are used

// q . k over the 64 channels of a head, channel order, f32 fused multiply-adds; the query line is the same for every lane
template <typename T>
__device__ __forceinline__ float dot_head(const T* __restrict__ qrow, const float* kreg) {
    constexpr int VEC = StreamVec<T>::VEC;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < ATT_HD; c += VEC) {
        float q[VEC];
        StreamVec<T>::ld(qrow + c, q);
#pragma unroll
        for (int e = 0; e < VEC; ++e) d = fmaf(q[e], kreg[c + e], d);
    }
    return d;
}

template <typename T>
__global__ __launch_bounds__(64 * AP_WAVES) void probs_temporal_kernel(int B, int nT, int S, int D, int heads, int diag, int vec_rows,
                                                                      const T* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse) {
    constexpr int VEC = StreamVec<T>::VEC;
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * AP_WAVES + (threadIdx.x >> 6);
    if (item >= (long)B * (S - 1) * heads) return;
    const int h = (int)(item % heads);
    const long bs = item / heads;
    const int s = 1 + (int)(bs % (S - 1)), b = (int)(bs / (S - 1));
    const long ld3 = 3L * D, fstride = (long)S * ld3;            // elements between two frames of one slot
    const T* base = qkv + ((long)b * nT * S + s) * ld3 + h * ATT_HD;
    float* orow = out + (size_t)item * nT * nT;
    const bool single = nT <= AP_TKEYS;
    const float scale = 0.125f;                                   // head_dim ** -0.5 (vit.py:74)
    float kreg[ATT_HD];
    for (int tq = 0; tq < nT; ++tq) {
        const T* qrow = base + tq * fstride;
        float* prow = orow + (size_t)tq * nT;
        const long klim = (long)tq + diag;                        // key allowed iff kt <= tq + diag
        float m = -INFINITY, l = 0.f, sreg = -INFINITY;
        for (int k0 = 0; k0 < nT; k0 += AP_TKEYS) {
            const int kt = k0 + lane;
            if (!single || tq == 0) {                             // (one trip: the registers of tq == 0 serve every query)
                if (kt < nT) {
                    const T* krow = base + kt * fstride + D;
#pragma unroll
                    for (int c = 0; c < ATT_HD; c += VEC) StreamVec<T>::ld(krow + c, kreg + c);
                } else {
#pragma unroll
                    for (int c = 0; c < ATT_HD; ++c) kreg[c] = 0.f;
                }
            }
            const bool ok = kt < nT && kt <= klim;
            const float sc = ok ? dot_head<T>(qrow, kreg) * scale : -INFINITY;
            if (single) sreg = sc; else if (kt < nT) prow[kt] = sc;
            if (ok) {
                const float mn = fmaxf(m, sc);
                l = l * expf(m - mn) + expf(sc - mn);             // (m == -inf: l == 0 and expf(-inf) == 0)
                m = mn;
            }
        }
        // every query sees key 0 at least (diag >= 0), so the maximum is finite
        const float M = wave_max(m);
        const float Z = wave_sum(m == -INFINITY ? 0.f : l * expf(m - M));
        const float inv = 1.f / Z;
        if (lse && lane == 0) lse[((long)(b * nT + tq) * S + s) * heads + h] = M + logf(Z);
        for (int k0 = 0; k0 < nT; k0 += AP_TKEYS) {
            const int kt = k0 + lane;
            const bool ok = kt < nT && kt <= klim;
            float sc = sreg;
            if (!single) sc = ok ? prow[kt] : -INFINITY;          // (the lane's own store of pass one)
            const float p = ok ? expf(sc - M) * inv : 0.f;        // masked: exactly +0.0
            if (vec_rows) {                                       // nT % 4 == 0, out 16-byte aligned: lane j < 16 stores keys k0 + 4j .. + 3
                const int src = (lane & 15) * 4;
                const float4 v = make_float4(__shfl(p, src, 64), __shfl(p, src + 1, 64), __shfl(p, src + 2, 64), __shfl(p, src + 3, 64));
                if (lane < 16 && k0 + src < nT) *reinterpret_cast<float4*>(prow + k0 + src) = v;
            } else if (kt < nT) {
                prow[kt] = p;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * AP_WAVES) void probs_rows_kernel(int G_seq, int nq, int S, int s0, int D, int heads, const int* __restrict__ pos,
                                                                  const T* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC, G = 64 / LPR;
    const int lane = threadIdx.x & 63, grp = lane / LPR, sub = lane - grp * LPR;
    const long item = (long)blockIdx.x * AP_WAVES + (threadIdx.x >> 6);
    if (item >= (long)G_seq * nq * heads) return;
    const int h = (int)(item % heads);
    const long gi = item / heads;
    const int i = (int)(gi % nq), g = (int)(gi / nq);
    const int L = S - s0;
    const int p = __builtin_amdgcn_readfirstlane(pos[i]);
    float* prow = out + (size_t)item * S;
    if (p < 0 || p >= L) {
        // an entry outside the sequence: NaN to its own rows, nothing read (the bad row of tcow_attn_temporal_step)
        for (int c = lane; c < S; c += 64) prow[c] = __builtin_nanf("");
        if (lse && lane == 0) lse[item] = __builtin_nanf("");
        return;
    }
    if (s0 && lane == 0) prow[0] = 0.f;                           // slot 0 takes no part: exactly +0.0
    prow += s0;
    const long ld3 = 3L * D;
    const T* base = qkv + ((long)g * S + s0) * ld3 + h * ATT_HD + sub * VEC;
    const float scale = 0.125f;
    float q[VEC];
    StreamVec<T>::ld(base + p * ld3, q);
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < L; k0 += G * AP_U) {
        float kv[AP_U][VEC];
#pragma unroll
        for (int u = 0; u < AP_U; ++u) {
            const int kt = k0 + u * G + grp;
            if (kt < L) {
                StreamVec<T>::ld(base + kt * ld3 + D, kv[u]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) kv[u][e] = 0.f;
            }
        }
        float sc[AP_U];
        float mb = m;
#pragma unroll
        for (int u = 0; u < AP_U; ++u) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) d = fmaf(q[e], kv[u][e], d);
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
            const int kt = k0 + u * G + grp;
            sc[u] = kt < L ? d * scale : -INFINITY;
            if (sub == u && kt < L) prow[kt] = sc[u];             // lane u of the group keeps batch u's score for pass two
            mb = fmaxf(mb, sc[u]);
        }
        // (a group without a key so far keeps m = -inf, l = 0; a group whose batch is empty keeps mb = m)
        if (mb != -INFINITY) {
            l *= (m == -INFINITY) ? 0.f : expf(m - mb);
#pragma unroll
            for (int u = 0; u < AP_U; ++u) l += (sc[u] == -INFINITY) ? 0.f : expf(sc[u] - mb);
            m = mb;
        }
    }
    // merge the G groups' (m, l): lanes with the same channel slice sit LPR apart (group 0 always has key 0: the result is finite)
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
        const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
        const float mn = fmaxf(m, mo);
        const float a = (m == -INFINITY) ? 0.f : expf(m - mn), bb = (mo == -INFINITY) ? 0.f : expf(mo - mn);
        l = l * a + lo * bb;
        m = mn;
    }
    const float inv = 1.f / l;
    if (lse && lane == 0) lse[item] = m + logf(l);
    if (sub < AP_U) {
        for (int kt = sub * G + grp; kt < L; kt += G * AP_U) prow[kt] = expf(prow[kt] - m) * inv;      // (the lane's own stores of pass one)
    }
}

}  // namespace

extern "C" {

// Every check runs before anything is launched; each has its own text, "<entry point>: <field> ...".
int tcow_attn_probs(void* stream, const tcow_attn_probs_args* args) {
    TCOW_CHECK_ARG(args != nullptr, "tcow_attn_probs: args is NULL");
    const tcow_attn_probs_args& a = *args;
    const tcow_attn_shape& s = a.shape;
    TCOW_CHECK_ARG(s.B >= 1, "tcow_attn_probs: shape.B = %d, must be >= 1", s.B);
    TCOW_CHECK_ARG(s.T >= 1, "tcow_attn_probs: shape.T = %d, must be >= 1", s.T);
    TCOW_CHECK_ARG(s.S >= 2, "tcow_attn_probs: shape.S = %d, must be >= 2", s.S);
    TCOW_CHECK_ARG(s.heads >= 1, "tcow_attn_probs: shape.heads = %d, must be >= 1", s.heads);
    TCOW_CHECK_ARG(s.D == s.heads * ATT_HD, "tcow_attn_probs: shape.D = %d, must be heads * 64 = %d", s.D, s.heads * ATT_HD);
    TCOW_CHECK_ARG(s.dtype == TCOW_F32 || s.dtype == TCOW_BF16 || s.dtype == TCOW_F32X3,
                   "tcow_attn_probs: shape.dtype = %d, must be TCOW_F32, TCOW_BF16 or TCOW_F32X3", s.dtype);
    TCOW_CHECK_ARG(a.form == TCOW_PROBS_TEMPORAL || a.form == TCOW_PROBS_ROWS, "tcow_attn_probs: form = %d, must be TCOW_PROBS_TEMPORAL or TCOW_PROBS_ROWS",
                   a.form);
    TCOW_CHECK_ARG(a.qkv, "tcow_attn_probs: qkv is NULL");
    TCOW_CHECK_ARG(a.out, "tcow_attn_probs: out is NULL");
    const bool rows = a.form == TCOW_PROBS_ROWS;
    long items;
    if (rows) {
        TCOW_CHECK_ARG(a.nq >= 1, "tcow_attn_probs: nq = %d, must be >= 1 in the rows form", a.nq);
        TCOW_CHECK_ARG(a.pos, "tcow_attn_probs: pos is NULL in the rows form");
        items = (long)s.B * s.T * a.nq * s.heads;
    } else {
        TCOW_CHECK_ARG(s.T <= TCOW_STREAM_MAX_FRAMES, "tcow_attn_probs: shape.T = %d, must be <= %d in the temporal form", s.T, TCOW_STREAM_MAX_FRAMES);
        TCOW_CHECK_ARG(a.nq == 0, "tcow_attn_probs: nq = %d, must be 0 in the temporal form", a.nq);
        TCOW_CHECK_ARG(a.pos == nullptr, "tcow_attn_probs: pos must be NULL in the temporal form");
        items = (long)s.B * (s.S - 1) * s.heads;
    }
    TCOW_CHECK_ARG(items <= (long)AP_WAVES * 0x7fffffffL, "tcow_attn_probs: shape asks for %ld waves, more than one grid holds", items);
    const dim3 grid((unsigned)cdiv(items, AP_WAVES)), block(64 * AP_WAVES);
    const hipStream_t st = (hipStream_t)stream;
    const int dtype = s.dtype == TCOW_F32X3 ? TCOW_F32 : s.dtype;        // (bf16x3 stores f32: the f32 kernel)
    TCOW_DISPATCH_STORAGE(dtype, [&](auto t) {
        using T = decltype(t);
        if (rows) {
            const int s0 = (s.causal == 0 || s.causal == 1) ? 0 : 1;     // the sequences of tcow_attn_spatial_fwd (spatial_desc)
            hipLaunchKernelGGL(probs_rows_kernel<T>, grid, block, 0, st, s.B * s.T, a.nq, s.S, s0, s.D, s.heads, a.pos, (const T*)a.qkv, a.out, a.lse);
        } else {
            const int vec_rows = (s.T % 4 == 0 && (uintptr_t)a.out % 16 == 0) ? 1 : 0;
            hipLaunchKernelGGL(probs_temporal_kernel<T>, grid, block, 0, st, s.B, s.T, s.S, s.D, s.heads, diag_from_causal(s.causal), vec_rows,
                               (const T*)a.qkv, a.out, a.lse);
        }
    });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // extern "C"
