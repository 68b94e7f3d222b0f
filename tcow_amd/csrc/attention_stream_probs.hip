// Attention maps of a live session (tcow_attn_temporal_step_probs): the softmax row of every frame of a stream step against the session's K
// cache, which the step itself (attention_stream.hip, an online-softmax body that stores no lse) never forms.  The record, its forms, layouts,
// cache types, refusals and bad rows are those of tcow_attn_temporal_step; the caches are only read and `out` is not touched.
//
// step_probs_kernel: one wave per (flat frame f, slot s >= 1, head h) in every form (temporal_ragged_kernel's item decomposition, so a long
// chunk spreads over its frames), ST_WAVES waves per workgroup, no LDS.  The wave's row of T_total floats is item * T_total of `probs`.
// A key's score is computed as temporal_query_frame computes it: the lane groups and batches of attention_stream_cache.h (key kt belongs to
// group (kt % (G * ST_U)) % G of batch (kt % (G * ST_U)) / G), VEC fused multiply-adds per lane, the xor-shuffle tree over the group's LPR lanes,
// d * 0.125f; a cached line is decoded and a line of the step's own qkv rows rounded through C when the cache is compact, q is not rounded.
// The passes are probs_rows_kernel's (attention_probs.hip): pass one leaves each raw score in its place of the wave's row (lane u of a group
// stores batch u's) while every group keeps an online (max, sum), merged by xor shuffles; pass two is exp-and-scale in place, each lane
// re-reading only what it wrote -- no fence, no barrier; then entries t + 1 .. T_total - 1 are written as +0.0 (16-byte stores where rows are
// 16-byte multiples on an aligned buffer, else coalesced 4-byte stores).  Maximum, exp, sum and division are f32 in a fixed order and nothing
// is atomic: a row is a fixed function of (q_t, K_0 .. K_t) -- not of the split into steps, the form or the layout.
// INVARIANT: a wave reads cache positions < t0 only; keys t0 .. t come from the step's qkv rows.  tcow_attn_temporal_step of the same record
// writes positions >= t0 only, so the two may be enqueued in either order.
#include <math.h>

#include "attention_stream_cache.h"
#include "internal.h"

namespace {

enum { FORM_ROWS = 0, FORM_RAGGED = 1, FORM_PAGED = 2 };

// the lane's slice of key kt as f32: a cached line (decoded when the cache is compact) or a line of the step's qkv rows (rounded through C)
template <typename T, typename C> __device__ __forceinline__ void cached_key(const C* p, float* v) {
    if constexpr (std::is_same_v<T, C>) StreamVec<T>::ld(p, v); else CacheVec<T, C>::dec(CacheVec<T, C>::ld(p), v);
}
template <typename T, typename C> __device__ __forceinline__ void own_key(const T* p, float* v) {
    if constexpr (std::is_same_v<T, C>) StreamVec<T>::ld(p, v); else CacheVec<T, C>::dec(encode_line<T, C>(p), v);
}

// The softmax row of chunk frame j (flat frame fb + j, t = t0 + j) over keys 0 .. t into prow[0 .. t]; every lane of the wave calls it.
template <typename T, typename C, typename Keys>
__device__ __forceinline__ void probs_query_frame(const T* qkv, const C* kc, const Keys keys, int fb, int j, int t0, int S, int s, int D, int col, int grp,
                                                  int sub, float* prow) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC, G = 64 / LPR;
    static_assert(ST_U <= LPR, "lane u of a group keeps batch u's score");
    const long ld3 = 3L * D;
    const float scale = 0.125f;      // head_dim ** -0.5 (vit.py:74)
    const int t = t0 + j;
    float q[VEC];
    StreamVec<T>::ld(qkv + ((long)(fb + j) * S + s) * ld3 + col, q);
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 <= t; k0 += G * ST_U) {
        float kv[ST_U][VEC];
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            const int kt = k0 + u * G + grp;
            const auto pg = keys.page(kt <= t ? kt : t);        // (every lane, ahead of the branch)
            if (kt < t0) {
                cached_key<T, C>(keys(kc, pg, kt), kv[u]);
            } else if (kt <= t) {
                own_key<T, C>(qkv + ((long)(fb + kt - t0) * S + s) * ld3 + D + col, kv[u]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) kv[u][e] = 0.f;
            }
        }
        float sc[ST_U];
        float mb = m;
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) d = fmaf(q[e], kv[u][e], d);
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
            const int kt = k0 + u * G + grp;
            sc[u] = kt <= t ? d * scale : -INFINITY;
            if (sub == u && kt <= t) prow[kt] = sc[u];            // lane u of the group keeps batch u's score for pass two
            mb = fmaxf(mb, sc[u]);
        }
        // (a group without a key so far keeps m = -inf, l = 0; a group whose batch is empty keeps mb = m)
        if (mb != -INFINITY) {
            l *= (m == -INFINITY) ? 0.f : expf(m - mb);
#pragma unroll
            for (int u = 0; u < ST_U; ++u) l += (sc[u] == -INFINITY) ? 0.f : expf(sc[u] - mb);
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
    if (sub < ST_U) {
        for (int kt = sub * G + grp; kt <= t; kt += G * ST_U) prow[kt] = expf(prow[kt] - m) * inv;      // (the lane's own stores of pass one)
    }
}

// FORM_ROWS: rows = B sessions of c frames each, t0_rows[b * t0_stride], slot = slot_rows ? slot_rows[b] : b (temporal_cached_kernel's session);
// FORM_RAGGED / FORM_PAGED: rows = n sessions over F frames with the tables of temporal_ragged_kernel / temporal_ragged_paged_kernel.  A frame is
// bad exactly where those kernels say so: its row is NaN and no cache byte is read.
template <typename T, typename C, int FORM>
__global__ __launch_bounds__(64 * ST_WAVES) void step_probs_kernel(int rows, int c_or_F, int S, int D, int heads, int T_total, int n_slots, int lgP, int pps,
                                                                  int vec_rows, const int* __restrict__ t0_rows, int t0_stride,
                                                                  const int* __restrict__ slot_rows, const int* __restrict__ page_rows,
                                                                  const int* __restrict__ first_rows, const int* __restrict__ c_rows,
                                                                  const int* __restrict__ row_of_frame, const T* __restrict__ qkv, const C* __restrict__ kc,
                                                                  float* __restrict__ probs) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC;
    const int lane = threadIdx.x & 63, grp = lane / LPR, sub = lane - grp * LPR;
    const int F = FORM == FORM_ROWS ? rows * c_or_F : c_or_F;
    const long item = (long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (item >= (long)F * (S - 1) * heads) return;
    const int h = (int)(item % heads);
    const long fs = item / heads;
    const int s = 1 + (int)(fs % (S - 1)), f = (int)(fs / (S - 1));
    const int col = h * ATT_HD + sub * VEC;
    float* prow = probs + (size_t)item * T_total;
    // (f is the same in every lane of the wave: the session's entries stay scalars)
    int t0, slot = 0, first, c, j;
    bool bad;
    const int* pages = nullptr;
    if constexpr (FORM == FORM_ROWS) {
        c = c_or_F;
        const int b = f / c;
        first = b * c;
        j = f - first;
        t0 = __builtin_amdgcn_readfirstlane(t0_rows[(long)b * t0_stride]);
        slot = __builtin_amdgcn_readfirstlane(slot_rows ? slot_rows[b] : b);
        bad = t0 < 0 || t0 > T_total - c || slot < 0 || slot >= n_slots;
    } else {
        const int r = __builtin_amdgcn_readfirstlane(row_of_frame[f]);
        const bool bad_r = r < 0 || r >= rows;             // (a table entry outside the step names no session: nothing of a session is read)
        const int rr = bad_r ? 0 : r;
        t0 = __builtin_amdgcn_readfirstlane(t0_rows[rr]);
        first = __builtin_amdgcn_readfirstlane(first_rows[rr]);
        c = __builtin_amdgcn_readfirstlane(c_rows[rr]);
        j = f - first;
        bad = bad_r || t0 < 0 || c < 1 || t0 > T_total - c || j < 0 || j >= c || first < 0 || first > F - c;
        if constexpr (FORM == FORM_RAGGED) {
            slot = __builtin_amdgcn_readfirstlane(slot_rows[rr]);
            bad = bad || slot < 0 || slot >= n_slots;
        } else {
            pages = page_rows + (size_t)rr * pps;
        }
    }
    int mine = 0;                                           // paged: entry `lane` of the session's row, kept for PagedKeys::page
    if constexpr (FORM == FORM_PAGED) {
        if (!bad) {
            // (bad is the same in every lane; 0 <= t0 + j < T_total here, so entries 0 .. (t0 + j) >> lgP are inside the session's table row;
            // the step checks all of them for this frame, so this kernel does: a bad row is the step's bad row)
            bool off = false;
            for (int q = lane; q <= (t0 + j) >> lgP; q += 64) {
                const int p = pages[q];
                off |= p < 0 || p >= n_slots;               // (n_slots carries n_pages in this form)
                if (q == lane) mine = p;
            }
            bad = __any(off);
        }
    }
    if (bad) {
        for (int k = lane; k < T_total; k += 64) prow[k] = __builtin_nanf("");
        return;
    }
    if constexpr (FORM == FORM_PAGED) {
        const size_t run = (size_t)ATT_HD << lgP;           // the P lines of one (token slot, head) of a page
        const PagedKeys keys{pages, (size_t)(S - 1) * heads * run, ((size_t)(s - 1) * heads + h) * run + sub * VEC, lgP, mine, ((t0 + j) >> lgP) >= 64};
        probs_query_frame<T, C>(qkv, kc, keys, first, j, t0, S, s, D, col, grp, sub, prow);
    } else {
        const ContiguousKeys keys{((((size_t)slot * (S - 1) + (s - 1)) * heads + h) * T_total) * ATT_HD + sub * VEC};
        probs_query_frame<T, C>(qkv, kc, keys, first, j, t0, S, s, D, col, grp, sub, prow);
    }
    // the frames after t: exactly +0.0
    int k = t0 + j + 1;
    if (vec_rows) {                                         // T_total % 4 == 0, probs 16-byte aligned: every row starts on a 16-byte boundary
        const int k4 = (k + 3) & ~3;
        if (k + lane < k4) prow[k + lane] = 0.f;
        for (int kk = k4 + 4 * lane; kk < T_total; kk += 256) *reinterpret_cast<float4*>(prow + kk) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (k += lane; k < T_total; k += 64) prow[k] = 0.f;
    }
}

}  // namespace

extern "C" {

int tcow_attn_temporal_step_probs(void* stream, const tcow_stream_attn_args* args, float* probs) {
    const int status = tcow_stream_attn_check("tcow_attn_temporal_step_probs", args, false);
    if (status != TCOW_OK) return status;
    TCOW_CHECK_ARG(probs != nullptr, "tcow_attn_temporal_step_probs: probs is NULL");
    const tcow_stream_attn_args& a = *args;
    const tcow_attn_shape& s = a.shape;
    const bool ragged = a.n_sessions != 0, paged = a.page_frames != 0;
    const int T_total = a.T_total;
    const long F = ragged ? s.T : (long)s.B * s.T, items = F * (s.S - 1) * s.heads;
    TCOW_CHECK_ARG(F <= 0x7fffffffL && items <= (long)ST_WAVES * 0x7fffffffL,
                   "tcow_attn_temporal_step_probs: the step asks for %ld waves, more than one grid holds", items);
    const dim3 grid((unsigned)cdiv(items, ST_WAVES)), block(64 * ST_WAVES);
    const hipStream_t st = (hipStream_t)stream;
    const int vec_rows = (T_total % 4 == 0 && (uintptr_t)probs % 16 == 0) ? 1 : 0;
    with_cache_types(s.dtype, a.cache_dtype, [&](auto t, auto c) {
        using T = decltype(t); using C = decltype(c);
        const T* qkv = (const T*)a.qkv;
        const C* kc = (const C*)a.k_cache;
        if (!ragged) {      // (the stream: one t0 entry for every row -- stride 0 --, slot = row, a slot per row)
            hipLaunchKernelGGL((step_probs_kernel<T, C, FORM_ROWS>), grid, block, 0, st, s.B, s.T, s.S, s.D, s.heads, T_total, a.slot_rows ? a.n_slots : s.B, 0, 0,
                               vec_rows, a.t0_rows, a.slot_rows ? 1 : 0, a.slot_rows, nullptr, nullptr, nullptr, nullptr, qkv, kc, probs);
        } else if (!paged) {
            hipLaunchKernelGGL((step_probs_kernel<T, C, FORM_RAGGED>), grid, block, 0, st, a.n_sessions, s.T, s.S, s.D, s.heads, T_total, a.n_slots, 0, 0, vec_rows,
                               a.t0_rows, 1, a.slot_rows, nullptr, a.first_rows, a.c_rows, a.row_of_frame, qkv, kc, probs);
        } else {
            int lgP = 0;
            while ((1 << lgP) < a.page_frames) ++lgP;
            hipLaunchKernelGGL((step_probs_kernel<T, C, FORM_PAGED>), grid, block, 0, st, a.n_sessions, s.T, s.S, s.D, s.heads, T_total, a.n_pages, lgP,
                               a.pages_per_session, vec_rows, a.t0_rows, 1, nullptr, a.page_rows, a.first_rows, a.c_rows, a.row_of_frame, qkv, kc, probs);
        }
    });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // extern "C"
