// Streaming inference (tcow_amd/stream.py): temporal attention of a chunk of c new frames against a per-block K / V cache of the frames before
// it, and the cls-row bookkeeping of causal_attention == 1 across chunks.  Replaces, for a stream, the temporal core of Attention.forward
// (vit.py:88-109 with the tril() mask of vit.py:93-99) and the frame-0 cls broadcast of vit.py:189-198,215.  This file has the per-frame body,
// the kernels and the two entry points; what a cache element is and where a key lives is attention_stream_cache.h.
//
// tcow_attn_temporal_step switches over three kernels (the record and its forms: the header).
// temporal_cached_kernel, the rows form: one wave per (row b, slot s, head h); four waves per workgroup.  A wave covers G key rows per load (lines
// and lane groups: the header).  Lane group g walks keys g, g + G, ... with its own online softmax (scores reduced over the group's lanes by xor
// shuffles), ST_U batches of G rows in flight per wave; the G partial states are merged by xor shuffles at the end.  No LDS.  The cache of
// (slot, s, h) is one contiguous [T_total, 64] block ([n_slots, S-1, heads, T_total, 64]), so a pass over it is a run of whole lines.  Keys of
// frames < t0 come from the cache, keys of the chunk's own frames from the chunk's qkv rows; the same wave copies the chunk's K / V rows into cache
// positions t0 .. t0+c-1 (nothing reads them in this launch).  Row r reads t0_rows[r * t0_stride] and works on cache block slot_rows[r]; a stream
// is the case "t0 broadcast (stride 0), slot = b (no table)".  Rows of different t0 run key loops of different length; nothing else differs.
// temporal_ragged_kernel (SeekerStreamPool.step_ragged): sessions that bring different numbers of frames to one step.  The frames lie flat in
// session order; one wave per (flat frame, slot, head) on the per-frame body it shares with temporal_cached_kernel (temporal_query_frame), so a
// long chunk spreads over as many waves as it has frames.
// temporal_ragged_paged_kernel (a paged SeekerStreamPool, stream_pool(page_frames=P)): the ragged kernel on a cache that is a heap of pages of P
// frames, [n_pages, S-1, heads, P, 64]; a session's row of the page table names the page of its frames q*P .. q*P+P-1.  Where a cached key lives
// is all that differs: temporal_query_frame takes that as a small functor (ContiguousKeys / PagedKeys), so the kernels keep one body and agree
// bit for bit.
// tcow_cls_step: cls_stream_kernel for the rows form (t0 and slot per row, or the stream's broadcast), cls_ragged_kernel for a ragged step.
//
// Compact cache (cache element type C != storage type T): a batch of keys is gathered as cache words -- cached lines
// loaded, the chunk's own lines (read from the step's qkv rows) encoded -- and decoded where it is used; the key order is that of the C == T
// path, whose code is unchanged.  Measured ("Compact cache"): the kernels are bound by issued instructions and by waves in
// flight, not by HBM, so what pays is gathering words (16 instead of 64 registers while the loads fly: 127 VGPRs and four waves per SIMD for
// 16-bit -> fp8, where decoding at the load took 136 and three) and a branch-free loop over the batches that lie wholly in the cache.
#include <math.h>

#include "attention_stream_cache.h"
#include "internal.h"

namespace {

// One query frame of a temporal stream step, shared by every kernel of this file so that they agree bit for bit: chunk frame j (flat frame
// fb + j of the step's rows, fb = the chunk's first flat frame) stands at t = t0 + j and attends to keys 0 .. t, keys < t0 from the cache at
// keys(kt) (each lane group looks up its own key: a batch of G * ST_U keys may span pages), keys t0 .. t from the step's qkv rows at flat
// frame fb + (kt - t0).  Every lane of the wave calls it; lane group 0 stores.  A compact cache (C != T): cached lines are decoded, the
// step's own keys / values rounded through C, so a key has one value wherever it is read from.
template <typename T, typename C, typename Keys>
__device__ __forceinline__ void temporal_query_frame(const T* qkv, const C* kc, const C* vc, T* out, const Keys keys, int fb, int j, int t0, int S, int s, int D,
                                                     int col, int grp) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC, G = 64 / LPR;
    const long ld3 = 3L * D;
    const float scale = 0.125f;      // head_dim ** -0.5 (vit.py:74)
    const int t = t0 + j;            // query frame; keys 0 .. t (tril() of causal 1 and 2)
    float q[VEC];
    StreamVec<T>::ld(qkv + ((long)(fb + j) * S + s) * ld3 + col, q);
    float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    if constexpr (std::is_same_v<T, C>) {
    for (int k0 = 0; k0 <= t; k0 += G * ST_U) {
        float kv[ST_U][VEC], vv[ST_U][VEC];
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            const int kt = k0 + u * G + grp;
            const auto pg = keys.page(kt <= t ? kt : t);        // (every lane, ahead of the branch)
            if (kt <= t) {
                const T* kp = kt < t0 ? keys(kc, pg, kt) : qkv + ((long)(fb + kt - t0) * S + s) * ld3 + D + col;
                const T* vp = kt < t0 ? keys(vc, pg, kt) : qkv + ((long)(fb + kt - t0) * S + s) * ld3 + 2 * D + col;
                StreamVec<T>::ld(kp, kv[u]);
                StreamVec<T>::ld(vp, vv[u]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) { kv[u][e] = 0.f; vv[u][e] = 0.f; }
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
            sc[u] = (k0 + u * G + grp <= t) ? d * scale : -INFINITY;
            mb = fmaxf(mb, sc[u]);
        }
        // (a group without a key so far keeps m = -inf, l = 0, acc = 0: both factors below are then 0)
        const float alpha = (m == -INFINITY) ? 0.f : expf(m - mb);
        l *= alpha;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] *= alpha;
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            const float p = (sc[u] == -INFINITY) ? 0.f : expf(sc[u] - mb);
            l += p;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = fmaf(p, vv[u][e], acc[e]);
        }
        m = mb;
    }
    } else {
    // A compact cache: the same loop (key order, lane groups, arithmetic), written apart so that the loop above keeps its code.  One batch of
    // G * ST_U keys from k0; all_cached: the whole batch lies below t0, so every key is a cached line and none is masked -- the batches of a
    // long stream's past run without a branch; the general batch takes cached lines as they are and rounds the step's own keys / values to C.
    auto batch = [&](const int k0, auto all_cached) {
        constexpr bool CACHED = decltype(all_cached)::value;
        typename CacheVec<T, C>::Raw kr[ST_U], vr[ST_U];                  // (gathered as cache words: few registers while the loads fly)
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            const int kt = k0 + u * G + grp;
            const auto pg = keys.page(CACHED || kt <= t ? kt : t);        // (every lane, ahead of the branch)
            if (CACHED || kt < t0) {                                      // (kt < t0 <= t)
                kr[u] = CacheVec<T, C>::ld(keys(kc, pg, kt));
                vr[u] = CacheVec<T, C>::ld(keys(vc, pg, kt));
            } else if (kt <= t) {
                const T* row = qkv + ((long)(fb + kt - t0) * S + s) * ld3 + col;
                kr[u] = encode_line<T, C>(row + D);
                vr[u] = encode_line<T, C>(row + 2 * D);
            } else {
                kr[u] = CacheVec<T, C>::zero();
                vr[u] = CacheVec<T, C>::zero();
            }
        }
        float sc[ST_U];
        float mb = m;
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            float kv[VEC], d = 0.f;
            CacheVec<T, C>::dec(kr[u], kv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) d = fmaf(q[e], kv[e], d);
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
            sc[u] = (CACHED || k0 + u * G + grp <= t) ? d * scale : -INFINITY;
            mb = fmaxf(mb, sc[u]);
        }
        const float alpha = (m == -INFINITY) ? 0.f : expf(m - mb);
        l *= alpha;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] *= alpha;
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            const float p = (sc[u] == -INFINITY) ? 0.f : expf(sc[u] - mb);
            l += p;
            float vv[VEC];
            CacheVec<T, C>::dec(vr[u], vv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = fmaf(p, vv[e], acc[e]);
        }
        m = mb;
    };
    int k0 = 0;
    for (; k0 + G * ST_U <= t0; k0 += G * ST_U) batch(k0, std::true_type{});
    for (; k0 <= t; k0 += G * ST_U) batch(k0, std::false_type{});
    }
    // merge the G groups' (m, l, acc): lanes with the same channel slice sit LPR apart
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
        const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
        const float mn = fmaxf(m, mo);
        const float a = (m == -INFINITY) ? 0.f : expf(m - mn), bb = (mo == -INFINITY) ? 0.f : expf(mo - mn);
        l = l * a + lo * bb;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { const float ao = __shfl_xor(acc[e], o, 64); acc[e] = acc[e] * a + ao * bb; }
        m = mn;
    }
    if (grp == 0) {
        const float inv = 1.f / l;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] *= inv;
        StreamVec<T>::st(out + ((long)(fb + j) * S + s) * D + col, acc);
    }
}

template <typename T, typename C>
__global__ __launch_bounds__(64 * ST_WAVES) void temporal_cached_kernel(int B, int c, int S, int D, int heads, int T_total, int n_slots,
                                                                       const int* __restrict__ t0_rows, int t0_stride, const int* __restrict__ slot_rows,
                                                                       const T* __restrict__ qkv, C* __restrict__ kc, C* __restrict__ vc, T* __restrict__ out) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC, G = 64 / LPR;
    const int lane = threadIdx.x & 63, grp = lane / LPR, sub = lane - grp * LPR;
    const long item = (long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (item >= (long)B * S * heads) return;
    const int h = (int)(item % heads);
    const long bs = item / heads;
    const int s = (int)(bs % S), b = (int)(bs / S);
    // (b is the same in every lane of the wave: t0 and the cache slot stay scalars, as the broadcast t0 of a stream was)
    const int t0 = __builtin_amdgcn_readfirstlane(t0_rows[(long)b * t0_stride]);
    const int slot = __builtin_amdgcn_readfirstlane(slot_rows ? slot_rows[b] : b);
    const long ld3 = 3L * D;
    const int col = h * ATT_HD + sub * VEC;
    const bool bad_t0 = t0 < 0 || t0 + c > T_total || slot < 0 || slot >= n_slots;
    if (s == 0 || bad_t0) {
        // slot 0 takes no part in temporal attention: its rows are defined as zero (as in the clip path).  A t0 outside the stream or a cache
        // slot outside the pool (the host checks both before it writes them) touches no cache row and writes NaN to the row's own output.
        float z[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) z[e] = bad_t0 ? __builtin_nanf("") : 0.f;
        for (int j = grp; j < c; j += G) StreamVec<T>::st(out + ((long)(b * c + j) * S + s) * D + col, z);
        return;
    }
    const ContiguousKeys keys{((((size_t)slot * (S - 1) + (s - 1)) * heads + h) * T_total) * ATT_HD + sub * VEC};
    // append the chunk's keys / values: cache[t0 + j] = chunk row j (bit copies; a compact cache: rounded to C)
    for (int j = grp; j < c; j += G) {
        const T* src = qkv + ((long)(b * c + j) * S + s) * ld3 + col;
        append_line<T, C>(keys(kc, keys.page(t0 + j), t0 + j), src + D);
        append_line<T, C>(keys(vc, keys.page(t0 + j), t0 + j), src + 2 * D);
    }
    for (int j = 0; j < c; ++j) temporal_query_frame<T, C>(qkv, kc, vc, out, keys, b * c, j, t0, S, s, D, col, grp);
}

// One wave per (flat frame f, token slot s, head h) of a ragged step: n sessions, session r with c_rows[r] frames at flat frames
// first_rows[r] .. first_rows[r] + c_rows[r] - 1 (row_of_frame[f] = r), standing at t0_rows[r] on cache block slot_rows[r].  The wave copies
// frame f's own K / V line to cache position t = t0 + (f - first) and attends frame f's query to keys 0 .. t with temporal_query_frame, the
// pool kernel's per-frame body.
// INVARIANT: no wave reads a cache position that this launch writes.  The launch writes positions t0 .. t0+c-1 of a session's block; a wave
// reads cache positions < t0 only and takes keys t0 .. t from the step's qkv rows (flat frame first + (kt - t0)).  That is what makes the
// per-frame split race-free: the waves of one session share no cache position between a writer and a reader, and sessions have distinct slots.
template <typename T, typename C>
__global__ __launch_bounds__(64 * ST_WAVES) void temporal_ragged_kernel(int n, int F, int S, int D, int heads, int T_total, int n_slots,
                                                                       const int* __restrict__ t0_rows, const int* __restrict__ slot_rows,
                                                                       const int* __restrict__ first_rows, const int* __restrict__ c_rows,
                                                                       const int* __restrict__ row_of_frame, const T* __restrict__ qkv, C* __restrict__ kc,
                                                                       C* __restrict__ vc, T* __restrict__ out) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC;
    const int lane = threadIdx.x & 63, grp = lane / LPR, sub = lane - grp * LPR;
    const long item = (long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (item >= (long)F * S * heads) return;
    const int h = (int)(item % heads);
    const long fs = item / heads;
    const int s = (int)(fs % S), f = (int)(fs / S);
    // (f is the same in every lane of the wave: the session's entries stay scalars)
    const int r = __builtin_amdgcn_readfirstlane(row_of_frame[f]);
    const bool bad_r = r < 0 || r >= n;             // (a table entry outside the step names no session: nothing of a session is read)
    const int rr = bad_r ? 0 : r;
    const int t0 = __builtin_amdgcn_readfirstlane(t0_rows[rr]);
    const int slot = __builtin_amdgcn_readfirstlane(slot_rows[rr]);
    const int first = __builtin_amdgcn_readfirstlane(first_rows[rr]);
    const int c = __builtin_amdgcn_readfirstlane(c_rows[rr]);
    const int j = f - first;
    const int col = h * ATT_HD + sub * VEC;
    // (first + c <= F: the keys t0 .. t of the chunk are read at flat frames first .. f, all inside the step when j is inside [0, c))
    const bool bad = bad_r || t0 < 0 || c < 1 || t0 > T_total - c || slot < 0 || slot >= n_slots || j < 0 || j >= c || first < 0 || first > F - c;
    if (s == 0 || bad) {
        // slot 0: zero, as in the pool kernel.  A bad row writes NaN to this frame's own output row and touches no cache row.
        if (grp == 0) {
            float z[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) z[e] = bad ? __builtin_nanf("") : 0.f;
            StreamVec<T>::st(out + ((long)f * S + s) * D + col, z);
        }
        return;
    }
    const ContiguousKeys keys{((((size_t)slot * (S - 1) + (s - 1)) * heads + h) * T_total) * ATT_HD + sub * VEC};
    if (grp == 0) {
        // append this frame's key / value: cache[t0 + j] = the frame's own row (bit copies)
        const T* src = qkv + ((long)f * S + s) * (3L * D) + col;
        append_line<T, C>(keys(kc, keys.page(t0 + j), t0 + j), src + D);
        append_line<T, C>(keys(vc, keys.page(t0 + j), t0 + j), src + 2 * D);
    }
    temporal_query_frame<T, C>(qkv, kc, vc, out, keys, first, j, t0, S, s, D, col, grp);
}

// temporal_ragged_kernel on a paged cache: the K / V array of a block is [n_pages, S-1, heads, P, 64] with P = 1 << lgP frames per page, and
// session r brings row r of the page table page_rows [n, pps]: entry q is the page of its frames q*P .. q*P+P-1.  Cache position kt of
// (session r, token slot s, head h) is line kt % P of the (s-1, h) run of page page_rows[r][kt / P] (PagedKeys).  One wave per (flat frame f,
// token slot s, head h), the append of the frame's own K / V line and the per-frame body exactly as in temporal_ragged_kernel.
// Before it touches any cache line the wave checks every table entry it would dereference: pages 0 .. (t0 + j) / P of its session must lie in
// [0, n_pages) (t0 + j < T_total <= pps * P, which the launcher checked: the entries exist).  A bad entry, like a bad row of the ragged kernel,
// writes NaN to this frame's own output row and touches no page.  The check loads entry `lane` into every lane; while the wave's keys reach
// entries < 64 only, a lane group's lookup is a shuffle from those (one load less in the wave's chain of dependent loads, which is what bounds
// this kernel at a few tens of frames), otherwise a load from the table.
// INVARIANT: no wave reads a cache position that this launch writes.  The launch writes positions t0 .. t0+c-1 of a session (in the pages its
// table row names for them); a wave reads positions < t0 of its own session's pages only and takes keys t0 .. t from the step's qkv rows.  The
// pages of two sessions of one launch are distinct: a page in two sessions' rows is the host's error, as a slot in two rows is in the kernels
// above (the pool's allocator never hands a page out twice).
template <typename T, typename C>
__global__ __launch_bounds__(64 * ST_WAVES) void temporal_ragged_paged_kernel(int n, int F, int S, int D, int heads, int T_total, int n_pages, int lgP, int pps,
                                                                             const int* __restrict__ t0_rows, const int* __restrict__ page_rows,
                                                                             const int* __restrict__ first_rows, const int* __restrict__ c_rows,
                                                                             const int* __restrict__ row_of_frame, const T* __restrict__ qkv,
                                                                             C* __restrict__ kc, C* __restrict__ vc, T* __restrict__ out) {
    constexpr int VEC = StreamVec<T>::VEC, LPR = ATT_HD / VEC;
    const int lane = threadIdx.x & 63, grp = lane / LPR, sub = lane - grp * LPR;
    const long item = (long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (item >= (long)F * S * heads) return;
    const int h = (int)(item % heads);
    const long fs = item / heads;
    const int s = (int)(fs % S), f = (int)(fs / S);
    // (f is the same in every lane of the wave: the session's entries stay scalars)
    const int r = __builtin_amdgcn_readfirstlane(row_of_frame[f]);
    const bool bad_r = r < 0 || r >= n;             // (a table entry outside the step names no session: nothing of a session is read)
    const int rr = bad_r ? 0 : r;
    const int t0 = __builtin_amdgcn_readfirstlane(t0_rows[rr]);
    const int first = __builtin_amdgcn_readfirstlane(first_rows[rr]);
    const int c = __builtin_amdgcn_readfirstlane(c_rows[rr]);
    const int j = f - first;
    const int col = h * ATT_HD + sub * VEC;
    const int* pages = page_rows + (size_t)rr * pps;
    bool bad = bad_r || t0 < 0 || c < 1 || t0 > T_total - c || j < 0 || j >= c || first < 0 || first > F - c;
    int mine = 0;                                   // entry `lane` of the session's row, kept for PagedKeys::page
    if (!bad) {
        // (bad is the same in every lane; 0 <= t0 + j < T_total here, so entries 0 .. (t0 + j) >> lgP are inside the session's table row)
        bool off = false;
        for (int q = lane; q <= (t0 + j) >> lgP; q += 64) {
            const int p = pages[q];
            off |= p < 0 || p >= n_pages;
            if (q == lane) mine = p;
        }
        bad = __any(off);
    }
    if (s == 0 || bad) {
        // slot 0: zero, as in the pool kernel.  A bad row or page writes NaN to this frame's own output row and touches no page.
        if (grp == 0) {
            float z[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) z[e] = bad ? __builtin_nanf("") : 0.f;
            StreamVec<T>::st(out + ((long)f * S + s) * D + col, z);
        }
        return;
    }
    const size_t run = (size_t)ATT_HD << lgP;       // the P lines of one (token slot, head) of a page
    const PagedKeys keys{pages, (size_t)(S - 1) * heads * run, ((size_t)(s - 1) * heads + h) * run + sub * VEC, lgP, mine, ((t0 + j) >> lgP) >= 64};
    const int own = keys.page(t0 + j);              // (every lane, ahead of the branch)
    if (grp == 0) {
        // append this frame's key / value: position t0 + j of the session = the frame's own row (bit copies)
        const T* src = qkv + ((long)f * S + s) * (3L * D) + col;
        append_line<T, C>(keys(kc, own, t0 + j), src + D);
        append_line<T, C>(keys(vc, own, t0 + j), src + 2 * D);
    }
    temporal_query_frame<T, C>(qkv, kc, vc, out, keys, first, j, t0, S, s, D, col, grp);
}

// causal_attention == 1 across chunks, for one session and 4 channels: `base` is slot 0 of the session's first frame of this step (these 4
// channels), its c frames lie fs floats apart, cls_cache + at is the session's cache row (these 4 channels).  t0 == 0: tcow_cls_merge mode 1 on the chunk
// (frame 0's slot-0 row to every frame), the row kept in the cache; t0 > 0: the cache row to slot 0 of every chunk frame.  A slot outside
// [0, n_slots) writes NaN and touches no cache row.
__device__ __forceinline__ void cls_session(int slot, int n_slots, int t0, float* base, int c, size_t fs, float* cls_cache, size_t at) {
    float4 a;
    if (slot < 0 || slot >= n_slots) {
        a.x = a.y = a.z = a.w = __builtin_nanf("");
    } else if (t0 == 0) {
        a = ld4(base);
        st4(cls_cache + at, a);
    } else {
        a = ld4(cls_cache + at);
    }
    for (int t = 0; t < c; ++t) st4(base + t * fs, a);
}

// Row b is a session of c frames with t0 = t0_rows[b * t0_stride] and cache row slot = slot_rows ? slot_rows[b] : b.  One thread per (b, 4 channels).
__global__ void cls_stream_kernel(int B, int c, int S, int D, float* __restrict__ x, float* __restrict__ cls_cache, int n_slots,
                                  const int* __restrict__ t0_rows, int t0_stride, const int* __restrict__ slot_rows) {
    const int d4 = D / 4;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)B * d4) return;
    const int b = (int)(i / d4), ch = (int)(i - (long)b * d4) * 4;
    const int slot = slot_rows ? slot_rows[b] : b;
    cls_session(slot, n_slots, t0_rows[(long)b * t0_stride], x + (size_t)b * c * S * D + ch, c, (size_t)S * D, cls_cache, (size_t)slot * D + ch);
}

// A ragged step: session r owns the flat frames first_rows[r] .. first_rows[r] + c_rows[r] - 1.  One thread per (session, 4 channels), looping
// over the session's frames: a thread per frame would read frame `first` while another wrote it.  Frames outside the step are not written.
__global__ void cls_ragged_kernel(int n, int F, int S, int D, float* __restrict__ x, float* __restrict__ cls_cache, int n_slots,
                                  const int* __restrict__ t0_rows, const int* __restrict__ slot_rows, const int* __restrict__ first_rows,
                                  const int* __restrict__ c_rows) {
    const int d4 = D / 4;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)n * d4) return;
    const int r = (int)(i / d4), ch = (int)(i - (long)r * d4) * 4;
    const int slot = slot_rows[r], first = first_rows[r], c = c_rows[r];
    if (first < 0 || c < 1 || first > F - c) return;          // (the host builds the tables; a session outside the step owns no row of x)
    cls_session(slot, n_slots, t0_rows[r], x + (size_t)first * S * D + ch, c, (size_t)S * D, cls_cache, (size_t)slot * D + ch);
}

}  // namespace

// What it asks of every step: a shape of s.T >= 1 frames per row, head_dim 64, a causal mask, a stream of T_min .. TCOW_STREAM_MAX_FRAMES frames
// (a chunk of s.B rows must fit into the cache: T_min = s.T; the F frames of a ragged step belong to several sessions and may exceed T_total:
// T_min = 1), a storage type of this file, at least one cache slot (the stream: a slot per row; a paged cache has pages, checked below), and a
// cache element type that is one of the three and no wider than the storage; of a ragged step of n sessions also its one row of F frames, of
// a paged cache its geometry; then the pointers of the form.  `who` is the entry point the refusal is reported under: tcow_attn_temporal_step, and
// tcow_attn_temporal_step_probs (attention_stream_probs.hip), which takes the same record and neither reads nor writes `out` (needs_out false).
int tcow_stream_attn_check(const char* who, const tcow_stream_attn_args* args, bool needs_out) {
    TCOW_CHECK_ARG(args != nullptr, "%s: null args", who);
    const tcow_stream_attn_args& a = *args;
    const tcow_attn_shape& s = a.shape;
    const bool ragged = a.n_sessions != 0, paged = a.page_frames != 0;
    const int n = a.n_sessions, cq = a.cache_dtype, T_total = a.T_total;
    TCOW_CHECK_ARG(ragged || !paged, "%s: a paged cache (page_frames=%d) serves ragged steps only (n_sessions=0 is the rows form)", who,
                   a.page_frames);
    TCOW_CHECK_ARG(s.B > 0 && s.T > 0 && s.S > 1 && s.heads > 0, "%s: bad step shape B=%d T=%d S=%d heads=%d", who, s.B, s.T, s.S, s.heads);
    TCOW_CHECK_ARG(s.D == s.heads * ATT_HD, "%s: head_dim must be 64 (D=%d heads=%d)", who, s.D, s.heads);
    TCOW_CHECK_ARG(s.causal == 1 || s.causal == 2, "%s: causal must be 1 or 2 (got %d): other masks let a frame see later frames", who, s.causal);
    const int T_min = ragged ? 1 : s.T;
    TCOW_CHECK_ARG(T_total >= T_min && T_total <= TCOW_STREAM_MAX_FRAMES, "%s: T_total=%d must be in [%d, %d]", who, T_total, T_min,
                   TCOW_STREAM_MAX_FRAMES);
    TCOW_CHECK_ARG(s.dtype == TCOW_F32 || s.dtype == TCOW_BF16, "%s: dtype must be TCOW_F32 or TCOW_BF16 (got %d)", who, s.dtype);
    const int n_slots = !ragged && !a.slot_rows ? s.B : a.n_slots;
    TCOW_CHECK_ARG(paged || n_slots >= 1, "%s: n_slots=%d must be >= 1", who, n_slots);
    TCOW_CHECK_ARG(cq == TCOW_F32 || cq == TCOW_BF16 || cq == TCOW_FP8E4M3,
                   "%s: cache_dtype must be TCOW_F32, TCOW_BF16 or TCOW_FP8E4M3 (got %d)", who, cq);
    TCOW_CHECK_ARG(!(s.dtype == TCOW_BF16 && cq == TCOW_F32), "%s: cache_dtype TCOW_F32 is wider than the 16-bit storage (dtype TCOW_BF16)", who);
    TCOW_CHECK_ARG(!ragged || (s.B == 1 && n > 0 && n <= s.T),
                   "%s: a ragged step is one row of F frames of 1 <= n <= F sessions (B=%d F=%d n=%d)", who, s.B, s.T, n);
    if (paged) {
        TCOW_CHECK_ARG(a.page_frames >= 1 && a.page_frames <= TCOW_STREAM_MAX_FRAMES && (a.page_frames & (a.page_frames - 1)) == 0,
                       "%s: page_frames=%d must be a power of two in [1, %d]", who, a.page_frames, TCOW_STREAM_MAX_FRAMES);
        TCOW_CHECK_ARG(a.n_pages >= 1, "%s: n_pages=%d must be >= 1", who, a.n_pages);
        TCOW_CHECK_ARG(a.pages_per_session >= 1 && (long)a.pages_per_session * a.page_frames >= T_total,
                       "%s: pages_per_session=%d x page_frames=%d does not cover T_total=%d", who, a.pages_per_session, a.page_frames, T_total);
    }
    TCOW_CHECK_ARG(a.t0_rows && a.qkv && a.k_cache && a.v_cache && (a.out || !needs_out) &&
                   (!ragged || (a.first_rows && a.c_rows && a.row_of_frame && (paged ? a.page_rows : a.slot_rows))), "%s: null pointer", who);
    return TCOW_OK;
}

extern "C" {

// One wave per item: (row, slot, head), ragged (flat frame, slot, head).
int tcow_attn_temporal_step(void* stream, const tcow_stream_attn_args* args) {
    const int status = tcow_stream_attn_check("tcow_attn_temporal_step", args, true);
    if (status != TCOW_OK) return status;
    const tcow_stream_attn_args& a = *args;
    const tcow_attn_shape& s = a.shape;
    const bool ragged = a.n_sessions != 0, paged = a.page_frames != 0;
    const int n = a.n_sessions, cq = a.cache_dtype, T_total = a.T_total;
    const int n_slots = !ragged && !a.slot_rows ? s.B : a.n_slots;
    const long items = (long)(ragged ? s.T : s.B) * s.S * s.heads;
    const dim3 grid((unsigned)cdiv(items, ST_WAVES)), block(64 * ST_WAVES);
    const hipStream_t st = (hipStream_t)stream;
    with_cache_types(s.dtype, cq, [&](auto t, auto c) {
        using T = decltype(t); using C = decltype(c);
        const T* qkv = (const T*)a.qkv;
        C *kc = (C*)a.k_cache, *vc = (C*)a.v_cache;
        T* out = (T*)a.out;
        if (!ragged) {      // (the stream: one t0 entry for every row -- stride 0 --, slot = row)
            hipLaunchKernelGGL((temporal_cached_kernel<T, C>), grid, block, 0, st, s.B, s.T, s.S, s.D, s.heads, T_total, n_slots, a.t0_rows,
                               a.slot_rows ? 1 : 0, a.slot_rows, qkv, kc, vc, out);
        } else if (!paged) {
            hipLaunchKernelGGL((temporal_ragged_kernel<T, C>), grid, block, 0, st, n, s.T, s.S, s.D, s.heads, T_total, n_slots, a.t0_rows, a.slot_rows,
                               a.first_rows, a.c_rows, a.row_of_frame, qkv, kc, vc, out);
        } else {
            int lgP = 0;
            while ((1 << lgP) < a.page_frames) ++lgP;
            hipLaunchKernelGGL((temporal_ragged_paged_kernel<T, C>), grid, block, 0, st, n, s.T, s.S, s.D, s.heads, T_total, a.n_pages, lgP,
                               a.pages_per_session, a.t0_rows, a.page_rows, a.first_rows, a.c_rows, a.row_of_frame, qkv, kc, vc, out);
        }
    });
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

int tcow_cls_step(void* stream, const tcow_stream_cls_args* args) {
    TCOW_CHECK_ARG(args != nullptr, "tcow_cls_step: args is NULL");
    const tcow_stream_cls_args& a = *args;
    const bool ragged = a.first_rows || a.c_rows;
    const int n_slots = !ragged && !a.slot_rows ? a.n : a.n_slots;          // (the stream: a cache row per row)
    TCOW_CHECK_ARG(a.n >= 1, "tcow_cls_step: n = %d, must be >= 1", a.n);
    TCOW_CHECK_ARG(ragged || a.c >= 1, "tcow_cls_step: c = %d, must be >= 1", a.c);
    TCOW_CHECK_ARG(!ragged || a.F >= a.n, "tcow_cls_step: F = %d, must be >= n = %d (a ragged step)", a.F, a.n);
    TCOW_CHECK_ARG(a.S > 1, "tcow_cls_step: S = %d, must be > 1", a.S);
    TCOW_CHECK_ARG(a.D > 0 && a.D % 4 == 0, "tcow_cls_step: D = %d, must be a positive multiple of 4", a.D);
    TCOW_CHECK_ARG(n_slots >= 1, "tcow_cls_step: n_slots = %d, must be >= 1", n_slots);
    TCOW_CHECK_ARG(a.x, "tcow_cls_step: x is NULL");
    TCOW_CHECK_ARG(a.cls_cache, "tcow_cls_step: cls_cache is NULL");
    TCOW_CHECK_ARG(a.t0_rows, "tcow_cls_step: t0_rows is NULL");
    const dim3 grid(cdiv((long)a.n * a.D / 4, 64)), block(64);
    if (ragged) {
        TCOW_CHECK_ARG(a.slot_rows, "tcow_cls_step: slot_rows is NULL in a ragged step");
        TCOW_CHECK_ARG(a.first_rows, "tcow_cls_step: first_rows is NULL with c_rows given");
        TCOW_CHECK_ARG(a.c_rows, "tcow_cls_step: c_rows is NULL with first_rows given");
        hipLaunchKernelGGL(cls_ragged_kernel, grid, block, 0, (hipStream_t)stream, a.n, a.F, a.S, a.D, a.x, a.cls_cache, n_slots, a.t0_rows, a.slot_rows,
                           a.first_rows, a.c_rows);
    } else {
        hipLaunchKernelGGL(cls_stream_kernel, grid, block, 0, (hipStream_t)stream, a.n, a.c, a.S, a.D, a.x, a.cls_cache, n_slots, a.t0_rows,
                           a.slot_rows ? 1 : 0, a.slot_rows);
    }
    TCOW_CHECK_LAUNCH();
    return TCOW_OK;
}

}  // extern "C"
