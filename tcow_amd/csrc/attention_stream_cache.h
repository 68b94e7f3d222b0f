// What the stream attention kernels (attention_stream.hip, attention_stream_probs.hip) know about a cache element and about where a key lives: a lane's slice of a line
// in the storage type (StreamVec), in the cache type (CacheVec, fp8_t), the append of a line, and the two cache layouts (ContiguousKeys /
// PagedKeys), the wave and batch counts and the switch over (storage, cache) types.  Everything else in the two sources is written against these.
//
// Lines.  The head's 64 channels of a K / V row are one 128-byte (16-bit) or 256-byte (f32) line: LPR lanes read it with one 16-byte load each,
// so a wave covers G = 64 / LPR key rows per load (16-bit: 8 lanes x 8 elements, 8 rows; f32: 16 lanes x 4, 4 rows).
//
// Compact cache: the cache element type C is a second template parameter next to the storage type T.  C == T copies bits.  Otherwise (16-bit ->
// fp8, f32 -> the build's 16-bit type, f32 -> fp8; fp8 = OCP e4m3fn, saturating) the append stores rnd_C(k), rnd_C(v) once and EVERY key and
// value enters the arithmetic at its rounded value, so a key has one value wherever it came from and outputs and caches do not depend on how the
// frames were split into chunks.  q is not rounded.  A lane keeps the storage type's channel slice (8 or 4 channels: 8 or 4 bytes of a cache
// line); CacheVec is all that knows C.
#pragma once
#include <type_traits>

#include "attention_common.h"

namespace {

constexpr int ST_WAVES = 4;     // waves (items) per workgroup
constexpr int ST_U = 4;         // batches of G key rows loaded before they are used

template <typename T> struct StreamVec;
template <> struct StreamVec<bf16_t> {
    static constexpr int VEC = 8;
    static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        v[0] = bflo(u.x); v[1] = bfhi(u.x); v[2] = bflo(u.y); v[3] = bfhi(u.y);
        v[4] = bflo(u.z); v[5] = bfhi(u.z); v[6] = bflo(u.w); v[7] = bfhi(u.w);
    }
    static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
        uint4 u;
        u.x = pack_bf2(v[0], v[1]); u.y = pack_bf2(v[2], v[3]); u.z = pack_bf2(v[4], v[5]); u.w = pack_bf2(v[6], v[7]);
        *reinterpret_cast<uint4*>(p) = u;
    }
};
template <> struct StreamVec<float> {
    static constexpr int VEC = 4;
    static __device__ __forceinline__ void ld(const float* p, float* v) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
    static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

__device__ __forceinline__ void copy16(void* dst, const void* src) { *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src); }

// ---- compact cache elements.  fp8_t: one OCP e4m3fn byte (gfx950's v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8).
struct fp8_t { uint8_t b; };

// f32 -> e4m3fn as torch's x.clamp(-448, 448).to(torch.float8_e4m3fn): saturating, round to nearest even, subnormals kept, NaN -> 0x7f | sign.
// The clamp is one v_med3_f32, which does not keep a NaN: a NaN's byte is set after the conversion, so what the instruction makes of a NaN
// never shows.  Four values -> four bytes, v[0] in the lowest; a NaN among them is rare and handled on a branch of its own.
__device__ __forceinline__ float fp8_clamp(float x) { return __builtin_amdgcn_fmed3f(x, -448.f, 448.f); }
__device__ __forceinline__ uint32_t pack_fp8x4(const float* v) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(v[0]), fp8_clamp(v[1]), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(v[2]), fp8_clamp(v[3]), w, true);
    uint32_t u = (uint32_t)w;
    if (__builtin_expect(v[0] != v[0] || v[1] != v[1] || v[2] != v[2] || v[3] != v[3], 0)) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] != v[e]) u = (u & ~(0xffu << (8 * e))) | ((0x7fu | ((__float_as_uint(v[e]) >> 24) & 0x80u)) << (8 * e));
    }
    return u;
}
__device__ __forceinline__ void unpack_fp8x4(uint32_t w, float* v) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
}

// A lane's StreamVec<T>::VEC channels of a cache line of C elements as a Raw word: ld from the cache, enc from f32 (what the append stores, and
// what a chunk's own key / value becomes before it is used), dec to f32, zero (decodes to 0).  A key therefore has ONE value, dec of its Raw,
// wherever it was read from.  Storage T, cache C; CacheVec<T, T> is never asked (C == T copies bits).
template <typename T, typename C> struct CacheVec;
template <> struct CacheVec<bf16_t, fp8_t> {           // 8 channels: 8 bytes
    typedef uint2 Raw;
    static __device__ __forceinline__ Raw ld(const fp8_t* p) { return *reinterpret_cast<const uint2*>(p); }
    static __device__ __forceinline__ void st(fp8_t* p, Raw r) { *reinterpret_cast<uint2*>(p) = r; }
    static __device__ __forceinline__ Raw enc(const float* v) { return make_uint2(pack_fp8x4(v), pack_fp8x4(v + 4)); }
    static __device__ __forceinline__ void dec(Raw r, float* v) { unpack_fp8x4(r.x, v); unpack_fp8x4(r.y, v + 4); }
    static __device__ __forceinline__ Raw zero() { return make_uint2(0u, 0u); }
};
template <> struct CacheVec<float, fp8_t> {            // 4 channels: 4 bytes
    typedef uint32_t Raw;
    static __device__ __forceinline__ Raw ld(const fp8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
    static __device__ __forceinline__ void st(fp8_t* p, Raw r) { *reinterpret_cast<uint32_t*>(p) = r; }
    static __device__ __forceinline__ Raw enc(const float* v) { return pack_fp8x4(v); }
    static __device__ __forceinline__ void dec(Raw r, float* v) { unpack_fp8x4(r, v); }
    static __device__ __forceinline__ Raw zero() { return 0u; }
};
template <> struct CacheVec<float, bf16_t> {           // 4 channels of the build's 16-bit type: 8 bytes
    typedef uint2 Raw;
    static __device__ __forceinline__ Raw ld(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
    static __device__ __forceinline__ void st(bf16_t* p, Raw r) { *reinterpret_cast<uint2*>(p) = r; }
    static __device__ __forceinline__ Raw enc(const float* v) { return make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])); }
    static __device__ __forceinline__ void dec(Raw r, float* v) { v[0] = bflo(r.x); v[1] = bfhi(r.x); v[2] = bflo(r.y); v[3] = bfhi(r.y); }
    static __device__ __forceinline__ Raw zero() { return make_uint2(0u, 0u); }
};

// the lane's slice of a row of the step's qkv, rounded to C
template <typename T, typename C> __device__ __forceinline__ typename CacheVec<T, C>::Raw encode_line(const T* src) {
    float v[StreamVec<T>::VEC];
    StreamVec<T>::ld(src, v);
    return CacheVec<T, C>::enc(v);
}

// cache[position] = the lane's slice of a chunk row's K or V: bit copy when the cache has the storage type, else rounded to C once
template <typename T, typename C> __device__ __forceinline__ void append_line(C* dst, const T* src) {
    if constexpr (std::is_same_v<T, C>) {
        copy16(dst, src);
    } else {
        CacheVec<T, C>::st(dst, encode_line<T, C>(src));
    }
}

// Where cache position kt of the wave's (session, token slot, head) lives in a block's K / V array `base` (const or not): the address of the
// lane's 16 bytes of that line.  The one thing in which the contiguous and the paged kernels differ.  In two steps: page(kt), which EVERY lane
// of the wave calls together (a paged lookup may be a lane shuffle), then keys(base, page, kt) by the lanes that load or store.
struct ContiguousKeys {             // [slots, S-1, heads, T_total, 64]: one run of whole lines from cbase (the lane's channel slice included)
    struct NoPage {};
    size_t cbase;
    __device__ __forceinline__ NoPage page(int) const { return NoPage{}; }
    template <typename P> __device__ __forceinline__ P operator()(P base, NoPage, int kt) const { return base + cbase + (size_t)kt * ATT_HD; }
};
struct PagedKeys {                  // [n_pages, S-1, heads, P, 64], P = 1 << lgP: page pages[kt / P], line kt % P of the (slot, head) run at `line`
    const int* pages;               // the session's row of the page table (entries 0 .. kt / P checked by the caller)
    size_t page_stride, line;       // (S-1) * heads * P * 64; ((s-1) * heads + h) * P * 64 + the lane's channel slice
    int lgP;
    int mine;                       // pages[lane], as the caller's check loaded it (lanes beyond the last checked entry: anything)
    bool wide;                      // the wave's keys reach entries >= 64: more entries than lanes, look them up in memory
    __device__ __forceinline__ int page(int kt) const { return wide ? pages[kt >> lgP] : __shfl(mine, kt >> lgP, 64); }
    template <typename P> __device__ __forceinline__ P operator()(P base, int pg, int kt) const {
        return base + ((size_t)pg * page_stride + line + (size_t)(kt & ((1 << lgP) - 1)) * ATT_HD);
    }
};

// Calls f(T{}, C{}) with the storage type T of `dtype` and the cache element type C of `cq` (both checked by tcow_stream_attn_check).
template <typename F> void with_cache_types(int dtype, int cq, F f) {
    if (dtype == TCOW_BF16) {
        if (cq == TCOW_FP8E4M3) f(bf16_t{}, fp8_t{}); else f(bf16_t{}, bf16_t{});
    } else {
        if (cq == TCOW_FP8E4M3) f(float{}, fp8_t{}); else if (cq == TCOW_BF16) f(float{}, bf16_t{}); else f(float{}, float{});
    }
}

}  // namespace
