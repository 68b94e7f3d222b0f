// Parameter block, its host-side builders and the element epilogue shared by the two f32-storage GEMM kernels (gemm_f32.hip: exact f32 MFMA,
// gemm_x3.hip: bf16 x 3).  Their split-K slabs are folded by reduce.hip.
#pragma once
#include "common.h"
#include "internal.h"

//   C[i,j] = sum_k A(i,k) * B(j,k),  A(i,k) = A[i*sai + k*sak],  B(j,k) = B[j*sbj + k*sbk]   (NT: sak = sbk = 1, TN: sai = sbj = 1)
struct F32Params {
    int M, N, K;
    const float* A; long sai, sak;
    const float* B; long sbj, sbk;
    void* C; long ldc;
    const float* bias; const float* row_scale; const float* resid; long ldr;
    int act; float* aux; long ldaux;
    const float* bias2; const float* row_scale2;      // second bias with its own row scale (folded temporal projection), or NULL
    int kps;          // contraction elements per z-slice (multiple of the kernel's k-slice)
    float* slab;      // if non-NULL: raw partial sums to slab[z][M][N], no epilogue
};

// the NT form of tcow_gemm_args with all its epilogue; one z-slice of the whole K, rounded up to the kernel's k-slice
static inline F32Params f32_params_nt(const tcow_gemm_args* a, int kslice) {
    F32Params p;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.A = (const float*)a->A; p.sai = a->lda; p.sak = 1;
    p.B = (const float*)a->W; p.sbj = a->ldw; p.sbk = 1;
    p.C = a->C; p.ldc = a->ldc; p.bias = a->bias; p.row_scale = a->row_scale; p.resid = a->resid; p.ldr = a->ldr;
    p.act = a->act; p.aux = (float*)a->aux; p.ldaux = a->ldaux; p.bias2 = a->bias2; p.row_scale2 = a->row_scale2; p.kps = ((a->K + kslice - 1) / kslice) * kslice; p.slab = nullptr;
    return p;
}
// a product with no epilogue (C, ldc and every epilogue field null): the TN forms write slabs, tcow_sgemm_x3_batched sets C itself
static inline F32Params f32_params_plain(int M, int N, int K, const float* A, long sai, long sak, const float* B, long sbj, long sbk, int kps, float* slab) {
    F32Params p = {};
    p.M = M; p.N = N; p.K = K;
    p.A = A; p.sai = sai; p.sak = sak;
    p.B = B; p.sbj = sbj; p.sbk = sbk;
    p.kps = kps; p.slab = slab;
    return p;
}

// The operand split of the bf16 x 3 kernels (gemm_x3.hip, gemm_nt_skinny_x3.hip): hi = bf16(x) (round to nearest even), lo = bf16(x - hi), two
// elements per call, packed.  (always bfloat16 splits, whatever 16-bit format the rest of the library is built for: bf16 keeps the f32 exponent
// range, so lo never underflows)
typedef __attribute__((ext_vector_type(8))) __bf16 x3_bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 x3_bf16x2;
__device__ __forceinline__ uint32_t x3_pack(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, x3_bf16x2));
}
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& h, uint32_t& l) {
    h = x3_pack(x0, x1);
    l = x3_pack(x0 - __builtin_bit_cast(float, h << 16), x1 - __builtin_bit_cast(float, h & 0xffff0000u));     // exact differences (hi shares the leading bits of x)
}

// bias, DropPath row scale, activation (with its side input / output), residual -- the semantics of tcow_gemm_args, one element
__device__ __forceinline__ void f32_epilogue_store(const F32Params& p, int gm, int gn, float x, float bv) {
    x += bv;
    if (p.row_scale) x *= p.row_scale[gm];
    if (p.act == TCOW_ACT_GELU) {
        if (p.aux) p.aux[(size_t)gm * p.ldaux + gn] = x;
        x = gelu_erf(x);
    } else if (p.act == TCOW_ACT_DGELU) {
        x *= gelu_erf_grad(p.aux[(size_t)gm * p.ldaux + gn]);
    } else if (p.act == TCOW_ACT_GELU_DSAVE) {
        p.aux[(size_t)gm * p.ldaux + gn] = gelu_erf_grad(x);
        x = gelu_erf(x);
    } else if (p.act == TCOW_ACT_MUL_AUX) {
        x *= p.aux[(size_t)gm * p.ldaux + gn];
    }
    if (p.bias2) x += (p.row_scale2 ? p.row_scale2[gm] : 1.0f) * p.bias2[gn];
    if (p.resid) x += p.resid[(size_t)gm * p.ldr + gn];
    reinterpret_cast<float*>(p.C)[(size_t)gm * p.ldc + gn] = x;
}

// the same on four consecutive columns gn .. gn+3 of row gm (all pointers / pitches 16-byte compatible: the caller checks)
__device__ __forceinline__ void f32_epilogue_store4(const F32Params& p, int gm, int gn, float4 x, float4 bv) {
    x.x += bv.x; x.y += bv.y; x.z += bv.z; x.w += bv.w;
    if (p.row_scale) { const float rs = p.row_scale[gm]; x.x *= rs; x.y *= rs; x.z *= rs; x.w *= rs; }
    float* ax = p.aux ? p.aux + (size_t)gm * p.ldaux + gn : nullptr;
    if (p.act == TCOW_ACT_GELU) {
        if (ax) st4(ax, x);
        x = make_float4(gelu_erf(x.x), gelu_erf(x.y), gelu_erf(x.z), gelu_erf(x.w));
    } else if (p.act == TCOW_ACT_DGELU) {
        const float4 a = ld4(ax);
        x.x *= gelu_erf_grad(a.x); x.y *= gelu_erf_grad(a.y); x.z *= gelu_erf_grad(a.z); x.w *= gelu_erf_grad(a.w);
    } else if (p.act == TCOW_ACT_GELU_DSAVE) {
        st4(ax, make_float4(gelu_erf_grad(x.x), gelu_erf_grad(x.y), gelu_erf_grad(x.z), gelu_erf_grad(x.w)));
        x = make_float4(gelu_erf(x.x), gelu_erf(x.y), gelu_erf(x.z), gelu_erf(x.w));
    } else if (p.act == TCOW_ACT_MUL_AUX) {
        const float4 a = ld4(ax);
        x.x *= a.x; x.y *= a.y; x.z *= a.z; x.w *= a.w;
    }
    if (p.bias2) { const float r2 = p.row_scale2 ? p.row_scale2[gm] : 1.0f; const float4 b2 = ld4(p.bias2 + gn); x.x += r2 * b2.x; x.y += r2 * b2.y; x.z += r2 * b2.z; x.w += r2 * b2.w; }
    if (p.resid) { const float4 r = ld4(p.resid + (size_t)gm * p.ldr + gn); x.x += r.x; x.y += r.y; x.z += r.z; x.w += r.w; }
    st4(reinterpret_cast<float*>(p.C) + (size_t)gm * p.ldc + gn, x);
}
