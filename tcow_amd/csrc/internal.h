// Functions that are defined in one csrc source and called from another and are not part of the C ABI (include/tcow_hip.h): one declaration
// each, included by the defining file and by every caller.  (The attention back ends take a SeqDesc: attention_common.h declares them.)
#pragma once
#include "common.h"
#include "gemm_tn_plan.h"      // TCOW_TN_GROUP_MAX, TnPlan, TnGroupPlan: the host rules of the weight-gradient GEMMs

constexpr int TCOW_LN_FOLD_MAX = 16;      // jobs of one tcow_layernorm_fold launch
constexpr int TCOW_COLSUM_GROUP_MAX = TCOW_LN_FOLD_MAX;      // problems of one tcow_colsum_grouped call: one row-fold launch finishes them

// ---- NT GEMM back ends (forward / input gradient)
int tcow_gemm_nt_bf16(hipStream_t stream, const tcow_gemm_args* a);                                 // gemm_bf16.hip
bool tcow_gemm_nt_c2_ok(const tcow_gemm_args* a);                                                   // gemm_nt_c2.hip
int tcow_gemm_nt_bf16_c2(hipStream_t stream, const tcow_gemm_args* a);
int tcow_nt_band_for(const tcow_gemm_args* a, int tiles_n, int tile);                               // gemm_bf16.hip
int tcow_gemm_nt_skinny_launch_bf16(hipStream_t stream, const tcow_gemm_args* a, int split, float* slab);  // gemm_nt_skinny.hip
int tcow_gemm_nt_skinny_launch_x3(hipStream_t stream, const tcow_gemm_args* a, int split, float* slab);    // gemm_nt_skinny_x3.hip
int tcow_gemm_nt_f32(hipStream_t stream, const tcow_gemm_args* a);                                  // gemm_f32.hip
int tcow_gemm_nt_x3(hipStream_t stream, const tcow_gemm_args* a);                                   // gemm_x3.hip

// ---- TN GEMM back ends (weight gradient): each launches its kernel into the slab as the plan (gemm_tn_plan.h) says; tcow_gemm_tn issues the fold
int tcow_gemm_tn_bf16(hipStream_t stream, const TnPlan& pl, int M, int N, int K, const bf16_t* dY, long ldy, const bf16_t* X, long ldx, float* slab,
                      float* bias_part);                                                            // gemm_tn_bf16.hip
int tcow_gemm_tn_bf16_group(hipStream_t stream, const TnGroupPlan& pl, int n, const tcow_tn_problem* pr, float* const* slabs, float* const* bias_parts);
int tcow_gemm_tn_f32(hipStream_t stream, const TnPlan& pl, int M, int N, int K, const float* dY, long ldy, const float* X, long ldx, float* slab);      // gemm_f32.hip
int tcow_gemm_tn_x3(hipStream_t stream, const TnPlan& pl, int M, int N, int K, const float* dY, long ldy, const float* X, long ldx, float* slab);       // gemm_x3.hip

// ---- the checks of a stream attention record (attention_stream.hip), reported under the entry point `who`: tcow_attn_temporal_step, and
// tcow_attn_temporal_step_probs (attention_stream_probs.hip), which does not ask for `out` (needs_out false)
int tcow_stream_attn_check(const char* who, const tcow_stream_attn_args* args, bool needs_out);

// ---- hand-off of a rollover stream pool (stream_requery.hip); tcow_requery_mask checks the arguments
int tcow_launch_requery_mask(hipStream_t stream, int n, long plane, const float* logits, long logits_len, const long* src_off, float threshold, float* mask,
                             const int* dst_rows, int n_dst, int* pixels);

// ---- reduction launchers (reduce.hip)
int tcow_launch_slab_reduce(hipStream_t stream, const float* slab, int nz, long slab_stride, long rows, long cols, float* out, long ldo, int accumulate,
                            const float* bias_part, int bias_nparts, int bias_n, float* bias_out);
bool tcow_fold_vec_ok(const float* slab, long slab_stride, long cols, float* out, long ldo);
int tcow_launch_slab_reduce_group(hipStream_t stream, int n, const float* const* slab, int nz, const long* rows, const long* cols, float* const* out, const long* ldo,
                                  const int* accumulate, const float* const* bias_part, const int* bias_nparts, float* const* bias_out);
int tcow_launch_row_reduce(hipStream_t stream, const float* part, int nrows, long ld, int N1, float* out1, int N2, float* out2, int N3, float* out3, int accumulate);
int tcow_launch_row_reduce_group(hipStream_t stream, int n, const float* const* part, const int* nrows, const long* ld, const int* N1, float* const* out1, const int* N2,
                                 float* const* out2, const int* N3, float* const* out3, const int* accumulate);
int tcow_launch_colsum(hipStream_t stream, int dtype, const void* Y, long ldy, int M, int N, float* out, int accumulate, float* part, int max_parts);
int tcow_launch_colsum_partials(hipStream_t stream, int dtype, const void* Y, long ldy, int M, int N, float* part, int max_parts, int* nparts);
