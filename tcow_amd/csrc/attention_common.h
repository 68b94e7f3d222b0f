// Sequence addressing shared by the attention kernels: a "sequence" is the list of token rows one softmax runs
// over -- T frames of one (clip, slot) for temporal attention, S slots of one (clip, frame) for spatial attention.
#pragma once
#include "common.h"

constexpr int ATT_HD = 64;    // head dim (all reference geometries: 768/12, 896/14, 1024/16)

struct SeqDesc {
    int n_outer, n_inner;                      // items = n_outer * n_inner
    long outer_stride, inner_stride, offset;   // base_row = outer*outer_stride + inner*inner_stride + offset
    long pos_stride;                           // rows between consecutive sequence positions
    int L;                                     // sequence length
    int diag;                                  // key allowed iff key_pos <= query_pos + diag (large = no mask)
    int heads, D;
};

__device__ __forceinline__ long seq_base(const SeqDesc& s, int item) {
    const int o = item / s.n_inner, i = item - o * s.n_inner;
    return o * s.outer_stride + i * s.inner_stride + s.offset;
}

// Work placement of the kernels in which several workgroups share one (sequence, head) "pair": the workgroups that own different query (key)
// chunks of the SAME pair stream the same K / V (Q / dO) tiles, so they should run at the same time on the same XCD (private L2): workgroups are
// dispatched round-robin over the 8 XCDs, so XCD x takes pairs x, x+8, ... and walks the chunks of one pair back to back.  (With the chunk in
// blockIdx.y the sharers ran a whole grid row apart and every chunk re-read its K / V from HBM: FETCH_SIZE 2.3x the algorithmic bytes.)
struct StreamWork { int pair, chunk; bool valid; };
__device__ __forceinline__ StreamWork stream_work(int pairs, int nchunk) {
    const int b = blockIdx.x, x = b & 7, k = b >> 3;
    const int i = k / nchunk;
    StreamWork w; w.chunk = k - i * nchunk; w.pair = 8 * i + x; w.valid = w.pair < pairs;
    return w;
}
static inline int stream_grid(int pairs, int nchunk) { return 8 * ((pairs + 7) / 8) * nchunk; }

// Causal tile ranges over the nt 32-position tiles of a sequence (key allowed iff key_pos <= query_pos + diag).  A workgroup's range is the
// same function of its last query tile / first key tile.
// key tiles [0, end) that query tile qt sees: its last query, 32 qt + 31, sees keys up to 32 qt + 31 + diag
__device__ __forceinline__ int causal_key_tiles(const SeqDesc& s, int nt, int qt) {
    const long klim = (long)32 * qt + 31 + s.diag;
    return klim >= (long)s.L - 1 ? nt : (int)(klim / 32) + 1;
}
// first query tile that sees any key of key tile j: q >= 32 j - diag
__device__ __forceinline__ int causal_first_query_tile(const SeqDesc& s, int j) {
    const long qlo = (long)32 * j - s.diag;
    return qlo > 0 ? (int)(qlo / 32) : 0;
}

static inline int diag_from_causal(int ca) {
    // vit.py:93-99: ca in {1,2}: tril(); ca >= 3: tril(diagonal=ca-2); ca <= 0: no mask.
    if (ca <= 0) return 1 << 28;
    return ca <= 2 ? 0 : ca - 2;
}
static inline SeqDesc temporal_desc(const tcow_attn_shape* s) {
    SeqDesc d;
    d.n_outer = s->B; d.n_inner = s->S - 1; d.outer_stride = (long)s->T * s->S; d.inner_stride = 1; d.offset = 1;
    d.pos_stride = s->S; d.L = s->T; d.diag = diag_from_causal(s->causal); d.heads = s->heads; d.D = s->D;
    return d;
}
static inline SeqDesc spatial_desc(const tcow_attn_shape* s) {
    // cls slot takes part iff causal_attention in {0,1} (vit.py:180-186 vs :202-208)
    const int s0 = (s->causal == 0 || s->causal == 1) ? 0 : 1;
    SeqDesc d;
    d.n_outer = s->B * s->T; d.n_inner = 1; d.outer_stride = s->S; d.inner_stride = 0; d.offset = s0;
    d.pos_stride = 1; d.L = s->S - s0; d.diag = 1 << 28; d.heads = s->heads; d.D = s->D;
    return d;
}

// Hand-off through wave-private LDS (some lanes write, other lanes of the SAME wave read; no workgroup barrier): a wave's LDS operations execute in
// order, so the hardware needs nothing -- a compiler barrier that emits no instruction would do.  What the hand-off does need is that hipcc keeps
// the reads after the writes, which it may not know to alias (accesses through different pointer types): TCOW_WAVE_LDS_ORDER.  TCOW_WAVE_LDS_FENCE also
// waits; it is what the exact-f32 one-tile kernels were measured with, and their code stays as it is.
#define TCOW_WAVE_LDS_ORDER() asm volatile("" ::: "memory")
#define TCOW_WAVE_LDS_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// ---- the attention back ends behind attention_api.hip's dispatch (host)
// 16-bit storage: MFMA flash attention (attention_bf16.hip)
bool tcow_attn_mfma_zeroes_slot0(const SeqDesc& d, bool shared, bool backward);
int tcow_attn_mfma_fwd(hipStream_t st, const SeqDesc& d, bool shared, const void* qkv, void* out, float* lse);
long tcow_attn_mfma_bwd_workspace_bytes(const SeqDesc& d);
int tcow_attn_mfma_bwd(hipStream_t st, const SeqDesc& d, bool shared, const void* qkv, const void* out, const void* dout, const float* lse, void* ws,
                       void* dqkv);
// f32 storage: exact-f32 MFMA (attention_f32.hip; dtype TCOW_F32)
int tcow_attn_f32_fwd(hipStream_t st, const SeqDesc& d, const void* qkv, void* out, float* lse);
int tcow_attn_f32_bwd(hipStream_t st, const SeqDesc& d, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv);
// f32 storage, split-bf16 MFMA arithmetic (attention_x3.hip; dtype TCOW_F32X3)
int tcow_attn_x3_fwd(hipStream_t st, const SeqDesc& d, const void* qkv, void* out, float* lse);
int tcow_attn_x3_bwd(hipStream_t st, const SeqDesc& d, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv);
