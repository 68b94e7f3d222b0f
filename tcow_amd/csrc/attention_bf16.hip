// 16-bit MFMA flash-style attention for the divided space-time blocks (gfx950), forward and backward: the dispatch to three kernel families.
//
// Replaces softmax(q k^T / 8 [causal]) v of Attention.forward (vit.py:88-109) without materialising the
// (T,T) / (S,S) score matrices the reference builds (13 MB + 130 MB f32 per block at the default config).
//
// Work unit = one 32-query tile against 32-key tiles, d = 64, on v_mfma_f32_32x32x16_bf16:
//   S^T = K Q^T    (A = K rows from LDS, B = Q rows)      -> lane (q = lane&31, hi) holds 16 keys of its query, so the
//                                                             softmax row statistics are lane-local (+1 exchange with lane^32)
//   O^T += V^T P^T (A = V gathered with ds_read_b64_tr_b16, B = P straight from the S^T accumulator registers)
// Token rows come straight from the qkv GEMM output [rows, 3D] (128-byte head slices, 1 cache line each) through
// direct-to-LDS loads.  LDS tiles are [32 rows][64 bf16]; 16-byte chunk c of row r is stored at chunk position
// c ^ g(r), g(r) = ((r>>1)&1)<<2 | ((r>>2)&3), which is conflict-free for both the ds_read_b128 row fragments and
// the transpose reads (applied on the SOURCE address: the LDS image of a direct-to-LDS load stays lane-linear).
// The tile helpers and tile steps are in attention_tiles.h.
//
// Backward (recompute from the saved log-sum-exp, delta = rowsum(dO * O)):
//   dK / dV: a wave owns key tile j: S = Q K^T and dP = dO V^T in the (rows = q in registers, cols = key in lanes)
//            orientation, so P and dS feed dV += P^T dO, dK += dS^T Q as A operands without any shuffle.
//   dQ     : a wave owns query tile i: S^T, dP^T in the forward orientation, dQ += dS K.
//
// Families (nt = number of 32-position tiles of a sequence; "shared" = spatial attention, a sequence per (clip, frame, head)), one file each:
//   wave-private (attention_bf16_private.inc): temporal sequences of nt <= 2.  One wave per (clip, slot, head) with wave-private LDS tiles, no
//                barriers.  Forward attn_fwd_mfma; backward attn_bwd_one_tile at nt = 1, attn_bwd_prep_kernel + attn_bwd_dkv_mfma + attn_bwd_dq_mfma
//                at nt = 2.  The forward, and the backward at nt = 1, also write the zero rows of the skipped slot 0.
//   chunked      (attention_bf16_chunked.inc): any length -- spatial sequences and temporal ones of nt > 2.  A 256-thread workgroup owns 4 query
//                (or key) tiles of one (sequence, head), one per wave, and walks the other side in chunks of 4 or 5 tiles through 32 / 40 KiB of LDS.
//                Forward attn_fwd_stream_nc without a causal mask (nt >= 2), attn_fwd_stream with one; backward attn_bwd_dq_stream + attn_bwd_dkv_stream.
//   one kernel   (attention_bf16_one.inc): the backward of spatial sequences of 4 <= nt <= 10.  One 12-wave workgroup per (frame, head) forms dQ, dK
//                and dV from a single visit of every (query tile, key tile) pair: attn_bwd_one_kernel.
// The three files are included here and compiled as ONE translation unit, on purpose: the machine code hipcc makes of a kernel changes with the set
// of kernels compiled next to it (it simplifies the shared always-inline tile helpers before it inlines them, evidently with what the module shows of
// their callers): attn_bwd_dkv_stream went from 237 to 239 registers when the families were built apart (profiles/attention_split_isa.txt).
// (The resident / persistent forward variants that were measured and not adopted are in tools/attn_fwd_variants.inc.)
#include <stdlib.h>

#include "attention_common.h"

#include "attention_tiles.h"

#include "attention_bf16_private.inc"
#include "attention_bf16_chunked.inc"
#include "attention_bf16_one.inc"

// chunked backward kernels: tiles per LDS chunk -- 5 when that saves a chunk round (nt = 10: two rounds instead of three), else 4
static bool stream_ch5(int nt) { return (nt + 4) / 5 < (nt + 3) / 4; }

// true when the kernel this shape dispatches to writes the zero rows of the skipped slot 0 itself (wave-private temporal kernels)
bool tcow_attn_mfma_zeroes_slot0(const SeqDesc& d, bool shared, bool backward) {
    const int nt = (d.L + 31) / 32;
    if (shared || d.offset != 1 || d.inner_stride != 1 || d.n_inner < 1) return false;
    return backward ? nt == 1 : nt <= 2;
}

int tcow_attn_mfma_fwd(hipStream_t st, const SeqDesc& d, bool shared, const void* qkv, void* out, float* lse) {
    const int nt = (d.L + 31) / 32;
    if (shared || nt > 2) return tcow_attn_chunked_fwd(st, d, nt, qkv, out, lse);
    return tcow_attn_private_fwd(st, d, nt, qkv, out, lse, tcow_attn_mfma_zeroes_slot0(d, shared, false) ? 1 : 0);
}

// the packed (lse, delta) table of the two- and three-kernel backward paths
long tcow_attn_mfma_bwd_workspace_bytes(const SeqDesc& d) {
    const int nt = (d.L + 31) / 32;
    return (long)d.n_outer * d.n_inner * d.heads * nt * 32 * 8;
}

int tcow_attn_mfma_bwd(hipStream_t st, const SeqDesc& d, bool shared, const void* qkv, const void* out, const void* dout, const float* lse, void* ws,
                       void* dqkv) {
    const int nt = (d.L + 31) / 32;
    if (!shared && nt == 1) return tcow_attn_private_bwd_one_tile(st, d, qkv, dout, lse, dqkv, tcow_attn_mfma_zeroes_slot0(d, shared, true) ? 1 : 0);
    // spatial sequences of four to ten tiles: the one-kernel backward (221 -> 150 us at S = 301 against the two chunked kernels, which longer
    // sequences keep)
    if (shared && nt <= ONE_MAX_NT && nt >= 4) return tcow_attn_one_bwd(st, d, nt, qkv, out, dout, lse, dqkv);
    if (shared || nt > 2) return tcow_attn_chunked_bwd(st, d, nt, stream_ch5(nt), qkv, out, dout, lse, ws, dqkv);
    return tcow_attn_private_bwd(st, d, nt, qkv, out, dout, lse, ws, dqkv);
}
