// LDS image of the 256-tile weight-gradient GEMM (gemm_tn_256.inc, tn256_body): where the direct-to-LDS loads put a stage, and where the transpose
// reads of the 16x16x32 MFMA operands and the column-sum reads find it.  Plain constexpr functions of integers, shared by the kernel and by the
// host program tools/tn_layout_check.cpp, which enumerates every lane of every load and read (tests/test_gemm_tn_plan_host.py runs it on the CPU).
//
// One operand tile of a stage is [64 token rows][256 columns] of 16-bit elements: 512-byte rows of 32 chunks of 16 bytes.  Chunk c of row r sits
// at chunk position c ^ tnl_swz(r).  A 16x16x32 operand fragment is 16 columns x 32 tokens, lane l holding column l & 15 and tokens
// 8 (l >> 4) ... + 7; one ds_read_b64_tr_b16 gathers, per 16-lane group, a block of 4 token rows x 16 columns (32 bytes of each row), so a
// 32-lane bank group touches the eight rows {b ... b + 3, b + 8 ... b + 11} of one 32-byte column piece.  Rows are 512 bytes apart and the
// bank is (address / 4) mod 64, so unswizzled all eight pieces would share 8 banks: row bits 0-1 move the piece by 64 and 128 bytes (chunk
// bits 2-3) and row bit 3 by 32 bytes (chunk bit 1) -- eight different 32-byte segments of the 256-byte bank row.  Chunk bit 0 is never
// touched: the two chunks of a 32-byte piece stay adjacent, and rows r and r + 4 (the "lo" and "hi" read of a fragment) share one swizzle.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TNL_FN __host__ __device__ __forceinline__ constexpr
#else
#define TNL_FN inline constexpr
#endif

constexpr int TNL_COLS = 256;                    // columns of an operand tile
constexpr int TNL_ROWS = 64;                     // token rows of a stage
constexpr int TNL_ROWB = TNL_COLS * 2;           // bytes of an LDS row
constexpr int TNL_TILE = TNL_ROWS * TNL_ROWB;    // bytes of one operand of one stage
constexpr int TNL_STEP = 32;                     // token rows of one MFMA step

TNL_FN int tnl_swz(int row) { return ((row & 3) << 2) ^ (((row >> 3) & 1) << 1); }
// byte offset, from the tile base, of 16-byte chunk `chunk` (0 ... 31) of token row `row` (0 ... 63)
TNL_FN int tnl_off(int row, int chunk) { return row * TNL_ROWB + ((chunk ^ tnl_swz(row)) << 4); }

// ---- direct-to-LDS loads.  Wave-load j (0 ... 3) of wave w (0 ... 7) writes 1024 contiguous bytes, 16 per lane, at tnl_load_dst: token rows
// 8 w + 2 j and + 1.  The lane fetches the source chunk that belongs at its position; that chunk depends on j only through j & 1 and on w only
// through w & 1 (row bits 1 and 3), so a lane keeps two source columns per operand.
TNL_FN int tnl_load_row(int wave, int j, int lane) { return 8 * wave + 2 * j + (lane >> 5); }
TNL_FN int tnl_load_dst(int wave, int j, int lane) { return (wave * 4 + j) * 1024 + lane * 16; }
TNL_FN int tnl_load_chunk(int wave, int j, int lane) { return (lane & 31) ^ tnl_swz(tnl_load_row(wave, j, lane)); }

// ---- transpose reads.  Address of lane `lane` for the "lo" read (tokens + 0 ... 3 of the lane's eight) of the fragment of columns col0 ... col0 + 15
// (col0 a multiple of 16) in MFMA step `step` (0, 1); the "hi" read (tokens + 4 ... 7) is TNL_HI bytes further.  In its 16-lane group lane 4 q + p
// supplies row q, columns 4 p ... 4 p + 3 of the block and receives column (lane & 15), rows 0 ... 3.
constexpr int TNL_HI = 4 * TNL_ROWB;
TNL_FN int tnl_read_row(int lane, int step) { return TNL_STEP * step + 8 * (lane >> 4) + ((lane & 15) >> 2); }
TNL_FN int tnl_read_off(int lane, int col0, int step) { return tnl_off(tnl_read_row(lane, step), (col0 >> 3) + ((lane & 3) >> 1)) + (lane & 1) * 8; }

// ---- column sums (bias gradient): one 16-byte read of chunk `chunk` of row `row`
TNL_FN int tnl_colsum_off(int row, int chunk) { return tnl_off(row, chunk); }
