// Output-tile edges and token rows per stage of the GEMM kernels whose host rules (gemm_tn_plan.h) need them outside the kernel's own source: plain
// constants, no HIP types.  (The 256-tile weight-gradient kernel's are TNL_COLS / TNL_ROWS of gemm_tn_layout.h.)
#pragma once

constexpr int FT = 64;                    // gemm_f32.hip: tile edge
constexpr int FK = 16;                    //               k-slice
constexpr int XT = 128;                   // gemm_x3.hip: tile edge
constexpr int XK = 32;                    //              k-slice
constexpr int TN_T = 128;                 // gemm_tn_128.inc: output tile edge (n and k)
constexpr int TN_MC = 32;                 //                token rows per LDS stage: 32 KiB of LDS, 4 workgroups/CU (64 rows, 2 workgroups/CU: 5-25 % behind, profiles/r01_gemm_tn_ab.txt)
