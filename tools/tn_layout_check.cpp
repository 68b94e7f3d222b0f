// Host check of the LDS image of the 256-tile weight-gradient GEMM (tcow_amd/csrc/gemm_tn_layout.h): enumerates every lane of every
// direct-to-LDS load, transpose read and column-sum read of one stage.  Build: c++ -std=c++17 -O1 -I tcow_amd/csrc tools/tn_layout_check.cpp
// Exit status 0 and a last line "ok" when
//   1. the loads of the 8 waves write every (token row, column) of the tile exactly once,
//   2. every transpose read hands lane l column col0 + (l & 15) and tokens 32 step + 8 (l >> 4) + {0 ... 3} (+ 4 for the "hi" read) -- the
//      16x16x32 operand layout --, and over the fragments of the wave rows (dY: 2 x 8) / wave columns (X: 4 x 4) every element is read once,
//   3. the column-sum read of (row, chunk) returns columns 8 chunk ... + 7 of that row,
//   4. under the bank model (bank = (byte address / 4) mod 64; only lanes of one group conflict; equal addresses broadcast) each 32-lane
//      half of every transpose read and each 16-lane group of every 16-byte column-sum read is conflict-free.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "gemm_tn_layout.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails < 20) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

struct Elem { int row, col; };

// most distinct addresses that lanes `lanes` put on one bank; `bytes` per lane at addr[lane]
static int worst_bank(const int* addr, const std::vector<int>& lanes, int bytes) {
    std::set<int> on_bank[64];
    for (int l : lanes)
        for (int b = 0; b < bytes; b += 4) on_bank[((addr[l] + b) / 4) % 64].insert(addr[l]);
    size_t w = 0;
    for (auto& s : on_bank) w = s.size() > w ? s.size() : w;
    return (int)w;
}

int main() {
    // ---- 1: the image the loads leave: element at every 2-byte LDS position
    std::vector<Elem> img(TNL_TILE / 2, Elem{-1, -1});
    std::vector<int> written(TNL_ROWS * TNL_COLS, 0);
    for (int wave = 0; wave < 8; ++wave)
        for (int j = 0; j < 4; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const int row = tnl_load_row(wave, j, lane), chunk = tnl_load_chunk(wave, j, lane), dst = tnl_load_dst(wave, j, lane);
                CHECK(row >= 0 && row < TNL_ROWS && chunk >= 0 && chunk < 32 && dst >= 0 && dst + 16 <= TNL_TILE && dst % 16 == 0, "load out of range: wave %d j %d lane %d", wave, j, lane);
                CHECK(dst == tnl_off(row, chunk), "load wave %d j %d lane %d: chunk %d of row %d lands at %d, the image has it at %d", wave, j, lane, chunk, row, dst, tnl_off(row, chunk));
                CHECK(tnl_load_chunk(wave, j, lane) == tnl_load_chunk(wave & 1, j & 1, lane), "load source chunk depends on more than (wave & 1, j & 1)");
                for (int e = 0; e < 8; ++e) {
                    CHECK(img[dst / 2 + e].row < 0, "LDS byte %d written twice", dst + 2 * e);
                    img[dst / 2 + e] = Elem{row, chunk * 8 + e};
                    ++written[row * TNL_COLS + chunk * 8 + e];
                }
            }
    for (int i = 0; i < TNL_ROWS * TNL_COLS; ++i) CHECK(written[i] == 1, "element (row %d, col %d) written %d times", i / TNL_COLS, i % TNL_COLS, written[i]);

    // ---- 2 + 4: transpose reads.  groups: number of wave rows / columns that split the tile, frags: 16-column fragments per wave
    auto reads = [&](const char* name, int groups, int frags) {
        int worst = 0;
        for (int w = 0; w < groups; ++w) {
            std::vector<int> seen(TNL_ROWS * TNL_COLS, 0);
            for (int f = 0; f < frags; ++f)
                for (int step = 0; step < TNL_ROWS / TNL_STEP; ++step)
                    for (int hi = 0; hi < 2; ++hi) {
                        const int col0 = (w * frags + f) * 16;
                        int addr[64];
                        for (int l = 0; l < 64; ++l) {
                            addr[l] = tnl_read_off(l, col0, step) + hi * TNL_HI;
                            CHECK(addr[l] % 8 == 0 && addr[l] >= 0 && addr[l] + 8 <= TNL_TILE, "%s read: lane %d address %d", name, l, addr[l]);
                        }
                        for (int l = 0; l < 64; ++l)
                            for (int q = 0; q < 4; ++q) {
                                // lane i of a 16-lane group receives, as element q, column i of the block row whose address lanes 4 q ... 4 q + 3 supply
                                const int g = l & ~15, i = l & 15;
                                const Elem e = img[(addr[g + 4 * q + (i >> 2)] + 2 * (i & 3)) / 2];
                                const int want_row = TNL_STEP * step + 8 * (l >> 4) + 4 * hi + q, want_col = col0 + i;
                                CHECK(e.row == want_row && e.col == want_col, "%s frag col0 %d step %d hi %d lane %d element %d: got (row %d, col %d), the MFMA operand wants (%d, %d)",
                                      name, col0, step, hi, l, q, e.row, e.col, want_row, want_col);
                                if (e.row >= 0) ++seen[e.row * TNL_COLS + e.col];
                            }
                        for (int half = 0; half < 2; ++half) {
                            std::vector<int> lanes;
                            for (int l = 32 * half; l < 32 * half + 32; ++l) lanes.push_back(l);
                            const int wb = worst_bank(addr, lanes, 8);
                            worst = wb > worst ? wb : worst;
                        }
                    }
            const int c0 = w * frags * 16, c1 = c0 + frags * 16;
            for (int r = 0; r < TNL_ROWS; ++r)
                for (int c = 0; c < TNL_COLS; ++c)
                    CHECK(seen[r * TNL_COLS + c] == ((c >= c0 && c < c1) ? 1 : 0), "%s wave group %d: element (row %d, col %d) read %d times", name, w, r, c, seen[r * TNL_COLS + c]);
        }
        std::printf("%s transpose reads: worst case %d address(es) per bank in a 32-lane half\n", name, worst);
        CHECK(worst == 1, "%s transpose reads have a %d-way bank conflict", name, worst);
    };
    reads("dY", 2, 8);       // wave row wm: columns 128 wm ... + 127, eight fragments
    reads("X", 4, 4);        // wave column wn: columns 64 wn ... + 63, four fragments

    // ---- 3 + 4: column-sum reads: thread t reads chunk t & 31 of rows lo + (t >> 5) + 16 u; the 16-lane groups of a 16-byte read
    static const int G128[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    int worst = 0;
    for (int row = 0; row < TNL_ROWS; ++row)
        for (int chunk = 0; chunk < 32; ++chunk) {
            const int off = tnl_colsum_off(row, chunk);
            for (int e = 0; e < 8; ++e) CHECK(img[off / 2 + e].row == row && img[off / 2 + e].col == chunk * 8 + e, "column-sum read of (row %d, chunk %d) element %d is (row %d, col %d)", row, chunk, e, img[off / 2 + e].row, img[off / 2 + e].col);
        }
    for (int lo = 0; lo < TNL_ROWS; ++lo)
        for (int wave = 0; wave < 8; ++wave)
            for (int u = 0; u < 4; ++u) {
                int addr[64]; bool live[64];
                for (int l = 0; l < 64; ++l) {
                    const int t = wave * 64 + l, r = lo + (t >> 5) + 16 * u;
                    live[l] = r < TNL_ROWS;
                    addr[l] = live[l] ? tnl_colsum_off(r, t & 31) : 0;
                }
                for (auto& grp : G128) {
                    std::vector<int> lanes;
                    for (int l : grp) if (live[l]) lanes.push_back(l);
                    const int wb = worst_bank(addr, lanes, 16);
                    worst = wb > worst ? wb : worst;
                }
            }
    std::printf("column-sum reads: worst case %d address(es) per bank in a 16-lane group\n", worst);
    CHECK(worst == 1, "column-sum reads have a %d-way bank conflict", worst);

    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
