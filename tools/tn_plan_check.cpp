// Host check of the plan of the weight-gradient GEMMs (tcow_amd/csrc/gemm_tn_plan.h), the header the library itself reads.
// Build: c++ -std=c++17 -O1 -I tcow_amd/csrc tools/tn_plan_check.cpp
//   tn_plan_check                                       the sweep below; exit status 0 and a last line "ok"
//   tn_plan_check one <dtype> M N K <bias 0|1> [ldy ldx]   that problem's plan as key=value pairs (dtype: 0 f32, 1 16-bit, 2 bf16 x 3)
//   tn_plan_check group <dtype> (M N K ldy ldx)...      that group's plan: one line per problem, then the group's line
// The sweep: M over 1 ... 700, 4000 ... 5000 and a few large values, N and K over tile multiples, ragged sizes and the bias table's edges, every dtype,
// with and without a bias gradient; the group sets of tests/test_gpu_gemm_tn.py and test_gpu_gemm_tn_k32.py over a row sweep.  For every plan
//   1. nz <= slices requested, 1 <= rows of the last slice <= rows per slice, rows per slice a multiple of the kernel's stage;
//   2. a fused bias gradient writes no more table rows than the table has (a group's table: than the group layout reserves);
//   3. the slab images written and the table lie inside the total, do not overlap, and are 16-byte aligned wherever N and K are multiples of 4
//      (what the vector fold asks of a slab);
//   4. the total of a group is not below that of any member (a group that does not group runs in the same workspace).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_tn_plan.h"

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

static const char* kKernel[] = {"none", "128-tile", "256-tile_SCHED_1", "256-tile_SCHED_2", "f32", "x3"};
static const char* kBias[] = {"none", "fused", "partials", "colsum"};

static void check_slices(int M, int splits, int mps, int nz, int stage, const char* what) {
    const int last = M - (nz - 1) * mps;
    CHECK(nz >= 1 && nz <= splits, "%s: nz %d, %d requested", what, nz, splits);
    CHECK(last >= 1 && last <= mps, "%s: last slice %d of %d rows", what, last, mps);
    CHECK(stage > 0 && mps % stage == 0, "%s: %d rows per slice, stage %d", what, mps, stage);
}

static void check_one(int dtype, int M, int N, int K, bool bias) {
    const TnPlan p = tcow_tn_plan(dtype, M, N, K, N, K, bias);
    char what[96];
    std::snprintf(what, sizeof what, "dtype %d (%d, %d, %d) bias %d", dtype, M, N, K, (int)bias);
    CHECK(p.kernel != TN_KNONE, "%s", what);
    check_slices(M, p.splits, p.mps, p.nz, p.stage, what);
    CHECK(p.tiles_n >= 1 && p.tiles_k >= 1, "%s", what);
    CHECK((p.bias != TN_BIAS_NONE) == bias, "%s", what);
    const int rows = p.bias == TN_BIAS_FUSED ? p.table_rows : p.bias == TN_BIAS_NONE ? 0 : TN_COLSUM_PARTS;
    CHECK(rows <= TN_TABLE_ROWS, "%s: %d table rows written, %d reserved", what, rows, TN_TABLE_ROWS);
    if (p.bias == TN_BIAS_FUSED) CHECK(p.table_rows == p.nz * p.tiles_k * 2 && p.rows_per_pk >= 1 && p.rows_per_pk <= p.stage, "%s", what);
    const long slab_end = p.slab_off + (long)p.nz * N * K * 4, table_end = p.table_off + (long)TN_TABLE_ROWS * N * 4;
    CHECK(p.slab_off >= 0 && slab_end <= p.table_off && table_end <= p.total, "%s: slab [%ld, %ld) table [%ld, %ld) total %ld", what, p.slab_off, slab_end, p.table_off, table_end, p.total);
    CHECK(p.slab_off % 16 == 0 && (N % 4 || K % 4 || p.table_off % 16 == 0), "%s: alignment", what);
    CHECK(p.total == tcow_tn_workspace_total(M, N, K), "%s", what);
}

static tcow_tn_problem problem(int M, int N, int K, long ldy, long ldx, bool bias = true, int accumulate = 0, long lddw = 0) {
    static float dummy[8];
    tcow_tn_problem q = {};
    q.M = M; q.N = N; q.K = K; q.ldy = ldy; q.ldx = ldx; q.dW = (float*)4096; q.lddw = lddw ? lddw : K; q.bias_grad = bias ? dummy : nullptr; q.accumulate = accumulate;
    return q;
}

static void check_group(int dtype, const std::vector<tcow_tn_problem>& pr, const char* name) {
    const int n = (int)pr.size();
    const TnGroupPlan g = tcow_tn_group_plan(dtype, n, pr.data());
    for (const tcow_tn_problem& q : pr) CHECK(g.total >= tcow_tn_workspace_total(q.M, q.N, q.K), "%s", name);
    if (!g.grouped) return;
    check_slices(pr[0].M, g.splits, g.mps, g.nz, TNL_ROWS, name);
    long end = 0; int wg = 0;
    for (int i = 0; i < n; ++i) {
        const TnPlan& p = g.p[i];
        const long N = pr[i].N, K = pr[i].K;
        CHECK(p.first == wg, "%s problem %d", name, i);
        wg += g.nz * p.tiles_n * p.tiles_k;
        CHECK(p.table_rows <= (g.splits + 1) * p.tiles_k * 2 && (p.table_rows == 0) == (pr[i].bias_grad == nullptr), "%s problem %d: table rows", name, i);
        CHECK(p.slab_off >= end && p.slab_off + g.nz * N * K * 4 <= p.table_off, "%s problem %d: slab", name, i);
        end = p.table_off + (long)(g.splits + 1) * p.tiles_k * 2 * N * 4;
        CHECK(p.slab_off % 16 == 0 && p.table_off % 16 == 0, "%s problem %d: alignment", name, i);
        CHECK(!p.in_place || (g.nz == 1 && !pr[i].accumulate && pr[i].lddw == K), "%s problem %d: in place", name, i);
    }
    CHECK(wg == g.workgroups && end <= g.total, "%s: %d workgroups, end %ld of %ld", name, wg, end, g.total);
}

static int sweep() {
    std::vector<int> Ms, Ns = {8, 72, 136, 256, 264, 768, 776, 2304, 3072}, Ks = Ns;
    for (int M = 1; M <= 700; ++M) Ms.push_back(M);
    for (int M = 4000; M <= 5000; ++M) Ms.push_back(M);
    for (int M : {8192, 16383, 16384, 27090, 36120, 65536, 100000, 1 << 20}) Ms.push_back(M);
    for (int K : {520, 4224, 16640, 24704}) Ks.push_back(K);
    long plans = 0;
    for (int dtype : {TCOW_F32, TCOW_BF16, TCOW_F32X3})
        for (int M : Ms)
            for (int N : Ns)
                for (int K : Ks)
                    for (int bias = 0; bias < 2; ++bias, ++plans) check_one(dtype, M, N, K, bias != 0);
    CHECK(tcow_tn_plan(7, 512, 64, 64, 64, 64, true).kernel == TN_KNONE, "an unknown dtype has no kernel");

    long groups = 0;
    std::vector<int> GMs = {27090, 36120};
    for (int M = 4096; M <= 4230; ++M) GMs.push_back(M);
    const int vitb[7][2] = {{2304, 768}, {768, 768}, {768, 768}, {2304, 768}, {768, 768}, {3072, 768}, {768, 3072}};
    for (int M : GMs) {
        std::vector<tcow_tn_problem> g7a = {problem(M, 768, 768, 776, 776), problem(M, 776, 520, 784, 528, false, 1, 528), problem(M, 256, 2304, 264, 2312, true, 1, 2312)};
        std::vector<tcow_tn_problem> g7c = {problem(M, 2048, 2048, 2056, 2056), problem(M, 1024, 4096, 1032, 4104, true, 1), problem(M, 4096, 1024, 4104, 1032, true, 0, 1032),
                                            problem(M, 2048, 2048, 2056, 2056, false)};
        std::vector<tcow_tn_problem> many, pairs, blocks, diff = {problem(M, 768, 768, 776, 776), problem(M + 67, 768, 768, 776, 776), problem(513, 264, 136, 272, 144)};
        for (int i = 0; i < TCOW_TN_GROUP_MAX + 1; ++i) many.push_back(problem(M, 768, 768, 776, 776, i % 3 != 1, i % 4 == 2, i % 2 ? 776 : 768));
        for (int i = 0; i < 14; ++i) pairs.push_back(problem(M, i % 2 ? 2304 : 768, 768, i % 2 ? 2304 : 768, 768));
        for (int i = 0; i < 35; ++i) blocks.push_back(problem(M, vitb[i % 7][0], vitb[i % 7][1], vitb[i % 7][0], vitb[i % 7][1]));
        for (int dtype : {TCOW_F32, TCOW_BF16, TCOW_F32X3}) {
            check_group(dtype, g7a, "7a"); check_group(dtype, g7c, "7c"); check_group(dtype, diff, "7f"); check_group(dtype, many, "7e");
            check_group(dtype, std::vector<tcow_tn_problem>(many.begin(), many.begin() + TCOW_TN_GROUP_MAX), "7d");
            check_group(dtype, std::vector<tcow_tn_problem>(pairs.begin(), pairs.begin() + 2), "k32 pair"); check_group(dtype, pairs, "k32 seven pairs");
            for (int b = 1; b <= 5; ++b) check_group(dtype, std::vector<tcow_tn_problem>(blocks.begin(), blocks.begin() + 7 * b), "vitb blocks");
            groups += 12;
        }
    }
    std::printf("%ld plans, %ld groups, %ld failures\n", plans, groups, fails);
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return sweep();
    if (!std::strcmp(argv[1], "one") && (argc == 7 || argc == 9)) {
        const int dtype = std::atoi(argv[2]), M = std::atoi(argv[3]), N = std::atoi(argv[4]), K = std::atoi(argv[5]);
        const TnPlan p = tcow_tn_plan(dtype, M, N, K, argc == 9 ? std::atol(argv[7]) : N, argc == 9 ? std::atol(argv[8]) : K, std::atoi(argv[6]) != 0);
        std::printf("kernel=%s  splits=%d  mps=%d  nz=%d  last=%d  stage=%d  tiles_n=%d  tiles_k=%d  rows_per_pk=%d  bias=%s  table_rows=%d  table_reserved=%d  slab_off=%ld  table_off=%ld  total=%ld\n",
                    kKernel[p.kernel + 1], p.splits, p.mps, p.nz, p.mps ? M - (p.nz - 1) * p.mps : 0, p.stage, p.tiles_n, p.tiles_k, p.rows_per_pk, kBias[p.bias], p.table_rows,
                    TN_TABLE_ROWS, p.slab_off, p.table_off, p.total);
        return 0;
    }
    if (!std::strcmp(argv[1], "group") && argc >= 8 && (argc - 3) % 5 == 0) {
        std::vector<tcow_tn_problem> pr;
        for (int a = 3; a < argc; a += 5) pr.push_back(problem(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), std::atol(argv[a + 3]), std::atol(argv[a + 4])));
        const TnGroupPlan g = tcow_tn_group_plan(std::atoi(argv[2]), (int)pr.size(), pr.data());
        for (size_t i = 0; g.grouped && i < pr.size(); ++i)
            std::printf("problem=%zu  tiles_n=%d  tiles_k=%d  rows_per_pk=%d  table_rows=%d  first=%d  in_place=%d  slab_off=%ld  table_off=%ld\n", i, g.p[i].tiles_n, g.p[i].tiles_k,
                        g.p[i].rows_per_pk, g.p[i].table_rows, g.p[i].first, (int)g.p[i].in_place, g.p[i].slab_off, g.p[i].table_off);
        std::printf("grouped=%d  kernel=%s  splits=%d  mps=%d  nz=%d  last=%d  workgroups=%d  total=%ld\n", (int)g.grouped, g.grouped ? kKernel[g.kernel + 1] : "none", g.splits, g.mps,
                    g.nz, g.grouped ? pr[0].M - (g.nz - 1) * g.mps : 0, g.workgroups, g.total);
        return 0;
    }
    std::fprintf(stderr, "usage: tn_plan_check | tn_plan_check one <dtype> M N K <bias> [ldy ldx] | tn_plan_check group <dtype> (M N K ldy ldx)...\n");
    return 2;
}
