// C ABI glue of libtcow_hip.so: argument validation, dtype dispatch, thread-local error text.
#include <stdarg.h>
#include <stdio.h>

#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "common.h"
#include "internal.h"

static thread_local char g_err[512] = "";

void tcow_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device property of a kernel: remember (device, kernel) pairs so that a
// process driving several GPUs (torch.nn.DataParallel replicas are threads of one process, train.py:222-223) sets it on each.
void tcow_ensure_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.insert(std::make_pair(dev, kernel)).second)
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

extern "C" {

int tcow_version(void) { return TCOW_ABI_VERSION; }
const char* tcow_last_error(void) { return g_err; }

// ---- optional low-overhead HIP-event timing of the dominant kernel (the NT GEMM), on the launch stream
static std::vector<hipEvent_t> g_prof_events;
static std::vector<double> g_prof_flops;
static size_t g_prof_used = 0;
static bool g_prof_on = false;
static std::mutex g_prof_mu;   // the profiling aid is process-wide: one measuring thread at a time, launches from others are serialised here

int tcow_prof_gemm_begin(int max_launches) {
    TCOW_CHECK_ARG(max_launches > 0, "tcow_prof_gemm_begin: max_launches must be positive");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    while (g_prof_events.size() < (size_t)max_launches * 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { tcow_set_error("tcow_prof_gemm_begin: hipEventCreate failed"); return TCOW_ERR_LAUNCH; }
        g_prof_events.push_back(e);
    }
    g_prof_flops.assign(max_launches, 0.0);
    g_prof_used = 0;
    g_prof_on = true;
    return TCOW_OK;
}

int tcow_prof_gemm_end(double* total_ms, double* total_flops, long* launches) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on = false;
    double ms = 0.0, fl = 0.0;
    for (size_t i = 0; i < g_prof_used; ++i) {
        if (hipEventSynchronize(g_prof_events[2 * i + 1]) != hipSuccess) { tcow_set_error("tcow_prof_gemm_end: event sync failed"); return TCOW_ERR_LAUNCH; }
        float t = 0.f;
        (void)hipEventElapsedTime(&t, g_prof_events[2 * i], g_prof_events[2 * i + 1]);
        ms += t; fl += g_prof_flops[i];
    }
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    if (launches) *launches = (long)g_prof_used;
    return TCOW_OK;
}

static int gemm_nt_dispatch(void* stream, const tcow_gemm_args* a);

int tcow_gemm_nt(void* stream, const tcow_gemm_args* a) {
    if (!g_prof_on) return gemm_nt_dispatch(stream, a);
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof_on || a == nullptr || g_prof_used >= g_prof_flops.size()) return gemm_nt_dispatch(stream, a);
    const size_t i = g_prof_used++;
    g_prof_flops[i] = 2.0 * a->M * (double)a->N * a->K;
    (void)hipEventRecord(g_prof_events[2 * i], (hipStream_t)stream);
    const int rc = gemm_nt_dispatch(stream, a);
    (void)hipEventRecord(g_prof_events[2 * i + 1], (hipStream_t)stream);
    return rc;
}

static int gemm_nt_dispatch(void* stream, const tcow_gemm_args* a) {
    TCOW_CHECK_ARG(a != nullptr, "tcow_gemm_nt: null args");
    TCOW_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "tcow_gemm_nt: bad shape M=%d N=%d K=%d", a->M, a->N, a->K);
    TCOW_CHECK_ARG(a->A && a->W && a->C, "tcow_gemm_nt: null operand");
    TCOW_CHECK_ARG((a->act != TCOW_ACT_DGELU && a->act != TCOW_ACT_GELU_DSAVE && a->act != TCOW_ACT_MUL_AUX) || a->aux, "tcow_gemm_nt: this activation needs aux");
    TCOW_CHECK_ARG(a->act >= TCOW_ACT_NONE && a->act <= TCOW_ACT_MUL_AUX, "tcow_gemm_nt: unknown activation %d", a->act);
    TCOW_CHECK_ARG(a->bias2 || !a->row_scale2, "tcow_gemm_nt: row_scale2 without bias2");
    if (a->dtype == TCOW_BF16) {
        return tcow_gemm_nt_bf16((hipStream_t)stream, a);
    }
    if (a->dtype == TCOW_F32) return tcow_gemm_nt_f32((hipStream_t)stream, a);
    if (a->dtype == TCOW_F32X3) return tcow_gemm_nt_x3((hipStream_t)stream, a);
    tcow_set_error("tcow_gemm_nt: unknown dtype %d", a->dtype);
    return TCOW_ERR_INVALID_ARG;
}

// ---- skinny-M NT GEMM (gemm_nt_skinny.hip): 64 x 64 tiles with a deterministic split over K, for the streaming steps
long tcow_gemm_nt_skinny_workspace_bytes(int M, int N, int split) {
    if (M <= 0 || N <= 0 || split <= 1) return 0;
    return (long)split * M * N * 4;
}

// What both entry points ask of a call, in one place; the dtype, the operand pitches and alignment are each entry point's own.
static int check_skinny_args(const char* who, const tcow_gemm_args* a, int split, void* ws, long ws_bytes) {
    TCOW_CHECK_ARG(a != nullptr, "%s: null args", who);
    TCOW_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "%s: bad shape M=%d N=%d K=%d", who, a->M, a->N, a->K);
    TCOW_CHECK_ARG(a->A && a->W && a->C, "%s: null operand", who);
    TCOW_CHECK_ARG((a->act != TCOW_ACT_DGELU && a->act != TCOW_ACT_GELU_DSAVE && a->act != TCOW_ACT_MUL_AUX) || a->aux, "%s: this activation needs aux", who);
    TCOW_CHECK_ARG(a->act >= TCOW_ACT_NONE && a->act <= TCOW_ACT_MUL_AUX, "%s: unknown activation %d", who, a->act);
    TCOW_CHECK_ARG(a->bias2 || !a->row_scale2, "%s: row_scale2 without bias2", who);
    TCOW_CHECK_ARG(a->K % 64 == 0, "%s: K=%d must be a multiple of 64", who, a->K);
    TCOW_CHECK_ARG(a->ldc % 4 == 0 && a->N % 4 == 0, "%s: N and ldc must be multiples of 4 (N=%d ldc=%ld)", who, a->N, a->ldc);
    TCOW_CHECK_ARG((!a->resid || a->ldr % 4 == 0) && (!a->aux || a->ldaux % 4 == 0), "%s: ldr / ldaux must be multiples of 4", who);
    TCOW_CHECK_ARG(split >= 1 && split <= 16, "%s: split=%d must be 1 .. 16", who, split);
    TCOW_CHECK_ARG(split <= a->K / 64, "%s: split=%d exceeds the K/64 = %d k-slices of K=%d", who, split, a->K / 64, a->K);
    const long need = tcow_gemm_nt_skinny_workspace_bytes(a->M, a->N, split);
    TCOW_CHECK_ARG(need == 0 || ws != nullptr, "%s: workspace is NULL (split=%d needs %ld bytes)", who, split, need);
    TCOW_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (workspace_bytes %ld < %ld)", who, ws_bytes, need);
    TCOW_CHECK_ARG(need == 0 || ((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    return TCOW_OK;
}

// (a wrong dtype is reported before anything else about the arguments, as it always was; a null `a` is check_skinny_args's to refuse)
int tcow_gemm_nt_skinny(void* stream, const tcow_gemm_args* a, int split, void* workspace, long workspace_bytes) {
    TCOW_CHECK_ARG(!a || a->dtype == TCOW_BF16, "tcow_gemm_nt_skinny: dtype %d is not served (the 16-bit mode only; TCOW_F32 and TCOW_F32X3 go to tcow_gemm_nt)", a->dtype);
    if (const int rc = check_skinny_args("tcow_gemm_nt_skinny", a, split, workspace, workspace_bytes)) return rc;
    TCOW_CHECK_ARG(a->lda % 8 == 0 && a->ldw % 8 == 0, "tcow_gemm_nt_skinny: lda/ldw must be multiples of 8 elements");
    return tcow_gemm_nt_skinny_launch_bf16((hipStream_t)stream, a, split, (float*)workspace);
}

// ---- the same for the bf16 x 3 arithmetic on f32 operands (gemm_nt_skinny_x3.hip); exact f32 has no skinny kernel
int tcow_gemm_nt_skinny_x3(void* stream, const tcow_gemm_args* a, int split, void* workspace, long workspace_bytes) {
    TCOW_CHECK_ARG(!a || a->dtype == TCOW_F32X3, "tcow_gemm_nt_skinny_x3: dtype %d is not served (TCOW_F32X3 only; TCOW_BF16 goes to tcow_gemm_nt_skinny, TCOW_F32 to tcow_gemm_nt)", a->dtype);
    if (const int rc = check_skinny_args("tcow_gemm_nt_skinny_x3", a, split, workspace, workspace_bytes)) return rc;
    TCOW_CHECK_ARG(a->lda >= a->K && a->ldw >= a->K && a->lda % 4 == 0 && a->ldw % 4 == 0, "tcow_gemm_nt_skinny_x3: lda/ldw must be multiples of 4 elements and at least K");
    TCOW_CHECK_ARG(a->ldc >= a->N, "tcow_gemm_nt_skinny_x3: ldc=%ld must be at least N=%d", a->ldc, a->N);
    TCOW_CHECK_ARG((((uintptr_t)a->A | (uintptr_t)a->W | (uintptr_t)a->C | (uintptr_t)a->bias | (uintptr_t)a->resid | (uintptr_t)a->aux | (uintptr_t)a->bias2) & 15) == 0,
                   "tcow_gemm_nt_skinny_x3: A, W, C, bias, resid, aux and bias2 must be 16-byte aligned");
    return tcow_gemm_nt_skinny_launch_x3((hipStream_t)stream, a, split, (float*)workspace);
}

// ---- hand-off of a rollover stream pool (stream_requery.hip): logit planes -> 0 / 1 query masks and their pixel counts, all on the device
int tcow_requery_mask(void* stream, int n, long plane, const float* logits, long logits_len, const long* src_off, float threshold, float* mask,
                      const int* dst_rows, int n_dst, int* pixels) {
    TCOW_CHECK_ARG(logits && src_off && mask && dst_rows && pixels, "tcow_requery_mask: null pointer");
    TCOW_CHECK_ARG(n >= 1, "tcow_requery_mask: n=%d must be >= 1", n);
    TCOW_CHECK_ARG(plane >= 1 && plane < (1L << 31), "tcow_requery_mask: plane=%ld must be 1 .. 2^31 - 1", plane);
    TCOW_CHECK_ARG(logits_len >= plane, "tcow_requery_mask: logits_len=%ld holds no plane of %ld elements", logits_len, plane);
    TCOW_CHECK_ARG(n_dst >= 1, "tcow_requery_mask: n_dst=%d must be >= 1", n_dst);
    TCOW_CHECK_ARG(threshold - threshold == 0.0f, "tcow_requery_mask: the threshold must be finite");
    return tcow_launch_requery_mask((hipStream_t)stream, n, plane, logits, logits_len, src_off, threshold, mask, dst_rows, n_dst, pixels);
}

// ---- weight gradients.  Every number below -- kernel, slices, how the bias gradient is produced, workspace offsets -- is the plan's (gemm_tn_plan.h).
long tcow_gemm_tn_workspace_bytes(int M, int N, int K) { return tcow_tn_workspace_total(M, N, K); }

int tcow_gemm_tn(void* stream, int dtype, int M, int N, int K, const void* dY, long ldy, const void* X, long ldx, float* dW, long lddw,
                 float* bias_grad, int accumulate, void* workspace, long workspace_bytes) {
    TCOW_CHECK_ARG(M > 0 && N > 0 && K > 0 && dY && X && dW && workspace, "tcow_gemm_tn: bad arguments");
    const TnPlan pl = tcow_tn_plan(dtype, M, N, K, ldy, ldx, bias_grad != nullptr);
    TCOW_CHECK_ARG(workspace_bytes >= pl.total, "tcow_gemm_tn: workspace too small (%ld < %ld)", workspace_bytes, pl.total);
    TCOW_CHECK_ARG(pl.kernel != TN_KNONE, "tcow_gemm_tn: unknown dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    float* slab = (float*)((char*)workspace + pl.slab_off);
    float* table = (float*)((char*)workspace + pl.table_off);
    int rc = TCOW_OK, nparts = pl.table_rows;
    if (pl.bias == TN_BIAS_PARTIALS) rc = tcow_launch_colsum_partials(st, TCOW_F32, dY, ldy, M, N, table, TN_COLSUM_PARTS, &nparts);
    if (rc) return rc;
    if (dtype == TCOW_BF16) rc = tcow_gemm_tn_bf16(st, pl, M, N, K, (const bf16_t*)dY, ldy, (const bf16_t*)X, ldx, slab, pl.bias == TN_BIAS_FUSED ? table : nullptr);
    else if (dtype == TCOW_F32) rc = tcow_gemm_tn_f32(st, pl, M, N, K, (const float*)dY, ldy, (const float*)X, ldx, slab);
    else rc = tcow_gemm_tn_x3(st, pl, M, N, K, (const float*)dY, ldy, (const float*)X, ldx, slab);
    if (rc) return rc;
    const bool folded = pl.bias == TN_BIAS_FUSED || pl.bias == TN_BIAS_PARTIALS;      // the table's fold rides on the slab fold
    rc = tcow_launch_slab_reduce(st, slab, pl.nz, (long)N * K, N, K, dW, lddw, accumulate, folded ? table : nullptr, nparts, N, bias_grad);
    if (rc || pl.bias != TN_BIAS_COLSUM) return rc;
    return tcow_launch_colsum(st, TCOW_BF16, dY, ldy, M, N, bias_grad, accumulate, table, TN_COLSUM_PARTS);
}

// ---- grouped weight gradients
int tcow_gemm_tn_group_max(void) { return TCOW_TN_GROUP_MAX; }
long tcow_gemm_tn_grouped_workspace_bytes(int dtype, int n, const tcow_tn_problem* pr) { return n <= 0 || pr == nullptr ? 0 : tcow_tn_group_plan(dtype, n, pr).total; }

int tcow_gemm_tn_grouped(void* stream, int dtype, int n, const tcow_tn_problem* pr, void* workspace, long workspace_bytes) {
    TCOW_CHECK_ARG(n > 0 && pr && workspace, "tcow_gemm_tn_grouped: bad arguments");
    const TnGroupPlan pl = tcow_tn_group_plan(dtype, n, pr);
    TCOW_CHECK_ARG(workspace_bytes >= pl.total, "tcow_gemm_tn_grouped: workspace too small (%ld < %ld)", workspace_bytes, pl.total);
    for (int i = 0; i < n; ++i)
        TCOW_CHECK_ARG(pr[i].M > 0 && pr[i].N > 0 && pr[i].K > 0 && pr[i].dY && pr[i].X && pr[i].dW, "tcow_gemm_tn_grouped: bad problem %d", i);
    if (!pl.grouped) {
        for (int i = 0; i < n; ++i) {
            const int rc = tcow_gemm_tn(stream, dtype, pr[i].M, pr[i].N, pr[i].K, pr[i].dY, pr[i].ldy, pr[i].X, pr[i].ldx, pr[i].dW, pr[i].lddw, pr[i].bias_grad,
                                        pr[i].accumulate, workspace, workspace_bytes);
            if (rc) return rc;
        }
        return TCOW_OK;
    }
    constexpr int G = TCOW_TN_GROUP_MAX;          // (a plan that groups has n <= G)
    float* slabs[G]; float* parts[G];
    bool vec = true;
    for (int i = 0; i < n; ++i) {
        slabs[i] = pl.p[i].in_place ? pr[i].dW : (float*)((char*)workspace + pl.p[i].slab_off);
        parts[i] = pr[i].bias_grad ? (float*)((char*)workspace + pl.p[i].table_off) : nullptr;
        vec = vec && tcow_fold_vec_ok(slabs[i], (long)pr[i].N * pr[i].K, pr[i].K, pr[i].dW, pr[i].lddw);
    }
    int rc = tcow_gemm_tn_bf16_group((hipStream_t)stream, pl, n, pr, slabs, parts);
    if (rc) return rc;
    if (vec) {       // one fold launch for the whole group
        long rows[G], cols[G], ldo[G]; int acc[G], nparts[G]; float* outs[G]; float* bouts[G];
        for (int i = 0; i < n; ++i) {
            rows[i] = pr[i].N; cols[i] = pr[i].K; ldo[i] = pr[i].lddw; acc[i] = pr[i].accumulate; outs[i] = pr[i].dW; bouts[i] = pr[i].bias_grad; nparts[i] = pl.p[i].table_rows;
        }
        return tcow_launch_slab_reduce_group((hipStream_t)stream, n, slabs, pl.nz, rows, cols, outs, ldo, acc, parts, nparts, bouts);
    }
    for (int i = 0; i < n; ++i) {
        rc = tcow_launch_slab_reduce((hipStream_t)stream, slabs[i], pl.nz, (long)pr[i].N * pr[i].K, pr[i].N, pr[i].K, pr[i].dW, pr[i].lddw, pr[i].accumulate,
                                     parts[i], pl.p[i].table_rows, pr[i].N, pr[i].bias_grad);
        if (rc) return rc;
    }
    return TCOW_OK;
}

}  // extern "C"
