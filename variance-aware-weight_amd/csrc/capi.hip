// Error plumbing and version of libvaw_hip.so (the kernels' extern "C" entry points live next to them).
#include <stdarg.h>
#include <stdio.h>

#include "common.h"

static thread_local char g_err[512] = "";

void vaw_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int vaw_version(void) { return 100; }   // 0.1.0
extern "C" const char* vaw_last_error_string(void) { return g_err; }

// Activation workspace of the DiT engine: every buffer dit.py's _Workspace allocates, in bytes (host arithmetic only).  The lists
// below follow _Workspace.__init__ line by line; _Workspace checks its allocations against `total`.
extern "C" int vaw_dit_ws_plan(int dtype, int B, int T, int D, int Dm, int depth, int heads, int Kp, int No, int defer_wgrad,
                               int checkpoint, vaw_dit_ws_plan_t* out) {
    VAW_CHECK_ARG(out != nullptr, "dit_ws_plan: out is NULL");
    VAW_CHECK_ARG(dtype == VAW_F32 || dtype == VAW_BF16, "dit_ws_plan: the act dtype is VAW_F32 or VAW_BF16, got %d", dtype);
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && Dm > 0 && depth > 0 && heads > 0 && Kp > 0 && No > 0,
                  "dit_ws_plan: sizes must be positive (B %d T %d D %d Dm %d depth %d heads %d Kp %d No %d)", B, T, D, Dm, depth, heads, Kp, No);
    VAW_CHECK_ARG(D % heads == 0, "dit_ws_plan: D %d is not a multiple of heads %d", D, heads);
    VAW_CHECK_ARG((defer_wgrad == 0 || defer_wgrad == 1) && (checkpoint == 0 || checkpoint == 1),
                  "dit_ws_plan: defer_wgrad %d and checkpoint %d are flags (0 / 1)", defer_wgrad, checkpoint);
    const int64_t es = dtype == VAW_BF16 ? 2 : 4, f4 = 4;
    const int64_t M = (int64_t)B * T, d = D, dm = Dm, Bq = B;
    const int64_t Bk = dtype == VAW_BF16 ? (Bq + 63) / 64 * 64 : Bq;          // zero rows up to the MFMA K tile (see _Workspace)
    const int64_t mod_cols = (6 * (int64_t)depth + 2) * d;
    const int own_dy = defer_wgrad && dtype == VAW_BF16 && M % 64 == 0;
    const int64_t lse = Bq * heads * T * f4;
    // one block record
    const int64_t rec_rows = M * (8 * d + 2 * dm) * es;                      // xm qkv(3) ao y1 xm2 y2 | hpre a
    const int64_t rec_stats = lse + 4 * M * f4;                              // lse | mean1 rstd1 mean2 rstd2
    const int64_t rec_dy = own_dy ? M * (5 * d + dm) * es : 0;               // dy2 dy1 dqkv(3) | dDm
    const int64_t row = M * d * f4;                                          // one f32 row of the residual stream
    // partial column sums of one set: cp_fc2, cp_proj [B][D]; cp_fc1 [ceil(M / 64)][Dm]; cp_qkv [max(B, M / 64)][3 D]
    const int64_t qkv_rows = Bq > M / 64 ? Bq : M / 64;
    const int64_t cp_set = (2 * Bq * d + (M + 63) / 64 * dm + qkv_rows * 3 * d) * f4;
    vaw_dit_ws_plan_t p;
    p.records = checkpoint ? 1 : depth;
    p.colsum_sets = checkpoint ? 1 : depth;
    p.own_dy = own_dy;
    p.Bk = (int)Bk;
    if (checkpoint) {
        p.block_bytes = row;
        p.block_stat_bytes = 0;
        p.shared_bytes = rec_rows + rec_stats + rec_dy + 2 * row;            // + xres_mid + fc2's scratch row
    } else {
        p.block_bytes = rec_rows + rec_dy + 2 * row;
        p.block_stat_bytes = rec_stats;
        p.shared_bytes = 0;
    }
    p.colsum_bytes = p.colsum_sets * cp_set;
    // backward scratch: dotok dD dao | dDm dqkv dyb | dres dxp | delta | dmod dmod_a | dcs dc dh1s dh1 | dc_a dh1_a
    p.scratch_bytes = M * (No + 2 * d) * es + (checkpoint && own_dy ? 0 : M * (dm + 4 * d) * es) + row + M * Kp * f4 + lse +
                      Bq * mod_cols * f4 + Bk * mod_cols * es + 4 * Bq * d * f4 + 2 * Bk * d * es;
    // forward outside the blocks: tfreq h1s cs | h1 temb c | mod | xp | xf | meanf rstdf | otok | the last residual-stream row
    p.cond_bytes = Bk * (256 + 2 * d) * es + 3 * Bq * d * f4 + Bq * mod_cols * f4 + M * Kp * es + M * d * es + 2 * M * f4 +
                   M * No * f4 + row;
    p.total = depth * (p.block_bytes + p.block_stat_bytes) + p.shared_bytes + p.colsum_bytes + p.scratch_bytes + p.cond_bytes;
    *out = p;
    return VAW_OK;
}

// Measurement aid (tools/contention_bench.py): n_wgs workgroups that each take a whole CU (160 KiB of LDS) and idle there for
// `microseconds` -- a stand-in for a collective kernel running on another stream beside the compute kernels.
__global__ void __launch_bounds__(64) cu_hog_kernel(uint64_t ticks) {
    extern __shared__ char hog_lds[];
    if (threadIdx.x == 0) hog_lds[0] = 1;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();       // 100 MHz
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
extern "C" int vaw_debug_cu_hog(int n_wgs, int microseconds, vaw_stream stream) {
    VAW_CHECK_ARG(n_wgs > 0 && n_wgs <= 256 && microseconds > 0 && microseconds <= 2000000, "cu_hog: arguments");
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)cu_hog_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; }
    cu_hog_kernel<<<n_wgs, 64, 160 * 1024, (hipStream_t)stream>>>((uint64_t)microseconds * 100);
    VAW_CHECK_LAUNCH("cu_hog");
    return VAW_OK;
}

// Uploads of descriptor tables (vaw_wgrad_grouped, vaw_reduce_rows_batched, vaw_fp8_quantize_delayed_batched).  The callers build the
// table in a reused pageable array, and an asynchronous copy from pageable memory is only guaranteed to have been STAGED when the
// call returns for small sizes -- a later call that rewrites the array could corrupt a table in flight.  The table is therefore
// copied into a pinned buffer and the asynchronous copy reads from there: no host synchronisation.
// Groups are built again and again over a long run (row counts that alternate, activation addresses that move), so the pinned
// buffers are recycled: a pool of {pointer, size class, device, event}.  Size classes are powers of two from 4 KiB and a buffer serves only
// its own class, so a fixed sequence of uploads needs a fixed set of buffers.  An upload takes a buffer of its class whose event has
// completed (hipEventQuery: never a host wait), allocates one if none has, and records the buffer's event behind its copy.
// Stream capture: the copy itself is a legal node, but a replay reads the pinned buffer AGAIN, so an upload made while `s` is
// capturing gets a buffer of its own that stays out of the pool for the life of the process.  Allocating it is a different matter:
// hipHostMalloc is one of the calls a global-mode capture (what torch.cuda.graph begins) refuses, and it invalidates that capture.
// So a group has to make its first launch outside such a capture; unet.py does not defer weight gradients under capture for
// this reason.
#include <mutex>
#include <string.h>
#include <vector>
namespace {
struct TableBuf { void* p; size_t cls; int device; hipEvent_t done; };      // (an event records only on streams of its own device)
std::mutex g_tab_mu;
std::vector<TableBuf> g_tab_pool;
int64_t g_tab_buffers = 0, g_tab_bytes = 0, g_tab_captured = 0;      // all pinned buffers ever made | their bytes | those a capture holds

hipError_t upload_table_locked(void* dev, const void* host, size_t bytes, hipStream_t s) {
    size_t cls = 4096;
    while (cls < bytes) cls <<= 1;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t rc = hipStreamIsCapturing(s, &cap);
    if (rc != hipSuccess) return rc;
    const bool capturing = cap != hipStreamCaptureStatusNone;
    int device = 0;
    if ((rc = hipGetDevice(&device)) != hipSuccess) return rc;
    TableBuf* b = nullptr;
    if (!capturing)
        for (TableBuf& t : g_tab_pool)
            if (t.cls == cls && t.device == device && hipEventQuery(t.done) == hipSuccess) { b = &t; break; }
    TableBuf made{nullptr, cls, device, nullptr};
    if (!b) {
        if ((rc = hipHostMalloc(&made.p, cls, hipHostMallocDefault)) != hipSuccess) return rc;
        if (!capturing && (rc = hipEventCreateWithFlags(&made.done, hipEventDisableTiming)) != hipSuccess) {
            (void)hipHostFree(made.p);
            return rc;
        }
        g_tab_buffers += 1;
        g_tab_bytes += (int64_t)cls;
        if (capturing) g_tab_captured += 1;
        else { g_tab_pool.push_back(made); b = &g_tab_pool.back(); }
    }
    void* pinned = b ? b->p : made.p;
    memcpy(pinned, host, bytes);
    if ((rc = hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return rc;
    return b ? hipEventRecord(b->done, s) : hipSuccess;
}
}  // namespace

int vaw_upload_table(const char* who, int upload, void* dev, const void* host, size_t bytes, hipStream_t s) {
    if (!upload) return VAW_OK;
    std::lock_guard<std::mutex> g(g_tab_mu);       // held up to the event record: nobody else may take the buffer before
    const hipError_t rc = upload_table_locked(dev, host, bytes, s);
    VAW_CHECK_ARG(rc == hipSuccess, "%s: descriptor upload failed: %s", who, hipGetErrorString(rc));
    return VAW_OK;
}

extern "C" void vaw_debug_upload_table_stats(int64_t* buffers, int64_t* bytes, int64_t* captured) {
    std::lock_guard<std::mutex> g(g_tab_mu);
    if (buffers) *buffers = g_tab_buffers;
    if (bytes) *bytes = g_tab_bytes;
    if (captured) *captured = g_tab_captured;
}
