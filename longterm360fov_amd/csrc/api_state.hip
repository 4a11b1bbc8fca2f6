// Process-wide host state of libfov360_hip.so: the error string, the launch check, the cached environment knobs, the epoch
// accounting and prepack marks per workspace, and the entry points that manage a workspace, a stream or the library itself.
#include <stdarg.h>
#include <stdio.h>

#include <mutex>
#include <unordered_map>

#include "fov_common.h"
#include "xch_common.h"

namespace fov {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

bool operand_fits_31bit(const char* what, int B, long ldb, const void* x2, long ldb2, long weight_bytes, long tiles) {
    const long lim = 1L << 31;
    if ((long)B * ldb * 4 < lim && (!x2 || (long)B * ldb2 * 4 < lim) && weight_bytes < lim && tiles < lim) return true;
    set_error("%s: operand larger than 2 GiB", what);
    return false;
}

int launch_check(const char* what) {
    if (env_knobs().dbg_trace) fprintf(stderr, "[fov trace] launched: %s\n", what);   // FOV_DBG_TRACE=1 (with HIP_LAUNCH_BLOCKING=1: the last line names the launch BEFORE a faulting one)
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", what, hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    return FOV_OK;
}


int check_ws(void* ws, size_t have, size_t need) {
    if (need == 0) return FOV_OK;
    if (!ws || have < need) {
        set_error("workspace too small: need %zu bytes, have %zu", need, ws ? have : (size_t)0);
        return FOV_ERR_WORKSPACE;
    }
    if (((uintptr_t)ws & 15) != 0) { set_error("workspace must be 16-byte aligned"); return FOV_ERR_WORKSPACE; }
    return FOV_OK;
}

// ---- cached environment knobs ----
static EnvKnobs g_env;
static std::once_flag g_env_once;
static int env_flag(const char* name) { const char* e = getenv(name); return (e && e[0] == '1') ? 1 : 0; }
void env_reload() {
    g_env.force_safe_exchange = env_flag("FOV_FORCE_SAFE_EXCHANGE");
    g_env.two_launches = getenv("FOV_TWO_LAUNCHES") ? 1 : 0;
    const char* lim = getenv("FOV_DBG_RESIDENT_LIMIT");
    g_env.resident_limit = lim ? atoi(lim) : 0;
    g_env.no_cell_patch = env_flag("FOV_NO_CELL_PATCH");
    g_env.no_conv_patch = env_flag("FOV_NO_CONV_PATCH");
    g_env.no_wide16 = env_flag("FOV_NO_WIDE16");
    g_env.no_xcd_pad = getenv("FOV_NO_XCD_PAD") ? 1 : 0;
    { const char* pm = getenv("FOV_XCD_PAD_MAX"); g_env.xcd_pad_max = pm ? atoi(pm) : 16; }
    g_env.no_bwd16_narrow = getenv("FOV_NO_BWD16_NARROW") ? 1 : 0;
    { const char* bg = getenv("FOV_BWD16_GROUPS"); g_env.bwd16_groups32 = (bg && atoi(bg) == 32) ? 1 : 0; }
    g_env.no_stack2 = env_flag("FOV_NO_STACK2");
    g_env.no_stacked_decode = env_flag("FOV_NO_STACKED_DECODE");
    g_env.no_selffed_fused = env_flag("FOV_NO_SELFFED_FUSED");
    g_env.no_selffed2_fused = env_flag("FOV_NO_SELFFED2_FUSED");
    g_env.no_stacked_train = env_flag("FOV_NO_STACKED_TRAIN");
    g_env.bwd_stepped = getenv("FOV_BWD_STEPPED") ? 1 : 0;
    g_env.no_wgrad_fusion = getenv("FOV_NO_WGRAD_FUSION") ? 1 : 0;
    g_env.no_dx_fusion = getenv("FOV_NO_DX_FUSION") ? 1 : 0;
    g_env.bwd_groups4 = getenv("FOV_BWD_GROUPS4") ? 1 : 0;
    g_env.gemm_bf16_noremap = getenv("FOV_GEMM_BF16_NOREMAP") ? 1 : 0;
    g_env.gemm_bf16_shallow = getenv("FOV_GEMM_BF16_SHALLOW") ? 1 : 0;
    g_env.no_wgrad_group = getenv("FOV_NO_WGRAD_GROUP") ? 1 : 0;
    g_env.no_wgrad_lines = getenv("FOV_NO_WGRAD_LINES") ? 1 : 0;
    g_env.no_wgrad_bf16_tiles = env_flag("FOV_NO_WGRAD_BF16_TILES");
    g_env.no_wide16_trio = getenv("FOV_NO_WIDE16_TRIO") ? 1 : 0;
    g_env.dbg_trace = getenv("FOV_DBG_TRACE") ? 1 : 0;
    const char* gb = getenv("FOV_GEMM_BF16_SPLIT");
    g_env.gemm_bf16_split = gb ? atoi(gb) : 0;
    const char* gv = getenv("FOV_GEMM_VARIANT");
    g_env.gemm_variant = gv ? atoi(gv) : 0;
    const char* gs = getenv("FOV_GEMM_SPLIT");
    g_env.gemm_split = gs ? atoi(gs) : 0;
}
const EnvKnobs& env_knobs() {
    std::call_once(g_env_once, env_reload);
    return g_env;
}

// ---- host-side epoch accounting per workspace ----
struct XchState { unsigned long long epoch; int force_safe; };
static std::unordered_map<void*, XchState> g_xch;
static std::mutex g_xch_mu;
int xch_account(void* workspace, long span, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_xch_mu);
    XchState& st = g_xch[workspace];
    st.epoch += (unsigned long long)(span > 0 ? span : 0) + 2ull;
    if (st.epoch > 0x70000000ull) {
        // every launch on this workspace passes here, so the device-side base is at most st.epoch: re-zero the header and the
        // granule area in front of this launch (stream-ordered; launches on one workspace are serialised by contract)
        // ... all of it but the sticky timeout word (header word 0): a give-up since the last fov_check_status must stay visible
        // to the guarded optimizer and to the next check
        static_assert(ST_TIMEOUT == 0, "the re-zero below skips header word 0");
        hipError_t e = hipMemsetAsync((char*)workspace + sizeof(unsigned), 0, kStatusBytes + kXchBytes - sizeof(unsigned), stream);
        if (e == hipSuccess && st.force_safe)
            e = hipMemsetD32Async((hipDeviceptr_t)((unsigned*)workspace + ST_FORCE_SAFE), 1, 1, stream);
        if (e != hipSuccess) { set_error("epoch re-zero: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
        st.epoch = (unsigned long long)(span > 0 ? span : 0) + 2ull;
    }
    return FOV_OK;
}
void xch_forget(void* workspace) {
    std::lock_guard<std::mutex> lock(g_xch_mu);
    XchState& st = g_xch[workspace];
    st.epoch = 0;
}
void xch_note_force_safe(void* workspace, int on) {
    std::lock_guard<std::mutex> lock(g_xch_mu);
    g_xch[workspace].force_safe = on ? 1 : 0;
}
// test hook: pretend `epoch` epochs have been consumed on this workspace (the device header is set to match by the caller)
void xch_set_epoch_for_test(void* workspace, unsigned long long epoch) {
    std::lock_guard<std::mutex> lock(g_xch_mu);
    g_xch[workspace].epoch = epoch;
}

static std::unordered_map<void*, const float*> g_prepacked;
static std::mutex g_prepacked_mu;
void prepack_mark(void* workspace, const float* K2) {
    std::lock_guard<std::mutex> lock(g_prepacked_mu);
    g_prepacked[workspace] = K2;
}
bool prepack_consume(void* workspace, const float* K2) {
    std::lock_guard<std::mutex> lock(g_prepacked_mu);
    auto it = g_prepacked.find(workspace);
    if (it == g_prepacked.end()) return false;
    const bool hit = it->second == K2;
    g_prepacked.erase(it);
    return hit;
}
// the workspace was zero-filled (fov_workspace_init, the reset of fov_check_status): a packed copy marked earlier is gone
void prepack_forget(void* workspace) {
    std::lock_guard<std::mutex> lock(g_prepacked_mu);
    g_prepacked.erase(workspace);
}

// a workspace at least as large as its status header, or the error "<who>: invalid workspace"
static bool has_header(const char* who, const void* workspace, size_t workspace_bytes) {
    if (workspace && workspace_bytes >= kStatusBytes) return true;
    set_error("%s: invalid workspace", who);
    return false;
}

}  // namespace fov

using namespace fov;

extern "C" {

const char* fov_last_error(void) { return g_err; }

void fov_reload_env(void) { env_reload(); }

int64_t fov_debug_generic_launches(void) { return (int64_t)generic_launch_count(); }

int fov_debug_set_epoch(void* workspace, size_t workspace_bytes, unsigned epoch, fov_stream_t stream) {
    if (!has_header("fov_debug_set_epoch", workspace, workspace_bytes)) return FOV_ERR_INVALID;
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)((unsigned*)workspace + ST_EPOCH), (int)epoch, 1, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("fov_debug_set_epoch: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    xch_set_epoch_for_test(workspace, epoch);
    return FOV_OK;
}
int fov_version(void) { return 100; }

int fov_stream_create(int priority, fov_stream_t* stream) {
    if (!stream) { set_error("fov_stream_create: stream is NULL"); return FOV_ERR_INVALID; }
    int least = 0, greatest = 0;     // numerically: least = lowest priority (largest value), greatest = highest (smallest value)
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) { set_error("hipDeviceGetStreamPriorityRange: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    int p = priority > 0 ? least : (priority < 0 ? greatest : 0);
    if (p > least) p = least;
    if (p < greatest) p = greatest;
    hipStream_t s = nullptr;
    e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, p);
    if (e != hipSuccess) { set_error("hipStreamCreateWithPriority(%d): %s", p, hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    *stream = (fov_stream_t)s;
    return FOV_OK;
}

int fov_stream_destroy(fov_stream_t stream) {
    if (!stream) return FOV_OK;
    hipError_t e = hipStreamDestroy((hipStream_t)stream);
    if (e != hipSuccess) { set_error("hipStreamDestroy: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    return FOV_OK;
}

int fov_workspace_init(void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (!has_header("fov_workspace_init", workspace, workspace_bytes)) return FOV_ERR_INVALID;
    hipError_t e = hipMemsetAsync(workspace, 0, workspace_bytes, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("fov_workspace_init: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    xch_forget(workspace);
    prepack_forget(workspace);
    xch_note_force_safe(workspace, 0);
    return FOV_OK;
}

int fov_workspace_force_safe(void* workspace, size_t workspace_bytes, int on, fov_stream_t stream) {
    if (!has_header("fov_workspace_force_safe", workspace, workspace_bytes)) return FOV_ERR_INVALID;
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)((unsigned*)workspace + ST_FORCE_SAFE), on ? 1 : 0, 1, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("fov_workspace_force_safe: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    xch_note_force_safe(workspace, on);
    return FOV_OK;
}

int fov_check_status(void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (!has_header("fov_check_status", workspace, workspace_bytes)) return FOV_ERR_INVALID;
    unsigned st[64] = {0};
    hipError_t e = hipMemcpyAsync(st, workspace, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { set_error("fov_check_status: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    // The timeout word is sticky (no launch clears it, later launches skip their bodies): reading it here is what
    // clears it.  After a give-up, or long before the 32-bit epoch tags could wrap, the whole workspace is re-zeroed;
    // the stream is idle at this point.
    if (st[ST_TIMEOUT] != 0 || st[ST_EPOCH] > 0x7fff0000u) {
        e = hipMemsetAsync(workspace, 0, workspace_bytes, (hipStream_t)stream);
        if (e == hipSuccess && st[ST_FORCE_SAFE] != 0)   // the A/B switch is the caller's setting, not launch state: it survives
            e = hipMemsetD32Async((hipDeviceptr_t)((unsigned*)workspace + ST_FORCE_SAFE), 1, 1, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) { set_error("fov_check_status: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
        xch_forget(workspace);
        prepack_forget(workspace);
    }
    if (st[ST_TIMEOUT] != 0) {
        set_error("a bounded in-kernel wait gave up (exchange launches on this workspace so far: %u); results since the last check are invalid",
                  st[ST_LAUNCHES]);
        return FOV_ERR_TIMEOUT;
    }
    return FOV_OK;
}

int fov_exchange_mode(const void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (!has_header("fov_exchange_mode", workspace, workspace_bytes)) return FOV_ERR_INVALID;
    unsigned st[64] = {0};
    hipError_t e = hipMemcpyAsync(st, workspace, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { set_error("fov_exchange_mode: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    if (st[ST_LAUNCHES] == 0) return 1;
    return st[ST_SAFE0 + ((st[ST_LAUNCHES] - 1u) & 1u)] == 0 ? 1 : 2;   // of the last exchange launch
}

}  // extern "C"
