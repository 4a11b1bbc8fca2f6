// extern "C" entry points of the LSTM layers, the seq2seq calls, the two-layer launches and the fused mixing decoder, forward
// and backward, with the one place that decides which forward kernel a call reaches and how much workspace that kernel needs.
#include "fov_common.h"
#include "xch_common.h"
#include "bf16_common.h"

namespace fov {

static bool want_cluster(int impl, int F, int H, int F_dec, bool decode) {
    if (impl == FOV_IMPL_GENERIC) return false;
    // impl = auto also needs one whole group co-resident (device_cu_count honours FOV_DBG_RESIDENT_LIMIT): otherwise generic
    const bool ok = cluster_shape_ok(F, H) && (!decode || (F_dec >= 1 && F_dec <= 8)) && device_cu_count() >= H / 64;
    return impl == FOV_IMPL_CLUSTER ? true : ok;
}

// The persistent kernels tag every exchange step with a 32-bit epoch and count a launch's span of them in an int: steps times
// the tile rounds a group may make (at most one per 8-row tile) must stay far below 2^31.  Decided here, as arithmetic, for
// every LSTM entry point alike - whichever kernel the call would reach.
static bool steps_ok_quiet(long steps, int B) { return (steps + 2) * (((long)B + 7) / 8 > 0 ? ((long)B + 7) / 8 : 1) <= (1L << 30); }
static bool steps_ok(const char* who, long steps, int B) {
    if (steps_ok_quiet(steps, B)) return true;
    set_error("%s: (steps + 2) * ceil(B / 8) exceeds 2^30 (steps = %ld, B = %d)", who, steps, B);
    return false;
}

// one layer's parameters (phase 1 of LstmParams) on its workspace
static LstmParams layer_params(const float* x, const float* K, const float* R, const float* b, const float* h0, const float* c0,
                               float* hs, float* hT, float* cT, float* reserve, int B, int T, int F, int H, int act, void* workspace) {
    LstmParams p = {};
    p.x = x; p.K = K; p.R = R; p.b = b; p.h0 = h0; p.c0 = c0; p.hs = hs; p.hT = hT; p.cT = cT; p.reserve = reserve;
    p.B = B; p.T = T; p.F = F; p.H = H; p.act = act;
    bind_workspace(p, workspace);
    return p;
}

// Forward plans: which kernel a call reaches and the workspace that kernel needs, decided in one place.  The size functions
// answer from the plan, the entry points check their workspace against it and switch on it.
enum class FwdKernel { Wide16, Wide512, Wide, Cluster, Stepwise, Generic };
struct FwdPlan {
    FwdKernel kernel;
    size_t need;      // workspace bytes of that kernel
    bool project_x;   // Wide512 with F > 96: x.K over all steps first (one GEMM into the workspace), the kernel adds it per step
};
// scratch of that GEMM, behind the projection (B,T,4H) itself
static constexpr size_t kWide512ScratchFloats = ((size_t)1 << 20) + 64;

// One layer forward.  x_aligned16: the forms that stage a wide x with 16-byte loads take an aligned x only.  zx_given: the
// caller supplies x.K (F = 1), which the 16-workgroup width-512 form, the cluster and the generic kernel take.
// impl = cluster on a shape the cluster kernel does not have still plans Cluster: launch_cluster refuses it with its message.
static FwdPlan plan_lstm_fwd(int B, int T, int F, int H, int impl, bool x_aligned16, bool zx_given) {
    const bool any = impl != FOV_IMPL_GENERIC, aut = impl == FOV_IMPL_AUTO && !zx_given;
    const bool wide16_ok = !zx_given && !env_knobs().no_wide16 && wide16_shape(B, F, H) && (F <= 96 || x_aligned16);
    // header + granule area (+ the fused decode's state) of every persistent kernel; an empty batch launches nothing
    const size_t granules = B > 0 ? cluster_workspace_bytes(B, H) : kStatusBytes;
    // width 512 (mycode/lstm.py's LSTMCell(400), zero-padded by the caller)
    if (any && wide512_shape_ok(F, H, zx_given || F > 96)) {
        // few tiles: 32 workgroups per tile, K and R both in registers (lstm_wide16.hip)
        if (wide16_ok) return {FwdKernel::Wide16, granules, false};
        // R register-resident over 16 workgroups per tile (lstm_wide.hip); an input wider than 96 is projected first
        const bool project_x = !zx_given && F > 96;
        const size_t zx_bytes = project_x && B > 0 ? sizeof(float) * ((size_t)B * T * 4 * H + kWide512ScratchFloats) : 0;
        return {FwdKernel::Wide512, granules + zx_bytes, project_x};
    }
    // The wide16 and the narrow-wide form below take no empty sequence: T = 0 goes on to a kernel that passes the state through.
    // Its workspace keeps the size of the T > 0 choice (`floor`), as fov_lstm_seq_workspace_bytes has always answered.
    size_t floor = kStatusBytes;
    // few tiles at width 128 / 256: H / 16 workgroups per tile (lstm_wide16.hip) - the latency regime of model.fit at batch 32
    if (aut && H != 512 && wide16_ok) {
        if (T > 0) return {FwdKernel::Wide16, granules, false};
        floor = granules;
    }
    // wide inputs (a stacked layer over a 256-wide sequence): K and R both register-resident (lstm_wide.hip)
    if (any && wide_shape_ok(F, H) && x_aligned16) return {FwdKernel::Wide, granules, false};
    // narrow inputs, at most 32 tiles: groups of eight workgroups fill the chip where lstm_cluster's groups of four leave half idle
    if (aut && wide_narrow_preferred(B, F, H)) {
        if (T > 0) return {FwdKernel::Wide, granules, false};
        floor = granules;
    }
    if (want_cluster(impl, F, H, 0, false)) return {FwdKernel::Cluster, cluster_shape_ok(F, H) ? granules : kStatusBytes, false};
    // widths above the persistent kernels': step-wise on the matrix-core GEMM instead of the VALU kernel
    if (aut && stepwise_preferred(B, F, H))
        return {FwdKernel::Stepwise, kStatusBytes + sizeof(float) * stepwise_workspace_floats(B, T, H), false};
    return {FwdKernel::Generic, floor, false};
}

// p: the layer's parameters with the workspace bound; p.x / p.K as the caller gave them
static int launch_lstm_fwd(const FwdPlan& plan, LstmParams& p, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (int rc = check_ws(workspace, workspace_bytes, plan.need)) return rc;
    switch (plan.kernel) {
        case FwdKernel::Wide16: return launch_wide16(p, s);
        case FwdKernel::Wide512:
            if (plan.project_x) {
                float* zx = (float*)((char*)workspace + cluster_workspace_bytes(p.B, p.H));
                prepack_forget(workspace);   // the projection lies where mix_decoder_prepack leaves its packed dec2_K
                if (p.B > 0 && p.T > 0)
                    if (int rc = matmul_f32(p.x, p.K, zx, p.B * p.T, p.F, 4 * p.H, zx + (size_t)p.B * p.T * 4 * p.H, kWide512ScratchFloats, s))
                        return rc;
                p.zx = zx;
            }
            return launch_wide(p, s);
        case FwdKernel::Wide: return launch_wide(p, s);
        case FwdKernel::Cluster: return launch_cluster(p, false, s);
        case FwdKernel::Stepwise:
            prepack_forget(workspace);   // (its buffers start at the header's end and may reach behind the granule area)
            return launch_stepwise(p, (float*)((char*)workspace + kStatusBytes), (workspace_bytes - kStatusBytes) / sizeof(float), s);
        case FwdKernel::Generic: break;
    }
    return launch_generic(p, false, s);
}

// The fused encoder + free-running decoder, and the decoder alone from a given state (F_enc = 1, no encoder steps).  Cluster
// covers the fused and the two-launch form (launch_cluster chooses) and, for the decoder alone, launch_cluster_decoder.
enum class DecodeKernel { Wide16, Cluster, Generic };
struct DecodePlan { DecodeKernel kernel; size_t need; };
static DecodePlan plan_decode(int B, int T_out, int F_enc, int F_dec, int H, int impl) {
    if (!want_cluster(impl, F_enc, H, F_dec, true)) return {DecodeKernel::Generic, kStatusBytes};
    // (impl = cluster on a shape the cluster kernel does not have: launch_cluster refuses it, the header is enough)
    const size_t need = B > 0 && cluster_shape_ok(F_enc, H) ? cluster_workspace_bytes(B, H) : kStatusBytes;
    // small batches (at most eight tiles): the tile spread over H / 16 workgroups instead of H / 64 (lstm_wide16.hip)
    if (impl == FOV_IMPL_AUTO && wide16_s2s_shape(B, F_enc, F_dec, H) && T_out > 0) return {DecodeKernel::Wide16, need};
    return {DecodeKernel::Cluster, need};
}

// the decoder half of a decode call's parameters
static void bind_decoder(LstmParams& p, const float* dec_in0, const float* dec_K, const float* dec_R, const float* dec_b,
                         const float* dense_W, const float* dense_b, float* out, float* hT, float* cT, int B, int T_out, int F_dec,
                         int H, int act, void* workspace) {
    p.dec_in0 = dec_in0; p.dK = dec_K; p.dR = dec_R; p.db = dec_b; p.dW = dense_W; p.dbias = dense_b; p.out = out;
    p.hT = hT; p.cT = cT;
    p.B = B; p.H = H; p.T_out = T_out; p.F_dec = F_dec; p.act = act;
    bind_workspace(p, workspace);
}

// workspace of the teacher-forced graph: [0, state) the two layers' own, [state, hs) the encoder's final (h, c), [hs, total) the
// decoder's hidden sequence
struct TfCarve { size_t state, hs, total; };
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
static TfCarve tf_carve(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int impl) {
    const size_t a = fov_lstm_seq_workspace_bytes(B, T_in, F_enc, H, impl), c = fov_lstm_seq_workspace_bytes(B, T_out, F_dec, H, impl);
    TfCarve v;
    v.state = align256(a > c ? a : c);
    v.hs = v.state + align256((size_t)2 * B * H * sizeof(float));
    v.total = v.hs + align256((size_t)B * T_out * H * sizeof(float));
    return v;
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_cluster_supported(int F, int H) { return cluster_shape_ok(F, H) ? 1 : 0; }

// the caller does not know x at query time: whichever form an aligned or an unaligned x reaches must fit
size_t fov_lstm_seq_workspace_bytes(int B, int T, int F, int H, int impl) {
    const size_t a = plan_lstm_fwd(B, T, F, H, impl, true, false).need, u = plan_lstm_fwd(B, T, F, H, impl, false, false).need;
    return a > u ? a : u;
}

static int lstm_seq_fwd_impl(const float* x, const float* K, const float* R, const float* b, const float* h0,
                             const float* c0, float* hs, float* hT, float* cT, float* reserve, int B, int T, int F,
                             int H, int act, int impl, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || F <= 0 || H <= 0 || !K || !R || !b || (B > 0 && T > 0 && !x) || !valid_act(act) ||
        !valid_impl(impl)) {
        set_error("fov_lstm_seq_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!steps_ok("fov_lstm_seq_fwd", T, B)) return FOV_ERR_UNSUPPORTED;
    LstmParams p = layer_params(x, K, R, b, h0, c0, hs, hT, cT, reserve, B, T, F, H, act, workspace);
    return launch_lstm_fwd(plan_lstm_fwd(B, T, F, H, impl, (((uintptr_t)x) & 15) == 0, false), p, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

int fov_lstm_seq_fwd(const float* x, const float* K, const float* R, const float* b, const float* h0,
                     const float* c0, float* hs, float* hT, float* cT, int B, int T, int F, int H, int act,
                     int impl, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    return lstm_seq_fwd_impl(x, K, R, b, h0, c0, hs, hT, cT, nullptr, B, T, F, H, act, impl, workspace, workspace_bytes,
                             stream);
}

int fov_lstm_seq_fwd_train(const float* x, const float* K, const float* R, const float* b, const float* h0,
                           const float* c0, float* hs, float* hT, float* cT, float* reserve, int B, int T, int F,
                           int H, int act, int impl, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (!reserve && B > 0 && T > 0) { set_error("fov_lstm_seq_fwd_train: reserve is NULL"); return FOV_ERR_INVALID; }
    return lstm_seq_fwd_impl(x, K, R, b, h0, c0, hs, hT, cT, reserve, B, T, F, H, act, impl, workspace, workspace_bytes,
                             stream);
}

int fov_lstm_seq_fwd_bf16(const float* x, const float* K, const float* R, const float* b, const float* h0, const float* c0,
                          float* hs, float* hT, float* cT, float* reserve, int B, int T, int F, int H, int act,
                          void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || F <= 0 || H <= 0 || !K || !R || !b || (B > 0 && T > 0 && !x) || !valid_act(act)) {
        set_error("fov_lstm_seq_fwd_bf16: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!layer_bf16_shape_ok(F, H)) { set_error("fov_lstm_seq_fwd_bf16: H = 256 and F <= 256 only"); return FOV_ERR_UNSUPPORTED; }
    if (!steps_ok("fov_lstm_seq_fwd_bf16", T, B)) return FOV_ERR_UNSUPPORTED;
    if (int rc = check_ws(workspace, workspace_bytes, B > 0 ? kStatusBytes + kXchBytes : kStatusBytes)) return rc;
    return launch_layer_bf16(layer_params(x, K, R, b, h0, c0, hs, hT, cT, reserve, B, T, F, H, act, workspace), (hipStream_t)stream);
}

int fov_seq2seq_decode_fwd_bf16(const float* enc_in, const float* dec_in0, const float* enc_K, const float* enc_R,
                                const float* enc_b, const float* dec_K, const float* dec_R, const float* dec_b,
                                const float* dense_W, const float* dense_b, float* out, float* hT, float* cT, int B,
                                int T_in, int T_out, int F_enc, int F_dec, int H, int act, void* workspace,
                                size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T_in < 0 || T_out < 0 || F_enc <= 0 || F_dec <= 0 || H <= 0 || !enc_K || !enc_R || !enc_b ||
        !dec_K || !dec_R || !dec_b || !dense_W || !dense_b ||
        (B > 0 && ((T_in > 0 && !enc_in) || !dec_in0 || (T_out > 0 && !out))) || !valid_act(act)) {
        set_error("fov_seq2seq_decode_fwd_bf16: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!s2s_bf16_shape_ok(F_enc, F_dec, H)) {
        set_error("fov_seq2seq_decode_fwd_bf16: H = 256, F_enc <= 256 and F_dec <= 8 only (got H=%d F_enc=%d F_dec=%d)", H, F_enc, F_dec);
        return FOV_ERR_UNSUPPORTED;
    }
    if (!steps_ok("fov_seq2seq_decode_fwd_bf16", (long)T_in + T_out, B)) return FOV_ERR_UNSUPPORTED;
    if (int rc = check_ws(workspace, workspace_bytes, B > 0 ? kStatusBytes + kXchBytes : kStatusBytes)) return rc;
    LstmParams p = {};
    p.x = enc_in; p.K = enc_K; p.R = enc_R; p.b = enc_b; p.T = T_in; p.F = F_enc;
    bind_decoder(p, dec_in0, dec_K, dec_R, dec_b, dense_W, dense_b, out, hT, cT, B, T_out, F_dec, H, act, workspace);
    return launch_s2s_bf16(p, (hipStream_t)stream);
}

int fov_lstm_stack2_supported_bf16(int B, int T, int F, int H) { return stack2_bf16_shape_ok(B, T, F, H) ? 1 : 0; }

int fov_lstm_stack2_fwd_bf16(const float* x, const float* K1, const float* R1, const float* b1, const float* K2, const float* R2,
                             const float* b2, float* hs1, float* hT1, float* cT1, float* reserve1, float* hs2, float* hT2,
                             float* cT2, float* reserve2, int B, int T, int F, int H, int act, void* workspace,
                             size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || F <= 0 || !K1 || !R1 || !b1 || !K2 || !R2 || !b2 || (B > 0 && T > 0 && !x) || !valid_act(act)) {
        set_error("fov_lstm_stack2_fwd_bf16: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    if (!stack2_bf16_shape_ok(B, T, F, H)) {
        set_error("fov_lstm_stack2_fwd_bf16: H = 256, F <= 96, T >= 2 and one 16-sequence tile per group of eight workgroups only");
        return FOV_ERR_UNSUPPORTED;
    }
    if (int rc = check_ws(workspace, workspace_bytes, kStatusBytes + kXchBytes)) return rc;
    return launch_stack2_bf16(x, K1, R1, b1, K2, R2, b2, hs1, hT1, cT1, reserve1, hs2, hT2, cT2, reserve2, B, T, F, act, workspace,
                              (hipStream_t)stream);
}

int fov_lstm_stack2_supported(int B, int T, int F, int H) { return wide16_pair_shape(B, T, F, H) ? 1 : 0; }

int fov_lstm_stack2_fwd(const float* x, const float* K1, const float* R1, const float* b1, const float* h0_1, const float* c0_1,
                        const float* K2, const float* R2, const float* b2, const float* h0_2, const float* c0_2, float* hs1,
                        float* hT1, float* cT1, float* reserve1, float* hs2, float* hT2, float* cT2, float* reserve2, int B, int T,
                        int F, int H, int act, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || F <= 0 || !K1 || !R1 || !b1 || !K2 || !R2 || !b2 || (B > 0 && T > 0 && !x) || !valid_act(act)) {
        set_error("fov_lstm_stack2_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    if (!wide16_pair_shape(B, T, F, H)) {
        set_error("fov_lstm_stack2_fwd: H = 512, F <= 96, T >= 2 and both layers' groups resident (<= 64 sequences on 256 CUs) only");
        return FOV_ERR_UNSUPPORTED;
    }
    if (int rc = check_ws(workspace, workspace_bytes, kStatusBytes + kXchBytes)) return rc;
    const LstmParams a = layer_params(x, K1, R1, b1, h0_1, c0_1, hs1, hT1, cT1, reserve1, B, T, F, H, act, workspace);
    const LstmParams b = layer_params(nullptr, K2, R2, b2, h0_2, c0_2, hs2, hT2, cT2, reserve2, B, T, H, H, act, workspace);
    return launch_wide16_pair(a, b, (hipStream_t)stream);
}

int fov_lstm_seq_fwd_zx(const float* zx, const float* R, const float* b, const float* h0, const float* c0, float* hs,
                        float* hT, float* cT, float* reserve, int B, int T, int H, int act, int impl, void* workspace,
                        size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || H <= 0 || !R || !b || (B > 0 && T > 0 && !zx) || !valid_act(act) || !valid_impl(impl)) {
        set_error("fov_lstm_seq_fwd_zx: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!steps_ok("fov_lstm_seq_fwd_zx", T, B)) return FOV_ERR_UNSUPPORTED;
    LstmParams p = layer_params(nullptr, nullptr, R, b, h0, c0, hs, hT, cT, reserve, B, T, 1, H, act, workspace);
    p.zx = zx;
    return launch_lstm_fwd(plan_lstm_fwd(B, T, 1, H, impl, true, true), p, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t fov_lstm_seq_bwd_workspace_bytes(int B, int T, int F, int H) {
    if (B <= 0 || T < 0 || F <= 0 || H <= 0) return 256;
    return sizeof(float) * lstm_bwd_workspace_floats(B, T, F, H);
}

// fp32 (any width) and bf16-operand (H = 256) BPTT of one layer: one body behind the two entry points, which fill the layer
// (LstmBwdLayer: the recurrence's operands, the weight-gradient problem, K, dx, the shape)
static int lstm_seq_bwd_entry(const LstmBwdLayer& l, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    const int B = l.B, T = l.T, F = l.F, H = l.H;
    if (B < 0 || T < 0 || F <= 0 || (l.bf16 ? H != 256 : H <= 0) || !l.K || !l.rec.R ||
        (B > 0 && T > 0 && (!l.wg.x || !l.wg.hs || !l.rec.reserve || !l.rec.dz)) || !valid_act(l.act)) {
        set_error(l.bf16 ? "fov_lstm_seq_bwd_bf16: invalid argument (H = 256 only)" : "fov_lstm_seq_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!steps_ok(l.bf16 ? "fov_lstm_seq_bwd_bf16" : "fov_lstm_seq_bwd", T, B)) return FOV_ERR_UNSUPPORTED;
    if (B == 0) return l.accumulate ? FOV_OK : zero_lstm_wgrads(l.wg.dK, l.wg.dR, l.wg.db, F, H, (hipStream_t)stream);
    if (int rc = check_ws(workspace, workspace_bytes, fov_lstm_seq_bwd_workspace_bytes(B, T, F, H))) return rc;
    return lstm_seq_bwd(l, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_lstm_seq_bwd(const float* x, const float* K, const float* R, const float* h0, const float* c0,
                     const float* hs, const float* reserve, const float* dhs, const float* dhT, const float* dcT,
                     float* dz, float* dx, float* dK, float* dR, float* db, float* dh0, float* dc0, int B, int T,
                     int F, int H, int act, int accumulate, void* workspace, size_t workspace_bytes,
                     fov_stream_t stream) {
    const LstmBwdLayer l = {{R, reserve, c0, dhs, dhT, dcT, dz, dh0, dc0, nullptr}, {x, hs, h0, dz, dK, dR, db, F, T}, K, dx,
                            B, T, F, H, act, accumulate, /*bf16=*/0};
    return lstm_seq_bwd_entry(l, workspace, workspace_bytes, stream);
}

int fov_lstm_seq_bwd_bf16(const float* x, const float* K, const float* R, const float* h0, const float* c0,
                          const float* hs, const float* reserve, const float* dhs, const float* dhT, const float* dcT,
                          float* dz, float* dx, float* dK, float* dR, float* db, float* dh0, float* dc0, int B, int T,
                          int F, int H, int act, int accumulate, void* workspace, size_t workspace_bytes,
                          fov_stream_t stream) {
    const LstmBwdLayer l = {{R, reserve, c0, dhs, dhT, dcT, dz, dh0, dc0, nullptr}, {x, hs, h0, dz, dK, dR, db, F, T}, K, dx,
                            B, T, F, H, act, accumulate, /*bf16=*/1};
    return lstm_seq_bwd_entry(l, workspace, workspace_bytes, stream);
}

// H = 32 / 64 (one workgroup per tile): arithmetic alone, any batch; H = 512: the three-role kernel's residency
int fov_lstm_stack2_bwd_supported(int B, int T, int F, int H) {
    if (stack2_tile_bwd_width(H)) return (B >= 1 && B <= kMaxTileBatch && T >= 1 && F >= 1) ? 1 : 0;
    return (F > 0 && bwd16_pair_shape(B, T, H)) ? 1 : 0;
}

size_t fov_lstm_stack2_bwd_workspace_bytes(int B, int T, int F, int H) {
    if (B <= 0 || T < 0 || F <= 0 || H <= 0) return 256;
    return sizeof(float) * lstm_stack2_bwd_workspace_floats(B, T, F, H);
}

int fov_lstm_stack2_bwd(const float* x, const float* R1, const float* K2, const float* R2, const float* h0_1, const float* c0_1,
                        const float* h0_2, const float* c0_2, const float* hs1, const float* reserve1, const float* hs2,
                        const float* reserve2, const float* dhs2, const float* dhT2, const float* dcT2, const float* dhT1,
                        const float* dcT1, float* dz1, float* dz2, float* dK1, float* dR1, float* db1, float* dK2, float* dR2,
                        float* db2, float* dh0_1, float* dc0_1, float* dh0_2, float* dc0_2, int B, int T, int F, int H, int act,
                        int accumulate, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || F <= 0 || H <= 0 || !R1 || !K2 || !R2 ||
        (B > 0 && T > 0 && (!x || !hs1 || !reserve1 || !hs2 || !reserve2 || !dz1 || !dz2)) || !valid_act(act)) {
        set_error("fov_lstm_stack2_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    // the width rule first, as arithmetic: an empty batch of a width the kernel does not have is refused like a full one
    const bool tile = stack2_tile_bwd_width(H);
    if (!tile && H != 512) { set_error("fov_lstm_stack2_bwd: H = 32, 64 or 512 only (got H=%d)", H); return FOV_ERR_UNSUPPORTED; }
    if (B == 0 || T == 0) {
        hipStream_t s = (hipStream_t)stream;
        int rc = accumulate ? FOV_OK : zero_lstm_wgrads(dK1, dR1, db1, F, H, s);
        if (!rc && !accumulate) rc = zero_lstm_wgrads(dK2, dR2, db2, H, H, s);
        // no steps: the state gradients pass through (as fov_lstm_seq_bwd at T = 0; the lower layer gets no dx from the upper one)
        const size_t bh = sizeof(float) * (size_t)B * H;
        const float* src[4] = {dhT2, dcT2, dhT1, dcT1};
        float* dst[4] = {dh0_2, dc0_2, dh0_1, dc0_1};
        for (int i = 0; i < 4 && !rc && bh; ++i) {
            if (!dst[i]) continue;
            hipError_t e = src[i] ? hipMemcpyAsync(dst[i], src[i], bh, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(dst[i], 0, bh, s);
            if (e != hipSuccess) { set_error("fov_lstm_stack2_bwd: %s", hipGetErrorString(e)); rc = FOV_ERR_LAUNCH; }
        }
        return rc;
    }
    if (tile ? B > kMaxTileBatch : !bwd16_pair_shape(B, T, H)) {
        set_error("fov_lstm_stack2_bwd: H = 512 with at most 32 sequences and three role-groups of sixteen workgroups per tile resident, "
                  "or H = 32 / 64 with at most 2^30 sequences only");
        return FOV_ERR_UNSUPPORTED;
    }
    if (int rc = check_ws(workspace, workspace_bytes, fov_lstm_stack2_bwd_workspace_bytes(B, T, F, H))) return rc;
    // the upper layer reads the lower one's hs; its dx stays inside the kernel, which needs no K1
    const LstmBwdLayer low = {{R1, reserve1, c0_1, nullptr, dhT1, dcT1, dz1, dh0_1, dc0_1, nullptr}, {x, hs1, h0_1, dz1, dK1, dR1, db1, F, T},
                              nullptr, nullptr, B, T, F, H, act, accumulate, 0};
    const LstmBwdLayer up = {{R2, reserve2, c0_2, dhs2, dhT2, dcT2, dz2, dh0_2, dc0_2, nullptr}, {hs1, hs2, h0_2, dz2, dK2, dR2, db2, H, T},
                             K2, nullptr, B, T, H, H, act, accumulate, 0};
    return lstm_stack2_bwd(low, up, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

size_t fov_mix_decoder_workspace_bytes(int B, int H) {
    if (B <= 0 || H != 256) return kStatusBytes;
    return mix_decoder_workspace_bytes(B);
}

static int mix_decoder_fwd_impl(const float* dec0, const float* h1, const float* c1, const float* h2, const float* c2,
                        const float* oth_proj, int64_t oth_batch_stride, int64_t oth_step_stride, const float* dec1_K,
                        const float* dec1_R, const float* dec1_b, const float* dec2_K, const float* dec2_R,
                        const float* dec2_b, const float* dense_W, const float* dense_b, const float* mix_Wp, float* out,
                        float* h1T, float* c1T, float* h2T, float* c2T, float* P, float* H1, float* C1, float* H2, float* C2,
                        float* res1, float* res2, int B, int T_out, int H, int O, int act, void* workspace,
                        size_t workspace_bytes, fov_stream_t stream, bool bf16) {
    if (B < 0 || T_out < 0 || O <= 0 || !dec1_K || !dec1_R || !dec1_b || !dec2_K || !dec2_R || !dec2_b || !dense_W ||
        !dense_b || !mix_Wp || (B > 0 && T_out > 0 && (!dec0 || !h1 || !c1 || !h2 || !c2 || !oth_proj || !out)) ||
        oth_batch_stride < 0 || oth_step_stride < 0 || !valid_act(act)) {
        set_error("fov_mix_decoder_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    const int ntrain = (P != nullptr) + (H1 != nullptr) + (C1 != nullptr) + (H2 != nullptr) + (C2 != nullptr) + (res1 != nullptr) +
                       (res2 != nullptr);
    if (ntrain != 0 && ntrain != 7) { set_error("fov_mix_decoder_fwd: give all training buffers or none"); return FOV_ERR_INVALID; }
    // H = 256: the persistent eight-workgroups-per-tile kernels; fp32 H = 32 / 64: one workgroup per tile (mix_tile.hip), no workspace
    const bool tile = !bf16 && (H == 32 || H == 64);
    if ((H != 256 && !tile) || O > 8) {
        set_error(bf16 ? "fov_mix_decoder_fwd_bf16: the fused decoder supports H = 256, O <= 8 (got H=%d O=%d)"
                       : "fov_mix_decoder_fwd: the fused decoder supports H = 256, 32 or 64, O <= 8 (got H=%d O=%d)", H, O);
        return FOV_ERR_UNSUPPORTED;
    }
    if (!steps_ok("fov_mix_decoder_fwd", T_out, B)) return FOV_ERR_UNSUPPORTED;
    if (tile && !mix_tile_shape_ok(B, T_out, H, O, false)) {
        set_error("fov_mix_decoder_fwd: at H = 32 / 64 at most 2^30 sequences and steps (got B=%d T_out=%d)", B, T_out);
        return FOV_ERR_UNSUPPORTED;
    }
    if (B == 0 || T_out == 0) return FOV_OK;
    if (!tile)
        if (int rc = check_ws(workspace, workspace_bytes, fov_mix_decoder_workspace_bytes(B, H))) return rc;
    MixDecParams p = {};
    p.K1 = dec1_K; p.R1 = dec1_R; p.b1 = dec1_b; p.R2 = dec2_R; p.b2 = dec2_b; p.Wd = dense_W; p.bd = dense_b; p.Wp = mix_Wp;
    p.oth_proj = oth_proj; p.oth_sb = (long)oth_batch_stride; p.oth_st = (long)oth_step_stride;
    p.dec0 = dec0; p.h1_0 = h1; p.c1_0 = c1; p.h2_0 = h2; p.c2_0 = c2;
    p.out = out; p.P = P; p.H1 = H1; p.C1 = C1; p.H2 = H2; p.C2 = C2; p.res1 = res1; p.res2 = res2;
    p.h1T = h1T; p.c1T = c1T; p.h2T = h2T; p.c2T = c2T;
    p.B = B; p.T_out = T_out; p.O = O;
    if (tile) {   // the tapes are written one by one, each where its pointer is given: "all or none" was checked above
        p.K2p = dec2_K;
        return mix_tile_fwd_launch(p, H, act, (hipStream_t)stream);
    }
    return bf16 ? mix_decoder_bf16_launch(p, dec2_K, act, ntrain == 7, workspace, (hipStream_t)stream)
                : mix_decoder_launch(p, dec2_K, act, ntrain == 7, workspace, (hipStream_t)stream);
}

int fov_mix_decoder_fwd(const float* dec0, const float* h1, const float* c1, const float* h2, const float* c2,
                        const float* oth_proj, int64_t oth_batch_stride, int64_t oth_step_stride, const float* dec1_K,
                        const float* dec1_R, const float* dec1_b, const float* dec2_K, const float* dec2_R,
                        const float* dec2_b, const float* dense_W, const float* dense_b, const float* mix_Wp, float* out,
                        float* h1T, float* c1T, float* h2T, float* c2T, float* P, float* H1, float* C1, float* H2, float* C2,
                        float* res1, float* res2, int B, int T_out, int H, int O, int act, void* workspace,
                        size_t workspace_bytes, fov_stream_t stream) {
    return mix_decoder_fwd_impl(dec0, h1, c1, h2, c2, oth_proj, oth_batch_stride, oth_step_stride, dec1_K, dec1_R, dec1_b, dec2_K,
                                dec2_R, dec2_b, dense_W, dense_b, mix_Wp, out, h1T, c1T, h2T, c2T, P, H1, C1, H2, C2, res1, res2,
                                B, T_out, H, O, act, workspace, workspace_bytes, stream, false);
}

int fov_mix_decoder_fwd_bf16(const float* dec0, const float* h1, const float* c1, const float* h2, const float* c2,
                             const float* oth_proj, int64_t oth_batch_stride, int64_t oth_step_stride, const float* dec1_K,
                             const float* dec1_R, const float* dec1_b, const float* dec2_K, const float* dec2_R,
                             const float* dec2_b, const float* dense_W, const float* dense_b, const float* mix_Wp, float* out,
                             float* h1T, float* c1T, float* h2T, float* c2T, float* P, float* H1, float* C1, float* H2,
                             float* C2, float* res1, float* res2, int B, int T_out, int H, int O, int act, void* workspace,
                             size_t workspace_bytes, fov_stream_t stream) {
    return mix_decoder_fwd_impl(dec0, h1, c1, h2, c2, oth_proj, oth_batch_stride, oth_step_stride, dec1_K, dec1_R, dec1_b, dec2_K,
                                dec2_R, dec2_b, dense_W, dense_b, mix_Wp, out, h1T, c1T, h2T, c2T, P, H1, C1, H2, C2, res1, res2,
                                B, T_out, H, O, act, workspace, workspace_bytes, stream, true);
}

size_t fov_mix_decoder_bwd_workspace_bytes(int B, int H) {
    if (B <= 0 || H != 256) return kStatusBytes;
    return mix_decoder_bwd_workspace_bytes(B);
}

static int mix_decoder_bwd_impl(const float* M, const float* P, const float* dloss, const float* res1, const float* res2,
                        const float* C1, const float* C2, const float* dec1_K, const float* dec1_R, const float* dec2_K,
                        const float* dec2_R, const float* dense_W, const float* mix_Wp, float* DZ1, float* DZ2,
                        float* dpre_m, float* dpre_p, float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0, int B,
                        int T_out, int H, int O, int act, void* workspace, size_t workspace_bytes, fov_stream_t stream, bool bf16) {
    if (B < 0 || T_out < 0 || O <= 0 || !dec1_K || !dec1_R || !dec2_K || !dec2_R || !dense_W || !mix_Wp ||
        (B > 0 && T_out > 0 && (!M || !P || !dloss || !res1 || !res2 || !C1 || !C2 || !DZ1 || !DZ2 || !dpre_m || !dpre_p ||
                                !dh1_0 || !dc1_0 || !dh2_0 || !dc2_0)) || !valid_act(act)) {
        set_error("fov_mix_decoder_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    const bool tile = !bf16 && H == 32;   // one workgroup per tile (mix_tile.hip), no workspace
    if (!bf16 && H == 64 && O <= 8) {
        set_error("fov_mix_decoder_bwd: H = 64 has a one-launch forward only: the backward keeps three transposed (H,4H) matrices in LDS, "
                  "192 KB at H = 64 (use the per-step entry points on the forward's tapes)");
        return FOV_ERR_UNSUPPORTED;
    }
    if ((H != 256 && !tile) || O > 8) {
        set_error(bf16 ? "fov_mix_decoder_bwd_bf16: the fused decoder supports H = 256, O <= 8 (got H=%d O=%d)"
                       : "fov_mix_decoder_bwd: the fused decoder supports H = 256 or 32, O <= 8 (got H=%d O=%d)", H, O);
        return FOV_ERR_UNSUPPORTED;
    }
    if (!steps_ok("fov_mix_decoder_bwd", T_out, B)) return FOV_ERR_UNSUPPORTED;
    if (tile && !mix_tile_shape_ok(B, T_out, H, O, true)) {
        set_error("fov_mix_decoder_bwd: at H = 32 at most 2^30 sequences and steps (got B=%d T_out=%d)", B, T_out);
        return FOV_ERR_UNSUPPORTED;
    }
    if (B == 0 || T_out == 0) return FOV_OK;
    if (!tile)
        if (int rc = check_ws(workspace, workspace_bytes, fov_mix_decoder_bwd_workspace_bytes(B, H))) return rc;
    MixDecBwdParams p = {};
    p.R1 = dec1_R; p.K1 = dec1_K; p.R2 = dec2_R; p.Wd = dense_W; p.Wp = mix_Wp;
    p.M = M; p.P = P; p.dloss = dloss; p.res1 = res1; p.res2 = res2; p.C1 = C1; p.C2 = C2;
    p.DZ1 = DZ1; p.DZ2 = DZ2; p.dpre_m = dpre_m; p.dpre_p = dpre_p;
    p.dh1_0 = dh1_0; p.dc1_0 = dc1_0; p.dh2_0 = dh2_0; p.dc2_0 = dc2_0;
    p.B = B; p.T_out = T_out; p.O = O;
    if (tile) {
        p.K2p = dec2_K;
        return mix_tile_bwd_launch(p, act, (hipStream_t)stream);
    }
    return bf16 ? mix_decoder_bwd_bf16_launch(p, dec2_K, act, workspace, (hipStream_t)stream)
                : mix_decoder_bwd_launch(p, dec2_K, act, workspace, (hipStream_t)stream);
}

int fov_mix_decoder_tile_supported(int B, int T_out, int H, int O, int backward) {
    return mix_tile_shape_ok(B, T_out, H, O, backward != 0) && steps_ok_quiet(T_out, B) ? 1 : 0;
}

int fov_mix_decoder_prepack(const float* dec2_K, void* workspace_fwd, size_t fwd_bytes, void* workspace_bwd, size_t bwd_bytes, int H,
                            fov_stream_t stream) {
    if (!dec2_K || H != 256) { set_error("fov_mix_decoder_prepack: invalid argument (H = 256)"); return FOV_ERR_INVALID; }
    // both workspaces before the first pack is launched
    if (workspace_fwd)
        if (int rc = check_ws(workspace_fwd, fwd_bytes, mix_decoder_workspace_bytes(1))) return rc;
    if (workspace_bwd)
        if (int rc = check_ws(workspace_bwd, bwd_bytes, mix_decoder_bwd_workspace_bytes(1))) return rc;
    int rc = FOV_OK;
    if (workspace_fwd) rc = mix_decoder_prepack(dec2_K, workspace_fwd, (hipStream_t)stream);
    if (!rc && workspace_bwd) rc = mix_decoder_bwd_prepack(dec2_K, workspace_bwd, (hipStream_t)stream);
    return rc;
}

int fov_mix_decoder_bwd(const float* M, const float* P, const float* dloss, const float* res1, const float* res2,
                        const float* C1, const float* C2, const float* dec1_K, const float* dec1_R, const float* dec2_K,
                        const float* dec2_R, const float* dense_W, const float* mix_Wp, float* DZ1, float* DZ2,
                        float* dpre_m, float* dpre_p, float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0, int B,
                        int T_out, int H, int O, int act, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    return mix_decoder_bwd_impl(M, P, dloss, res1, res2, C1, C2, dec1_K, dec1_R, dec2_K, dec2_R, dense_W, mix_Wp, DZ1, DZ2, dpre_m,
                                dpre_p, dh1_0, dc1_0, dh2_0, dc2_0, B, T_out, H, O, act, workspace, workspace_bytes, stream, false);
}

int fov_mix_decoder_bwd_bf16(const float* M, const float* P, const float* dloss, const float* res1, const float* res2,
                             const float* C1, const float* C2, const float* dec1_K, const float* dec1_R, const float* dec2_K,
                             const float* dec2_R, const float* dense_W, const float* mix_Wp, float* DZ1, float* DZ2,
                             float* dpre_m, float* dpre_p, float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0, int B,
                             int T_out, int H, int O, int act, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    return mix_decoder_bwd_impl(M, P, dloss, res1, res2, C1, C2, dec1_K, dec1_R, dec2_K, dec2_R, dense_W, mix_Wp, DZ1, DZ2, dpre_m,
                                dpre_p, dh1_0, dc1_0, dh2_0, dc2_0, B, T_out, H, O, act, workspace, workspace_bytes, stream, true);
}

size_t fov_seq2seq_decode_workspace_bytes(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int impl) {
    (void)T_in;
    return plan_decode(B, T_out, F_enc, F_dec, H, impl).need;
}

// enc_Rpack / dec_Rpack: fov_lstm_pack_r of enc_R / dec_R or NULL (fov_seq2seq_decode_fwd: both NULL)
static int seq2seq_decode_fwd_impl(const float* enc_in, const float* dec_in0, const float* enc_K, const float* enc_R,
                                   const float* enc_b, const float* dec_K, const float* dec_R, const float* dec_b,
                                   const float* dense_W, const float* dense_b, float* out, float* hT, float* cT,
                                   const float* enc_Rpack, const float* dec_Rpack, int B, int T_in, int T_out, int F_enc,
                                   int F_dec, int H, int act, int impl, void* workspace, size_t workspace_bytes,
                                   fov_stream_t stream) {
    if (B < 0 || T_in < 0 || T_out < 0 || F_enc <= 0 || F_dec <= 0 || H <= 0 || !enc_K || !enc_R || !enc_b ||
        !dec_K || !dec_R || !dec_b || !dense_W || !dense_b ||
        (B > 0 && ((T_in > 0 && !enc_in) || !dec_in0 || (T_out > 0 && !out))) || !valid_act(act) || !valid_impl(impl)) {
        set_error("fov_seq2seq_decode_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if ((((uintptr_t)enc_Rpack | (uintptr_t)dec_Rpack) & 15) != 0) {
        set_error("fov_seq2seq_decode_fwd_packed: a pack must be 16-byte aligned");
        return FOV_ERR_INVALID;
    }
    if (F_dec > 64) { set_error("fov_seq2seq_decode_fwd: F_dec > 64 unsupported"); return FOV_ERR_UNSUPPORTED; }
    if (!steps_ok("fov_seq2seq_decode_fwd", (long)T_in + T_out, B)) return FOV_ERR_UNSUPPORTED;
    const DecodePlan plan = plan_decode(B, T_out, F_enc, F_dec, H, impl);
    if (int rc = check_ws(workspace, workspace_bytes, plan.need)) return rc;
    LstmParams p = {};
    p.x = enc_in; p.K = enc_K; p.R = enc_R; p.b = enc_b; p.T = T_in; p.F = F_enc;
    bind_decoder(p, dec_in0, dec_K, dec_R, dec_b, dense_W, dense_b, out, hT, cT, B, T_out, F_dec, H, act, workspace);
    // the packs are read by the fused cluster launch alone (launch_cluster's gate); every other kernel reads R as it is
    if (lstm_pack_shape_ok(H)) { p.Rpack = enc_Rpack; p.dRpack = dec_Rpack; }
    hipStream_t s = (hipStream_t)stream;
    switch (plan.kernel) {
        case DecodeKernel::Wide16: return launch_wide16_s2s(p, s);
        case DecodeKernel::Cluster: return launch_cluster(p, true, s);
        case DecodeKernel::Generic: break;
    }
    return launch_generic(p, true, s);
}

int fov_seq2seq_decode_fwd(const float* enc_in, const float* dec_in0, const float* enc_K, const float* enc_R,
                           const float* enc_b, const float* dec_K, const float* dec_R, const float* dec_b,
                           const float* dense_W, const float* dense_b, float* out, float* hT, float* cT, int B,
                           int T_in, int T_out, int F_enc, int F_dec, int H, int act, int impl, void* workspace,
                           size_t workspace_bytes, fov_stream_t stream) {
    return seq2seq_decode_fwd_impl(enc_in, dec_in0, enc_K, enc_R, enc_b, dec_K, dec_R, dec_b, dense_W, dense_b, out, hT, cT,
                                   nullptr, nullptr, B, T_in, T_out, F_enc, F_dec, H, act, impl, workspace, workspace_bytes, stream);
}

int fov_seq2seq_decode_fwd_packed(const float* enc_in, const float* dec_in0, const float* enc_K, const float* enc_R,
                                  const float* enc_b, const float* dec_K, const float* dec_R, const float* dec_b,
                                  const float* dense_W, const float* dense_b, float* out, float* hT, float* cT,
                                  const float* enc_Rpack, const float* dec_Rpack, int B, int T_in, int T_out, int F_enc,
                                  int F_dec, int H, int act, int impl, void* workspace, size_t workspace_bytes,
                                  fov_stream_t stream) {
    return seq2seq_decode_fwd_impl(enc_in, dec_in0, enc_K, enc_R, enc_b, dec_K, dec_R, dec_b, dense_W, dense_b, out, hT, cT,
                                   enc_Rpack, dec_Rpack, B, T_in, T_out, F_enc, F_dec, H, act, impl, workspace, workspace_bytes,
                                   stream);
}

int fov_seq2seq_decoder_fwd(const float* dec_in0, const float* h0, const float* c0, const float* dec_K,
                            const float* dec_R, const float* dec_b, const float* dense_W, const float* dense_b, float* out,
                            float* hT, float* cT, int B, int T_out, int F_dec, int H, int act, int impl, void* workspace,
                            size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T_out < 0 || F_dec <= 0 || H <= 0 || !dec_K || !dec_R || !dec_b || !dense_W || !dense_b ||
        (B > 0 && (!dec_in0 || (T_out > 0 && !out))) || !valid_act(act) || !valid_impl(impl)) {
        set_error("fov_seq2seq_decoder_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (F_dec > 64) { set_error("fov_seq2seq_decoder_fwd: F_dec > 64 unsupported"); return FOV_ERR_UNSUPPORTED; }
    if (!steps_ok("fov_seq2seq_decoder_fwd", T_out, B)) return FOV_ERR_UNSUPPORTED;
    const DecodePlan plan = plan_decode(B, T_out, 1, F_dec, H, impl);
    if (int rc = check_ws(workspace, workspace_bytes, plan.need)) return rc;
    LstmParams p = {};
    p.h0 = h0; p.c0 = c0; p.T = 0; p.F = 1;
    bind_decoder(p, dec_in0, dec_K, dec_R, dec_b, dense_W, dense_b, out, hT, cT, B, T_out, F_dec, H, act, workspace);
    hipStream_t s = (hipStream_t)stream;
    if (plan.kernel == DecodeKernel::Cluster) return launch_cluster_decoder(p, s);
    p.K = dec_K; p.R = dec_R; p.b = dec_b;   // the empty encoder phase's weight slots of the other two kernels: any valid pointers
    return plan.kernel == DecodeKernel::Wide16 ? launch_wide16_s2s(p, s) : launch_generic(p, true, s);
}

size_t fov_seq2seq_tf_workspace_bytes(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int impl) {
    if (B <= 0) return kStatusBytes;
    return tf_carve(B, T_in, T_out, F_enc, F_dec, H, impl).total;
}

int fov_seq2seq_tf_fwd(const float* enc_in, const float* dec_in, const float* enc_K, const float* enc_R,
                       const float* enc_b, const float* dec_K, const float* dec_R, const float* dec_b,
                       const float* dense_W, const float* dense_b, float* out, int B, int T_in, int T_out,
                       int F_enc, int F_dec, int H, int act, int impl, void* workspace, size_t workspace_bytes,
                       fov_stream_t stream) {
    // all three calls' operands before the first launch: a refused call has enqueued nothing
    if (B < 0 || T_in < 0 || T_out < 0 || F_enc <= 0 || F_dec <= 0 || H <= 0 || !enc_K || !enc_R || !enc_b || !dec_K || !dec_R ||
        !dec_b || !dense_W || (B > 0 && ((T_in > 0 && !enc_in) || (T_out > 0 && (!dec_in || !out)))) || !valid_act(act) ||
        !valid_impl(impl)) {
        set_error("fov_seq2seq_tf_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!steps_ok("fov_seq2seq_tf_fwd", T_in > T_out ? T_in : T_out, B)) return FOV_ERR_UNSUPPORTED;
    if ((long)B * T_out > 0x7fffffffL) {      // the head's row count is an int
        set_error("fov_seq2seq_tf_fwd: B * T_out exceeds 2^31 - 1");
        return FOV_ERR_UNSUPPORTED;
    }
    if (B == 0) return check_ws(workspace, workspace_bytes, kStatusBytes);
    const TfCarve at = tf_carve(B, T_in, T_out, F_enc, F_dec, H, impl);
    int rc = check_ws(workspace, workspace_bytes, at.total);
    if (rc) return rc;
    float* hT = (float*)((char*)workspace + at.state);
    float* cT = hT + (size_t)B * H;
    float* hs = (float*)((char*)workspace + at.hs);
    prepack_forget(workspace);   // state and hidden sequence lie where mix_decoder_prepack leaves its packed dec2_K
    rc = fov_lstm_seq_fwd(enc_in, enc_K, enc_R, enc_b, nullptr, nullptr, nullptr, hT, cT, B, T_in, F_enc, H, act,
                          impl, workspace, at.state, stream);
    if (rc) return rc;
    rc = fov_lstm_seq_fwd(dec_in, dec_K, dec_R, dec_b, hT, cT, hs, nullptr, nullptr, B, T_out, F_dec, H, act, impl,
                          workspace, at.state, stream);
    if (rc) return rc;
    return fov_dense_fwd(hs, dense_W, dense_b, out, B * T_out, H, F_dec, 1, stream);
}

}  // extern "C"
