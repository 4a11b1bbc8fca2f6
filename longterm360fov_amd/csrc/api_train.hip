// extern "C" entry points of training: weight gradients, Dense backward, losses, pointwise ops, optimizers, the deferred
// reductions and the plain GEMM / column sum.
#include <math.h>

#include "fov_common.h"
#include "bf16_common.h"

using namespace fov;

extern "C" {

int fov_lstm_seq_wgrad(const float* x, const float* hs, const float* h0, const float* dz, float* dK, float* dR, float* db, int B,
                       int T, int F, int H, int accumulate, int bf16, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T < 0 || F <= 0 || H <= 0 || (B > 0 && T > 0 && (!dz || (dK && !x) || (dR && !hs))) || (bf16 && H != 256)) {
        set_error("fov_lstm_seq_wgrad: invalid argument (bf16 operands: H = 256 only)");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, fov_lstm_seq_bwd_workspace_bytes(B, T, F, H))) return rc;
    const LayerWgrad layer = {x, hs, h0, dz, dK, dR, db, F, T};
    return lstm_seq_wgrad(layer, B, H, accumulate, bf16 ? 1 : 0, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_lstm_seq_wgrad_pair_one_launch(int B, int T1, int T2, int H) {
    return (B > 0 && T1 > 0 && T2 > 0 && H > 0 && lstm_seq_wgrad_pair_one_launch(B, T1, T2, H)) ? 1 : 0;
}

int fov_lstm_seq_wgrad_pair(const float* x1, const float* hs1, const float* h0_1, const float* dz1, float* dK1, float* dR1, float* db1,
                            int T1, int F1, const float* x2, const float* hs2, const float* h0_2, const float* dz2, float* dK2,
                            float* dR2, float* db2, int T2, int F2, int B, int H, int accumulate, void* workspace,
                            size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || T1 < 0 || T2 < 0 || F1 <= 0 || F2 <= 0 || H <= 0 || (B > 0 && T1 > 0 && (!dz1 || (dK1 && !x1) || (dR1 && !hs1))) ||
        (B > 0 && T2 > 0 && (!dz2 || (dK2 && !x2) || (dR2 && !hs2)))) {
        set_error("fov_lstm_seq_wgrad_pair: invalid argument");
        return FOV_ERR_INVALID;
    }
    const size_t n1 = fov_lstm_seq_bwd_workspace_bytes(B, T1, F1, H), n2 = fov_lstm_seq_bwd_workspace_bytes(B, T2, F2, H);
    if (int rc = check_ws(workspace, workspace_bytes, n1 > n2 ? n1 : n2)) return rc;
    const LayerWgrad layers[2] = {{x1, hs1, h0_1, dz1, dK1, dR1, db1, F1, T1}, {x2, hs2, h0_2, dz2, dK2, dR2, db2, F2, T2}};
    return lstm_seq_wgrad_layers(2, layers, B, H, accumulate, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_lstm_seq_wgrad_layers(int L, const float* const* x, const int* F, const int* T, const float* const* hs, const float* const* h0,
                              const float* const* dz, float* const* dK, float* const* dR, float* const* db, int B, int H, int accumulate,
                              void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (L < 1 || L > kMaxWgradLayers) {
        set_error("fov_lstm_seq_wgrad_layers: 1 to 4 layers (got %d)", L);
        return FOV_ERR_UNSUPPORTED;
    }
    bool ok = B >= 0 && H > 0 && x && F && T && hs && h0 && dz && dK && dR && db;
    size_t need = 0;
    LayerWgrad layers[kMaxWgradLayers];
    for (int l = 0; ok && l < L; ++l) {
        ok = T[l] >= 0 && F[l] > 0 && !(B > 0 && T[l] > 0 && (!dz[l] || (dK[l] && !x[l]) || (dR[l] && !hs[l])));
        if (ok) {
            const size_t n = fov_lstm_seq_bwd_workspace_bytes(B, T[l], F[l], H);
            need = n > need ? n : need;
            layers[l] = {x[l], hs[l], h0[l], dz[l], dK[l], dR[l], db[l], F[l], T[l]};
        }
    }
    if (!ok) {
        set_error("fov_lstm_seq_wgrad_layers: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, need)) return rc;
    return lstm_seq_wgrad_layers(L, layers, B, H, accumulate, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

size_t fov_dense_bwd_workspace_bytes(int N, int In, int Out) {
    if (N <= 0 || In <= 0 || Out <= 0) return 256;
    size_t a = (size_t)(Out <= 8 ? 1024 : 64) * In * Out, b = (size_t)256 * Out, c = (size_t)(N + 255) / 256 + 64;
    size_t m = a > b ? a : b;
    return sizeof(float) * ((m > c ? m : c) + 64);
}

int fov_dense_bwd(const float* x, const float* W, const float* dpre, float* dx, float* dW, float* db, int N, int In,
                  int Out, int accumulate, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (N < 0 || In <= 0 || Out <= 0 || (N > 0 && (!x || !W || !dpre))) {
        set_error("fov_dense_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, fov_dense_bwd_workspace_bytes(N, In, Out))) return rc;
    return dense_bwd(x, W, dpre, dx, dW, db, N, In, Out, accumulate, (float*)workspace, workspace_bytes / sizeof(float),
                     (hipStream_t)stream, 0);
}

size_t fov_wgrad_fused_workspace_bytes(int64_t N, int In1, int In2, int Out) {
    if (N <= 0 || In1 <= 0 || In2 < 0 || Out <= 0) return 256;
    const size_t a = fov_dense_bwd_workspace_bytes((int)N, In1 + In2 + 1, Out);
    const size_t b = sizeof(float) * gemm_bf16_tn_scratch_floats(In1 + In2 + 1, Out);
    return a > b ? a : b;
}

int fov_wgrad_fused(const float* x1, int In1, const float* x2, int In2, const float* dpre, float* out, int64_t N, int Out,
                    int bias, int accumulate, int bf16, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (N < 0 || In1 <= 0 || In2 < 0 || Out <= 0 || !out || (N > 0 && (!x1 || !dpre || (In2 > 0 && !x2))) || N > 0x7fffffffL) {
        set_error("fov_wgrad_fused: invalid argument");
        return FOV_ERR_INVALID;
    }
    int rc = check_ws(workspace, workspace_bytes, fov_wgrad_fused_workspace_bytes(N, In1, In2, Out));
    if (rc) return rc;
    float* ws = (float*)workspace;
    const size_t wsf = workspace_bytes / sizeof(float);
    const float* a2 = In2 > 0 ? x2 : nullptr;
    if (N > 0 && wgrad_fusable(x1, In1, 0, In1, a2, In2, 0, In2, dpre, Out, 0, out, Out) && (!bf16 || Out >= 64))
        return wgrad_fused(x1, In1, 0, In1, 0, a2, In2, 0, In2, 0, dpre, Out, 0, out, Out, 1, (int)N, bias, accumulate, bf16, ws, wsf,
                           (hipStream_t)stream);
    // shapes the fused product does not take: the same result from the separate products
    rc = dense_bwd(x1, nullptr, dpre, nullptr, out, bias ? out + (size_t)(In1 + In2) * Out : nullptr, (int)N, In1, Out, accumulate, ws,
                   wsf, (hipStream_t)stream, bf16);
    if (rc == 0 && In2 > 0)
        rc = dense_bwd(x2, nullptr, dpre, nullptr, out + (size_t)In1 * Out, nullptr, (int)N, In2, Out, accumulate, ws, wsf,
                       (hipStream_t)stream, bf16);
    return rc;
}

int fov_dense_bwd_bf16(const float* x, const float* W, const float* dpre, float* dx, float* dW, float* db, int N, int In,
                       int Out, int accumulate, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (N < 0 || In <= 0 || Out <= 0 || (N > 0 && (!x || !W || !dpre))) {
        set_error("fov_dense_bwd_bf16: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, fov_dense_bwd_workspace_bytes(N, In, Out))) return rc;
    return dense_bwd(x, W, dpre, dx, dW, db, N, In, Out, accumulate, (float*)workspace, workspace_bytes / sizeof(float),
                     (hipStream_t)stream, 1);
}

int fov_mse_dense_grad(const float* y, const float* target, float* dpre, float* loss, int64_t n, int activation,
                       void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (n < 0 || (n > 0 && (!y || !target || !dpre)) || (activation != 0 && activation != 1)) {
        set_error("fov_mse_dense_grad: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * ((size_t)(n + 255) / 256 + 64))) return rc;
    return mse_dense_grad(y, target, dpre, loss, (long)n, activation, (float*)workspace, workspace_bytes / sizeof(float),
                          (hipStream_t)stream);
}

int fov_mse_dense_grad_w(const float* y, const float* target, float* dpre, float* loss, int64_t n, int activation,
                         float weight, int time_major_B, int time_major_T, int O, void* workspace, size_t workspace_bytes,
                         fov_stream_t stream) {
    const bool tm = time_major_T > 0;
    if (n < 0 || (n > 0 && (!y || !target || !dpre)) || (activation != 0 && activation != 1) ||
        (tm && (time_major_B <= 0 || O <= 0 || (int64_t)time_major_B * time_major_T * O != n))) {
        set_error("fov_mse_dense_grad_w: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * ((size_t)(n + 255) / 256 + 64))) return rc;
    return mse_dense_grad_w(y, target, dpre, loss, (long)n, activation, weight, tm ? time_major_B : 1, tm ? time_major_T : 0,
                            tm ? O : 1, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_mse_dense_grad_db(const float* y, const float* target, float* dpre, float* loss, float* db, int64_t n, int O, int activation,
                          float weight, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (n < 0 || O < 1 || n % O || (n > 0 && (!y || !target || !dpre)) || !db || (activation != 0 && activation != 1)) {
        set_error("fov_mse_dense_grad_db: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * (9 * ((size_t)(n + 255) / 256) + 64 + (size_t)256 * O))) return rc;
    return mse_dense_grad_w(y, target, dpre, loss, (long)n, activation, weight, 1, 0, 1, (float*)workspace, workspace_bytes / sizeof(float),
                            (hipStream_t)stream, db, O);
}

int fov_dense_mse_head_supported(int64_t N, int H, int O) { return dense_mse_head_shape_ok((long)N, H, O) ? 1 : 0; }
size_t fov_dense_mse_head_workspace_bytes(int64_t N, int H, int O) { return sizeof(float) * dense_mse_head_scratch_floats((long)N, H, O); }
int fov_dense_mse_head(const float* hs, const float* W, const float* b, const float* target, float* y, float* dX, float* dW, float* db,
                       float* loss, int64_t N, int H, int O, int activation, float weight, void* workspace, size_t workspace_bytes,
                       fov_stream_t stream) {
    if (N < 0 || H <= 0 || O <= 0 || (N > 0 && (!hs || !W || !b || !target || !dW || !db)) || (activation != 0 && activation != 1)) {
        set_error("fov_dense_mse_head: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (N == 0) return FOV_OK;
    if (int rc = check_ws(workspace, workspace_bytes, fov_dense_mse_head_workspace_bytes(N, H, O))) return rc;
    return dense_mse_head(hs, W, b, target, y, dX, dW, db, loss, (long)N, H, O, activation, weight, (float*)workspace,
                          workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_scale(float* x, int64_t n, float s, fov_stream_t stream) {
    if (n < 0 || (n > 0 && !x)) { set_error("fov_scale: invalid argument"); return FOV_ERR_INVALID; }
    return scale_inplace(x, (long)n, s, (hipStream_t)stream);
}

int fov_act_bwd(const float* dy, const float* y, const float* base, float* out, int64_t n, int activation,
                fov_stream_t stream) {
    if (n < 0 || (n > 0 && (!dy || !y || !out)) || (activation < 0 || activation > 3)) {
        set_error("fov_act_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    return act_bwd(dy, y, base, out, (long)n, activation, (hipStream_t)stream);
}

int fov_act_fwd(const float* x, float* y, int64_t n, int activation, fov_stream_t stream) {
    if (n < 0 || (n > 0 && (!x || !y)) || activation < 0 || activation > 3) {
        set_error("fov_act_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    return act_fwd(x, y, (long)n, activation, (hipStream_t)stream);
}

int fov_gauss_nll_grad(const float* mu, const float* var, const float* y, float* loss, float* dmu, float* dvar, int B,
                       int T_y, int fps, float scale, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || B > kMaxRows3 || T_y <= 0 || fps <= 0 || (long)T_y * fps * 3 > 0x7fffffffL ||
        (B > 0 && (!mu || !var || !y || !dmu || !dvar))) {
        set_error("fov_gauss_nll_grad: invalid argument (B <= 2^29, 3 T_y fps < 2^31)");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * ((size_t)B + 64))) return rc;
    return gauss_nll_grad(mu, var, y, loss, dmu, dvar, B, T_y, fps, scale, (float*)workspace, workspace_bytes / sizeof(float),
                          (hipStream_t)stream);
}

int fov_categorical_crossentropy_grad(const float* p, const float* target, float* dp, float* loss, int64_t n_pix, int C,
                                      void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (n_pix < 0 || C <= 0 || (n_pix > 0 && (!p || !target || !dp))) {
        set_error("fov_categorical_crossentropy_grad: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (n_pix == 0) return FOV_OK;
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * ((size_t)(n_pix + 255) / 256 + 64))) return rc;
    return cce_grad(p, target, dp, loss, (long)n_pix, C, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_xyz_sum1_grad(const float* p, float* dp, float* reg, int64_t n_pix, int C, void* workspace, size_t workspace_bytes,
                      fov_stream_t stream) {
    if (n_pix < 0 || C < 3 || (n_pix > 0 && (!p || !dp))) {
        set_error("fov_xyz_sum1_grad: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (n_pix == 0) return FOV_OK;
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * ((size_t)(n_pix + 255) / 256 + 64))) return rc;
    return xyz_sum1_grad(p, dp, reg, (long)n_pix, C, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_sample_refeed_fwd(const float* mu, const float* var, const float* noise, float* x, int64_t ldx, int B, int fps,
                          int std_mode, int layout, fov_stream_t stream) {
    if (B < 0 || B > kMaxRows3 || fps <= 0 || fps > kMaxFps || ldx < 3 * (int64_t)fps || (std_mode | layout) & ~1 ||
        (B > 0 && (!mu || !var || !noise || !x))) {
        set_error("fov_sample_refeed_fwd: invalid argument (B <= 2^29, fps <= 2^20)");
        return FOV_ERR_INVALID;
    }
    return sample_refeed_fwd(mu, var, noise, x, (long)ldx, B, fps, std_mode, layout, (hipStream_t)stream);
}

int fov_sample_refeed_bwd(const float* dx, int64_t ldx, const float* var, const float* noise, float* dmu, float* dvar, int B,
                          int fps, int std_mode, int layout, int accumulate, fov_stream_t stream) {
    if (B < 0 || B > kMaxRows3 || fps <= 0 || fps > kMaxFps || ldx < 3 * (int64_t)fps || (std_mode | layout) & ~1 ||
        (B > 0 && (!dx || !var || !noise || !dmu || !dvar))) {
        set_error("fov_sample_refeed_bwd: invalid argument (B <= 2^29, fps <= 2^20)");
        return FOV_ERR_INVALID;
    }
    return sample_refeed_bwd(dx, (long)ldx, var, noise, dmu, dvar, B, fps, std_mode, layout, accumulate, (hipStream_t)stream);
}

int fov_rmsprop_tf_step(float* params, const float* grads, float* ms, int64_t n, float lr, float decay, float eps,
                        float clip_value, fov_stream_t stream) {
    if (n < 0 || (n > 0 && (!params || !grads || !ms))) {
        set_error("fov_rmsprop_tf_step: invalid argument");
        return FOV_ERR_INVALID;
    }
    return rmsprop_tf_step(params, grads, ms, (long)n, lr, decay, eps, clip_value, nullptr, nullptr, (hipStream_t)stream);
}

int fov_rmsprop_tf_step_guarded(float* params, const float* grads, float* ms, int64_t n, float lr, float decay, float eps,
                                float clip_value, const void* guard0, const void* guard1, const void* guard2, int64_t* applied,
                                fov_stream_t stream) {
    if (n < 0 || (n > 0 && (!params || !grads || !ms))) {
        set_error("fov_rmsprop_tf_step_guarded: invalid argument");
        return FOV_ERR_INVALID;
    }
    const unsigned* guards[3] = {(const unsigned*)guard0, (const unsigned*)guard1, (const unsigned*)guard2};
    return rmsprop_tf_step(params, grads, ms, (long)n, lr, decay, eps, clip_value, guards, (long long*)applied, (hipStream_t)stream);
}

int fov_adam_step_guarded(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1,
                          float beta2, float eps, int64_t step, const void* guard0, const void* guard1, const void* guard2,
                          int64_t* applied, fov_stream_t stream) {
    if (n < 0 || step < 1 || (n > 0 && (!params || !grads || !m || !v))) {
        set_error("fov_adam_step: invalid argument");
        return FOV_ERR_INVALID;
    }
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    const unsigned* guards[3] = {(const unsigned*)guard0, (const unsigned*)guard1, (const unsigned*)guard2};
    return adam_step(params, grads, m, v, (long)n, (float)lr_t, beta1, beta2, eps, guards, (long long*)applied, (hipStream_t)stream);
}

int fov_reduce_defer_begin(float* grad_base, size_t grad_floats, void* arena, size_t arena_bytes, fov_stream_t stream) {
    if (grad_base && (!arena || arena_bytes < 256)) { set_error("fov_reduce_defer_begin: invalid arena"); return FOV_ERR_INVALID; }
    return defer_begin(grad_base, grad_floats, (float*)arena, arena_bytes / sizeof(float), (hipStream_t)stream);
}
int fov_reduce_defer_flush(const float* grad_base, fov_stream_t stream) { return defer_flush(grad_base, (hipStream_t)stream); }
int fov_reduce_defer_end(const float* grad_base, fov_stream_t stream) { return defer_end(grad_base, (hipStream_t)stream); }

int fov_guard_flag(const void* guard0, const void* guard1, const void* guard2, float* out, fov_stream_t stream) {
    if (!out) { set_error("fov_guard_flag: invalid argument"); return FOV_ERR_INVALID; }
    const unsigned* guards[3] = {(const unsigned*)guard0, (const unsigned*)guard1, (const unsigned*)guard2};
    return guard_flag(guards, out, (hipStream_t)stream);
}

int fov_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, int64_t step, fov_stream_t stream) {
    return fov_adam_step_guarded(params, grads, m, v, n, lr, beta1, beta2, eps, step, nullptr, nullptr, nullptr, nullptr, stream);
}

int fov_rmsprop_step_guarded(float* params, const float* grads, float* accum, int64_t n, float lr, float rho, float eps,
                             const void* guard0, const void* guard1, const void* guard2, int64_t* applied, fov_stream_t stream) {
    if (n < 0 || (n > 0 && (!params || !grads || !accum))) {
        set_error("fov_rmsprop_step: invalid argument");
        return FOV_ERR_INVALID;
    }
    const unsigned* guards[3] = {(const unsigned*)guard0, (const unsigned*)guard1, (const unsigned*)guard2};
    return rmsprop_step(params, grads, accum, (long)n, lr, rho, eps, guards, (long long*)applied, (hipStream_t)stream);
}

int fov_rmsprop_step(float* params, const float* grads, float* accum, int64_t n, float lr, float rho, float eps,
                     fov_stream_t stream) {
    return fov_rmsprop_step_guarded(params, grads, accum, n, lr, rho, eps, nullptr, nullptr, nullptr, nullptr, stream);
}

size_t fov_mix_head_wgrad_workspace_bytes(int B, int T_out, int H, int O, int n_others) {
    if (B <= 0 || T_out <= 0 || H <= 0 || O <= 0 || n_others < 0) return 256;
    return sizeof(float) * mix_head_wgrad_scratch_floats(B, T_out, H, O, n_others);
}

int fov_mix_head_wgrad(const float* h2, const float* dpre_p, const float* others, const float* p, const float* dpre_m, float* out,
                       int B, int T_out, int H, int O, int n_others, int accumulate, void* workspace, size_t workspace_bytes,
                       fov_stream_t stream) {
    if (B < 0 || T_out < 0 || H <= 0 || O <= 0 || O > 8 || n_others < 0 || !out ||
        (B > 0 && T_out > 0 && (!h2 || !dpre_p || !p || !dpre_m || (n_others > 0 && !others)))) {
        set_error("fov_mix_head_wgrad: invalid argument (O <= 8)");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, fov_mix_head_wgrad_workspace_bytes(B, T_out, H, O, n_others))) return rc;
    return mix_head_wgrad(h2, dpre_p, others, p, dpre_m, out, B, T_out, H, O, n_others, accumulate, (float*)workspace,
                          workspace_bytes / sizeof(float), (hipStream_t)stream);
}

size_t fov_matmul_workspace_bytes(int M, int K, int N) {
    (void)K;
    if (M <= 0 || N <= 0) return 256;
    size_t part = (size_t)64 * M * N;
    if (part > ((size_t)64 << 20)) part = (size_t)64 << 20;   // split-K partials are optional: cap at 256 MB
    return sizeof(float) * (part + 64);
}

int fov_matmul(const float* a, const float* b, float* c, int M, int K, int N, void* workspace, size_t workspace_bytes,
               fov_stream_t stream) {
    if (M < 0 || K < 0 || N < 0 || (M > 0 && N > 0 && (!c || (K > 0 && (!a || !b))))) {
        set_error("fov_matmul: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (workspace && (((uintptr_t)workspace) & 15)) { set_error("workspace must be 16-byte aligned"); return FOV_ERR_WORKSPACE; }
    return matmul_f32(a, b, c, M, K, N, (float*)workspace, workspace ? workspace_bytes / sizeof(float) : 0, (hipStream_t)stream);
}

int fov_colsum(const float* x, float* out, int64_t rows, int cols, int accumulate, void* workspace, size_t workspace_bytes,
               fov_stream_t stream) {
    // cols <= 2^24: the wide form counts its column blocks, (cols + 255) / 256, in an int
    if (rows < 0 || cols <= 0 || cols > (1 << 24) || !out || (rows > 0 && !x)) {
        set_error("fov_colsum: invalid argument (1 <= cols <= 2^24)");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, sizeof(float) * ((size_t)256 * cols + 64))) return rc;
    if (rows == 0) {
        return accumulate ? FOV_OK : zero_grad(out, (size_t)cols, (hipStream_t)stream);
    }
    return colsum(x, out, (long)rows, cols, accumulate, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

}  // extern "C"
