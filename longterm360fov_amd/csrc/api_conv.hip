// extern "C" entry points of the convolution path: Conv2D, the ConvLSTM2D cell and gates, forward and backward, and the
// last-axis softmax of the heat-map head.
#include "fov_common.h"

using namespace fov;

// a (kh,kw,C,N) fp32 kernel of 2 GiB or more: the weight-gradient launchers count its tiles and taps in ints
static bool weights_over_2g(int kh, int kw, int C, int N) {
    const long lim = 1L << 29;
    long t = (long)kh * kw;
    if (t >= lim) return true;
    t *= C;
    if (t >= lim) return true;
    return t * N >= lim;
}

extern "C" {

int fov_conv2d_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, const float* w, const float* b,
                   const float* add, float* y, int B, int H, int W, int C, int N, int kh, int kw, int activation,
                   fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 ||
        x_pixel_stride < C || x_batch_stride < (int64_t)H * W * x_pixel_stride || !w || (B > 0 && (!x || !y)) || (activation != 0 && activation != 2)) {
        set_error("fov_conv2d_fwd: invalid argument (odd kernel sizes only, activation 0 or 2)");
        return FOV_ERR_INVALID;
    }
    return conv2d_fwd(x, (long)x_pixel_stride, (long)x_batch_stride, w, b, add, y, B, H, W, C, N, kh, kw, activation, (hipStream_t)stream);
}

size_t fov_conv2d_bf16_packed_bytes(int C, int N, int kh, int kw) {
    if (C <= 0 || N <= 0 || kh <= 0 || kw <= 0) return 0;
    return conv2d_bf16_packed_bytes(C, N, kh, kw);
}

int fov_conv2d_pack_bf16(const float* w, void* packed, int C, int N, int kh, int kw, fov_stream_t stream) {
    if (!w || !packed || (((uintptr_t)packed) & 15) || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0) {
        set_error("fov_conv2d_pack_bf16: invalid argument (odd kernel sizes only, packed 16-byte aligned)");
        return FOV_ERR_INVALID;
    }
    if (conv2d_bf16_packed_bytes(C, N, kh, kw) >= ((size_t)1 << 31) || (int64_t)kh * kw * C * N * 4 >= ((int64_t)1 << 31)) {
        set_error("fov_conv2d_pack_bf16: operand larger than 2 GiB");
        return FOV_ERR_UNSUPPORTED;
    }
    return conv2d_pack_bf16(w, packed, C, N, kh, kw, (hipStream_t)stream);
}

int fov_conv2d_fwd_bf16(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, const void* w_packed, const float* b,
                        float* y, int B, int H, int W, int C, int N, int kh, int kw, int activation, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 ||
        x_pixel_stride < C || x_batch_stride < (int64_t)H * W * x_pixel_stride || !w_packed || (((uintptr_t)w_packed) & 15) ||
        (B > 0 && (!x || !y)) || (activation != 0 && activation != 2)) {
        set_error("fov_conv2d_fwd_bf16: invalid argument (odd kernel sizes only, activation 0 or 2, w_packed 16-byte aligned)");
        return FOV_ERR_INVALID;
    }
    return conv2d_fwd_bf16(x, (long)x_pixel_stride, (long)x_batch_stride, w_packed, b, y, B, H, W, C, N, kh, kw, activation,
                           (hipStream_t)stream);
}

int fov_conv2d_dilated_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, const float* w, const float* b,
                           const float* add, float* y, int B, int H, int W, int C, int N, int kh, int kw, int dilation, int activation,
                           fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 || dilation < 1 ||
        x_pixel_stride < C || x_batch_stride < (int64_t)H * W * x_pixel_stride || !w || (B > 0 && (!x || !y)) || (activation != 0 && activation != 2)) {
        set_error("fov_conv2d_dilated_fwd: invalid argument (odd kernel sizes only, dilation >= 1, activation 0 or 2)");
        return FOV_ERR_INVALID;
    }
    return conv2d_fwd(x, (long)x_pixel_stride, (long)x_batch_stride, w, b, add, y, B, H, W, C, N, kh, kw, activation, (hipStream_t)stream, dilation);
}

int fov_conv2d_fwd2(const float* x1, int64_t x1_pixel_stride, int64_t x1_batch_stride, int C1, const float* x2,
                    int64_t x2_pixel_stride, int64_t x2_batch_stride, int C2, const float* w, const float* b, const float* add,
                    float* y, int B, int H, int W, int N, int kh, int kw, int activation, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C1 <= 0 || C2 <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 ||
        x1_pixel_stride < C1 || x1_batch_stride < (int64_t)H * W * x1_pixel_stride || x2_pixel_stride < C2 ||
        x2_batch_stride < (int64_t)H * W * x2_pixel_stride || !w || (B > 0 && (!x1 || !x2 || !y)) ||
        (activation != 0 && activation != 2)) {
        set_error("fov_conv2d_fwd2: invalid argument (odd kernel sizes only, activation 0 or 2)");
        return FOV_ERR_INVALID;
    }
    return conv2d_fwd2(x1, (long)x1_pixel_stride, (long)x1_batch_stride, C1, x2, (long)x2_pixel_stride, (long)x2_batch_stride, C2,
                       w, b, add, y, B, H, W, N, kh, kw, activation, (hipStream_t)stream);
}

int fov_convlstm_cell_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, int C, const float* h_prev,
                          int64_t h_prev_pixel_stride, int64_t h_prev_batch_stride, const float* w, const float* b,
                          const float* c_prev, float* c_new, float* h, int64_t h_pixel_stride, float* gates, int B, int H, int W,
                          int F, int kh, int kw, int recurrent_activation, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || F <= 0 || kh <= 0 || kw <= 0 || !(kh & 1) || !(kw & 1) ||
        (B > 0 && (!x || !w || !c_new || !h)) || x_pixel_stride < C || x_batch_stride < (int64_t)H * W * x_pixel_stride ||
        h_pixel_stride < F ||
        (h_prev && (h_prev_pixel_stride < F || h_prev_batch_stride < (int64_t)H * W * h_prev_pixel_stride || h_prev == h)) ||
        !valid_act(recurrent_activation)) {
        set_error("fov_convlstm_cell_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    return convlstm_cell_fwd(x, (long)x_pixel_stride, (long)x_batch_stride, C, h_prev, (long)h_prev_pixel_stride,
                             (long)h_prev_batch_stride, w, b, c_prev, c_new, h, (long)h_pixel_stride, gates, B, H, W, F, kh, kw,
                             recurrent_activation, (hipStream_t)stream);
}

size_t fov_convlstm_cell_bf16_packed_bytes(int Ctot, int F, int kh, int kw) {
    if (Ctot <= 0 || F <= 0 || kh <= 0 || kw <= 0) return 0;
    return convlstm_cell_bf16_packed_bytes(Ctot, F, kh, kw);
}

int fov_convlstm_cell_pack_bf16(const float* w, void* packed, int Ctot, int F, int kh, int kw, fov_stream_t stream) {
    if (!w || !packed || (((uintptr_t)packed) & 15) || Ctot <= 0 || F <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0) {
        set_error("fov_convlstm_cell_pack_bf16: invalid argument (odd kernel sizes only, packed 16-byte aligned)");
        return FOV_ERR_INVALID;
    }
    if (convlstm_cell_bf16_packed_bytes(Ctot, F, kh, kw) >= ((size_t)1 << 31) || (int64_t)kh * kw * Ctot * 4 * F * 4 >= ((int64_t)1 << 31)) {
        set_error("fov_convlstm_cell_pack_bf16: operand larger than 2 GiB");
        return FOV_ERR_UNSUPPORTED;
    }
    return convlstm_cell_pack_bf16(w, packed, Ctot, F, kh, kw, (hipStream_t)stream);
}

int fov_convlstm_cell_fwd_bf16(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, int C, const float* h_prev,
                               int64_t h_prev_pixel_stride, int64_t h_prev_batch_stride, const void* w_packed, const float* b,
                               const float* c_prev, float* c_new, float* h, int64_t h_pixel_stride, float* gates, int B, int H, int W,
                               int F, int kh, int kw, int recurrent_activation, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || F <= 0 || kh <= 0 || kw <= 0 || !(kh & 1) || !(kw & 1) || !w_packed ||
        (((uintptr_t)w_packed) & 15) || (B > 0 && (!x || !c_new || !h)) || x_pixel_stride < C ||
        x_batch_stride < (int64_t)H * W * x_pixel_stride || h_pixel_stride < F ||
        (h_prev && (h_prev_pixel_stride < F || h_prev_batch_stride < (int64_t)H * W * h_prev_pixel_stride || h_prev == h)) ||
        !valid_act(recurrent_activation)) {
        set_error("fov_convlstm_cell_fwd_bf16: invalid argument (odd kernel sizes only, w_packed 16-byte aligned)");
        return FOV_ERR_INVALID;
    }
    return convlstm_cell_fwd_bf16(x, (long)x_pixel_stride, (long)x_batch_stride, C, h_prev, (long)h_prev_pixel_stride,
                                  (long)h_prev_batch_stride, w_packed, b, c_prev, c_new, h, (long)h_pixel_stride, gates, B, H, W, F,
                                  kh, kw, recurrent_activation, (hipStream_t)stream);
}

int fov_convlstm_cell_dilated_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, int C, const float* h_prev,
                                  int64_t h_prev_pixel_stride, int64_t h_prev_batch_stride, const float* w, const float* b,
                                  const float* c_prev, float* c_new, float* h, int64_t h_pixel_stride, float* gates, int B, int H, int W,
                                  int F, int kh, int kw, int dilation, int recurrent_activation, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || F <= 0 || kh <= 0 || kw <= 0 || !(kh & 1) || !(kw & 1) || dilation < 1 ||
        (B > 0 && (!x || !w || !c_new || !h)) || x_pixel_stride < C || x_batch_stride < (int64_t)H * W * x_pixel_stride ||
        h_pixel_stride < F ||
        (h_prev && (h_prev_pixel_stride < F || h_prev_batch_stride < (int64_t)H * W * h_prev_pixel_stride || h_prev == h)) ||
        !valid_act(recurrent_activation)) {
        set_error("fov_convlstm_cell_dilated_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    return convlstm_cell_fwd(x, (long)x_pixel_stride, (long)x_batch_stride, C, h_prev, (long)h_prev_pixel_stride,
                             (long)h_prev_batch_stride, w, b, c_prev, c_new, h, (long)h_pixel_stride, gates, B, H, W, F, kh, kw,
                             recurrent_activation, (hipStream_t)stream, dilation);
}

int fov_convlstm_gates(const float* z, float* c, float* h, int64_t h_pixel_stride, int64_t rows, int F, int act,
                       fov_stream_t stream) {
    if (rows < 0 || F <= 0 || h_pixel_stride < F || (rows > 0 && (!z || !c || !h)) || !valid_act(act)) {
        set_error("fov_convlstm_gates: invalid argument");
        return FOV_ERR_INVALID;
    }
    return convlstm_gates(z, c, h, (long)h_pixel_stride, (long)rows, F, act, (hipStream_t)stream);
}

int fov_softmax_lastdim(const float* x, float* y, int64_t rows, int n, fov_stream_t stream) {
    if (rows < 0 || n <= 0 || (rows > 0 && (!x || !y))) {
        set_error("fov_softmax_lastdim: invalid argument");
        return FOV_ERR_INVALID;
    }
    return softmax_lastdim(x, y, (long)rows, n, (hipStream_t)stream);
}

int fov_convlstm_gates_train(const float* z, const float* c_prev, float* c_new, float* h, int64_t h_pixel_stride,
                             float* gates, int64_t rows, int F, int act, fov_stream_t stream) {
    if (rows < 0 || F <= 0 || h_pixel_stride < F || (rows > 0 && (!z || !c_new || !h || !gates)) || !valid_act(act)) {
        set_error("fov_convlstm_gates_train: invalid argument");
        return FOV_ERR_INVALID;
    }
    return convlstm_gates_train(z, c_prev, c_new, h, (long)h_pixel_stride, gates, (long)rows, F, act, (hipStream_t)stream);
}

int fov_convlstm_gates_bwd(const float* dh, int64_t dh_pixel_stride, float* dc, const float* gates, const float* c_prev,
                           const float* c_new, float* dz, int64_t rows, int F, int act, fov_stream_t stream) {
    if (rows < 0 || F <= 0 || dh_pixel_stride < F || (rows > 0 && (!dh || !dc || !gates || !c_new || !dz)) || !valid_act(act)) {
        set_error("fov_convlstm_gates_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    return convlstm_gates_bwd(dh, (long)dh_pixel_stride, dc, gates, c_prev, c_new, dz, (long)rows, F, act, (hipStream_t)stream);
}

size_t fov_conv2d_wgrad_workspace_bytes(int C, int N, int kh, int kw) {
    if (C <= 0 || N <= 0 || kh <= 0 || kw <= 0) return 256;
    return sizeof(float) * conv2d_wgrad_workspace_floats(C, N, kh, kw);
}

int fov_conv2d_wgrad(const float* x, int64_t x_pixel_stride, const float* dy, float* dw, int B, int H, int W, int C, int N,
                     int kh, int kw, int accumulate, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 ||
        x_pixel_stride < C || !dw || (B > 0 && (!x || !dy))) {
        set_error("fov_conv2d_wgrad: invalid argument (odd kernel sizes only)");
        return FOV_ERR_INVALID;
    }
    if (weights_over_2g(kh, kw, C, N)) { set_error("fov_conv2d_wgrad: dw of 2 GiB or more"); return FOV_ERR_UNSUPPORTED; }
    if (workspace && (((uintptr_t)workspace) & 15)) { set_error("workspace must be 16-byte aligned"); return FOV_ERR_WORKSPACE; }
    return conv2d_wgrad(x, (long)x_pixel_stride, dy, dw, B, H, W, C, N, kh, kw, accumulate, (float*)workspace,
                        workspace ? workspace_bytes / sizeof(float) : 0, (hipStream_t)stream);
}

size_t fov_conv2d_wgrad_bf16_workspace_bytes(int C, int N, int kh, int kw) {
    if (C <= 0 || N <= 0 || kh <= 0 || kw <= 0) return 256;
    return sizeof(float) * conv2d_wgrad_bf16_workspace_floats(C, N, kh, kw);
}

int fov_conv2d_wgrad_bf16(const float* x, int64_t x_pixel_stride, const float* dy, int64_t dy_row_stride, float* dw, int B, int H,
                          int W, int C, int N, int kh, int kw, int accumulate, void* workspace, size_t workspace_bytes,
                          fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 ||
        x_pixel_stride < C || dy_row_stride < N || !dw || (B > 0 && (!x || !dy))) {
        set_error("fov_conv2d_wgrad_bf16: invalid argument (odd kernel sizes only)");
        return FOV_ERR_INVALID;
    }
    if (int rc = check_ws(workspace, workspace_bytes, fov_conv2d_wgrad_bf16_workspace_bytes(C, N, kh, kw))) return rc;
    return conv2d_wgrad_bf16(x, (long)x_pixel_stride, dy, (long)dy_row_stride, dw, B, H, W, C, N, kh, kw, accumulate,
                             (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

int fov_conv2d_dilated_wgrad(const float* x, int64_t x_pixel_stride, const float* dy, float* dw, int B, int H, int W, int C, int N,
                             int kh, int kw, int dilation, int accumulate, void* workspace, size_t workspace_bytes, fov_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || kh <= 0 || kw <= 0 || (kh & 1) == 0 || (kw & 1) == 0 || dilation < 1 ||
        x_pixel_stride < C || !dw || (B > 0 && (!x || !dy))) {
        set_error("fov_conv2d_dilated_wgrad: invalid argument (odd kernel sizes only, dilation >= 1)");
        return FOV_ERR_INVALID;
    }
    if (weights_over_2g(kh, kw, C, N)) { set_error("fov_conv2d_dilated_wgrad: dw of 2 GiB or more"); return FOV_ERR_UNSUPPORTED; }
    if (workspace && (((uintptr_t)workspace) & 15)) { set_error("workspace must be 16-byte aligned"); return FOV_ERR_WORKSPACE; }
    return conv2d_wgrad(x, (long)x_pixel_stride, dy, dw, B, H, W, C, N, kh, kw, accumulate, (float*)workspace,
                        workspace ? workspace_bytes / sizeof(float) : 0, (hipStream_t)stream, dilation);
}

int fov_conv2d_weight_transpose(const float* w, float* wt, int kh, int kw, int C, int N, fov_stream_t stream) {
    if (kh <= 0 || kw <= 0 || C <= 0 || N <= 0 || !w || !wt) {
        set_error("fov_conv2d_weight_transpose: invalid argument");
        return FOV_ERR_INVALID;
    }
    return conv_weight_transpose(w, wt, kh, kw, C, N, (hipStream_t)stream);
}

int fov_softmax_lastdim_bwd(const float* dp, const float* p, float* dy, int64_t rows, int n, fov_stream_t stream) {
    if (rows < 0 || n <= 0 || (rows > 0 && (!dp || !p || !dy))) {
        set_error("fov_softmax_lastdim_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    return softmax_lastdim_bwd(dp, p, dy, (long)rows, n, (hipStream_t)stream);
}

}  // extern "C"
