// Shared device/host helpers for libfov360_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fov360.h"

namespace fov {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Gate activations.  v_exp_f32 / v_rcp_f32 based (about 1 ulp each); absolute error of the
// logistic and of tanh is below 3e-7, far inside the 1e-3 relative parity bound on outputs.
// __builtin_amdgcn_rcpf is the bare v_rcp_f32: __frcp_rn expands to the 10-instruction
// correctly-rounded division sequence, which tripled the cell-update time.
__device__ __forceinline__ float sigmoid_f(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float hard_sigmoid_f(float x) {
    return fminf(fmaxf(fmaf(0.2f, x, 0.5f), 0.0f), 1.0f);
}
__device__ __forceinline__ float tanh_f(float x) {
    // 1 - 2/(1+e^{2x}); saturates cleanly to +-1, no NaN for any finite x
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
}
template <int ACT>
__device__ __forceinline__ float rec_act(float x) {
    return ACT == FOV_ACT_HARD_SIGMOID ? hard_sigmoid_f(x) : sigmoid_f(x);
}
// its derivative s'(a) from the stored OUTPUT a (as Keras/TF autodiff evaluates it): a(1-a) (sigmoid) or 0.2*[0<a<1] (hard_sigmoid)
template <int ACT>
__device__ __forceinline__ float rec_act_grad(float a) {
    return ACT == FOV_ACT_HARD_SIGMOID ? ((a > 0.f && a < 1.f) ? 0.2f : 0.f) : a * (1.f - a);
}
// BPTT pointwise step t of one cell (Keras LSTMCell backward), from the activated gates i,f,g,o, c = c_t and c_prev = c_{t-1}:
//   dh = dhs[:,t] + dh_rec;  tc = tanh(c_t);  do = dh*tc;  dc += dh*o*(1-tc^2)
//   dz = [dc*g*s'(i), dc*c_{t-1}*s'(f), dc*i*(1-g^2), do*s'(o)];  dc *= f
// `dc` comes in as the gradient that reaches c_t from step t+1 and goes out as the gradient for c_{t-1}.  No masking here:
// a kernel that zeroes the dz of dead rows does so on the result.
// The other BPTT kernels (lstm_bwd16, lstm_bwd_cluster, mix_decoder_bwd, the bf16 forms, the stepped pointwise kernels) still
// write the same expression tree out, with rec_act_grad: through this helper their instruction schedule changes (the
// values do not), and a schedule change of those kernels wants a measurement of its own.
template <int ACT>
__device__ __forceinline__ void lstm_cell_bwd(float i, float f, float g, float o, float c, float c_prev, float dh, float& dc,
                                              float (&dz)[4]) {
    const float tc = tanh_f(c);
    const float dcv = dc + dh * o * (1.f - tc * tc);
    dz[0] = dcv * g * rec_act_grad<ACT>(i);
    dz[1] = dcv * c_prev * rec_act_grad<ACT>(f);
    dz[2] = dcv * i * (1.f - g * g);
    dz[3] = dh * tc * rec_act_grad<ACT>(o);
    dc = dcv * f;
}

// Everything one launch of the LSTM kernels needs.  Phase 1 ("layer"/encoder): T steps over
// x:(B,T,F) with weights K,R,b from (h0,c0).  Phase 2 (decode only): T_out autoregressive
// steps with weights dK,dR,db fed by y_{t-1} = tanh(h W + bias), y_{-1} = dec_in0.
struct LstmParams {
    const float* x;
    const float* zx;           // optional (B,T,4H): precomputed x.K (stacked layers); then x/K are unused, b is still added
    const float* K;
    const float* R;
    const float* b;
    const float* h0;
    const float* c0;
    float* hs;
    float* hT;
    float* cT;
    float* reserve;            // training only: (B,T,5,H) = i,f,g,o,c of every step (phase 1), or NULL
    const float* dec_in0;
    const float* dK;
    const float* dR;
    const float* db;
    const float* dW;
    const float* dbias;
    float* out;
    int B, T, F, H;
    int T_out, F_dec;
    int act;
    // cluster kernel only
    unsigned long long* xch;   // granule exchange buffers
    unsigned* status;          // status[0] = timeout flag
    int num_groups;            // resident groups (persistent loop over 16-sequence tiles)
    int num_tiles;
    int epoch_span;            // epochs this launch may consume: the last workgroup to leave adds it to the header's base
    int force_safe_exchange;   // 1: never take the same-XCD fast path (tests)
    int xcd_pad;               // lstm_wide16.hip: grid padded to 8 x (workgroups per tile), block b = member b / 8 of group b % 8
    int trio;                  // lstm_wide16.hip, stacked launch on the XCD-per-group grid: 3 three roles, 2 two roles (0: not stacked) -
                               // layer 1 also publishes h_t (sc1) into a mirror ring for its readers on other XCDs
    // lstm_cluster.hip, fused encode + decode launch only: R / dR in fragment order (lstm_pack.hip), or NULL.  Both given: each
    // phase loads its R slice as 16-byte loads from the pack; otherwise (and in every other kernel) R / dR are read as they are
    const float* Rpack;
    const float* dRpack;
};
// lstm_pack.hip: out (H * 4H floats, 16-byte aligned) = R (H,4H) in the order the cluster kernel's MFMA B fragments take it
bool lstm_pack_shape_ok(int H);
int launch_lstm_pack_r(const float* R, int H, float* out, hipStream_t stream);

int launch_generic(const LstmParams& p, bool decode, hipStream_t stream);
long generic_launch_count();   // launches of the generic (VALU) LSTM kernel so far in this process (diagnostic)
bool wide16_s2s_shape(int B, int F_enc, int F_dec, int H);   // lstm_wide16.hip: encoder + free-running decoder, small batches
int launch_wide16_s2s(const LstmParams& p, hipStream_t stream);
int launch_cluster(const LstmParams& p, bool decode, hipStream_t stream);
int launch_cluster_decoder(const LstmParams& p, hipStream_t stream);   // MODE_DECODE alone, from (p.h0, p.c0)
bool cluster_shape_ok(int F, int H);
bool stacked_s2s_shape_ok(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L);   // lstm_stacked_s2s.hip, lstm_stacked_train.hip: the L-layer seq2seq decode / training graph as one launch per direction
bool selffed_shape_ok(int B, int T, int O, int H);   // lstm_selffed.hip: the self-fed one-layer decoder's unroll (forward with tapes, BPTT) as one launch each
bool selffed2_shape_ok(int B, int T, int O, int H, bool backward);   // lstm_selffed2.hip: the self-fed two-layer decoder's unroll; the BPTT at H = 32 only
size_t cluster_workspace_bytes(int B, int H);
int cluster_num_groups(int B, int H);
int device_cu_count();                               // CUs of the current device a persistent grid may count on (FOV_DBG_RESIDENT_LIMIT caps it: tests)
// getenv results cached at first use (fov_reload_env re-reads them): nothing on a launch path calls getenv
struct EnvKnobs {
    int force_safe_exchange, two_launches, resident_limit;
    int bwd_stepped, no_wgrad_fusion, no_dx_fusion, bwd_groups4, gemm_bf16_split, gemm_bf16_noremap, gemm_bf16_shallow, no_wgrad_group, dbg_trace, no_wide16_trio, no_wgrad_lines;   // experiment switches (tools/)
    int gemm_variant, gemm_split;   // FOV_GEMM_VARIANT / FOV_GEMM_SPLIT: tile shape / K slices of the fp32 GEMM forced (experiments)
    int no_wide16;       // FOV_NO_WIDE16=1: width-512 layers stay on the 16-workgroup form (tests / A-B timing)
    int no_cell_patch;   // FOV_NO_CELL_PATCH=1: ConvLSTM2D steps stay on the implicit-GEMM cell (tests compare the two forms)
    int no_conv_patch;   // FOV_NO_CONV_PATCH=1: Conv2D layers stay on the tap-gathering implicit GEMM (tests / A-B timing; conv_patch.hip)
    int no_xcd_pad;      // FOV_NO_XCD_PAD=1: no padded grids for same-XCD placement (lstm_wide16 / lstm_bwd16 / fused H = 128 kernel)
    int xcd_pad_max;     // FOV_XCD_PAD_MAX: members per group up to which a grid is padded (default 16; 32 measured slower)
    int no_bwd16_narrow; // FOV_NO_BWD16_NARROW=1: widths 128 / 256 keep the 2- / 4- / 8-workgroup BPTT kernels at small batches
    int bwd16_groups32;  // FOV_BWD16_GROUPS=32: width-512 BPTT on thirty-two workgroups per tile up to eight tiles (default: sixteen)
    int no_stack2;       // FOV_NO_STACK2=1: two stacked width-512 layers as two launches (fov_lstm_stack2_supported -> 0)
    int no_wgrad_bf16_tiles;   // FOV_NO_WGRAD_BF16_TILES=1: the bf16 Conv2D weight gradient on its plain kernel (tests; conv_wgrad_bf16.hip)
    int no_stacked_decode;     // FOV_NO_STACKED_DECODE=1: fov_stacked_seq2seq_decode_supported -> 0, the stacked model's decode stays a host loop (tests / A-B timing)
    int no_selffed_fused;      // FOV_NO_SELFFED_FUSED=1: fov_selffed_decoder_supported -> 0, the self-fed decoder's unroll stays a host loop (tests / A-B timing)
    int no_selffed2_fused;     // FOV_NO_SELFFED2_FUSED=1: fov_selffed2_decoder_supported -> 0, the self-fed two-layer decoder's unroll stays a host loop (tests / A-B timing)
    int no_stacked_train;      // FOV_NO_STACKED_TRAIN=1: fov_stacked_seq2seq_train_supported -> 0, the stacked model trains and predicts layer by layer (tests / A-B timing)
};
const EnvKnobs& env_knobs();
void env_reload();
// Host-side epoch accounting of a workspace (xch_common.h): every exchange launch adds its span; long before the 32-bit
// tags could wrap, the header and the granule area are re-zeroed IN STREAM ORDER in front of the launch - whether or not
// the caller ever calls fov_check_status.
int xch_account(void* workspace, long span, hipStream_t stream);
void xch_forget(void* workspace);                        // the workspace was (re)initialised
void xch_note_force_safe(void* workspace, int on);
void xch_set_epoch_for_test(void* workspace, unsigned long long epoch);
int ensure_dynamic_lds(const void* kern, size_t lds, int block = 256);  // cached hipFuncSetAttribute(MaxDynamicSharedMemorySize) + occupancy check (>= 1 workgroup per CU)
void set_error(const char* fmt, ...);
// 31-bit byte offsets inside one buffer descriptor: B maps of batch stride ldb (and of ldb2 when there is a second input x2),
// weight_bytes of weights and, for the bf16 forms, `tiles` 16-row tiles.  false with the error "<what>: operand larger than
// 2 GiB" when one of them does not fit.
bool operand_fits_31bit(const char* what, int B, long ldb, const void* x2, long ldb2, long weight_bytes, long tiles = 0);
// after a launch: FOV_OK, or FOV_ERR_LAUNCH with the error "<what> launch: <hip string>"; under FOV_DBG_TRACE=1 the line
// "[fov trace] launched: <what>" first - every launch names its kernel form, so a test can assert the form a launcher chose
int launch_check(const char* what);
// FOV_OK when `need` bytes fit the 16-byte aligned workspace (need = 0: no workspace wanted), else FOV_ERR_WORKSPACE with its message
int check_ws(void* ws, size_t have, size_t need);
inline bool valid_act(int act) { return act == FOV_ACT_SIGMOID || act == FOV_ACT_HARD_SIGMOID; }
// one-workgroup-per-tile launches count their tiles in an int: batches and lengths beyond this are refused as arithmetic
constexpr int kMaxTileBatch = 1 << 30;
// kernels that index rows as 3 * b and frames as 3 * f in an int: the bounds their entry points refuse beyond
constexpr int kMaxFps = 1 << 20, kMaxRows3 = 1 << 29;
inline bool valid_impl(int impl) { return impl == FOV_IMPL_AUTO || impl == FOV_IMPL_GENERIC || impl == FOV_IMPL_CLUSTER; }
// wide-input layer, H = 256, 96 < F <= 256 (lstm_wide.hip)
bool wide_shape_ok(int F, int H);
bool wide_narrow_preferred(int B, int F, int H);
// width 512 on 32 workgroups per tile (lstm_wide16.hip): small batches (one tile per group), K in registers for F <= 96 or F = 512
bool wide16_shape(int B, int F, int H);
bool wide16_preferred(const float* x, int B, int F, int H);
int launch_wide16(const LstmParams& p, hipStream_t stream);
bool wide512_shape_ok(int F, int H, bool zx);   // width 512: 16 workgroups per tile; F <= 96 in-kernel, else precomputed x.K
int launch_wide(const LstmParams& p, hipStream_t stream);
// step-wise layer forward on the matrix-core GEMM (lstm_train.hip): hidden widths above the persistent kernels' 256
bool stepwise_preferred(int B, int F, int H);
size_t stepwise_workspace_floats(int B, int T, int H);
int launch_stepwise(const LstmParams& p, float* ws, size_t ws_floats, hipStream_t stream);

constexpr size_t kStatusBytes = 256;  // head of every workspace: status words (layout: xch_common.h)
// the status words and, behind them, the granule area of the exchanging kernels
inline void bind_workspace(LstmParams& p, void* workspace) {
    p.status = (unsigned*)workspace;
    p.xch = (unsigned long long*)((char*)workspace + kStatusBytes);
}

// ConvLSTM building blocks (conv_kernels.hip)
// dil: dilation of the taps over x (Keras dilation_rate; 'same' padding grows with it); the second segment of conv2d_fwd2 / the
// recurrent map of convlstm_cell_fwd is never dilated (Keras ConvLSTM2D dilates its input convolution only)
int conv2d_fwd(const float* x, long ldx, long ldb, const float* w, const float* bias, const float* add, float* y, int B, int H,
               int W, int C, int N, int kh, int kw, int act, hipStream_t stream, int dil = 1);
int conv2d_fwd2(const float* x, long ldx, long ldb, int C, const float* x2, long ldx2, long ldb2, int C2, const float* w,
                const float* bias, const float* add, float* y, int B, int H, int W, int N, int kh, int kw, int act,
                hipStream_t stream, int dil = 1);
int convlstm_gates(const float* z, float* c, float* h, long ldh, long rows, int F, int act, hipStream_t stream);
// LDS-resident-patch form of the ConvLSTM2D step (convlstm_patch.hip); convlstm_cell_fwd takes it when the shape allows
// 'same' Conv2D with the input map resident in LDS (conv_patch.hip): the wide layers of the ConvLSTM prediction head
bool conv_patch_shape_ok(const float* x, long ldx, long ldb, int B, int H, int W, int C, int N, int kh, int kw);
int launch_conv_patch(const float* x, long ldx, long ldb, const float* w, const float* bias, const float* add, float* y, int B, int H,
                      int W, int C, int N, int kh, int kw, int act, hipStream_t stream);
// the same convolution with bf16 matrix-core operands on weights packed once (conv_patch_bf16.hip): inference of the ConvLSTM head
size_t conv2d_bf16_packed_bytes(int C, int N, int kh, int kw);
int conv2d_pack_bf16(const float* w, void* packed, int C, int N, int kh, int kw, hipStream_t stream);
int conv2d_fwd_bf16(const float* x, long ldx, long ldb, const void* w_packed, const float* bias, float* y, int B, int H, int W, int C,
                    int N, int kh, int kw, int act, hipStream_t stream);
// one ConvLSTM2D step with bf16 matrix-core operands on weights packed once (convlstm_patch_bf16.hip): inference of the ConvLSTM cells
size_t convlstm_cell_bf16_packed_bytes(int Ctot, int F, int kh, int kw);
int convlstm_cell_pack_bf16(const float* w, void* packed, int Ctot, int F, int kh, int kw, hipStream_t stream);
int convlstm_cell_fwd_bf16(const float* x, long ldx, long ldb, int C, const float* h_prev, long ldx2, long ldb2, const void* w_packed,
                           const float* bias, const float* c_prev, float* c_new, float* h, long ldh, float* gates, int B, int H, int W,
                           int F, int kh, int kw, int act, hipStream_t stream);
bool cell_patch_shape_ok(const float* x, long ldx, long ldb, int C, const float* h_prev, long ldx2, long ldb2, int F, int H, int W,
                         int kh, int kw);
int launch_cell_patch(const float* x, long ldx, long ldb, int C, const float* h_prev, long ldx2, long ldb2, const float* w,
                      const float* bias, const float* c_prev, float* c_new, float* h, long ldh, float* gates, int B, int H, int W,
                      int F, int kh, int kw, int act, hipStream_t stream);
int convlstm_cell_fwd(const float* x, long ldx, long ldb, int C, const float* h_prev, long ldx2, long ldb2, const float* w,
                      const float* bias, const float* c_prev, float* c_new, float* h, long ldh, float* gates, int B, int H, int W,
                      int F, int kh, int kw, int act, hipStream_t stream, int dil = 1);
int softmax_lastdim(const float* x, float* y, long rows, int n, hipStream_t stream);

// ConvLSTM training (conv_train_kernels.hip)
bool conv_wgrad_lines_takes(int H, int W, int C, int N, int kh, int kw, int dil);      // conv_wgrad_lines.hip
int conv_wgrad_lines(const float* x, long ldx, const float* dz, float* dw, int B, int H, int W, int C, int N, int ks, int accumulate,
                     float* scratch, size_t scratch_floats, hipStream_t stream);
size_t conv2d_wgrad_workspace_floats(int C, int N, int kh, int kw);
int conv2d_wgrad(const float* x, long ldx, const float* dz, float* dw, int B, int H, int W, int C, int N, int kh, int kw,
                 int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream, int dil = 1);
// the same product with bf16 matrix-core operands (conv_wgrad_bf16.hip): dy rows ldy floats apart; scratch >= the workspace floats
size_t conv2d_wgrad_bf16_workspace_floats(int C, int N, int kh, int kw);
int conv2d_wgrad_bf16(const float* x, long ldx, const float* dy, long ldy, float* dw, int B, int H, int W, int C, int N, int kh, int kw,
                      int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream);
int convlstm_gates_train(const float* z, const float* c_prev, float* c_new, float* h, long ldh, float* gates, long rows, int F,
                         int act, hipStream_t stream);
int convlstm_gates_bwd(const float* dh, long lddh, float* dc, const float* gates, const float* c_prev, const float* c_new,
                       float* dz, long rows, int F, int act, hipStream_t stream);
int conv_weight_transpose(const float* w, float* wt, int kh, int kw, int C, int N, hipStream_t stream);
int softmax_lastdim_bwd(const float* dp, const float* p, float* dy, long rows, int n, hipStream_t stream);
int splitk_reduce(const float* part, float* out, long n, int S, int accumulate, hipStream_t stream);
// deferred split reductions of a training step (reduce_defer.hip): one reduce launch per step instead of one per product
int defer_begin(float* grad_base, size_t grad_floats, float* arena, size_t arena_floats, hipStream_t stream);
int defer_flush(const float* grad_base, hipStream_t stream);
int defer_end(const float* grad_base, hipStream_t stream);
int defer_touch(const float* out, size_t n, hipStream_t stream);
int zero_grad(float* g, size_t n, hipStream_t stream);
int zero_lstm_wgrads(float* dK, float* dR, float* db, int F, int H, hipStream_t stream);
float* defer_alloc(const float* out, size_t n, size_t floats, hipStream_t stream);
void defer_record(const float* part, float* out, long n, int S, int accumulate);
int reduce_or_defer(bool deferred, const float* part, float* out, long n, int S, int accumulate, hipStream_t stream, const char* what);
int colsum(const float* x, float* out, long rows, int cols, int accumulate, float* scratch, size_t scratch_floats,
           hipStream_t stream);

// fused decoder of the others-mixing model (mix_decoder.hip)
struct MixDecParams {
    const float *K1, *R1, *b1, *K2p, *R2, *b2, *Wd, *bd, *Wp;
    const float* oth_proj;   // others_t . W_oth + b_mix, element (b, t, o) at b*oth_sb + t*oth_st + o
    long oth_sb, oth_st;
    const float* dec0;       // (B,O)
    const float *h1_0, *c1_0, *h2_0, *c2_0;   // (B,H)
    float* out;              // (T_out,B,O) step-major: m_t
    float* P;                // TRAIN: (T_out,B,O)
    float *H1, *C1, *H2, *C2;   // TRAIN: (T_out,B,H), state after step t
    float *res1, *res2;      // TRAIN: (T_out,B,5,H) activated i,f,g,o and c of step t
    float *h1T, *c1T, *h2T, *c2T;   // final state (B,H), optional
    unsigned long long* xch; // granules: [group][layer 2][parity 2][16][256]
    unsigned* status;
    int B, T_out, O, num_groups, num_tiles;
    int epoch_span;          // epochs this launch may consume (xch_common.h)
};
// one-shot marks 'the packed K2 of this workspace is current' (api_state.hip)
void prepack_mark(void* workspace, const float* K2);
bool prepack_consume(void* workspace, const float* K2);
void prepack_forget(void* workspace);                    // the workspace was zero-filled: no packed copy in it any more
int mix_decoder_prepack(const float* K2, void* workspace, hipStream_t stream);
int mix_decoder_bwd_prepack(const float* K2, void* workspace, hipStream_t stream);
size_t mix_decoder_workspace_bytes(int B);
int mix_decoder_launch(MixDecParams p, const float* K2, int act, int train, void* workspace, hipStream_t stream);
int mix_decoder_bf16_launch(MixDecParams p, const float* K2, int act, int train, void* workspace, hipStream_t stream);   // mix_decoder_bf16.hip

// backward of the fused decoder (mix_decoder_bwd.hip)
struct MixDecBwdParams {
    const float *R1, *K1, *R2, *K2p, *Wd, *Wp;
    const float *M, *P, *dloss;      // (T_out,B,O): m_t, p_t, dL/d(pre-tanh of m_t) from the loss
    const float *res1, *res2;        // (T_out,B,5,H) reserves of the forward
    const float *C1, *C2;            // (T_out,B,H): cell state BEFORE step t (row 0 = the decoder's initial state)
    float *DZ1, *DZ2;                // (T_out,B,4H) out
    float *dpre_m, *dpre_p;          // (T_out,B,O) out
    float *dh1_0, *dc1_0, *dh2_0, *dc2_0;   // (B,H) out: gradient w.r.t. the decoder's initial state
    unsigned long long* xch;
    unsigned* status;
    int B, T_out, O, num_groups, num_tiles;
    int epoch_span;          // epochs this launch may consume (xch_common.h)
};
size_t mix_decoder_bwd_workspace_bytes(int B);
int mix_decoder_bwd_launch(MixDecBwdParams p, const float* K2, int act, void* workspace, hipStream_t stream);
int mix_decoder_bwd_bf16_launch(MixDecBwdParams p, const float* K2, int act, void* workspace, hipStream_t stream);   // mix_decoder_bwd_bf16.hip
// mix_tile.hip: the same decoder at H = 32 / 64 (the backward at H = 32), one workgroup per tile, no workspace; K2p = dec2_K as it is
bool mix_tile_shape_ok(int B, int T_out, int H, int O, bool backward);
int mix_tile_fwd_launch(const MixDecParams& p, int H, int act, hipStream_t stream);
int mix_tile_bwd_launch(const MixDecBwdParams& p, int act, hipStream_t stream);

// lstm_wide16.hip: two stacked width-512 layers as one launch (layer 2 a few steps behind layer 1 on other CUs)
bool wide16_pair_shape(int B, int T, int F, int H);
int launch_wide16_pair(const LstmParams& a, const LstmParams& b, hipStream_t stream);

// A layer's BPTT as plain aggregates: the entry points fill them once, lstm_train.hip plans and runs them.
// The recurrence's operands: the ten fields every BPTT kernel's own parameter struct starts with (set_rec copies them over)
struct BwdRec {
    const float *R, *reserve, *c0, *dhs, *dhT, *dcT;   // (H,4H), (B,T,5,H), then (B,H) / (B,T,H) / (B,H) / (B,H) or NULL
    float *dz, *dh0, *dc0, *db_part;                   // (B,T,4H), (B,H), (B,H), per-tile bias partials (tiles,4H) or NULL
};
template <class KernelParams>
inline void set_rec(KernelParams& p, const BwdRec& r) {
    p.R = r.R; p.reserve = r.reserve; p.c0 = r.c0; p.dhs = r.dhs; p.dhT = r.dhT; p.dcT = r.dcT; p.dz = r.dz; p.dh0 = r.dh0; p.dc0 = r.dc0; p.db_part = r.db_part;
}
// A layer's weight-gradient problem: dK (F,4H) = x^T dz, dR (H,4H) = h_{t-1}^T dz (h_{-1} = h0 or 0), db (4H) = colsum(dz);
// any of dK / dR / db may be NULL
struct LayerWgrad {
    const float *x, *hs, *h0, *dz;                     // (B,T,F), (B,T,H), (B,H) or NULL, (B,T,4H)
    float *dK, *dR, *db;
    int F, T;
};
// A layer's whole backward; rec.dz and wg.dz are the same tape, rec.db_part belongs to lstm_seq_bwd
struct LstmBwdLayer {
    BwdRec rec;
    LayerWgrad wg;
    const float* K;                                    // (F,4H)
    float* dx;                                         // (B,T,F) or NULL
    int B, T, F, H, act, accumulate, bf16;
};

// The persistent BPTT recurrences; the status word and the granule buffers live at `xch_ws` (kStatusBytes + kXchBytes)
// lstm_bwd16.hip: 16 / 32 units per workgroup (fp32): width 512, and 128 / 256 at small batches
bool bwd16_takes(int B, int H);
int launch_bwd16(const BwdRec& r, int B, int T, int H, int act, void* xch_ws, hipStream_t stream);
// ... two stacked width-512 layers as one launch: `low` takes its dhs from `up` through K2 inside the kernel (low.dhs is not read)
bool bwd16_pair_shape(int B, int T, int H);
int launch_bwd16_pair(const BwdRec& up, const BwdRec& low, const float* K2, int B, int T, int act, void* xch_ws, hipStream_t stream);
// lstm_stacked_train.hip: the same two-layer contract at H = 32 / 64, one workgroup per 16-sequence tile, any batch, no workspace;
// up's dx reaches low through low.dz itself
bool stack2_tile_bwd_width(int H);
int launch_stack2_tile_bwd(const BwdRec& up, const BwdRec& low, const float* K2, int B, int T, int H, int act, hipStream_t stream);
// lstm_bwd8.hip: groups of eight workgroups (H = 256), fp32 or bf16 operands; K_dx and dx: dx = dz K^T inside the kernel
// (fp32: dx = eight partial tapes [slice][B][T][256])
bool bwd8_preferred(int B, int H);
int launch_bwd8(const BwdRec& r, int B, int T, int act, int bf16, void* xch_ws, hipStream_t stream, const float* K_dx = nullptr,
                float* dx = nullptr);
// lstm_bwd_cluster.hip: groups of H / 64 workgroups
bool bwd_cluster_shape_ok(int H);
size_t bwd_cluster_xch_bytes(int B, int H);
int launch_bwd_cluster(const BwdRec& r, int B, int T, int H, int act, void* xch_ws, hipStream_t stream);

// wgrad_group.hip: the weight gradients of up to four layers that share the batch and the width, in one launch
bool wgrad_rows_takes(long rows, int H);       // few rows AND narrow layers - 16 x 64 tiles, rows split over a workgroup's waves
int wgrad_rows_layers(int L, const LayerWgrad* layers, int B, int H, int accumulate, hipStream_t stream);
bool wgrad_group_takes(int B, int T, int H);   // few rows - every (product, output tile) one workgroup; the layers share T too
int wgrad_group_layers(int L, const LayerWgrad* layers, int B, int H, int accumulate, hipStream_t stream);

// fp32 matrix-core GEMM (gemm_f32.hip; the strided forms: gemm_f32.h)
int matmul_f32(const float* a, const float* b, float* c, int M, int K, int N, float* scratch, size_t scratch_floats,
               hipStream_t stream);

// a layer's training step: BPTT dispatch, weight-gradient products, Dense backward (lstm_train.hip)
size_t lstm_bwd_workspace_floats(int B, int T, int F, int H);
int lstm_seq_bwd(const LstmBwdLayer& layer, float* ws, size_t ws_floats, hipStream_t stream);
// two stacked width-512 layers, both recurrences in one launch (bwd16_pair_shape): low.rec.dhs and up.dx are not used, the
// upper layer's dx reaches the lower one inside the kernel
size_t lstm_stack2_bwd_workspace_floats(int B, int T, int F, int H);
int lstm_stack2_bwd(const LstmBwdLayer& low, const LstmBwdLayer& up, float* ws, size_t ws_floats, hipStream_t stream);
int lstm_seq_wgrad(const LayerWgrad& layer, int B, int H, int accumulate, int bf16, float* scratch, size_t scratch_floats, hipStream_t stream);
// all weight gradients of up to four layers that share the batch and the width (a stack, an encoder / decoder pair): one launch
// where the few-row form takes every layer, else one lstm_seq_wgrad per layer - the same bits either way
constexpr int kMaxWgradLayers = 4;
bool lstm_seq_wgrad_pair_one_launch(int B, int T1, int T2, int H);
int lstm_seq_wgrad_layers(int L, const LayerWgrad* layers, int B, int H, int accumulate, float* scratch, size_t scratch_floats,
                          hipStream_t stream);
size_t mix_head_wgrad_scratch_floats(int B, int T, int H, int O, int n_oth);
int mix_head_wgrad(const float* h2, const float* dpre_p, const float* others, const float* p, const float* dpre_m, float* out, int B,
                   int T, int H, int O, int n_oth, int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream);
bool wgrad_fusable(const float* a1, long lda1, long a1_so, int M1, const float* a2, long lda2, long a2_so, int M2, const float* b,
                   long ldb, long b_so, const float* c, int N);
int wgrad_fused(const float* a1, long lda1, long a1_so, int M1, int shift1, const float* a2, long lda2, long a2_so, int M2, int shift2,
                const float* b, long ldb, long b_so, float* c, int N, int RO, int RI, int bias_row, int accumulate, int bf16,
                float* scratch, size_t scratch_floats, hipStream_t stream);
int dense_bwd(const float* x, const float* W, const float* dpre, float* dx, float* dW, float* db, int N, int In, int Out,
              int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream, int bf16 = 0);

// losses, pointwise kernels and optimizers (loss_optim_kernels.hip)
int mse_dense_grad(const float* y, const float* target, float* dpre, float* loss, long n, int activation, float* scratch,
                   size_t scratch_floats, hipStream_t stream);
bool dense_mse_head_shape_ok(long N, int H, int O);
size_t dense_mse_head_scratch_floats(long N, int H, int O);
int dense_mse_head(const float* hs, const float* W, const float* b, const float* target, float* y, float* dX, float* dW, float* db,
                   float* loss, long N, int H, int O, int activation, float weight, float* scratch, size_t scratch_floats, hipStream_t stream);
int mse_dense_grad_w(const float* y, const float* target, float* dpre, float* loss, long n, int activation, float weight,
                     int tmB, int tmT, int O, float* scratch, size_t scratch_floats, hipStream_t stream, float* db = nullptr, int dbO = 0);
int scale_inplace(float* x, long n, float s, hipStream_t stream);
int act_bwd(const float* dy, const float* y, const float* base, float* out, long n, int activation, hipStream_t stream);
int adam_step(float* p, const float* g, float* m, float* v, long n, float lr_t, float b1, float b2, float eps,
              const unsigned* const* guards, long long* applied, hipStream_t stream);   // guards: NULL or three (nullable) timeout words; applied: nullable counter of updates that ran
int rmsprop_step(float* p, const float* g, float* a, long n, float lr, float rho, float eps, const unsigned* const* guards,
                 long long* applied, hipStream_t stream);
int guard_flag(const unsigned* const* guards, float* out, hipStream_t stream);
int act_fwd(const float* x, float* y, long n, int activation, hipStream_t stream);
int gauss_nll_grad(const float* mu, const float* var, const float* y, float* loss, float* dmu, float* dvar, int B, int Ty,
                   int fps, float scale, float* scratch, size_t scratch_floats, hipStream_t stream);
int rmsprop_tf_step(float* p, const float* g, float* ms, long n, float lr, float decay, float eps, float clip,
                    const unsigned* const* guards, long long* applied, hipStream_t stream);
int cce_grad(const float* p, const float* t, float* dp, float* loss, long n_pix, int C, float* scratch, size_t scratch_floats,
             hipStream_t stream);
int xyz_sum1_grad(const float* p, float* dp, float* reg, long n_pix, int C, float* scratch, size_t scratch_floats, hipStream_t stream);
int sample_refeed_fwd(const float* mu, const float* var, const float* noise, float* x, long ldx, int B, int fps, int std_mode,
                      int layout, hipStream_t stream);
int sample_refeed_bwd(const float* dx, long ldx, const float* var, const float* noise, float* dmu, float* dvar, int B, int fps,
                      int std_mode, int layout, int accumulate, hipStream_t stream);

}  // namespace fov
