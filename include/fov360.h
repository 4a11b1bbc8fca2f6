/*
 * fov360.h - C ABI of the MI355X-native seq2seq-LSTM hot path (libfov360_hip.so).
 *
 * Drop-in boundary for the path BASELINE.json:north_star names in ChengeLi/LongTerm360FoV:
 * the reference has no native code; every entry point below replaces a Keras/TensorFlow
 * layer call made by the reference's model scripts (file:line cited per function, relative to
 * /root/reference/).  A maintainer of the reference binds these with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / HIP types in the signatures
 *     (fov_stream_t is an opaque hipStream_t; NULL = the default stream).
 *   - All tensors are DEVICE pointers, row-major contiguous fp32.  The caller owns every
 *     buffer; the library allocates NO DEVICE MEMORY.  Scratch comes from a caller-provided
 *     workspace whose size is queried first (fov_*_workspace_bytes).
 *   - Weights use the Keras layout so weight files round-trip:
 *       kernel K:(F,4H), recurrent_kernel R:(H,4H), bias b:(4H); gate column blocks i,f,c,o.
 *   - A workspace handed to a persistent-kernel entry point (every call that takes `workspace` and whose
 *     fov_*_workspace_bytes is larger than a few KB) is STATEFUL: zero-fill it ONCE after allocating it
 *     (fov_workspace_init, or hipMemset) and then leave its contents alone between calls.  It carries a
 *     256-byte header and a 64 MB granule area whose {value, epoch} words use epoch tags that increase
 *     monotonically across calls, so no call has to clear anything (csrc/xch_common.h).  One workspace
 *     serves one stream at a time; different entry points may share it.  The header's timeout word is
 *     sticky: once a bounded in-kernel wait has given up, every later call on that workspace returns
 *     without computing until fov_check_status has reported (and cleared) the failure.
 *   - Weight gradients over an empty batch or sequence (B = 0, T = 0, no rows): accumulate = 0 writes zeros
 *     (the gradient of an empty sum), accumulate != 0 leaves the output unchanged.  Every weight-gradient entry
 *     point keeps this rule (a data-parallel rank with an empty shard contributes zero, not a stale gradient).
 *   - Arguments are checked on the host: the refusals this header names - a NULL required pointer, a size, stride or
 *     enumeration out of range, an unsupported shape, a short workspace - come before the call's first HIP call, so
 *     such a call has enqueued and written nothing.  (An entry point made of several launches can still fail in a
 *     later one - a kernel attribute the runtime refuses, an inner product's own limit - after the earlier ones were
 *     enqueued; fov_seq2seq_tf_fwd names its case.)  A required pointer that is
 *     NULL, a negative size, a negative stride or a value outside an enumeration (act, impl, activation, ...) is
 *     FOV_ERR_INVALID; a width of zero is refused, an empty batch / sequence / row count is FOV_OK (a weight-gradient
 *     entry point still zeroes its outputs, see above).  A workspace that is NULL or smaller than its size function
 *     answers is FOV_ERR_WORKSPACE, and so is one whose base is not 16-byte aligned.
 *   - The persistent kernels tag every step with a 32-bit epoch and count a launch's span of them in an int.
 *     fov_lstm_seq_fwd (_train, _zx, _bf16), fov_lstm_seq_bwd(_bf16), fov_seq2seq_decode_fwd (_packed, _bf16),
 *     fov_seq2seq_decoder_fwd, fov_seq2seq_tf_fwd and fov_mix_decoder_fwd / _bwd (_bf16) therefore refuse, whichever
 *     kernel the call would reach, (steps + 2) * ceil(B / 8) > 2^30 (steps = T, T_out, or T_in + T_out of the fused
 *     calls; the longer of the two for fov_seq2seq_tf_fwd): FOV_ERR_UNSUPPORTED.  (The fov_lstm_stack2_* calls are
 *     bounded by their granule area, see their predicates; the fov_lstm_seq_wgrad* calls exchange nothing.)
 *   - Every function returns FOV_OK (0) or a negative FOV_ERR_*; fov_last_error() gives the
 *     message of the calling thread's last failure.  No host synchronisation inside a call
 *     (except fov_check_status, which is the explicit "did the persistent kernel finish
 *     cleanly" query).
 *   - Threading and state.  One stream per call; calls from different threads are safe as long as they do not
 *     share a workspace / scratch / gradient buffer (those are single-owner: one stream at a time).  What the
 *     library keeps between calls, all of it on the HOST, all of it behind mutexes and keyed so that callers do
 *     not meet:
 *       * a thread-local error string (fov_last_error);
 *       * read-only caches filled on first use: device properties per device, and the FOV_* environment knobs
 *         (diagnostic switches between kernel forms; read once, re-read by fov_reload_env);
 *       * per WORKSPACE POINTER: the host copy of the workspace's epoch counter / exchange mode and the address
 *         of a weight matrix a caller pre-packed into it (fov_workspace_init forgets both; call it again when a
 *         workspace's memory is freed and the address comes back from the allocator);
 *       * per open fov_reduce_defer_begin region, keyed by its gradient buffer: the table of pending reductions
 *         (see there);
 *       * per (device, stream): the index of that stream's word in a 1024-word device-side ticket table of the
 *         loss entry points (a module-level __device__ array, not an allocation).  A device on which more than
 *         1024 distinct streams have issued loss calls takes the two-launch form for the later ones
 *         (fov_dense_mse_head refuses there);
 *       * streams exist only where the caller asked for one (fov_stream_create) and belong to the caller.
 *     One process per GPU - the deployment this library is written for - and several devices / trainers /
 *     threads in one process are both within this contract (tests/test_gpu_threads.py drives two trainers
 *     from two threads on two streams against the serial result).
 */
#ifndef FOV360_H
#define FOV360_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fov_stream_t; /* hipStream_t */

/* recurrent_activation of keras.layers.LSTM.  Keras < 2.3 (the reference's era) defaults to
 * hard_sigmoid = clip(0.2x+0.5,0,1); BASELINE.json:north_star names sigmoid. */
enum { FOV_ACT_SIGMOID = 0, FOV_ACT_HARD_SIGMOID = 1 };

/* kernel family selection; any other value of `impl` is FOV_ERR_INVALID */
enum {
    FOV_IMPL_AUTO = 0,    /* cluster kernel when the shape is supported, else generic        */
    FOV_IMPL_GENERIC = 1, /* one workgroup per 4 sequences, weights streamed from L2; any H,F */
    FOV_IMPL_CLUSTER = 2  /* persistent MFMA kernel: H/64 workgroups per 16-sequence tile,
                             recurrent weights resident in registers, h exchanged per step   */
};

enum {
    FOV_OK = 0,
    FOV_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, ...)              */
    FOV_ERR_UNSUPPORTED = -2, /* shape not supported by the requested implementation          */
    FOV_ERR_WORKSPACE = -3,   /* workspace missing or too small                               */
    FOV_ERR_LAUNCH = -4,      /* HIP runtime error (message in fov_last_error)                */
    FOV_ERR_TIMEOUT = -5      /* a bounded in-kernel wait gave up (fov_check_status)          */
};

const char* fov_last_error(void);
int fov_version(void);

/* 1 if FOV_IMPL_CLUSTER supports (F,H) for a layer / (F_enc,F_dec,H) for the fused decode. */
int fov_cluster_supported(int F, int H);

/* ---------------------------------------------------------------------------------------
 * keras.layers.LSTM(H, return_sequences=True, return_state=True)(x, initial_state=[h0,c0])
 *   replaces: mycode/FoV_seq2seq.py:83-86 (encoder), :93-95 (teacher-forced decoder),
 *             mycode/given_others_gt_mean_var_seq2seq.py:108-112.
 *   x:(B,T,F)  h0,c0:(B,H) or NULL (= zeros)  hs:(B,T,H) or NULL  hT,cT:(B,H) or NULL
 *   B = 0: nothing is launched; T = 0: hT, cT receive the initial state.
 * ------------------------------------------------------------------------------------- */
size_t fov_lstm_seq_workspace_bytes(int B, int T, int F, int H, int impl);
int fov_lstm_seq_fwd(const float* x, const float* K, const float* R, const float* b,
                     const float* h0, const float* c0, float* hs, float* hT, float* cT,
                     int B, int T, int F, int H, int act, int impl,
                     void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * keras.layers.Dense(Out, activation)(x)   y = act(x W + b), W:(In,Out)
 *   replaces: mycode/FoV_seq2seq.py:96-97; given_others...py:127-130,168.
 *   activation: 0 = linear, 1 = tanh.   x:(N,In)  y:(N,Out); b may be NULL (no bias).
 *   In, Out <= 2^24 (also for fov_dense_add_fwd), else FOV_ERR_INVALID.
 * ------------------------------------------------------------------------------------- */
int fov_dense_fwd(const float* x, const float* W, const float* b, float* y,
                  int N, int In, int Out, int activation, fov_stream_t stream);

/* y = act(x W + b + add[row*add_row_stride + :]) - Dense with an additive per-row term, used to fold the
 * precomputed "others" part of the mixing layer into the decoder step:
 *   replaces: Concatenate(axis=1)([others_t, pred]) -> Flatten -> Dense(6,'tanh')
 *             (mycode/given_others_gt_mean_var_seq2seq.py:257-265), with W = mix_W[-6:], add = others_t . mix_W[:-6].
 * add_row_stride >= 0 floats (0 broadcasts one row); b may be NULL. */
int fov_dense_add_fwd(const float* x, const float* W, const float* b, const float* add, int64_t add_row_stride,
                      float* y, int N, int In, int Out, int activation, fov_stream_t stream);

/* One decoder step of the others-mixing head in ONE launch (given_others...py:127-130,168,257-265):
 *   p (N,O) = tanh(h dense_W + dense_b);   m (N,O) = tanh(p mix_Wp + add[row*add_row_stride + :])
 * with mix_Wp = mix_W[-O:] (O x O) and add = others_t . mix_W[:-O] + mix_b (fov_dense_fwd, hoisted out of the loop).
 * O <= 8, H % 4 == 0, H <= 2048, h 16-byte aligned, add_row_stride >= 0 (the forward; anything else is FOV_ERR_INVALID).
 * Backward of the same step: dm_loss = dL/d(pre-tanh of m) from the loss, dm_feedback =
 * dL/dm arriving through x_{t+1} = m_t (NULL at the last step); writes dpre_m, dpre_p (N,O: the pre-activation
 * gradients the weight-gradient products need) and dh (N,H) = dL/dh.  Outputs must not alias inputs. */
int fov_mix_head_fwd(const float* h, const float* dense_W, const float* dense_b, const float* mix_Wp, const float* add,
                     int64_t add_row_stride, float* p, float* m, int N, int H, int O, fov_stream_t stream);
int fov_mix_head_bwd(const float* dm_loss, const float* dm_feedback, const float* m, const float* p, const float* mix_Wp,
                     const float* dense_W, float* dpre_m, float* dpre_p, float* dh, int N, int H, int O,
                     fov_stream_t stream);

/* Weight gradients of that head over ALL steps of the unrolled decoder in one launch + one reduce (what Keras/TF
 * autodiff forms as six separate reductions, given_others...py:308): with rows r = (t, b),
 *     [dense_W ; dense_b] = [h2_t | 1]^T dpre_p,      [mix_W ; mix_b] = [others_t | p_t | 1]^T dpre_m
 * written into out as one (H + 1 + n_others + O + 1, O) block - dense_W, dense_b, mix_W (others' rows, then the
 * prediction's), mix_b as they lie adjacent in a flat gradient buffer.  h2 (T_out*B, H), dpre_p, p, dpre_m (T_out*B, O)
 * time-major; others (B, T_out, n_others) batch-major as the model receives it (no transposed copy).  O <= 8. */
size_t fov_mix_head_wgrad_workspace_bytes(int B, int T_out, int H, int O, int n_others);
int fov_mix_head_wgrad(const float* h2, const float* dpre_p, const float* others, const float* p, const float* dpre_m,
                       float* out, int B, int T_out, int H, int O, int n_others, int accumulate,
                       void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The whole unrolled no-teacher-forcing decoder of the others-mixing model in ONE persistent launch
 * (given_others...py:203-299): per step LSTM1(x_t) -> LSTM2 -> Dense(O,'tanh') -> mixing Dense -> x_{t+1}.
 *   dec0 (B,O); h1,c1,h2,c2 (B,H) = encoder states; oth_proj: others_t . mix_W[:-O] + mix_b, element (b,t,o) at
 *   b*oth_batch_stride + t*oth_step_stride + o; weights in Keras layout; mix_Wp = mix_W[-O:] (O,O).
 *   (both strides >= 0).  out (T_out,B,O) step-major = m_t.  h1T..c2T (B,H): final states or NULL.
 *   Training buffers (all or none): P (T_out,B,O) = p_t; H1,C1,H2,C2 (T_out,B,H) = states after step t;
 *   res1,res2 (T_out,B,5,H) = activated i,f,g,o and c (the reserve layout of fov_lstm_seq_fwd_train with T = 1).
 * Supported: O <= 8 and H = 256, 32 or 64 (FOV_ERR_UNSUPPORTED otherwise: use the per-step entry points).
 *   H = 256       the persistent kernel, eight workgroups per 16-sequence tile exchanging h through the workspace.
 *   H = 32 or 64  the script's own latent_dim (given_others...py:38) and twice it: ONE workgroup owns a tile for both layers and
 *                 every step (the ownership of fov_selffed2_decoder_fwd): no exchange, nothing to wait on, and NO workspace -
 *                 `workspace` may be NULL and workspace_bytes is not looked at (fov_mix_decoder_workspace_bytes answers the
 *                 status header's size there).  fp32 only: fov_mix_decoder_fwd_bf16 / _bwd_bf16 stay H = 256.  The backward
 *                 has H = 32 alone (at 64 its three transposed matrices would take 192 KB of LDS): fov_mix_decoder_bwd at
 *                 H = 64 is FOV_ERR_UNSUPPORTED and the caller walks the forward's tapes with the per-step entry points.
 * The argument checks, their order and the B = 0 / T_out = 0 behaviour (FOV_OK, nothing launched, nothing written) are the
 * same at every width.  fov_mix_decoder_tile_supported(B, T_out, H, O, backward) is the rule of the H = 32 / 64 kernels as
 * arithmetic (no device query): 1 where fov_mix_decoder_fwd (backward = 0) / fov_mix_decoder_bwd (backward != 0) would run the
 * one-workgroup-per-tile kernel - H = 32, or 64 for the forward, 1 <= O <= 8, 0 <= B, T_out <= 2^30 and (T_out + 2) * ceil(B / 8)
 * <= 2^30, the bound of every LSTM entry point - and 0 for every other shape, H = 256 included. */
size_t fov_mix_decoder_workspace_bytes(int B, int H);
int fov_mix_decoder_tile_supported(int B, int T_out, int H, int O, int backward);
int fov_mix_decoder_fwd(const float* dec0, const float* h1, const float* c1, const float* h2, const float* c2,
                        const float* oth_proj, int64_t oth_batch_stride, int64_t oth_step_stride,
                        const float* dec1_K, const float* dec1_R, const float* dec1_b,
                        const float* dec2_K, const float* dec2_R, const float* dec2_b,
                        const float* dense_W, const float* dense_b, const float* mix_Wp,
                        float* out, float* h1T, float* c1T, float* h2T, float* c2T,
                        float* P, float* H1, float* C1, float* H2, float* C2, float* res1, float* res2,
                        int B, int T_out, int H, int O, int act,
                        void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* =======================================================================================
 * bf16 forms (BASELINE.json configs[4]): the SAME fp32 tensors in and out, but every product with x or h on its left
 * (gate GEMMs, the Dense(6) head of the fused decoder) takes bf16 operands - round-to-nearest-even of the fp32 values,
 * made on the fly - into v_mfma_f32_16x16x32_bf16 with fp32 accumulation; gates, cell state, mixing layer, tapes and
 * the master weights stay fp32.  H = 256 (F <= 256 for the layer).  Outputs differ from the fp32 entry points by the
 * operand rounding: ~1e-2 absolute on tanh-range outputs after 20 recurrent steps (bound stated in the tests).
 * ======================================================================================= */
int fov_mix_decoder_fwd_bf16(const float* dec0, const float* h1, const float* c1, const float* h2, const float* c2,
                             const float* oth_proj, int64_t oth_batch_stride, int64_t oth_step_stride,
                             const float* dec1_K, const float* dec1_R, const float* dec1_b,
                             const float* dec2_K, const float* dec2_R, const float* dec2_b,
                             const float* dense_W, const float* dense_b, const float* mix_Wp, float* out,
                             float* h1T, float* c1T, float* h2T, float* c2T,
                             float* P, float* H1, float* C1, float* H2, float* C2, float* res1, float* res2,
                             int B, int T_out, int H, int O, int act,
                             void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* fov_mix_decoder_bwd with bf16 operands in its FOUR transposed products: the recurrences dz2 R2^T -> dh2_{t-1} and
 * dz1 R1^T -> dh1_{t-1}, and the data products dz2 K2^T -> dh1_t and dz1 K1^T -> dx_t (the feedback gradient into the previous
 * step's mixing output).  The mixing head's backward (dpre_m mix_Wp^T, dpre_p dense_W^T), gates backward, dc and every output
 * (DZ1, DZ2 unrounded) stay fp32. */
int fov_mix_decoder_bwd_bf16(const float* M, const float* P, const float* dloss, const float* res1, const float* res2,
                             const float* C1, const float* C2,
                             const float* dec1_K, const float* dec1_R, const float* dec2_K, const float* dec2_R,
                             const float* dense_W, const float* mix_Wp,
                             float* DZ1, float* DZ2, float* dpre_m, float* dpre_p,
                             float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0,
                             int B, int T_out, int H, int O, int act,
                             void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* fov_lstm_seq_bwd / fov_dense_bwd with bf16 operands (round-to-nearest-even on the fly, fp32 accumulation); gates backward,
 * dz (stored unrounded), dc and db (the column sums of the unrounded dz) stay fp32.  Same arguments, same workspaces.
 * fov_lstm_seq_bwd_bf16, per product:
 *   - recurrence dh_{t-1} = dz_t R^T: always bf16 (eight-workgroup BPTT kernel); R must be 16-byte aligned (else FOV_ERR_INVALID);
 *   - data gradient dx = dz K^T: bf16 when K is 16-byte aligned - inside the BPTT kernel when F == 256 and FOV_NO_DX_FUSION is
 *     unset, else the bf16 NT product; fp32 when K is not aligned (a view at a 4-, 8- or 12-byte offset of a flat buffer);
 *   - weight products x^T dz and h_{t-1}^T dz (h0^T dz_0 included): bf16, except dK = x^T dz for F <= 8 over >= 1024 rows
 *     (the fp32 skinny product).
 * fov_dense_bwd_bf16: dW = x^T dpre is bf16 only when Out >= 64, Out % 4 == 0 and dpre is 16-byte aligned (the K / R gradients
 * of an unrolled decoder), fp32 otherwise; dx = dpre W^T and db are always fp32. */
int fov_lstm_seq_bwd_bf16(const float* x, const float* K, const float* R, const float* h0, const float* c0,
                          const float* hs, const float* reserve, const float* dhs, const float* dhT, const float* dcT,
                          float* dz, float* dx, float* dK, float* dR, float* db, float* dh0, float* dc0,
                          int B, int T, int F, int H, int act, int accumulate,
                          void* workspace, size_t workspace_bytes, fov_stream_t stream);
int fov_dense_bwd_bf16(const float* x, const float* W, const float* dpre, float* dx, float* dW, float* db,
                       int N, int In, int Out, int accumulate,
                       void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* BPTT of two stacked LSTM layers in ONE launch, then the two layers' weight gradients.  Arguments are those of two
 * fov_lstm_seq_bwd calls (upper layer first, its dx as the lower layer's dhs): layer 1 = lower (input x (B,T,F), tape hs1,
 * reserve1), layer 2 = upper (input hs1, tape hs2, reserve2); h0_* / c0_* (B,H) or NULL (zero initial states);
 * dhs2 (B,T,H) / dhT2 / dcT2 / dhT1 / dcT1 optional upstream gradients;
 * dz1, dz2 (B,T,4H) out; dK / dR / db of either layer optional (NULL: data path only); dh0 / dc0 optional.  The gradient with
 * respect to x is NOT produced.  Two forms, chosen by the width, which is decided first and as arithmetic: H = 32, 64 or 512,
 * anything else is FOV_ERR_UNSUPPORTED whatever B and T are.
 *   H = 512 (fov_lstm_stack2_fwd's layers, mycode/lstm.py:218-240 under the train_op of :556-567): one persistent launch in which
 *     the upper layer's recurrence, the data-gradient product dx = dz2 . K2^T and the lower layer's recurrence run as three roles
 *     on disjoint CUs, the lower layer about a step behind the upper one; at most 32 sequences on 256 CUs.  Results equal the
 *     two-call path's up to the summation order of dx (sixteen partial sums added in slice order instead of a split GEMM's
 *     reduce).  The workspace is stateful like every exchange workspace (zero-filled once).
 *   H = 32 / 64 (the encoder of given_others_gt_mean_var_seq2seq.py at its own latent_dim): one workgroup per tile of 16 sequences
 *     walks the upper layer, then the lower one; any batch (up to 2^30 sequences) and any T.  dx reaches the lower layer through dz1
 *     itself (the first H floats of every step, overwritten by dz1 afterwards): no exchange, nothing to wait for.  The workspace
 *     is plain scratch for the weight-gradient products; its header is neither read nor written.  dK / dR / db are what
 *     fov_lstm_seq_wgrad_layers gives on dz1 and dz2, bit for bit.
 * Shapes: fov_lstm_stack2_bwd_supported (1 at H = 32 / 64 for B, T, F >= 1).  An empty call (B = 0 or T = 0) of a width that is
 * taken zeroes the weight gradients (accumulate = 0) and, at T = 0, passes dhT / dcT through to dh0 / dc0 - although the
 * predicate answers 0 for it (there is nothing to fuse).  workspace: fov_lstm_stack2_bwd_workspace_bytes. */
int fov_lstm_stack2_bwd_supported(int B, int T, int F, int H);
size_t fov_lstm_stack2_bwd_workspace_bytes(int B, int T, int F, int H);
int fov_lstm_stack2_bwd(const float* x, const float* R1, const float* K2, const float* R2,
                        const float* h0_1, const float* c0_1, const float* h0_2, const float* c0_2,
                        const float* hs1, const float* reserve1, const float* hs2, const float* reserve2,
                        const float* dhs2, const float* dhT2, const float* dcT2, const float* dhT1, const float* dcT1,
                        float* dz1, float* dz2, float* dK1, float* dR1, float* db1, float* dK2, float* dR2, float* db2,
                        float* dh0_1, float* dc0_1, float* dh0_2, float* dc0_2,
                        int B, int T, int F, int H, int act, int accumulate,
                        void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The weight-gradient half of fov_lstm_seq_bwd[_bf16] on its own: dK (F,4H) = x^T dz, dR (H,4H) = h_{t-1}^T dz (h_{-1} = h0, or
 * zero when h0 is NULL), db (4H) = column sums of dz, from the dz tape (B,T,4H) a call with dK = dR = db = NULL left behind.  Same
 * products in the same order (one fused product when dK, dR, db lie adjacent), so the results equal the single call's bit for bit.
 * It exists so that a trainer can enqueue a layer's products on ANOTHER stream, under the next layer's latency-bound recurrence
 * (Keras computes the same gradients inside `model.fit`, given_others_gt_mean_var_seq2seq.py:494-506).  Any of dK / dR / db may be
 * NULL.  bf16 != 0: operands rounded to bf16 (H = 256).  workspace: fov_lstm_seq_bwd_workspace_bytes(B, T, F, H) bytes of plain
 * scratch - NOT the workspace a concurrently running fov_lstm_seq_bwd uses. */
int fov_lstm_seq_wgrad(const float* x, const float* hs, const float* h0, const float* dz, float* dK, float* dR, float* db,
                       int B, int T, int F, int H, int accumulate, int bf16,
                       void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The same for an encoder / decoder pair of layers that share the batch (FoV_seq2seq.py:68-93: layer 1 = encoder over T1 steps,
 * layer 2 = decoder over T2 steps, h0_2 = the encoder's final h): all six gradients from the two dz tapes.  When
 * fov_lstm_seq_wgrad_pair_one_launch(B, T1, T2, H) is 1 (few rows, H <= 256: the reference's batch of 32) they are ONE launch
 * without split products or reduces - a trainer then runs both BPTT calls with dK = dR = db = NULL and calls this once; otherwise
 * the call equals two fov_lstm_seq_wgrad calls.  workspace: max over the two layers of fov_lstm_seq_bwd_workspace_bytes. */
int fov_lstm_seq_wgrad_pair_one_launch(int B, int T1, int T2, int H);
int fov_lstm_seq_wgrad_pair(const float* x1, const float* hs1, const float* h0_1, const float* dz1, float* dK1, float* dR1, float* db1,
                            int T1, int F1,
                            const float* x2, const float* hs2, const float* h0_2, const float* dz2, float* dK2, float* dR2, float* db2,
                            int T2, int F2,
                            int B, int H, int accumulate,
                            void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The same for the layers of a STACK (Fov_seq2seq_2layers.py:232-272,332-343: the encoder stack or the decoder stack under
 * model.fit): 1 <= L <= 4 layers that share the batch and the width, arrays of L entries - x[l] (B,T[l],F[l]), hs[l] (B,T[l],H),
 * h0[l] (B,H) or NULL, dz[l] (B,T[l],4H) -> dK[l] (F[l],4H), dR[l] (H,4H), db[l] (4H), any of which may be NULL.  Where the
 * few-row form takes every layer (B T[l] <= 640 rows, H <= 512 a multiple of 16, 16-byte aligned dz and gradients) all of them are
 * ONE launch; otherwise the call makes one fov_lstm_seq_wgrad-equivalent call per layer.  Either way the results equal the
 * per-layer calls' bit for bit.  Another L: FOV_ERR_UNSUPPORTED.  workspace: max over the layers of
 * fov_lstm_seq_bwd_workspace_bytes(B, T[l], F[l], H). */
int fov_lstm_seq_wgrad_layers(int L, const float* const* x, const int* F, const int* T, const float* const* hs,
                              const float* const* h0, const float* const* dz,
                              float* const* dK, float* const* dR, float* const* db,
                              int B, int H, int accumulate,
                              void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* A HIP stream of a given priority for such side work: priority < 0 high, 0 normal, > 0 low (clamped to the device's range).
 * Work enqueued on a LOW-priority stream yields the compute units to the caller's stream whenever both have workgroups ready:
 * weight-gradient products put there fill the gaps of the persistent recurrence kernels instead of delaying their launch.
 * Destroy with fov_stream_destroy after synchronising it. */
int fov_stream_create(int priority, fov_stream_t* stream);
int fov_stream_destroy(fov_stream_t stream);

/* The three weight gradients of an (unrolled) LSTM layer as ONE product and one reduce - what Keras/TF autodiff
 * computes as three (given_others...py:308 under model.fit):
 *     out (In1 + In2 + bias, Out) (+)= [x1 | x2 | 1]^T dpre        over the N rows (all steps x sequences)
 * i.e. rows [0, In1) = dK = x^T dz, rows [In1, In1+In2) = dR = h_prev^T dz, last row = db = column sums of dz: the layout
 * of a layer's kernel, recurrent_kernel and bias when they are adjacent in a flat gradient buffer.  x1 (N,In1), x2
 * (N,In2) or NULL with In2 = 0, dpre (N,Out), all dense row-major.  dpre is read once instead of three times and the
 * split partials are reduced by one launch.  bf16 != 0: operands rounded to bf16 (the bias row is summed in fp32 from
 * the unrounded values).  Shapes the fused kernel does not take (operands not 16-byte aligned, In1 not a multiple of
 * 128 with x2 given, In1 + In2 <= 96) produce the same result from the separate products.
 * fov_lstm_seq_bwd[_bf16] does the same internally when it is handed adjacent dK, dR, db and no initial state. */
size_t fov_wgrad_fused_workspace_bytes(int64_t N, int In1, int In2, int Out);
int fov_wgrad_fused(const float* x1, int In1, const float* x2, int In2, const float* dpre, float* out,
                    int64_t N, int Out, int bias, int accumulate, int bf16,
                    void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* fov_lstm_seq_fwd_train with bf16 operands (reserve may be NULL for inference); workspace >= 256 + 64 MB. */
int fov_lstm_seq_fwd_bf16(const float* x, const float* K, const float* R, const float* b, const float* h0,
                          const float* c0, float* hs, float* hT, float* cT, float* reserve, int B, int T, int F, int H,
                          int act, void* workspace, size_t workspace_bytes, fov_stream_t stream);
/* fov_seq2seq_decode_fwd with bf16 operands (BASELINE.json configs[1] shape; replaces the host loop of
 * mycode/FoV_seq2seq.py:137-178 over encoder_model / decoder_model, batched): the encoder over T_in steps from a zero
 * state, then T_out autoregressive decoder steps, each = LSTM step + Dense(F_dec, tanh) + feedback, in ONE persistent
 * launch.  Every product with x or h on its left (encoder gates, decoder gates, the Dense head) rounds both operands to
 * bf16 (round to nearest even) into the matrix core with fp32 accumulation; gates, cell state, y_t and every stored tensor
 * stay fp32; the fed-back y_t is rounded only where it enters the next step's x . dec_K.  A decoder step equals one
 * fov_lstm_seq_fwd_bf16 step from the fed-back state followed by fov_dense_fwd_bf16, bit for bit.
 * Arguments as fov_seq2seq_decode_fwd without impl; shapes: H = 256, F_enc <= 256, F_dec <= 8, either activation (others:
 * FOV_ERR_UNSUPPORTED).  B = 0: nothing is launched; T_in = 0: the decoder starts from a zero state; T_out = 0: the encoder
 * alone, `out` is not written; hT / cT (B,H) or NULL: the final state of the last phase that ran.  Workspace: the size of
 * fov_lstm_seq_fwd_bf16 (256 + 64 MB for B > 0), same header, sticky timeout word and fail-stop. */
int fov_seq2seq_decode_fwd_bf16(const float* enc_in, const float* dec_in0,
                                const float* enc_K, const float* enc_R, const float* enc_b,
                                const float* dec_K, const float* dec_R, const float* dec_b,
                                const float* dense_W, const float* dense_b,
                                float* out, float* hT, float* cT,
                                int B, int T_in, int T_out, int F_enc, int F_dec, int H,
                                int act, void* workspace, size_t workspace_bytes, fov_stream_t stream);
/* fov_dense_fwd with bf16 operands: y (N,Out) = act(x (N,In) . W (In,Out) + b), activation 0 = linear, 1 = tanh; b may be
 * NULL.  The products and their summation order are those of fov_seq2seq_decode_fwd_bf16's head (hidden units summed in
 * four 64-unit partials on the matrix core, added in order, then the bias): the teacher-forced paths use it
 * (FoV_seq2seq.py:82-101 in bf16), so training, predict and the fused call compute one arithmetic.  In <= 256, Out <= 16. */
int fov_dense_fwd_bf16(const float* x, const float* W, const float* b, float* y, int N, int In, int Out,
                       int activation, fov_stream_t stream);
/* Two stacked fp32 LSTM layers (F <= 96 -> 512 -> 512) in ONE launch - mycode/lstm.py:128-132,218-240: MultiRNNCell of two
 * LSTMCell(400) under dynamic_rnn with a fed state, zero-padded to the matrix-core width 512 (models.pad_lstm).  At the
 * script's batch a layer occupies 64 of 256 CUs, so layer 2 runs beside layer 1, a few steps behind: layer 1 publishes h_t of
 * every step as {value, epoch} granules into a ring of T slots and layer 2 takes its input from there (its 512-wide input never
 * comes from HBM).  At most 32 sequences: THREE roles - a third set of workgroups forms layer 2's input projection h1_t . K2 and
 * hands it over in tagged mailboxes, layer 2 keeps R2 only; every 32-workgroup group runs on an XCD of its own.  Same results
 * as two fov_lstm_seq_fwd[_train] calls: bit-identical for layer 1 and for the two-role form (33..64 sequences,
 * FOV_NO_WIDE16_TRIO=1), up to the order of layer 2's fp32 sums (2e-5 relative) in the three-role form.  h0_* / c0_* (B,H) or
 * NULL; reserve* (B,T,5,H) or NULL (training tape); hs1 may be NULL when only the top layer's sequence is wanted; hs2, hT*
 * and cT* may be NULL.
 * Shapes: fov_lstm_stack2_supported (H = 512, F <= 96, T >= 2, both layers' groups resident: <= 64 sequences on 256 CUs);
 * workspace >= fov_lstm_seq_workspace_bytes of a width-512 layer (header + granule area). */
int fov_lstm_stack2_supported(int B, int T, int F, int H);
int fov_lstm_stack2_fwd(const float* x, const float* K1, const float* R1, const float* b1, const float* h0_1, const float* c0_1,
                        const float* K2, const float* R2, const float* b2, const float* h0_2, const float* c0_2, float* hs1,
                        float* hT1, float* cT1, float* reserve1, float* hs2, float* hT2, float* cT2, float* reserve2, int B, int T,
                        int F, int H, int act, void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* BOTH encoder layers of the others-mixing model with bf16 operands in ONE launch, as a wavefront over (layer, step)
 * (given_others_gt_mean_var_seq2seq.py:108-112: LSTM(F -> 256) then LSTM(256 -> 256), zero initial states): layer 2 runs one
 * step behind layer 1 on the same CUs and takes its input tile straight from layer 1's exchange granules - T + 1
 * exchange-bound steps instead of 2 T.  Same results bit for bit as two fov_lstm_seq_fwd_bf16 calls.  H = 256, F <= 96,
 * T >= 2, at most CUs / 8 tiles of 16 sequences (fov_lstm_stack2_supported_bf16); hs / hT / cT / reserve of either layer may
 * be NULL; workspace as fov_lstm_seq_fwd_bf16. */
int fov_lstm_stack2_supported_bf16(int B, int T, int F, int H);
int fov_lstm_stack2_fwd_bf16(const float* x, const float* K1, const float* R1, const float* b1, const float* K2,
                             const float* R2, const float* b2, float* hs1, float* hT1, float* cT1, float* reserve1,
                             float* hs2, float* hT2, float* cT2, float* reserve2, int B, int T, int F, int H, int act,
                             void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* Backward of fov_mix_decoder_fwd (data path): BPTT through the whole unrolled decoder in ONE persistent launch.
 *   in : M, P (T_out,B,O) from the forward; dloss (T_out,B,O) = dL/d(pre-tanh of m_t) from the loss;
 *        res1, res2 (T_out,B,5,H); C1, C2 (T_out,B,H) = cell state BEFORE step t (row 0 = initial state);
 *        weights as in the forward (mix_Wp = mix_W[-O:]).
 *   out: DZ1, DZ2 (T_out,B,4H) gate pre-activation gradients of both layers and dpre_m, dpre_p (T_out,B,O)
 *        pre-activation gradients of the mixing / Dense layers, for every step (each weight gradient is then one
 *        product over all steps: dK = x^T dz, dR = h_prev^T dz, dW = in^T dpre); dh1_0..dc2_0 (B,H) gradient
 *        w.r.t. the decoder's initial state (= the encoder's final state).
 * Supported: O <= 8 and H = 256 (persistent kernel, workspace) or H = 32 (one workgroup per tile, workspace may be NULL and
 * its size is not looked at); H = 64 is FOV_ERR_UNSUPPORTED (see fov_mix_decoder_fwd). */
size_t fov_mix_decoder_bwd_workspace_bytes(int B, int H);
/* The fp32 fused decoder kernels keep a fragment-ordered copy of dec2_K in their workspaces, packed at every launch (the
 * weights change every optimizer step).  The pack depends on the weights only: this call runs it for the forward and / or
 * the backward workspace (either may be NULL) on `stream` - a side stream, under the encoder layers - and marks the
 * workspaces; the NEXT fov_mix_decoder_fwd / _bwd on a marked workspace with the same dec2_K skips its own pack.  The caller
 * orders the streams (the launch must come behind the pack).  The mark is valid for that one launch and only while dec2_K's
 * CONTENTS are unchanged (it is keyed by pointer: a caller that updates the weights in place packs again); fov_workspace_init and
 * the reset inside fov_check_status erase it, since they zero the packed copy; so does every other call that keeps something
 * of its own behind the workspace's granule area, where the packed copy lies (fov_lstm_seq_bwd, fov_lstm_stack2_bwd, the
 * two-launch cluster decode, the width-512 layer that projects its input first, fov_seq2seq_tf_fwd, the step-wise layer):
 * the launch behind such a call packs again.  H = 256 (another H: FOV_ERR_INVALID); both
 * workspaces are checked against their size functions before the first pack is launched. */
int fov_mix_decoder_prepack(const float* dec2_K, void* workspace_fwd, size_t fwd_bytes, void* workspace_bwd, size_t bwd_bytes,
                            int H, fov_stream_t stream);
int fov_mix_decoder_bwd(const float* M, const float* P, const float* dloss, const float* res1, const float* res2,
                        const float* C1, const float* C2, const float* dec1_K, const float* dec1_R,
                        const float* dec2_K, const float* dec2_R, const float* dense_W, const float* mix_Wp,
                        float* DZ1, float* DZ2, float* dpre_m, float* dpre_p,
                        float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0,
                        int B, int T_out, int H, int O, int act,
                        void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* C (M,N) = A (M,K) . B (K,N), row-major dense fp32 (keras.backend.dot on 2-D operands).  The
 * workspace is optional (NULL allowed): with it, short-and-wide products use split-K. */
size_t fov_matmul_workspace_bytes(int M, int K, int N);
int fov_matmul(const float* a, const float* b, float* c, int M, int K, int N,
               void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* LSTM layer whose input projection zx = x.K (B,T,4H) was computed by the caller (fov_matmul): the
 * form stacked layers use - given_others...py:111-112 (encoder2 over encoder1's sequence) and
 * :217 (decoder_lstm2) - because an (H,4H) input kernel does not fit beside the recurrent one.
 * Bias b is added inside.  Other arguments as fov_lstm_seq_fwd_train (reserve may be NULL). */
int fov_lstm_seq_fwd_zx(const float* zx, const float* R, const float* b, const float* h0, const float* c0,
                        float* hs, float* hT, float* cT, float* reserve,
                        int B, int T, int H, int act, int impl,
                        void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused inference path: encoder LSTM over T_in steps from zero state, then T_out
 * autoregressive decoder steps, each = LSTM step + Dense(F_dec,'tanh') + feedback, all on
 * device in ONE launch.
 *   replaces: the host loop mycode/FoV_seq2seq.py:154-178 over encoder_model / decoder_model
 *             (:137-148), batched.
 *   enc_in:(B,T_in,F_enc)  dec_in0:(B,1,F_dec)  out:(B,T_out,F_dec)
 *   hT,cT: final decoder state (B,H) or NULL.   F_dec <= 64 (wider: FOV_ERR_UNSUPPORTED).
 *   B = 0: nothing is launched.
 * ------------------------------------------------------------------------------------- */
size_t fov_seq2seq_decode_workspace_bytes(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int impl);
int fov_seq2seq_decode_fwd(const float* enc_in, const float* dec_in0,
                           const float* enc_K, const float* enc_R, const float* enc_b,
                           const float* dec_K, const float* dec_R, const float* dec_b,
                           const float* dense_W, const float* dense_b,
                           float* out, float* hT, float* cT,
                           int B, int T_in, int T_out, int F_enc, int F_dec, int H,
                           int act, int impl,
                           void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The recurrent kernel R (H,4H) in the order the fused call's waves hold it, for callers whose weights stay the same from
 * call to call (predict): made once per weight set, it lets the fused launch load a wave's slice as 16-byte loads.
 *   out: H * 4H floats, 16-byte aligned.  Element ((((c * NQ + jj) * 4 + s) * 64 + lane) * 4 + g), NQ = H / 16,
 *   lane = 16 * g4 + n, is R[16 * jj + 4 * g4 + s][g * H + 16 * c + n]  (c: 16-unit column block, jj: 16-row k-block,
 *   s: k-step of the block, g: gate).  A permutation of R: the values are copied, nothing is rounded.
 * R needs no alignment beyond a float's.  H in {64, 128, 256} (others: FOV_ERR_UNSUPPORTED).  One small launch on `stream`. */
int fov_lstm_pack_r(const float* R, int H, float* out, fov_stream_t stream);

/* fov_seq2seq_decode_fwd with the packs of enc_R and dec_R (fov_lstm_pack_r; either may be NULL).  The results are the same
 * bit for bit: the packs only change how the one-launch form of the call (H in {64, 128, 256}, one 16-sequence tile per
 * group of workgroups) loads its recurrent weights, and that form uses them when BOTH are given.  Every other form of the
 * call reads enc_R / dec_R, which must be valid either way.  The caller keeps a pack in step with its R: after R changes
 * the pack is made again (or NULL is passed).  A pack that is not 16-byte aligned is FOV_ERR_INVALID. */
int fov_seq2seq_decode_fwd_packed(const float* enc_in, const float* dec_in0,
                                  const float* enc_K, const float* enc_R, const float* enc_b,
                                  const float* dec_K, const float* dec_R, const float* dec_b,
                                  const float* dense_W, const float* dense_b,
                                  float* out, float* hT, float* cT,
                                  const float* enc_Rpack, const float* dec_Rpack,
                                  int B, int T_in, int T_out, int F_enc, int F_dec, int H,
                                  int act, int impl,
                                  void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The decoder half alone: T_out autoregressive steps from a GIVEN state (h0, c0) (B,H) (NULL = zeros) - what the
 * reference's sampling loop does after encoder_model.predict (FoV_seq2seq.py:156-178: decoder_model.predict fed its own
 * output), any batch, one launch.  out (B,T_out,F_dec); hT, cT (B,H) optional final state.  Workspace as for
 * fov_seq2seq_decode_fwd. */
int fov_seq2seq_decoder_fwd(const float* dec_in0, const float* h0, const float* c0, const float* dec_K,
                            const float* dec_R, const float* dec_b, const float* dense_W, const float* dense_b,
                            float* out, float* hT, float* cT, int B, int T_out, int F_dec, int H, int act, int impl,
                            void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The 2- and 3-layer target-only seq2seq model's inference in ONE launch (replaces the sampling models and the host loop of
 * mycode/Fov_seq2seq_2layers.py:360-430 and 3layers.py's loop, batched): the L-layer encoder over enc_in (B,T_in,F_enc) from
 * zero states (layer l reads layer l-1's h_t), then T_out decoder steps - decoder layer l, seeded with encoder layer l's
 * (h_T, c_T), takes one LSTM step from its own carried state (layer 0 on the fed-back input, layer l on layer l-1's new h),
 * y_t = tanh(h_top . dense_W + dense_b) is stored to out (B,T_out,F_dec) and fed back; the first input is dec_in0 (B,1,F_dec).
 * fp32 on the matrix core, exact expf / tanhf; pre-activations summed in the order bias, x . K, h . R.
 * Weights per layer, Keras layout: enc0_K (F_enc,4H), dec0_K (F_dec,4H), every other K and every R (H,4H), b (4H); the third
 * layer's six pointers are NULL (and ignored) for L = 2.  hT, cT (L,B,H) or NULL: every layer's final state of the last
 * phase that ran.  B = 0: nothing is launched; T_in = 0: the decoder starts from zero states; T_out = 0: the encoder stack
 * alone, `out` is not written.
 * One workgroup owns a 16-sequence tile for all layers and steps, so the call takes NO workspace, keeps NO library state, waits
 * on nothing, and writes every element of `out` exactly once (rows of a ragged last tile beyond B are neither read nor written).
 * Shapes: H = 32 or 64 (a narrower model zero-padded by the caller, which is exact), L = 2 or 3, 1 <= F_enc <= 96,
 * 1 <= F_dec <= 8, 0 <= B, T_in, T_out <= 2^30; anything else: FOV_ERR_UNSUPPORTED before any HIP call.
 * fov_stacked_seq2seq_decode_supported is that rule as arithmetic (no device query), and 0 under FOV_NO_STACKED_DECODE=1
 * (the caller's host loop stays: A/B timing, cross-check); the _fwd entry itself does not read the knob. */
int fov_stacked_seq2seq_decode_supported(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L);
int fov_stacked_seq2seq_decode_fwd(const float* enc_in, const float* dec_in0,
                                   const float* enc0_K, const float* enc0_R, const float* enc0_b,
                                   const float* enc1_K, const float* enc1_R, const float* enc1_b,
                                   const float* enc2_K, const float* enc2_R, const float* enc2_b,
                                   const float* dec0_K, const float* dec0_R, const float* dec0_b,
                                   const float* dec1_K, const float* dec1_R, const float* dec1_b,
                                   const float* dec2_K, const float* dec2_R, const float* dec2_b,
                                   const float* dense_W, const float* dense_b,
                                   float* out, float* hT, float* cT,
                                   int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L,
                                   int act, fov_stream_t stream);

/* The self-fed one-layer decoder (mycode/FoV_seq2seq_no_teac_forc.py:37-149, `onelayer_tar_seq2seq`; the unrolled loop is
 * :96-118, its gradient is Keras autodiff under model.fit, :147-149) as ONE launch per direction, fp32 on the matrix core,
 * exact expf / tanhf.  One workgroup owns a 16-sequence tile for every step: no workspace, no library state, nothing to wait
 * on; rows of a ragged last tile beyond B read zeros and store nothing.
 *
 * fov_selffed_decoder_fwd - replaces the T iterations of :96-118.  From x0 (B,O) and the state (h0, c0) (B,H; both NULL = the
 * zero state of :98-99), for t < T:  z = b + x_t . K + h . R  (this order);  the Keras cell update;  a_t = dact(h_t . W + bd);
 * y_t = a_t + r  (r (B,O): the residual link's term of :103-107, or NULL);  x_{t+1} = y_t, kept on the chip.
 * K (O,4H), R (H,4H), b (4H), W (H,O), bd (O), Keras gate order.  act: FOV_ACT_*; dact: 1 tanh, 2 relu (the codes of fov_act_fwd).
 * Outputs, each of which may be NULL and is then not written - the tapes of the training step, time-major:
 *   Hs, Cs (T+1,B,H)  row t = state before step t (row 0 = the initial state)
 *   XA (T+1,B,O)      row 0 = x0, row t+1 = y_t          A (T,B,O)  a_t (of interest with a residual only)
 *   RES (T,B,1,5,H)   activated i, f, g, o and c of step t (the reserve layout of fov_lstm_seq_fwd_train at T = 1)
 *   y (B,T,O)         the prediction, batch-major
 *
 * fov_selffed_decoder_bwd - replaces Keras autodiff through that loop.  dloss (T,B,O) = dL/dy_t.  For t = T-1 .. 0:
 *   dy_t = dloss_t + dx_{t+1};  dpre_t = dy_t dact'(a_t);  dh = dpre_t . W^T + dz_{t+1} . R^T;  the cell's pointwise backward
 *   with the gate derivative taken from the stored gate and c_{t-1} = Cs[t];  dx_t = dz_t . K^T  (dx_{T} = dz_{T} = 0).
 * a_t is read from A when a_from_A != 0, else from XA[1:].  Outputs: DY, DPRE (T,B,O), DZ (T,B,4H), dx0 (B,O), and dh0, dc0
 * (B,H; either may be NULL).  The weight gradients are products over all steps of these tapes (fov_dense_bwd).
 *
 * Shapes: H = 32 or 64, 1 <= O <= 8, 0 <= B, T <= 2^30; anything else is FOV_ERR_UNSUPPORTED, decided before any HIP call.  A
 * missing required pointer or an unknown activation is FOV_ERR_INVALID.  B = 0 or T = 0 launches nothing: the forward then
 * writes nothing (no tape row 0 either); the backward, which takes no gradient of the final state, sets dx0, dh0 and dc0 to
 * zero with T = 0.  fov_selffed_decoder_supported is the shape rule as arithmetic (no device query), and 0 under
 * FOV_NO_SELFFED_FUSED=1 (the caller's host loop stays: A/B timing, cross-check); the two entries do not read the knob. */
int fov_selffed_decoder_supported(int B, int T, int O, int H);
int fov_selffed_decoder_fwd(const float* x0, const float* h0, const float* c0,
                            const float* K, const float* R, const float* b, const float* W, const float* bd, const float* r,
                            float* Hs, float* Cs, float* XA, float* A, float* RES, float* y,
                            int B, int T, int O, int H, int act, int dact, fov_stream_t stream);
int fov_selffed_decoder_bwd(const float* Cs, const float* XA, const float* A, const float* RES, const float* dloss,
                            const float* K, const float* R, const float* W,
                            float* DY, float* DPRE, float* DZ, float* dx0, float* dh0, float* dc0,
                            int B, int T, int O, int H, int act, int dact, int a_from_A, fov_stream_t stream);

/* The self-fed TWO-layer decoder of mycode/given_others_gt_mean_var_seq2seq.py:203-299 (the unrolled loop over predict_step
 * seconds; heads `target_user_only` :219-220, `others_mlp` :223-233, `others_lstm` :234-240; its gradient is Keras autodiff
 * under model.fit) as ONE launch per direction, fp32 on the matrix core, exact expf / tanhf.  The others only enter through a
 * per-step context that does not depend on the decoder: the caller projects it through its rows of decoder_dense once
 * (ctx (B,T,O) = ctx_t . W_c [+ bias]) and the head adds it inside the tanh.  One workgroup owns a 16-sequence tile for both
 * layers and every step: no workspace, no library state, nothing to wait on; rows of a ragged last tile beyond B read zeros and
 * store nothing.
 *
 * fov_selffed2_decoder_fwd - replaces the T iterations of :209-299.  From x0 (B,O) and the states h1_0, c1_0, h2_0, c2_0 (B,H;
 * each may be NULL = zeros), for t < T:
 *   z1 = b1 + x_t . K1 + h1 . R1     -> the Keras cell update -> h1_t, c1_t
 *   z2 = b2 + h1_t . K2 + h2 . R2    -> the Keras cell update -> h2_t, c2_t                     (sums in this order)
 *   y_t = tanh(bd + h2_t . W + ctx[:, t]);   x_{t+1} = y_t, kept on the chip
 * K1 (O,4H), K2, R1, R2 (H,4H), b1, b2 (4H), W (H,O), Keras gate order; bd (O) and ctx (B,T,O) are each optional (NULL = absent).
 * act: FOV_ACT_*.  Outputs, each of which may be NULL and is then not written - the tapes of the training step, time-major:
 *   H1, C1, H2, C2 (T+1,B,H)  row t = state before step t (row 0 = the initial state)
 *   XY (T+1,B,O)              row 0 = x0, row t+1 = y_t
 *   RES1, RES2 (T,B,1,5,H)    activated i, f, g, o and c of step t (the reserve layout of fov_lstm_seq_fwd_train at T = 1)
 *   y (B,T,O)                 the prediction, batch-major
 *   hT, cT (2,B,H)            the final states, layer 1 then layer 2
 * With every tape NULL the call is the inference forward.
 *
 * fov_selffed2_decoder_bwd - replaces Keras autodiff through that loop.  dloss (T,B,O) = dL/dy_t.  For t = T-1 .. 0:
 *   dy_t = dloss_t + dx_{t+1};  dpre_t = dy_t (1 - y_t^2)  with y_t = XY[t+1]
 *   dh2 = dpre_t . W^T + dz2_{t+1} . R2^T;  the cell's pointwise backward (stored gates, c_{t-1} = C2[t]) -> dz2_t
 *   dh1 = dz2_t . K2^T + dz1_{t+1} . R1^T;  the cell's pointwise backward (stored gates, c_{t-1} = C1[t]) -> dz1_t
 *   dx_t = dz1_t . K1^T                                                       (dx_T = dz1_T = dz2_T = 0)
 * Outputs: DPRE (T,B,O), DZ1, DZ2 (T,B,4H), and dx0 (B,O), dh1_0, dc1_0, dh2_0, dc2_0 (B,H), each of these five optional (NULL
 * = not written).  The final states carry no incoming gradient.  The weight gradients are products over all steps of these
 * tapes (fov_dense_bwd); the gradient of ctx is DPRE.
 *
 * Shapes: 1 <= O <= 8, 0 <= B, T <= 2^30; H = 32 or 64 for the forward, H = 32 for the backward (R2^T, K2^T and R1^T stay in LDS:
 * 48 KB at H = 32, 192 KB at H = 64, more than a CU has).  Anything else is FOV_ERR_UNSUPPORTED, decided before any pointer is
 * looked at and before any HIP call.  A missing required pointer or an unknown activation is FOV_ERR_INVALID.  B = 0 or T = 0
 * launches nothing: the forward then writes nothing (no tape row 0 either); the backward sets dx0 and the four state gradients
 * to zero with T = 0.  fov_selffed2_decoder_supported(B, T, O, H, backward) is the shape rule of the forward (backward = 0) or
 * of the backward (backward != 0) as arithmetic (no device query), and 0 under FOV_NO_SELFFED2_FUSED=1 (the caller's host loop
 * stays: A/B timing, cross-check); the two entries do not read the knob. */
int fov_selffed2_decoder_supported(int B, int T, int O, int H, int backward);
int fov_selffed2_decoder_fwd(const float* x0, const float* h1_0, const float* c1_0, const float* h2_0, const float* c2_0,
                             const float* K1, const float* R1, const float* b1, const float* K2, const float* R2, const float* b2,
                             const float* W, const float* bd, const float* ctx,
                             float* H1, float* C1, float* H2, float* C2, float* XY, float* RES1, float* RES2, float* y,
                             float* hT, float* cT,
                             int B, int T, int O, int H, int act, fov_stream_t stream);
int fov_selffed2_decoder_bwd(const float* C1, const float* C2, const float* XY, const float* RES1, const float* RES2,
                             const float* dloss,
                             const float* K1, const float* R1, const float* K2, const float* R2, const float* W,
                             float* DPRE, float* DZ1, float* DZ2, float* dx0,
                             float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0,
                             int B, int T, int O, int H, int act, fov_stream_t stream);

/* The 2- and 3-layer target-only seq2seq model's TRAINING graph as ONE launch per direction (replaces the layer-by-layer
 * graph of mycode/Fov_seq2seq_2layers.py:232-272 under model.fit / model.predict, :332-343, and 3layers.py's): fp32 on the matrix
 * core, exact expf / tanhf, pre-activations summed in the order bias, x . K, h . R.  One workgroup owns a 16-sequence tile for
 * every layer and step: no exchange, no workspace header, no library state, nothing to wait on; rows of a ragged last tile beyond
 * B read zeros and store nothing.  Weights as arrays of L pointers, Keras layout: enc_K[0] (F_enc,4H), dec_K[0] (F_dec,4H),
 * every other K and every R (H,4H), b (4H).
 *
 * fov_stacked_seq2seq_train_fwd - replaces the forward of :232-272.  The L-layer encoder over enc_in (B,T_in,F_enc) from zero
 * states (layer l reads layer l-1's h_t), then the L-layer teacher-forced decoder over dec_in (B,T_out,F_dec), decoder layer l
 * seeded with encoder layer l's (h_T, c_T).  The Dense head is not part of it.  Outputs, each of which may be NULL and is then
 * not written, in the layouts of the per-layer entry points - slice l is a valid operand of fov_lstm_seq_bwd / _wgrad:
 *   enc_hs (L,B,T_in,H), enc_res (L,B,T_in,5,H)     h_t and the activated i, f, g, o and c_t (fov_lstm_seq_fwd_train's reserve)
 *   dec_hs (L,B,T_out,H), dec_res (L,B,T_out,5,H)   the same of the decoder stack
 *   dec_top (B,T_out,H)                             the top decoder layer's h_t alone: with every tape NULL, the inference forward
 *   hT, cT (L,B,H)                                  the encoder's final states (zeros with T_in = 0)
 * T_in = 0: the decoder starts from zero states; T_out = 0: the encoder stack alone.
 *
 * fov_stacked_seq2seq_train_bwd - replaces Keras autodiff through both stacks (:332-343).  From the reserves, cT, every R_l, K_l of
 * the layers l >= 1 (entry 0 of enc_K / dec_K is not read) and dhs_top (B,T_out,H), the gradient that reaches the top decoder
 * layer's h_t from the head: BPTT through the decoder stack, top layer first,
 *   dh_{l,t} = (dx_{l+1,t}, or dhs_top at the top) + dz_{l,t+1} . R_l^T;  the cell's pointwise backward with the gate derivative
 *   taken from the stored gate;  dx_{l,t} = dz_{l,t} . K_l^T for l >= 1;
 * then each decoder layer's (dh_0, dc_0) enters the matching encoder layer as (dh_T, dc_T) and the encoder stack is walked the
 * same way.  Outputs: dec_dz (L,B,T_out,4H), enc_dz (L,B,T_in,4H); the weight gradients are products over these tapes
 * (fov_lstm_seq_wgrad_layers), the h tapes and hT are read there only.  scratch: fov_stacked_seq2seq_train_bwd_scratch_bytes
 * bytes of plain memory (the dx hand-off between layers), nothing is kept in it between calls.
 *
 * Shapes: H = 32 or 64 (a narrower model zero-padded by the caller, which is exact), L = 2 or 3, 1 <= F_enc <= 96,
 * 1 <= F_dec <= 8, 0 <= B, T_in, T_out <= 2^30; anything else is FOV_ERR_UNSUPPORTED, decided before any pointer is looked at and
 * before any HIP call.  A missing required pointer or an unknown activation is FOV_ERR_INVALID.  B = 0 launches nothing.
 * fov_stacked_seq2seq_train_supported is the shape rule as arithmetic (no device query), and 0 under FOV_NO_STACKED_TRAIN=1 (the
 * caller's per-layer path stays: A/B timing, cross-check); the two entries do not read the knob. */
int fov_stacked_seq2seq_train_supported(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L);
size_t fov_stacked_seq2seq_train_bwd_scratch_bytes(int B, int T_in, int T_out, int H);
int fov_stacked_seq2seq_train_fwd(const float* enc_in, const float* dec_in,
                                  const float* const* enc_K, const float* const* enc_R, const float* const* enc_b,
                                  const float* const* dec_K, const float* const* dec_R, const float* const* dec_b,
                                  float* enc_hs, float* enc_res, float* dec_hs, float* dec_res, float* dec_top, float* hT, float* cT,
                                  int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L, int act, fov_stream_t stream);
int fov_stacked_seq2seq_train_bwd(const float* enc_res, const float* dec_res, const float* cT, const float* dhs_top,
                                  const float* const* enc_R, const float* const* enc_K,
                                  const float* const* dec_R, const float* const* dec_K,
                                  float* enc_dz, float* dec_dz,
                                  int B, int T_in, int T_out, int H, int L, int act,
                                  void* scratch, size_t scratch_bytes, fov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Teacher-forced training-graph forward: encoder, decoder seeded with the encoder state over
 * GT decoder inputs, Dense(tanh) on every decoder output.
 *   replaces: model.predict / the forward half of model.fit on the graph built at
 *             mycode/FoV_seq2seq.py:82-101.
 *   dec_in:(B,T_out,F_dec)  out:(B,T_out,F_dec)
 *   workspace additionally holds the decoder hidden sequence (B,T_out,H).
 *   dense_b may be NULL.  The call is three launches in a row (encoder, decoder, head): every pointer, act and impl
 *   of all three are checked before the first one; only a shape that the requested impl does not have for the
 *   decoder layer is refused by the second call, after the encoder has been enqueued.
 *   B * T_out <= 2^31 - 1 (the head's row count), else FOV_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
size_t fov_seq2seq_tf_workspace_bytes(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int impl);
int fov_seq2seq_tf_fwd(const float* enc_in, const float* dec_in,
                       const float* enc_K, const float* enc_R, const float* enc_b,
                       const float* dec_K, const float* dec_R, const float* dec_b,
                       const float* dense_W, const float* dense_b,
                       float* out,
                       int B, int T_in, int T_out, int F_enc, int F_dec, int H,
                       int act, int impl,
                       void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * mu / sigma^2 feature op: per row of `fps` interleaved xyz frames -> [mx,my,mz,vx,vy,vz]
 * (population variance, ddof = 0).
 *   replaces: mycode/utility.py:483-500 (get_gt_target_xyz) and :505-517 (_oth); the (N,T,90)
 *   and (N,T,30,3) layouts are the same bytes, so `rows` = N*T (or N*T*U for others).
 *   y:(rows, 3*fps)  out:(rows, 6);  1 <= fps <= 2^20, else FOV_ERR_INVALID.
 * ------------------------------------------------------------------------------------- */
int fov_meanvar_xyz(const float* y, float* out, int64_t rows, int fps, fov_stream_t stream);

/* =======================================================================================
 * Training side (a6/a7): what `model.fit` runs under Keras - mycode/FoV_seq2seq.py:103,112-117
 * (model.compile(optimizer='Adam', loss='mean_squared_error'); TensorFlow autodiff = BPTT).
 * ===================================================================================== */

/* fov_lstm_seq_fwd that also writes the reserve (B,T,5,H) = gates i,f,g,o and cell state c of
 * every step, which the backward consumes. */
int fov_lstm_seq_fwd_train(const float* x, const float* K, const float* R, const float* b,
                           const float* h0, const float* c0, float* hs, float* hT, float* cT,
                           float* reserve, int B, int T, int F, int H, int act, int impl,
                           void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* BPTT of one LSTM layer.
 *   in : x (B,T,F), K, R, h0/c0 (B,H) or NULL, hs (B,T,H) and reserve from the forward,
 *        dhs (B,T,H) or NULL (gradient w.r.t. every h_t), dhT/dcT (B,H) or NULL (w.r.t. final state)
 *   out: dz (B,T,4H) pre-activation gradients (always), dx (B,T,F) or NULL,
 *        dK (F,4H), dR (H,4H), db (4H) (each may be NULL), dh0/dc0 (B,H) or NULL
 *   accumulate != 0 adds into dK/dR/db instead of overwriting. */
size_t fov_lstm_seq_bwd_workspace_bytes(int B, int T, int F, int H);
int fov_lstm_seq_bwd(const float* x, const float* K, const float* R, const float* h0, const float* c0,
                     const float* hs, const float* reserve,
                     const float* dhs, const float* dhT, const float* dcT,
                     float* dz, float* dx, float* dK, float* dR, float* db, float* dh0, float* dc0,
                     int B, int T, int F, int H, int act, int accumulate,
                     void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* Dense backward from dpre = dL/d(pre-activation) (N,Out): dW (In,Out) = x^T dpre, db = column sums,
 * dx (N,In) = dpre W^T; each output may be NULL. */
size_t fov_dense_bwd_workspace_bytes(int N, int In, int Out);
int fov_dense_bwd(const float* x, const float* W, const float* dpre, float* dx, float* dW, float* db,
                  int N, int In, int Out, int accumulate,
                  void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* Keras mean_squared_error averaged over all n elements, fused with the Dense activation
 * derivative: dpre = 2 (y - target)/n * (activation == 1 ? 1 - y^2 : 1); *loss = mean((y-target)^2)
 * (loss may be NULL).  workspace >= 4*((n+255)/256 + 64) bytes. */
int fov_mse_dense_grad(const float* y, const float* target, float* dpre, float* loss, int64_t n,
                       int activation, void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The same with (1) `weight` applied to dpre AND to *loss - under data parallelism a rank passes
 * n_local / n_global, so a plain SUM all-reduce of the flat gradient buffer (which also carries the loss) yields the
 * global-batch mean without a scaling pass - and (2) optionally a time-major prediction: time_major_T > 0 means y
 * and dpre are (T,B,O) while target stays (B,T,O) (the unrolled decoders of given_others...py keep their tape
 * time-major); then n must equal B*T*O.  time_major_T = 0: dense, same order (B, O unused). */
int fov_mse_dense_grad_w(const float* y, const float* target, float* dpre, float* loss, int64_t n, int activation,
                         float weight, int time_major_B, int time_major_T, int O, void* workspace, size_t workspace_bytes,
                         fov_stream_t stream);

/* fov_mse_dense_grad_w (batch-major) that also leaves the Dense head's BIAS gradient: db[o] = sum over the n / O rows of
 * dpre[row][o] (written, not added) - the `db` half of fov_dense_bwd (keras Dense(O) behind mean_squared_error,
 * mycode/FoV_seq2seq.py:96-101,267) from the launch that forms dpre; widths O <= 8 inside the kernel, wider heads by a column-sum
 * launch.  Pass db = NULL to fov_dense_bwd afterwards.  n is a multiple of O; workspace >= 4*(9*((n+255)/256) + 64 + 256*O) bytes. */
int fov_mse_dense_grad_db(const float* y, const float* target, float* dpre, float* loss, float* db, int64_t n, int O, int activation,
                          float weight, void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* Dense(O, tanh | linear) head + Keras mean_squared_error, FORWARD AND BACKWARD as ONE launch (round 5; two beyond 4 096 rows: the
 * blocks' partial sums are added by a second one) - what model.fit runs around the
 * decoder's hidden sequence in mycode/FoV_seq2seq.py:96-103: hs (N,H), W (H,O), b (O), target (N,O) ->
 *   y (N,O) = act(hs . W + b) (may be NULL), *loss = weight * mean (y - target)^2 (may be NULL), dX (N,H) = dloss/dhs (may be NULL),
 *   dW (H,O), db (O).  activation 0 linear, 1 tanh; weight as in fov_mse_dense_grad_w.  N <= 2^20, H <= 512 (multiple of 4), O <= 8
 *   (fov_dense_mse_head_supported); other shapes: fov_dense_fwd + fov_mse_dense_grad_db + fov_dense_bwd.  Deterministic. */
int fov_dense_mse_head_supported(int64_t N, int H, int O);
size_t fov_dense_mse_head_workspace_bytes(int64_t N, int H, int O);
int fov_dense_mse_head(const float* hs, const float* W, const float* b, const float* target, float* y, float* dX, float* dW,
                       float* db, float* loss, int64_t N, int H, int O, int activation, float weight, void* workspace,
                       size_t workspace_bytes, fov_stream_t stream);

/* x[0..n) *= s */
int fov_scale(float* x, int64_t n, float s, fov_stream_t stream);

/* Backward of an elementwise activation given its OUTPUT y: out = base + dy * act'(y), act' = 1 - y^2 for tanh
 * (activation 1), [y > 0] for relu (activation 2), y for exp (activation 3) or 1 (activation 0); base may be NULL; out may alias base or dy.  Used where a Dense output is
 * fed back as the next decoder input (given_others...py:292-293): the feedback gradient joins the loss gradient. */
int fov_act_bwd(const float* dy, const float* y, const float* base, float* out, int64_t n, int activation,
                fov_stream_t stream);

/* Pieces of the raw-TensorFlow model's training graph (mycode/lstm.py:218-240,321-337,556-567, cost.py:190-229).
 *   fov_act_fwd: y = act(x), 0 identity, 1 tanh, 2 relu, 3 exp (the two-layer heads of _pred_mean_var_xyz2_new);
 *     fov_act_bwd takes the same codes (exp: dy * y).
 *   fov_gauss_nll_grad: likelihood_loss_tf - mu, var (B,3); y (B,T_y,3*fps) interleaved x,y,z; per element
 *     l = log(var + 1e-20) + (y - mu)^2 / (var + 1e-20) clipped to [-10,10]; *loss = scale * mean_b sum l (scale =
 *     1/(running_length*fps) under cfg.process_in_seconds); dmu, dvar (B,3).  workspace >= 4*(B + 64) bytes.
 *     B <= 2^29 and 3 T_y fps <= 2^31 - 1, else FOV_ERR_INVALID.
 *   fov_rmsprop_tf_step: tf.train.RMSPropOptimizer (momentum 0): g' = clip_by_value(g, -clip, clip) if clip > 0;
 *     ms = decay*ms + (1-decay) g'^2; p -= lr * g' / sqrt(ms + eps)   (TF initialises ms to ONE, eps = 1e-10). */
int fov_act_fwd(const float* x, float* y, int64_t n, int activation, fov_stream_t stream);
int fov_gauss_nll_grad(const float* mu, const float* var, const float* y, float* loss, float* dmu, float* dvar,
                       int B, int T_y, int fps, float scale, void* workspace, size_t workspace_bytes,
                       fov_stream_t stream);
int fov_rmsprop_tf_step(float* params, const float* grads, float* ms, int64_t n, float lr, float decay, float eps,
                        float clip_value, fov_stream_t stream);
/* The same, fail-stop like fov_adam_step_guarded: skipped on the device when the sticky timeout word of one of the guard
 * workspaces (each may be NULL) is set - under data parallelism the all-reduced poison slot of the flat gradient buffer;
 * *applied += 1 by every update that ran (lstm.py:583-660's loop keeps going, fov_check_status reports once per epoch). */
int fov_rmsprop_tf_step_guarded(float* params, const float* grads, float* ms, int64_t n, float lr, float decay, float eps,
                                float clip_value, const void* guard0, const void* guard1, const void* guard2,
                                int64_t* applied, fov_stream_t stream);

/* The two two-layer heads of _pred_mean_var_xyz2_new (mycode/lstm.py:321-337) on the top layer's final state h (B,H), as one
 * launch each way: a1 = relu(h mu_W1 + mu_b1), mu = tanh(a1 mu_W2 + mu_b2), a3 = relu(h var_W1 + var_b1),
 * var = exp(a3 var_W2 + var_b2); W1 (H,M), W2 (M,O).  fov_tf_head_bwd takes d loss / d mu and d loss / d var (B,O) and writes
 * (accumulate != 0: adds) the eight weight gradients and dh (B,H) (always overwritten).  Shapes the fused kernels take:
 * fov_tf_head_supported (B <= 64, H <= 2048, M <= 32, O <= 8: the script runs B = 32, H = 400, M = 32, O = 3); for others the
 * same graph is available from fov_dense_fwd / fov_act_fwd / fov_dense_bwd / fov_act_bwd. */
int fov_tf_head_supported(int B, int H, int M, int O);
int fov_tf_head_fwd(const float* h, const float* mu_W1, const float* mu_b1, const float* mu_W2, const float* mu_b2,
                    const float* var_W1, const float* var_b1, const float* var_W2, const float* var_b2, float* a1, float* mu,
                    float* a3, float* var, int B, int H, int M, int O, fov_stream_t stream);
int fov_tf_head_bwd(const float* h, const float* mu_W1, const float* mu_W2, const float* var_W1, const float* var_W2,
                    const float* a1, const float* mu, const float* a3, const float* var, const float* dmu, const float* dvar,
                    float* g_mu_W1, float* g_mu_b1, float* g_mu_W2, float* g_mu_b2, float* g_var_W1, float* g_var_b1,
                    float* g_var_W2, float* g_var_b2, float* dh, int B, int H, int M, int O, int accumulate, fov_stream_t stream);

/* The heads of mycode/lstm.py's other two branches - the ones taken when cfg.predict_mean_var is False, i.e. under the committed
 * mycode/config.py:69,71 - as a fused chain of up to four small Dense layers on the top layer's final state (B rows, the script runs 32):
 *   _GMM_3dgassian (lstm.py:377-400): dims {H, 64, 128, 256, 10 n_mix}, activations relu (2) x3, final_mode 1 = the mixture split
 *     of :386-399 on the last layer: [n softmax weights (exp / sum exp) | 3n means | 3n sigmas = exp | 3n correlations = tanh];
 *   pred_cnn_model_fn (lstm.py:147-174): dims {H, 128, 256, 3 fps}, activations relu, relu, tanh (1), final_mode 0 - the centre taps
 *     of the three k = 5 'same' conv1d kernels, all that one time step ever meets.
 * W[l] (dims[l], dims[l+1]) row-major, b[l] (dims[l+1]); masks (array or NULL) hold optional (B, dims[l+1]) multipliers applied behind
 * layer l's activation (tf.layers.dropout, already scaled; the script calls it with training=False, so NULL is the reference);
 * acts[l] (B, dims[l+1]) receives layer l's output (behind activation and mask; the last one behind the split) - the tape of the
 * backward.  fov_mlp_head_bwd takes dlast = d loss / d PRE-activation of the last layer (what fov_gmm3d_loss_grad and
 * fov_mse_dense_grad produce) and writes (accumulate != 0: adds) gW[l], gb[l] and, if dx != NULL, dx (B, dims[0]).
 * Shapes: 1..4 layers, dims[0] <= 2048, the other widths <= 512 (fov_mlp_head_supported); pointer arrays live on the HOST, what they point to on the device. */
int fov_mlp_head_supported(int B, int L, const int* dims);
int fov_mlp_head_fwd(const float* x, const float* const* W, const float* const* b, const float* const* masks, float* const* acts,
                     const int* dims, const int* act_codes, int L, int final_mode, int n_mix, int B, fov_stream_t stream);
size_t fov_mlp_head_bwd_workspace_bytes(int B, int L, const int* dims);
int fov_mlp_head_bwd(const float* x, const float* const* W, const float* const* masks, const float* const* acts, const float* dlast,
                     float* const* gW, float* const* gb, float* dx, const int* dims, const int* act_codes, int L, int B,
                     int accumulate, void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* costfunc.mixture_3d_gaussian_loss (mycode/cost.py:486-549) with its gradient.  params (B, 10 n_mix) as fov_mlp_head_fwd's mixture
 * split lays them out (mixture m: means params[n+3m..], sigmas params[4n+3m..], rho12, rho13, rho23 params[7n+3m..]); y: n_pts frames
 * (x, y, z interleaved) per row, rows ldy floats apart (cfg.process_in_seconds: second 0 of y (B,T_y,3 fps), ldy = T_y * 3 fps, n_pts =
 * fps; per frame: y (B,T,3), n_pts = T).  Per (row, mixture): covariance [[s1^2, r12 s1 s2, r13 s1 s3], ...], repaired as
 * cost.py:335-348 (smallest eigenvalue lambda < 0: Sigma - 10 lambda I), density N(y_t; mu_m, Sigma'_m);
 *   *loss (may be NULL: gradient only) = scale * sum_{b,t} -log(sum_m [pi_m] N_bmt + 1e-20)      (scale = 1 / (batch_size * running_length [* fps]), cost.py:544-549)
 * weight_by_pi = 0 is the reference: cost.py:532-538 never multiplies by mixture_pi, so the softmax weights get no gradient.
 * dpre (B, 10 n_mix) = d loss / d the head's PRE-activations (through softmax / exp / tanh and the eigenvalue repair).  The 3x3
 * work runs in fp64.  n_mix <= 32, n_pts <= 256.  workspace >= 256 + 4 * B bytes, STATEFUL like the exchange workspaces: its first
 * word is the ticket by which the last workgroup to finish adds the B per-row parts in row order (one launch, run-to-run identical
 * loss); it must be zero on entry (zero-fill the buffer once), every call leaves it zero, and the buffer must not be shared
 * with calls on other streams.
 * fov_gmm3d_sample: one draw per frame - component = first m with cumsum(pi)[m] > u (u (B, n_pts) uniform), value mu_m + chol(Sigma'_m) z
 * (z (B, n_pts, 3) normal) -> out rows of 3 n_pts floats, ldo apart: what utility.sample_mixture_3D (utility.py:178-208) documents and
 * the GMM test loop (lstm.py:735-745,820-825) feeds back; the committed function itself stops in pdb and indexes two dimensions. */
int fov_gmm3d_loss_grad(const float* params, const float* y, int64_t ldy, float* loss, float* dpre, int B, int n_mix, int n_pts,
                        float scale, int weight_by_pi, void* workspace, size_t workspace_bytes, fov_stream_t stream);
int fov_gmm3d_sample(const float* params, const float* u, const float* z, float* out, int64_t ldo, int B, int n_mix, int n_pts,
                     fov_stream_t stream);

/* Keras-2.2 `categorical_crossentropy` on probabilities, TensorFlow backend form - the loss the heat-map fork compiles
 * (mycode/convlstm_heatmap.py:192): per pixel (row of C channels) q = p / sum p, q' = clip(q, 1e-7, 1 - 1e-7),
 * l = - sum_c target_c log q'_c; *loss (may be NULL) = mean over the n_pix rows; dp = d loss / d p, through the clip (zero
 * outside it) and the renormalisation.  p, target, dp (n_pix, C) dense; workspace >= 4*(n_pix/256 + 65) bytes. */
int fov_categorical_crossentropy_grad(const float* p, const float* target, float* dp, float* loss, int64_t n_pix, int C,
                                      void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* The optional term of costfunc._mse under cfg.add_xyz_sum1 (mycode/cost.py:20-29): reg = 0.5 * mean over pixels of
 * (ux^2 + uy^2 + uz^2 - 1)^2 on the first three channels of p (n_pix, C), C >= 3.  Its gradient 2 (s - 1) u_k / n_pix is
 * ADDED into dp (which holds the MSE gradient); *reg (may be NULL) receives the term.  workspace >= 4*(n_pix/256 + 65) bytes. */
int fov_xyz_sum1_grad(const float* p, float* dp, float* reg, int64_t n_pix, int C, void* workspace, size_t workspace_bytes,
                      fov_stream_t stream);

/* Sampled re-feed: the next input second drawn around the predicted mean / variance - what lstm.py:460-468 builds from
 * utility.generate_fake_batch_tf (utility.py:83-89) in its predict_len > 1 training graph, and lstm_keras.py:39-44,139-149
 * in its cfg.sample_and_refeed sampling model.  x[b, e] = mu[b, a(e)] + sd(var[b, a(e)]) * noise[b, e] for the 3*fps
 * elements e of one second; noise ~ N(0,1) (B, 3*fps) comes from the caller (TF's generator is not reproducible anyway)
 * and has the layout of x.  std_mode 0: sd = sqrt(var) (lstm.py), 1: sd = var (lstm_keras.py hands the variance to
 * `stddev`).  layout 0: a(e) = e % 3, frames interleaved x,y,z; 1: a(e) = e / fps, planar.  Rows of x / dx are ldx floats
 * apart, so a slot of the (B,T,3*fps) window is written / read in place.  Backward (reparameterisation, what TF
 * differentiates): dmu[b,a] = sum_e dx, dvar[b,a] = sum_e dx * noise * sd'(var); accumulate != 0 adds into dmu / dvar.
 * B <= 2^29, fps <= 2^20 and ldx >= 3 fps, else FOV_ERR_INVALID. */
int fov_sample_refeed_fwd(const float* mu, const float* var, const float* noise, float* x, int64_t ldx, int B, int fps,
                          int std_mode, int layout, fov_stream_t stream);
int fov_sample_refeed_bwd(const float* dx, int64_t ldx, const float* var, const float* noise, float* dmu, float* dvar,
                          int B, int fps, int std_mode, int layout, int accumulate, fov_stream_t stream);

/* Keras-2.2 optimizers on one flat parameter buffer.
 *   Adam   : lr_t = lr*sqrt(1-beta2^step)/(1-beta1^step); p -= lr_t*m/(sqrt(v)+eps)   (step >= 1)
 *   RMSprop: a = rho*a + (1-rho) g^2; p -= lr*g/(sqrt(a)+eps) */
int fov_adam_step(float* params, const float* grads, float* m, float* v, int64_t n,
                  float lr, float beta1, float beta2, float eps, int64_t step, fov_stream_t stream);
int fov_rmsprop_step(float* params, const float* grads, float* accum, int64_t n,
                     float lr, float rho, float eps, fov_stream_t stream);
/* The same, fail-stop: guard0..2 (each may be NULL) are the workspaces the training step's persistent-kernel calls
 * used.  If the sticky timeout word of one of them is set the gradients are garbage and the update is skipped ON THE
 * DEVICE (no host synchronisation); the parameters stay as they were until fov_check_status reports the failure.
 * applied (device pointer, may be NULL): *applied += 1 by every update that was NOT skipped - a caller that counts steps on the
 * host (Adam's bias correction) and only looks at the status now and then reads back how many updates really ran. */
int fov_adam_step_guarded(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1,
                          float beta2, float eps, int64_t step, const void* guard0, const void* guard1,
                          const void* guard2, int64_t* applied, fov_stream_t stream);
int fov_rmsprop_step_guarded(float* params, const float* grads, float* accum, int64_t n, float lr, float rho, float eps,
                             const void* guard0, const void* guard1, const void* guard2, int64_t* applied,
                             fov_stream_t stream);
/* Deferred split reductions of a training step (model.fit's backward, FoV_seq2seq.py:103,112-117): between _begin and
 * _flush / _end every weight-gradient entry point of this library whose OUTPUT lies inside [grad_base, grad_base +
 * grad_floats) - the caller's flat gradient buffer - keeps the partial slices of its split product in `arena` (caller-owned
 * device memory, any size >= 256 bytes: what does not fit is reduced at once) and the flush sums all of them in ONE launch
 * instead of one per product; results are bit-identical.  In-stream order is kept for writes made through this library (a
 * later product over a pending range flushes first); a caller that reads or writes the gradient buffer by other means
 * between _begin and _end calls _flush before.  Writers covered: fov_lstm_seq_bwd(_bf16), fov_lstm_seq_wgrad,
 * fov_lstm_seq_wgrad_pair, fov_lstm_seq_wgrad_layers, fov_lstm_stack2_bwd, fov_dense_bwd(_bf16), fov_wgrad_fused, fov_colsum, fov_mix_head_wgrad,
 * fov_mse_dense_grad_db / _w (db), fov_dense_mse_head, fov_mlp_head_bwd, fov_tf_head_bwd, fov_conv2d_wgrad,
 * fov_conv2d_dilated_wgrad, fov_conv2d_wgrad_bf16, in every kernel form and in their empty-shape zeroing; readers covered (they
 * flush over the gradients they read): fov_adam_step(_guarded), fov_rmsprop_step(_guarded), fov_rmsprop_tf_step(_guarded).
 * A region is KEYED BY ITS GRADIENT BUFFER: each caller (trainer, thread, stream, device) opens its own with _begin and names
 * it again by grad_base (any address inside the buffer) in _flush / _end; regions of different buffers share nothing - their
 * arenas and pending records are separate - so several may be open at once from different threads (at most 16 per process;
 * _begin on a buffer that overlaps an open region flushes and replaces that region).  The library holds the record table of
 * an open region (16 records, host memory) until _end; it allocates no device memory.  _flush / _end with grad_base = NULL
 * address every open region of the process; _begin with grad_base = NULL opens nothing (FOV_OK), a grad_base without an arena
 * of at least 256 bytes is FOV_ERR_INVALID, a 17th open region FOV_ERR_UNSUPPORTED. */
int fov_reduce_defer_begin(float* grad_base, size_t grad_floats, void* arena, size_t arena_bytes, fov_stream_t stream);
int fov_reduce_defer_flush(const float* grad_base, fov_stream_t stream);
int fov_reduce_defer_end(const float* grad_base, fov_stream_t stream);
/* Data-parallel training (the all-reduce of model.fit's gradients, given_others_gt_mean_var_seq2seq.py:494-506):
 * *out = 1.0f if the timeout word of one of the workspaces is set, else 0.0f.  The trainers keep `out` inside the flat
 * gradient buffer: after the SUM all-reduce it is nonzero on EVERY rank if any rank's step failed, and handed to the
 * guarded optimizer as its guard (a nonzero float is a nonzero word) all replicas skip the update together.  guard0..2: each
 * may be NULL, as for the optimizers. */
int fov_guard_flag(const void* guard0, const void* guard1, const void* guard2, float* out, fov_stream_t stream);

/* =======================================================================================
 * ConvLSTM2D seq2seq building blocks (a8/a9) - mycode/convlstm_seq2seq.py:100-126,146-165 (ConvLSTM2D),
 * :170-189,224-258 (Conv2D / Conv1D heads, channel Softmax).  NHWC activations, Keras kernel layout
 * (kh,kw,C,N), zero 'same' padding, stride 1, dilation 1, odd kernel sizes.  The inference forms with bf16 matrix-core
 * operands - fov_conv2d_fwd_bf16 (the head) and fov_convlstm_cell_fwd_bf16 (the cells) - take weights packed once by
 * their fov_*_pack_bf16; everything they read or store besides is the fp32 tensor of the fp32 entry point.
 * ===================================================================================== */

/* y (B,H,W,N) = act(conv2d_same(x, w) + b + add);  x may be strided: x_pixel_stride >= C floats (a layer can
 * read its input from a slot of a channel-concatenated map) and x_batch_stride >= H*W*x_pixel_stride (one time
 * step of a (B,T,H,W,C) sequence); b, add (B,H,W,N) may be NULL; add may alias y.  activation: 0 none, 2 relu.
 * A Conv1D(k) over (B,W,C) is kh = 1, kw = k, H = 1. */
int fov_conv2d_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, const float* w, const float* b,
                   const float* add, float* y, int B, int H, int W, int C, int N, int kh, int kw, int activation,
                   fov_stream_t stream);

/* fov_conv2d_fwd with bf16 matrix-core operands - inference of the Conv2D / Conv1D prediction head
 * (convlstm_seq2seq.py:176-181,231-238).  Arithmetic contract:
 *     y = act(conv2d_same(bf16(x), bf16(w)) + b)
 * both operands of every product rounded to bf16 round-to-nearest-even, products accumulated in fp32 in an order the
 * kernel chooses, bias added and relu applied in fp32, y stored fp32.  Stride 1, 'same' zero padding, odd kh, kw,
 * dilation 1.  The weights are constant across a predict call, so they are packed ONCE: fov_conv2d_pack_bf16 writes
 * fov_conv2d_bf16_packed_bytes(C, N, kh, kw) bytes (16-byte aligned, caller-owned device memory) from the fp32
 * (kh,kw,C,N) kernel; the layout is private to the library and depends on (C, N, kh, kw) only. */
size_t fov_conv2d_bf16_packed_bytes(int C, int N, int kh, int kw);
/* convlstm_seq2seq.py:176-181,231-238: the head's kernels, rounded and reordered for fov_conv2d_fwd_bf16. */
int fov_conv2d_pack_bf16(const float* w, void* packed, int C, int N, int kh, int kw, fov_stream_t stream);
/* convlstm_seq2seq.py:176-181,231-238: x, its strides, b, y, B .. activation as in fov_conv2d_fwd; w_packed is what
 * fov_conv2d_pack_bf16 wrote for the same (C, N, kh, kw).  The empty batch is FOV_OK; operands beyond 2 GiB are
 * FOV_ERR_UNSUPPORTED. */
int fov_conv2d_fwd_bf16(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, const void* w_packed, const float* b,
                        float* y, int B, int H, int W, int C, int N, int kh, int kw, int activation, fov_stream_t stream);

/* The same convolution over the channel concatenation [x1 | x2] (w: (kh,kw,C1+C2,N)) without the concatenated
 * map ever existing: one ConvLSTM2D step is z = conv([x_t | h_{t-1}], [K ; R]) + b in ONE launch
 * (convlstm_seq2seq.py:100-126: Keras runs input_conv and recurrent_conv separately and adds). */
int fov_conv2d_fwd2(const float* x1, int64_t x1_pixel_stride, int64_t x1_batch_stride, int C1,
                    const float* x2, int64_t x2_pixel_stride, int64_t x2_batch_stride, int C2,
                    const float* w, const float* b, const float* add, float* y,
                    int B, int H, int W, int N, int kh, int kw, int activation, fov_stream_t stream);

/* One whole ConvLSTM2D step in ONE launch (convlstm_seq2seq.py:100-126,146-165: Keras' ConvLSTM2DCell.call =
 * input_conv + recurrent_conv + bias, gate activations, c and h update):
 *     z = conv_same([x_t | h_prev], [K ; R]) + b;  i,f,o = recurrent_activation(z_i, z_f, z_o);  g = tanh(z_c)
 *     c_new = f * c_prev + i * g;  h = o * tanh(c_new)
 * x (B,H,W,C) and h_prev (B,H,W,F) with their pixel / batch strides; w (kh,kw,C+F,4F) with Keras' gate order i,f,c,o
 * in the last axis (w = K alone, (kh,kw,C,4F), when h_prev is NULL = zero state); b (4F) or NULL; c_prev (B*H*W,F) or
 * NULL; c_new may alias c_prev; h is written with pixel stride h_pixel_stride >= F and must NOT alias h_prev; gates
 * (B*H*W,4F) or NULL receives the ACTIVATED i,f,g,o (the tape fov_convlstm_gates_bwd reads).  The gate columns of a
 * unit are brought into one lane by the weight staging, so z never exists in memory.  Results are bit-identical to
 * fov_conv2d_fwd2 followed by fov_convlstm_gates[_train]. */
int fov_convlstm_cell_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, int C,
                          const float* h_prev, int64_t h_prev_pixel_stride, int64_t h_prev_batch_stride,
                          const float* w, const float* b, const float* c_prev, float* c_new,
                          float* h, int64_t h_pixel_stride, float* gates,
                          int B, int H, int W, int F, int kh, int kw, int recurrent_activation, fov_stream_t stream);

/* fov_convlstm_cell_fwd with bf16 matrix-core operands - inference of the six ConvLSTM2D layers
 * (convlstm_seq2seq.py:100-126,146-165).  Arithmetic contract:
 *     z = conv_same(bf16([x_t | h_prev]), bf16([K ; R])) + b
 *     i,f,o = recurrent_activation(z_i, z_f, z_o);  g = tanh(z_c)
 *     c_new = f * c_prev + i * g;  h = o * tanh(c_new)
 * both operands of every product rounded to bf16 round-to-nearest-even, products accumulated in fp32 in an order the
 * kernel chooses; bias, gates and cell update in fp32 with the activations fov_convlstm_cell_fwd uses; c_new, h and the
 * optional activated-gates tape stored fp32 - h is rounded only where a later product takes it as an operand, so every
 * other consumer of h sees fp32.  Stride 1, 'same' zero padding, odd kh, kw, dilation 1.  The weights are constant across
 * a predict call, so they are packed ONCE: fov_convlstm_cell_pack_bf16 writes fov_convlstm_cell_bf16_packed_bytes(Ctot, F,
 * kh, kw) bytes (16-byte aligned, caller-owned device memory) from the fp32 (kh,kw,Ctot,4F) stack [K ; R], Ctot = C + F
 * (or from K alone, Ctot = C, for the zero state); the layout is private to the library and depends on (Ctot, F, kh, kw)
 * only. */
size_t fov_convlstm_cell_bf16_packed_bytes(int Ctot, int F, int kh, int kw);
/* convlstm_seq2seq.py:100-126,146-165: a cell's kernels, rounded and reordered for fov_convlstm_cell_fwd_bf16. */
int fov_convlstm_cell_pack_bf16(const float* w, void* packed, int Ctot, int F, int kh, int kw, fov_stream_t stream);
/* convlstm_seq2seq.py:100-126,146-165: the parameters and aliasing rules of fov_convlstm_cell_fwd, with w_packed - what
 * fov_convlstm_cell_pack_bf16 wrote for (C + F, F, kh, kw), or for (C, F, kh, kw) when h_prev is NULL - in place of w.
 * c_prev NULL is the zero state.  The empty batch is FOV_OK; operands beyond 2 GiB are FOV_ERR_UNSUPPORTED. */
int fov_convlstm_cell_fwd_bf16(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, int C,
                               const float* h_prev, int64_t h_prev_pixel_stride, int64_t h_prev_batch_stride,
                               const void* w_packed, const float* b, const float* c_prev, float* c_new,
                               float* h, int64_t h_pixel_stride, float* gates,
                               int B, int H, int W, int F, int kh, int kw, int recurrent_activation, fov_stream_t stream);

/* ConvLSTM2DCell gates on z (rows, 4F) = conv(x,K)+b+conv(h,R), channel blocks i,f,c,o; c (rows,F) is
 * updated in place; h is written with pixel stride h_pixel_stride >= F. */
int fov_convlstm_gates(const float* z, float* c, float* h, int64_t h_pixel_stride, int64_t rows, int F,
                       int act, fov_stream_t stream);

/* Softmax over the last dimension of (rows, n) - keras.layers.Softmax(axis=-1), convlstm_seq2seq.py:236. */
int fov_softmax_lastdim(const float* x, float* y, int64_t rows, int n, fov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * ConvLSTM2D training (a8 backward): what model.fit runs under Keras/TF autodiff for the graph of
 * mycode/convlstm_seq2seq.py:100-126,146-165,209-282 compiled at :287 (RMSprop + costfunc._mse).
 * ------------------------------------------------------------------------------------- */

/* Forward gates that keep what the backward pass needs: gates (rows,4F) = activated i,f,g,o (may alias z),
 * c_new (rows,F) = f*c_prev + i*g (c_prev may be NULL = zero state), h = o*tanh(c_new) with pixel stride. */
int fov_convlstm_gates_train(const float* z, const float* c_prev, float* c_new, float* h, int64_t h_pixel_stride,
                             float* gates, int64_t rows, int F, int act, fov_stream_t stream);

/* Backward of the gates: dh (rows,F) with pixel stride; dc (rows,F) holds dL/dc_t on entry and dL/dc_{t-1} on
 * return; gates, c_prev (NULL = zero), c_new from the forward; dz (rows,4F) out (may alias gates). */
int fov_convlstm_gates_bwd(const float* dh, int64_t dh_pixel_stride, float* dc, const float* gates,
                           const float* c_prev, const float* c_new, float* dz, int64_t rows, int F, int act,
                           fov_stream_t stream);

/* Weight gradient of y = conv2d_same(x, w): dw (kh,kw,C,N) (+)= sum over the B*H*W pixels of
 * x[pixel + tap][c] * dy[pixel][n].  x: batch-dense NHWC with pixel stride x_pixel_stride >= C; dy (B*H*W, N).
 * workspace >= fov_conv2d_wgrad_workspace_bytes (split-K partials; deterministic fixed-order reduce).  With accumulate = 0,
 * without a workspace (NULL) or with a smaller one the product is split less or not at all; accumulate != 0 forms the product
 * in the workspace and needs kh*kw*C*N floats of it (FOV_ERR_WORKSPACE otherwise).  dw of 2 GiB or more (kh*kw*C*N >= 2^29):
 * FOV_ERR_UNSUPPORTED, also for fov_conv2d_dilated_wgrad. */
size_t fov_conv2d_wgrad_workspace_bytes(int C, int N, int kh, int kw);
int fov_conv2d_wgrad(const float* x, int64_t x_pixel_stride, const float* dy, float* dw, int B, int H, int W,
                     int C, int N, int kh, int kw, int accumulate, void* workspace, size_t workspace_bytes,
                     fov_stream_t stream);

/* fov_conv2d_wgrad with bf16 matrix-core operands - training of the Conv2D / Conv1D prediction head
 * (convlstm_seq2seq.py:176-181,231-238 under model.fit).  Arithmetic contract:
 *     dw[i][j][c][n] (+)= sum over the B*H*W pixels p of  bf16(x[p + tap(i,j)][c]) * bf16(dy[p][n])
 * both operands rounded to bf16 round-to-nearest-even, products accumulated in fp32 in an order the kernel chooses.
 * Unlike fov_conv2d_wgrad the tuned form multiplies the zero padding in: a non-finite x[.][c] makes every tap of channel c
 * non-finite, and a non-finite dy[.][n] every tap of output n, where the exact sum would skip the terms outside the image.  dw fp32 in the Keras (kh,kw,C,N) layout.  'same' zero padding,
 * stride 1, odd kh, kw, dilation 1.  x: batch-dense NHWC with pixel stride x_pixel_stride >= C; dy (B*H*W, N) with rows
 * dy_row_stride >= N floats apart (N for a dense dy; a trainer that keeps dy in a channel-padded buffer passes the view).
 * accumulate as in fov_conv2d_wgrad; the empty batch writes zeros (accumulate = 0) or leaves dw alone.  Any split is
 * deterministic (partial slices in the workspace - or in the arena of an open deferred region that holds dw -, fixed-order
 * reduce); results are bit-identical inside and outside a region.  workspace >= fov_conv2d_wgrad_bf16_workspace_bytes
 * (FOV_ERR_WORKSPACE otherwise).  x and dy may be larger than 2 GiB as a whole (the trainer's one product over all decoder steps
 * is): the maps are cut into slices of at most 2 GiB each; FOV_ERR_UNSUPPORTED only where one map alone exceeds 2 GiB or the
 * workspace cannot hold that many slices. */
size_t fov_conv2d_wgrad_bf16_workspace_bytes(int C, int N, int kh, int kw);
int fov_conv2d_wgrad_bf16(const float* x, int64_t x_pixel_stride, const float* dy, int64_t dy_row_stride, float* dw, int B, int H,
                          int W, int C, int N, int kh, int kw, int accumulate, void* workspace, size_t workspace_bytes,
                          fov_stream_t stream);

/* The same three with a dilation (Keras `dilation_rate`; cfg.dilation_rate of mycode/config.py:105 reaches the six ConvLSTM2D
 * layers of mycode/convlstm_seq2seq.py:100-126,146-165): tap (i, j) reads the pixel (i - kh/2, j - kw/2) * dilation away, 'same'
 * zero padding grows with it.  Keras's ConvLSTM2D dilates its INPUT convolution only: fov_convlstm_cell_dilated_fwd applies
 * `dilation` to the taps over x and leaves those over h_prev at 1.  The data gradient of a dilated convolution is the dilated
 * convolution with the transposed weights (fov_conv2d_weight_transpose + fov_conv2d_dilated_fwd).  dilation = 1 is exactly the
 * entry points above; dilation > 1 runs on the tap-gathering implicit GEMM (the LDS-resident forms are built for dilation 1). */
int fov_conv2d_dilated_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, const float* w, const float* b,
                           const float* add, float* y, int B, int H, int W, int C, int N, int kh, int kw, int dilation,
                           int activation, fov_stream_t stream);
int fov_convlstm_cell_dilated_fwd(const float* x, int64_t x_pixel_stride, int64_t x_batch_stride, int C, const float* h_prev,
                                  int64_t h_prev_pixel_stride, int64_t h_prev_batch_stride, const float* w, const float* b,
                                  const float* c_prev, float* c_new, float* h, int64_t h_pixel_stride, float* gates, int B,
                                  int H, int W, int F, int kh, int kw, int dilation, int recurrent_activation,
                                  fov_stream_t stream);
int fov_conv2d_dilated_wgrad(const float* x, int64_t x_pixel_stride, const float* dy, float* dw, int B, int H, int W, int C,
                             int N, int kh, int kw, int dilation, int accumulate, void* workspace, size_t workspace_bytes,
                             fov_stream_t stream);

/* wt (kh,kw,N,C) = w (kh,kw,C,N) flipped in both spatial axes and transposed in the channel axes: the data
 * gradient of y = conv2d_same(x, w) is dx = conv2d_same(dy, wt) (fov_conv2d_fwd). */
int fov_conv2d_weight_transpose(const float* w, float* wt, int kh, int kw, int C, int N, fov_stream_t stream);

/* Backward of fov_softmax_lastdim given its output p: dy = p * (dp - sum_c dp*p); dy may alias dp. */
int fov_softmax_lastdim_bwd(const float* dp, const float* p, float* dy, int64_t rows, int n, fov_stream_t stream);

/* out (cols) (+)= column sums of x (rows, cols): bias gradients.  workspace >= 4*(256*cols + 64) bytes.  1 <= cols <= 2^24,
 * else FOV_ERR_INVALID. */
int fov_colsum(const float* x, float* out, int64_t rows, int cols, int accumulate, void* workspace,
               size_t workspace_bytes, fov_stream_t stream);

/* Device-side windowing, the step in front of the path: reshape2second_stacks
 * (mycode/utility.py:264-305).  x:(U,S,feat) whole seconds of one video -> W = fov_window_count(S,T,stride)
 * windows; enc / fut / fut_in are (W*U, T, feat) window-major when collapse_user != 0, else (U, W, T, feat).
 * fut is `T/stride` windows ahead of enc; fut_in is fut shifted right one second, seeded with enc's last second. */
int64_t fov_window_count(int S, int T, int stride);
int fov_window_stacks(const float* x, float* enc, float* fut, float* fut_in, int U, int S, int feat, int T,
                      int stride, int collapse_user, fov_stream_t stream);

/* The seq2seq LSTM models' inputs gathered from tracks that stay on the device (wired in):
 *   replaces: mycode/utility.py:264-305, 359-446, 483-517 (reshape2second_stacks, get_data, get_gt_target_xyz[_oth]),
 *             mycode/given_others_gt_mean_var_seq2seq.py:675-695 and mycode/data_generator_including_saliency.py:93-182.
 * secs (rows, 3*fps): every whole second of every (video, user) track, a track a contiguous run of rows; feat (rows, 6) =
 * fov_meanvar_xyz(secs).  sample (n, 3) int32: [first row of the target's track, row of others_base, first second of the
 * window]; others_base (n_pairs, n_others) int32: the first rows of the tracks in the others' slots of a (video, target)
 * pair (NULL when n_others == 0).  Outputs, contiguous, any of them NULL (not written):
 *   enc        (n, T_in, enc_width)       seconds start .. start+T_in-1 of the target: raw from secs when enc_width == 3*fps,
 *                                         from feat when enc_width == 6; any other width of a non-NULL enc: FOV_ERR_INVALID
 *   dec_in     (n, 6)                     feat of second start+T_in-1 (the decoder's seed: the encoder's last second)
 *   target     (n, T_out, 6)              feat of the target at start+fut_offset+t
 *   others     (n, T_out, n_others, 6)    feat at others_base[pair][j] + start+fut_offset+t
 *   future_raw (n, T_out, 3*fps)          secs of the target at start+fut_offset+t
 * Bit copies, no arithmetic; ONE launch per call, 8-byte accesses when every base is 8-byte aligned and 3*fps is even,
 * else 4-byte ones (same result).  Nothing outside the tables is read: a sample is taken only if base >= 0, start >= 0 and
 * base + start + max(T_in, fut_offset + T_out) <= rows, else all its outputs are zeros; an others slot also needs
 * 0 <= pair < n_pairs and its own track's seconds inside [0, rows), else that slot is zeros.  That a track is as long as
 * the samples say is the caller's business (rows of the next track would be copied).  n == 0: FOV_OK, no launch. */
int fov_window_inputs(const float* secs, const float* feat, int64_t rows, int fps, const int32_t* sample, int64_t n,
                      const int32_t* others_base, int64_t n_pairs, int n_others, int T_in, int T_out, int fut_offset,
                      float* enc, int enc_width, float* dec_in, float* target, float* others, float* future_raw,
                      fov_stream_t stream);

/* FoV hit rate per predicted second, the evaluation step that consumes the path's output:
 * centres as unit xyz vectors -> (theta, phi) (mycode/dataIO.py:77-82), +-2pi seam fix
 * (baseline_knn_mean.py:78-85), area(pred box ^ gt box) / area(gt box) (:62-82).  Row strides in floats
 * (>= 3) let `pred_xyz` be the first three columns of the model's (N*T, 6) mean/variance output. */
int fov_fov_hit_rate(const float* pred_xyz, int64_t pred_row_stride, const float* gt_xyz, int64_t gt_row_stride,
                     float* out, int64_t rows, float span_deg, float gt_span_deg, fov_stream_t stream);

/* One-hot FoV heat maps of the ConvLSTM heat-map model (cfg.use_one_hot), built from the trajectories they encode:
 *   replaces: mycode/utility.py:522-544 (_save_theta_phi_index: frame centre xyz -> 10-degree (theta, phi) bin indices,
 *             through xyz2thetaphi of mycode/dataIO.py:77-82), :557-571 (_create_one_hot) and the transpose to channels-last
 *             of mycode/convlstm_seq2seq.py:356-374 (convlstm_heatmap.py:45-130).
 * Input: xyz (N,T,30,3) fp32, each step's 30 frames contiguous, steps / sequences `xyz_step_stride` / `xyz_seq_stride` floats
 * apart (the (N,T,1,30,3) form is a stride); OR theta_index, phi_index (N,T,30) int32 contiguous (the reference's cached
 * pickles).  Pass xyz = NULL for the second form.  Bins are computed in fp64, in the reference's operation order:
 *   theta = mod(atan2(y,x), 2pi) - pi, phi = mod(atan2(z, sqrt(x^2+y^2)) + pi/2, pi)  (mod with the divisor's sign),
 *   ti = floor((theta+pi)/pi*180/10) (36 -> 35), pi = floor(phi/pi*180/10) (18 -> 17).
 * Output: maps (N,T,36,18,C) fp32, C = 30 or 32: frame f sets channel f of pixel (ti, pi) to 1, every other element -
 * channels 30, 31 included - is written 0 (no memset needed).  Slab (n, t) starts at maps + n*maps_seq_stride +
 * t*maps_step_stride (floats, multiples of 4; base 16-byte aligned): batch-major or time-major from one launch.  maps may be
 * NULL when theta_out / phi_out ((N,T,30) int32, both or neither) are given: indices only.
 * status: a device int the caller zeroes once.  A NaN / infinite coordinate or an index outside [0,36) x [0,18) ORs a bit
 * into it (that frame's channel stays all zero, its index outputs are -1); fov_onehot_status synchronises `stream`,
 * returns FOV_ERR_INVALID if the word is set (and clears it), else FOV_OK. */
int fov_onehot_maps(const float* xyz, int64_t xyz_seq_stride, int64_t xyz_step_stride, const int* theta_index,
                    const int* phi_index, float* maps, int64_t maps_seq_stride, int64_t maps_step_stride, int channels,
                    int* theta_out, int* phi_out, int* status, int N, int T, fov_stream_t stream);
int fov_onehot_status(int* status, fov_stream_t stream);

/* The heat-map model's predictions decoded on the device, the step the reference's test loop runs right after model.predict:
 *   replaces: mycode/convlstm_seq2seq.py:537-542 and mycode/convlstm_heatmap.py:556-558,
 *             max_ind = np.argmax(decoded_sentence.reshape(batch_size, cfg.predict_step, -1, fps), axis=-2)
 * Map m is n_pix pixels of C channels, element (p, c) at maps + m*map_stride + p*pixel_stride + c (strides in floats,
 * pixel_stride >= C: a 30-channel view of a 32-channel buffer, a channel slice).  index[m*out_stride + c] is the pixel
 * number of channel c's maximum over the n_pix pixels, value[m*out_stride + c] (value may be NULL) that maximum bit for
 * bit; out_stride >= C lets a caller write slot t of an (N, T_out, C) tensor from step t.  Exactly np.argmax: the lowest
 * pixel number among equal maxima (compared by value, -0.0 == +0.0), a NaN counts as the maximum and the first NaN wins.
 * Every map is read once, in 8-byte loads when C, both strides and the base allow them, else in 4-byte loads; same result.
 * Domain: 1 <= C <= 64, 1 <= n_pix <= 2^20, n_maps >= 0 (0 launches nothing), else FOV_ERR_INVALID. */
int fov_heatmap_argmax(const float* maps, int64_t map_stride, int64_t pixel_stride, int* index, float* value,
                       int64_t out_stride, int64_t n_maps, int n_pix, int C, fov_stream_t stream);
/* Pixel number -> frame centre, the inverse of fov_onehot_maps' binning (mycode/utility.py:522-544) for the 36 x 18 /
 * 10-degree geometry: i in [0, 648), ti = i / 18, pi = i % 18, az = (ti + 0.5) * 10 deg, el = (pi + 0.5) * 10 deg - 90 deg,
 * xyz[3i..3i+2] = (cos el cos az, cos el sin az, sin el), evaluated in fp64 and rounded to fp32; each centre bins back to
 * its own (ti, pi).  index (n) int32 and xyz (n, 3) contiguous.  An index outside [0, 648) writes three zeros and ORs a bit
 * into `status`, the word of fov_onehot_maps' protocol: the caller zeroes it once, fov_onehot_status reads and clears it. */
int fov_heatmap_index_xyz(const int* index, float* xyz, int64_t n, int* status, fov_stream_t stream);

/* The 'accuracy' metric of Keras 2.1-2.2's model.compile(metrics=['accuracy']), counted on the device:
 *   replaces: the `acc` / `val_acc` that fit, fit_generator and evaluate report for the models compiled at
 *             mycode/given_others_gt_mean_var_seq2seq.py:308, FoV_seq2seq_mu_var.py:248, Fov_seq2seq_2layers.py:335,
 *             3layers.py:302, lstm_keras.py:87,247,392 and convlstm_heatmap.py:281 (keras/engine/training.py chooses
 *             categorical_accuracy, K.argmax(y_true, -1) == K.argmax(y_pred, -1), for an output of C > 1 channels and
 *             binary_accuracy, y_true == K.round(y_pred), for C == 1).
 * Row (i0, i1, r), 0 <= i0 < n0, 0 <= i1 < n1, 0 <= r < rows, of either operand starts at i0*s0 + i1*s1 + r*row_stride
 * floats; its C channels are contiguous, row_stride >= C (a 30-of-32-channel view works as it lies), outer strides >= 0.
 * A time-major prediction (T, B, H*W, C) meets a batch-major target (B, T, H*W, C) by swapping s0 and s1, not by a copy.
 * *matches (device memory, 8-byte aligned) receives the number of matching rows, or has it added when accumulate != 0; an
 * empty shape writes 0 or leaves it alone (and looks at neither operand).  Every refusal - a NULL or misaligned matches, a NULL
 * operand, a stride below its bound - comes before the count is cleared: a refused call leaves *matches as it was.  The count is an exact integer, the same in every run (integer atomics only).
 * C > 1: a row matches when both arg-maxes agree; arg-max takes the lowest index among equal maxima (-0.0 == +0.0) and
 * the first NaN of a row as its maximum (np.argmax, the rule of fov_heatmap_argmax; TensorFlow leaves both unspecified).
 * C == 1: an element matches when target == rint(pred), half to even (0.5 -> 0, 1.5 -> 2); a NaN matches nothing.
 * Forms: C <= 8 a thread per row; 8 < C a group of 4 ... 64 lanes per row, each on 2 channels by 8-byte loads when both
 * bases are 8-byte aligned and all six strides are even, else on 1 channel by 4-byte loads (same result); C beyond a
 * group's reach (128 / 64 channels) loops.  Domain: C >= 1, n0 * n1 * rows <= 2^40, else FOV_ERR_INVALID. */
int fov_categorical_accuracy(const float* pred, int64_t pred_s0, int64_t pred_s1, int64_t pred_row_stride,
                             const float* target, int64_t tgt_s0, int64_t tgt_s1, int64_t tgt_row_stride,
                             int64_t n0, int64_t n1, int64_t rows, int C,
                             int64_t* matches, int accumulate, fov_stream_t stream);

/* Zero-fills a freshly allocated workspace (asynchronously on `stream`): required once before its first use by
 * a persistent-kernel entry point, and again whenever the buffer is re-allocated. */
int fov_workspace_init(void* workspace, size_t workspace_bytes, fov_stream_t stream);

/* Synchronises `stream`, reads the sticky status word the persistent-kernel calls leave in `workspace` and
 * returns FOV_OK or FOV_ERR_TIMEOUT (= some call since the previous check gave up a bounded wait; its outputs and
 * those of every later call on this workspace are invalid).  Reporting a failure clears it (the workspace is
 * re-zeroed and usable again).  Workspaces of non-persistent calls report FOV_OK. */
int fov_check_status(void* workspace, size_t workspace_bytes, fov_stream_t stream);
/* Test switch: on != 0 makes every exchanging kernel launched on this workspace keep the placement-independent
 * (write-through) granule exchange even where its run-time handshake finds a whole group on one XCD.  Results are
 * bit-identical either way (tests/test_gpu_parity.py, tests/test_gpu_train.py); fov_exchange_mode tells which ran. */
int fov_workspace_force_safe(void* workspace, size_t workspace_bytes, int on, fov_stream_t stream);
/* The library reads its environment knobs (FOV_FORCE_SAFE_EXCHANGE, FOV_TWO_LAUNCHES, FOV_DBG_RESIDENT_LIMIT)
 * once, at first use; call this after changing them.  No launch path calls getenv. */
void fov_reload_env(void);
/* Diagnostic: launches of the generic (VALU, any-shape) LSTM kernel so far in this process - lets a test assert that a
 * call was served by the persistent matrix-core kernels. */
int64_t fov_debug_generic_launches(void);
/* Test hook: set the workspace's epoch base (device header and the host-side accounting) - lets a test reach the
 * re-zero threshold of the 32-bit epoch tags without 10^7 launches. */
int fov_debug_set_epoch(void* workspace, size_t workspace_bytes, unsigned epoch, fov_stream_t stream);

/* Diagnostic: which h-exchange protocol the last persistent-kernel call on `workspace` used.
 * 1 = every group verified (HW_REG_XCC_ID handshake) that its workgroups share an XCD and took the
 *     L2-resident fast path; 2 = at least one workgroup used the placement-independent
 *     write-through path (also forced by the environment variable FOV_FORCE_SAFE_EXCHANGE=1).
 * Results are identical either way.  Synchronises `stream`. */
int fov_exchange_mode(const void* workspace, size_t workspace_bytes, fov_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FOV360_H */
