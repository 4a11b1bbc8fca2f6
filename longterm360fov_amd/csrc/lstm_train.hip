// Host dispatch of a layer's training step (a6: mycode/FoV_seq2seq.py:103,112-117 leave it to Keras autodiff):
// lstm_seq_bwd / lstm_stack2_bwd run the recurrence on a persistent BPTT kernel (lstm_bwd_cluster / lstm_bwd8 /
// lstm_bwd16.hip) or, for other widths and under FOV_BWD_STEPPED, step it from the host, then form dK / dR / db / dx
// through wgrad_group.hip, the fused [x | h_prev | 1]^T dz product or single GEMMs - which of these, decided once per call by
// plan_lstm_bwd on the workspace that bwd_carve cuts up; dense_bwd and mix_head_wgrad do the
// same for the heads.  launch_stepwise is the step-wise forward of layers wider than the persistent kernels take.
// The only kernels here are the pointwise halves of the two stepped recurrences and mix_head_wgrad_kernel.
#include "xch_common.h"
#include "bf16_common.h"
#include "gemm_f32.h"

namespace fov {

// ---------------------------------------------------------------------------------------
// BPTT pointwise step t of the host-stepped recurrence: the formula of lstm_cell_bwd (fov_common.h), written out.
// dh_rec / dc live in (B,H) buffers.
// ---------------------------------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void lstm_bwd_pointwise(const float* __restrict__ reserve, const float* __restrict__ c0,
                                                          const float* __restrict__ dhs, const float* __restrict__ dh_rec,
                                                          float* __restrict__ dc, float* __restrict__ dz, int B, int T,
                                                          int H, int t) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H) return;
    const int b = (int)(idx / H), j = (int)(idx - (long)b * H);
    const float* rp = reserve + (((size_t)b * T + t) * 5) * H + j;
    const float i = rp[0], f = rp[H], g = rp[2 * H], o = rp[3 * H], c = rp[4 * H];
    const float cprev = (t > 0) ? rp[4 * H - 5 * (long)H] : (c0 ? c0[idx] : 0.f);
    float dh = dh_rec[idx];
    if (dhs) dh += dhs[((size_t)b * T + t) * H + j];
    const float tc = tanh_f(c);
    const float dov = dh * tc;
    const float dcv = dc[idx] + dh * o * (1.f - tc * tc);
    float* zp = dz + ((size_t)b * T + t) * 4 * H + j;
    zp[0] = dcv * g * rec_act_grad<ACT>(i);
    zp[H] = dcv * cprev * rec_act_grad<ACT>(f);
    zp[2 * H] = dcv * i * (1.f - g * g);
    zp[3 * H] = dov * rec_act_grad<ACT>(o);
    dc[idx] = dcv * f;
}

// The workspace of lstm_seq_bwd, cut up in one place: the size function answers `total`, the launch side reads the offsets
// (floats from the workspace's start), so whatever has an offset here fits a workspace that passed the size check.
struct BwdCarve {
    size_t dh_rec, dc;   // (B,H) each, behind the header and the fixed granule area (xch_common.h): the stepped recurrence's
                         // carries; the persistent kernels' state gradients when the caller asks for none
    size_t scratch;      // split-K partials of the products and column sums; at its start, while the recurrence runs:
    size_t db_part;      //   the persistent kernels' per-tile bias partials (tiles,4H), with colsum's partials behind them
    size_t dx_parts;     //   fp32, 256 -> 256 on the eight-workgroup kernel: the eight partial tapes of dx = dz K^T behind the
                         //   bias partials; 0 for every other shape
    size_t total;
};
static constexpr size_t kDxTapeFloats = 8 * 256;   // per (sequence, step)

static BwdCarve bwd_carve(int B, int T, int F, int H) {
    BwdCarve c = {};
    const size_t bh = (size_t)B * H, db_floats = (size_t)((B + 15) / 16) * 4 * H;
    c.dh_rec = (kStatusBytes + kXchBytes) / sizeof(float);
    c.dc = c.dh_rec + bh;
    c.scratch = c.db_part = c.dc + bh;
    size_t m = (size_t)64 * (size_t)(F > H ? F : H) * 4 * H;   // split-K partials of dK / dR (<= 64 slices)
    auto at_least = [&m](size_t floats) { if (floats > m) m = floats; };
    at_least(db_floats + (size_t)256 * 4 * H);
    at_least((size_t)8 * bh);                                   // split-K partials of the stepped recurrence's dh GEMM
    if (F == 256 && H == 256) {
        c.dx_parts = c.scratch + ((db_floats + 63) & ~(size_t)63);
        at_least(c.dx_parts - c.scratch + kDxTapeFloats * B * T + 64);
    }
    c.total = c.scratch + m + 64;
    return c;
}

size_t lstm_bwd_workspace_floats(int B, int T, int F, int H) { return bwd_carve(B, T, F, H).total; }

// ---------------------------------------------------------------------------------------------------------------
// Step-wise layer forward on the matrix-core GEMM, for hidden widths the persistent kernels do not take (H > 256: the
// raw-TensorFlow model's LSTMCell(400), mycode/lstm.py:59,128-132).  zx = x K for ALL steps is one product; a step is
// zr = h_{t-1} R (one product over all sequences, every CU takes a tile) + one pointwise launch (gates, c, h, tape).
// The generic kernel walks the steps inside one launch but streams all of K and R through every workgroup in every
// step on the VALU: 6.3 ms for two layers at (32, 10, 90, H = 400); this path is launch-bound at ~3 launches a step.
// ---------------------------------------------------------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void lstm_pointwise_fwd_kernel(const float* __restrict__ zx, long ldzx, const float* __restrict__ zr,
                                                                 const float* __restrict__ b, const float* __restrict__ c_in,
                                                                 float* __restrict__ c_out, float* __restrict__ h_out, long ldh,
                                                                 float* __restrict__ reserve, long ldres, float* __restrict__ hT,
                                                                 float* __restrict__ cT, int B, int H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * H) return;
    const int row = (int)(i / H), u = (int)(i - (long)row * H);
    const float* zp = zx + (size_t)row * ldzx + u;
    const float* rp = zr ? zr + (size_t)row * 4 * H + u : nullptr;
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) z[g] = zp[g * H] + b[g * H + u] + (rp ? rp[g * H] : 0.f);
    const float ig = rec_act<ACT>(z[0]), fg = rec_act<ACT>(z[1]), gg = tanh_f(z[2]), og = rec_act<ACT>(z[3]);
    const float c = fmaf(fg, c_in ? c_in[i] : 0.f, ig * gg);
    const float h = og * tanh_f(c);
    c_out[i] = c;
    h_out[(size_t)row * ldh + u] = h;
    if (reserve) {
        float* q = reserve + (size_t)row * ldres + u;
        q[0] = ig; q[H] = fg; q[2 * H] = gg; q[3 * H] = og; q[4 * H] = c;
    }
    if (hT) hT[i] = h;
    if (cT) cT[i] = c;
}

bool stepwise_preferred(int B, int F, int H) { return B > 0 && F > 0 && H > 256; }

size_t stepwise_workspace_floats(int B, int T, int H) {
    return (size_t)B * T * 4 * H + (size_t)B * 4 * H + (size_t)3 * B * H + ((size_t)1 << 20) + 64;
}

int launch_stepwise(const LstmParams& p, float* ws, size_t ws_floats, hipStream_t stream) {
    const int B = p.B, T = p.T, F = p.F, H = p.H;
    if (B == 0) return FOV_OK;
    if (ws_floats < stepwise_workspace_floats(B, T, H)) { set_error("step-wise layer: workspace too small"); return FOV_ERR_WORKSPACE; }
    const size_t bh = (size_t)B * H;
    if (T == 0) {
        const size_t nb = sizeof(float) * bh;
        if (p.hT) (void)(p.h0 ? hipMemcpyAsync(p.hT, p.h0, nb, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(p.hT, 0, nb, stream));
        if (p.cT) (void)(p.c0 ? hipMemcpyAsync(p.cT, p.c0, nb, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(p.cT, 0, nb, stream));
        return FOV_OK;
    }
    float* zx = ws;
    float* zr = zx + (size_t)B * T * 4 * H;
    float* cbuf = zr + (size_t)B * 4 * H;
    float* hbuf[2] = {cbuf + bh, cbuf + 2 * bh};
    float* scratch = cbuf + 3 * bh;
    const size_t scratch_floats = ws_floats - (size_t)(scratch - ws);
    // zx (B*T, 4H) = x (B*T, F) . K (F, 4H)
    int rc = matmul_f32(p.x, p.K, zx, B * T, F, 4 * H, scratch, scratch_floats, stream);
    if (rc) return rc;
    const dim3 pgrid((unsigned)((bh + 255) / 256));
    const float* hprev = p.h0;
    long ldhp = H;
    const float* cprev = p.c0;
    const auto pointwise = p.act == FOV_ACT_HARD_SIGMOID ? lstm_pointwise_fwd_kernel<FOV_ACT_HARD_SIGMOID> : lstm_pointwise_fwd_kernel<FOV_ACT_SIGMOID>;
    for (int t = 0; t < T; ++t) {
        const float* zrp = nullptr;
        if (hprev) {   // zr (B, 4H) = h_{t-1} (B, H) . R (H, 4H)
            rc = gemm_f32(gemm_nn(hprev, ldhp, p.R, 4 * H, zr, 4 * H, B, 4 * H, H), 0, scratch, scratch_floats, stream);
            if (rc) return rc;
            zrp = zr;
        }
        float* hout = p.hs ? p.hs + (size_t)t * H : hbuf[t & 1];
        const long ldh = p.hs ? (long)T * H : H;
        const bool last = (t == T - 1);
        float* res = p.reserve ? p.reserve + (size_t)t * 5 * H : nullptr;
        hipLaunchKernelGGL(pointwise, pgrid, dim3(256), 0, stream, zx + (size_t)t * 4 * H, (long)T * 4 * H, zrp, p.b, cprev, cbuf,
                           hout, ldh, res, (long)T * 5 * H, last ? p.hT : nullptr, last ? p.cT : nullptr, B, H);
        rc = launch_check("lstm_pointwise_fwd");
        if (rc) return rc;
        hprev = hout;
        ldhp = ldh;
        cprev = cbuf;      // in place: element i is read and written by the same thread
    }
    return FOV_OK;
}

// [dK ; dR ; db] = [A1 | A2 | 1]^T B as ONE product and one reduce: c is a dense (M1 + M2 + bias_row, N) matrix - the
// layout of a layer's kernel, recurrent kernel and bias in a trainer's flat gradient buffer.  Rows of the product are
// (ro, ri) pairs; a shifted operand presents its element (ro, ri - 1) at (ro, ri) and zero at ri == 0 (h_{t-1} read
// from the (B,T,H) tape of h_t).  A2 may be NULL.
bool wgrad_fusable(const float* a1, long lda1, long a1_so, int M1, const float* a2, long lda2, long a2_so, int M2, const float* b,
                   long ldb, long b_so, const float* c, int N) {
    auto al = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    if (!al(a1) || !al(b) || !al(c) || (lda1 & 3) || (a1_so & 3) || (M1 & 3) || (ldb & 3) || (b_so & 3) || (N & 3) || M1 <= 0) return false;
    if (a2 && (!al(a2) || (lda2 & 3) || (a2_so & 3) || (M2 & 3) || (M1 % 128) || M2 <= 0)) return false;
    return M1 + (a2 ? M2 : 0) > 96;   // the 128-row tile shape (gemm_f32) / the 128 x 128 bf16 tile
}

int wgrad_fused(const float* a1, long lda1, long a1_so, int M1, int shift1, const float* a2, long lda2, long a2_so, int M2, int shift2,
                const float* b, long ldb, long b_so, float* c, int N, int RO, int RI, int bias_row, int accumulate, int bf16,
                float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (bf16)
        return gemm_bf16_tn_fused(a1, lda1, a1_so, M1, shift1, a2, lda2, a2_so, M2, shift2, b, ldb, b_so, c, N, N, RO, RI, bias_row,
                                  accumulate, scratch, scratch_floats, stream);
    GemmArgs g = {};
    g.a = a1; g.b = b; g.c = c; g.M = M1 + (a2 ? M2 : 0); g.N = N; g.KO = RO; g.KI = RI;
    g.a_sm = 1; g.a_sko = a1_so; g.a_ski = lda1; g.b_sn = 1; g.b_sko = b_so; g.b_ski = ldb; g.ldc = N;
    g.a2 = a2; g.a2_sko = a2_so; g.a2_ski = lda2; g.M1 = M1; g.bias_row = bias_row ? 1 : 0;
    if (shift1 || shift2) {
        // the (ro, ri) rows are kept flat - full 16-row k-tiles instead of tiles that end with every ro row - and the
        // shifted operand is masked where ri == 0; needs rows that are contiguous across ro
        if (a1_so != (long)RI * lda1 || (a2 && a2_so != (long)RI * lda2) || b_so != (long)RI * ldb) {
            set_error("wgrad_fused: a shifted operand needs (ro, ri) rows that are contiguous");
            return FOV_ERR_UNSUPPORTED;
        }
        g.KO = 1; g.KI = RO * RI; g.a_sko = g.a2_sko = g.b_sko = 0;
        g.a_period = shift1 ? RI : 0;
        g.a2_period = shift2 ? RI : 0;
    }
    return gemm_f32(g, accumulate, scratch, scratch_floats, stream);
}

// dR += h0^T dz[:, 0]: the initial state's share of the recurrent-kernel gradient
static int h0_dz0_product(const float* h0, const float* dz, float* dR, int B, int T, int H, int bf16, float* scratch, size_t scratch_floats,
                          hipStream_t stream) {
    return bf16 ? gemm_bf16_tn(h0, H, 0, dz, (long)T * 4 * H, 0, dR, 4 * H, H, 4 * H, 1, B, 1, scratch, scratch_floats, stream)
                : gemm_f32(gemm_tn(h0, H, dz, (long)T * 4 * H, dR, H, 4 * H, 1, B), 1, scratch, scratch_floats, stream);
}

// The form a layer's weight gradients take, in the order of precedence.  Rows, Grouped: fp32 at few rows, all of a layer's (or of
// several layers') gradients in one launch of wgrad_group.hip, no split, no reduce.  FusedKR, FusedR: dK, dR, db (dR, db) adjacent
// in memory - a trainer's flat gradient buffer - as ONE product [x | h_{t-1} | 1]^T dz ([h_{t-1} | 1]^T dz plus dK on its own).
// Separate: a product each and a column sum.
enum class WgradForm { Rows, Grouped, FusedKR, FusedR, Separate };

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Rows: few rows (batch x time <= 640) AND narrow layers (the reference's batch of 32 at H <= 512): wgrad_rows_kernel, 16 x 64
// tiles, rows split over the waves.  Grouped: batch x time <= 1024 at H >= 512.  Separate: neither.  (db alone rides on neither.)
static WgradForm plan_few_rows(const LayerWgrad& w, int B, int H, int bf16) {
    if (bf16 || !(w.dK || w.dR)) return WgradForm::Separate;
    if (wgrad_rows_takes((long)B * w.T, H) && w.F <= 2048 &&
        ((((uintptr_t)w.dz) | ((uintptr_t)w.dK) | ((uintptr_t)w.dR) | ((uintptr_t)w.db)) & 15) == 0)
        return WgradForm::Rows;
    return wgrad_group_takes(B, w.T, H) && aligned16(w.dz) ? WgradForm::Grouped : WgradForm::Separate;
}

static WgradForm plan_products(const LayerWgrad& w, int H) {
    const int F = w.F, N4 = 4 * H;
    const long T = w.T;
    if (!w.dR || !w.db || T <= 1 || w.db != w.dR + (size_t)H * N4 || env_knobs().no_wgrad_fusion) return WgradForm::Separate;
    if (w.dK && w.dR == w.dK + (size_t)F * N4 && wgrad_fusable(w.x, F, T * F, F, w.hs, H, T * H, H, w.dz, N4, T * N4, w.dK, N4))
        return WgradForm::FusedKR;
    // F too narrow for a row tile, or dK elsewhere
    return wgrad_fusable(w.hs, H, T * H, H, nullptr, 0, 0, 0, w.dz, N4, T * N4, w.dR, N4) ? WgradForm::FusedR : WgradForm::Separate;
}

static WgradForm plan_wgrad(const LayerWgrad& w, int B, int H, int bf16) {
    const WgradForm few = plan_few_rows(w, B, H, bf16);
    return few != WgradForm::Separate ? few : plan_products(w, H);
}

// A layer's products from its dz tape in the form FusedKR, FusedR or Separate; a NULL gradient is skipped (db: the caller's
// persistent kernel has produced it already).  h_{-1} = 0 in the fused product: a given initial state adds its h0^T dz_0 afterwards.
static int lstm_seq_weight_products(const LayerWgrad& w, WgradForm form, int B, int H, int accumulate, int bf16, float* scratch,
                                    size_t scratch_floats, hipStream_t stream) {
    const float *x = w.x, *hs = w.hs, *h0 = w.h0, *dz = w.dz;
    float *dK = w.dK, *dR = w.dR, *db = w.db;
    const int T = w.T, F = w.F;
    const bool fuse_kr = form == WgradForm::FusedKR, fuse_r = form == WgradForm::FusedR;
    int rc;
    const long BT = (long)B * T;
    if (fuse_kr || fuse_r) {
        rc = fuse_kr ? wgrad_fused(x, F, (long)T * F, F, 0, hs, H, (long)T * H, H, 1, dz, 4 * H, (long)T * 4 * H, dK, 4 * H, B, T, 1,
                                   accumulate, bf16, scratch, scratch_floats, stream)
                     : wgrad_fused(hs, H, (long)T * H, H, 1, nullptr, 0, 0, 0, 0, dz, 4 * H, (long)T * 4 * H, dR, 4 * H, B, T, 1,
                                   accumulate, bf16, scratch, scratch_floats, stream);
        if (rc) return rc;
        if (h0 && (rc = h0_dz0_product(h0, dz, dR, B, T, H, bf16, scratch, scratch_floats, stream)) != 0) return rc;
        if (fuse_kr) dK = nullptr;
        dR = db = nullptr;
    }
    if (dK) {   // dK (F,4H) = x^T dz : A(m=f,k=(b,t)) = x[k][f], B(k,n) = dz[k][n]
        rc = skinny_tn(x, F, F, dz, 4 * H, 4 * H, BT, dK, 4 * H, 1, accumulate, scratch, scratch_floats, stream);
        if (rc == 0) rc = bf16 ? gemm_bf16_tn(x, F, 0, dz, 4 * H, 0, dK, 4 * H, F, 4 * H, 1, (int)BT, accumulate, scratch, scratch_floats, stream)
                               : gemm_f32(gemm_tn(x, F, dz, 4 * H, dK, F, 4 * H, 1, (int)BT), accumulate, scratch, scratch_floats, stream);
        if (rc < 0) return rc;
    }
    if (dR) {   // dR (H,4H) = sum_b sum_{t>=1} hs[b][t-1]^T dz[b][t]  +  h0^T dz[:,0]
        if (T > 1) {
            rc = bf16 ? gemm_bf16_tn(hs, H, (long)T * H, dz + (size_t)4 * H, 4 * H, (long)T * 4 * H, dR, 4 * H, H, 4 * H, B, T - 1,
                                     accumulate, scratch, scratch_floats, stream)
                      : gemm_f32(gemm_tn(hs, H, dz + (size_t)4 * H, 4 * H, dR, H, 4 * H, B, T - 1, (long)T * H, (long)T * 4 * H), accumulate,
                                 scratch, scratch_floats, stream);
            if (rc) return rc;
        } else if (!accumulate) {
            rc = zero_grad(dR, (size_t)H * 4 * H, stream);
            if (rc) return rc;
        }
        if (h0 && T > 0 && (rc = h0_dz0_product(h0, dz, dR, B, T, H, bf16, scratch, scratch_floats, stream)) != 0) return rc;
    }
    return db ? colsum(dz, db, BT, 4 * H, accumulate, scratch, scratch_floats, stream) : FOV_OK;
}

// accumulate = 0 on an empty batch or sequence: dK (F,4H), dR (H,4H), db (4H) = 0 (NULL ones are skipped)
int zero_lstm_wgrads(float* dK, float* dR, float* db, int F, int H, hipStream_t stream) {
    int rc = zero_grad(dK, (size_t)F * 4 * H, stream);
    if (!rc) rc = zero_grad(dR, (size_t)H * 4 * H, stream);
    if (!rc) rc = zero_grad(db, (size_t)4 * H, stream);
    return rc;
}

// one layer's weight gradients in the form planned for it
static int run_wgrad(const LayerWgrad& w, WgradForm form, int B, int H, int accumulate, int bf16, float* scratch, size_t scratch_floats,
                     hipStream_t stream) {
    if (w.T == 0 || B == 0) return accumulate ? FOV_OK : zero_lstm_wgrads(w.dK, w.dR, w.db, w.F, H, stream);
    if (form == WgradForm::Rows) return wgrad_rows_layers(1, &w, B, H, accumulate, stream);
    if (form == WgradForm::Grouped) return wgrad_group_layers(1, &w, B, H, accumulate, stream);
    return lstm_seq_weight_products(w, form, B, H, accumulate, bf16, scratch, scratch_floats, stream);
}

// Weight gradients of one layer from a dz tape its BPTT left behind (fov_lstm_seq_bwd* with dK = dR = db = NULL): lets a trainer
// put a layer's products on another stream than the next layer's recurrence.  Same arithmetic, same order as inside lstm_seq_bwd.
int lstm_seq_wgrad(const LayerWgrad& w, int B, int H, int accumulate, int bf16, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (bf16 && H != 256) { set_error("lstm_seq_wgrad: the bf16 path is built for H = 256"); return FOV_ERR_UNSUPPORTED; }
    return run_wgrad(w, plan_wgrad(w, B, H, bf16), B, H, accumulate, bf16, scratch, scratch_floats, stream);
}

// TWO layers that share the batch but not the time length (an encoder and its decoder: FoV_seq2seq.py:68-93): at the reference's
// batch all six gradients are ONE launch (wgrad_rows_kernel)
bool lstm_seq_wgrad_pair_one_launch(int B, int T1, int T2, int H) {
    return T1 > 0 && T2 > 0 && wgrad_rows_takes((long)B * (T1 > T2 ? T1 : T2), H);
}

// Weight gradients of an encoder / decoder pair or of the layers of a STACK (Fov_seq2seq_2layers.py:232-272: up to four layers that
// share the batch and the width, each with its own input width and time length) from their dz tapes, fp32.  One launch
// (wgrad_rows_kernel) when the rows form takes every layer; else each layer in its own form.  A workgroup of that kernel owns one
// output tile of one problem whatever else shares the launch, so both ways give the bits of the per-layer calls.
int lstm_seq_wgrad_layers(int L, const LayerWgrad* w, int B, int H, int accumulate, float* scratch, size_t scratch_floats,
                          hipStream_t stream) {
    WgradForm form[kMaxWgradLayers];      // L <= kMaxWgradLayers: the entry points check
    bool all_rows = true;
    for (int l = 0; l < L; ++l) {
        form[l] = plan_wgrad(w[l], B, H, 0);
        all_rows = all_rows && form[l] == WgradForm::Rows;
    }
    if (all_rows) return wgrad_rows_layers(L, w, B, H, accumulate, stream);
    for (int l = 0; l < L; ++l)
        if (int rc = run_wgrad(w[l], form[l], B, H, accumulate, 0, scratch, scratch_floats, stream)) return rc;
    return FOV_OK;
}

// How one layer's BPTT is executed, decided in one place from the layer's shape, its pointers and the knobs.
enum class BwdRecurrence {
    Bwd16,     // lstm_bwd16.hip (fp32, R 16-byte aligned): width 512, small batches at 128 / 256
    Bwd8,      // lstm_bwd8.hip: H = 256 up to 32 tiles (groups of eight workgroups fill the chip where the 4-group kernel leaves
               // half of it idle at 512 sequences) unless FOV_BWD_GROUPS4; bf16 operands exist in this kernel only
    Cluster,   // lstm_bwd_cluster.hip: H = 64 / 128 / 256
    Stepped    // other widths, a misaligned R at width 512, FOV_BWD_STEPPED: a pointwise launch and a GEMM per step
};
enum class DxSource {
    None,            // the caller wants no dx
    InKernel,        // bf16, 256-wide input (the stacked layer): the kernel forms dx = dz K^T from the dz tile it has gathered anyway
    InKernelParts,   // fp32 on the eight-workgroup kernel, 256 -> 256: every workgroup forms its gate columns' share of dx in the
                     // shadow of the exchange - eight partial tapes in the scratch, one reduce launch
    Gemm             // a product behind the weight gradients
};
struct BwdPlan {
    BwdRecurrence rec;
    WgradForm wgrad;   // a stepped recurrence takes the separate products; Rows and Grouped go before the fusions
    bool db_part;      // the persistent kernel writes per-tile bias partials and a column sum follows: db wanted, form Separate
    DxSource dx;
    BwdCarve carve;
};

static BwdPlan plan_lstm_bwd(const LstmBwdLayer& l) {
    const EnvKnobs& knobs = env_knobs();
    BwdPlan p = {};
    p.carve = bwd_carve(l.B, l.T, l.F, l.H);
    const bool wide16 = !l.bf16 && bwd16_takes(l.B, l.H) && aligned16(l.rec.R);
    p.rec = (knobs.bwd_stepped || !(wide16 || bwd_cluster_shape_ok(l.H))) ? BwdRecurrence::Stepped
            : wide16                                                       ? BwdRecurrence::Bwd16
            : (l.bf16 || (bwd8_preferred(l.B, l.H) && !knobs.bwd_groups4)) ? BwdRecurrence::Bwd8
                                                                           : BwdRecurrence::Cluster;
    const bool persistent = p.rec != BwdRecurrence::Stepped;
    p.wgrad = persistent ? plan_wgrad(l.wg, l.B, l.H, l.bf16) : WgradForm::Separate;
    p.db_part = persistent && l.wg.db && p.wgrad == WgradForm::Separate;
    const bool dx_in_bwd8 = p.rec == BwdRecurrence::Bwd8 && l.F == 256 && aligned16(l.K) && !knobs.no_dx_fusion;
    p.dx = !l.dx                                                 ? DxSource::None
           : dx_in_bwd8 && l.bf16                                ? DxSource::InKernel
           : dx_in_bwd8 && p.carve.dx_parts && aligned16(l.dx)   ? DxSource::InKernelParts
                                                                 : DxSource::Gemm;
    return p;
}

// BPTT of one layer.  dz:(B,T,4H) is an output (kept: the caller may need it for dx of the layer
// below).  dK,dR,db are overwritten (accumulate = 0) or added to (accumulate = 1).
int lstm_seq_bwd(const LstmBwdLayer& l, float* ws, size_t ws_floats, hipStream_t stream) {
    const int B = l.B, T = l.T, F = l.F, H = l.H, accumulate = l.accumulate, bf16 = l.bf16;
    if (bf16 && H != 256) { set_error("lstm_seq_bwd: the bf16 path is built for H = 256"); return FOV_ERR_UNSUPPORTED; }
    const BwdPlan plan = plan_lstm_bwd(l);
    if (ws_floats < plan.carve.total) { set_error("lstm_seq_bwd: workspace too small"); return FOV_ERR_WORKSPACE; }
    BwdRec r = l.rec;
    LayerWgrad wg = l.wg;
    const size_t bh = sizeof(float) * (size_t)B * H;
    if (T == 0) {
        if (!accumulate)
            if (int rc = zero_lstm_wgrads(wg.dK, wg.dR, wg.db, F, H, stream)) return rc;
        if (r.dh0) (void)(r.dhT ? hipMemcpyAsync(r.dh0, r.dhT, bh, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(r.dh0, 0, bh, stream));
        if (r.dc0) (void)(r.dcT ? hipMemcpyAsync(r.dc0, r.dcT, bh, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(r.dc0, 0, bh, stream));
        return FOV_OK;
    }
    float *dh_rec = ws + plan.carve.dh_rec, *dc = ws + plan.carve.dc, *scratch = ws + plan.carve.scratch;
    const size_t scratch_floats = ws_floats - plan.carve.scratch;
    prepack_forget(ws);   // carries and scratch lie where mix_decoder_prepack leaves its packed dec2_K
    int rc;
    if (plan.rec != BwdRecurrence::Stepped) {
        // one launch for the whole recurrence: dz (B,T,4H), dh0, dc0
        if (!r.dh0) r.dh0 = dh_rec;
        if (!r.dc0) r.dc0 = dc;
        r.db_part = plan.db_part ? ws + plan.carve.db_part : nullptr;
        float* dx_parts = plan.dx == DxSource::InKernelParts ? ws + plan.carve.dx_parts : nullptr;
        float* dx_out = dx_parts ? dx_parts : plan.dx == DxSource::InKernel ? l.dx : nullptr;
        if (env_knobs().dbg_trace)
            fprintf(stderr, "[fov trace] lstm_seq_bwd B=%d T=%d F=%d H=%d wide16=%d fuse_kr=%d fuse_r=%d grouped=%d acc=%d: recurrence next\n", B, T, F, H,
                    plan.rec == BwdRecurrence::Bwd16, plan.wgrad == WgradForm::FusedKR, plan.wgrad == WgradForm::FusedR, plan.wgrad <= WgradForm::Grouped, accumulate);
        rc = plan.rec == BwdRecurrence::Bwd16  ? launch_bwd16(r, B, T, H, l.act, ws, stream)
             : plan.rec == BwdRecurrence::Bwd8 ? launch_bwd8(r, B, T, l.act, bf16, ws, stream, dx_out ? l.K : nullptr, dx_out)
                                               : launch_bwd_cluster(r, B, T, H, l.act, ws, stream);
        if (rc) return rc;
        if (dx_parts) {      // dx = the eight workgroups' shares in slice order (before anything else touches the scratch)
            rc = splitk_reduce(dx_parts, l.dx, (long)B * T * 256, 8, 0, stream);
            if (rc) return rc;
        }
        if (env_knobs().dbg_trace) fprintf(stderr, "[fov trace] lstm_seq_bwd: recurrence done\n");
        if (r.db_part) {     // db = the column sum of the tiles' partials; colsum's own partials behind them
            const int tiles = (B + 15) / 16;
            const size_t part_floats = (size_t)tiles * 4 * H;
            rc = colsum(r.db_part, wg.db, tiles, 4 * H, accumulate, scratch + part_floats, scratch_floats - part_floats, stream);
            if (rc) return rc;
            wg.db = nullptr;
        }
    } else {
        hipError_t e = r.dhT ? hipMemcpyAsync(dh_rec, r.dhT, bh, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dh_rec, 0, bh, stream);
        if (e == hipSuccess) e = r.dcT ? hipMemcpyAsync(dc, r.dcT, bh, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dc, 0, bh, stream);
        if (e != hipSuccess) { set_error("lstm_seq_bwd init: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
        const long nelem = (long)B * H;
        const dim3 pgrid((unsigned)((nelem + 255) / 256));
        const auto pointwise = l.act == FOV_ACT_HARD_SIGMOID ? lstm_bwd_pointwise<FOV_ACT_HARD_SIGMOID> : lstm_bwd_pointwise<FOV_ACT_SIGMOID>;
        for (int t = T - 1; t >= 0; --t) {
            hipLaunchKernelGGL(pointwise, pgrid, dim3(256), 0, stream, r.reserve, r.c0, r.dhs, dh_rec, dc, r.dz, B, T, H, t);
            rc = launch_check("lstm_bwd_pointwise");
            if (rc) return rc;
            // dh_rec (B,H) = dz_t (B,4H) . R^T :  A(m,k) = dz[m][t][k], B(k,n) = R[n][k]
            rc = gemm_f32(gemm_nt(r.dz + (size_t)t * 4 * H, (long)T * 4 * H, r.R, 4 * H, dh_rec, H, B, H, 4 * H), 0, scratch, scratch_floats, stream);
            if (rc) return rc;
        }
        if (r.dh0) { e = hipMemcpyAsync(r.dh0, dh_rec, bh, hipMemcpyDeviceToDevice, stream); if (e != hipSuccess) { set_error("dh0 copy"); return FOV_ERR_LAUNCH; } }
        if (r.dc0) { e = hipMemcpyAsync(r.dc0, dc, bh, hipMemcpyDeviceToDevice, stream); if (e != hipSuccess) { set_error("dc0 copy"); return FOV_ERR_LAUNCH; } }
    }
    rc = run_wgrad(wg, plan.wgrad, B, H, accumulate, bf16, scratch, scratch_floats, stream);
    if (rc) return rc;
    if (plan.dx == DxSource::Gemm) {   // dx (B*T,F) = dz . K^T : A(m,k) = dz[m][k], B(k,n) = K[n][k]
        const long BT = (long)B * T;
        rc = (bf16 && aligned16(l.K)) ? gemm_bf16_nt(r.dz, 4 * H, l.K, 4 * H, l.dx, F, (int)BT, F, 4 * H, stream)
                                      : gemm_f32(gemm_nt(r.dz, 4 * H, l.K, 4 * H, l.dx, F, (int)BT, F, 4 * H), 0, scratch, scratch_floats, stream);
        if (rc) return rc;
    }
    return FOV_OK;
}

// BPTT of two stacked layers in ONE launch.  Width 512 (lstm_bwd16.hip: both recurrences and dx = dz2 . K2^T between them as three
// roles of one persistent kernel), then the two layers' weight-gradient products.  Same outputs as two lstm_seq_bwd calls
// (upper layer first, its dx as the lower layer's dhs) except that the intermediate dx is not materialised.
// The workspace: behind the header and the granule area the two layers' bias partials and four (B,H) of state gradients the
// caller does not ask for, then the scratch - what one layer's call with the wider of the two inputs has behind its header.
struct Stack2Carve {
    size_t db_part_up, db_part_low, spare, scratch, total;
};
static Stack2Carve stack2_carve(int B, int T, int F, int H) {
    Stack2Carve c = {};
    const size_t part_floats = (size_t)((B + 15) / 16) * 4 * H;
    const BwdCarve one = bwd_carve(B, T, F > H ? F : H, H);
    c.db_part_up = one.dh_rec;
    c.db_part_low = c.db_part_up + part_floats;
    c.spare = c.db_part_low + part_floats;
    c.scratch = c.spare + (size_t)4 * B * H;
    c.total = c.scratch + (one.total - one.dh_rec) + 64;
    return c;
}

size_t lstm_stack2_bwd_workspace_floats(int B, int T, int F, int H) { return stack2_carve(B, T, F, H).total; }

// At H = 32 / 64 (stack2_tile_bwd_kernel, lstm_stacked_train.hip): one workgroup per 16-sequence tile walks both layers, any batch;
// the workspace's header and granule area are neither read nor written, what lies behind them is the scratch of the products.
// The kernel writes no bias partials: db is the column sum of dz, with dK and dR through lstm_seq_wgrad_layers.
static int lstm_stack2_tile_bwd(const LstmBwdLayer& low, const LstmBwdLayer& up, float* ws, size_t ws_floats, hipStream_t stream) {
    const int B = low.B, T = low.T, H = low.H;
    const Stack2Carve carve = stack2_carve(B, T, low.F, H);
    if (ws_floats < carve.total) { set_error("lstm_stack2_bwd: workspace too small"); return FOV_ERR_WORKSPACE; }
    prepack_forget(ws);   // (as lstm_seq_bwd)
    if (int rc = launch_stack2_tile_bwd(up.rec, low.rec, up.K, B, T, H, low.act, stream)) return rc;
    const LayerWgrad wg[2] = {low.wg, up.wg};
    return lstm_seq_wgrad_layers(2, wg, B, H, low.accumulate, ws + carve.scratch, ws_floats - carve.scratch, stream);
}

int lstm_stack2_bwd(const LstmBwdLayer& low, const LstmBwdLayer& up, float* ws, size_t ws_floats, hipStream_t stream) {
    const int B = low.B, T = low.T, H = low.H, accumulate = low.accumulate;
    if (stack2_tile_bwd_width(H)) return lstm_stack2_tile_bwd(low, up, ws, ws_floats, stream);
    if (!bwd16_pair_shape(B, T, H)) { set_error("lstm_stack2_bwd: unsupported shape (H = 512, <= 32 sequences on 256 CUs)"); return FOV_ERR_UNSUPPORTED; }
    const Stack2Carve carve = stack2_carve(B, T, low.F, H);
    if (ws_floats < carve.total) { set_error("lstm_stack2_bwd: workspace too small"); return FOV_ERR_WORKSPACE; }
    prepack_forget(ws);   // (as lstm_seq_bwd)
    const size_t bh = (size_t)B * H;
    float *spare = ws + carve.spare, *scratch = ws + carve.scratch;
    const size_t scratch_floats = ws_floats - carve.scratch;
    LayerWgrad wg[2] = {low.wg, up.wg};
    // few rows: ALL weight gradients of both layers in one launch behind the recurrences (wgrad_group.hip; at this width a layer
    // the rows form takes, the grouped form takes too); else each layer's products, no few-row form for one layer alone
    WgradForm form[2] = {plan_few_rows(wg[0], B, H, 0), plan_few_rows(wg[1], B, H, 0)};
    const bool rows_form = form[0] == WgradForm::Rows && form[1] == WgradForm::Rows;
    const bool grouped = form[0] != WgradForm::Separate && form[1] != WgradForm::Separate;
    if (!grouped)
        for (int i = 0; i < 2; ++i) form[i] = plan_products(wg[i], H);
    BwdRec r[2] = {low.rec, up.rec};
    for (int i = 0; i < 2; ++i) {
        if (!r[i].dh0) r[i].dh0 = spare + (size_t)(2 - 2 * i) * bh;
        if (!r[i].dc0) r[i].dc0 = spare + (size_t)(3 - 2 * i) * bh;
        r[i].db_part = (!grouped && wg[i].db && form[i] == WgradForm::Separate) ? ws + (i ? carve.db_part_up : carve.db_part_low) : nullptr;
    }
    int rc = launch_bwd16_pair(r[1], r[0], up.K, B, T, low.act, ws, stream);
    if (rc) return rc;
    if (grouped) return rows_form ? wgrad_rows_layers(2, wg, B, H, accumulate, stream) : wgrad_group_layers(2, wg, B, H, accumulate, stream);
    for (int i = 1; i >= 0; --i) {
        if (r[i].db_part) {
            rc = colsum(r[i].db_part, wg[i].db, (long)((B + 15) / 16), 4 * H, accumulate, scratch, scratch_floats, stream);
            if (rc) return rc;
            wg[i].db = nullptr;
        }
        rc = lstm_seq_weight_products(wg[i], form[i], B, H, accumulate, 0, scratch, scratch_floats, stream);
        if (rc) return rc;
    }
    return FOV_OK;
}

// Dense backward given dpre (N,Out): dW (In,Out) = x^T dpre, db = colsum(dpre), dx (N,In) = dpre W^T
int dense_bwd(const float* x, const float* W, const float* dpre, float* dx, float* dW, float* db, int N, int In, int Out,
              int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream, int bf16) {
    int rc;
    if (dW && bf16 && Out >= 64 && (Out & 3) == 0 && (((uintptr_t)dpre) & 15) == 0) {
        // dW (In,Out) = x^T dpre with bf16 operands (the unrolled decoder's K / R gradients: one product over all steps)
        rc = gemm_bf16_tn(x, In, 0, dpre, Out, 0, dW, Out, In, Out, 1, N, accumulate, scratch, scratch_floats, stream);
        if (rc) return rc;
        dW = nullptr;
    }
    if (dW) {
        // skinny forms: out[s = output unit][w = input unit] stored transposed into dW (In,Out) for a narrow output (Dense(6)),
        // out[s = input unit][w = output unit] for a narrow input (the decoder LSTM's 6-wide kernel over all steps)
        rc = skinny_tn(dpre, Out, Out, x, In, In, N, dW, 1, Out, accumulate, scratch, scratch_floats, stream);
        if (rc == 0) rc = skinny_tn(x, In, In, dpre, Out, Out, N, dW, Out, 1, accumulate, scratch, scratch_floats, stream);
        if (rc == 0) rc = gemm_f32(gemm_tn(x, In, dpre, Out, dW, In, Out, 1, N), accumulate, scratch, scratch_floats, stream);
        if (rc < 0) return rc;
    }
    if (db) {
        rc = colsum(dpre, db, N, Out, accumulate, scratch, scratch_floats, stream);
        if (rc) return rc;
    }
    return dx ? gemm_f32(gemm_nt(dpre, Out, W, Out, dx, In, N, In, Out), 0, scratch, scratch_floats, stream) : FOV_OK;
}

// Weight gradients of the others-mixing head (given_others...py:127-130,166-168,257-265 under model.fit) in ONE launch and
// one reduce: with rows r = (t, b) of the unrolled decoder's tape,
//     [dense_W ; dense_b]       = [h2_t | 1]^T dpre_p              (H + 1, O)
//     [mix_W ; mix_b]           = [others_t | p_t | 1]^T dpre_m    (n_oth + O + 1, O)
// written as one (H + 1 + n_oth + O + 1, O) block - the layout of dense_W, dense_b, mix_W, mix_b in a trainer's flat
// gradient buffer.  Same scheme as skinny_tn (thread = one column of the wide operand, block = 64 columns x 4 row
// groups, eight rows in flight, the O values of a row are broadcast loads), the column decides which array it reads;
// `others` stays in its (B, T, n_oth) layout (row (t, b) is others[b][t]).
template <int NS>
__global__ __launch_bounds__(256) void mix_head_wgrad_kernel(const float* __restrict__ h2, const float* __restrict__ dpre_p,
                                                             const float* __restrict__ others, const float* __restrict__ p,
                                                             const float* __restrict__ dpre_m, float* __restrict__ part, int B,
                                                             int T, int H, int n_oth, long rows_per_chunk) {
    __shared__ float red[4][NS][64];
    const int li = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int w = blockIdx.x * 64 + li;
    const int ncol = H + 1 + n_oth + NS + 1;
    const long rows = (long)B * T;
    const long r0 = (long)blockIdx.y * rows_per_chunk;
    long r1 = r0 + rows_per_chunk;
    if (r1 > rows) r1 = rows;
    // what this thread's column reads: kind 0 = array with row stride ld (row r), 1 = ones, 2 = others[b][t][col]
    int kind = 1, col = 0;
    long ld = 0;
    const float* src = dpre_p;
    const float* S = dpre_p;
    if (w < H) { kind = 0; src = h2; ld = H; col = w; }
    else if (w == H) { kind = 1; }
    else {
        S = dpre_m;
        const int j = w - (H + 1);
        if (j < n_oth) { kind = 2; src = others; col = j; }
        else if (j < n_oth + NS) { kind = 0; src = p; ld = NS; col = j - n_oth; }
    }
    float acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.f;
    if (w < ncol) {
        for (long r = r0 + q; r < r1; r += 32) {
            float wv[8];
            long rr[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool ok = r + 4 * u < r1;
                rr[u] = ok ? r + 4 * u : r;
                // one unconditional load per row whatever the column reads (a load inside a branch is waited for at the merge)
                const int t = (int)((unsigned)rr[u] / (unsigned)B), b = (int)rr[u] - t * B;
                const long off = kind == 2 ? ((long)b * T + t) * n_oth + col : rr[u] * ld + col;   // kind 1: element 0 of dpre_p, unused
                const float v = src[off];
                wv[u] = ok ? (kind == 1 ? 1.f : v) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int i = 0; i < NS; ++i) acc[i] = fmaf(S[rr[u] * NS + i], wv[u], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) red[q][i][li] = acc[i];
    __syncthreads();
    if (q == 0 && w < ncol) {
        float* pp = part + (long)blockIdx.y * NS * ncol + (long)w * NS;
#pragma unroll
        for (int i = 0; i < NS; ++i) pp[i] = (red[0][i][li] + red[1][i][li]) + (red[2][i][li] + red[3][i][li]);
    }
}

size_t mix_head_wgrad_scratch_floats(int B, int T, int H, int O, int n_oth) {
    const long rows = (long)B * T;
    long chunks = rows / 32;
    if (chunks > 256) chunks = 256;
    if (chunks < 1) chunks = 1;
    return (size_t)chunks * (H + 1 + n_oth + O + 1) * O + 64;
}

int mix_head_wgrad(const float* h2, const float* dpre_p, const float* others, const float* p, const float* dpre_m, float* out, int B,
                   int T, int H, int O, int n_oth, int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    const long rows = (long)B * T;
    const int ncol = H + 1 + n_oth + O + 1;
    const size_t n = (size_t)ncol * O;
    if (rows <= 0) {
        return accumulate ? FOV_OK : zero_grad(out, n, stream);
    }
    long chunks = rows / 32;
    if (chunks > 256) chunks = 256;
    if (chunks < 1) chunks = 1;
    if ((size_t)chunks * n > scratch_floats) { set_error("mix_head_wgrad: scratch too small"); return FOV_ERR_WORKSPACE; }
    const long rpc = (rows + chunks - 1) / chunks;
    chunks = (rows + rpc - 1) / rpc;
    const dim3 grid((ncol + 63) / 64, (unsigned)chunks);
    bool deferred = false;
    if (float* arena = defer_alloc(out, n, (size_t)chunks * n, stream)) { scratch = arena; deferred = true; }
#define FOV_HEADW(NSV) \
    case NSV: hipLaunchKernelGGL(mix_head_wgrad_kernel<NSV>, grid, dim3(256), 0, stream, h2, dpre_p, others, p, dpre_m, scratch, B, T, H, n_oth, rpc); break
    switch (O) {
        FOV_HEADW(1); FOV_HEADW(2); FOV_HEADW(3); FOV_HEADW(4); FOV_HEADW(5); FOV_HEADW(6); FOV_HEADW(7); FOV_HEADW(8);
        default: set_error("mix_head_wgrad: O <= 8"); return FOV_ERR_UNSUPPORTED;
    }
#undef FOV_HEADW
    int rc = launch_check("mix_head_wgrad");
    if (rc) return rc;
    return reduce_or_defer(deferred, scratch, out, (long)n, (int)chunks, accumulate, stream, "mix_head_wgrad reduce");
}

}  // namespace fov
