// Host dispatch of a layer's training step (a6: mycode/FoV_seq2seq.py:103,112-117 leave it to Keras autodiff):
// lstm_seq_bwd / lstm_stack2_bwd run the recurrence on a persistent BPTT kernel (lstm_bwd_cluster / lstm_bwd8 /
// lstm_bwd16.hip) or, for other widths and under FOV_BWD_STEPPED, step it from the host, then form dK / dR / db / dx
// through wgrad_group.hip, the fused [x | h_prev | 1]^T dz product or single GEMMs; dense_bwd and mix_head_wgrad do the
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

size_t lstm_bwd_workspace_floats(int B, int T, int F, int H) {
    // dh_rec (B,H) + dc (B,H) + split-K scratch for the largest weight-gradient GEMM / colsum
    size_t wg = (size_t)64 * (size_t)(F > H ? F : H) * 4 * H;   // split-K partials of dK / dR (<= 64 slices)
    size_t cs = (size_t)256 * 4 * H + (size_t)((B + 15) / 16) * 4 * H;   // colsum partials + per-tile db partials
    size_t st = (size_t)8 * B * H;                               // split-K partials of the per-step dh GEMM
    size_t m = wg > cs ? wg : cs;
    // fp32, 256 -> 256 on the eight-workgroup BPTT kernel: the eight partial tapes of dx = dz K^T behind the per-tile db partials
    const size_t dxp = (F == 256 && H == 256) ? (size_t)8 * B * T * 256 + (size_t)((B + 15) / 16) * 4 * H + 64 : 0;
    if (dxp > m) m = dxp;
    // head: status word + granule buffers of the persistent BPTT kernel (when the shape allows it)
    size_t head = (kStatusBytes + kXchBytes) / sizeof(float);   // header + the fixed granule area (xch_common.h)
    return head + (size_t)2 * B * H + (m > st ? m : st) + 64;
}

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

// The weight-gradient half of a layer's BPTT, from its dz tape: dK = x^T dz, dR = h_{t-1}^T dz (h_{-1} = h0 or 0), db = colsum(dz).
// fuse_kr / fuse_r: the adjacent-in-memory forms (one product for all three / for dR and db); db_done: the caller's persistent
// kernel has produced db already (unfused forms only).
static int lstm_seq_weight_products(const float* x, const float* hs, const float* h0, const float* dz, float* dK, float* dR, float* db,
                                    int B, int T, int F, int H, int accumulate, int bf16, bool fuse_kr, bool fuse_r, bool db_done,
                                    float* scratch, size_t scratch_floats, hipStream_t stream) {
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
    return (db && !db_done) ? colsum(dz, db, BT, 4 * H, accumulate, scratch, scratch_floats, stream) : FOV_OK;
}

// few rows (batch x time <= ~1000), fp32: all of a layer's weight gradients by wgrad_group.hip - one launch, no split, no reduce
static bool lstm_seq_wgrad_grouped(int bf16, int B, int T, int H, const float* dz, float* dK, float* dR, float* db) {
    return !bf16 && wgrad_group_takes(B, T, H) && (dK || dR) && (((uintptr_t)dz) & 15) == 0 && (!db || dK || dR);
}

// few rows AND narrow layers (the reference's batch of 32 at H <= 256): wgrad_rows_kernel, 16 x 64 tiles, rows split over the waves
static bool lstm_seq_wgrad_rows(int bf16, int B, int T, int F, int H, const float* dz, float* dK, float* dR, float* db) {
    return !bf16 && wgrad_rows_takes((long)B * T, H) && F <= 2048 && (dK || dR) && (!db || dK || dR) &&
           ((((uintptr_t)dz) | ((uintptr_t)dK) | ((uintptr_t)dR) | ((uintptr_t)db)) & 15) == 0;
}

static int wgrad_few_rows(bool rows_form, const float* x, const float* hs, const float* h0, const float* dz, float* dK, float* dR, float* db,
                          int B, int T, int F, int H, int accumulate, hipStream_t stream) {
    return rows_form ? wgrad_rows_layers(1, &x, &F, &T, &hs, &h0, &dz, &dK, &dR, &db, B, H, accumulate, stream)
                     : wgrad_group_layers(1, &x, &F, &hs, &h0, &dz, &dK, &dR, &db, B, T, H, accumulate, stream);
}

static void lstm_seq_wgrad_fusion(const float* x, const float* hs, const float* dz, float* dK, float* dR, float* db, int T, int F, int H,
                                  bool* fuse_kr, bool* fuse_r) {
    const int N4 = 4 * H;
    *fuse_kr = dK && dR && db && T > 1 && dR == dK + (size_t)F * N4 && db == dR + (size_t)H * N4 &&
               wgrad_fusable(x, F, (long)T * F, F, hs, H, (long)T * H, H, dz, N4, (long)T * N4, dK, N4) && !env_knobs().no_wgrad_fusion;
    *fuse_r = !*fuse_kr && dR && db && T > 1 && db == dR + (size_t)H * N4 &&
              wgrad_fusable(hs, H, (long)T * H, H, nullptr, 0, 0, 0, dz, N4, (long)T * N4, dR, N4) && !env_knobs().no_wgrad_fusion;
}

// accumulate = 0 on an empty batch or sequence: dK (F,4H), dR (H,4H), db (4H) = 0 (NULL ones are skipped)
int zero_lstm_wgrads(float* dK, float* dR, float* db, int F, int H, hipStream_t stream) {
    int rc = zero_grad(dK, (size_t)F * 4 * H, stream);
    if (!rc) rc = zero_grad(dR, (size_t)H * 4 * H, stream);
    if (!rc) rc = zero_grad(db, (size_t)4 * H, stream);
    return rc;
}

// Weight gradients of one layer from a dz tape its BPTT left behind (fov_lstm_seq_bwd* with dK = dR = db = NULL): lets a trainer
// put a layer's products on another stream than the next layer's recurrence.  Same arithmetic, same order as inside lstm_seq_bwd.
int lstm_seq_wgrad(const float* x, const float* hs, const float* h0, const float* dz, float* dK, float* dR, float* db, int B, int T,
                   int F, int H, int accumulate, int bf16, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (bf16 && H != 256) { set_error("lstm_seq_wgrad: the bf16 path is built for H = 256"); return FOV_ERR_UNSUPPORTED; }
    if (T == 0 || B == 0) {
        if (!accumulate)
            if (int rc = zero_lstm_wgrads(dK, dR, db, F, H, stream)) return rc;
        return FOV_OK;
    }
    const bool rows_form = lstm_seq_wgrad_rows(bf16, B, T, F, H, dz, dK, dR, db);
    if (rows_form || lstm_seq_wgrad_grouped(bf16, B, T, H, dz, dK, dR, db))
        return wgrad_few_rows(rows_form, x, hs, h0, dz, dK, dR, db, B, T, F, H, accumulate, stream);
    bool fuse_kr, fuse_r;
    lstm_seq_wgrad_fusion(x, hs, dz, dK, dR, db, T, F, H, &fuse_kr, &fuse_r);
    return lstm_seq_weight_products(x, hs, h0, dz, dK, dR, db, B, T, F, H, accumulate, bf16, fuse_kr, fuse_r, false, scratch,
                                    scratch_floats, stream);
}

// Weight gradients of TWO layers that share the batch but not the time length (an encoder and its decoder: FoV_seq2seq.py:68-93)
// from the dz tapes their BPTT calls left.  At the reference's batch all six gradients are ONE launch (wgrad_rows_kernel).
bool lstm_seq_wgrad_pair_one_launch(int B, int T1, int T2, int H) {
    return T1 > 0 && T2 > 0 && wgrad_rows_takes((long)B * (T1 > T2 ? T1 : T2), H);
}

int lstm_seq_wgrad_pair(const float* x1, const float* hs1, const float* h0_1, const float* dz1, float* dK1, float* dR1, float* db1, int T1, int F1,
                        const float* x2, const float* hs2, const float* h0_2, const float* dz2, float* dK2, float* dR2, float* db2, int T2, int F2,
                        int B, int H, int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (B > 0 && T1 > 0 && T2 > 0 && lstm_seq_wgrad_rows(0, B, T1, F1, H, dz1, dK1, dR1, db1) && lstm_seq_wgrad_rows(0, B, T2, F2, H, dz2, dK2, dR2, db2)) {
        const float* xs[2] = {x1, x2};
        const int Fs[2] = {F1, F2}, Ts[2] = {T1, T2};
        const float* hss[2] = {hs1, hs2};
        const float* h0s[2] = {h0_1, h0_2};
        const float* dzs[2] = {dz1, dz2};
        float* dKs[2] = {dK1, dK2};
        float* dRs[2] = {dR1, dR2};
        float* dbs[2] = {db1, db2};
        return wgrad_rows_layers(2, xs, Fs, Ts, hss, h0s, dzs, dKs, dRs, dbs, B, H, accumulate, stream);
    }
    int rc = lstm_seq_wgrad(x1, hs1, h0_1, dz1, dK1, dR1, db1, B, T1, F1, H, accumulate, 0, scratch, scratch_floats, stream);
    if (rc) return rc;
    return lstm_seq_wgrad(x2, hs2, h0_2, dz2, dK2, dR2, db2, B, T2, F2, H, accumulate, 0, scratch, scratch_floats, stream);
}

// Weight gradients of the layers of a STACK (Fov_seq2seq_2layers.py:232-272: up to four layers that share the batch and the width,
// each with its own input width and time length) from their dz tapes.  One launch (wgrad_rows_kernel) when the few-row form takes
// every layer; else a lstm_seq_wgrad per layer.  A workgroup of that kernel owns one output tile of one problem whatever else
// shares the launch, so both ways give the bits of the per-layer calls.
int lstm_seq_wgrad_layers(int L, const float* const* x, const int* F, const int* T, const float* const* hs, const float* const* h0,
                          const float* const* dz, float* const* dK, float* const* dR, float* const* db, int B, int H, int accumulate,
                          float* scratch, size_t scratch_floats, hipStream_t stream) {
    bool rows_form = B > 0;
    for (int l = 0; l < L && rows_form; ++l) rows_form = T[l] > 0 && lstm_seq_wgrad_rows(0, B, T[l], F[l], H, dz[l], dK[l], dR[l], db[l]);
    if (rows_form) return wgrad_rows_layers(L, x, F, T, hs, h0, dz, dK, dR, db, B, H, accumulate, stream);
    for (int l = 0; l < L; ++l)
        if (int rc = lstm_seq_wgrad(x[l], hs[l], h0[l], dz[l], dK[l], dR[l], db[l], B, T[l], F[l], H, accumulate, 0, scratch, scratch_floats, stream))
            return rc;
    return FOV_OK;
}

// BPTT of one layer.  dz:(B,T,4H) is an output (kept: the caller may need it for dx of the layer
// below).  dK,dR,db are overwritten (accumulate = 0) or added to (accumulate = 1).
int lstm_seq_bwd(const float* x, const float* K, const float* R, const float* h0, const float* c0, const float* hs,
                 const float* reserve, const float* dhs, const float* dhT, const float* dcT, float* dz, float* dx,
                 float* dK, float* dR, float* db, float* dh0, float* dc0, int B, int T, int F, int H, int act,
                 int accumulate, float* ws, size_t ws_floats, hipStream_t stream, int bf16) {
    if (bf16 && H != 256) { set_error("lstm_seq_bwd: the bf16 path is built for H = 256"); return FOV_ERR_UNSUPPORTED; }
    if (ws_floats < lstm_bwd_workspace_floats(B, T, F, H)) { set_error("lstm_seq_bwd: workspace too small"); return FOV_ERR_WORKSPACE; }
    if (T == 0) {
        if (!accumulate)
            if (int rc = zero_lstm_wgrads(dK, dR, db, F, H, stream)) return rc;
        const size_t bh0 = sizeof(float) * (size_t)B * H;
        if (dh0) (void)(dhT ? hipMemcpyAsync(dh0, dhT, bh0, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dh0, 0, bh0, stream));
        if (dc0) (void)(dcT ? hipMemcpyAsync(dc0, dcT, bh0, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dc0, 0, bh0, stream));
        return FOV_OK;
    }
    const bool wide16 = !bf16 && bwd16_takes(B, H) && (((uintptr_t)R) & 15) == 0;   // width 512, small batches at 128 / 256: lstm_bwd16.hip
    const bool persistent = (bwd_cluster_shape_ok(H) || wide16) && !env_knobs().bwd_stepped;
    bool fuse_kr = false, fuse_r = false, dx_in_kernel = false, grouped = false, rows_form = false;
    const size_t head = (kStatusBytes + kXchBytes) / sizeof(float);
    float* dh_rec = ws + head;
    float* dc = dh_rec + (size_t)B * H;
    float* scratch = dc + (size_t)B * H;
    const size_t scratch_floats = ws_floats - head - (size_t)2 * B * H;
    const size_t bh = sizeof(float) * (size_t)B * H;
    hipError_t e = hipSuccess;
    if (persistent) {
        // one launch for the whole recurrence: dz (B,T,4H), dh0, dc0
        // bias gradient: per-tile partials from the kernel (db_part lives in the split-K scratch), summed below
        // dK, dR, db adjacent (a trainer's flat gradient buffer): ONE product [x | h_{t-1} | 1]^T dz (h_{-1} = 0; a given initial
        // state adds its h0^T dz_0 afterwards)
        // below gives all three (no bias partials from the kernel, no column-sum launches); F too narrow for a row tile:
        // [h_{t-1} | 1]^T dz gives dR and db
        lstm_seq_wgrad_fusion(x, hs, dz, dK, dR, db, T, F, H, &fuse_kr, &fuse_r);
        rows_form = lstm_seq_wgrad_rows(bf16, B, T, F, H, dz, dK, dR, db);
        grouped = rows_form || lstm_seq_wgrad_grouped(bf16, B, T, H, dz, dK, dR, db);
        if (grouped) fuse_kr = fuse_r = false;
        float* db_part = (db && !fuse_kr && !fuse_r && !grouped) ? scratch : nullptr;
        // bf16, 256-wide input (the stacked layer): the BPTT kernel forms dx = dz K^T from the dz tile it has gathered anyway
        dx_in_kernel = bf16 && dx && F == 256 && (((uintptr_t)K) & 15) == 0 && !env_knobs().no_dx_fusion;
        // fp32 on the eight-workgroup kernel (round 5): every workgroup forms its gate columns' share of dx in the shadow of the
        // exchange; eight partial tapes in the scratch, one reduce launch (was: a GEMM + reduce behind the recurrence)
        const bool on_bwd8 = !wide16 && !bf16 && bwd8_preferred(B, H) && !env_knobs().bwd_groups4;
        float* dx_parts = nullptr;
        if (on_bwd8 && dx && F == 256 && (((uintptr_t)K) & 15) == 0 && (((uintptr_t)dx) & 15) == 0 && !env_knobs().no_dx_fusion) {
            const size_t off = ((size_t)((B + 15) / 16) * 4 * H + 63) & ~(size_t)63;      // behind the db partials
            if (off + (size_t)8 * B * T * 256 <= scratch_floats) { dx_parts = scratch + off; dx_in_kernel = true; }
        }
        // H = 256: groups of eight workgroups fill the chip up to 32 tiles (the 4-group kernel leaves half of it idle
        // at 512 sequences); bf16 operands exist in the 8-group kernel only
        if (env_knobs().dbg_trace) fprintf(stderr, "[fov trace] lstm_seq_bwd B=%d T=%d F=%d H=%d wide16=%d fuse_kr=%d fuse_r=%d grouped=%d acc=%d: recurrence next\n", B, T, F, H, (int)wide16, (int)fuse_kr, (int)fuse_r, (int)grouped, accumulate);
        int rc = wide16 ? launch_bwd16(R, reserve, c0, dhs, dhT, dcT, dz, dh0 ? dh0 : dh_rec, dc0 ? dc0 : dc, db_part, B, T, H, act, ws, stream)
                 : (bf16 || (bwd8_preferred(B, H) && !env_knobs().bwd_groups4))
                     ? launch_bwd8(R, reserve, c0, dhs, dhT, dcT, dz, dh0 ? dh0 : dh_rec, dc0 ? dc0 : dc, db_part, B, T, act, bf16, ws, stream,
                                   dx_in_kernel ? K : nullptr, dx_in_kernel ? (dx_parts ? dx_parts : dx) : nullptr)
                     : launch_bwd_cluster(R, reserve, c0, dhs, dhT, dcT, dz, dh0 ? dh0 : dh_rec, dc0 ? dc0 : dc, db_part, B, T, H,
                                          act, ws, stream);
        if (rc) return rc;
        if (dx_parts) {      // dx = the eight workgroups' shares in slice order (before anything else touches the scratch)
            rc = splitk_reduce(dx_parts, dx, (long)B * T * 256, 8, 0, stream);
            if (rc) return rc;
        }
        if (env_knobs().dbg_trace) fprintf(stderr, "[fov trace] lstm_seq_bwd: recurrence done\n");
        if (db_part) {
            const int tiles = (B + 15) / 16;
            if ((size_t)tiles * 4 * H + (size_t)256 * 4 * H > scratch_floats) { set_error("lstm_seq_bwd: scratch too small for db"); return FOV_ERR_WORKSPACE; }
            rc = colsum(db_part, db, tiles, 4 * H, accumulate, scratch + (size_t)tiles * 4 * H,
                        scratch_floats - (size_t)tiles * 4 * H, stream);
            if (rc) return rc;
        }
    } else {
        e = dhT ? hipMemcpyAsync(dh_rec, dhT, bh, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dh_rec, 0, bh, stream);
        if (e == hipSuccess) e = dcT ? hipMemcpyAsync(dc, dcT, bh, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dc, 0, bh, stream);
        if (e != hipSuccess) { set_error("lstm_seq_bwd init: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
        const long nelem = (long)B * H;
        const dim3 pgrid((unsigned)((nelem + 255) / 256));
        const auto pointwise = act == FOV_ACT_HARD_SIGMOID ? lstm_bwd_pointwise<FOV_ACT_HARD_SIGMOID> : lstm_bwd_pointwise<FOV_ACT_SIGMOID>;
        for (int t = T - 1; t >= 0; --t) {
            hipLaunchKernelGGL(pointwise, pgrid, dim3(256), 0, stream, reserve, c0, dhs, dh_rec, dc, dz, B, T, H, t);
            int rc = launch_check("lstm_bwd_pointwise");
            if (rc) return rc;
            // dh_rec (B,H) = dz_t (B,4H) . R^T :  A(m,k) = dz[m][t][k], B(k,n) = R[n][k]
            rc = gemm_f32(gemm_nt(dz + (size_t)t * 4 * H, (long)T * 4 * H, R, 4 * H, dh_rec, H, B, H, 4 * H), 0, scratch, scratch_floats, stream);
            if (rc) return rc;
        }
        if (dh0) { e = hipMemcpyAsync(dh0, dh_rec, bh, hipMemcpyDeviceToDevice, stream); if (e != hipSuccess) { set_error("dh0 copy"); return FOV_ERR_LAUNCH; } }
        if (dc0) { e = hipMemcpyAsync(dc0, dc, bh, hipMemcpyDeviceToDevice, stream); if (e != hipSuccess) { set_error("dc0 copy"); return FOV_ERR_LAUNCH; } }
    }
    int rc = grouped ? wgrad_few_rows(rows_form, x, hs, h0, dz, dK, dR, db, B, T, F, H, accumulate, stream)
                     : lstm_seq_weight_products(x, hs, h0, dz, dK, dR, db, B, T, F, H, accumulate, bf16, fuse_kr, fuse_r, /*db_done=*/persistent,
                                                scratch, scratch_floats, stream);
    if (rc) return rc;
    if (dx && !dx_in_kernel) {   // dx (B*T,F) = dz . K^T : A(m,k) = dz[m][k], B(k,n) = K[n][k]
        const long BT = (long)B * T;
        rc = (bf16 && (((uintptr_t)K) & 15) == 0) ? gemm_bf16_nt(dz, 4 * H, K, 4 * H, dx, F, (int)BT, F, 4 * H, stream)
                                                 : gemm_f32(gemm_nt(dz, 4 * H, K, 4 * H, dx, F, (int)BT, F, 4 * H), 0, scratch, scratch_floats, stream);
        if (rc) return rc;
    }
    return FOV_OK;
}

// BPTT of two stacked width-512 layers in ONE launch (lstm_bwd16.hip: both recurrences and dx = dz2 . K2^T between them as three
// roles of one persistent kernel), then the two layers' weight-gradient products.  Same outputs as two lstm_seq_bwd calls
// (upper layer first, its dx as the lower layer's dhs) except that the intermediate dx is not materialised.
size_t lstm_stack2_bwd_workspace_floats(int B, int T, int F, int H) {
    const size_t tiles = (size_t)(B + 15) / 16;
    return lstm_bwd_workspace_floats(B, T, F > H ? F : H, H) + 2 * tiles * 4 * H + (size_t)4 * B * H + 64;
}

int lstm_stack2_bwd(const float* x, const float* R1, const float* K2, const float* R2, const float* h0_1, const float* c0_1,
                    const float* h0_2, const float* c0_2, const float* hs1, const float* res1, const float* hs2, const float* res2,
                    const float* dhs2, const float* dhT2, const float* dcT2, const float* dhT1, const float* dcT1, float* dz1, float* dz2,
                    float* dK1, float* dR1, float* db1, float* dK2, float* dR2, float* db2, float* dh0_1, float* dc0_1, float* dh0_2,
                    float* dc0_2, int B, int T, int F, int H, int act, int accumulate, float* ws, size_t ws_floats, hipStream_t stream) {
    if (!bwd16_pair_shape(B, T, H)) { set_error("lstm_stack2_bwd: unsupported shape (H = 512, <= 32 sequences on 256 CUs)"); return FOV_ERR_UNSUPPORTED; }
    if (ws_floats < lstm_stack2_bwd_workspace_floats(B, T, F, H)) { set_error("lstm_stack2_bwd: workspace too small"); return FOV_ERR_WORKSPACE; }
    const size_t head = (kStatusBytes + kXchBytes) / sizeof(float);
    const size_t tiles = (size_t)(B + 15) / 16, bh = (size_t)B * H;
    float* dbp2 = ws + head;
    float* dbp1 = dbp2 + tiles * 4 * H;
    float* spare = dbp1 + tiles * 4 * H;          // state gradients the caller does not ask for
    float* scratch = spare + 4 * bh;
    const size_t scratch_floats = ws_floats - head - 2 * tiles * 4 * H - 4 * bh;
    bool kr1, r1, kr2, r2;
    lstm_seq_wgrad_fusion(x, hs1, dz1, dK1, dR1, db1, T, F, H, &kr1, &r1);
    lstm_seq_wgrad_fusion(hs1, hs2, dz2, dK2, dR2, db2, T, H, H, &kr2, &r2);
    // few rows: ALL weight gradients of both layers in one launch behind the recurrences (wgrad_group.hip)
    const bool rows_form = lstm_seq_wgrad_rows(0, B, T, F, H, dz1, dK1, dR1, db1) && lstm_seq_wgrad_rows(0, B, T, H, H, dz2, dK2, dR2, db2);
    const bool grouped = rows_form || (lstm_seq_wgrad_grouped(0, B, T, H, dz1, dK1, dR1, db1) && lstm_seq_wgrad_grouped(0, B, T, H, dz2, dK2, dR2, db2));
    if (grouped) kr1 = r1 = kr2 = r2 = true;      // (no bias partials from the kernel)
    float* db_part1 = (db1 && !kr1 && !r1) ? dbp1 : nullptr;
    float* db_part2 = (db2 && !kr2 && !r2) ? dbp2 : nullptr;
    int rc = launch_bwd16_pair(R2, K2, res2, c0_2, dhs2, dhT2, dcT2, dz2, dh0_2 ? dh0_2 : spare, dc0_2 ? dc0_2 : spare + bh, db_part2, R1,
                               res1, c0_1, dhT1, dcT1, dz1, dh0_1 ? dh0_1 : spare + 2 * bh, dc0_1 ? dc0_1 : spare + 3 * bh, db_part1, B,
                               T, act, ws, stream);
    if (rc) return rc;
    if (grouped) {
        const float* xs[2] = {x, hs1};
        const int Fs[2] = {F, H};
        const float* hss[2] = {hs1, hs2};
        const float* h0s[2] = {h0_1, h0_2};
        const float* dzs[2] = {dz1, dz2};
        float* dKs[2] = {dK1, dK2};
        float* dRs[2] = {dR1, dR2};
        float* dbs[2] = {db1, db2};
        const int Ts[2] = {T, T};
        return rows_form ? wgrad_rows_layers(2, xs, Fs, Ts, hss, h0s, dzs, dKs, dRs, dbs, B, H, accumulate, stream)
                         : wgrad_group_layers(2, xs, Fs, hss, h0s, dzs, dKs, dRs, dbs, B, T, H, accumulate, stream);
    }
    for (int l = 2; l >= 1; --l) {
        float* part = l == 2 ? db_part2 : db_part1;
        float* db = l == 2 ? db2 : db1;
        if (part) {
            if (tiles * 4 * H + (size_t)256 * 4 * H > scratch_floats) { set_error("lstm_stack2_bwd: scratch too small for db"); return FOV_ERR_WORKSPACE; }
            rc = colsum(part, db, (long)tiles, 4 * H, accumulate, scratch, scratch_floats, stream);
            if (rc) return rc;
        }
        rc = l == 2 ? lstm_seq_weight_products(hs1, hs2, h0_2, dz2, dK2, dR2, db2, B, T, H, H, accumulate, 0, kr2, r2, true, scratch, scratch_floats, stream)
                    : lstm_seq_weight_products(x, hs1, h0_1, dz1, dK1, dR1, db1, B, T, F, H, accumulate, 0, kr1, r1, true, scratch, scratch_floats, stream);
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
