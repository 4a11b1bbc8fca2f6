// Fused seq2seq inference with bf16 matrix-core operands: the encoder LSTM over T_in steps from a zero state, then T_out
// autoregressive decoder steps - LSTM step, Dense(F_dec, tanh), the output fed back as the next input - in ONE persistent
// launch.  The bf16 form of fov_seq2seq_decode_fwd (replaces the host loop of mycode/FoV_seq2seq.py:137-178, batched).
//
//   encoder, t < T_in:   h, c = LSTM_enc(x_t; h, c)                         K:(F_enc,4H)  R:(H,4H)
//   decoder, s < T_out:  h, c = LSTM_dec(x_s; h, c)                         K:(F_dec,4H)  R:(H,4H)
//                        y_s = tanh(h . W + b);  x_{s+1} = y_s;  x_0 = dec_in0
//
// Ownership, exchange and tile loop are lstm_layer_bf16.hip's (a 16-sequence tile per group of QG = 8 workgroups,
// workgroup `slice` owns hidden units [32 slice, +32), one {bf16 pair, epoch} granule per lane and exchanged step), and
// an encoder step is that kernel's step.  A decoder step is mix_decoder_bf16.hip's layer 1 plus its Dense head: wave w
// contracts units [64 w, 64 w + 64) of the gathered h tile and the four partial products meet in LDS; every wave then sums
// them itself for the x_{s+1} fragment it needs, so no barrier guards the fed-back input.  The gate pre-activations keep
// the layer kernel's order - bias, then x . K, then h . R - so a decoder step equals one fov_lstm_seq_fwd_bf16 step bit for
// bit, and the head equals fov_dense_fwd_bf16 (below).  State passes from the encoder to the decoder in registers (c, h)
// and in LDS (the gathered h tile).  All four weight sets stay register-resident from the prologue: encoder K + R
// (24 or 64 + 64 registers per lane), decoder K + R (8 + 64), Dense (8).
#include <stdlib.h>

#include "bf16_common.h"

namespace fov {

namespace {

// NKB / XVEC: the encoder input's k-blocks and x staging, as lstm_layer_bf16_kernel
template <int ACT, int NKB, bool XVEC>
__global__ __launch_bounds__(256, 1) void s2s_bf16_kernel(LstmParams p) {
    __shared__ __attribute__((aligned(16))) unsigned short sH[QBT * QLD];
    __shared__ __attribute__((aligned(16))) unsigned short sX[2 * QBT * QLD];
    __shared__ float sPart[4 * 256];   // [4 waves][16 rows][16 cols] partial Dense products
    __shared__ int sFlag[4];
    __shared__ __attribute__((aligned(16))) unsigned sStage[QST_LDS_WORDS];   // the prologue's weight staging (bf16_common.h)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int T_in = p.T, T_out = p.T_out, S = T_in + T_out, O = p.F_dec;
    const bool xch_used = T_out > 0 || T_in > 1;   // an h_t some later step reads
    int group, slice;
    if (!q_group_slice(p.num_groups, group, slice)) { q_spare_leaves(p.status, xch_used); return; }
    const int F = p.F;
    const int unit = 32 * slice + 8 * wave + (n & 7);
    const int hi = n >> 3;
    const int col0 = hi * QH + unit, col1 = (2 + hi) * QH + unit;   // gate columns of N-tile 0 ([i | f]) / 1 ([g | o])
    constexpr int H4 = 4 * QH;
    __shared__ unsigned sXch[4];
    const XchHeader header = xch_arrive_request(p.status, xch_used);
    const unsigned timeout_word = xch_timeout_word(p.status);

    // ---- resident weights: packed bf16 B fragments ----
    qu32x4 wk[NKB][2], wr[8][2], wkd[1][2], wrd[8][2], wd[2];
    load_weight_set<1>(wkd, p.dK, H4, O, g4, col0, col1);   // decoder K (F_dec <= 8 rows): one zero-padded k-block
    stage_weight_sets(wk, p.K, F, wr, p.R, QH, wrd, p.dR, QH, H4, slice, sStage, [&]() {
        xch_arrive_commit(p.status, sXch, header, group, slice, xch_used);
        for (int i = tid; i < 2 * QBT * QLD; i += 256) sX[i] = 0;   // columns >= F stay zero
    });
    const bool poisoned = xch_timeout_set(timeout_word) && xch_used;
    if (tid == 0) sFlag[0] = poisoned ? 1 : 0;
    const float bv[2] = {p.b[col0], p.b[col1]}, bdv[2] = {p.db[col0], p.db[col1]};
    // Dense kernel: wave w contracts hidden units [64w, 64w + 64) = k-blocks 2w, 2w + 1; column n = output (zero for n >= O)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (n < O) ? p.dW[(size_t)(32 * (2 * wave + q) + 8 * g4 + j) * O + n] : 0.f;
        wd[q] = (qu32x4){pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
    }
    float ybias[8];   // Dense bias of the outputs j of the row this lane feeds back (g4 == 0)
#pragma unroll
    for (int j = 0; j < 8; ++j) ybias[j] = (j < O) ? p.dbias[j] : 0.f;

    // ---- exchange bookkeeping ----
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        p.xch + (size_t)group * 2 * (Q_TILE_BYTES / 8), 0, (int)(2 * Q_TILE_BYTES), 0x00020000);
    const int my_row0 = 4 * g4 + 2 * hi;   // this lane's cells: rows my_row0, +1 of `unit`
    const unsigned pub_off = (unsigned)((my_row0 >> 1) * QH + unit) * 8u;
    if (xch_used) xch_hello_poll(p.status, sXch, group, QG, &sFlag[0]);
    __syncthreads();
    XchTicket ticket = {0u, 0u, false};
    if (xch_used) ticket = xch_ticket(sXch);
    unsigned epoch = ticket.base;
    bool aborted = sFlag[0] != 0;
    if (xch_used && tid == 0 && !ticket.same_xcd && !aborted) xch_count_safe(p.status, ticket);   // (fov_exchange_mode)

    const int xrw = tid >> 4, xc = tid & 15;
    constexpr int NXE = XVEC ? NKB / 2 : 2 * NKB;
    const int nx4 = F >> 2;
    QGather gq;
    for (int tile = group; tile < p.num_tiles && !aborted; tile += p.num_groups) {
        const int b0 = tile * QBT;
        __syncthreads();   // previous tile fully consumed
        constexpr unsigned OORB = 0x80000000u;
        const int live_rows = p.B - b0 < QBT ? p.B - b0 : QBT;
        const __amdgpu_buffer_rsrc_t xgrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.x + (size_t)b0 * T_in * F), 0, live_rows * T_in * F * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t d0rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.dec_in0 + (size_t)b0 * O), 0, live_rows * O * 4, 0x00020000);
        for (int e = tid; e < QBT * QH; e += 256) sH[(e >> 8) * QLD + (e & 255)] = 0;   // zero initial state
        float c[2] = {0.f, 0.f}, hc[2] = {0.f, 0.f};
        // x_0 of the decoder as this lane's A fragment: row n, k = 8 g4 + j (only g4 == 0 carries data)
        qu32x4 xa;
        {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(d0rs, (g4 == 0 && j < O) ? (unsigned)((n * O + j) * 4) : OORB, 0, 0));
            xa = (qu32x4){pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
        }
        // ================= encoder: lstm_layer_bf16_kernel's step =================
        unsigned xoff[NXE];
#pragma unroll
        for (int i = 0; i < NXE; ++i) {
            if constexpr (XVEC) xoff[i] = (xc + 16 * i < nx4) ? (unsigned)((xrw * T_in * F + 4 * xc + 64 * i) * 4) : OORB;
            else xoff[i] = (xc + 16 * i < F) ? (unsigned)((xrw * T_in * F + xc + 16 * i) * 4) : OORB;
        }
        auto load_x4 = [&](int i, int t) {
            const qu32x4 q = __builtin_amdgcn_raw_buffer_load_b128(xgrs, xoff[i], (unsigned)(t * F * 4), 0);
            return (f32x4){__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]), __uint_as_float(q[3])};
        };
        auto load_x1 = [&](int i, int t) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xgrs, xoff[i], (unsigned)(t * F * 4), 0)); };
        unsigned short* xl = sX + xrw * QLD + (XVEC ? 4 : 1) * xc;
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        if (T_in > 0) {
            f32x4 v4[2][XVEC ? NXE : 1];
            float v1[2][XVEC ? 1 : NXE];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int i = 0; i < NXE; ++i) {
                    const int tc = tt < T_in ? tt : 0;
                    if constexpr (XVEC) v4[tt][i] = load_x4(i, tc);
                    else v1[tt][i] = load_x1(i, tc);
                }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int i = 0; i < NXE; ++i) {
                    if constexpr (XVEC) {
                        if (xc + 16 * i < nx4)
                            *(qu32x2*)(xl + tt * QBT * QLD + 64 * i) = (qu32x2){pack_bf16(v4[tt][i][0], v4[tt][i][1]), pack_bf16(v4[tt][i][2], v4[tt][i][3])};
                    } else {
                        if (xc + 16 * i < F) xl[tt * QBT * QLD + 16 * i] = bf16_bits(v1[tt][i]);
                    }
                }
        }
        __syncthreads();
        f32x4 acc[2];
        acc[0] = (f32x4){bv[0], bv[0], bv[0], bv[0]};
        acc[1] = (f32x4){bv[1], bv[1], bv[1], bv[1]};
        if (T_in > 0) {
            qmm<0, NKB, NKB>(acc, sX, n, g4, wk);
            qmm<0, 8, 8>(acc, sH, n, g4, wr);
        }
        f32x4 xr[XVEC ? NXE : 1];
        float xs[XVEC ? 1 : NXE];
#pragma unroll
        for (int i = 0; i < (XVEC ? NXE : 1); ++i) xr[i] = z4;
#pragma unroll
        for (int i = 0; i < (XVEC ? 1 : NXE); ++i) xs[i] = 0.f;
        for (int t = 0; t < T_in; ++t) {
            if (t > 0 && t + 1 < T_in) {
                unsigned short* xb = xl + ((t + 1) & 1) * QBT * QLD;
#pragma unroll
                for (int i = 0; i < NXE; ++i) {
                    if constexpr (XVEC) {
                        if (xc + 16 * i < nx4) *(qu32x2*)(xb + 64 * i) = (qu32x2){pack_bf16(xr[i][0], xr[i][1]), pack_bf16(xr[i][2], xr[i][3])};
                    } else {
                        if (xc + 16 * i < F) xb[16 * i] = bf16_bits(xs[i]);
                    }
                }
            }
            if (t + 2 < T_in) {
#pragma unroll
                for (int i = 0; i < NXE; ++i) {
                    if constexpr (XVEC) xr[i] = load_x4(i, t + 2);
                    else xs[i] = load_x1(i, t + 2);
                }
            }
            {
                float zi[2], zf[2], zg[2], zo[2];
                gates_of_lane(acc, hi, zi, zf, zg, zo);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const float ig = rec_act<ACT>(zi[r]), fg = rec_act<ACT>(zf[r]), gg = tanh_f(zg[r]), og = rec_act<ACT>(zo[r]);
                    c[r] = fmaf(fg, c[r], ig * gg);
                    hc[r] = og * tanh_f(c[r]);
                }
            }
            const bool more = (t + 1 < T_in);   // another encoder step
            const bool keep = (t + 1 < S);      // h_t is read by a later step (after the last encoder step: the decoder's first)
            unsigned par = 0;
            const unsigned hpair = pack_bf16(hc[0], hc[1]);
            if (keep) {
                ++epoch;
                par = (epoch & 1u) * Q_TILE_BYTES;
                XCH_STORE_B64(ticket.same_xcd, ((qu32x2){hpair, epoch}), xrs, pub_off, par);
            }
            __syncthreads();   // barrier 1: every wave is done reading sH; x_{t+1} is in LDS
            if (keep) {
                sH[my_row0 * QLD + unit] = (unsigned short)(hpair & 0xffffu);
                sH[(my_row0 + 1) * QLD + unit] = (unsigned short)(hpair >> 16);
            }
            acc[0] = (f32x4){bv[0], bv[0], bv[0], bv[0]};
            acc[1] = (f32x4){bv[1], bv[1], bv[1], bv[1]};
            if (more) qmm<0, NKB, NKB>(acc, sX + ((t + 1) & 1) * QBT * QLD, n, g4, wk);
            if (keep) {
                q_gather_issue(gq, xrs, par, slice, tid);
                if (!q_gather_finish(gq, xrs, par, slice, tid, epoch, sH, p.status)) sFlag[0] = 1;
            }
            __syncthreads();   // barrier 2: the whole h_t tile is in LDS
            if (sFlag[0]) { aborted = true; break; }
            if (more) qmm<0, 8, 8>(acc, sH, n, g4, wr);
        }
        // ================= decoder =================
        for (int s = 0; s < T_out && !aborted; ++s) {
            // pre-activations in the layer kernel's order: bias, x_s . K_dec, h_{s-1} . R_dec
            acc[0] = (f32x4){bdv[0], bdv[0], bdv[0], bdv[0]};
            acc[1] = (f32x4){bdv[1], bdv[1], bdv[1], bdv[1]};
            qmfma(acc[0], xa, wkd[0][0]);
            qmfma(acc[1], xa, wkd[0][1]);
            qmm<0, 8, 8>(acc, sH, n, g4, wrd);
            {
                float zi[2], zf[2], zg[2], zo[2];
                gates_of_lane(acc, hi, zi, zf, zg, zo);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const float ig = rec_act<ACT>(zi[r]), fg = rec_act<ACT>(zf[r]), gg = tanh_f(zg[r]), og = rec_act<ACT>(zo[r]);
                    c[r] = fmaf(fg, c[r], ig * gg);
                    hc[r] = og * tanh_f(c[r]);
                }
            }
            ++epoch;
            const unsigned par = (epoch & 1u) * Q_TILE_BYTES;
            const unsigned hpair = pack_bf16(hc[0], hc[1]);
            XCH_STORE_B64(ticket.same_xcd, ((qu32x2){hpair, epoch}), xrs, pub_off, par);
            __syncthreads();   // barrier 1: every wave is done reading sH (and the previous step's partials)
            sH[my_row0 * QLD + unit] = (unsigned short)(hpair & 0xffffu);
            sH[(my_row0 + 1) * QLD + unit] = (unsigned short)(hpair >> 16);
            q_gather_issue(gq, xrs, par, slice, tid);
            if (!q_gather_finish(gq, xrs, par, slice, tid, epoch, sH, p.status)) sFlag[0] = 1;
            __syncthreads();   // barrier 2: the whole h_s tile is in LDS
            if (sFlag[0]) { aborted = true; break; }
            // ---- head: y_s = tanh(h_s . W + b), the four 64-unit partials meet in LDS ----
            {
                f32x4 dacc = {0.f, 0.f, 0.f, 0.f};
                qmfma(dacc, lds_afrag(sH, n, g4, 2 * wave), wd[0]);
                qmfma(dacc, lds_afrag(sH, n, g4, 2 * wave + 1), wd[1]);
#pragma unroll
                for (int r = 0; r < 4; ++r) sPart[(wave * 16 + 4 * g4 + r) * 16 + n] = dacc[r];
            }
            __syncthreads();   // barrier 3: the four partials are in LDS
            {
                // every wave forms the x_{s+1} fragment it needs itself: lane (n, g4 = 0) takes y[row n][0..7]
                float y[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = 0.f;
                    if (g4 == 0 && j < O) {
                        v = sPart[n * 16 + j] + sPart[(16 + n) * 16 + j] + sPart[(32 + n) * 16 + j] + sPart[(48 + n) * 16 + j];
                        v = tanh_f(v + ybias[j]);
                    }
                    y[j] = v;
                }
                xa = (qu32x4){pack_bf16(y[0], y[1]), pack_bf16(y[2], y[3]), pack_bf16(y[4], y[5]), pack_bf16(y[6], y[7])};
                const int row = b0 + n;
                if (slice == 0 && wave == 0 && g4 == 0 && row < p.B) {
                    float* op = p.out + ((size_t)row * T_out + s) * O;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (j < O) op[j] = y[j];
                }
            }
        }
        if (!aborted) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int row = b0 + my_row0 + r;
                if (row < p.B) {
                    if (p.hT) p.hT[(size_t)row * QH + unit] = hc[r];
                    if (p.cT) p.cT[(size_t)row * QH + unit] = c[r];
                }
            }
        }
    }
    if (xch_used) xch_settle(p.status, ticket, (unsigned)p.epoch_span);
}

// Dense(Out) with bf16 operands, In <= 256, Out <= 16: one 16-row tile per workgroup, the fused kernel's head arithmetic
// (wave w: k-blocks 2w, 2w + 1 on the matrix pipe from 0; the four partials added in wave order, then the bias).
__global__ __launch_bounds__(256) void dense_bf16_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ b, float* __restrict__ y, int N, int In,
                                                         int Out, int act) {
    __shared__ __attribute__((aligned(16))) unsigned short sA[QBT * QLD];
    __shared__ float sPart[4 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int r0 = blockIdx.x * QBT;
    for (int e = tid; e < QBT * QH; e += 256) {
        const int row = e >> 8, k = e & 255;
        sA[row * QLD + k] = bf16_bits((r0 + row < N && k < In) ? x[(size_t)(r0 + row) * In + k] : 0.f);
    }
    qu32x4 wd[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * (2 * wave + q) + 8 * g4 + j;
            v[j] = (n < Out && k < In) ? W[(size_t)k * Out + n] : 0.f;
        }
        wd[q] = (qu32x4){pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
    }
    __syncthreads();
    f32x4 dacc = {0.f, 0.f, 0.f, 0.f};
    qmfma(dacc, lds_afrag(sA, n, g4, 2 * wave), wd[0]);
    qmfma(dacc, lds_afrag(sA, n, g4, 2 * wave + 1), wd[1]);
#pragma unroll
    for (int r = 0; r < 4; ++r) sPart[(wave * 16 + 4 * g4 + r) * 16 + n] = dacc[r];
    __syncthreads();
    const int row = tid >> 4, o = tid & 15;
    if (o < Out && r0 + row < N) {
        float v = sPart[row * 16 + o] + sPart[(16 + row) * 16 + o] + sPart[(32 + row) * 16 + o] + sPart[(48 + row) * 16 + o];
        v = v + (b ? b[o] : 0.f);
        y[(size_t)(r0 + row) * Out + o] = act ? tanh_f(v) : v;
    }
}

}  // namespace

bool s2s_bf16_shape_ok(int F_enc, int F_dec, int H) { return H == QH && F_enc >= 1 && F_enc <= 256 && F_dec >= 1 && F_dec <= 8; }

// p.status / p.xch point into the caller's workspace (header + the fixed granule area)
int launch_s2s_bf16(const LstmParams& p_in, hipStream_t stream) {
    LstmParams p = p_in;
    if (p.B == 0) return FOV_OK;
    if (!s2s_bf16_shape_ok(p.F, p.F_dec, p.H)) {
        set_error("bf16 seq2seq decode: H = 256, F_enc <= 256 and F_dec <= 8 only (got H=%d F_enc=%d F_dec=%d)", p.H, p.F, p.F_dec);
        return FOV_ERR_UNSUPPORTED;
    }
    p.num_tiles = (p.B + QBT - 1) / QBT;
    const int max_groups = device_cu_count() / QG;   // one workgroup per CU: every group must be co-resident
    if (max_groups < 1) { set_error("bf16 seq2seq decode needs at least %d CUs", QG); return FOV_ERR_UNSUPPORTED; }
    p.num_groups = p.num_tiles < max_groups ? p.num_tiles : max_groups;
    if ((size_t)p.num_groups * 2 * Q_TILE_BYTES > kXchBytes - kHelloBytes) { set_error("bf16 seq2seq decode: granule area too small"); return FOV_ERR_WORKSPACE; }
    p.epoch_span = (p.T + p.T_out) * ((p.num_tiles + p.num_groups - 1) / p.num_groups) + 1;
    if (int rc_ = xch_account(p.status, p.epoch_span, stream)) return rc_;
    const bool narrow = p.F <= 96;
    const bool xvec = !narrow && (p.F & 3) == 0 && (((uintptr_t)p.x) & 15) == 0;
    const bool hs_ = p.act == FOV_ACT_HARD_SIGMOID;
    void (*kern)(LstmParams) =
        narrow ? (hs_ ? s2s_bf16_kernel<FOV_ACT_HARD_SIGMOID, 3, false> : s2s_bf16_kernel<FOV_ACT_SIGMOID, 3, false>)
        : xvec ? (hs_ ? s2s_bf16_kernel<FOV_ACT_HARD_SIGMOID, 8, true> : s2s_bf16_kernel<FOV_ACT_SIGMOID, 8, true>)
               : (hs_ ? s2s_bf16_kernel<FOV_ACT_HARD_SIGMOID, 8, false> : s2s_bf16_kernel<FOV_ACT_SIGMOID, 8, false>);
    hipLaunchKernelGGL(kern, dim3(q_padded_groups(p.num_groups) * QG), dim3(256), 0, stream, p);
    return launch_check(narrow ? "bf16 seq2seq decode (narrow x)" : xvec ? "bf16 seq2seq decode (vector x)" : "bf16 seq2seq decode (scalar x)");
}

bool dense_bf16_shape_ok(int In, int Out) { return In >= 1 && In <= QH && Out >= 1 && Out <= 16; }

int launch_dense_bf16(const float* x, const float* W, const float* b, float* y, int N, int In, int Out, int act, hipStream_t stream) {
    if (N == 0) return FOV_OK;
    hipLaunchKernelGGL(dense_bf16_kernel, dim3((unsigned)(((long)N + QBT - 1) / QBT)), dim3(256), 0, stream, x, W, b, y, N, In, Out, act);
    return launch_check("bf16 dense");
}

}  // namespace fov
