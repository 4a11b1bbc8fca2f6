// The 2- and 3-layer target-only seq2seq LSTM (mycode/Fov_seq2seq_2layers.py:360-430, 3layers.py's loop, batched) in ONE launch:
// the L-layer encoder over T_in steps from zero states, then T_out autoregressive steps through the L decoder layers and the
// Dense(F_dec, tanh) head, each output fed back as the next input.  fp32 throughout (v_mfma_f32_16x16x4_f32, exact expf / tanhf).
//
//   encoder, t < T_in:   h_l, c_l = LSTM_enc_l(h_{l-1,t}; h_l, c_l)        h_{-1,t} = x_t      K_0:(F_enc,4H)  K_l, R_l:(H,4H)
//   decoder, s < T_out:  h_l, c_l = LSTM_dec_l(h_{l-1,s}; h_l, c_l)        h_{-1,s} = y_{s-1}  K_0:(F_dec,4H)
//                        y_s = tanh(h_{L-1,s} . W + b);  y_{-1} = dec_in0;  decoder layer l starts from encoder layer l's state
//
// Ownership.  One workgroup owns one tile of 16 sequences for every layer and every step; the grid is the number of tiles and
// workgroups never communicate: no exchange, no workspace, no wait.  The width runs at HP = 32 or 64 (narrower models zero-
// padded by the host, which is exact) on HP / 16 waves; wave w owns units [16 w, 16 w + 16) of all four gates of every layer.
// With the sequences as the M of the MFMA and a gate's 16 units as its N, lane (n, g4) holds the four pre-activations of unit
// 16 w + n for sequences 4 g4 .. 4 g4 + 3: the cell update is lane-local and c never leaves registers.
//
// Weights.  A (Kd, 4 HP) matrix is Kd registers per lane as B operands, w[j][s][g] = W[16 j + 4 g4 + s][g HP + unit] (the k
// order inside a 16-block is a permutation the A operand shares: one ds_read_b128 of a tile row feeds four k-steps).  The
// encoder holds R_0 and K_l, R_l (l >= 1) in registers and K_0 (F_enc <= 96 rows) in LDS in B-operand order; the decoder's set
// (K_0 has F_dec <= 8 rows) and the head's fragments replace them at the phase switch.  No weight load from global memory is
// inside a step loop.
//
// A layer-step.  Every layer's running h tile lies in LDS twice (step parity), so one barrier per layer-step is enough: a
// layer reads the tile below of this step and its own of the previous step, and writes its own of this step.  The gate
// pre-activations are summed in the order bias, x . K, h . R.  The head runs on the matrix core as y^T = W^T . h^T - the LDS
// read of h is the same as a layer's - which leaves y[sequence n][output 4 g4 + r] in register r of lane (n, g4): exactly the
// A fragment of the next step's layer 0, without LDS or memory in between.  Every wave computes the (tiny) head itself.
//
// Rows of a ragged last tile beyond B read zeros (masked, not clamped) and store nothing; MFMA rows are independent, so a
// sequence's result does not depend on its tile-mates or on its place in the batch.
#include "stacked_tile.h"

namespace fov {

namespace {

struct StackedParams {
    const float* x;         // (B, T_in, F)
    const float* dec_in0;   // (B, 1, O)
    const float *eK[3], *eR[3], *eb[3], *dK[3], *dR[3], *db[3];
    const float *dW, *dbias;
    float *out, *hT, *cT;   // (B, T_out, O); (L, B, HP) or NULL
    int B, T_in, T_out, F, O;
};

template <int HP, int L, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void stacked_s2s_kernel(StackedParams p) {
    extern __shared__ __attribute__((aligned(16))) float ss_smem[];
    constexpr int NT = 4 * HP, NJ = HP / 16, H4 = 4 * HP, LDH = ss_ldh(HP), HT = SS_BT * LDH;
    constexpr int XROWS = NT / 16, XP = SS_BT / XROWS;   // x staging: a thread loads column xc + 16 i of rows xrow + XROWS pp
    float* sH = ss_smem;                         // [3][2][16][LDH]
    float* sX = sH + 6 * HT;                     // [2][16][SS_LDX]
    f32x4* sK = (f32x4*)(sX + 2 * SS_BT * SS_LDX);   // [nkb][4][NT] {i, f, g, o} of input row 16 j + 4 g4 + s
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SS_BT;
    const int B = p.B, T_in = p.T_in, T_out = p.T_out, F = p.F, O = p.O;
    const int nkb = (F + 15) >> 4;
    const float* a_rd = sH + n * LDH + 4 * g4;          // + tile: this lane's A fragments
    float* h_wr = sH + 4 * g4 * LDH + unit;             // + tile: this lane's four h values (rows 4 g4 + r)

    for (int i = tid; i < 2 * L * HT; i += NT) sH[i] = 0.f;   // zero initial states
    float c[L][4], h[L][4];
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[l][r] = h[l][r] = 0.f;

    // ================= encoder =================
    if (T_in > 0) {
        float wR0[NJ][4][4], wK[L - 1][NJ][4][4], wR[L - 1][NJ][4][4], bias[L][4];
        load_frag<HP>(wR0, p.eR[0], unit, g4);
        load_bias<HP>(bias[0], p.eb[0], unit);
#pragma unroll
        for (int l = 1; l < L; ++l) {
            load_frag<HP>(wK[l - 1], p.eK[l], unit, g4);
            load_frag<HP>(wR[l - 1], p.eR[l], unit, g4);
            load_bias<HP>(bias[l], p.eb[l], unit);
        }
        {   // K_0 -> LDS; rows >= F lie past the descriptor and read as zero (the whole offset is in the vector register)
            const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.eK[0]), 0, F * H4 * 4, SS_RSRC);
            for (int j = 0; j < nkb; ++j)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned voff = (unsigned)(((16 * j + 4 * g4 + s) * H4 + unit) * 4);
                    f32x4 kv;
#pragma unroll
                    for (int g = 0; g < 4; ++g) kv[g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(krs, voff + (unsigned)(g * HP * 4), 0, 0));
                    sK[(j * 4 + s) * NT + tid] = kv;
                }
        }
        const int xrow = tid >> 4, xc = tid & 15;
        float xr[XP][SS_MAX_F / 16];
        auto load_x = [&](int t) {
#pragma unroll
            for (int pp = 0; pp < XP; ++pp)
#pragma unroll
                for (int i = 0; i < SS_MAX_F / 16; ++i) {
                    const int row = b0 + xrow + XROWS * pp, col = xc + 16 * i;
                    xr[pp][i] = (i < nkb && row < B && col < F) ? p.x[((size_t)row * T_in + t) * F + col] : 0.f;
                }
        };
        auto store_x = [&](float* dst) {   // columns F .. 16 nkb - 1 are written as zeros; none beyond is read
#pragma unroll
            for (int pp = 0; pp < XP; ++pp)
#pragma unroll
                for (int i = 0; i < SS_MAX_F / 16; ++i)
                    if (i < nkb) dst[(xrow + XROWS * pp) * SS_LDX + xc + 16 * i] = xr[pp][i];
        };
        load_x(0);
        store_x(sX);
        __syncthreads();
        for (int t = 0; t < T_in; ++t) {
            const int cur = t & 1, prv = cur ^ 1;
            const bool more = t + 1 < T_in;
            if (more) load_x(t + 1);
            f32x4 acc[4];
            {   // layer 0: bias, x_t . K_0 (LDS-resident), h . R_0
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[0][g], bias[0][g], bias[0][g], bias[0][g]};
                const float* xa = sX + cur * SS_BT * SS_LDX + n * SS_LDX + 4 * g4;
                for (int j = 0; j < nkb; ++j) {
                    const f32x4 av = *(const f32x4*)(xa + 16 * j);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const f32x4 kv = sK[(j * 4 + s) * NT + tid];
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], kv[g], acc[g], 0, 0, 0);
                    }
                }
                mm_frag<NJ>(acc, a_rd + prv * HT, wR0);
                cell_update<ACT>(acc, c[0], h[0], h_wr + cur * HT, LDH);
            }
            if (more) store_x(sX + prv * SS_BT * SS_LDX);
            __syncthreads();
#pragma unroll
            for (int l = 1; l < L; ++l) {
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[l][g], bias[l][g], bias[l][g], bias[l][g]};
                mm_frag<NJ>(acc, a_rd + (2 * (l - 1) + cur) * HT, wK[l - 1]);
                mm_frag<NJ>(acc, a_rd + (2 * l + prv) * HT, wR[l - 1]);
                cell_update<ACT>(acc, c[l], h[l], h_wr + (2 * l + cur) * HT, LDH);
                __syncthreads();
            }
        }
    } else {
        __syncthreads();
    }

    // ================= decoder =================
    if (T_out > 0) {
        float wK0[4][4], wR0[NJ][4][4], wK[L - 1][NJ][4][4], wR[L - 1][NJ][4][4], bias[L][4], wd[NJ][4], dbv[4], xa[4];
        {   // K_0: register r of the fed-back fragment is output 4 g4 + r, so k-step r contracts input rows 4 g4 + r (zero from O on)
            const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dK[0]), 0, O * H4 * 4, SS_RSRC);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    wK0[r][g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(krs, (unsigned)(((4 * g4 + r) * H4 + g * HP + unit) * 4), 0, 0));
        }
        load_frag<HP>(wR0, p.dR[0], unit, g4);
        load_bias<HP>(bias[0], p.db[0], unit);
#pragma unroll
        for (int l = 1; l < L; ++l) {
            load_frag<HP>(wK[l - 1], p.dK[l], unit, g4);
            load_frag<HP>(wR[l - 1], p.dR[l], unit, g4);
            load_bias<HP>(bias[l], p.db[l], unit);
        }
        // head as y^T = W^T . h^T: the A operand is W^T (row = output n, zero from O on), the B operand the h tile
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) wd[j][s] = (n < O) ? p.dW[(size_t)(16 * j + 4 * g4 + s) * O + n] : 0.f;
        const bool row_live = b0 + n < B;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool o_live = 4 * g4 + r < O;
            dbv[r] = o_live ? p.dbias[4 * g4 + r] : 0.f;
            xa[r] = (o_live && row_live) ? p.dec_in0[(size_t)(b0 + n) * O + 4 * g4 + r] : 0.f;
        }
        for (int s_ = 0; s_ < T_out; ++s_) {
            const int cur = (T_in + s_) & 1, prv = cur ^ 1;
            f32x4 acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[0][g], bias[0][g], bias[0][g], bias[0][g]};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[r], wK0[r][g], acc[g], 0, 0, 0);
            mm_frag<NJ>(acc, a_rd + prv * HT, wR0);
            cell_update<ACT>(acc, c[0], h[0], h_wr + cur * HT, LDH);
            __syncthreads();
#pragma unroll
            for (int l = 1; l < L; ++l) {
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[l][g], bias[l][g], bias[l][g], bias[l][g]};
                mm_frag<NJ>(acc, a_rd + (2 * (l - 1) + cur) * HT, wK[l - 1]);
                mm_frag<NJ>(acc, a_rd + (2 * l + prv) * HT, wR[l - 1]);
                cell_update<ACT>(acc, c[l], h[l], h_wr + (2 * l + cur) * HT, LDH);
                __syncthreads();
            }
            // ---- head: y_s = tanh(h_top . W + b), every wave for itself ----
            f32x4 yacc = {0.f, 0.f, 0.f, 0.f};
            const float* ht = a_rd + (2 * (L - 1) + cur) * HT;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 hv = *(const f32x4*)(ht + 16 * j);
#pragma unroll
                for (int s = 0; s < 4; ++s) yacc = __builtin_amdgcn_mfma_f32_16x16x4f32(wd[j][s], hv[s], yacc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) xa[r] = (4 * g4 + r < O) ? tanh_f(yacc[r] + dbv[r]) : 0.f;
            if (wave == 0 && row_live) {
                float* op = p.out + ((size_t)(b0 + n) * T_out + s_) * O + 4 * g4;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * g4 + r < O) op[r] = xa[r];
            }
        }
    }

    // every layer's final state of the last phase that ran
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = b0 + 4 * g4 + r;
            if (row < B) {
                if (p.hT) p.hT[((size_t)l * B + row) * HP + unit] = h[l][r];
                if (p.cT) p.cT[((size_t)l * B + row) * HP + unit] = c[l][r];
            }
        }
}

template <int HP, int L>
int launch_stacked(const StackedParams& p, int act, hipStream_t stream) {
    void (*kern)(StackedParams) = act == FOV_ACT_HARD_SIGMOID ? stacked_s2s_kernel<HP, L, FOV_ACT_HARD_SIGMOID> : stacked_s2s_kernel<HP, L, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)ss_lds_floats(HP, p.T_in > 0 ? (p.F + 15) / 16 : 0) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("stacked seq2seq decode");
}

}  // namespace

// pure arithmetic (and the knob): no device query
bool stacked_s2s_shape_ok(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L) {
    return B >= 0 && B <= kMaxTileBatch && T_in >= 0 && T_in <= kMaxTileBatch && T_out >= 0 && T_out <= kMaxTileBatch && (H == 32 || H == 64) && (L == 2 || L == 3) && F_enc >= 1 && F_enc <= SS_MAX_F &&
           F_dec >= 1 && F_dec <= 8;
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_stacked_seq2seq_decode_supported(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L) {
    return (!env_knobs().no_stacked_decode && stacked_s2s_shape_ok(B, T_in, T_out, F_enc, F_dec, H, L)) ? 1 : 0;
}

int fov_stacked_seq2seq_decode_fwd(const float* enc_in, const float* dec_in0, const float* enc0_K, const float* enc0_R,
                                   const float* enc0_b, const float* enc1_K, const float* enc1_R, const float* enc1_b,
                                   const float* enc2_K, const float* enc2_R, const float* enc2_b, const float* dec0_K,
                                   const float* dec0_R, const float* dec0_b, const float* dec1_K, const float* dec1_R,
                                   const float* dec1_b, const float* dec2_K, const float* dec2_R, const float* dec2_b,
                                   const float* dense_W, const float* dense_b, float* out, float* hT, float* cT, int B, int T_in,
                                   int T_out, int F_enc, int F_dec, int H, int L, int act, fov_stream_t stream) {
    if (!stacked_s2s_shape_ok(B, T_in, T_out, F_enc, F_dec, H, L)) {   // decided before any HIP call
        set_error("fov_stacked_seq2seq_decode_fwd: H = 32 or 64, L = 2 or 3, F_enc <= %d, F_dec <= 8 and non-negative sizes only "
                  "(got B=%d T_in=%d T_out=%d F_enc=%d F_dec=%d H=%d L=%d)", SS_MAX_F, B, T_in, T_out, F_enc, F_dec, H, L);
        return FOV_ERR_UNSUPPORTED;
    }
    StackedParams p = {};
    const float* w[2][3][3] = {{{enc0_K, enc0_R, enc0_b}, {enc1_K, enc1_R, enc1_b}, {enc2_K, enc2_R, enc2_b}},
                               {{dec0_K, dec0_R, dec0_b}, {dec1_K, dec1_R, dec1_b}, {dec2_K, dec2_R, dec2_b}}};
    bool missing = !dense_W || !dense_b;
    for (int l = 0; l < L; ++l) {
        for (int side = 0; side < 2; ++side)
            for (int k = 0; k < 3; ++k) missing = missing || !w[side][l][k];
        p.eK[l] = w[0][l][0]; p.eR[l] = w[0][l][1]; p.eb[l] = w[0][l][2];
        p.dK[l] = w[1][l][0]; p.dR[l] = w[1][l][1]; p.db[l] = w[1][l][2];
    }
    if (missing || (B > 0 && ((T_in > 0 && !enc_in) || (T_out > 0 && (!dec_in0 || !out)))) ||
        (act != FOV_ACT_SIGMOID && act != FOV_ACT_HARD_SIGMOID)) {
        set_error("fov_stacked_seq2seq_decode_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    p.x = enc_in; p.dec_in0 = dec_in0; p.dW = dense_W; p.dbias = dense_b; p.out = out; p.hT = hT; p.cT = cT;
    p.B = B; p.T_in = T_in; p.T_out = T_out; p.F = F_enc; p.O = F_dec;
    hipStream_t st = (hipStream_t)stream;
    if (H == 32) return L == 2 ? launch_stacked<32, 2>(p, act, st) : launch_stacked<32, 3>(p, act, st);
    return L == 2 ? launch_stacked<64, 2>(p, act, st) : launch_stacked<64, 3>(p, act, st);
}

}  // extern "C"
