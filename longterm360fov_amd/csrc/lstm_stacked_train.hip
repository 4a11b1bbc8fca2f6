// The 2- and 3-layer target-only seq2seq LSTM's TRAINING graph (mycode/Fov_seq2seq_2layers.py:232-272,332-343 and 3layers.py,
// teacher-forced, under model.fit) as ONE launch per direction: the forward with the training tapes, and the BPTT through both
// stacks.  fp32 throughout (v_mfma_f32_16x16x4_f32, exact expf / tanhf).  The Dense head, the loss and the weight gradients
// are not here: they are products over all steps (fov_dense_mse_head, fov_lstm_seq_wgrad_layers).
//
//   forward   encoder, t < T_in:   h_l, c_l = LSTM_enc_l(h_{l-1,t}; h_l, c_l)     h_{-1,t} = enc_in_t   from zero states
//             decoder, s < T_out:  h_l, c_l = LSTM_dec_l(h_{l-1,s}; h_l, c_l)     h_{-1,s} = dec_in_s   layer l from encoder layer l's state
//   backward  decoder layers L-1 .. 0, then encoder layers L-1 .. 0; a layer walks t = T-1 .. 0:
//             dh_t = d(input of layer l+1)_t [dhs_top at the top decoder layer, nothing at the top encoder layer] + dz_{t+1} . R_l^T
//             gate backward (lstm_cell_bwd: the derivative from the stored gate);  dx_t = dz_t . K_l^T for l >= 1
//             the decoder layer's (dh_0, dc_0) enters encoder layer l as (dh_T, dc_T)
//
// Ownership (both kernels): lstm_stacked_s2s.hip's.  One workgroup owns one tile of 16 sequences for every layer and every step;
// the grid is the number of tiles and workgroups never communicate: no exchange, no workspace header, no wait.  HP / 16 waves,
// lane (n, g4) holds unit 16 w + n for the sequences 4 g4 .. 4 g4 + 3: the cell update and the gate backward are lane-local, c
// and dc never leave registers.  Rows of a ragged last tile beyond B read zeros (masked, not clamped) and store nothing; MFMA
// rows are independent, so a sequence's result does not depend on its tile-mates or on its place in the batch.
//
// Forward.  The decode kernel's encoder phase, twice: the second one starts from the first one's states with K_0 of F_dec <= 8
// rows in registers and its input rows read from dec_in.  Every tape store is optional; with none of them but dec_top this is
// the inference forward.  No weight load from global memory is inside a step loop.
//
// Backward, layer by layer.  The teacher-forced graph has no feedback, so layer l-1 needs only layer l's dx over all t: one
// layer's [R^T | K^T] lies in LDS in B-operand order (lstm_selffed.hip's layout; 128 KB at HP = 64) next to the dz tile of the
// step.  The step-interleaved order would need every layer's transposes at once (320 KB at HP = 64, L = 3).  dx goes from layer l
// to layer l-1 through a plain (B, max T, HP) scratch: the lane that writes an element is the lane that reads it, one
// __syncthreads() (workgroup-scope release / acquire) between the layers orders the two.  No atomics, no spin.
//
// stack2_tile_bwd_kernel is the same layer walk for two stacked layers whose gradients come from outside (fov_lstm_stack2_bwd at
// H = 32 / 64: the encoder of the others-mixing and others-context models under a decoder with kernels of its own).
#include "stacked_tile.h"

namespace fov {

namespace {

struct StackedTrainFwdParams {
    const float *x, *dec_in;            // (B, T_in, F), (B, T_out, O)
    const float *eK[3], *eR[3], *eb[3], *dK[3], *dR[3], *db[3];
    float *enc_hs, *enc_res, *dec_hs, *dec_res;   // (L, B, T, HP), (L, B, T, 5, HP) or NULL
    float *dec_top;                     // (B, T_out, HP) or NULL: the top decoder layer's h alone
    float *hT, *cT;                     // (L, B, HP) or NULL: the encoder's final states
    int B, T_in, T_out, F, O;
};

struct StackedTrainBwdParams {
    const float *enc_res, *dec_res, *cT, *dhs_top;
    const float *eR[3], *eK[3], *dR[3], *dK[3];   // K of layer 0 is not read
    float *enc_dz, *dec_dz;             // (L, B, T, 4 HP)
    float *dx;                          // scratch (B, Tmax, HP)
    int B, T_in, T_out, Tmax;
};

__host__ __device__ constexpr int st_ldz(int HP) { return 4 * HP + 4; }
// floats of the backward's LDS: R^T and K^T in B-operand order, the dz tile
__host__ __device__ constexpr int st_bwd_lds_floats(int HP) { return 2 * HP * 4 * HP + SS_BT * st_ldz(HP); }

// K_0 (F rows) -> LDS in B-operand order, sK[(j * 4 + s) * NT + tid] = {i, f, g, o} of input row 16 j + 4 g4 + s; rows >= F
// lie past the descriptor and read as zero (the whole offset is in the vector register)
template <int HP>
__device__ __forceinline__ void stage_k0(f32x4* sK, const float* K0, int F, int nkb, int tid, int unit, int g4) {
    constexpr int NT = 4 * HP, H4 = 4 * HP;
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(K0), 0, F * H4 * 4, SS_RSRC);
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

// acc += x . K_0 for the x tile row `xa` (the lane's row n, columns 4 g4 ..) and K_0 as stage_k0 left it
template <int HP>
__device__ __forceinline__ void mm_k0(f32x4 (&acc)[4], const float* xa, const f32x4* sK, int nkb, int tid) {
    constexpr int NT = 4 * HP;
    for (int j = 0; j < nkb; ++j) {
        const f32x4 av = *(const f32x4*)(xa + 16 * j);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f32x4 kv = sK[(j * 4 + s) * NT + tid];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], kv[g], acc[g], 0, 0, 0);
        }
    }
}

// cell_update (stacked_tile.h: the same expressions, the same bits) with the tape: hs / top (+ r T HP) and the reserve's
// activated i, f, g, o and c (+ r T 5 HP) of the lane's `live` rows; each pointer is at (row 4 g4, step, unit) or NULL
template <int HP, int ACT>
__device__ __forceinline__ void cell_update_tape(const f32x4 (&acc)[4], float (&c)[4], float (&h)[4], float* hw, float* hs, float* top,
                                                 float* res, size_t T, int live) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float ig = rec_act<ACT>(acc[0][r]), fg = rec_act<ACT>(acc[1][r]), gg = tanh_f(acc[2][r]), og = rec_act<ACT>(acc[3][r]);
        c[r] = fmaf(fg, c[r], ig * gg);
        h[r] = og * tanh_f(c[r]);
        hw[r * ss_ldh(HP)] = h[r];
        if (r < live) {
            if (hs) hs[r * T * HP] = h[r];
            if (top) top[r * T * HP] = h[r];
            if (res) {
                float* q = res + r * T * 5 * HP;
                q[0] = ig; q[HP] = fg; q[2 * HP] = gg; q[3 * HP] = og; q[4 * HP] = c[r];
            }
        }
    }
}

template <int HP, int L, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void stacked_train_fwd_kernel(StackedTrainFwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float st_smem[];
    constexpr int NT = 4 * HP, NJ = HP / 16, LDH = ss_ldh(HP), HT = SS_BT * LDH;
    constexpr int XROWS = NT / 16, XP = SS_BT / XROWS;   // x staging: a thread loads column xc + 16 i of rows xrow + XROWS pp
    float* sH = st_smem;                         // [3][2][16][LDH]
    float* sX = sH + 6 * HT;                     // [2][16][SS_LDX]
    f32x4* sK = (f32x4*)(sX + 2 * SS_BT * SS_LDX);   // [nkb][4][NT]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SS_BT;
    const int B = p.B, T_in = p.T_in, T_out = p.T_out, F = p.F, O = p.O;
    const int nkb = (F + 15) >> 4;
    const float* a_rd = sH + n * LDH + 4 * g4;          // + tile: this lane's A fragments
    float* h_wr = sH + 4 * g4 * LDH + unit;             // + tile: this lane's four h values (rows 4 g4 + r)
    const int row0 = b0 + 4 * g4;                       // this lane's first sequence
    const int live = min(max(B - row0, 0), 4);

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
        stage_k0<HP>(sK, p.eK[0], F, nkb, tid, unit, g4);
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
        // this lane's tape positions of (layer l, row0, step t, unit): + (l B T + t) HP for hs, 5 times that for the reserve
        const size_t T = (size_t)T_in, lstride = (size_t)B * T * HP;
        float* hs0 = p.enc_hs ? p.enc_hs + (size_t)row0 * T * HP + unit : nullptr;
        float* rs0 = p.enc_res ? p.enc_res + (size_t)row0 * T * 5 * HP + unit : nullptr;
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
                mm_k0<HP>(acc, sX + cur * SS_BT * SS_LDX + n * SS_LDX + 4 * g4, sK, nkb, tid);
                mm_frag<NJ>(acc, a_rd + prv * HT, wR0);
                cell_update_tape<HP, ACT>(acc, c[0], h[0], h_wr + cur * HT, hs0 ? hs0 + (size_t)t * HP : nullptr, nullptr,
                                          rs0 ? rs0 + (size_t)t * 5 * HP : nullptr, T, live);
            }
            if (more) store_x(sX + prv * SS_BT * SS_LDX);
            __syncthreads();
#pragma unroll
            for (int l = 1; l < L; ++l) {
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[l][g], bias[l][g], bias[l][g], bias[l][g]};
                mm_frag<NJ>(acc, a_rd + (2 * (l - 1) + cur) * HT, wK[l - 1]);
                mm_frag<NJ>(acc, a_rd + (2 * l + prv) * HT, wR[l - 1]);
                cell_update_tape<HP, ACT>(acc, c[l], h[l], h_wr + (2 * l + cur) * HT, hs0 ? hs0 + l * lstride + (size_t)t * HP : nullptr,
                                          nullptr, rs0 ? rs0 + 5 * (l * lstride + (size_t)t * HP) : nullptr, T, live);
                __syncthreads();
            }
        }
    } else {
        __syncthreads();
    }

    // the encoder's final states (zeros without an encoder step): what seeds the decoder
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < live) {
                if (p.hT) p.hT[((size_t)l * B + row0 + r) * HP + unit] = h[l][r];
                if (p.cT) p.cT[((size_t)l * B + row0 + r) * HP + unit] = c[l][r];
            }

    // ================= decoder, teacher-forced =================
    if (T_out > 0) {
        float wK0[4][4], wR0[NJ][4][4], wK[L - 1][NJ][4][4], wR[L - 1][NJ][4][4], bias[L][4], xa[4], xn[4];
        {   // K_0: register r of the input fragment is feature 4 g4 + r, so k-step r contracts input rows 4 g4 + r (zero from O on)
            const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dK[0]), 0, O * 4 * HP * 4, SS_RSRC);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    wK0[r][g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(krs, (unsigned)(((4 * g4 + r) * 4 * HP + g * HP + unit) * 4), 0, 0));
        }
        load_frag<HP>(wR0, p.dR[0], unit, g4);
        load_bias<HP>(bias[0], p.db[0], unit);
#pragma unroll
        for (int l = 1; l < L; ++l) {
            load_frag<HP>(wK[l - 1], p.dK[l], unit, g4);
            load_frag<HP>(wR[l - 1], p.dR[l], unit, g4);
            load_bias<HP>(bias[l], p.db[l], unit);
        }
        // the A fragment of layer 0: dec_in[sequence n][step][feature 4 g4 + r], straight from memory, one step ahead
        const bool row_live = b0 + n < B;
        auto load_in = [&](float (&v)[4], int s_) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                v[r] = (row_live && 4 * g4 + r < O) ? p.dec_in[((size_t)(b0 + n) * T_out + s_) * O + 4 * g4 + r] : 0.f;
        };
        const size_t T = (size_t)T_out, lstride = (size_t)B * T * HP;
        float* hs0 = p.dec_hs ? p.dec_hs + (size_t)row0 * T * HP + unit : nullptr;
        float* rs0 = p.dec_res ? p.dec_res + (size_t)row0 * T * 5 * HP + unit : nullptr;
        float* tp0 = p.dec_top ? p.dec_top + (size_t)row0 * T * HP + unit : nullptr;
        load_in(xa, 0);
        for (int s_ = 0; s_ < T_out; ++s_) {
            const int cur = (T_in + s_) & 1, prv = cur ^ 1;
            if (s_ + 1 < T_out) load_in(xn, s_ + 1);
            f32x4 acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[0][g], bias[0][g], bias[0][g], bias[0][g]};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[r], wK0[r][g], acc[g], 0, 0, 0);
            mm_frag<NJ>(acc, a_rd + prv * HT, wR0);
            cell_update_tape<HP, ACT>(acc, c[0], h[0], h_wr + cur * HT, hs0 ? hs0 + (size_t)s_ * HP : nullptr, nullptr,
                                      rs0 ? rs0 + (size_t)s_ * 5 * HP : nullptr, T, live);
            __syncthreads();
#pragma unroll
            for (int l = 1; l < L; ++l) {
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[l][g], bias[l][g], bias[l][g], bias[l][g]};
                mm_frag<NJ>(acc, a_rd + (2 * (l - 1) + cur) * HT, wK[l - 1]);
                mm_frag<NJ>(acc, a_rd + (2 * l + prv) * HT, wR[l - 1]);
                cell_update_tape<HP, ACT>(acc, c[l], h[l], h_wr + (2 * l + cur) * HT, hs0 ? hs0 + l * lstride + (size_t)s_ * HP : nullptr,
                                          (l == L - 1 && tp0) ? tp0 + (size_t)s_ * HP : nullptr,
                                          rs0 ? rs0 + 5 * (l * lstride + (size_t)s_ * HP) : nullptr, T, live);
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) xa[r] = xn[r];
        }
    }
}

// W (HP, 4 HP) -> LDS as the B operand of dz . W^T: [wave][jj][lane (n, g4)] {s = 0..3} = W[16 w + n][16 jj + 4 g4 + s].  Here the
// lane is (n, s): four consecutive floats of a row of W are one lane's b128 later.
template <int HP>
__device__ __forceinline__ void stage_transposed(f32x4* sT, const float* W, int wave, int unit, int n, int g4) {
    constexpr int H4 = 4 * HP, NJ4 = H4 / 16;
    const float* Wrow = W + (size_t)unit * H4;
    float* dst = (float*)(sT + wave * NJ4 * 64);
#pragma unroll 8
    for (int q = 0; q < NJ4 * 4; ++q) dst[(q * 16 + n) * 4 + g4] = Wrow[4 * q + g4];
}

// BPTT of one layer over its T steps.  res / dz: the layer's slices (B, T, 5 HP) / (B, T, 4 HP); c0 (B, HP) or NULL (zero);
// din (B, din_T, din_ld >= HP) or NULL: the gradient that reaches h_t from above; dh / dc: in (dh_T, dc_T), out (dh_0, dc_0).
// HASK: also dx_t = dz_t . K^T into p_dx (B, dx_T, dx_ld >= HP).  din may lie inside dzo (din_ld = 4 HP, the gate-i slot of every
// step: stack2_tile_bwd_kernel): the lane that reads din of (row, t, unit) is the one that overwrites it with dz_t afterwards, and
// load_step(t - 1) touches only step t - 1.
template <int HP, int ACT, bool HASK>
__device__ __forceinline__ void bwd_layer(float* smem, const float* res, const float* c0, const float* din, int din_T, int din_ld,
                                          const float* R, const float* K, float* dzo, float* p_dx, int dx_T, int dx_ld, int B, int T,
                                          f32x4& dh_io, float (&dc)[4]) {
    constexpr int NW = HP / 16, H4 = 4 * HP, NJ4 = H4 / 16, LDZ = st_ldz(HP);
    f32x4* sRT = (f32x4*)smem;                        // [NW][NJ4][64]
    f32x4* sKT = sRT + HP * HP;                       // the same for K
    float* sZ = smem + 2 * HP * H4;                   // [16][LDZ]: dz of the step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int row0 = blockIdx.x * SS_BT + 4 * g4;
    const int live = min(max(B - row0, 0), 4);
    (void)NW;

    __syncthreads();      // the layer before is through with the LDS; its dx stores are visible to this workgroup
    if (T <= 0) return;   // (uniform) nothing to walk: (dh, dc) pass through
    stage_transposed<HP>(sRT, R, wave, unit, n, g4);
    if constexpr (HASK) stage_transposed<HP>(sKT, K, wave, unit, n, g4);

    // tape rows of one step: gates, c_t, c_{t-1} and the gradient from above of (row row0 + r, unit)
    float gi[4], gf[4], gg[4], go[4], cc[4], cp[4], dn[4];
    auto load_step = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = r < live;
            const size_t row = (size_t)(row0 + r);
            const float* q = res + (row * T + t) * 5 * HP + unit;
            gi[r] = on ? q[0] : 0.f;
            gf[r] = on ? q[HP] : 0.f;
            gg[r] = on ? q[2 * HP] : 0.f;
            go[r] = on ? q[3 * HP] : 0.f;
            cc[r] = on ? q[4 * HP] : 0.f;
            cp[r] = !on ? 0.f : t > 0 ? q[4 * HP - 5 * HP] : c0 ? c0[row * HP + unit] : 0.f;
            dn[r] = (on && din) ? din[(row * din_T + t) * din_ld + unit] : 0.f;
        }
    };
    load_step(T - 1);
    f32x4 dhR = dh_io;
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        // ---- gate backward, lane-local; dz_t to the tile and to the tape ----
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float dz[4];
            {   // lstm_cell_bwd's expression tree (fov_common.h), every operation rounded once: left to contract, the compiler packs
                // some of a lane's four rows into v_pk_mul_f32 + add and fuses the others into v_fma_f32, and a row's last bit
                // then depends on its place in the tile
#pragma clang fp contract(off)
                const float dh = dhR[r] + dn[r];
                const float tc = tanh_f(cc[r]);
                const float dcv = dc[r] + dh * go[r] * (1.f - tc * tc);
                dz[0] = dcv * gg[r] * rec_act_grad<ACT>(gi[r]);
                dz[1] = dcv * cp[r] * rec_act_grad<ACT>(gf[r]);
                dz[2] = dcv * gi[r] * (1.f - gg[r] * gg[r]);
                dz[3] = dh * tc * rec_act_grad<ACT>(go[r]);
                dc[r] = dcv * gf[r];
            }
            float* zt = sZ + (4 * g4 + r) * LDZ + unit;
            float* zg = dzo + ((size_t)(row0 + r) * T + t) * H4 + unit;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                zt[g * HP] = dz[g];
                if (r < live) zg[g * HP] = dz[g];
            }
        }
        __syncthreads();
        if (t > 0) load_step(t - 1);
        // ---- dz_t . R^T for the step below (dh_0 after the last one) and dx_t = dz_t . K^T; four accumulators each, summed in a fixed order ----
        {
            f32x4 a4[4], k4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a4[i] = k4[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* zr = sZ + n * LDZ + 4 * g4;
            const f32x4* rt = sRT + wave * NJ4 * 64 + lane;
            const f32x4* kt = sKT + wave * NJ4 * 64 + lane;
#pragma unroll
            for (int jj = 0; jj < NJ4; ++jj) {
                const f32x4 zv = *(const f32x4*)(zr + 16 * jj);
                const f32x4 rv = rt[jj * 64];
#pragma unroll
                for (int s = 0; s < 4; ++s) a4[jj & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[s], rv[s], a4[jj & 3], 0, 0, 0);
                if constexpr (HASK) {
                    const f32x4 kv = kt[jj * 64];
#pragma unroll
                    for (int s = 0; s < 4; ++s) k4[jj & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[s], kv[s], k4[jj & 3], 0, 0, 0);
                }
            }
            dhR = (a4[0] + a4[1]) + (a4[2] + a4[3]);
            if constexpr (HASK) {
                const f32x4 dxv = (k4[0] + k4[1]) + (k4[2] + k4[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (r < live) p_dx[((size_t)(row0 + r) * dx_T + t) * dx_ld + unit] = dxv[r];
            }
        }
        __syncthreads();
    }
    dh_io = dhR;
}

template <int HP, int L, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void stacked_train_bwd_kernel(StackedTrainBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float st_smem[];
    const int B = p.B, T_in = p.T_in, T_out = p.T_out, Tmax = p.Tmax;
    f32x4 dh[L];
    float dc[L][4];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        dh[l] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) dc[l][r] = 0.f;
    }
    // ---- decoder stack, top layer first: (dh, dc)[l] leave as the layer's (dh_0, dc_0) ----
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        const float* res = p.dec_res + (size_t)l * B * T_out * 5 * HP;
        const float* c0 = p.cT + (size_t)l * B * HP;
        float* dzo = p.dec_dz + (size_t)l * B * T_out * 4 * HP;
        const float* din = l == L - 1 ? p.dhs_top : p.dx;
        const int din_T = l == L - 1 ? T_out : Tmax;
        if (l > 0) bwd_layer<HP, ACT, true>(st_smem, res, c0, din, din_T, HP, p.dR[l], p.dK[l], dzo, p.dx, Tmax, HP, B, T_out, dh[l], dc[l]);
        else bwd_layer<HP, ACT, false>(st_smem, res, c0, din, din_T, HP, p.dR[l], nullptr, dzo, nullptr, 0, 0, B, T_out, dh[l], dc[l]);
    }
    // ---- encoder stack: layer l takes decoder layer l's (dh_0, dc_0) as its (dh_T, dc_T) ----
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        const float* res = p.enc_res + (size_t)l * B * T_in * 5 * HP;
        float* dzo = p.enc_dz + (size_t)l * B * T_in * 4 * HP;
        const float* din = l == L - 1 ? nullptr : p.dx;
        if (l > 0) bwd_layer<HP, ACT, true>(st_smem, res, nullptr, din, Tmax, HP, p.eR[l], p.eK[l], dzo, p.dx, Tmax, HP, B, T_in, dh[l], dc[l]);
        else bwd_layer<HP, ACT, false>(st_smem, res, nullptr, din, Tmax, HP, p.eR[l], nullptr, dzo, nullptr, 0, 0, B, T_in, dh[l], dc[l]);
    }
}

// BPTT of two stacked layers that takes its gradients from outside (fov_lstm_stack2_bwd at H = 32 / 64): the upper layer, then the
// lower one, each from its own (dh_T, dc_T) and to its own (dh_0, dc_0).  The upper layer's dx_t = dz2_t . K2^T is staged in the
// lower layer's dz tape itself - the first HP floats of dz1[row][t], row stride 4 HP - which the lower layer reads as its din and
// then overwrites with its own dz_t (bwd_layer's comment: same lane, one step at a time).  No scratch, no header, no wait.
struct Stack2TileBwdParams {
    BwdRec up, low;                     // db_part of neither is written, low.dhs is not read
    const float* K2;
    int B, T;
};

// (dh, dc) of the lane's rows 4 g4 + r and unit: zeros for a NULL pointer and for rows beyond B
template <int HP>
__device__ __forceinline__ void load_state_grad(f32x4& dh, float (&dc)[4], const float* dhT, const float* dcT, int row0, int unit, int live) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t at = (size_t)(row0 + r) * HP + unit;
        dh[r] = (dhT && r < live) ? dhT[at] : 0.f;
        dc[r] = (dcT && r < live) ? dcT[at] : 0.f;
    }
}

template <int HP>
__device__ __forceinline__ void store_state_grad(const f32x4& dh, const float (&dc)[4], float* dh0, float* dc0, int row0, int unit, int live) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < live) {
            const size_t at = (size_t)(row0 + r) * HP + unit;
            if (dh0) dh0[at] = dh[r];
            if (dc0) dc0[at] = dc[r];
        }
}

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void stack2_tile_bwd_kernel(Stack2TileBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float st_smem[];
    const int B = p.B, T = p.T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int unit = 16 * wave + (lane & 15);
    const int row0 = blockIdx.x * SS_BT + 4 * (lane >> 4);
    const int live = min(max(B - row0, 0), 4);
    f32x4 dh;
    float dc[4];
    // ---- upper layer: dz2, and dx_t into the gate-i slot of dz1's step t ----
    load_state_grad<HP>(dh, dc, p.up.dhT, p.up.dcT, row0, unit, live);
    bwd_layer<HP, ACT, true>(st_smem, p.up.reserve, p.up.c0, p.up.dhs, T, HP, p.up.R, p.K2, p.up.dz, p.low.dz, T, 4 * HP, B, T, dh, dc);
    store_state_grad<HP>(dh, dc, p.up.dh0, p.up.dc0, row0, unit, live);
    // ---- lower layer: din from its own dz tape ----
    load_state_grad<HP>(dh, dc, p.low.dhT, p.low.dcT, row0, unit, live);
    bwd_layer<HP, ACT, false>(st_smem, p.low.reserve, p.low.c0, p.low.dz, T, 4 * HP, p.low.R, nullptr, p.low.dz, nullptr, 0, 0, B, T, dh, dc);
    store_state_grad<HP>(dh, dc, p.low.dh0, p.low.dc0, row0, unit, live);
}

template <int HP>
int launch_stack2_tile(const Stack2TileBwdParams& p, int act, hipStream_t stream) {
    void (*kern)(Stack2TileBwdParams) = act == FOV_ACT_HARD_SIGMOID ? stack2_tile_bwd_kernel<HP, FOV_ACT_HARD_SIGMOID>
                                                                    : stack2_tile_bwd_kernel<HP, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)st_bwd_lds_floats(HP) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("two-layer tile BPTT");
}

template <int HP, int L>
int launch_train_fwd(const StackedTrainFwdParams& p, int act, hipStream_t stream) {
    void (*kern)(StackedTrainFwdParams) = act == FOV_ACT_HARD_SIGMOID ? stacked_train_fwd_kernel<HP, L, FOV_ACT_HARD_SIGMOID>
                                                                      : stacked_train_fwd_kernel<HP, L, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)ss_lds_floats(HP, p.T_in > 0 ? (p.F + 15) / 16 : 0) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("stacked seq2seq training forward");
}

template <int HP, int L>
int launch_train_bwd(const StackedTrainBwdParams& p, int act, hipStream_t stream) {
    void (*kern)(StackedTrainBwdParams) = act == FOV_ACT_HARD_SIGMOID ? stacked_train_bwd_kernel<HP, L, FOV_ACT_HARD_SIGMOID>
                                                                      : stacked_train_bwd_kernel<HP, L, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)st_bwd_lds_floats(HP) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("stacked seq2seq training backward");
}

int train_refuse(const char* entry, int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L) {
    set_error("%s: H = 32 or 64, L = 2 or 3, 1 <= F_enc <= %d, 1 <= F_dec <= 8 and non-negative sizes only "
              "(got B=%d T_in=%d T_out=%d F_enc=%d F_dec=%d H=%d L=%d)", entry, SS_MAX_F, B, T_in, T_out, F_enc, F_dec, H, L);
    return FOV_ERR_UNSUPPORTED;
}

// NULL, or an array whose first L entries (from `first` on) are all there
bool all_there(const float* const* a, int L, int first = 0) {
    if (!a) return false;
    for (int l = first; l < L; ++l)
        if (!a[l]) return false;
    return true;
}

}  // namespace

bool stack2_tile_bwd_width(int H) { return H == 32 || H == 64; }

int launch_stack2_tile_bwd(const BwdRec& up, const BwdRec& low, const float* K2, int B, int T, int H, int act, hipStream_t stream) {
    if (B <= 0 || T <= 0) return FOV_OK;
    if (!stack2_tile_bwd_width(H) || B > kMaxTileBatch) { set_error("two-layer tile BPTT: H = 32 or 64 only (got H=%d B=%d)", H, B); return FOV_ERR_UNSUPPORTED; }
    Stack2TileBwdParams p = {up, low, K2, B, T};
    return H == 32 ? launch_stack2_tile<32>(p, act, stream) : launch_stack2_tile<64>(p, act, stream);
}

}  // namespace fov

using namespace fov;

extern "C" {

// pure arithmetic (and the knob): no device query.  The shape rule is the decode kernel's.
int fov_stacked_seq2seq_train_supported(int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L) {
    return (!env_knobs().no_stacked_train && stacked_s2s_shape_ok(B, T_in, T_out, F_enc, F_dec, H, L)) ? 1 : 0;
}

size_t fov_stacked_seq2seq_train_bwd_scratch_bytes(int B, int T_in, int T_out, int H) {
    if (B <= 0 || H <= 0) return 0;
    const int Tmax = T_in > T_out ? T_in : T_out;
    return Tmax > 0 ? sizeof(float) * (size_t)B * Tmax * H : 0;
}

int fov_stacked_seq2seq_train_fwd(const float* enc_in, const float* dec_in, const float* const* enc_K, const float* const* enc_R,
                                  const float* const* enc_b, const float* const* dec_K, const float* const* dec_R,
                                  const float* const* dec_b, float* enc_hs, float* enc_res, float* dec_hs, float* dec_res,
                                  float* dec_top, float* hT, float* cT, int B, int T_in, int T_out, int F_enc, int F_dec, int H, int L,
                                  int act, fov_stream_t stream) {
    if (!stacked_s2s_shape_ok(B, T_in, T_out, F_enc, F_dec, H, L))   // decided before any pointer is looked at and any HIP call
        return train_refuse("fov_stacked_seq2seq_train_fwd", B, T_in, T_out, F_enc, F_dec, H, L);
    if (!all_there(enc_K, L) || !all_there(enc_R, L) || !all_there(enc_b, L) || !all_there(dec_K, L) || !all_there(dec_R, L) ||
        !all_there(dec_b, L) || (B > 0 && ((T_in > 0 && !enc_in) || (T_out > 0 && !dec_in))) || !valid_act(act)) {
        set_error("fov_stacked_seq2seq_train_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    StackedTrainFwdParams p = {};
    for (int l = 0; l < L; ++l) {
        p.eK[l] = enc_K[l]; p.eR[l] = enc_R[l]; p.eb[l] = enc_b[l];
        p.dK[l] = dec_K[l]; p.dR[l] = dec_R[l]; p.db[l] = dec_b[l];
    }
    p.x = enc_in; p.dec_in = dec_in;
    p.enc_hs = enc_hs; p.enc_res = enc_res; p.dec_hs = dec_hs; p.dec_res = dec_res; p.dec_top = dec_top; p.hT = hT; p.cT = cT;
    p.B = B; p.T_in = T_in; p.T_out = T_out; p.F = F_enc; p.O = F_dec;
    hipStream_t st = (hipStream_t)stream;
    if (H == 32) return L == 2 ? launch_train_fwd<32, 2>(p, act, st) : launch_train_fwd<32, 3>(p, act, st);
    return L == 2 ? launch_train_fwd<64, 2>(p, act, st) : launch_train_fwd<64, 3>(p, act, st);
}

int fov_stacked_seq2seq_train_bwd(const float* enc_res, const float* dec_res, const float* cT, const float* dhs_top,
                                  const float* const* enc_R, const float* const* enc_K, const float* const* dec_R,
                                  const float* const* dec_K, float* enc_dz, float* dec_dz, int B, int T_in, int T_out, int H, int L,
                                  int act, void* scratch, size_t scratch_bytes, fov_stream_t stream) {
    if (!stacked_s2s_shape_ok(B, T_in, T_out, 1, 1, H, L))   // decided before any pointer is looked at and any HIP call
        return train_refuse("fov_stacked_seq2seq_train_bwd", B, T_in, T_out, 1, 1, H, L);
    const bool enc_work = B > 0 && T_in > 0, dec_work = B > 0 && T_out > 0;
    if (!all_there(enc_R, L) || !all_there(dec_R, L) || !all_there(enc_K, L, 1) || !all_there(dec_K, L, 1) ||
        (enc_work && (!enc_res || !enc_dz)) || (dec_work && (!dec_res || !dec_dz || !dhs_top || !cT)) || !valid_act(act)) {
        set_error("fov_stacked_seq2seq_train_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!enc_work && !dec_work) return FOV_OK;
    if (int rc = check_ws(scratch, scratch_bytes, fov_stacked_seq2seq_train_bwd_scratch_bytes(B, T_in, T_out, H))) return rc;
    StackedTrainBwdParams p = {};
    for (int l = 0; l < L; ++l) {
        p.eR[l] = enc_R[l]; p.eK[l] = enc_K[l]; p.dR[l] = dec_R[l]; p.dK[l] = dec_K[l];
    }
    p.enc_res = enc_res; p.dec_res = dec_res; p.cT = cT; p.dhs_top = dhs_top; p.enc_dz = enc_dz; p.dec_dz = dec_dz;
    p.dx = (float*)scratch;
    p.B = B; p.T_in = T_in; p.T_out = T_out; p.Tmax = T_in > T_out ? T_in : T_out;
    hipStream_t st = (hipStream_t)stream;
    if (H == 32) return L == 2 ? launch_train_bwd<32, 2>(p, act, st) : launch_train_bwd<32, 3>(p, act, st);
    return L == 2 ? launch_train_bwd<64, 2>(p, act, st) : launch_train_bwd<64, 3>(p, act, st);
}

}  // extern "C"
