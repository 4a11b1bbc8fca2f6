// The self-fed one-layer decoder (mycode/FoV_seq2seq_no_teac_forc.py:37-149, `onelayer_tar_seq2seq`: the loop at :96-118
// unrolled predict_step times on its own Dense output) as ONE launch per direction: the forward with the training tapes, and
// the BPTT through the feedback.  fp32 throughout (v_mfma_f32_16x16x4_f32, exact expf / tanhf).
//
//   forward,  t = 0 .. T-1:   z = b + x_t . K + h . R;  cell update;  a_t = dact(h_t . W + bd);  y_t = a_t + r;  x_{t+1} = y_t
//   backward, t = T-1 .. 0:   dy_t = dloss_t + dx_{t+1};  dpre_t = dy_t dact'(a_t);  dh = dpre_t . W^T + dz_{t+1} . R^T;
//                             gate backward (lstm_train.hip's pointwise step, c_{t-1} = Cs[t]);  dx_t = dz_t . K^T
//
// Ownership (both kernels).  One workgroup owns one tile of 16 sequences for every step; the grid is the number of tiles and
// workgroups never communicate: no exchange, no workspace, no wait, any grid size runs.  H / 16 waves; wave w owns units
// [16 w, 16 w + 16) of all four gates.  The lane layout is lstm_stacked_s2s.hip's: lane (n, g4) holds unit 16 w + n for the
// sequences 4 g4 .. 4 g4 + 3, so the cell update and the gate backward are lane-local and c / dc never leave registers.
// Rows of a ragged last tile beyond B read zeros (masked, not clamped) and store nothing; MFMA rows are independent, so a
// sequence's result does not depend on its tile-mates or on its place in the batch.
//
// Forward.  K (O <= 8 rows), R and the head's W^T fragments stay in registers for the whole launch; the running h tile lies in
// LDS twice (step parity): one barrier per step.  The head runs as y^T = W^T . h^T, which leaves y[sequence n][output 4 g4 + r]
// in register r of lane (n, g4): exactly the A fragment of the next step's x . K.  Every wave computes the (tiny) head itself.
//
// Backward.  R^T as the B operand of dz . R^T is 4 H registers per lane at one N-tile per wave, so it lies in LDS in B-operand
// order (one ds_read_b128 feeds four k-steps; 64 KB at H = 64) next to the dz tile of the step (16 x 4 H).  dx^T = K . dz^T
// comes out in the same fragment layout as the forward's y; its contraction over the 4 H gate columns is split over the waves
// (each takes 64 of them) and the partial sums meet in LDS, added in wave order by every wave: two barriers per step.  K's and
// W^T's fragments are registers.  The next step's tape rows are loaded under the step's products.
#include "fov_common.h"

namespace fov {

namespace {

struct SelfFedFwdParams {
    const float *x0, *h0, *c0, *K, *R, *b, *W, *bd, *r;
    float *Hs, *Cs, *XA, *A, *RES, *y;
    int B, T, O, dact;
};

struct SelfFedBwdParams {
    const float *Cs, *RES, *aout, *dloss, *K, *R, *W;   // aout (T,B,O): a_t, either A or XA[1:]
    float *DY, *DPRE, *DZ, *dx0, *dh0, *dc0;
    int B, T, O, dact;
};

constexpr int SF_BT = 16;         // sequences per tile
constexpr int SF_DACT_TANH = 1, SF_DACT_RELU = 2;   // fov_act_fwd's codes

__host__ __device__ constexpr int sf_ldz(int HP) { return 4 * HP + 4; }
// floats of the backward's LDS: R^T in B-operand order, the dz tile, one partial dx fragment per wave
__host__ __device__ constexpr int sf_bwd_lds_floats(int HP) { return HP * 4 * HP + SF_BT * sf_ldz(HP) + (HP / 16) * 64 * 4; }

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void selffed_fwd_kernel(SelfFedFwdParams p) {
    constexpr int NJ = HP / 16, H4 = 4 * HP, LDH = HP + 4, HT = SF_BT * LDH;
    __shared__ __attribute__((aligned(16))) float sH[2 * HT];   // [parity][16][LDH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SF_BT;
    const int B = p.B, T = p.T, O = p.O;
    const size_t BH = (size_t)B * HP, BO = (size_t)B * O;
    const bool relu = p.dact == SF_DACT_RELU;
    const float* a_rd = sH + n * LDH + 4 * g4;          // + parity: this lane's A fragments
    float* h_wr = sH + 4 * g4 * LDH + unit;             // + parity: this lane's four h values (rows 4 g4 + r)

    // ---- weights: registers for the whole launch ----
    float wK[4][4], wR[NJ][4][4], bias[4], wd[NJ][4], dbv[4], xa[4], rv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)      // k-step r of x . K contracts input row 4 g4 + r (zero from O on)
#pragma unroll
        for (int g = 0; g < 4; ++g) wK[r][g] = (4 * g4 + r < O) ? p.K[(size_t)(4 * g4 + r) * H4 + g * HP + unit] : 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int g = 0; g < 4; ++g) wR[j][s][g] = p.R[(size_t)(16 * j + 4 * g4 + s) * H4 + g * HP + unit];
            wd[j][s] = (n < O) ? p.W[(size_t)(16 * j + 4 * g4 + s) * O + n] : 0.f;   // head: A operand W^T, row = output n
        }
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = p.b[g * HP + unit];
    const bool row_live = b0 + n < B;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = 4 * g4 + r;
        const bool o_live = o < O && row_live;
        dbv[r] = (o < O) ? p.bd[o] : 0.f;
        xa[r] = o_live ? p.x0[(size_t)(b0 + n) * O + o] : 0.f;
        rv[r] = (p.r && o_live) ? p.r[(size_t)(b0 + n) * O + o] : 0.f;
        if (p.XA && wave == 0 && o_live) p.XA[(size_t)(b0 + n) * O + o] = xa[r];
    }
    // ---- initial state: registers, the tile of parity 1 (step 0 reads it), tape row 0 ----
    float c[4], h[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        const bool live = row < B;
        h[r] = (p.h0 && live) ? p.h0[(size_t)row * HP + unit] : 0.f;
        c[r] = (p.c0 && live) ? p.c0[(size_t)row * HP + unit] : 0.f;
        h_wr[HT + r * LDH] = h[r];
        if (live) {
            if (p.Hs) p.Hs[(size_t)row * HP + unit] = h[r];
            if (p.Cs) p.Cs[(size_t)row * HP + unit] = c[r];
        }
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, prv = cur ^ 1;
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias[g], bias[g], bias[g], bias[g]};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[r], wK[r][g], acc[g], 0, 0, 0);
        {
            const float* a = a_rd + prv * HT;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 av = *(const f32x4*)(a + 16 * j);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wR[j][s][g], acc[g], 0, 0, 0);
            }
        }
        // cell update of this lane's unit for its four sequences; h into the tile of this step; the tape
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ig = rec_act<ACT>(acc[0][r]), fg = rec_act<ACT>(acc[1][r]), gg = tanh_f(acc[2][r]), og = rec_act<ACT>(acc[3][r]);
            c[r] = fmaf(fg, c[r], ig * gg);
            h[r] = og * tanh_f(c[r]);
            h_wr[cur * HT + r * LDH] = h[r];
            const int row = b0 + 4 * g4 + r;
            if (row < B) {
                const size_t at = (size_t)(t + 1) * BH + (size_t)row * HP + unit;
                if (p.Hs) p.Hs[at] = h[r];
                if (p.Cs) p.Cs[at] = c[r];
                if (p.RES) {
                    float* q = p.RES + ((size_t)t * B + row) * 5 * HP + unit;
                    q[0] = ig; q[HP] = fg; q[2 * HP] = gg; q[3 * HP] = og; q[4 * HP] = c[r];
                }
            }
        }
        __syncthreads();
        // ---- head: a_t = dact(h_t . W + bd), y_t = a_t + r, every wave for itself ----
        f32x4 yacc = {0.f, 0.f, 0.f, 0.f};
        const float* ht = a_rd + cur * HT;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x4 hv = *(const f32x4*)(ht + 16 * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) yacc = __builtin_amdgcn_mfma_f32_16x16x4f32(wd[j][s], hv[s], yacc, 0, 0, 0);
        }
        float av[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = yacc[r] + dbv[r];
            av[r] = (4 * g4 + r < O) ? (relu ? fmaxf(v, 0.f) : tanh_f(v)) : 0.f;
            xa[r] = av[r] + rv[r];
        }
        if (wave == 0 && row_live) {
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4;
            float* yp = p.y ? p.y + ((size_t)(b0 + n) * T + t) * O + 4 * g4 : nullptr;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g4 + r < O) {
                    if (p.A) p.A[at + r] = av[r];
                    if (p.XA) p.XA[BO + at + r] = xa[r];
                    if (yp) yp[r] = xa[r];
                }
        }
    }
}

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void selffed_bwd_kernel(SelfFedBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float sf_smem[];
    constexpr int NW = HP / 16, H4 = 4 * HP, NJ4 = H4 / 16, LDZ = sf_ldz(HP), KQ = H4 / NW;   // KQ = 64 gate columns of dx per wave
    f32x4* sRT = (f32x4*)sf_smem;                        // [NW][NJ4][64] {s = 0..3}: R[16 w + n][16 jj + 4 g4 + s]
    float* sZ = sf_smem + HP * H4;                       // [16][LDZ]: dz of the step
    f32x4* sP = (f32x4*)(sZ + SF_BT * LDZ);              // [NW][64]: partial dx fragments
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SF_BT;
    const int B = p.B, T = p.T, O = p.O;
    const size_t BH = (size_t)B * HP, BO = (size_t)B * O;
    const bool relu = p.dact == SF_DACT_RELU;
    const bool row_live = b0 + n < B;

    {   // R^T -> LDS: here the lane is (n, s); four consecutive floats of a row of R are one lane's b128 later
        const float* Rrow = p.R + (size_t)unit * H4;
        float* dst = (float*)(sRT + wave * NJ4 * 64);
        for (int q = 0; q < NJ4 * 4; ++q) dst[(q * 16 + n) * 4 + g4] = Rrow[4 * q + g4];
    }
    float kA[KQ / 16][4], wWT[4];
    const int kb = wave * KQ;
#pragma unroll
    for (int j = 0; j < KQ / 16; ++j)     // dx^T = K . dz^T: A operand K, row = input n (zero from O on)
#pragma unroll
        for (int s = 0; s < 4; ++s) kA[j][s] = (n < O) ? p.K[(size_t)n * H4 + kb + 16 * j + 4 * g4 + s] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) wWT[r] = (4 * g4 + r < O) ? p.W[(size_t)unit * O + 4 * g4 + r] : 0.f;

    // tape rows of one step: gates, c_t, c_{t-1} of (row 4 g4 + r, unit); dloss and a_t of (sequence n, output 4 g4 + r)
    float gi[4], gf[4], gg[4], go[4], cc[4], cp[4], dl[4], av[4];
    auto load_step = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = b0 + 4 * g4 + r;
            const bool live = row < B;
            const float* q = p.RES + ((size_t)t * B + row) * 5 * HP + unit;
            gi[r] = live ? q[0] : 0.f;
            gf[r] = live ? q[HP] : 0.f;
            gg[r] = live ? q[2 * HP] : 0.f;
            go[r] = live ? q[3 * HP] : 0.f;
            cc[r] = live ? q[4 * HP] : 0.f;
            cp[r] = live ? p.Cs[(size_t)t * BH + (size_t)row * HP + unit] : 0.f;
            const bool o_live = 4 * g4 + r < O && row_live;
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4 + r;
            dl[r] = o_live ? p.dloss[at] : 0.f;
            av[r] = o_live ? p.aout[at] : 0.f;
        }
    };
    load_step(T - 1);
    f32x4 dhR = {0.f, 0.f, 0.f, 0.f}, dxv = {0.f, 0.f, 0.f, 0.f};
    float dc[4] = {0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        // ---- dy_t = dloss_t + dx_{t+1}; dpre_t = dy_t dact'(a_t) ----
        float dy[4], dpre[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dy[r] = dl[r] + dxv[r];
            dpre[r] = dy[r] * (relu ? (av[r] > 0.f ? 1.f : 0.f) : (1.f - av[r] * av[r]));
        }
        if (wave == 0 && row_live) {
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g4 + r < O) { p.DY[at + r] = dy[r]; p.DPRE[at + r] = dpre[r]; }
        }
        // ---- dh = dz_{t+1} . R^T + dpre_t . W^T ----
        f32x4 dh = dhR;
#pragma unroll
        for (int r = 0; r < 4; ++r) dh = __builtin_amdgcn_mfma_f32_16x16x4f32(dpre[r], wWT[r], dh, 0, 0, 0);
        // ---- gate backward, lane-local; dz_t to the tile and to the tape ----
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float tc = tanh_f(cc[r]);
            const float dov = dh[r] * tc;
            const float dcv = dc[r] + dh[r] * go[r] * (1.f - tc * tc);
            float dz[4];
            dz[0] = dcv * gg[r] * rec_act_grad<ACT>(gi[r]);
            dz[1] = dcv * cp[r] * rec_act_grad<ACT>(gf[r]);
            dz[2] = dcv * gi[r] * (1.f - gg[r] * gg[r]);
            dz[3] = dov * rec_act_grad<ACT>(go[r]);
            dc[r] = dcv * gf[r];
            const int row = b0 + 4 * g4 + r;
            float* zt = sZ + (4 * g4 + r) * LDZ + unit;
            float* zg = p.DZ + ((size_t)t * B + row) * H4 + unit;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                zt[g * HP] = dz[g];
                if (row < B) zg[g * HP] = dz[g];
            }
        }
        __syncthreads();
        if (t > 0) load_step(t - 1);
        // ---- dz_t . R^T for the step below (dh0 after the last one); four accumulators, summed in a fixed order ----
        {
            f32x4 a4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a4[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* zr = sZ + n * LDZ + 4 * g4;
            const f32x4* rt = sRT + wave * NJ4 * 64 + lane;
#pragma unroll
            for (int jj = 0; jj < NJ4; ++jj) {
                const f32x4 zv = *(const f32x4*)(zr + 16 * jj);
                const f32x4 rv = rt[jj * 64];
#pragma unroll
                for (int s = 0; s < 4; ++s) a4[jj & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[s], rv[s], a4[jj & 3], 0, 0, 0);
            }
            dhR = (a4[0] + a4[1]) + (a4[2] + a4[3]);
            // ---- this wave's share of dx_t^T = K . dz_t^T ----
            f32x4 px[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int j = 0; j < KQ / 16; ++j) {
                const f32x4 zv = *(const f32x4*)(zr + kb + 16 * j);
#pragma unroll
                for (int s = 0; s < 4; ++s) px[j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(kA[j][s], zv[s], px[j & 1], 0, 0, 0);
            }
            sP[wave * 64 + lane] = px[0] + px[1];
        }
        __syncthreads();
        dxv = sP[lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) dxv += sP[w * 64 + lane];
    }

    if (wave == 0 && row_live) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * g4 + r < O) p.dx0[(size_t)(b0 + n) * O + 4 * g4 + r] = dxv[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        if (row < B) {
            if (p.dh0) p.dh0[(size_t)row * HP + unit] = dhR[r];
            if (p.dc0) p.dc0[(size_t)row * HP + unit] = dc[r];
        }
    }
}

template <int HP>
int launch_selffed_fwd(const SelfFedFwdParams& p, int act, hipStream_t stream) {
    void (*kern)(SelfFedFwdParams) = act == FOV_ACT_HARD_SIGMOID ? selffed_fwd_kernel<HP, FOV_ACT_HARD_SIGMOID> : selffed_fwd_kernel<HP, FOV_ACT_SIGMOID>;
    hipLaunchKernelGGL(kern, dim3((p.B + SF_BT - 1) / SF_BT), dim3(4 * HP), 0, stream, p);
    return launch_check("self-fed decoder forward");
}

template <int HP>
int launch_selffed_bwd(const SelfFedBwdParams& p, int act, hipStream_t stream) {
    void (*kern)(SelfFedBwdParams) = act == FOV_ACT_HARD_SIGMOID ? selffed_bwd_kernel<HP, FOV_ACT_HARD_SIGMOID> : selffed_bwd_kernel<HP, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)sf_bwd_lds_floats(HP) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SF_BT - 1) / SF_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("self-fed decoder backward");
}

int selffed_refuse(const char* entry, int B, int T, int O, int H) {
    set_error("%s: H = 32 or 64, 1 <= O <= 8 and non-negative sizes only (got B=%d T=%d O=%d H=%d)", entry, B, T, O, H);
    return FOV_ERR_UNSUPPORTED;
}

}  // namespace

// pure arithmetic: no device query
bool selffed_shape_ok(int B, int T, int O, int H) { return B >= 0 && B <= kMaxTileBatch && T >= 0 && T <= kMaxTileBatch && (H == 32 || H == 64) && O >= 1 && O <= 8; }

}  // namespace fov

using namespace fov;

extern "C" {

int fov_selffed_decoder_supported(int B, int T, int O, int H) {
    return (!env_knobs().no_selffed_fused && selffed_shape_ok(B, T, O, H)) ? 1 : 0;
}

int fov_selffed_decoder_fwd(const float* x0, const float* h0, const float* c0, const float* K, const float* R, const float* b,
                            const float* W, const float* bd, const float* r, float* Hs, float* Cs, float* XA, float* A, float* RES,
                            float* y, int B, int T, int O, int H, int act, int dact, fov_stream_t stream) {
    if (!selffed_shape_ok(B, T, O, H)) return selffed_refuse("fov_selffed_decoder_fwd", B, T, O, H);   // before any HIP call
    const bool work = B > 0 && T > 0;
    if (!K || !R || !b || !W || !bd || (work && !x0) || (h0 == nullptr) != (c0 == nullptr) ||
        (act != FOV_ACT_SIGMOID && act != FOV_ACT_HARD_SIGMOID) || (dact != SF_DACT_TANH && dact != SF_DACT_RELU)) {
        set_error("fov_selffed_decoder_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!work) return FOV_OK;
    SelfFedFwdParams p = {x0, h0, c0, K, R, b, W, bd, r, Hs, Cs, XA, A, RES, y, B, T, O, dact};
    return H == 32 ? launch_selffed_fwd<32>(p, act, (hipStream_t)stream) : launch_selffed_fwd<64>(p, act, (hipStream_t)stream);
}

int fov_selffed_decoder_bwd(const float* Cs, const float* XA, const float* A, const float* RES, const float* dloss, const float* K,
                            const float* R, const float* W, float* DY, float* DPRE, float* DZ, float* dx0, float* dh0, float* dc0,
                            int B, int T, int O, int H, int act, int dact, int a_from_A, fov_stream_t stream) {
    if (!selffed_shape_ok(B, T, O, H)) return selffed_refuse("fov_selffed_decoder_bwd", B, T, O, H);   // before any HIP call
    const bool work = B > 0 && T > 0;
    if (!K || !R || !W || (B > 0 && !dx0) || (work && (!Cs || !RES || !dloss || !DY || !DPRE || !DZ || !(a_from_A ? A : XA))) ||
        (act != FOV_ACT_SIGMOID && act != FOV_ACT_HARD_SIGMOID) || (dact != SF_DACT_TANH && dact != SF_DACT_RELU)) {
        set_error("fov_selffed_decoder_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {   // no step and no gradient of the final state comes in: all three are zero
        hipError_t e = hipMemsetAsync(dx0, 0, sizeof(float) * (size_t)B * O, st);
        if (e == hipSuccess && dh0) e = hipMemsetAsync(dh0, 0, sizeof(float) * (size_t)B * H, st);
        if (e == hipSuccess && dc0) e = hipMemsetAsync(dc0, 0, sizeof(float) * (size_t)B * H, st);
        if (e != hipSuccess) { set_error("fov_selffed_decoder_bwd: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
        return FOV_OK;
    }
    SelfFedBwdParams p = {Cs, RES, a_from_A ? A : XA + (size_t)B * O, dloss, K, R, W, DY, DPRE, DZ, dx0, dh0, dc0, B, T, O, dact};
    return H == 32 ? launch_selffed_bwd<32>(p, act, st) : launch_selffed_bwd<64>(p, act, st);
}

}  // extern "C"
