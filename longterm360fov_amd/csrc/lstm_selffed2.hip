// The self-fed TWO-layer decoder of mycode/given_others_gt_mean_var_seq2seq.py:203-299 (heads `target_user_only` :219-220,
// `others_mlp` :223-233, `others_lstm` :234-240: the loop unrolled predict_step times on its own Dense output, with a per-step
// additive context inside the head's tanh) as ONE launch per direction: the forward with the training tapes, and the BPTT
// through the feedback.  fp32 throughout (v_mfma_f32_16x16x4_f32, exact expf / tanhf).
//
//   forward,  t = 0 .. T-1:   z1 = b1 + x_t . K1 + h1 . R1;    cell update -> h1_t, c1_t
//                             z2 = b2 + h1_t . K2 + h2 . R2;   cell update -> h2_t, c2_t
//                             y_t = tanh(bd + h2_t . W + ctx[:, t]);   x_{t+1} = y_t            (sums in exactly this order)
//   backward, t = T-1 .. 0:   dy_t = dloss_t + dx_{t+1};  dpre_t = dy_t (1 - y_t^2)
//                             dh2 = dpre_t . W^T + dz2_{t+1} . R2^T;  gate backward (c_{t-1} = C2[t]) -> dz2_t
//                             dh1 = dz2_t . K2^T + dz1_{t+1} . R1^T;  gate backward (c_{t-1} = C1[t]) -> dz1_t
//                             dx_t = dz1_t . K1^T
//
// Ownership (both kernels): stacked_tile.h's.  One workgroup owns one tile of 16 sequences for both layers and every step; the
// grid is the number of tiles and workgroups never communicate: no exchange, no workspace, no wait, any grid size runs.  H / 16
// waves; wave w owns units [16 w, 16 w + 16) of all four gates of both layers; lane (n, g4) holds unit 16 w + n for the sequences
// 4 g4 .. 4 g4 + 3, so both cell updates and both gate backwards are lane-local and c / dc never leave registers.  Rows of a
// ragged last tile beyond B read zeros (masked, not clamped) and store nothing; MFMA rows are independent, so a sequence's result
// does not depend on its tile-mates or on its place in the batch.
//
// Forward.  K1 (O <= 8 rows), R1, K2, R2 and the head's W^T fragments stay in registers for the whole launch.  The running h
// tile of EACH layer lies in LDS twice (step parity): layer 1 of step t reads h1 of parity t-1 and writes parity t; layer 2
// reads h1 of parity t and h2 of parity t-1 and writes h2 of parity t; the head reads h2 of parity t.  TWO barriers per step,
// one behind each layer's h store (2 T + 1 per launch with the one behind the initial state).  The head runs as
// y^T = W^T . h2^T, which leaves y[sequence n][output 4 g4 + r] in register r of lane (n, g4): exactly the A fragment of the
// next step's x . K1; every wave computes the (tiny) head itself.  The next step's ctx row is loaded behind the first barrier,
// under layer 2's products and the head.
//
// Backward (H = 32; at H = 64 the three resident matrices would be 192 KB of LDS).  R2^T, K2^T and R1^T lie in LDS in B-operand
// order (lstm_selffed.hip's layout: one ds_read_b128 feeds four k-steps; 3 x 16 KB) next to the two dz tiles of the step
// (16 x 4 H each).  TWO barriers per step, one behind each layer's dz store: dz2_t . R2^T (for the step below) and
// dz2_t . K2^T follow the first, dz1_t . R1^T and dx_t follow the second.  dx^T = K1 . dz1^T comes out in the fragment layout
// of the forward's y; every wave contracts all 4 H gate columns itself (K1's fragments are 32 registers), so the feedback
// needs no partial sums and no third barrier.  The next step's tape rows are loaded under the step's products: layer 2's,
// dloss and y behind the first barrier, layer 1's behind the second.
#include "selffed2_tile.h"

namespace fov {

namespace {

struct SelfFed2FwdParams {
    const float *x0, *h1_0, *c1_0, *h2_0, *c2_0, *K1, *R1, *b1, *K2, *R2, *b2, *W, *bd, *ctx;
    float *H1, *C1, *H2, *C2, *XY, *RES1, *RES2, *y, *hT, *cT;
    int B, T, O;
};

struct SelfFed2BwdParams {
    const float *C1, *C2, *XY, *RES1, *RES2, *dloss, *K1, *R1, *K2, *R2, *W;
    float *DPRE, *DZ1, *DZ2, *dx0, *dh1_0, *dc1_0, *dh2_0, *dc2_0;
    int B, T, O;
};

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void selffed2_fwd_kernel(SelfFed2FwdParams p) {
    constexpr int NJ = HP / 16, H4 = 4 * HP, LDH = ss_ldh(HP), HT = SS_BT * LDH;
    __shared__ __attribute__((aligned(16))) float sH[4 * HT];   // [layer][parity][16][LDH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SS_BT;
    const int B = p.B, T = p.T, O = p.O;
    const size_t BH = (size_t)B * HP, BO = (size_t)B * O;
    const float* a_rd = sH + n * LDH + 4 * g4;          // + (2 layer + parity) HT: this lane's A fragments
    float* h_wr = sH + 4 * g4 * LDH + unit;             // + (2 layer + parity) HT: this lane's four h values (rows 4 g4 + r)

    // ---- weights: registers for the whole launch ----
    float wK1[4][4], wR1[NJ][4][4], wK2[NJ][4][4], wR2[NJ][4][4], bias1[4], bias2[4], wd[NJ][4], dbv[4], xa[4], cx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)      // k-step r of x . K1 contracts input row 4 g4 + r (zero from O on)
#pragma unroll
        for (int g = 0; g < 4; ++g) wK1[r][g] = (4 * g4 + r < O) ? p.K1[(size_t)(4 * g4 + r) * H4 + g * HP + unit] : 0.f;
    load_frag<HP>(wR1, p.R1, unit, g4);
    load_frag<HP>(wK2, p.K2, unit, g4);
    load_frag<HP>(wR2, p.R2, unit, g4);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) wd[j][s] = (n < O) ? p.W[(size_t)(16 * j + 4 * g4 + s) * O + n] : 0.f;   // head: A operand W^T, row = output n
    load_bias<HP>(bias1, p.b1, unit);
    load_bias<HP>(bias2, p.b2, unit);
    const bool row_live = b0 + n < B;
    const float* ctx_row = p.ctx ? p.ctx + (size_t)(b0 + n) * T * O + 4 * g4 : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = 4 * g4 + r;
        const bool o_live = o < O && row_live;
        dbv[r] = (p.bd && o < O) ? p.bd[o] : 0.f;
        xa[r] = o_live ? p.x0[(size_t)(b0 + n) * O + o] : 0.f;
        cx[r] = (ctx_row && o_live && T > 0) ? ctx_row[r] : 0.f;
        if (p.XY && wave == 0 && o_live) p.XY[(size_t)(b0 + n) * O + o] = xa[r];
    }
    // ---- initial states: registers, the tiles of parity 1 (step 0 reads them), tape row 0 ----
    float c1[4], h1[4], c2[4], h2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        const bool live = row < B;
        const size_t at = (size_t)row * HP + unit;
        h1[r] = (p.h1_0 && live) ? p.h1_0[at] : 0.f;
        c1[r] = (p.c1_0 && live) ? p.c1_0[at] : 0.f;
        h2[r] = (p.h2_0 && live) ? p.h2_0[at] : 0.f;
        c2[r] = (p.c2_0 && live) ? p.c2_0[at] : 0.f;
        h_wr[HT + r * LDH] = h1[r];
        h_wr[3 * HT + r * LDH] = h2[r];
        if (live) {
            if (p.H1) p.H1[at] = h1[r];
            if (p.C1) p.C1[at] = c1[r];
            if (p.H2) p.H2[at] = h2[r];
            if (p.C2) p.C2[at] = c2[r];
        }
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, prv = cur ^ 1;
        f32x4 acc[4];
        // ---- layer 1: z1 = b1 + x_t . K1 + h1 . R1 ----
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias1[g], bias1[g], bias1[g], bias1[g]};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[r], wK1[r][g], acc[g], 0, 0, 0);
        mm_frag<NJ>(acc, a_rd + prv * HT, wR1);
        s2_cell<HP, ACT>(acc, c1, h1, h_wr + cur * HT, p.H1, p.C1, p.RES1, t, t + 1, B, b0 + 4 * g4, unit);
        __syncthreads();
        // the next step's context row, under layer 2 and the head
        float cn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) cn[r] = (ctx_row && 4 * g4 + r < O && row_live && t + 1 < T) ? ctx_row[(size_t)(t + 1) * O + r] : 0.f;
        // ---- layer 2: z2 = b2 + h1_t . K2 + h2 . R2 ----
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias2[g], bias2[g], bias2[g], bias2[g]};
        mm_frag<NJ>(acc, a_rd + cur * HT, wK2);
        mm_frag<NJ>(acc, a_rd + (2 + prv) * HT, wR2);
        s2_cell<HP, ACT>(acc, c2, h2, h_wr + (2 + cur) * HT, p.H2, p.C2, p.RES2, t, t + 1, B, b0 + 4 * g4, unit);
        __syncthreads();
        // ---- head: y_t = tanh(bd + h2_t . W + ctx_t), every wave for itself ----
        f32x4 yacc = {dbv[0], dbv[1], dbv[2], dbv[3]};
        const float* ht = a_rd + (2 + cur) * HT;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x4 hv = *(const f32x4*)(ht + 16 * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) yacc = __builtin_amdgcn_mfma_f32_16x16x4f32(wd[j][s], hv[s], yacc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xa[r] = (4 * g4 + r < O) ? tanh_f(yacc[r] + cx[r]) : 0.f;
            cx[r] = cn[r];
        }
        if (wave == 0 && row_live) {
            const size_t at = (size_t)(t + 1) * BO + (size_t)(b0 + n) * O + 4 * g4;
            float* yp = p.y ? p.y + ((size_t)(b0 + n) * T + t) * O + 4 * g4 : nullptr;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g4 + r < O) {
                    if (p.XY) p.XY[at + r] = xa[r];
                    if (yp) yp[r] = xa[r];
                }
        }
    }
    // ---- final states (2,B,H) ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        if (row < B) {
            const size_t at = (size_t)row * HP + unit;
            if (p.hT) { p.hT[at] = h1[r]; p.hT[BH + at] = h2[r]; }
            if (p.cT) { p.cT[at] = c1[r]; p.cT[BH + at] = c2[r]; }
        }
    }
}

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void selffed2_bwd_kernel(SelfFed2BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float s2_smem[];
    constexpr int H4 = 4 * HP, NJ4 = H4 / 16, LDZ = s2_ldz(HP);
    f32x4* sR2T = (f32x4*)s2_smem;                        // [NW][NJ4][64]
    f32x4* sK2T = sR2T + HP * H4 / 4;
    f32x4* sR1T = sK2T + HP * H4 / 4;
    float* sZ2 = s2_smem + 3 * HP * H4;                   // [16][LDZ]: dz2 of the step
    float* sZ1 = sZ2 + SS_BT * LDZ;                       // [16][LDZ]: dz1 of the step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SS_BT;
    const int B = p.B, T = p.T, O = p.O;
    const size_t BO = (size_t)B * O;
    const bool row_live = b0 + n < B;
    const int slice = wave * NJ4 * 64;

    s2_stage_bt<HP>(sR2T + slice, p.R2, unit, n, g4);
    s2_stage_bt<HP>(sK2T + slice, p.K2, unit, n, g4);
    s2_stage_bt<HP>(sR1T + slice, p.R1, unit, n, g4);
    float kA[NJ4][4], wWT[4];
#pragma unroll
    for (int j = 0; j < NJ4; ++j)         // dx^T = K1 . dz1^T: A operand K1, row = input n (zero from O on)
#pragma unroll
        for (int s = 0; s < 4; ++s) kA[j][s] = (n < O) ? p.K1[(size_t)n * H4 + 16 * j + 4 * g4 + s] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) wWT[r] = (4 * g4 + r < O) ? p.W[(size_t)unit * O + 4 * g4 + r] : 0.f;

    S2Tape t1, t2;
    float dl[4], yv[4];     // dloss_t and y_t of (sequence n, output 4 g4 + r)
    auto load_head = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool o_live = 4 * g4 + r < O && row_live;
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4 + r;
            dl[r] = o_live ? p.dloss[at] : 0.f;
            yv[r] = o_live ? p.XY[BO + at] : 0.f;
        }
    };
    load_head(T - 1);
    s2_load_tape<HP>(t2, p.RES2, p.C2, T - 1, B, b0 + 4 * g4, unit);
    s2_load_tape<HP>(t1, p.RES1, p.C1, T - 1, B, b0 + 4 * g4, unit);
    f32x4 dhR2 = {0.f, 0.f, 0.f, 0.f}, dhR1 = {0.f, 0.f, 0.f, 0.f}, dxv = {0.f, 0.f, 0.f, 0.f};
    float dc2[4] = {0.f, 0.f, 0.f, 0.f}, dc1[4] = {0.f, 0.f, 0.f, 0.f};
    const float* zr2 = sZ2 + n * LDZ + 4 * g4;
    const float* zr1 = sZ1 + n * LDZ + 4 * g4;
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        // ---- dy_t = dloss_t + dx_{t+1}; dpre_t = dy_t (1 - y_t^2) ----
        float dpre[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) dpre[r] = (dl[r] + dxv[r]) * (1.f - yv[r] * yv[r]);
        if (wave == 0 && row_live) {
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g4 + r < O) p.DPRE[at + r] = dpre[r];
        }
        // ---- dh2 = dpre_t . W^T + dz2_{t+1} . R2^T; layer 2's gate backward ----
        f32x4 dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) dh = __builtin_amdgcn_mfma_f32_16x16x4f32(dpre[r], wWT[r], dh, 0, 0, 0);
        dh += dhR2;
        s2_gate_bwd<HP, ACT>(t2, dh, dc2, sZ2 + 4 * g4 * LDZ + unit, p.DZ2, t, B, b0 + 4 * g4, unit);
        __syncthreads();
        if (t > 0) {
            load_head(t - 1);
            s2_load_tape<HP>(t2, p.RES2, p.C2, t - 1, B, b0 + 4 * g4, unit);
        }
        // ---- dh1 = dz2_t . K2^T + dz1_{t+1} . R1^T; dz2_t . R2^T for the step below (dh2_0 after the last one) ----
        dh = s2_mm_bt<NJ4>(zr2, sK2T + slice + lane) + dhR1;
        dhR2 = s2_mm_bt<NJ4>(zr2, sR2T + slice + lane);
        s2_gate_bwd<HP, ACT>(t1, dh, dc1, sZ1 + 4 * g4 * LDZ + unit, p.DZ1, t, B, b0 + 4 * g4, unit);
        __syncthreads();
        if (t > 0) s2_load_tape<HP>(t1, p.RES1, p.C1, t - 1, B, b0 + 4 * g4, unit);
        // ---- dz1_t . R1^T for the step below (dh1_0 after the last one); dx_t^T = K1 . dz1_t^T, every wave for itself ----
        dhR1 = s2_mm_bt<NJ4>(zr1, sR1T + slice + lane);
        {
            f32x4 px[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int j = 0; j < NJ4; ++j) {
                const f32x4 zv = *(const f32x4*)(zr1 + 16 * j);
#pragma unroll
                for (int s = 0; s < 4; ++s) px[j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(kA[j][s], zv[s], px[j & 1], 0, 0, 0);
            }
            dxv = px[0] + px[1];
        }
    }

    if (p.dx0 && wave == 0 && row_live) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * g4 + r < O) p.dx0[(size_t)(b0 + n) * O + 4 * g4 + r] = dxv[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        if (row < B) {
            const size_t at = (size_t)row * HP + unit;
            if (p.dh1_0) p.dh1_0[at] = dhR1[r];
            if (p.dc1_0) p.dc1_0[at] = dc1[r];
            if (p.dh2_0) p.dh2_0[at] = dhR2[r];
            if (p.dc2_0) p.dc2_0[at] = dc2[r];
        }
    }
}

template <int HP>
int launch_selffed2_fwd(const SelfFed2FwdParams& p, int act, hipStream_t stream) {
    void (*kern)(SelfFed2FwdParams) = act == FOV_ACT_HARD_SIGMOID ? selffed2_fwd_kernel<HP, FOV_ACT_HARD_SIGMOID> : selffed2_fwd_kernel<HP, FOV_ACT_SIGMOID>;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), 0, stream, p);
    return launch_check("self-fed 2-layer decoder forward");
}

int launch_selffed2_bwd(const SelfFed2BwdParams& p, int act, hipStream_t stream) {
    constexpr int HP = 32;
    void (*kern)(SelfFed2BwdParams) = act == FOV_ACT_HARD_SIGMOID ? selffed2_bwd_kernel<HP, FOV_ACT_HARD_SIGMOID> : selffed2_bwd_kernel<HP, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)s2_bwd_lds_floats(HP) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("self-fed 2-layer decoder backward");
}

int selffed2_refuse(const char* entry, const char* widths, int B, int T, int O, int H) {
    set_error("%s: H = %s, 1 <= O <= 8 and non-negative sizes only (got B=%d T=%d O=%d H=%d)", entry, widths, B, T, O, H);
    return FOV_ERR_UNSUPPORTED;
}

}  // namespace

// pure arithmetic: no device query.  The backward keeps R2^T, K2^T and R1^T in LDS: 48 KB at H = 32, 192 KB (> 160 KB) at H = 64
bool selffed2_shape_ok(int B, int T, int O, int H, bool backward) {
    return B >= 0 && B <= kMaxTileBatch && T >= 0 && T <= kMaxTileBatch && (H == 32 || (H == 64 && !backward)) && O >= 1 && O <= 8;
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_selffed2_decoder_supported(int B, int T, int O, int H, int backward) {
    return (!env_knobs().no_selffed2_fused && selffed2_shape_ok(B, T, O, H, backward != 0)) ? 1 : 0;
}

int fov_selffed2_decoder_fwd(const float* x0, const float* h1_0, const float* c1_0, const float* h2_0, const float* c2_0,
                             const float* K1, const float* R1, const float* b1, const float* K2, const float* R2, const float* b2,
                             const float* W, const float* bd, const float* ctx, float* H1, float* C1, float* H2, float* C2, float* XY,
                             float* RES1, float* RES2, float* y, float* hT, float* cT, int B, int T, int O, int H, int act,
                             fov_stream_t stream) {
    if (!selffed2_shape_ok(B, T, O, H, false)) return selffed2_refuse("fov_selffed2_decoder_fwd", "32 or 64", B, T, O, H);   // before any HIP call
    const bool work = B > 0 && T > 0;
    if (!K1 || !R1 || !b1 || !K2 || !R2 || !b2 || !W || (work && !x0) || !valid_act(act)) {
        set_error("fov_selffed2_decoder_fwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!work) return FOV_OK;
    SelfFed2FwdParams p = {x0, h1_0, c1_0, h2_0, c2_0, K1, R1, b1, K2, R2, b2, W, bd, ctx, H1, C1, H2, C2, XY, RES1, RES2, y, hT, cT, B, T, O};
    return H == 32 ? launch_selffed2_fwd<32>(p, act, (hipStream_t)stream) : launch_selffed2_fwd<64>(p, act, (hipStream_t)stream);
}

int fov_selffed2_decoder_bwd(const float* C1, const float* C2, const float* XY, const float* RES1, const float* RES2, const float* dloss,
                             const float* K1, const float* R1, const float* K2, const float* R2, const float* W, float* DPRE, float* DZ1,
                             float* DZ2, float* dx0, float* dh1_0, float* dc1_0, float* dh2_0, float* dc2_0, int B, int T, int O, int H,
                             int act, fov_stream_t stream) {
    if (!selffed2_shape_ok(B, T, O, H, true)) return selffed2_refuse("fov_selffed2_decoder_bwd", "32", B, T, O, H);   // before any HIP call
    const bool work = B > 0 && T > 0;
    if (!K1 || !R1 || !K2 || !R2 || !W || (work && (!C1 || !C2 || !XY || !RES1 || !RES2 || !dloss || !DPRE || !DZ1 || !DZ2)) ||
        !valid_act(act)) {
        set_error("fov_selffed2_decoder_bwd: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (B == 0) return FOV_OK;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {   // no step and no gradient of the final states comes in: all five are zero
        hipError_t e = hipSuccess;
        if (dx0) e = hipMemsetAsync(dx0, 0, sizeof(float) * (size_t)B * O, st);
        for (float* s : {dh1_0, dc1_0, dh2_0, dc2_0})
            if (e == hipSuccess && s) e = hipMemsetAsync(s, 0, sizeof(float) * (size_t)B * H, st);
        if (e != hipSuccess) { set_error("fov_selffed2_decoder_bwd: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
        return FOV_OK;
    }
    SelfFed2BwdParams p = {C1, C2, XY, RES1, RES2, dloss, K1, R1, K2, R2, W, DPRE, DZ1, DZ2, dx0, dh1_0, dc1_0, dh2_0, dc2_0, B, T, O};
    return launch_selffed2_bwd(p, act, st);
}

}  // extern "C"
