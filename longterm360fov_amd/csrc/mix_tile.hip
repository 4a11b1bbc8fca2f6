// The unrolled others-mixing decoder of mycode/given_others_gt_mean_var_seq2seq.py:203-299 (`mlp_mixing`, :166-168, 262-265) at
// the script's own width, latent_dim = 32 (:38), and at 64: ONE launch per direction behind fov_mix_decoder_fwd / _bwd, which
// run the eight-workgroups-per-tile exchange kernels (mix_decoder.hip, mix_decoder_bwd.hip) at H = 256.  fp32 throughout
// (v_mfma_f32_16x16x4_f32, exact expf / tanhf).  It is lstm_selffed2.hip's decoder with one more head stage:
//
//   forward,  t = 0 .. T-1:   z1 = b1 + x_t . K1 + h1 . R1;    cell update -> h1_t, c1_t
//                             z2 = b2 + h1_t . K2 + h2 . R2;   cell update -> h2_t, c2_t
//                             p_t = tanh(bd + h2_t . Wd);   m_t = tanh(p_t . Wp + oth_proj[:, t]);   x_{t+1} = m_t
//   backward, t = T-1 .. 0:   dm_t = dloss_t + dx_{t+1} (1 - m_t^2)                 (dloss is already dL/d(pre-tanh of m_t))
//                             dpp_t = (dm_t . Wp^T) (1 - p_t^2)
//                             dh2 = dpp_t . Wd^T + dz2_{t+1} . R2^T;  gate backward (c_{t-1} = C2[t]) -> dz2_t
//                             dh1 = dz2_t . K2^T + dz1_{t+1} . R1^T;  gate backward (c_{t-1} = C1[t]) -> dz1_t
//                             dx_t = dz1_t . K1^T
//
// Ownership, LDS and barriers are lstm_selffed2.hip's: one workgroup per 16-sequence tile for both layers and every step on
// H / 16 waves, no exchange, no workspace, no wait, two barriers per step; rows beyond B read zeros and store nothing, and a
// sequence's result does not depend on its tile-mates.  Operands and tapes are the H = 256 kernels' (fov360.h): out, P
// (T,B,O) step-major, the state tapes (T,B,H) = the state AFTER step t with no row for the initial state, res (T,B,5,H); the
// backward reads C1 / C2 whose row t is the cell state BEFORE step t.
//
// The mixing stage.  The head runs as p^T = Wd^T . h2^T, which leaves p[sequence n][output 4 g4 + r] in register r of lane
// (n, g4).  That register is the B operand of m^T = Wp^T . p^T at k-step r (the k index g4 of the MFMA stands for input
// 4 g4 + r), against the A operand Wp[4 g4 + r][n]: four more MFMAs and four resident registers, and m comes out in the
// layout of p, which is the A fragment of the next step's x . K1.  The backward's mirror image: dm in that layout is the B
// operand of dp^T = Wp . dm^T against the A operand Wp[n][4 g4 + r].  The next step's oth_proj row is loaded behind the first
// barrier, under layer 2's products and the head; element (b, t, o) lies at b * oth_sb + t * oth_st + o, either stride may be 0.
#include "selffed2_tile.h"

namespace fov {

namespace {

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void mix_tile_fwd_kernel(MixDecParams p) {
    constexpr int NJ = HP / 16, H4 = 4 * HP, LDH = ss_ldh(HP), HT = SS_BT * LDH;
    __shared__ __attribute__((aligned(16))) float sH[4 * HT];   // [layer][parity][16][LDH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SS_BT;
    const int B = p.B, T = p.T_out, O = p.O;
    const size_t BO = (size_t)B * O;
    const float* a_rd = sH + n * LDH + 4 * g4;          // + (2 layer + parity) HT: this lane's A fragments
    float* h_wr = sH + 4 * g4 * LDH + unit;             // + (2 layer + parity) HT: this lane's four h values (rows 4 g4 + r)

    // ---- weights: registers for the whole launch ----
    float wK1[4][4], wR1[NJ][4][4], wK2[NJ][4][4], wR2[NJ][4][4], bias1[4], bias2[4], wd[NJ][4], wp[4], dbv[4], xa[4], cx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)      // k-step r of x . K1 contracts input row 4 g4 + r (zero from O on)
#pragma unroll
        for (int g = 0; g < 4; ++g) wK1[r][g] = (4 * g4 + r < O) ? p.K1[(size_t)(4 * g4 + r) * H4 + g * HP + unit] : 0.f;
    load_frag<HP>(wR1, p.R1, unit, g4);
    load_frag<HP>(wK2, p.K2p, unit, g4);
    load_frag<HP>(wR2, p.R2, unit, g4);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) wd[j][s] = (n < O) ? p.Wd[(size_t)(16 * j + 4 * g4 + s) * O + n] : 0.f;   // head: A operand Wd^T, row = output n
    load_bias<HP>(bias1, p.b1, unit);
    load_bias<HP>(bias2, p.b2, unit);
    const bool row_live = b0 + n < B;
    const float* oth_row = p.oth_proj + (size_t)(b0 + n) * p.oth_sb + 4 * g4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = 4 * g4 + r;
        const bool o_live = o < O && row_live;
        wp[r] = (o < O && n < O) ? p.Wp[(size_t)o * O + n] : 0.f;      // mixing: A operand Wp^T, row = output n, k-step r = input o
        dbv[r] = o < O ? p.bd[o] : 0.f;
        xa[r] = o_live ? p.dec0[(size_t)(b0 + n) * O + o] : 0.f;
        cx[r] = o_live ? oth_row[r] : 0.f;
    }
    // ---- initial states: registers and the tiles of parity 1 (step 0 reads them) ----
    float c1[4], h1[4], c2[4], h2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        const bool live = row < B;
        const size_t at = (size_t)row * HP + unit;
        h1[r] = live ? p.h1_0[at] : 0.f;
        c1[r] = live ? p.c1_0[at] : 0.f;
        h2[r] = live ? p.h2_0[at] : 0.f;
        c2[r] = live ? p.c2_0[at] : 0.f;
        h_wr[HT + r * LDH] = h1[r];
        h_wr[3 * HT + r * LDH] = h2[r];
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
        s2_cell<HP, ACT>(acc, c1, h1, h_wr + cur * HT, p.H1, p.C1, p.res1, t, t, B, b0 + 4 * g4, unit);
        __syncthreads();
        // the next step's row of the others' projection, under layer 2 and the head
        float cn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) cn[r] = (4 * g4 + r < O && row_live && t + 1 < T) ? oth_row[(size_t)(t + 1) * p.oth_st + r] : 0.f;
        // ---- layer 2: z2 = b2 + h1_t . K2 + h2 . R2 ----
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = (f32x4){bias2[g], bias2[g], bias2[g], bias2[g]};
        mm_frag<NJ>(acc, a_rd + cur * HT, wK2);
        mm_frag<NJ>(acc, a_rd + (2 + prv) * HT, wR2);
        s2_cell<HP, ACT>(acc, c2, h2, h_wr + (2 + cur) * HT, p.H2, p.C2, p.res2, t, t, B, b0 + 4 * g4, unit);
        __syncthreads();
        // ---- head: p_t = tanh(bd + h2_t . Wd), every wave for itself ----
        f32x4 pacc = {dbv[0], dbv[1], dbv[2], dbv[3]};
        const float* ht = a_rd + (2 + cur) * HT;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x4 hv = *(const f32x4*)(ht + 16 * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(wd[j][s], hv[s], pacc, 0, 0, 0);
        }
        float pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[r] = (4 * g4 + r < O) ? tanh_f(pacc[r]) : 0.f;
        // ---- mixing: m_t = tanh(p_t . Wp + oth_proj_t) ----
        f32x4 macc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) macc = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[r], pv[r], macc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xa[r] = (4 * g4 + r < O) ? tanh_f(macc[r] + cx[r]) : 0.f;
            cx[r] = cn[r];
        }
        if (wave == 0 && row_live) {
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g4 + r < O) {
                    p.out[at + r] = xa[r];
                    if (p.P) p.P[at + r] = pv[r];
                }
        }
    }
    // ---- final states (B,H) each ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        if (row < B) {
            const size_t at = (size_t)row * HP + unit;
            if (p.h1T) p.h1T[at] = h1[r];
            if (p.c1T) p.c1T[at] = c1[r];
            if (p.h2T) p.h2T[at] = h2[r];
            if (p.c2T) p.c2T[at] = c2[r];
        }
    }
}

template <int HP, int ACT>
__global__ __launch_bounds__(4 * HP, 1) void mix_tile_bwd_kernel(MixDecBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float mt_smem[];
    constexpr int H4 = 4 * HP, NJ4 = H4 / 16, LDZ = s2_ldz(HP);
    f32x4* sR2T = (f32x4*)mt_smem;                        // [NW][NJ4][64]
    f32x4* sK2T = sR2T + HP * H4 / 4;
    f32x4* sR1T = sK2T + HP * H4 / 4;
    float* sZ2 = mt_smem + 3 * HP * H4;                   // [16][LDZ]: dz2 of the step
    float* sZ1 = sZ2 + SS_BT * LDZ;                       // [16][LDZ]: dz1 of the step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g4 = lane >> 4;
    const int unit = 16 * wave + n;
    const int b0 = blockIdx.x * SS_BT;
    const int B = p.B, T = p.T_out, O = p.O;
    const size_t BO = (size_t)B * O;
    const bool row_live = b0 + n < B;
    const int slice = wave * NJ4 * 64;

    s2_stage_bt<HP>(sR2T + slice, p.R2, unit, n, g4);
    s2_stage_bt<HP>(sK2T + slice, p.K2p, unit, n, g4);
    s2_stage_bt<HP>(sR1T + slice, p.R1, unit, n, g4);
    float kA[NJ4][4], wWT[4], wpA[4];
#pragma unroll
    for (int j = 0; j < NJ4; ++j)         // dx^T = K1 . dz1^T: A operand K1, row = input n (zero from O on)
#pragma unroll
        for (int s = 0; s < 4; ++s) kA[j][s] = (n < O) ? p.K1[(size_t)n * H4 + 16 * j + 4 * g4 + s] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        wWT[r] = (4 * g4 + r < O) ? p.Wd[(size_t)unit * O + 4 * g4 + r] : 0.f;
        wpA[r] = (n < O && 4 * g4 + r < O) ? p.Wp[(size_t)n * O + 4 * g4 + r] : 0.f;   // dp^T = Wp . dm^T: A operand Wp, row = input n
    }

    S2Tape t1, t2;
    float dl[4], mv[4], pv[4];     // dloss_t, m_t and p_t of (sequence n, output 4 g4 + r)
    auto load_head = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool o_live = 4 * g4 + r < O && row_live;
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4 + r;
            dl[r] = o_live ? p.dloss[at] : 0.f;
            mv[r] = o_live ? p.M[at] : 0.f;
            pv[r] = o_live ? p.P[at] : 0.f;
        }
    };
    load_head(T - 1);
    s2_load_tape<HP>(t2, p.res2, p.C2, T - 1, B, b0 + 4 * g4, unit);
    s2_load_tape<HP>(t1, p.res1, p.C1, T - 1, B, b0 + 4 * g4, unit);
    f32x4 dhR2 = {0.f, 0.f, 0.f, 0.f}, dhR1 = {0.f, 0.f, 0.f, 0.f}, dxv = {0.f, 0.f, 0.f, 0.f};
    float dc2[4] = {0.f, 0.f, 0.f, 0.f}, dc1[4] = {0.f, 0.f, 0.f, 0.f};
    const float* zr2 = sZ2 + n * LDZ + 4 * g4;
    const float* zr1 = sZ1 + n * LDZ + 4 * g4;
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        // ---- dm_t = dloss_t + dx_{t+1} (1 - m_t^2); dpp_t = (dm_t . Wp^T) (1 - p_t^2) ----
        float dm[4], dpp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) dm[r] = fmaf(dxv[r], 1.f - mv[r] * mv[r], dl[r]);
        f32x4 dpa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) dpa = __builtin_amdgcn_mfma_f32_16x16x4f32(wpA[r], dm[r], dpa, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) dpp[r] = dpa[r] * (1.f - pv[r] * pv[r]);
        if (wave == 0 && row_live) {
            const size_t at = (size_t)t * BO + (size_t)(b0 + n) * O + 4 * g4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g4 + r < O) {
                    p.dpre_m[at + r] = dm[r];
                    p.dpre_p[at + r] = dpp[r];
                }
        }
        // ---- dh2 = dpp_t . Wd^T + dz2_{t+1} . R2^T; layer 2's gate backward ----
        f32x4 dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) dh = __builtin_amdgcn_mfma_f32_16x16x4f32(dpp[r], wWT[r], dh, 0, 0, 0);
        dh += dhR2;
        s2_gate_bwd<HP, ACT>(t2, dh, dc2, sZ2 + 4 * g4 * LDZ + unit, p.DZ2, t, B, b0 + 4 * g4, unit);
        __syncthreads();
        if (t > 0) {
            load_head(t - 1);
            s2_load_tape<HP>(t2, p.res2, p.C2, t - 1, B, b0 + 4 * g4, unit);
        }
        // ---- dh1 = dz2_t . K2^T + dz1_{t+1} . R1^T; dz2_t . R2^T for the step below (dh2_0 after the last one) ----
        dh = s2_mm_bt<NJ4>(zr2, sK2T + slice + lane) + dhR1;
        dhR2 = s2_mm_bt<NJ4>(zr2, sR2T + slice + lane);
        s2_gate_bwd<HP, ACT>(t1, dh, dc1, sZ1 + 4 * g4 * LDZ + unit, p.DZ1, t, B, b0 + 4 * g4, unit);
        __syncthreads();
        if (t > 0) s2_load_tape<HP>(t1, p.res1, p.C1, t - 1, B, b0 + 4 * g4, unit);
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

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = b0 + 4 * g4 + r;
        if (row < B) {
            const size_t at = (size_t)row * HP + unit;
            p.dh1_0[at] = dhR1[r];
            p.dc1_0[at] = dc1[r];
            p.dh2_0[at] = dhR2[r];
            p.dc2_0[at] = dc2[r];
        }
    }
}

template <int HP>
int launch_mix_tile_fwd(const MixDecParams& p, int act, hipStream_t stream) {
    void (*kern)(MixDecParams) = act == FOV_ACT_HARD_SIGMOID ? mix_tile_fwd_kernel<HP, FOV_ACT_HARD_SIGMOID> : mix_tile_fwd_kernel<HP, FOV_ACT_SIGMOID>;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), 0, stream, p);
    return launch_check("mixing decoder forward, one workgroup per tile");
}

}  // namespace

// pure arithmetic: no device query.  The backward keeps R2^T, K2^T and R1^T in LDS: 48 KB at H = 32, 192 KB (> 160 KB) at H = 64
bool mix_tile_shape_ok(int B, int T_out, int H, int O, bool backward) {
    return B >= 0 && B <= kMaxTileBatch && T_out >= 0 && T_out <= kMaxTileBatch && (H == 32 || (H == 64 && !backward)) && O >= 1 && O <= 8;
}

// p.K2p carries dec2_K itself (Keras layout, not a packed copy); the exchange fields of the parameter structs are not read
int mix_tile_fwd_launch(const MixDecParams& p, int H, int act, hipStream_t stream) {
    return H == 32 ? launch_mix_tile_fwd<32>(p, act, stream) : launch_mix_tile_fwd<64>(p, act, stream);
}

int mix_tile_bwd_launch(const MixDecBwdParams& p, int act, hipStream_t stream) {
    constexpr int HP = 32;
    void (*kern)(MixDecBwdParams) = act == FOV_ACT_HARD_SIGMOID ? mix_tile_bwd_kernel<HP, FOV_ACT_HARD_SIGMOID> : mix_tile_bwd_kernel<HP, FOV_ACT_SIGMOID>;
    const size_t lds = (size_t)s2_bwd_lds_floats(HP) * sizeof(float);
    if (int rc = ensure_dynamic_lds((const void*)kern, lds, 4 * HP)) return rc;
    hipLaunchKernelGGL(kern, dim3((p.B + SS_BT - 1) / SS_BT), dim3(4 * HP), lds, stream, p);
    return launch_check("mixing decoder backward, one workgroup per tile");
}

}  // namespace fov
