// Device helpers the two-layer self-fed decoders share (lstm_selffed2.hip: additive context inside the head's tanh;
// mix_tile.hip: the others-mixing head behind it): the cell update that writes the training tapes, the backward's tape
// loads, gate backward, the staging of a transposed matrix into LDS and the product against it.  Ownership and fragment
// layouts are stacked_tile.h's.
#pragma once
#include "stacked_tile.h"

namespace fov {

namespace {

__host__ __device__ constexpr int s2_ldz(int HP) { return 4 * HP + 4; }
// floats of the backward's LDS: R2^T, K2^T, R1^T in B-operand order, the dz tiles of the two layers
__host__ __device__ constexpr int s2_bwd_lds_floats(int HP) { return 3 * HP * 4 * HP + 2 * SS_BT * s2_ldz(HP); }

// the cell update of this lane's unit for its four sequences; h into the layer's tile of this step; the tape rows of step t
// (Hs / Cs: row `srow` of the state stacks - t + 1 where row 0 is the initial state, t where the stacks have no such row)
template <int HP, int ACT>
__device__ __forceinline__ void s2_cell(const f32x4 (&acc)[4], float (&c)[4], float (&h)[4], float* hw, float* Hs, float* Cs, float* RES,
                                        int t, int srow, int B, int row0, int unit) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float ig = rec_act<ACT>(acc[0][r]), fg = rec_act<ACT>(acc[1][r]), gg = tanh_f(acc[2][r]), og = rec_act<ACT>(acc[3][r]);
        c[r] = fmaf(fg, c[r], ig * gg);
        h[r] = og * tanh_f(c[r]);
        hw[r * ss_ldh(HP)] = h[r];
        const int row = row0 + r;
        if (row < B) {
            const size_t at = ((size_t)srow * B + row) * HP + unit;
            if (Hs) Hs[at] = h[r];
            if (Cs) Cs[at] = c[r];
            if (RES) {
                float* q = RES + ((size_t)t * B + row) * 5 * HP + unit;
                q[0] = ig; q[HP] = fg; q[2 * HP] = gg; q[3 * HP] = og; q[4 * HP] = c[r];
            }
        }
    }
}

// one step's tape rows of one layer: gates, c_t, c_{t-1} of (row 4 g4 + r, unit)
struct S2Tape { float gi[4], gf[4], gg[4], go[4], cc[4], cp[4]; };

template <int HP>
__device__ __forceinline__ void s2_load_tape(S2Tape& tp, const float* RES, const float* Cs, int t, int B, int row0, int unit) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + r;
        const bool live = row < B;
        const float* q = RES + ((size_t)t * B + row) * 5 * HP + unit;
        tp.gi[r] = live ? q[0] : 0.f;
        tp.gf[r] = live ? q[HP] : 0.f;
        tp.gg[r] = live ? q[2 * HP] : 0.f;
        tp.go[r] = live ? q[3 * HP] : 0.f;
        tp.cc[r] = live ? q[4 * HP] : 0.f;
        tp.cp[r] = live ? Cs[((size_t)t * B + row) * HP + unit] : 0.f;
    }
}

// gate backward of this lane's unit for its four sequences; dz_t to the layer's tile and to the tape
template <int HP, int ACT>
__device__ __forceinline__ void s2_gate_bwd(const S2Tape& tp, const f32x4& dh, float (&dc)[4], float* zt, float* DZ, int t, int B, int row0,
                                            int unit) {
    constexpr int H4 = 4 * HP, LDZ = s2_ldz(HP);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float tc = tanh_f(tp.cc[r]);
        const float dov = dh[r] * tc;
        const float dcv = dc[r] + dh[r] * tp.go[r] * (1.f - tc * tc);
        float dz[4];
        dz[0] = dcv * tp.gg[r] * rec_act_grad<ACT>(tp.gi[r]);
        dz[1] = dcv * tp.cp[r] * rec_act_grad<ACT>(tp.gf[r]);
        dz[2] = dcv * tp.gi[r] * (1.f - tp.gg[r] * tp.gg[r]);
        dz[3] = dov * rec_act_grad<ACT>(tp.go[r]);
        dc[r] = dcv * tp.gf[r];
        const int row = row0 + r;
        float* zg = DZ + ((size_t)t * B + row) * H4 + unit;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            zt[r * LDZ + g * HP] = dz[g];
            if (row < B) zg[g * HP] = dz[g];
        }
    }
}

// a (HP, 4 HP) matrix M into LDS as the B operand of dz . M^T: this wave's slice [NJ4][64] {s = 0..3} = M[16 w + n][16 jj + 4 g4 + s].
// Here the lane is (n, s): four consecutive floats of a row of M are one lane's b128 later.
template <int HP>
__device__ __forceinline__ void s2_stage_bt(f32x4* dst4, const float* M, int unit, int n, int g4) {
    constexpr int H4 = 4 * HP;
    const float* row = M + (size_t)unit * H4;
    float* dst = (float*)dst4;
    for (int q = 0; q < H4 / 4; ++q) dst[(q * 16 + n) * 4 + g4] = row[4 * q + g4];
}

// dz . M^T for this wave's 16 units: four accumulators, summed in a fixed order
template <int NJ4>
__device__ __forceinline__ f32x4 s2_mm_bt(const float* zr, const f32x4* bt) {
    f32x4 a4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a4[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < NJ4; ++jj) {
        const f32x4 zv = *(const f32x4*)(zr + 16 * jj);
        const f32x4 rv = bt[jj * 64];
#pragma unroll
        for (int s = 0; s < 4; ++s) a4[jj & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[s], rv[s], a4[jj & 3], 0, 0, 0);
    }
    return (a4[0] + a4[1]) + (a4[2] + a4[3]);
}

}  // namespace

}  // namespace fov
