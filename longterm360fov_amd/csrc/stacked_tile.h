// Device helpers of the kernels in which ONE workgroup owns a tile of 16 sequences for every layer and every step
// (lstm_stacked_s2s.hip, lstm_stacked_train.hip): HP / 16 waves, wave w owns units [16 w, 16 w + 16) of all four gates, and
// lane (n, g4) holds unit 16 w + n for the sequences 4 g4 .. 4 g4 + 3.  fp32 on v_mfma_f32_16x16x4_f32.
//
// Weights.  A (Kd, 4 HP) matrix is Kd registers per lane as B operands, w[j][s][g] = W[16 j + 4 g4 + s][g HP + unit] (the k
// order inside a 16-block is a permutation the A operand shares: one ds_read_b128 of a tile row feeds four k-steps).
#pragma once
#include "fov_common.h"

namespace fov {

namespace {

constexpr int SS_BT = 16;         // sequences per tile
constexpr int SS_MAX_F = 96;      // encoder input features
constexpr int SS_LDX = SS_MAX_F + 4;
constexpr unsigned SS_RSRC = 0x00020000;

__host__ __device__ constexpr int ss_ldh(int HP) { return HP + 4; }
// floats of LDS: 3 layers x 2 parities of h, two x tiles, nkb k-blocks of K_0 in B-operand order
__host__ __device__ constexpr int ss_lds_floats(int HP, int nkb) { return 6 * SS_BT * ss_ldh(HP) + 2 * SS_BT * SS_LDX + nkb * 4 * (4 * HP) * 4; }

// this lane's B fragments of a (HP, 4 HP) matrix: every row exists, the (j, s, g) part of the address is the scalar offset
template <int HP>
__device__ __forceinline__ void load_frag(float (&w)[HP / 16][4][4], const float* W, int unit, int g4) {
    constexpr int H4 = 4 * HP;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, HP * H4 * 4, SS_RSRC);
    const unsigned voff = (unsigned)((4 * g4 * H4 + unit) * 4);
#pragma unroll
    for (int j = 0; j < HP / 16; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                w[j][s][g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, (unsigned)(((16 * j + s) * H4 + g * HP) * 4), 0));
}

template <int HP>
__device__ __forceinline__ void load_bias(float (&b)[4], const float* bias, int unit) {
#pragma unroll
    for (int g = 0; g < 4; ++g) b[g] = bias[g * HP + unit];
}

// acc += A . W for a 16 x HP tile in LDS (a = the lane's row n, columns 4 g4 ..) and resident fragments
template <int NJ>
__device__ __forceinline__ void mm_frag(f32x4 (&acc)[4], const float* a, const float (&w)[NJ][4][4]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const f32x4 av = *(const f32x4*)(a + 16 * j);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], w[j][s][g], acc[g], 0, 0, 0);
    }
}

// the cell update of this lane's unit for its four sequences, then h into the layer's tile of this step
template <int ACT>
__device__ __forceinline__ void cell_update(const f32x4 (&acc)[4], float (&c)[4], float (&h)[4], float* hw, int ldh) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float ig = rec_act<ACT>(acc[0][r]), fg = rec_act<ACT>(acc[1][r]), gg = tanh_f(acc[2][r]), og = rec_act<ACT>(acc[3][r]);
        c[r] = fmaf(fg, c[r], ig * gg);
        h[r] = og * tanh_f(c[r]);
        hw[r * ldh] = h[r];
    }
}

}  // namespace

}  // namespace fov
