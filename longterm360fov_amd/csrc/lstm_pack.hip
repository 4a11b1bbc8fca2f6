// The recurrent kernel R (H,4H) of an LSTM in the order the cluster kernel's waves hold it (lstm_cluster.hip: wR[j][s][g]),
// made once per weight set: the fused encode + decode launch then loads a wave's 64 KB slice as 16-byte loads, 1 KB
// contiguous per wave instruction, instead of 4-byte loads H floats apart.
//
// Element ((((c * NQ + jj) * 4 + s) * 64 + lane) * 4 + g) of the pack, NQ = H / 16, lane = 16 * g4 + n, is
//     R[16 * jj + 4 * g4 + s][g * H + 16 * c + n]
// c: the 16-unit column block (the wave with col0 = 16 * c), jj: the 16-row k-block, s: the k-step inside it (MFMA s of a block
// uses k = 16 * jj + 4 * g4 + s on the lanes with lane >> 4 == g4), g: the gate.  A permutation of R: every element once.
#include "fov_common.h"

namespace fov {

// one thread per (c, jj, s, lane): four gate values H floats apart in, one 16-byte store out
template <int H>
__global__ __launch_bounds__(256) void lstm_pack_r_kernel(const float* __restrict__ R, float* __restrict__ out) {
    constexpr int NQ = H / 16;
    const int t = blockIdx.x * 256 + threadIdx.x;   // < H * H (the grid is exact: H * H is a multiple of 256)
    const int lane = t & 63, s = (t >> 6) & 3, blk = t >> 8;
    const int jj = blk % NQ, c = blk / NQ;
    const int n = lane & 15, g4 = lane >> 4;
    const float* src = R + (size_t)(16 * jj + 4 * g4 + s) * (4 * H) + 16 * c + n;
    f32x4 v;
#pragma unroll
    for (int g = 0; g < 4; ++g) v[g] = src[g * H];
    *(f32x4*)(out + (size_t)t * 4) = v;
}

bool lstm_pack_shape_ok(int H) { return H == 64 || H == 128 || H == 256; }

int launch_lstm_pack_r(const float* R, int H, float* out, hipStream_t stream) {
    const dim3 grid(H * H / 256), block(256);
    switch (H) {
        case 64: hipLaunchKernelGGL(lstm_pack_r_kernel<64>, grid, block, 0, stream, R, out); break;
        case 128: hipLaunchKernelGGL(lstm_pack_r_kernel<128>, grid, block, 0, stream, R, out); break;
        default: hipLaunchKernelGGL(lstm_pack_r_kernel<256>, grid, block, 0, stream, R, out); break;
    }
    return launch_check("lstm_pack_r");
}

}  // namespace fov

using namespace fov;

extern "C" int fov_lstm_pack_r(const float* R, int H, float* out, fov_stream_t stream) {
    if (!R || !out) { set_error("fov_lstm_pack_r: invalid argument"); return FOV_ERR_INVALID; }
    if (!lstm_pack_shape_ok(H)) { set_error("fov_lstm_pack_r: H in {64, 128, 256} only (got %d)", H); return FOV_ERR_UNSUPPORTED; }
    if (((uintptr_t)out & 15) != 0) { set_error("fov_lstm_pack_r: out must be 16-byte aligned"); return FOV_ERR_INVALID; }
    return launch_lstm_pack_r(R, H, out, (hipStream_t)stream);
}
