// One-hot FoV heat maps of the ConvLSTM heat-map model, built on the device from the trajectories they encode:
//   mycode/utility.py:522-544 (_save_theta_phi_index)  frame centre xyz -> (theta, phi) bin indices, 10-degree bins
//   mycode/utility.py:557-571 (_create_one_hot)         indices -> (N, T, 30, 36, 18) zero/one maps
//   mycode/convlstm_seq2seq.py:356-374                  transposed to channels-last (N, T, 36, 18, 30) for the model
// A frame is 12 bytes of xyz; its map is 648 floats.  The kernel is a pure write stream: one workgroup per (sequence,
// second) slab computes the slab's 30 pixel indices once into LDS, then writes the whole slab (648 x C floats, every
// element, zeros included: the output needs no memset) as 16-byte stores, consecutive lanes on consecutive 16 bytes.
#include "fov_common.h"

namespace fov {

constexpr int OH_FRAMES = 30;            // frames per second: the map's channels
constexpr int OH_H = 36, OH_W = 18;      // 360 / 10 longitude bins x 180 / 10 latitude bins, indexed [theta, phi]
constexpr int OH_PIX = OH_H * OH_W;
constexpr int OH_NT = 256;
enum { OH_BAD_XYZ = 1, OH_BAD_INDEX = 2, OH_BAD_PIXEL = 4 };    // OH_BAD_PIXEL: heatmap_decode.hip's HD_BAD_PIXEL

struct OnehotParams {
    const float* xyz;       // (N, T, 30, 3): frame-contiguous inside a step, strided steps / sequences (floats)
    long xyz_seq, xyz_step;
    const int* ti_in;       // or (N, T, 30) bin indices, contiguous
    const int* pi_in;
    float* maps;            // slab (n, t) at maps + n * map_seq + t * map_step: (36, 18, C) contiguous; NULL = indices only
    long map_seq, map_step;
    int* ti_out;            // optional (N, T, 30) bin indices
    int* pi_out;
    int* status;            // sticky error word (OH_BAD_*)
    int T;
};

// np.mod for floats (numpy's npy_divmod): the result takes the sign of the divisor; fmod alone would leave negative
// atan2 values negative and put them in the wrong bin.
__device__ __forceinline__ double floor_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// dataIO.py:77-82 (xyz2thetaphi) then utility.py:536-542, in fp64 and in the reference's operation order.  Contraction is
// off: x*x + y*y fused into one fma, or theta/pi*180/bin reassociated, would move frames across bin edges.
__device__ __forceinline__ void xyz_bins(double x, double y, double z, int& ti, int& pi) {
#pragma clang fp contract(off)
    const double kPi = 3.141592653589793;   // np.pi
    const double theta = floor_mod(atan2(y, x), 2.0 * kPi) - kPi;
    const double phi = floor_mod(atan2(z, sqrt(x * x + y * y)) + kPi / 2.0, kPi);
    ti = (int)floor((theta + kPi) / kPi * 180.0 / 10.0);
    if (ti == OH_H) ti = OH_H - 1;
    pi = (int)floor(phi / kPi * 180.0 / 10.0);
    if (pi == OH_W) pi = OH_W - 1;
}

template <int C>
__global__ __launch_bounds__(OH_NT) void onehot_maps_kernel(OnehotParams p) {
    __shared__ int fpix[32];       // pixel (ti * 18 + pi) of the frame on channel c; -1 for channels 30, 31 and bad frames
    const long slab = blockIdx.x;
    const long n = slab / p.T, t = slab - n * p.T;
    const int tid = threadIdx.x;
    if (tid < 32) {
        int pix = -1;
        if (tid < OH_FRAMES) {
            int ti = -1, pi = -1;
            bool ok;
            if (p.xyz) {
                const float* q = p.xyz + n * p.xyz_seq + t * p.xyz_step + 3 * tid;
                const float x = q[0], y = q[1], z = q[2];
                ok = isfinite(x) && isfinite(y) && isfinite(z);     // the reference raises on int(nan)
                if (ok) xyz_bins(x, y, z, ti, pi);
                if (!ok) atomicOr(p.status, OH_BAD_XYZ);
            } else {
                ti = p.ti_in[slab * OH_FRAMES + tid];
                pi = p.pi_in[slab * OH_FRAMES + tid];
                ok = ti >= 0 && ti < OH_H && pi >= 0 && pi < OH_W;
                if (!ok) atomicOr(p.status, OH_BAD_INDEX);
            }
            if (p.ti_out) {
                p.ti_out[slab * OH_FRAMES + tid] = ok ? ti : -1;
                p.pi_out[slab * OH_FRAMES + tid] = ok ? pi : -1;
            }
            if (ok) pix = ti * OH_W + pi;
        }
        fpix[tid] = pix;
    }
    if (!p.maps) return;
    __syncthreads();
    float* out = p.maps + n * p.map_seq + t * p.map_step;
    constexpr int NV = OH_PIX * C / 4;     // 16-byte vectors per slab (C = 30: a vector may straddle two pixels)
    for (int v = tid; v < NV; v += OH_NT) {
        f32x4 val;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = 4 * v + k;
            const int pix = e / C, ch = e - pix * C;
            val[k] = fpix[ch] == pix ? 1.f : 0.f;
        }
        *reinterpret_cast<f32x4*>(out + 4 * v) = val;
    }
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_onehot_maps(const float* xyz, int64_t xyz_seq_stride, int64_t xyz_step_stride, const int* theta_index,
                    const int* phi_index, float* maps, int64_t maps_seq_stride, int64_t maps_step_stride, int channels,
                    int* theta_out, int* phi_out, int* status, int N, int T, fov_stream_t stream) {
    const bool from_xyz = xyz != nullptr, from_index = theta_index != nullptr || phi_index != nullptr;
    if (N < 0 || T < 0 || (long)N * T > 0x7fffffffL || from_xyz == from_index || (from_index && (!theta_index || !phi_index)) ||
        (from_xyz && (xyz_seq_stride < 0 || xyz_step_stride < 0)) || !status || (!theta_out != !phi_out) ||
        (!maps && !theta_out)) {
        set_error("fov_onehot_maps: invalid argument (xyz or both index arrays, a status word, maps and / or index outputs)");
        return FOV_ERR_INVALID;
    }
    if (maps && ((channels != 30 && channels != 32) || maps_seq_stride < 0 || maps_step_stride < 0 || (maps_seq_stride & 3) ||
                 (maps_step_stride & 3) || (((uintptr_t)maps) & 15))) {
        set_error("fov_onehot_maps: maps need 30 or 32 channels, a 16-byte aligned base and strides that are multiples of 4");
        return FOV_ERR_INVALID;
    }
    if ((long)N * T == 0) return FOV_OK;
    OnehotParams p;
    p.xyz = xyz; p.xyz_seq = (long)xyz_seq_stride; p.xyz_step = (long)xyz_step_stride;
    p.ti_in = theta_index; p.pi_in = phi_index;
    p.maps = maps; p.map_seq = (long)maps_seq_stride; p.map_step = (long)maps_step_stride;
    p.ti_out = theta_out; p.pi_out = phi_out; p.status = status; p.T = T;
    const dim3 grid((unsigned)((long)N * T)), block(OH_NT);
    if (channels == 32)
        hipLaunchKernelGGL(onehot_maps_kernel<32>, grid, block, 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(onehot_maps_kernel<30>, grid, block, 0, (hipStream_t)stream, p);
    return launch_check("onehot_maps");
}

int fov_onehot_status(int* status, fov_stream_t stream) {
    if (!status) { set_error("fov_onehot_status: invalid argument"); return FOV_ERR_INVALID; }
    int word = 0;
    hipError_t e = hipMemcpyAsync(&word, status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess && word) e = hipMemsetAsync(status, 0, sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) { set_error("fov_onehot_status: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    if (word & OH_BAD_PIXEL) {      // fov_heatmap_index_xyz shares the word's protocol
        set_error("fov_heatmap_index_xyz: a pixel number lies outside [0, 648)");
        return FOV_ERR_INVALID;
    }
    if (word) {
        set_error("fov_onehot_maps: %s", (word & OH_BAD_XYZ) ? "a frame centre is NaN or infinite"
                                                               : "a bin index lies outside [0, 36) x [0, 18)");
        return FOV_ERR_INVALID;
    }
    return FOV_OK;
}

}  // extern "C"
