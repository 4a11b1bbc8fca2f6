// The small non-recurrent kernels of the path with their entry points: Dense(+tanh) in three forms, the mixing head, the
// mu/sigma^2 feature op, the FoV hit rate and the device-side windowing.
#include <math.h>

#include "fov_common.h"
#include "bf16_common.h"

namespace fov {

// ---------------------------------------------------------------------------------------
// Dense: y = act(x W + b).  One wave per output row; lanes stride over In, shuffle-reduce.
// Memory-bound streaming op (x is read once; W stays in L2): used for the teacher-forced
// graph's Dense over (B*T_out, H) -> F_dec and for tests.
// ---------------------------------------------------------------------------------------
constexpr int DENSE_MAX_OUT = 16;

__global__ __launch_bounds__(256) void dense_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                    const float* __restrict__ b, const float* __restrict__ add,
                                                    long add_stride, float* __restrict__ y,
                                                    int N, int In, int Out, int activation) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* xr = x + (size_t)row * In;
    for (int o0 = 0; o0 < Out; o0 += DENSE_MAX_OUT) {
        const int no = (Out - o0 < DENSE_MAX_OUT) ? Out - o0 : DENSE_MAX_OUT;
        float acc[DENSE_MAX_OUT];
#pragma unroll
        for (int o = 0; o < DENSE_MAX_OUT; ++o) acc[o] = 0.f;
        for (int k = lane; k < In; k += 64) {
            const float xv = xr[k];
            const float* wr = W + (size_t)k * Out + o0;
#pragma unroll
            for (int o = 0; o < DENSE_MAX_OUT; ++o)
                if (o < no) acc[o] = fmaf(xv, wr[o], acc[o]);
        }
#pragma unroll
        for (int o = 0; o < DENSE_MAX_OUT; ++o)
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc[o] += __shfl_xor(acc[o], m);
        float mine = 0.f;
#pragma unroll
        for (int o = 0; o < DENSE_MAX_OUT; ++o) mine = (lane == o) ? acc[o] : mine;
        if (lane < no) {
            float v = mine + (b ? b[o0 + lane] : 0.f);
            if (add) v += add[(size_t)row * add_stride + o0 + lane];
            if (activation == 1) v = tanh_f(v);
            y[(size_t)row * Out + o0 + lane] = v;
        }
    }
}

// Narrow heads (Out <= 8, the Dense(6) of every model here): 16 lanes per row and four rows per wave, x read
// as 16-byte pieces, W transposed in LDS (the four row groups of a wave read the same addresses - broadcast),
// four butterfly steps instead of six and only over Out values.  ~4x fewer instructions per row than the
// generic kernel above; HBM-bound on x.
template <int VEC>   // VEC = 4: In % 4 == 0 and x 16-byte aligned; VEC = 1: any In (the others' projection: In = 198)
__global__ __launch_bounds__(256) void dense_small_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                          const float* __restrict__ b, const float* __restrict__ add,
                                                          long add_stride, float* __restrict__ y, int N, int In, int Out,
                                                          int activation) {
    extern __shared__ __attribute__((aligned(16))) float Wt[];   // [8][In]
    for (int e = threadIdx.x; e < 8 * In; e += 256) {
        const int o = e / In, k = e - o * In;
        Wt[e] = (o < Out) ? W[(size_t)k * Out + o] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    for (long row0 = ((long)blockIdx.x * 4 + wave) * 4; row0 < N; row0 += (long)gridDim.x * 16) {
        const long row = row0 + g;
        const bool ok = row < N;
        const float* xr = x + (size_t)(ok ? row : 0) * In;
        float acc[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[o] = 0.f;
        if constexpr (VEC == 4) {
            for (int k = 4 * l16; k < In; k += 64) {
                const f32x4 xv = *(const f32x4*)(xr + k);
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const f32x4 wv = *(const f32x4*)&Wt[o * In + k];
                    acc[o] = fmaf(xv[0], wv[0], fmaf(xv[1], wv[1], fmaf(xv[2], wv[2], fmaf(xv[3], wv[3], acc[o]))));
                }
            }
        } else {
            for (int k0 = 0; k0 < In; k0 += 64) {   // four elements per lane in flight
                float xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 16 * u + l16;
                    xv[u] = xr[k < In ? k : In - 1];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 16 * u + l16;
                    const float xm = k < In ? xv[u] : 0.f;
                    const int kc = k < In ? k : In - 1;
#pragma unroll
                    for (int o = 0; o < 8; ++o) acc[o] = fmaf(xm, Wt[o * In + kc], acc[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 8; ++o)
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) acc[o] += __shfl_xor(acc[o], m);
        float mine = 0.f;
#pragma unroll
        for (int o = 0; o < 8; ++o) mine = (l16 == o) ? acc[o] : mine;
        if (ok && l16 < Out) {
            float v = mine + (b ? b[l16] : 0.f);
            if (add) v += add[(size_t)row * add_stride + l16];
            if (activation == 1) v = tanh_f(v);
            y[(size_t)row * Out + l16] = v;
        }
    }
}

// Few rows, a wide input and more than eight outputs (the 400 -> 32 heads of lstm.py:321-337 on a batch of 32 final states):
// the wave-per-row kernel above walks In / 64 dependent rounds of Out strided loads - 34 us for a 32 x 512 x 32 product.
// Here a workgroup takes four rows; thread (o, kq) contracts an eighth of In for output o of all four rows: its W loads are
// independent and coalesced over o (issued back to back), x comes from LDS as a broadcast, the eight partial sums meet in LDS.
constexpr int DW_ROWS = 4, DW_KQ = 8, DW_OT = 32;
__global__ __launch_bounds__(256) void dense_fewrows_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                            const float* __restrict__ b, const float* __restrict__ add,
                                                            long add_stride, float* __restrict__ y, int N, int In, int Out,
                                                            int activation) {
    extern __shared__ __attribute__((aligned(16))) float dw_lds[];   // [DW_ROWS][In] rows of x, then [DW_KQ][DW_ROWS][DW_OT] partials
    float* xs = dw_lds;
    float* red = dw_lds + DW_ROWS * In;
    const int row0 = blockIdx.x * DW_ROWS;
    for (int e = threadIdx.x; e < DW_ROWS * In; e += 256) {
        const int r = e / In, k = e - r * In;
        xs[e] = (row0 + r < N) ? x[(size_t)(row0 + r) * In + k] : 0.f;
    }
    __syncthreads();
    const int ol = threadIdx.x & (DW_OT - 1), kq = threadIdx.x / DW_OT;
    const int kc = (In + DW_KQ - 1) / DW_KQ;
    const int k0 = kq * kc, k1 = (k0 + kc < In) ? k0 + kc : In;
    for (int o0 = 0; o0 < Out; o0 += DW_OT) {
        const int o = o0 + ol;
        float acc[DW_ROWS] = {0.f, 0.f, 0.f, 0.f};
        if (o < Out) {
            int k = k0;
            for (; k + 8 <= k1; k += 8) {
                float w[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) w[u] = W[(size_t)(k + u) * Out + o];
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int r = 0; r < DW_ROWS; ++r) acc[r] = fmaf(xs[r * In + k + u], w[u], acc[r]);
            }
            for (; k < k1; ++k) {
                const float w = W[(size_t)k * Out + o];
#pragma unroll
                for (int r = 0; r < DW_ROWS; ++r) acc[r] = fmaf(xs[r * In + k], w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < DW_ROWS; ++r) red[(kq * DW_ROWS + r) * DW_OT + ol] = acc[r];
        __syncthreads();
        if (threadIdx.x < DW_ROWS * DW_OT) {
            const int r = threadIdx.x / DW_OT, row = row0 + r;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < DW_KQ; ++q) v += red[(q * DW_ROWS + r) * DW_OT + ol];   // fixed order
            if (row < N && o < Out) {
                v += b ? b[o] : 0.f;
                if (add) v += add[(size_t)row * add_stride + o];
                if (activation == 1) v = tanh_f(v);
                y[(size_t)row * Out + o] = v;
            }
        }
        __syncthreads();
    }
}

static int launch_dense(const float* x, const float* W, const float* b, const float* add, long add_stride, float* y, int N,
                        int In, int Out, int activation, hipStream_t stream) {
    if (Out > 8 && N <= 256 && In >= 128 && In <= 2048) {
        const size_t lds = sizeof(float) * ((size_t)DW_ROWS * In + DW_KQ * DW_ROWS * DW_OT);
        hipLaunchKernelGGL(dense_fewrows_kernel, dim3((unsigned)((N + DW_ROWS - 1) / DW_ROWS)), dim3(256), lds, stream, x, W, b, add,
                           add_stride, y, N, In, Out, activation);
        return launch_check("dense (few rows)");
    }
    // (each kernel form under its own name in the FOV_DBG_TRACE line: a test asserts the one it reached)
    if (Out <= 8 && In <= 2048 && N >= 64) {
        long blocks = ((long)N + 15) / 16;
        if (blocks > 2048) blocks = 2048;
        const bool xvec = (In & 3) == 0 && (((uintptr_t)x) & 15) == 0;
        if (xvec)
            hipLaunchKernelGGL(dense_small_kernel<4>, dim3((unsigned)blocks), dim3(256), sizeof(float) * 8 * In, stream, x, W, b, add,
                               add_stride, y, N, In, Out, activation);
        else
            hipLaunchKernelGGL(dense_small_kernel<1>, dim3((unsigned)blocks), dim3(256), sizeof(float) * 8 * In, stream, x, W, b, add,
                               add_stride, y, N, In, Out, activation);
        return launch_check(xvec ? "dense (16 rows, vector x)" : "dense (16 rows, scalar x)");
    }
    hipLaunchKernelGGL(dense_kernel, dim3((unsigned)(((long)N + 3) / 4)), dim3(256), 0, stream, x, W, b, add, add_stride, y, N, In, Out, activation);
    return launch_check("dense (wave per row)");
}

// ---------------------------------------------------------------------------------------
// Mixing head of the others model, one decoder step (given_others...py:127-130,168,257-265):
//   p = tanh(h W_d + b_d)                     Dense(O,'tanh') on the layer-2 output
//   m = tanh(p W_p + add)                     mixing Dense: W_p = mix_W[-O:], add = others_t . mix_W[:-O] + mix_b
// Forward: 16 lanes per row as dense_small_kernel, then the O values of p are exchanged inside the 16-lane group.
// Backward (one thread per (row, hidden unit); the O-wide row quantities are recomputed by every thread of the
// row - 2*O*O FMAs): dpre_m = dm_loss + dm_feedback * (1 - m^2), dpre_p = (dpre_m W_p^T) * (1 - p^2),
// dh = dpre_p W_d^T.  One launch each instead of two / five: the step-wise decoder is launch-bound.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mix_head_fwd_kernel(const float* __restrict__ h, const float* __restrict__ Wd,
                                                           const float* __restrict__ bd, const float* __restrict__ Wp,
                                                           const float* __restrict__ add, long add_stride, float* __restrict__ p_out,
                                                           float* __restrict__ m_out, int N, int H, int O) {
    extern __shared__ __attribute__((aligned(16))) float Wt[];   // [8][H] transposed W_d, then W_p (O x O)
    float* sWp = Wt + 8 * H;
    for (int e = threadIdx.x; e < 8 * H; e += 256) {
        const int o = e / H, k = e - o * H;
        Wt[e] = (o < O) ? Wd[(size_t)k * O + o] : 0.f;
    }
    for (int e = threadIdx.x; e < 64; e += 256) sWp[e] = (e < O * O) ? Wp[e] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    for (long row0 = ((long)blockIdx.x * 4 + wave) * 4; row0 < N; row0 += (long)gridDim.x * 16) {
        const long row = row0 + g;
        const bool ok = row < N;
        const float* xr = h + (size_t)(ok ? row : 0) * H;
        float acc[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[o] = 0.f;
        for (int k = 4 * l16; k < H; k += 64) {
            const f32x4 xv = *(const f32x4*)(xr + k);
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const f32x4 wv = *(const f32x4*)&Wt[o * H + k];
                acc[o] = fmaf(xv[0], wv[0], fmaf(xv[1], wv[1], fmaf(xv[2], wv[2], fmaf(xv[3], wv[3], acc[o]))));
            }
        }
#pragma unroll
        for (int o = 0; o < 8; ++o)
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) acc[o] += __shfl_xor(acc[o], m);
        // every lane of the group now holds all eight sums: p[o] = tanh(acc[o] + bd[o])
        float pv[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) pv[o] = (o < O) ? tanh_f(acc[o] + bd[o]) : 0.f;
        if (ok && l16 < O) {
            float pm = 0.f, z = add[(size_t)row * add_stride + l16];
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                pm = (l16 == o) ? pv[o] : pm;
                z = fmaf(pv[o], sWp[o * O + l16], z);   // rows o >= O of sWp are never read past O*O: pv is 0 there
            }
            p_out[(size_t)row * O + l16] = pm;
            m_out[(size_t)row * O + l16] = tanh_f(z);
        }
    }
}

__global__ __launch_bounds__(256) void mix_head_bwd_kernel(const float* __restrict__ dm_loss, const float* __restrict__ dm_fb,
                                                           const float* __restrict__ m, const float* __restrict__ p,
                                                           const float* __restrict__ Wp, const float* __restrict__ Wd,
                                                           float* __restrict__ dpre_m, float* __restrict__ dpre_p,
                                                           float* __restrict__ dh, int N, int H, int O) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * H) return;
    const long row = idx / H;
    const int j = (int)(idx - row * H);
    float dm[8], dp[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        dm[o] = 0.f;
        if (o < O) {
            const float mv = m[row * O + o];
            dm[o] = dm_loss[row * O + o] + (dm_fb ? dm_fb[row * O + o] * (1.f - mv * mv) : 0.f);
        }
    }
    float out = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        dp[i] = 0.f;
        if (i < O) {
            float s = 0.f;
#pragma unroll
            for (int o = 0; o < 8; ++o)
                if (o < O) s = fmaf(dm[o], Wp[i * O + o], s);
            const float pv = p[row * O + i];
            dp[i] = s * (1.f - pv * pv);
            out = fmaf(dp[i], Wd[(size_t)j * O + i], out);
        }
    }
    dh[idx] = out;
    if (j < O) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            a = (j == o) ? dm[o] : a;
            b = (j == o) ? dp[o] : b;
        }
        dpre_m[row * O + j] = a;
        dpre_p[row * O + j] = b;
    }
}

// ---------------------------------------------------------------------------------------
// mu / sigma^2 feature op (utility.py:483-517): one thread per (row, axis); two-pass
// population variance like numpy.var (mean first, then mean of squared deviations).
// HBM-bound: 12*fps bytes in, 24 bytes out per row.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void meanvar_kernel(const float* __restrict__ y, float* __restrict__ out,
                                                      long rows, int fps) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 3) return;
    const long row = i / 3;
    const int ax = (int)(i - row * 3);
    const float* p = y + (size_t)row * 3 * fps + ax;
    float s = 0.f;
    for (int f = 0; f < fps; ++f) s += p[3 * f];
    const float mean = s / (float)fps;
    float v = 0.f;
    for (int f = 0; f < fps; ++f) {
        const float d = p[3 * f] - mean;
        v = fmaf(d, d, v);
    }
    out[row * 6 + ax] = mean;
    out[row * 6 + 3 + ax] = v / (float)fps;
}

// ---------------------------------------------------------------------------------------
// FoV hit rate per predicted second (the consumer of the path's output):
// xyz -> (theta, phi) as dataIO.py:77-82, +-2pi seam fix as baseline_knn_mean.py:78-85, overlap of the two
// span x span boxes over the ground-truth box area as :62-82.  One thread per (sequence, second); HBM-bound.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float fmod_pos(float a, float m) {
    float r = fmodf(a, m);
    return r < 0.f ? r + m : r;
}

__global__ __launch_bounds__(256) void hit_rate_kernel(const float* __restrict__ pred, long pred_stride,
                                                       const float* __restrict__ gt, long gt_stride,
                                                       float* __restrict__ out, long rows, float span, float gt_span) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const float kPi = 3.14159265358979323846f;
    const float* p = pred + i * pred_stride;
    const float* g = gt + i * gt_stride;
    float pt = fmod_pos(atan2f(p[1], p[0]), 2.f * kPi) - kPi;
    const float pp = fmod_pos(atan2f(p[2], sqrtf(p[0] * p[0] + p[1] * p[1])) + 0.5f * kPi, kPi);
    float gth = fmod_pos(atan2f(g[1], g[0]), 2.f * kPi) - kPi;
    const float gp = fmod_pos(atan2f(g[2], sqrtf(g[0] * g[0] + g[1] * g[1])) + 0.5f * kPi, kPi);
    if (gth > 2.f / 3.f * kPi && pt < -2.f / 3.f * kPi) pt += 2.f * kPi;
    else if (gth < -2.f / 3.f * kPi && pt > 2.f / 3.f * kPi) gth += 2.f * kPi;
    const float iw = fminf(pt + 0.5f * span, gth + 0.5f * gt_span) - fmaxf(pt - 0.5f * span, gth - 0.5f * gt_span);
    const float ih = fminf(pp + 0.5f * span, gp + 0.5f * gt_span) - fmaxf(pp - 0.5f * span, gp - 0.5f * gt_span);
    out[i] = (iw > 0.f && ih > 0.f) ? iw * ih / (gt_span * gt_span) : 0.f;
}

// ---------------------------------------------------------------------------------------
// Device-side windowing: reshape2second_stacks (mycode/utility.py:264-305) as one gather.
// x:(U,S,feat) seconds of one video -> enc / future / future_input windows of T seconds every `stride`
// seconds; collapse_user: window-major (W*U, T, feat), else user-major (U, W, T, feat).  HBM-bound copy.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_stacks_kernel(const float* __restrict__ x, float* __restrict__ enc,
                                                            float* __restrict__ fut, float* __restrict__ fut_in, int U,
                                                            int S, int feat, int T, int stride, int shift, int W,
                                                            int collapse) {
    const long total = (long)W * U * T * feat;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % feat);
    long r = i / feat;
    const int t = (int)(r % T);
    r /= T;
    int w, u;
    if (collapse) { u = (int)(r % U); w = (int)(r / U); } else { w = (int)(r % W); u = (int)(r / W); }
    const float* xu = x + (size_t)u * S * feat;
    const int s_enc = stride * w + t, s_fut = stride * (w + shift) + t;
    enc[i] = xu[(size_t)s_enc * feat + f];
    fut[i] = xu[(size_t)s_fut * feat + f];
    // decoder input = future shifted right by one second, seeded with the encoder's last second
    fut_in[i] = (t == 0) ? xu[(size_t)(stride * w + T - 1) * feat + f] : xu[(size_t)(s_fut - 1) * feat + f];
}

}  // namespace fov

using namespace fov;

// the wave-per-row kernel strides its int loops over In by 64 and over Out by its tile: widths far below INT_MAX only
static constexpr int kMaxDenseWidth = 1 << 24;

extern "C" {

int fov_dense_fwd(const float* x, const float* W, const float* b, float* y, int N, int In, int Out,
                  int activation, fov_stream_t stream) {
    if (N < 0 || In <= 0 || Out <= 0 || In > kMaxDenseWidth || Out > kMaxDenseWidth || !W || (N > 0 && (!x || !y)) ||
        (activation != 0 && activation != 1)) {
        set_error("fov_dense_fwd: invalid argument (In, Out <= 2^24)");
        return FOV_ERR_INVALID;
    }
    if (N == 0) return FOV_OK;
    return launch_dense(x, W, b, nullptr, 0L, y, N, In, Out, activation, (hipStream_t)stream);
}

int fov_dense_add_fwd(const float* x, const float* W, const float* b, const float* add, int64_t add_row_stride,
                      float* y, int N, int In, int Out, int activation, fov_stream_t stream) {
    if (N < 0 || In <= 0 || Out <= 0 || In > kMaxDenseWidth || Out > kMaxDenseWidth || !W || (N > 0 && (!x || !y || !add)) || add_row_stride < 0 ||
        (activation != 0 && activation != 1)) {
        set_error("fov_dense_add_fwd: invalid argument (In, Out <= 2^24, add_row_stride >= 0)");
        return FOV_ERR_INVALID;
    }
    if (N == 0) return FOV_OK;
    return launch_dense(x, W, b, add, (long)add_row_stride, y, N, In, Out, activation, (hipStream_t)stream);
}

int fov_mix_head_fwd(const float* h, const float* dense_W, const float* dense_b, const float* mix_Wp, const float* add,
                     int64_t add_row_stride, float* p, float* m, int N, int H, int O, fov_stream_t stream) {
    if (N < 0 || H <= 0 || O <= 0 || O > 8 || (H & 3) || H > 2048 || !dense_W || !dense_b || !mix_Wp ||
        (N > 0 && (!h || !add || !p || !m)) || add_row_stride < 0 || (((uintptr_t)h) & 15)) {
        set_error("fov_mix_head_fwd: invalid argument (O <= 8, H a multiple of 4 and <= 2048, h 16-byte aligned, add_row_stride >= 0)");
        return FOV_ERR_INVALID;
    }
    if (N == 0) return FOV_OK;
    long blocks = ((long)N + 15) / 16;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(mix_head_fwd_kernel, dim3((unsigned)blocks), dim3(256), sizeof(float) * (8 * H + 64), (hipStream_t)stream, h,
                       dense_W, dense_b, mix_Wp, add, (long)add_row_stride, p, m, N, H, O);
    return launch_check("mix_head_fwd");
}

int fov_mix_head_bwd(const float* dm_loss, const float* dm_feedback, const float* m, const float* p, const float* mix_Wp,
                     const float* dense_W, float* dpre_m, float* dpre_p, float* dh, int N, int H, int O, fov_stream_t stream) {
    if (N < 0 || H <= 0 || O <= 0 || O > 8 || !mix_Wp || !dense_W || (N > 0 && (!dm_loss || !m || !p || !dpre_m || !dpre_p || !dh))) {
        set_error("fov_mix_head_bwd: invalid argument (O <= 8)");
        return FOV_ERR_INVALID;
    }
    if (N == 0) return FOV_OK;
    const long n = (long)N * H;
    hipLaunchKernelGGL(mix_head_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dm_loss, dm_feedback,
                       m, p, mix_Wp, dense_W, dpre_m, dpre_p, dh, N, H, O);
    return launch_check("mix_head_bwd");
}

int fov_dense_fwd_bf16(const float* x, const float* W, const float* b, float* y, int N, int In, int Out, int activation,
                       fov_stream_t stream) {
    if (N < 0 || In <= 0 || Out <= 0 || !W || (N > 0 && (!x || !y)) || (activation != 0 && activation != 1)) {
        set_error("fov_dense_fwd_bf16: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (!dense_bf16_shape_ok(In, Out)) {
        set_error("fov_dense_fwd_bf16: In <= 256 and Out <= 16 only (got In=%d Out=%d)", In, Out);
        return FOV_ERR_UNSUPPORTED;
    }
    return launch_dense_bf16(x, W, b, y, N, In, Out, activation, (hipStream_t)stream);
}

int fov_meanvar_xyz(const float* y, float* out, int64_t rows, int fps, fov_stream_t stream) {
    if (rows < 0 || fps <= 0 || fps > kMaxFps || (rows > 0 && (!y || !out))) {
        set_error("fov_meanvar_xyz: invalid argument (1 <= fps <= 2^20)");
        return FOV_ERR_INVALID;
    }
    if (rows == 0) return FOV_OK;
    const long n = rows * 3;
    hipLaunchKernelGGL(meanvar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, out,
                       (long)rows, fps);
    return launch_check("meanvar");
}

int fov_fov_hit_rate(const float* pred_xyz, int64_t pred_row_stride, const float* gt_xyz, int64_t gt_row_stride,
                     float* out, int64_t rows, float span_deg, float gt_span_deg, fov_stream_t stream) {
    if (rows < 0 || pred_row_stride < 3 || gt_row_stride < 3 || span_deg <= 0.f || gt_span_deg <= 0.f ||
        (rows > 0 && (!pred_xyz || !gt_xyz || !out))) {
        set_error("fov_fov_hit_rate: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (rows == 0) return FOV_OK;
    const float d2r = 3.14159265358979323846f / 180.f;
    hipLaunchKernelGGL(hit_rate_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred_xyz,
                       (long)pred_row_stride, gt_xyz, (long)gt_row_stride, out, (long)rows, span_deg * d2r, gt_span_deg * d2r);
    return launch_check("hit_rate");
}

int64_t fov_window_count(int S, int T, int stride) {
    if (S < 2 * T || T <= 0 || stride <= 0 || stride > T) return 0;
    const int shift = T / stride;
    const int nrows = (S - T) / stride + 1;
    return nrows - shift > 0 ? nrows - shift : 0;
}

int fov_window_stacks(const float* x, float* enc, float* fut, float* fut_in, int U, int S, int feat, int T, int stride,
                      int collapse_user, fov_stream_t stream) {
    if (U < 0 || S < 0 || feat <= 0 || T <= 0 || stride <= 0 || stride > T || (U > 0 && S >= 2 * T && (!x || !enc || !fut || !fut_in))) {
        set_error("fov_window_stacks: invalid argument");
        return FOV_ERR_INVALID;
    }
    const int W = (int)fov_window_count(S, T, stride);
    if (U == 0 || W == 0) return FOV_OK;
    const long total = (long)W * U * T * feat;
    hipLaunchKernelGGL(window_stacks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, enc,
                       fut, fut_in, U, S, feat, T, stride, T / stride, W, collapse_user ? 1 : 0);
    return launch_check("window_stacks");
}

}  // extern "C"
