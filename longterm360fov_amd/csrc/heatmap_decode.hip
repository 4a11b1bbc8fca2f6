// The ConvLSTM heat-map model's predictions decoded on the device, the step the reference's test loop runs right after
// model.predict:
//   mycode/convlstm_seq2seq.py:537-542, mycode/convlstm_heatmap.py:556-558
//       max_ind = np.argmax(decoded_sentence.reshape(batch_size, cfg.predict_step, -1, fps), axis=-2)
// and the way back from a pixel number to a frame centre, the inverse of the binning of onehot_maps.hip
// (mycode/utility.py:522-544).
// A map is n_pix pixels of C channels, 78 KB at 648 x 30, and is read exactly once: one workgroup per map, HD_NT threads
// laid out as G = HD_NT / L pixel groups of L lanes, a lane on V fixed channels (V = 2: L = C / 2 lanes x 8 bytes, 15 lanes
// at C 30; V = 1, the scalar form: L = C lanes x 4 bytes).  Consecutive lanes of a group read consecutive V * 4 bytes of one
// pixel, consecutive groups consecutive pixels; a thread walks pixels g, g + G, g + 2G, ... in increasing order and takes a
// later pixel only on a strict `>` (or on the first NaN), four loads in flight.  The G partial results of a channel then meet
// in LDS in a binary tree whose comparison is np.argmax's total order - NaN above everything, then the larger value, then the
// LOWER pixel number - so the result does not depend on the tree's shape.  No atomics, no scratch, bit-repeatable.
#include "fov_common.h"

namespace fov {

constexpr int HD_NT = 512;               // threads per workgroup (8 waves): a 648 x 30 map is 19 or 20 loads a thread
constexpr int HD_MAX_C = 64;
constexpr int HD_MAX_PIX = 1 << 20;
constexpr int HD_H = 36, HD_W = 18;      // the one-hot geometry of onehot_maps.hip: pixel number = ti * 18 + pi
enum { HD_BAD_PIXEL = 4 };               // status bit next to onehot_maps.hip's OH_BAD_XYZ = 1, OH_BAD_INDEX = 2

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct ArgmaxParams {
    const float* maps;
    long map_stride, pixel_stride;       // floats
    int* index;
    float* value;                        // may be NULL
    long out_stride;
    long n_maps;
    int n_pix, C;
};

// np.argmax's walk (numpy's FLOAT_argmax: `if (!(*ip <= mp))` take, stop at a NaN): does v, at a LATER pixel, replace best?
__device__ __forceinline__ bool later_wins(float v, float best) { return v > best || (v != v && best == best); }

// The same order between two partial results at any two pixels; pixel -1 = a thread that owned no pixel.
__device__ __forceinline__ bool entry_wins(float v, int p, float bv, int bp) {
    if (p < 0) return false;
    if (bp < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || p < bp);
    return v > bv || (v == bv && p < bp);
}

template <int V>
__device__ __forceinline__ void load_channels(const float* q, float (&v)[V]) {
    if constexpr (V == 2) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(q);
        v[0] = t[0]; v[1] = t[1];
    } else {
        v[0] = q[0];
    }
}

template <int V>
__global__ __launch_bounds__(HD_NT) void heatmap_argmax_kernel(ArgmaxParams p) {
    __shared__ float sval[HD_NT * V];    // [pixel group][channel] partial maxima ...
    __shared__ int spix[HD_NT * V];      // ... and their pixel numbers
    const int tid = threadIdx.x;
    const int L = p.C / V, G = HD_NT / L;            // lanes per pixel, pixels per pass (8 <= G <= 512)
    const int g = tid / L, cp = tid - g * L;
    const int n_pix = p.n_pix;
    const long ps = p.pixel_stride;
    int tree = 1;
    while (tree < G) tree <<= 1;
    for (long m = blockIdx.x; m < p.n_maps; m += gridDim.x) {
        const float* q = p.maps + m * p.map_stride + V * cp;
        float bv[V];
        int bp[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { bv[k] = 0.f; bp[k] = -1; }
        if (g < G && g < n_pix) {                    // the HD_NT - G * L threads past the last whole group own nothing
            load_channels<V>(q + (long)g * ps, bv);
#pragma unroll
            for (int k = 0; k < V; ++k) bp[k] = g;
            int pix = g + G;
            for (; pix + 3 * G < n_pix; pix += 4 * G) {
                float v[4][V];
#pragma unroll
                for (int j = 0; j < 4; ++j) load_channels<V>(q + (long)(pix + j * G) * ps, v[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const bool take = later_wins(v[j][k], bv[k]);
                        bv[k] = take ? v[j][k] : bv[k];
                        bp[k] = take ? pix + j * G : bp[k];
                    }
            }
            for (; pix < n_pix; pix += G) {
                float v[V];
                load_channels<V>(q + (long)pix * ps, v);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const bool take = later_wins(v[k], bv[k]);
                    bv[k] = take ? v[k] : bv[k];
                    bp[k] = take ? pix : bp[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) { sval[tid * V + k] = bv[k]; spix[tid * V + k] = bp[k]; }
        // group g takes group g + s: it reads entries [s, 2s) and writes entries [0, s), so one barrier a level is enough
        for (int s = tree >> 1; s >= 1; s >>= 1) {
            __syncthreads();
            if (g < s && g + s < G) {
                const int o = (tid + s * L) * V;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float ov = sval[o + k];
                    const int op = spix[o + k];
                    const bool take = entry_wins(ov, op, bv[k], bp[k]);
                    bv[k] = take ? ov : bv[k];
                    bp[k] = take ? op : bp[k];
                    sval[tid * V + k] = bv[k];
                    spix[tid * V + k] = bp[k];
                }
            }
        }
        if (g == 0) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                p.index[m * p.out_stride + V * cp + k] = bp[k];
                if (p.value) p.value[m * p.out_stride + V * cp + k] = bv[k];
            }
        }
        __syncthreads();                             // the next map's partial results overwrite the entries read above
    }
}

// Bin centre of pixel ti * 18 + pi: az = (ti + 0.5) * 10 deg, el = (pi + 0.5) * 10 deg - 90 deg, evaluated in fp64 (sinpi /
// cospi of the angle in half turns: exact argument reduction, no large-argument path) and rounded to fp32.
__global__ __launch_bounds__(256) void heatmap_index_xyz_kernel(const int* index, float* xyz, long n, int* status) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const int pix = index[i];
    float x = 0.f, y = 0.f, z = 0.f;
    if (pix >= 0 && pix < HD_H * HD_W) {
        const int ti = pix / HD_W, pi = pix - ti * HD_W;
        const double az = (ti + 0.5) / 18.0, el = (pi + 0.5) / 18.0 - 0.5;      // in units of pi
        const double ce = cospi(el);
        x = (float)(ce * cospi(az));
        y = (float)(ce * sinpi(az));
        z = (float)sinpi(el);
    } else {
        atomicOr(status, HD_BAD_PIXEL);
    }
    xyz[3 * i] = x; xyz[3 * i + 1] = y; xyz[3 * i + 2] = z;
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_heatmap_argmax(const float* maps, int64_t map_stride, int64_t pixel_stride, int* index, float* value,
                       int64_t out_stride, int64_t n_maps, int n_pix, int C, fov_stream_t stream) {
    if (C < 1 || C > HD_MAX_C || n_pix < 1 || n_pix > HD_MAX_PIX || n_maps < 0 || map_stride < 0 || pixel_stride < C ||
        pixel_stride > 0x7fffffffL || out_stride < C) {
        set_error("fov_heatmap_argmax: invalid argument (1 <= C <= 64, 1 <= n_pix <= 2^20, n_maps >= 0, pixel_stride >= C, "
                  "out_stride >= C, map_stride >= 0)");
        return FOV_ERR_INVALID;
    }
    if (n_maps == 0) return FOV_OK;
    if (!maps || !index) { set_error("fov_heatmap_argmax: maps and index must not be NULL"); return FOV_ERR_INVALID; }
    ArgmaxParams p;
    p.maps = maps; p.map_stride = (long)map_stride; p.pixel_stride = (long)pixel_stride;
    p.index = index; p.value = value; p.out_stride = (long)out_stride; p.n_maps = (long)n_maps; p.n_pix = n_pix; p.C = C;
    const dim3 grid((unsigned)(n_maps < 65536 ? n_maps : 65536)), block(HD_NT);
    // 8-byte loads need every pixel of every map on an 8-byte boundary and whole channel pairs; anything else: scalar form
    const bool vec = !(C & 1) && !(pixel_stride & 1) && !(map_stride & 1) && !(((uintptr_t)maps) & 7);
    if (vec)
        hipLaunchKernelGGL(heatmap_argmax_kernel<2>, grid, block, 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(heatmap_argmax_kernel<1>, grid, block, 0, (hipStream_t)stream, p);
    return launch_check("heatmap_argmax");
}

int fov_heatmap_index_xyz(const int* index, float* xyz, int64_t n, int* status, fov_stream_t stream) {
    if (n < 0 || n > 0x7fffffffL || !status || (n > 0 && (!index || !xyz))) {
        set_error("fov_heatmap_index_xyz: invalid argument (0 <= n < 2^31, index, xyz and a status word)");
        return FOV_ERR_INVALID;
    }
    if (n == 0) return FOV_OK;
    hipLaunchKernelGGL(heatmap_index_xyz_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, index,
                       xyz, (long)n, status);
    return launch_check("heatmap_index_xyz");
}

}  // extern "C"
