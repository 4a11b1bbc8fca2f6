// The element-wise end of the training step (all HBM- or launch-bound): the loss kernels with their per-stream
// ticket table (MSE of a Dense head, the Dense + MSE head in one launch, Gaussian NLL, categorical cross-entropy, the
// unit-norm regulariser, the sampled re-feed), the pointwise kernels (scale, act_fwd, act_bwd) and the flat-buffer
// optimizers (Keras Adam / RMSprop, tf.train.RMSPropOptimizer) with their fail-stop guard words.
#include <mutex>
#include <unordered_map>

#include "fov_common.h"

namespace fov {

// Dense(tanh|linear) + Keras mean_squared_error: dpre = 2 (y - target) / n * act'(y); per-block
// partial sums of (y - target)^2 into loss_part[blockIdx.x].
// Tickets of the loss kernels' "last block adds the partials" step (round 4: the separate one-block sum launch is gone, 5 us of
// every training step's critical path).  Zero at module load, left at zero again by the block that takes the last ticket; every
// stream of a device has its own slot (loss_ticket_of), so launches in flight never share one.
constexpr int kLossTickets = 1024;
__device__ unsigned g_loss_tickets[kLossTickets];

__global__ __launch_bounds__(256) void mse_dense_grad_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                             float* __restrict__ dpre, float* __restrict__ loss_part,
                                                             long n, float scale, int activation, int tmB, int tmT, int O,
                                                             unsigned* __restrict__ ticket, float* __restrict__ loss_out, float loss_scale,
                                                             float* __restrict__ col_part = nullptr, float* __restrict__ db_out = nullptr,
                                                             int dbO = 0) {
    // tmT > 0: y / dpre are time-major (T,B,O) against a batch-major target (B,T,O) - the unrolled decoders keep
    // their tape time-major, no transposed copies
    // dbO > 0 (batch-major only, with a ticket): the Dense bias gradient db[o] = sum over rows of dpre[row][o] as well - per-block
    // column sums in a fixed order, added over the blocks (in block order) by the block that takes the last ticket: the
    // column-sum launches of dense_bwd (7.6 us at the reference's batch) are gone
    __shared__ float red[256];
    __shared__ float gval[256];
    __shared__ int is_last;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    float sq = 0.f;
    if (dbO > 0) gval[threadIdx.x] = 0.f;
    if (i < n) {
        long ti = i;
        if (tmT > 0) {   // i = (t*B + b)*O + o  ->  (b*T + t)*O + o
            const long row = i / O;
            const int o = (int)(i - row * O);
            const long t = row / tmB, b = row - t * tmB;
            ti = (b * tmT + t) * O + o;
        }
        const float yv = y[i], d = yv - target[ti];
        sq = d * d;
        float gsc = 2.f * d * scale;
        if (activation == 1) gsc *= (1.f - yv * yv);
        dpre[i] = gsc;
        if (dbO > 0) gval[threadIdx.x] = gsc;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sq += __shfl_xor(sq, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    __shared__ float cpart[32][8];
    const int co = threadIdx.x & 7, cq = threadIdx.x >> 3;   // column, one of 32 strands of it
    if (dbO > 0) {
        // element j of the block is i0 + j, its column (i0 + j) % dbO: strand cq of column co takes every 32nd of them, the
        // 32 strand sums are added in strand order (a fixed order: the same bits every time)
        const int c0 = (int)(((long)blockIdx.x * 256) % dbO);
        float a = 0.f;
        if (co < dbO)
            for (int j = (co - c0 + dbO) % dbO + dbO * cq; j < 256; j += dbO * 32) a += gval[j];
        cpart[cq][co] = a;
        __syncthreads();
        if (threadIdx.x < 8) {
            float sum = 0.f;
            for (int q = 0; q < 32; ++q) sum += cpart[q][threadIdx.x];
            gval[threadIdx.x] = sum;   // (every strand has been read: the barrier above; columns >= dbO are zero)
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float part = red[0] + red[1] + red[2] + red[3];
        if (ticket) {
            __hip_atomic_store(loss_part + blockIdx.x, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // the block's column sums leave through the SAME thread and fence (a fence per storing thread made the kernel
            // 32 us at 720 blocks where it had been 4.8)
            // two 16-byte stores (the fence below publishes them; col_part rows are 32 bytes, the area 16-byte aligned)
            if (dbO > 0) {
                f32x4* cp = (f32x4*)(col_part + (size_t)blockIdx.x * 8);
                cp[0] = (f32x4){gval[0], gval[1], gval[2], gval[3]};
                cp[1] = (f32x4){gval[4], gval[5], gval[6], gval[7]};
            }
            __threadfence();
            is_last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
        } else {
            loss_part[blockIdx.x] = part;
            is_last = 0;
        }
    }
    __syncthreads();
    if (is_last) {   // the arithmetic of sum_scale_kernel (same order: bit-identical loss), by the block that finished last
        __threadfence();
        if (dbO > 0) {   // (block-uniform) the blocks' column sums: 32 strands per column over the blocks, then in strand order
            // (L1-bypassing buffer loads, eight in flight: agent-scope atomic loads are issued one round trip at a time - 23 of them
            // per lane made this kernel 36 us at 720 blocks)
            const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(col_part, 0, (int)(gridDim.x * 8u * 4u), 0x00020000);
            float a = 0.f;
            for (int b0 = cq; b0 < (int)gridDim.x; b0 += 32 * 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)   // blocks beyond the grid: offset past the descriptor, reads as 0
                    v[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(prs, (unsigned)(((b0 + 32 * u) * 8 + co) * 4), 0, 16 /* sc1 */));
#pragma unroll
                for (int u = 0; u < 8; ++u) a += v[u];
            }
            if (co >= dbO) a = 0.f;
            cpart[cq][co] = a;
            __syncthreads();
            if ((int)threadIdx.x < dbO) {
                float sum = 0.f;
                for (int q = 0; q < 32; ++q) sum += cpart[q][threadIdx.x];
                db_out[threadIdx.x] = sum;
            }
            __syncthreads();
        }
        float a = 0.f;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) a += __hip_atomic_load(loss_part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        red[threadIdx.x] = a;
        __syncthreads();
        for (int m = 128; m >= 1; m >>= 1) {
            if (threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            loss_out[0] = red[0] * loss_scale;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the slot's next user finds it at zero
        }
    }
}

__global__ __launch_bounds__(256) void sum_scale_kernel(const float* __restrict__ part, float* __restrict__ out, int n,
                                                        float scale) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] * scale;
}

// Gaussian negative log-likelihood of mycode/cost.py:190-229 (likelihood_loss_tf): per sequence b, target second t,
// frame f and axis a:  l = log(var_a + eps) + (y - mu_a)^2 / (var_a + eps), clipped to [-10, 10];
// loss = scale * mean_b sum_{t,f,a} l.  One block per sequence: partial loss into part[b], dmu / dvar (B,3) with the
// clip's zero gradient outside [-10, 10].
__global__ __launch_bounds__(256) void gauss_nll_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                        const float* __restrict__ y, float* __restrict__ part,
                                                        float* __restrict__ dmu, float* __restrict__ dvar, int B, int Ty,
                                                        int fps, float scale, unsigned* __restrict__ ticket, float* __restrict__ loss_out,
                                                        float loss_scale) {
    __shared__ float red[256][7];
    __shared__ int is_last;
    const int b = blockIdx.x;
    const int per = Ty * fps * 3;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // loss, dmu[3], dvar[3]
    const float eps = 1e-20f;
    for (int e = threadIdx.x; e < per; e += 256) {
        const int a = e % 3;
        const float m = mu[b * 3 + a], v = var[b * 3 + a] + eps;
        const float d = y[(size_t)b * per + e] - m;
        const float l = __logf(v) + d * d / v;
        acc[0] += fminf(fmaxf(l, -10.f), 10.f);
        if (l > -10.f && l < 10.f) {
            acc[1 + a] += -2.f * d / v;
            acc[4 + a] += 1.f / v - d * d / (v * v);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) red[threadIdx.x][k] = acc[k];
    __syncthreads();
    for (int s_ = 128; s_ > 0; s_ >>= 1) {
        if ((int)threadIdx.x < s_)
#pragma unroll
            for (int k = 0; k < 7; ++k) red[threadIdx.x][k] += red[threadIdx.x + s_][k];
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        dmu[b * 3 + threadIdx.x] = red[0][1 + threadIdx.x] * scale / (float)B;
        dvar[b * 3 + threadIdx.x] = red[0][4 + threadIdx.x] * scale / (float)B;
    }
    if (threadIdx.x == 0) {
        if (ticket) {
            __hip_atomic_store(part + b, red[0][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
            is_last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
        } else {
            part[b] = red[0][0];
            is_last = 0;
        }
    }
    __syncthreads();
    if (is_last) {   // the arithmetic of sum_scale_kernel, by the block that finished last (round 4: one launch less per step)
        __threadfence();
        float a = 0.f;
        for (int i = threadIdx.x; i < B; i += 256) a += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        red[threadIdx.x][0] = a;
        __syncthreads();
        for (int m = 128; m >= 1; m >>= 1) {
            if ((int)threadIdx.x < m) red[threadIdx.x][0] += red[threadIdx.x + m][0];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            loss_out[0] = red[0][0] * loss_scale;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Sampled re-feed (mycode/lstm.py:460-468 via utility.py:83-89; lstm_keras.py:39-44,139-149): one second of fps frames
// drawn around the predicted mean, x = mu_a + sd(var_a) * noise, noise ~ N(0,1) supplied by the caller in the layout of x.
// std_mode 0: sd = sqrt(var) (lstm.py); 1: sd = var (lstm_keras.py passes the variance as stddev).  layout 0: frames
// interleaved x,y,z (tf.stack axis=-1 + reshape); 1: planar [x*fps | y*fps | z*fps] (Concatenate axis=-1).
// One wave per sequence; x / dx rows are ldx floats apart (a slot of the (B,T,3*fps) window).
__global__ __launch_bounds__(64) void sample_refeed_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                               const float* __restrict__ noise, float* __restrict__ x, long ldx,
                                                               int fps, int std_mode, int layout) {
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < 3 * fps; e += 64) {
        const int a = layout ? e / fps : e % 3;
        const float v = var[b * 3 + a];
        x[(size_t)b * ldx + e] = mu[b * 3 + a] + (std_mode ? v : sqrtf(v)) * noise[(size_t)b * 3 * fps + e];
    }
}

// dmu_a (+)= sum_frames dx;  dvar_a (+)= sum_frames dx * noise * sd'(var_a)   (sd' = 1/(2 sqrt(var)) or 1, IEEE as in TF)
__global__ __launch_bounds__(64) void sample_refeed_bwd_kernel(const float* __restrict__ dx, long ldx, const float* __restrict__ var,
                                                               const float* __restrict__ noise, float* __restrict__ dmu,
                                                               float* __restrict__ dvar, int fps, int std_mode, int layout,
                                                               int accumulate) {
    const int b = blockIdx.x;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = threadIdx.x; e < 3 * fps; e += 64) {
        const int a = layout ? e / fps : e % 3;
        const float d = dx[(size_t)b * ldx + e], n = noise[(size_t)b * 3 * fps + e];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] += a == k ? d : 0.f;
            acc[3 + k] += a == k ? d * n : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float v = var[b * 3 + a];
        const float gm = a == 0 ? acc[0] : (a == 1 ? acc[1] : acc[2]);
        const float gs = a == 0 ? acc[3] : (a == 1 ? acc[4] : acc[5]);
        const float gv = std_mode ? gs : gs * 0.5f / sqrtf(v);
        dmu[b * 3 + a] = (accumulate ? dmu[b * 3 + a] : 0.f) + gm;
        dvar[b * 3 + a] = (accumulate ? dvar[b * 3 + a] : 0.f) + gv;
    }
}

// Unit-norm regulariser of costfunc._mse under cfg.add_xyz_sum1 (mycode/cost.py:20-29): per pixel (row of C >= 3 channels)
// r = ux^2 + uy^2 + uz^2 - 1;  reg = 0.5 * mean_pixels r^2;  d reg / d u_k = 2 r u_k / n_pix, ADDED to dp.  Block partials of
// sum r^2 go to part[] (reduced in fixed order by sum_scale_kernel, so the loss is deterministic).
__global__ __launch_bounds__(256) void xyz_sum1_kernel(const float* __restrict__ p, float* __restrict__ dp, float* __restrict__ part,
                                                       long n_pix, int C) {
    __shared__ float red[256];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    float r2 = 0.f;
    if (i < n_pix) {
        const float x = p[i * C], y = p[i * C + 1], z = p[i * C + 2];
        const float r = x * x + y * y + z * z - 1.f;
        const float gsc = 2.f * r / (float)n_pix;
        dp[i * C] += gsc * x;
        dp[i * C + 1] += gsc * y;
        dp[i * C + 2] += gsc * z;
        r2 = r * r;
    }
    red[threadIdx.x] = r2;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// Keras-2.2 categorical_crossentropy on probabilities (convlstm_heatmap.py:192: model.compile(loss='categorical_crossentropy',
// optimizer='adam')), TensorFlow backend form: q = p / sum_c p;  q' = clip(q, 1e-7, 1 - 1e-7);  l = - sum_c t_c log q'_c per pixel,
// loss = mean over pixels.  Gradient w.r.t. p through the clip (zero outside) and the renormalisation:
//   g_c = -t_c / q'_c [eps < q_c < 1 - eps];   dl/dp_k = (g_k - sum_c g_c q_c) / S;   dp = that / n_pix.
// One thread per pixel (C <= 64 channels re-read from cache for the second pass).
__global__ __launch_bounds__(256) void cce_grad_kernel(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ dp,
                                                       float* __restrict__ part, long n_pix, int C) {
    __shared__ float red[256];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    float l = 0.f;
    if (i < n_pix) {
        const float* pi = p + i * C;
        const float* ti = t + i * C;
        const float eps = 1e-7f;
        float S = 0.f;
        for (int c = 0; c < C; ++c) S += pi[c];
        const float inv = 1.f / S;
        float dot = 0.f;
        for (int c = 0; c < C; ++c) {
            const float q = pi[c] * inv;
            const float qc = fminf(fmaxf(q, eps), 1.f - eps);
            l -= ti[c] * __logf(qc);
            const float g = (q > eps && q < 1.f - eps) ? -ti[c] / qc : 0.f;
            dot += g * q;
        }
        const float sc = inv / (float)n_pix;
        for (int c = 0; c < C; ++c) {
            const float q = pi[c] * inv;
            const float qc = fminf(fmaxf(q, eps), 1.f - eps);
            const float g = (q > eps && q < 1.f - eps) ? -ti[c] / qc : 0.f;
            dp[i * C + c] = (g - dot) * sc;
        }
    }
    red[threadIdx.x] = l;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------------------------------
// Dense(O, tanh | linear) head + Keras mean_squared_error, FORWARD AND BACKWARD IN ONE LAUNCH (round 5) - what model.fit runs
// around the decoder's hidden sequence in mycode/FoV_seq2seq.py:96-103: y = act(hs . W + b), loss = w mean (y - target)^2,
// dpre = dloss/d(pre-activation), dX = dpre . W^T (into the decoder's BPTT), dW = hs^T . dpre, db = column sums of dpre.
// At the reference's batch (32 x 10 = 320 rows, H = 128, O = 6) these were five launches of 4-8 us each - the Dense forward,
// the loss kernel, two GEMMs and a column sum - for 0.5 MFLOP: a sixth of the training step.  A block takes 64 rows: the hs
// tile and W sit in LDS, four lanes share a row's dot products, dX rows leave as whole 16-byte-per-lane lines, the block's
// partial dW / db / squared-error sum go to scratch and the block that takes the last ticket adds the partials IN BLOCK ORDER
// (deterministic).  Rows <= 4096 (64 blocks); larger heads keep the separate launches, which are <= 1 % of their step.
// ---------------------------------------------------------------------------------------
constexpr int HD_RB = 64;        // rows per block
constexpr int HD_MAXB = 64;      // blocks per launch at most
__host__ __device__ inline size_t dense_mse_head_lds_floats(int H) { return (size_t)HD_RB * (H + 4) + (size_t)H * 8 + HD_RB * 8 + 16; }
__global__ __launch_bounds__(256) void dense_mse_head_kernel(const float* __restrict__ hs, const float* __restrict__ W, const float* __restrict__ bias,
                                                             const float* __restrict__ target, float* __restrict__ y_out, float* __restrict__ dX,
                                                             float* __restrict__ part, float* __restrict__ dW, float* __restrict__ db,
                                                             float* __restrict__ loss, int N, int H, int O, int activation, float scale,
                                                             unsigned* __restrict__ ticket, int chunks_per_block, int finish) {
    extern __shared__ __attribute__((aligned(16))) float hd_sm[];
    const int LDH = H + 4;
    float* sHs = hd_sm;                       // [64][H + 4]
    float* sWt = sHs + HD_RB * LDH;           // [H][8] (columns >= O zero)
    float* sD = sWt + H * 8;                  // dpre [64][8] (rows >= N, columns >= O zero)
    float* sRed = sD + HD_RB * 8;             // 4 wave sums of the squared error
    __shared__ int is_last;
    const int tid = threadIdx.x;
    const int C4 = H >> 2;                    // 16-byte pieces per row
    // More than 64 x 64 rows (round 5: the 30 720 rows of configs[1]'s training step): a block walks `chunks_per_block` tiles of 64
    // rows, its partial dW / db / squared error stay in registers across them, and a second launch adds the blocks' partials
    // (finish = 0) - the last-block reduce below is one block reading every partial.
    float aw[2][8], adb = 0.f, sq_tot = 0.f;      // dW rows tid and tid + 256 (H <= 512), db[tid], squared error (thread 0)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int o = 0; o < 8; ++o) aw[kk][o] = 0.f;
    const int chunk0 = blockIdx.x * chunks_per_block;
    for (int ch = 0; ch < chunks_per_block; ++ch) {
    const int r0 = (chunk0 + ch) * HD_RB;
    if (r0 >= N) break;
    if (ch > 0) __syncthreads();              // the previous tile's readers are done
    // ---- stage the hs tile (rows past N: zero) and W ----
    // (every request of the tile goes out before the first LDS store: a load-then-store loop is one memory round trip per
    // iteration on a CU that runs one wave per SIMD - 8 us of the kernel's first 18)
    {
        const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hs + (size_t)r0 * H), 0,
                                                                             (N - r0 < HD_RB ? N - r0 : HD_RB) * H * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, H * O * 4, 0x00020000);
        constexpr int HIT = HD_RB * 128 / 256;      // 16-byte pieces per thread at H = 512
        typedef unsigned hu32x4 __attribute__((ext_vector_type(4)));
        hu32x4 hv[HIT];
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int i = tid + 256 * it;
            hv[it] = __builtin_amdgcn_raw_buffer_load_b128(hrs, i < HD_RB * C4 ? (unsigned)(i * 16) : 0x80000000u, 0, 0);   // rows past N: beyond the descriptor = 0
        }
        float wv[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {      // (W: the block's first tile only - later passes request nothing)
            const int i = tid + 256 * it, k = i >> 3, o = i & 7;
            wv[it] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, (ch == 0 && i < H * 8 && o < O) ? (unsigned)((k * O + o) * 4) : 0x80000000u, 0, 0));
        }
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int i = tid + 256 * it;
            if (i < HD_RB * C4) {
                const int r = i / C4, c4 = i - r * C4;
                *(hu32x4*)(sHs + r * LDH + 4 * c4) = hv[it];
            }
        }
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int i = tid + 256 * it;
            if (ch == 0 && i < H * 8) sWt[i] = wv[it];
        }
    }
    __syncthreads();
    // ---- forward + loss gradient: lanes 4r .. 4r+3 share row r (k = 4j + q: the four read neighbouring words) ----
    const int r = tid >> 2, q = tid & 3;
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = 0.f;
#pragma unroll 8
    for (int j = 0; j < C4; ++j) {
        const int k = 4 * j + q;
        const float h = sHs[r * LDH + k];
        const f32x4 w0 = *(const f32x4*)(sWt + k * 8), w1 = *(const f32x4*)(sWt + k * 8 + 4);
#pragma unroll
        for (int o = 0; o < 4; ++o) { acc[o] = fmaf(h, w0[o], acc[o]); acc[4 + o] = fmaf(h, w1[o], acc[4 + o]); }
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        acc[o] += __shfl_xor(acc[o], 1);
        acc[o] += __shfl_xor(acc[o], 2);
    }
    float sq = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {    // lane q owns the outputs q and q + 4
        const int o = q + 4 * half;
        float g = 0.f;
        if (o < O && r0 + r < N) {
            const float lo = q == 0 ? acc[0] : (q == 1 ? acc[1] : (q == 2 ? acc[2] : acc[3]));      // (register arrays take no lane-dependent index)
            const float hi2 = q == 0 ? acc[4] : (q == 1 ? acc[5] : (q == 2 ? acc[6] : acc[7]));
            const float pre = (half ? hi2 : lo) + bias[o];
            const float yv = activation == 1 ? tanh_f(pre) : pre;
            const size_t e = (size_t)(r0 + r) * O + o;
            if (y_out) y_out[e] = yv;
            const float d = yv - target[e];
            sq += d * d;
            g = 2.f * d * scale;
            if (activation == 1) g *= (1.f - yv * yv);
        }
        sD[r * 8 + o] = g;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sq += __shfl_xor(sq, m);
    if ((tid & 63) == 0) sRed[tid >> 6] = sq;
    __syncthreads();
    // ---- dX = dpre . W^T: a thread keeps its four k rows of W, a wave instruction writes whole rows ----
    if (dX) {
        const int c4 = tid % C4, rsub = tid / C4, rstep = 256 / C4;      // (H <= 512: C4 <= 128, at least two rows per pass)
        if (rsub < rstep) {
            float wk[4][8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 w0 = *(const f32x4*)(sWt + (4 * c4 + i) * 8), w1 = *(const f32x4*)(sWt + (4 * c4 + i) * 8 + 4);
#pragma unroll
                for (int o = 0; o < 4; ++o) { wk[i][o] = w0[o]; wk[i][4 + o] = w1[o]; }
            }
            for (int rr = rsub; rr < HD_RB && r0 + rr < N; rr += rstep) {
                const f32x4 g0 = *(const f32x4*)(sD + rr * 8), g1 = *(const f32x4*)(sD + rr * 8 + 4);
                f32x4 out;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float a = 0.f;
#pragma unroll
                    for (int o = 0; o < 4; ++o) a = fmaf(g0[o], wk[i][o], fmaf(g1[o], wk[i][4 + o], a));
                    out[i] = a;
                }
                *(f32x4*)(dX + (size_t)(r0 + rr) * H + 4 * c4) = out;
            }
        }
    }
    // ---- the block's partial dW[k][o] += sum_r hs[r][k] dpre[r][o], db[o] += sum_r dpre[r][o], squared error ----
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int k = tid + 256 * kk;
        if (k < H) {
#pragma unroll 8
            for (int rr = 0; rr < HD_RB; ++rr) {
                const float h = sHs[rr * LDH + k];
                const f32x4 g0 = *(const f32x4*)(sD + rr * 8), g1 = *(const f32x4*)(sD + rr * 8 + 4);
#pragma unroll
                for (int o = 0; o < 4; ++o) { aw[kk][o] = fmaf(h, g0[o], aw[kk][o]); aw[kk][4 + o] = fmaf(h, g1[o], aw[kk][4 + o]); }
            }
        }
    }
    if (tid < O) {
        float a = 0.f;
        for (int rr = 0; rr < HD_RB; ++rr) a += sD[rr * 8 + tid];
        adb += a;
    }
    if (tid == 0) sq_tot += (sRed[0] + sRed[1]) + (sRed[2] + sRed[3]);
    }   // tiles of this block
    const int NE = H * O + O + 1;
    float* mypart = part + (size_t)blockIdx.x * NE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int k = tid + 256 * kk;
        if (k < H)
        {
#pragma unroll
            for (int o = 0; o < 8; ++o)
                if (o < O) mypart[(size_t)k * O + o] = aw[kk][o];
        }
    }
    if (tid < O) mypart[(size_t)H * O + tid] = adb;
    if (tid == 0) mypart[NE - 1] = sq_tot;
    if (!finish) return;                      // a reduce launch adds the blocks' partials (dense_mse_head_reduce_kernel)
    __threadfence();
    __syncthreads();
    if (tid == 0) is_last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (is_last) {
        __threadfence();
        // L1-bypassing loads (another launch's partials may sit in this CU's L1 under the same addresses), ALL of an element's
        // requested before the first is used: as a chain of load-then-add the five partials of the reference's batch cost a
        // memory round trip each (the kernel took 19 us, 14 of them here)
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(part, 0, (int)(gridDim.x * (unsigned)NE * 4u), 0x00020000);
        for (int e = tid; e < NE; e += 256) {
            float v[HD_MAXB];
#pragma unroll
            for (int blk = 0; blk < HD_MAXB; ++blk)
                v[blk] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(prs, (unsigned)((blk * NE + e) * 4), 0, 16 /* sc1 */));   // blocks past the grid: out of range = 0
            float a = 0.f;
#pragma unroll
            for (int blk = 0; blk < HD_MAXB; ++blk) a += v[blk];      // block order: deterministic (absent blocks add +0)
            if (e < H * O) dW[e] = a;
            else if (e < H * O + O) db[e - H * O] = a;
            else if (loss) loss[0] = a * scale;
        }
        if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the slot is this stream's again
    }
}

// The second launch of the head at more than 4 096 rows: element e of (dW | db | squared error) = the blocks' partials in block
// order.  16 elements x 16 partial groups per block (group q adds partials q, q + 16, ...; the 16 group sums are folded in a fixed
// order): a hundred blocks instead of one block reading everything.
__global__ __launch_bounds__(256) void dense_mse_head_reduce_kernel(const float* __restrict__ part, int nb, int NE, int HO, int O,
                                                                    float* __restrict__ dW, float* __restrict__ db, float* __restrict__ loss,
                                                                    float scale) {
    __shared__ float red[16][17];
    const int el = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    float a = 0.f;
    if (e < NE) {
        int b = q;
        for (; b + 7 * 16 < nb; b += 8 * 16) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(b + 16 * u) * NE + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += v[u];
        }
        for (; b < nb; b += 16) a += part[(size_t)b * NE + e];
    }
    red[q][el] = a;
    __syncthreads();
    if (q == 0 && e < NE) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[g][el];
        if (e < HO) dW[e] = t;
        else if (e < HO + O) db[e - HO] = t;
        else if (loss) loss[0] = t * scale;
    }
}

// The ticket word of a loss launch: one slot of the device's ticket table PER STREAM (first use of a stream on a device takes
// the next free slot; the device address of g_loss_tickets is looked up once per device).  Launches on one stream run in
// stream order, so the word a launch finds is the zero its predecessor on that stream left: two launches in flight never share
// a slot however many there are, whichever threads issued them.  Slots are never handed back (a stream handle may still have a
// launch in flight when its owner forgets it): a device on which kLossTickets = 1024 distinct streams have issued loss calls
// gets NULL for further ones - the callers below fall back to the separate sum / column-sum launches, fov_dense_mse_head refuses.
// (A captured graph replayed on two streams AT ONCE would share the slot of its capture stream: not supported.)
static unsigned* loss_ticket_of(hipStream_t stream) {
    struct PerDevice { unsigned* base = nullptr; std::unordered_map<hipStream_t, int> slot; };
    static std::mutex mu;
    static PerDevice devs[64];
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    PerDevice& d = devs[dev];
    if (!d.base) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_loss_tickets)) != hipSuccess) return nullptr;
        d.base = static_cast<unsigned*>(p);
    }
    auto it = d.slot.find(stream);
    if (it != d.slot.end()) return d.base + it->second;
    if ((int)d.slot.size() == kLossTickets) return nullptr;
    const int idx = (int)d.slot.size();
    d.slot.emplace(stream, idx);
    return d.base + idx;
}

// a loss asked for without a ticket slot (or by a kernel that takes none): the blocks' partials added by a launch of its own
static int sum_partials(const float* part, float* out, int n, float scale, hipStream_t stream) {
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, stream, part, out, n, scale);
    return launch_check("sum_scale");
}

// Body of the two entries below (`name`: the entry's error prefix and trace label).  weight: on the gradient AND the loss
// (data parallelism: this rank's share n_local / n_global of the global mean, so that a SUM all-reduce of gradients and
// loss gives the global-batch values without a scaling pass); tmT > 0: a time-major prediction.
static int mse_dense_grad_body(const char* name, const float* y, const float* target, float* dpre, float* loss, long n, int activation,
                               float weight, int tmB, int tmT, int O, float* scratch, size_t scratch_floats, hipStream_t stream,
                               float* db, int dbO) {
    if (n <= 0) return (db && dbO > 0) ? zero_grad(db, (size_t)dbO, stream) : FOV_OK;
    const long blocks = (n + 255) / 256;
    if ((size_t)blocks * (db ? 9 : 1) + (db ? 4 : 0) > scratch_floats) { set_error("%s: scratch too small", name); return FOV_ERR_WORKSPACE; }
    unsigned* ticket = loss ? loss_ticket_of(stream) : nullptr;
    const bool fused_db = db && ticket && dbO >= 1 && dbO <= 8 && tmT == 0 && n % dbO == 0;
    if (fused_db)       // the kernel's last block stores db: pending deferred reductions over it go first
        if (int rc = defer_touch(db, (size_t)dbO, stream)) return rc;
    hipLaunchKernelGGL(mse_dense_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, y, target, dpre, scratch, n,
                       weight / (float)n, activation, tmB, tmT, O, ticket, loss, weight / (float)n,
                       fused_db ? scratch + ((blocks + 3) & ~3L) : nullptr, fused_db ? db : nullptr, fused_db ? dbO : 0);
    int rc = launch_check(name);
    if (rc) return rc;
    if (db && !fused_db) {   // (no ticket slot, wide or time-major head: the column-sum launches)
        if (dbO < 1 || n % dbO) { set_error("%s: db needs the head's width", name); return FOV_ERR_INVALID; }
        rc = colsum(dpre, db, (int)(n / dbO), dbO, 0, scratch + ((blocks + 3) & ~3L), scratch_floats - ((blocks + 3) & ~3L), stream);
        if (rc) return rc;
    }
    return (loss && !ticket) ? sum_partials(scratch, loss, (int)blocks, weight / (float)n, stream) : rc;
}

int mse_dense_grad(const float* y, const float* target, float* dpre, float* loss, long n, int activation, float* scratch,
                   size_t scratch_floats, hipStream_t stream) {
    return mse_dense_grad_body("mse_dense_grad", y, target, dpre, loss, n, activation, 1.0f, 0, 0, 1, scratch, scratch_floats, stream, nullptr, 0);
}

int mse_dense_grad_w(const float* y, const float* target, float* dpre, float* loss, long n, int activation, float weight,
                     int tmB, int tmT, int O, float* scratch, size_t scratch_floats, hipStream_t stream, float* db, int dbO) {
    return mse_dense_grad_body("mse_dense_grad_w", y, target, dpre, loss, n, activation, weight, tmB, tmT, O, scratch, scratch_floats, stream, db, dbO);
}

bool dense_mse_head_shape_ok(long N, int H, int O) {
    return N >= 1 && N <= (1L << 20) && H >= 4 && H <= 512 && (H & 3) == 0 && O >= 1 && O <= 8;
}
size_t dense_mse_head_scratch_floats(long N, int H, int O) { return (size_t)((N + HD_RB - 1) / HD_RB) * ((size_t)H * O + O + 1) + 64; }
// weight: this rank's share of the global batch (data parallelism), 1 otherwise; loss = weight * mean over all N * O elements
int dense_mse_head(const float* hs, const float* W, const float* b, const float* target, float* y, float* dX, float* dW, float* db,
                   float* loss, long N, int H, int O, int activation, float weight, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (!dense_mse_head_shape_ok(N, H, O)) { set_error("dense_mse_head: rows <= 2^20, H <= 512 (a multiple of 4), O <= 8 only"); return FOV_ERR_UNSUPPORTED; }
    if (dense_mse_head_scratch_floats(N, H, O) > scratch_floats) { set_error("dense_mse_head: scratch too small"); return FOV_ERR_WORKSPACE; }
    unsigned* ticket = loss_ticket_of(stream);
    if (!ticket) { set_error("dense_mse_head: no ticket slot left for this stream (1024 distinct streams have issued loss calls on the device)"); return FOV_ERR_UNSUPPORTED; }
    int rc = defer_touch(dW, (size_t)H * O, stream);     // pending deferred reductions over the gradients written here go first
    if (!rc) rc = defer_touch(db, (size_t)O, stream);
    if (rc) return rc;
    const size_t lds = dense_mse_head_lds_floats(H) * sizeof(float);
    rc = ensure_dynamic_lds((const void*)dense_mse_head_kernel, lds);
    if (rc) return rc;
    const int chunks = (int)((N + HD_RB - 1) / HD_RB);
    const float scale = weight / (float)(N * O);
    if (chunks <= HD_MAXB) {      // one launch: the last block to finish adds the partials
        hipLaunchKernelGGL(dense_mse_head_kernel, dim3((unsigned)chunks), dim3(256), lds, stream, hs, W, b, target, y, dX, scratch, dW, db, loss,
                           (int)N, H, O, activation, scale, ticket, 1, 1);
        return launch_check("dense_mse_head");
    }
    // many rows: about one block per CU walking several tiles (two per CU measured no faster: 39.9 vs 37.1 us at 30 720 rows), then the reduce launch
    const int cus = device_cu_count() > 0 ? device_cu_count() : 256;
    const int cpb = (chunks + cus - 1) / cus;
    const int blocks = (chunks + cpb - 1) / cpb;
    hipLaunchKernelGGL(dense_mse_head_kernel, dim3((unsigned)blocks), dim3(256), lds, stream, hs, W, b, target, y, dX, scratch, dW, db, loss,
                       (int)N, H, O, activation, scale, ticket, cpb, 0);
    rc = launch_check("dense_mse_head");
    if (rc) return rc;
    const int NE = H * O + O + 1;
    hipLaunchKernelGGL(dense_mse_head_reduce_kernel, dim3((unsigned)((NE + 15) / 16)), dim3(256), 0, stream, scratch, blocks, NE, H * O, O, dW, db,
                       loss, scale);
    return launch_check("dense_mse_head_reduce");
}

int gauss_nll_grad(const float* mu, const float* var, const float* y, float* loss, float* dmu, float* dvar, int B, int Ty,
                   int fps, float scale, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (B <= 0) return FOV_OK;
    if ((size_t)B > scratch_floats) { set_error("gauss_nll_grad: scratch too small"); return FOV_ERR_WORKSPACE; }
    unsigned* ticket = loss ? loss_ticket_of(stream) : nullptr;
    hipLaunchKernelGGL(gauss_nll_kernel, dim3(B), dim3(256), 0, stream, mu, var, y, scratch, dmu, dvar, B, Ty, fps, scale, ticket, loss,
                       scale / (float)B);
    int rc = launch_check("gauss_nll");
    if (rc || !loss || ticket) return rc;
    return sum_partials(scratch, loss, B, scale / (float)B, stream);
}

int cce_grad(const float* p, const float* t, float* dp, float* loss, long n_pix, int C, float* scratch, size_t scratch_floats,
             hipStream_t stream) {
    if (n_pix <= 0) return FOV_OK;
    const long blocks = (n_pix + 255) / 256;
    if ((size_t)blocks > scratch_floats) { set_error("categorical_crossentropy_grad: scratch too small"); return FOV_ERR_WORKSPACE; }
    hipLaunchKernelGGL(cce_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, t, dp, scratch, n_pix, C);
    int rc = launch_check("cce_grad");
    if (rc || !loss) return rc;
    return sum_partials(scratch, loss, (int)blocks, 1.0f / (float)n_pix, stream);
}

int xyz_sum1_grad(const float* p, float* dp, float* reg, long n_pix, int C, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (n_pix <= 0) return FOV_OK;
    const long blocks = (n_pix + 255) / 256;
    if ((size_t)blocks > scratch_floats) { set_error("xyz_sum1_grad: scratch too small"); return FOV_ERR_WORKSPACE; }
    hipLaunchKernelGGL(xyz_sum1_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, dp, scratch, n_pix, C);
    int rc = launch_check("xyz_sum1");
    if (rc || !reg) return rc;
    return sum_partials(scratch, reg, (int)blocks, 0.5f / (float)n_pix, stream);
}

int sample_refeed_fwd(const float* mu, const float* var, const float* noise, float* x, long ldx, int B, int fps, int std_mode,
                      int layout, hipStream_t stream) {
    if (B <= 0) return FOV_OK;
    hipLaunchKernelGGL(sample_refeed_fwd_kernel, dim3(B), dim3(64), 0, stream, mu, var, noise, x, ldx, fps, std_mode, layout);
    return launch_check("sample_refeed_fwd");
}

int sample_refeed_bwd(const float* dx, long ldx, const float* var, const float* noise, float* dmu, float* dvar, int B, int fps,
                      int std_mode, int layout, int accumulate, hipStream_t stream) {
    if (B <= 0) return FOV_OK;
    hipLaunchKernelGGL(sample_refeed_bwd_kernel, dim3(B), dim3(64), 0, stream, dx, ldx, var, noise, dmu, dvar, fps, std_mode, layout,
                       accumulate);
    return launch_check("sample_refeed_bwd");
}

// x *= s (fallback gradient weighting of the trainers that do not fold the weight into their loss kernel)
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, long n, float s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] *= s;
}
int scale_inplace(float* x, long n, float s, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, s);
    return launch_check("scale");
}

// y = act(x): 1 tanh, 2 relu, 3 exp (heads of mycode/lstm.py:321-337); in place allowed
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* x, float* y, long n, int activation) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = activation == 1 ? tanh_f(v) : (activation == 2 ? fmaxf(v, 0.f) : (activation == 3 ? __expf(v) : v));
}
int act_fwd(const float* x, float* y, long n, int activation, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    hipLaunchKernelGGL(act_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n, activation);
    return launch_check("act_fwd");
}

// out = base + dy * act'(y)   (act' = 1 - y^2 for tanh, [y > 0] for relu, y for exp, 1 for linear); base may be NULL; out may alias base/dy
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                      const float* base, float* out, long n, int activation) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float yv = y[i];
    const float d = dy[i] * (activation == 1 ? (1.f - yv * yv) : (activation == 2 ? (yv > 0.f ? 1.f : 0.f) : (activation == 3 ? yv : 1.f)));
    out[i] = (base ? base[i] : 0.f) + d;
}
int act_bwd(const float* dy, const float* y, const float* base, float* out, long n, int activation, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    hipLaunchKernelGGL(act_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dy, y, base, out, n, activation);
    return launch_check("act_bwd");
}

// Keras-2.2 optimizers on one flat buffer (oracle/fov_oracle.py::adam_step / rmsprop_step)
// guard0..2 (each may be NULL): sticky timeout words of the workspaces the step's persistent kernels used
// (xch_common.h).  If one is set the gradients are garbage: the update is skipped on the device - no host sync - and
// the parameters stay as they were until fov_check_status reports the failure.
__device__ __forceinline__ bool optimizer_poisoned(const unsigned* g0, const unsigned* g1, const unsigned* g2) {
    return (g0 && *g0 != 0u) || (g1 && *g1 != 0u) || (g2 && *g2 != 0u);
}

// data parallelism: this rank's guard words as ONE float slot of the gradient buffer, so that the SUM all-reduce of that
// buffer tells every rank whether ANY rank's step failed and all of them skip (or apply) the update together
__global__ void guard_flag_kernel(const unsigned* g0, const unsigned* g1, const unsigned* g2, float* out) {
    *out = optimizer_poisoned(g0, g1, g2) ? 1.f : 0.f;
}
int guard_flag(const unsigned* const* guards, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(guard_flag_kernel, dim3(1), dim3(1), 0, stream, guards[0], guards[1], guards[2], out);
    return launch_check("guard_flag");
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr_t, float b1, float b2, float eps,
                                                   const unsigned* g0, const unsigned* g1, const unsigned* g2, long long* applied) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || optimizer_poisoned(g0, g1, g2)) return;
    if (i == 0 && applied) *applied += 1;      // updates that really ran: what the host's step counter is set back to after a failure
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
}

// Four parameters per thread, 16-byte accesses (round 4: the one-element form moved 47 MB in 11.4 us at config 3's 1.68 M
// parameters - a quarter of the waves, a quarter of the memory instructions).  Same arithmetic per element.
__global__ __launch_bounds__(256) void adam_kernel4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, float lr_t, float b1, float b2, float eps,
                                                    const unsigned* g0, const unsigned* g1, const unsigned* g2, long long* applied) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n || optimizer_poisoned(g0, g1, g2)) return;
    if (i == 0 && applied) *applied += 1;
    if (i + 3 < n) {
        const f32x4 gi = *(const f32x4*)(g + i), m0 = *(const f32x4*)(m + i), v0 = *(const f32x4*)(v + i), p0 = *(const f32x4*)(p + i);
        f32x4 mi, vi, pi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mi[e] = b1 * m0[e] + (1.f - b1) * gi[e];
            vi[e] = b2 * v0[e] + (1.f - b2) * gi[e] * gi[e];
            pi[e] = p0[e] - lr_t * mi[e] / (sqrtf(vi[e]) + eps);
        }
        *(f32x4*)(m + i) = mi;
        *(f32x4*)(v + i) = vi;
        *(f32x4*)(p + i) = pi;
    } else {
        for (long k = i; k < n; ++k) {
            const float gk = g[k];
            const float mk = b1 * m[k] + (1.f - b1) * gk;
            const float vk = b2 * v[k] + (1.f - b2) * gk * gk;
            m[k] = mk;
            v[k] = vk;
            p[k] = p[k] - lr_t * mk / (sqrtf(vk) + eps);
        }
    }
}

__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ a,
                                                      long n, float lr, float rho, float eps, const unsigned* g0,
                                                      const unsigned* g1, const unsigned* g2, long long* applied) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || optimizer_poisoned(g0, g1, g2)) return;
    if (i == 0 && applied) *applied += 1;
    const float gi = g[i];
    const float ai = rho * a[i] + (1.f - rho) * gi * gi;
    a[i] = ai;
    p[i] = p[i] - lr * gi / (sqrtf(ai) + eps);
}

// tf.train.RMSPropOptimizer (TF 1.x, momentum 0, not centered; mycode/lstm.py:556-567) with the script's optional
// clip_by_value(grad, -clip, clip):  ms = decay*ms + (1-decay) g^2;  p -= lr * g / sqrt(ms + eps).  (eps INSIDE the
// root, ms initialised to ONE - both unlike Keras RMSprop.)
__global__ __launch_bounds__(256) void rmsprop_tf_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                                                         long n, float lr, float decay, float eps, float clip, const unsigned* g0,
                                                         const unsigned* g1, const unsigned* g2, long long* applied) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || optimizer_poisoned(g0, g1, g2)) return;     // fail-stop: a persistent kernel of the step gave up -> no update
    if (i == 0 && applied) *applied += 1;
    float gi = g[i];
    if (clip > 0.f) gi = fminf(fmaxf(gi, -clip), clip);
    const float m = decay * ms[i] + (1.f - decay) * gi * gi;
    ms[i] = m;
    p[i] = p[i] - lr * gi / sqrtf(m + eps);
}

static const unsigned* const kNoGuards[3] = {nullptr, nullptr, nullptr};   // an optimizer step handed guards == NULL

int adam_step(float* p, const float* g, float* m, float* v, long n, float lr_t, float b1, float b2, float eps,
              const unsigned* const* guards, long long* applied, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    if (int rc = defer_touch(g, (size_t)n, stream)) return rc;      // pending deferred reductions into the gradients go first
    const unsigned* const* w = guards ? guards : kNoGuards;
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0 && n >= 1024)
        hipLaunchKernelGGL(adam_kernel4, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, stream, p, g, m, v, n, lr_t, b1, b2, eps, w[0], w[1], w[2], applied);
    else
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, g, m, v, n, lr_t, b1, b2, eps, w[0], w[1], w[2], applied);
    return launch_check("adam");
}

int rmsprop_step(float* p, const float* g, float* a, long n, float lr, float rho, float eps, const unsigned* const* guards,
                 long long* applied, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    if (int rc = defer_touch(g, (size_t)n, stream)) return rc;
    const unsigned* const* w = guards ? guards : kNoGuards;
    hipLaunchKernelGGL(rmsprop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, g, a, n, lr, rho, eps, w[0], w[1], w[2], applied);
    return launch_check("rmsprop");
}

int rmsprop_tf_step(float* p, const float* g, float* ms, long n, float lr, float decay, float eps, float clip,
                    const unsigned* const* guards, long long* applied, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    if (int rc = defer_touch(g, (size_t)n, stream)) return rc;
    const unsigned* const* w = guards ? guards : kNoGuards;
    hipLaunchKernelGGL(rmsprop_tf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, g, ms, n, lr, decay, eps, clip, w[0], w[1], w[2], applied);
    return launch_check("rmsprop_tf");
}

}  // namespace fov
