// Weight gradient of a 'same' Conv2D with bf16 matrix-core operands and fp32 accumulation: the third product of a head layer's
// training step (mycode/convlstm_seq2seq.py:176-181,231-238 under model.fit; forward and data gradient are conv_patch_bf16.hip).
//
//     dw[i][j][c][n] (+)= sum over the B*H*W pixels p of  bf16(x[p + tap(i,j)][c]) * bf16(dy[p][n])
// both operands rounded to bf16 round-to-nearest-even (pack_bf16 = v_cvt_pk_bf16_f32) while they are staged into LDS - fp32 stays
// in HBM -, products accumulated in fp32 (v_mfma_f32_16x16x32_bf16), dw fp32 in the Keras (kh,kw,C,N) layout.
//
// Why not conv_wgrad_kernel's layout (one workgroup per (channel tile, tap)): at 512 -> 1024, k = 5, 1.66 M pixels the product is
// 43.5 TFLOP = 45 ms at 0.4 of the bf16 peak, and 128 x 128 tiles PER TAP pull 25 taps x 32 tiles x 1.7 GB = 2 x 680 GB of fp32
// operands through L2: 30 TB/s for those 45 ms.  The fp32 kernel lives with that at a sixth of the matrix rate; bf16 does not.
//
// conv_wgrad_bf16_kernel (the tuned form): a workgroup owns a 128 (C) x 128 (N) tile of the kw taps of ONE KERNEL ROW i and a
// slice of the maps.  The trick that makes the taps of a row share their operands is a PADDED PIXEL STREAM: a map is walked as
// H rows of PW = W + kw - 1 positions; position (y, t) of the dy stream is dy[y][t] for t < W and ZERO in the kw - 1 pad
// positions, position (y, t) of the x stream is x[y + i - kh/2][t - kw/2] or zero outside the image.  Then
//     dw[i][j] = sum over stream positions r of  xs[r + j] * dys[r]
// - the tap's shift along the row is a shift of the flat stream, the zero padding and the row wrap are the stream's own zeros
// (a product that would wrap into the next row meets a zero of dys).  A stage is 32 positions = one MFMA k-step: the dy image
// [32][128] and the x image [32 + kw - 1][128] go into LDS as bf16 as they lie (k-slow, 16-byte global loads, ds_write_b64),
// and the fragments come out through ds_read_b64_tr_b16 exactly as in gemm_bf16.hip's TN product (same k permutation, row
// stride 72 dwords: conflict-free); tap j reads the x image j rows further down, which moves every lane's bank by the same
// amount.  The price is PW / W of the matrix work (22 / 18 at the heat maps) and kw - 1 of 32 x rows staged twice.
// 8 waves as 4 (C) x 2 (N), a wave owns 32 x 64 of every tap: kw x 2 x 4 accumulator tiles (160 registers at kw = 5), and per
// stage 4 dy fragments shared by the taps + 2 x kw x fragments for 8 kw MFMAs.
//
// Operand delivery per CU and clock at kw = 5 (8 waves x 40 MFMAs x 16 cycles / 4 SIMDs = 1 280 cycles per stage):
//   LDS reads   8 waves x 14 fragments x 1 KB = 112 KB per stage =  88 B/clk of the 256 the transposed read delivers
//   LDS writes  (32 + 48) rows x 256 B        =  20 KB per stage =  16 B/clk of 128 (the x image is written 48 rows deep)
//   L2          (32 + 36) rows x 512 B fp32   =  34 KB per stage =  27 B/clk per CU (a tap-wise 128 x 128 tile at the same MFMA
//               rate would ask 32 KB per 8 x 16 x 16 / 4 = 512 cycles = 64 B/clk); x and dy are read kh = 5 times per tile pair
//               instead of 25: 2 x 136 GB at 512 -> 1024.
// Split over the maps (blockIdx.z), partial slices, fixed-order reduce: deterministic, no float atomics, no waiting.
//
// Each slice addresses its maps through 32-bit offsets from its own base, so a SLICE spans at most 2 GiB of x and of dy and the
// host cuts at least that many slices (the 6.8 GB dy of 512 -> 1024 at B 256, T 10: four at least, six chosen).  C and N need
// not be multiples of 4 where the strides are: the quad that straddles the end is loaded whole and its tail zeroed (the
// trainer's 30-channel dy lives in a 32-channel buffer).
// conv_wgrad_plain_bf16_kernel takes every other shape (strides that are no multiple of 4, unaligned views, 1 x 1 maps,
// kw > 5, and everything under FOV_NO_WGRAD_BF16_TILES=1): one thread per (tap, c, n), the rounded operands multiplied on the
// VALU - the product of two bf16 values is exact in fp32, so this is the same contract.
#include <stdio.h>

#include "bf16_common.h"

namespace fov {

namespace {

typedef short ws16x4 __attribute__((ext_vector_type(4)));

constexpr int WT = 128;          // output tile (WT channels x WT outputs) per tap
constexpr int WKB = 32;          // stream positions per stage = one MFMA k-step
constexpr int WLD = 144;         // bf16 per LDS row of a [k][WT] image: 72 dwords = 8 (mod 64)
constexpr int WXR = 48;          // rows of the x image: WKB + kw - 1 <= 48
constexpr int WTHREADS = 512;
constexpr unsigned W_OOR = 0x80000000u;

struct WgradBf16Args {
    const float* x;
    const float* dy;
    float* out;              // [slice][kh*kw][C][N]
    unsigned ldx, ldy;       // pixel stride of x, row stride of dy (floats)
    int C, N, H, W, kh, kw;
    int PW;                  // W + kw - 1 stream positions per image row
    unsigned per_map;        // H * PW
    unsigned pw_magic, h_magic;   // floor(2^32 / PW), floor(2^32 / H) (0xffffffff for 1)
    int maps, maps_per_split;
};

// (q, rem) = divmod(r, d) with magic = floor(2^32 / d): the estimate is q or q - 1 (gemm_bf16.hip, tn_row_split)
__device__ __forceinline__ void wg_divmod(unsigned r, unsigned d, unsigned magic, unsigned& q, unsigned& rem) {
    q = __umulhi(r, magic);
    rem = r - q * d;
    if (rem >= d) { ++q; rem -= d; }
}

// two transposed reads = the 8 k-values of one column for this lane group (k permutation: gemm_bf16.hip's file header)
__device__ __forceinline__ qu32x4 wg_frag(const unsigned short* img, int g4, int n, int col0) {
    const int q = n >> 2, p = n & 3;
    const unsigned short* p0 = img + (4 * g4 + q) * WLD + col0 + 4 * p;
    const ws16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ws16x4 __attribute__((address_space(3)))*)p0);
    const ws16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ws16x4 __attribute__((address_space(3)))*)(p0 + 16 * WLD));
    const qu32x2 l2 = __builtin_bit_cast(qu32x2, lo), h2 = __builtin_bit_cast(qu32x2, hi);
    return (qu32x4){l2.x, l2.y, h2.x, h2.y};
}

// ldx, ldy multiples of 4, x and dy 16-byte aligned, a slice's byte offsets and stream positions below 2^31 (host-checked)
template <int KW>
__global__ __launch_bounds__(WTHREADS) void conv_wgrad_bf16_kernel(WgradBf16Args g) {
    __shared__ __attribute__((aligned(16))) unsigned short sX[2][WXR * WLD];
    __shared__ __attribute__((aligned(16))) unsigned short sD[2][WKB * WLD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g4 = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;          // 4 x 2 waves: channels 32 * wm, outputs 64 * wn
    const int ctile = blockIdx.y / g.kh, ti = blockIdx.y - ctile * g.kh;      // kernel row i of this workgroup
    const int c0 = ctile * WT, n0 = blockIdx.x * WT;
    const int m_beg = blockIdx.z * g.maps_per_split;
    const int m_end = min(g.maps, m_beg + g.maps_per_split);
    const unsigned r_end = (unsigned)(m_end - m_beg) * g.per_map;            // stream positions of this slice
    const int dyo = ti - (g.kh - 1) / 2, pw = (g.kw - 1) / 2;
    // staging: thread = (row tid >> 5 (+ 16 i), 4 columns (tid & 31) * 4)
    const int srow = tid >> 5, scol = (tid & 31) * 4;
    // a quad that straddles C / N is loaded whole (the strides are multiples of 4 and hold it) and its tail zeroed in store_stage
    const bool xcol_ok = c0 + scol < g.C, dcol_ok = n0 + scol < g.N;
    const int xkeep = g.C - (c0 + scol), dkeep = g.N - (n0 + scol);           // elements of this thread's quads inside C / N
    // Each slice addresses its maps from ITS OWN 64-bit base: only a slice has to stay below 2 GiB (the host sizes the slices).
    const size_t slice_px = (size_t)m_beg * g.H * g.W;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.x + slice_px * g.ldx), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.dy + slice_px * g.ldy), 0, 0x7fffffff, 0x00020000);
    const unsigned xcol4 = (unsigned)(c0 + scol) * 4u, dcol4 = (unsigned)(n0 + scol) * 4u;
    const unsigned H = (unsigned)g.H, W = (unsigned)g.W, PW = (unsigned)g.PW;
    qu32x4 rx[3], rd[2];
    // Every load is unconditional (gemm_bf16.hip): positions past the slice, pad positions and pixels outside the image present
    // an out-of-range offset and read as zeros.
    auto load_stage = [&](unsigned r0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const unsigned r = r0 + (unsigned)(srow + 16 * i);
            unsigned mrow, t, m, y;
            wg_divmod(r, PW, g.pw_magic, mrow, t);
            wg_divmod(mrow, H, g.h_magic, m, y);
            const bool in = r < r_end && srow + 16 * i < WKB + KW - 1;      // (rows of the x image no tap reads are not fetched)
            const unsigned map_px = m * H * W;
            const int iy = (int)y + dyo, ix = (int)t - pw;
            const bool xok = in && xcol_ok && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            const unsigned xoff = (map_px + (unsigned)iy * W + (unsigned)ix) * g.ldx * 4u + xcol4;
            rx[i] = __builtin_amdgcn_raw_buffer_load_b128(xrs, xok ? xoff : W_OOR, 0, 0);
            if (i < 2) {
                const bool dok = in && dcol_ok && t < W;
                const unsigned doff = (map_px + y * W + t) * g.ldy * 4u + dcol4;
                rd[i] = __builtin_amdgcn_raw_buffer_load_b128(drs, dok ? doff : W_OOR, 0, 0);
            }
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int e = 1; e < 4; ++e) {
#pragma unroll
            for (int i = 0; i < 3; ++i) rx[i][e] = e < xkeep ? rx[i][e] : 0u;
#pragma unroll
            for (int i = 0; i < 2; ++i) rd[i][e] = e < dkeep ? rd[i][e] : 0u;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
            *(qu32x2*)(sX[buf] + (srow + 16 * i) * WLD + scol) =
                (qu32x2){pack_bf16(__uint_as_float(rx[i][0]), __uint_as_float(rx[i][1])), pack_bf16(__uint_as_float(rx[i][2]), __uint_as_float(rx[i][3]))};
#pragma unroll
        for (int i = 0; i < 2; ++i)
            *(qu32x2*)(sD[buf] + (srow + 16 * i) * WLD + scol) =
                (qu32x2){pack_bf16(__uint_as_float(rd[i][0]), __uint_as_float(rd[i][1])), pack_bf16(__uint_as_float(rd[i][2]), __uint_as_float(rd[i][3]))};
    };
    f32x4 acc[KW][2][4];
#pragma unroll
    for (int j = 0; j < KW; ++j)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[j][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const unsigned nstages = (r_end + WKB - 1) / WKB;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (unsigned s = 0; s < nstages; ++s) {
        const int buf = (int)(s & 1);
        load_stage((s + 1) * WKB);          // the next stage travels under the MFMAs (past the slice: zeros)
        qu32x4 bf[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) bf[b] = wg_frag(sD[buf], g4, n, wn * 64 + b * 16);
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            qu32x4 af[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = wg_frag(sX[buf] + j * WLD, g4, n, wm * 32 + a * 16);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) qmfma(acc[j][a][b], af[a], bf[b]);
        }
        store_stage(buf ^ 1);
        __syncthreads();
    }
    // ---- partial slice: out[z][tap][c][n]; D fragment: rows 4 g4 + r, column n ----
    float* out = g.out + (size_t)blockIdx.z * g.kh * g.kw * g.C * g.N;
#pragma unroll
    for (int j = 0; j < KW; ++j) {
        float* ot = out + (size_t)(ti * g.kw + j) * g.C * g.N;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = n0 + wn * 64 + b * 16 + n;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = c0 + wm * 32 + a * 16 + 4 * g4 + r;
                    if (row < g.C && col < g.N) ot[(size_t)row * g.N + col] = acc[j][a][b][r];
                }
            }
    }
}

// Every other shape: thread = (tap, c, n) of the slice's partial, pixels of the slice's maps one after the other.
__global__ __launch_bounds__(256) void conv_wgrad_plain_bf16_kernel(WgradBf16Args g) {
    const int tn = threadIdx.x & 15, tc = threadIdx.x >> 4;
    const int ctiles = (g.C + 15) / 16;
    const int tap = blockIdx.y / ctiles, ct = blockIdx.y - tap * ctiles;
    const int c = ct * 16 + tc, nn = blockIdx.x * 16 + tn;
    if (c >= g.C || nn >= g.N) return;
    const int ti = tap / g.kw, tj = tap - ti * g.kw;
    const int dyo = ti - (g.kh - 1) / 2, dxo = tj - (g.kw - 1) / 2;
    const int m_beg = blockIdx.z * g.maps_per_split;
    const int m_end = min(g.maps, m_beg + g.maps_per_split);
    const int y_lo = max(0, -dyo), y_hi = min(g.H, g.H - dyo), x_lo = max(0, -dxo), x_hi = min(g.W, g.W - dxo);
    float acc = 0.f;
    for (int m = m_beg; m < m_end; ++m) {
        const size_t map_px = (size_t)m * g.H * g.W;
        for (int y = y_lo; y < y_hi; ++y)
            for (int xx = x_lo; xx < x_hi; ++xx) {
                const float xv = g.x[(map_px + (size_t)(y + dyo) * g.W + (xx + dxo)) * g.ldx + c];
                const float dv = g.dy[(map_px + (size_t)y * g.W + xx) * g.ldy + nn];
                acc = fmaf(bf16_to_f32(bf16_bits(xv)), bf16_to_f32(bf16_bits(dv)), acc);
            }
    }
    g.out[((size_t)blockIdx.z * g.kh * g.kw + tap) * g.C * g.N + (size_t)c * g.N + nn] = acc;
}

unsigned magic_of(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)((1ull << 32) / d); }

bool wgrad_bf16_tiles_take(const float* x, long ldx, const float* dy, long ldy, int H, int W, int C, int N, int kw) {
    if (env_knobs().no_wgrad_bf16_tiles) return false;
    // whole 16-byte quads: strides that are multiples of 4 (a ragged C / N is masked in the staging: the stride holds the quad)
    if ((ldx & 3) || (ldy & 3) || (((uintptr_t)x) & 15) || (((uintptr_t)dy) & 15)) return false;
    if (kw != 1 && kw != 3 && kw != 5) return false;      // kw = 7 would be 224 accumulator registers
    return H * W > 1;
}

// map slices of a product of `tiles` workgroups per slice (one workgroup per CU at a time): the largest count up to 32 and B whose
// last round of workgroups leaves at most a tenth of the chip idle, else the one that leaves the least
int wgrad_bf16_split(long tiles, int B, long min_split, long max_split) {
    const long cus = device_cu_count();
    long smax = B < 32 ? B : 32;
    if (smax > max_split) smax = max_split;
    if (smax < min_split) smax = min_split;
    int best = (int)min_split;
    double best_e = 0.;
    for (long s = min_split; s <= smax; ++s) {
        const long wg = tiles * s;
        const double e = (double)wg / (double)((wg + cus - 1) / cus * cus);
        if (e >= 0.9 || e > best_e) { best = (int)s; best_e = e >= 0.9 ? 2. : e; }
    }
    return best;
}

}  // namespace

size_t conv2d_wgrad_bf16_workspace_floats(int C, int N, int kh, int kw) {
    // up to 32 slices of partials within 128 MB, eight where that is more (the head's 512 -> 1024: 52 MB each - its 6.8 GB dy
    // at B 256 needs four slices for the 2 GiB a slice may span, six fill the chip)
    const size_t wn = (size_t)kh * kw * C * N;
    size_t cap = 32 * wn;
    if (cap > ((size_t)32 << 20)) cap = (size_t)32 << 20;
    return (8 * wn > cap ? 8 * wn : cap) + 64;
}

int conv2d_wgrad_bf16(const float* x, long ldx, const float* dy, long ldy, float* dw, int B, int H, int W, int C, int N, int kh, int kw,
                      int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    const long P = (long)B * H * W;
    const size_t wn = (size_t)kh * kw * C * N;
    if (P == 0) return accumulate ? FOV_OK : zero_grad(dw, wn, stream);
    const long PW = (long)W + kw - 1;
    if (scratch_floats < conv2d_wgrad_bf16_workspace_floats(C, N, kh, kw)) { set_error("conv2d_wgrad_bf16: workspace too small"); return FOV_ERR_WORKSPACE; }
    WgradBf16Args g = {};
    g.x = x; g.dy = dy; g.ldx = (unsigned)ldx; g.ldy = (unsigned)ldy; g.C = C; g.N = N; g.H = H; g.W = W; g.kh = kh; g.kw = kw;
    g.PW = (int)PW; g.per_map = (unsigned)(H * PW); g.pw_magic = magic_of((unsigned)PW); g.h_magic = magic_of((unsigned)H);
    g.maps = B;
    const bool tiled = wgrad_bf16_tiles_take(x, ldx, dy, ldy, H, W, C, N, kw);
    const int gn = tiled ? (N + WT - 1) / WT : (N + 15) / 16;
    const int gy = tiled ? ((C + WT - 1) / WT) * kh : ((C + 15) / 16) * kh * kw;
    if (gy > 65535) { set_error("conv2d_wgrad_bf16: too many channel tiles"); return FOV_ERR_UNSUPPORTED; }
    // The tuned kernel forms 32-bit byte offsets from the base of a SLICE: the maps a slice may hold, and from that the fewest
    // slices.  (The trainer's one product over all steps is 2 560 maps, 6.8 GB of dy at 512 -> 1024: four slices at least.)
    long min_split = 1;
    if (tiled) {
        const long map_bytes = (long)H * W * (ldx > ldy ? ldx : ldy) * 4, map_pos = (long)H * PW;
        long fit = ((1L << 31) - 4 * (long)(C > N ? C : N) - 64) / map_bytes;
        const long fit_pos = ((1L << 31) - 4 * WKB) / map_pos;
        if (fit > fit_pos) fit = fit_pos;
        if (fit < 1) { set_error("conv2d_wgrad_bf16: operand larger than 2 GiB (one map)"); return FOV_ERR_UNSUPPORTED; }
        min_split = (B + fit - 1) / fit;
    }
    const long max_split = (long)((scratch_floats - 64) / wn);
    if (min_split > max_split || min_split > 65535) {
        set_error("conv2d_wgrad_bf16: operand larger than 2 GiB (%ld slices of at most 2 GiB needed, the workspace holds %ld)", min_split, max_split);
        return FOV_ERR_UNSUPPORTED;
    }
    int split = wgrad_bf16_split((long)gn * gy, B, min_split, max_split);
    g.maps_per_split = (B + split - 1) / split;
    split = (B + g.maps_per_split - 1) / g.maps_per_split;
    if (env_knobs().dbg_trace)
        fprintf(stderr, "[fov trace] conv2d_wgrad_bf16: %s form, %d slices of %d maps\n", tiled ? "tuned" : "plain", split, g.maps_per_split);
    // the slices go through the reduce whenever there is more than one or dw is added to; into the open deferred region's
    // arena when dw lies in one (same kernel, same slices, same reduce order: bit-identical)
    const bool via_scratch = split > 1 || accumulate;
    bool deferred = false;
    if (via_scratch) {
        if (float* arena = defer_alloc(dw, wn, (size_t)split * wn, stream)) { scratch = arena; deferred = true; }
    } else if (int rc = defer_touch(dw, wn, stream)) {
        return rc;
    }
    g.out = via_scratch ? scratch : dw;
    const dim3 grid((unsigned)gn, (unsigned)gy, (unsigned)split);
    if (tiled) {
        if (kw == 1) hipLaunchKernelGGL(conv_wgrad_bf16_kernel<1>, grid, dim3(WTHREADS), 0, stream, g);
        else if (kw == 3) hipLaunchKernelGGL(conv_wgrad_bf16_kernel<3>, grid, dim3(WTHREADS), 0, stream, g);
        else hipLaunchKernelGGL(conv_wgrad_bf16_kernel<5>, grid, dim3(WTHREADS), 0, stream, g);
    } else {
        hipLaunchKernelGGL(conv_wgrad_plain_bf16_kernel, grid, dim3(256), 0, stream, g);
    }
    if (int rc = launch_check(tiled ? "conv_wgrad_bf16" : "conv_wgrad_plain_bf16")) return rc;
    if (!via_scratch) return FOV_OK;
    return reduce_or_defer(deferred, scratch, dw, (long)wn, split, accumulate, stream, "splitk_reduce");
}

}  // namespace fov
