// 'same' Conv2D with bf16 matrix-core operands and fp32 accumulation: the bf16 twin of conv_patch.hip (the prediction head of
// mycode/convlstm_seq2seq.py:176-181,231-238 - Conv2D 56 -> 512 -> 1024 -> 30, k = 5, on 36 x 18 heat maps - at inference).
//
//     y = act(conv2d_same(bf16(x), bf16(w)) + b)
// both operands of every product rounded to bf16 round-to-nearest-even (pack_bf16 = v_cvt_pk_bf16_f32), products accumulated in
// fp32 (v_mfma_f32_16x16x32_bf16), bias and relu in fp32, y stored fp32.
//
// Weights are PACKED ONCE (conv2d_pack_bf16_kernel) into bf16 in B-fragment order: fragment (tap, k-block kb of 32 input
// channels, 16-column tile nt) is 64 lanes x 16 bytes = 1 KB, lane (li, lq) holding w[tap][32 kb + 8 lq + 0..7][16 nt + li];
// channels past C and columns past N are zero.  Both kernel forms read that one buffer with 16-byte loads.
//
// conv2d_patch_bf16_kernel (the map-resident form) keeps conv_patch.hip's ownership and geometry - a workgroup owns one MAP
// and BN output channels, a wave 32 columns for MTW row tiles, row tile i + 9 is row tile i moved down a whole number of image
// rows - with what the operand type changes:
//   * a slab is 32 channels = one MFMA k-step: the halo patch is staged as bf16 (fp32 loads a slab ahead into registers, in
//     chunks spread over the slab's taps; pack_bf16 at the LDS write), pixel stride 48 bf16 = 96 bytes = 6 sixteen-byte slots:
//     the sixteen lanes a ds_read_b128 serves per LDS cycle (all li, lq in {0,1} or {2,3}) fall on sixteen distinct slots;
//   * one ds_read_b128 per lane is the whole A fragment of a row tile and tap (8 channels of one pixel), read PB_AHEAD row
//     tiles in front of its two MFMAs;
//   * the B fragments of the (tap, slab) pair two ahead are two 16-byte loads per lane from the packed buffer (L2-resident).
// conv2d_plain_bf16_kernel takes every other shape (small maps, 1 x 30 Conv1D maps, unaligned or ragged-channel inputs, and
// everything under FOV_NO_CONV_PATCH=1): one wave per 16 pixels x 16 columns, A gathered from global memory, no LDS.
#include <stdlib.h>

#include "bf16_common.h"

namespace fov {

namespace {

struct ConvBf16Args {
    const float* x;        // (B,H,W,*) pixel stride ldx, batch stride ldb, C channels
    const void* wp;        // packed bf16 weights: [tap][kb][nt][lane 64][8]
    const float* bias;     // (N) or NULL
    float* y;              // (B*H*W, N)
    long ldx, ldb;
    int B, H, W, C, N, kh, kw, act;
    int per, rs;           // row tile i + per = row tile i moved down rs image rows
    int nkb, ntl;          // k-blocks of 32 input channels, 16-column tiles of the packed buffer
};

constexpr int PBK = 32;           // channels per slab = one MFMA k-step
constexpr int PBS = PBK + 16;     // pixel stride in LDS (bf16 elements): 96 bytes
constexpr int PB_MAXPER = 9;      // base addresses a lane keeps
constexpr int PB_SLACK_ROWS = 5;  // patch rows allocated below the halo: row tiles past the end of the map (up to tile 43 = pixel 703)
                                  // read there; their results are never stored
constexpr int PB_STAGE = 28;      // 16-byte fp32 vectors of the next slab per thread: 28 * 256 >= (40 * 22) * 8
constexpr int PB_CHUNK = 4;       // ... requested four at a time, a chunk every few taps of the slab in front
constexpr int PB_AHEAD = 6;       // row tiles between an A fragment's LDS read and its MFMAs (12 MFMAs = ~190 cycles)
constexpr int PB_MAXTILE = 44;    // row tiles a wave may address (4 waves x 11)

__host__ __device__ inline int pb_nkb(int C) { return (C + PBK - 1) / PBK; }
__host__ __device__ inline int pb_ntl(int N) { return (N + 15) / 16; }

template <int WAVES_N, int TSTEP>
__global__ __launch_bounds__(256, 1) void conv2d_patch_bf16_kernel(ConvBf16Args g) {
    constexpr int WAVES_M = 4 / WAVES_N;
    constexpr int MT = 41;                                  // row tiles of a map at most (656 pixels)
    constexpr int MTW = (MT + WAVES_M - 1) / WAVES_M;       // row tiles per wave: 21 | 11
    constexpr int NT = 2;                                   // 16-column tiles per wave
    constexpr int BN = 16 * NT * WAVES_N;
    constexpr unsigned OOR = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned short bpatch[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lq = lane >> 4;
    const int nb = blockIdx.x / g.B, b = blockIdx.x - nb * g.B;      // n-block major: neighbours share the weights
    const int PW = g.W + g.kw - 1, PH = g.H + g.kh - 1;
    const int ph = (g.kh - 1) / 2, pw = (g.kw - 1) / 2;
    const int npix = g.H * g.W, npp = PH * PW;
    const int N = g.N;
    const int wn = wave % WAVES_N, wm = wave / WAVES_N;
    const int n0 = nb * BN + wn * 16 * NT;
    const int nslab = g.nkb;
    const int ntaps = g.kh * g.kw;

    // ---- the slab loader: patch pixel pp, channel quad qd of the slab <- x[b][iy][ix][32 slab + 4 qd ..]; zeros outside the image
    // and beyond C (a multiple of four here).  Element e = tid + 256 v -> (pp = e / 8, qd = e % 8): the byte offsets do not depend
    // on the slab and are kept in LDS behind the patch, read back by the thread that wrote them.
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.x + (long)b * g.ldb), 0, 0x7fffffff, 0x00020000);
    unsigned* soff = (unsigned*)(bpatch + (size_t)(PH + PB_SLACK_ROWS) * PW * PBS);
#pragma unroll
    for (int v = 0; v < PB_STAGE; ++v) {
        const int e = tid + 256 * v, pp = e >> 3, qd = e & 7;
        const int py = pp / PW, px = pp - py * PW;
        const int iy = py - ph, ix = px - pw;
        const bool ok = pp < npp && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
        soff[e] = ok ? (unsigned)((((long)iy * g.W + ix) * g.ldx + 4 * qd) * 4) : OOR;
    }
    qu32x4 st[PB_STAGE];
    auto stage_load = [&](int slab, int chunk) {
        const int c0 = slab * PBK;
        const bool in = c0 + 4 * (tid & 7) < g.C;        // 256 v keeps e % 8: one quad index per thread
        asm volatile("" ::: "memory");                   // the offsets are read HERE, not hoisted in front of the taps (28 registers)
#pragma unroll
        for (int v = PB_CHUNK * chunk; v < PB_CHUNK * chunk + PB_CHUNK; ++v) {
            const unsigned so = soff[tid + 256 * v];
            st[v] = __builtin_amdgcn_raw_buffer_load_b128(xrs, in ? so : OOR, (unsigned)(c0 * 4), 0);
        }
    };
    constexpr int NCH = PB_STAGE / PB_CHUNK;
    auto stage_write = [&]() {
#pragma unroll
        for (int v = 0; v < PB_STAGE; ++v) {
            const int e = tid + 256 * v, pp = e >> 3, qd = e & 7;
            if (pp < npp)
                *(qu32x2*)&bpatch[pp * PBS + 4 * qd] =
                    (qu32x2){pack_bf16(__uint_as_float(st[v][0]), __uint_as_float(st[v][1])),
                             pack_bf16(__uint_as_float(st[v][2]), __uint_as_float(st[v][3]))};
        }
    };

    // A: LDS element index of the window origin of this lane's pixel in row tiles 0 .. per-1 of the wave (+ the lane group's 8 channels)
    int abase[PB_MAXPER];
    const int tile0 = wm * MTW;
#pragma unroll
    for (int i = 0; i < PB_MAXPER; ++i) {
        int p = 16 * (tile0 + i) + li;
        p = p < npix ? p : npix - 1;         // pixels past the map: a valid address, results dropped
        const int yy = p / g.W, xx = p - yy * g.W;
        abase[i] = (yy * PW + xx) * PBS + 8 * lq;
    }
    const int tile_step = TSTEP ? TSTEP : g.rs * PW * PBS;   // elements from row tile i to row tile i + per
    // B: fragment (tap, slab, column tile) of the packed buffer; a column tile past the buffer's last reads as zero
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.wp), 0, ntaps * g.nkb * g.ntl * 1024, 0x00020000);
    unsigned bcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bcol[j] = (n0 / 16 + j < g.ntl) ? (unsigned)((n0 / 16 + j) * 1024 + lane * 16) : OOR;
    // (tap, slab) pairs in the order the loops below visit them: pair q = slab * ntaps + tap; a pair past the last re-reads the last
    const int npairs = nslab * ntaps;
    qu32x4 bw[NT], bw1[NT], bw2[NT];
    auto load_b = [&](int q, qu32x4 (&dst)[NT]) {
        q = q < npairs ? q : npairs - 1;
        const int slab = q / ntaps, tap = q - slab * ntaps;
        const unsigned frag = (unsigned)((tap * g.nkb + slab) * g.ntl) * 1024u;
#pragma unroll
        for (int j = 0; j < NT; ++j) dst[j] = __builtin_amdgcn_raw_buffer_load_b128(wrs, bcol[j], frag, 0);
    };

    f32x4 acc[MTW][NT];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // row tiles this wave really has: the map's ceil(npix / 16) dealt MTW per wave - the last wave's share is shorter, and its
    // missing tiles are skipped as a whole (wave-uniform), not multiplied and dropped
    const int ntile_map = (npix + 15) >> 4;
    const int my_tiles = ntile_map - tile0 < MTW ? (ntile_map - tile0 > 0 ? ntile_map - tile0 : 0) : MTW;

    // The next slab is requested in NCH chunks, one every `cstride` taps (25 taps: every third): buffer loads return in order, so
    // a tap's wait for its weights also waits for every patch load requested in front of them - with a whole slab requested at once
    // the first taps of every slab waited for its 112 KB.  The weights are requested two pairs ahead: those behind a chunk have
    // two taps for both to arrive (512 -> 1024 at B 256: 4.60 -> 4.30 ms).
    const int cstride = ntaps / (NCH + 1) > 0 ? ntaps / (NCH + 1) : 1;
#pragma unroll
    for (int k = 0; k < NCH; ++k) stage_load(0, k);
    load_b(0, bw);
    load_b(1, bw1);
    stage_write();
    __syncthreads();
    for (int slab = 0; slab < nslab; ++slab) {
        const bool more = slab + 1 < nslab;
        int dy = 0, dx = 0;
        auto tap_body = [&](int tap) {
            load_b(slab * ntaps + tap + 2, bw2);
            const int coff = (dy * PW + dx) * PBS;
            const unsigned short* ab[PB_MAXPER];     // the tap's shift goes into the nine base addresses once, not into every read
#pragma unroll
            for (int r = 0; r < PB_MAXPER; ++r) ab[r] = bpatch + abase[r] + coff;
            auto read_a = [&](int i) { return *(const qu32x4*)(ab[i % PB_MAXPER] + (i / PB_MAXPER) * tile_step); };
            // PB_AHEAD row tiles ahead: the scheduling barriers keep every read that far in front of the MFMAs that consume it (left
            // alone, hipcc sinks the reads to just in front of their first use and the wave, alone on its SIMD, sits out the latency)
            qu32x4 a[PB_AHEAD];
#pragma unroll
            for (int i = 0; i < PB_AHEAD; ++i) a[i] = read_a(i < MTW ? i : 0);
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
                qu32x4 an = a[i % PB_AHEAD];
                if (i + PB_AHEAD < MTW) an = read_a(i + PB_AHEAD);
                __builtin_amdgcn_sched_barrier(0);
                // a tile past the wave's share (wave-uniform; only trailing tiles can be missing) is skipped
                if (i < MTW - 3 || i < my_tiles) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) qmfma(acc[i][j], a[i % PB_AHEAD], bw[j]);
                }
                __builtin_amdgcn_sched_barrier(0);
                a[i % PB_AHEAD] = an;
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) { bw[j] = bw1[j]; bw1[j] = bw2[j]; }
            if (++dx == g.kw) { dx = 0; ++dy; }
        };
        // the taps in NCH + 1 runs, a chunk of the next slab requested in front of each of the first NCH (a kernel of fewer taps
        // than chunks has empty runs: their chunks are requested back to back)
#pragma unroll
        for (int k = 0; k <= NCH; ++k) {
            if (k < NCH && more) stage_load(slab + 1, k);
            const int t0 = k * cstride < ntaps ? k * cstride : ntaps;
            const int t1 = (k == NCH || (k + 1) * cstride > ntaps) ? ntaps : (k + 1) * cstride;
            for (int tap = t0; tap < t1; ++tap) tap_body(tap);
        }
        if (more) {
            __syncthreads();                     // every wave is done reading this slab
            stage_write();
            __syncthreads();
        }
    }

    // ---- epilogue: bias, activation; D fragment: rows 4 lq + r of the tile, column li ----
    const long mbase = (long)b * npix;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + 16 * j + li;
        if (col >= N) continue;
        const float bz = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = 16 * (tile0 + i) + 4 * lq + r;
                if (p < npix) {
                    const float v = acc[i][j][r] + bz;
                    g.y[(mbase + p) * N + col] = g.act == 2 ? fmaxf(v, 0.f) : v;
                }
            }
    }
}

// Every other shape: a wave owns 16 consecutive pixels of the (B*H*W) row space and one 16-column tile; per (tap, k-block) a lane
// gathers its 8 channels of its pixel from global memory (zeros outside the image and beyond C), rounds them and multiplies.
__global__ __launch_bounds__(256) void conv2d_plain_bf16_kernel(ConvBf16Args g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int nt = blockIdx.y * 4 + wave;
    if (nt >= g.ntl) return;                      // wave-uniform
    const int npix = g.H * g.W;
    const long M = (long)g.B * npix;
    const long m0 = (long)blockIdx.x * 16;
    const long m = m0 + li;
    const bool mok = m < M;
    const long bi = mok ? m / npix : 0;
    const int p = mok ? (int)(m - bi * npix) : 0;
    const int oy = p / g.W, ox = p - oy * g.W;
    const int ph = (g.kh - 1) / 2, pw = (g.kw - 1) / 2;
    const float* xb = g.x + bi * g.ldb;
    const qu32x4* wp = (const qu32x4*)g.wp;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < g.kh; ++dy)
        for (int dx = 0; dx < g.kw; ++dx) {
            const int iy = oy + dy - ph, ix = ox + dx - pw;
            const bool ok = mok && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            const float* xp = xb + (ok ? ((long)iy * g.W + ix) * g.ldx : 0);
            const long frag = ((long)(dy * g.kw + dx) * g.nkb) * g.ntl;
            for (int kb = 0; kb < g.nkb; ++kb) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = PBK * kb + 8 * lq + j;
                    v[j] = (ok && c < g.C) ? xp[c] : 0.f;
                }
                const qu32x4 a = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
                const qu32x4 bq = wp[(frag + (long)kb * g.ntl + nt) * 64 + lane];
                qmfma(acc, a, bq);
            }
        }
    const int col = 16 * nt + li;
    if (col >= g.N) return;
    const float bz = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long mm = m0 + 4 * lq + r;
        if (mm < M) {
            const float v = acc[r] + bz;
            g.y[mm * g.N + col] = g.act == 2 ? fmaxf(v, 0.f) : v;
        }
    }
}

// one thread per (fragment, lane): its 8 bf16 of the packed buffer
__global__ __launch_bounds__(256) void conv2d_pack_bf16_kernel(const float* __restrict__ w, qu32x4* __restrict__ out, int C, int N,
                                                               int nkb, int ntl, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    const long f = idx >> 6;
    const int nt = (int)(f % ntl);
    const long f2 = f / ntl;
    const int kb = (int)(f2 % nkb);
    const long tap = f2 / nkb;
    const int n = 16 * nt + (lane & 15), c0 = PBK * kb + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (n < N && c0 + j < C) ? w[(tap * C + c0 + j) * N + n] : 0.f;
    out[idx] = (qu32x4){pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
}

int gcd_b(int a, int b) { return b ? gcd_b(b, a % b) : a; }

size_t patch_bf16_lds(int H, int W, int kh, int kw) {
    return sizeof(unsigned short) * (size_t)(H + kh - 1 + PB_SLACK_ROWS) * (W + kw - 1) * PBS + sizeof(unsigned) * PB_STAGE * 256;
}

// Shapes the map-resident form takes: what conv_patch.hip takes (maps of at most 656 pixels, row tiles that repeat after nine,
// at least 32 input channels, 16-byte aligned pixels) with C a multiple of four, a map large enough that the farthest row tile a
// wave addresses (tile 43) still lies inside the patch's slack rows, and the slab's staging within PB_STAGE vectors per thread.
bool patch_bf16_shape_ok(const float* x, long ldx, long ldb, int B, int H, int W, int C, int N, int kh, int kw) {
    if (env_knobs().no_conv_patch) return false;
    if (H < 1 || W < 1 || H * W > 656 || C < 32 || (C & 3) || N < 1 || B < 1) return false;
    if ((ldx & 3) || (ldb & 3) || (((uintptr_t)x) & 15)) return false;
    if (kh < 1 || kw < 1 || !(kh & 1) || !(kw & 1) || kh * kw > 49) return false;
    if (W / gcd_b(16, W) != PB_MAXPER) return false;
    if ((H + PB_SLACK_ROWS) * W < 16 * PB_MAXTILE) return false;
    if (patch_bf16_lds(H, W, kh, kw) > 150 * 1024 || (size_t)(H + kh - 1) * (W + kw - 1) * 8 > (size_t)PB_STAGE * 256) return false;
    return true;
}

}  // namespace

size_t conv2d_bf16_packed_bytes(int C, int N, int kh, int kw) { return (size_t)kh * kw * pb_nkb(C) * pb_ntl(N) * 1024; }

int conv2d_pack_bf16(const float* w, void* packed, int C, int N, int kh, int kw, hipStream_t stream) {
    const int nkb = pb_nkb(C), ntl = pb_ntl(N);
    const long total = (long)kh * kw * nkb * ntl * 64;
    hipLaunchKernelGGL(conv2d_pack_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, (qu32x4*)packed, C, N,
                       nkb, ntl, total);
    return launch_check("conv2d_pack_bf16");
}

int conv2d_fwd_bf16(const float* x, long ldx, long ldb, const void* w_packed, const float* bias, float* y, int B, int H, int W, int C,
                    int N, int kh, int kw, int act, hipStream_t stream) {
    const long M = (long)B * H * W;
    if (M == 0 || N == 0) return FOV_OK;
    if (!operand_fits_31bit("conv2d_bf16", B, ldb, nullptr, 0, (long)conv2d_bf16_packed_bytes(C, N, kh, kw), (M + 15) / 16))
        return FOV_ERR_UNSUPPORTED;
    ConvBf16Args g = {};
    g.x = x; g.wp = w_packed; g.bias = bias; g.y = y; g.ldx = ldx; g.ldb = ldb;
    g.B = B; g.H = H; g.W = W; g.C = C; g.N = N; g.kh = kh; g.kw = kw; g.act = act;
    g.nkb = pb_nkb(C); g.ntl = pb_ntl(N);
    if (patch_bf16_shape_ok(x, ldx, ldb, B, H, W, C, N, kh, kw)) {
        g.per = W / gcd_b(16, W);
        g.rs = 16 * g.per / W;
        const size_t lds = patch_bf16_lds(H, W, kh, kw);
        void (*kern)(ConvBf16Args);
        int bn;
        const bool fixed = g.rs * (W + kw - 1) * PBS == 8448;      // the heat maps' geometry: immediate row-tile offsets
        if (N > 32) { kern = fixed ? conv2d_patch_bf16_kernel<2, 8448> : conv2d_patch_bf16_kernel<2, 0>; bn = 64; }
        else { kern = fixed ? conv2d_patch_bf16_kernel<1, 8448> : conv2d_patch_bf16_kernel<1, 0>; bn = 32; }
        const int nblocks = (N + bn - 1) / bn;
        int rc = ensure_dynamic_lds((const void*)kern, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)(nblocks * B)), dim3(256), lds, stream, g);
        return launch_check("conv2d_patch_bf16");
    }
    hipLaunchKernelGGL(conv2d_plain_bf16_kernel, dim3((unsigned)((M + 15) / 16), (unsigned)((g.ntl + 3) / 4)), dim3(256), 0, stream, g);
    return launch_check("conv2d_plain_bf16");
}

}  // namespace fov
