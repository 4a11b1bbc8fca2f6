// ConvLSTM2D step with bf16 matrix-core operands: the bf16 twin of convlstm_patch.hip (the six cell layers of
// mycode/convlstm_seq2seq.py:100-126,146-165 at inference).
//
//     z = conv_same(bf16([x_t | h_prev]), bf16([K ; R])) + b
//     i,f,o = recurrent_activation(z_i, z_f, z_o);  g = tanh(z_c);  c_new = f * c_prev + i * g;  h = o * tanh(c_new)
// both operands of every product rounded to bf16 round-to-nearest-even (pack_bf16 = v_cvt_pk_bf16_f32), products accumulated in
// fp32 (v_mfma_f32_16x16x32_bf16), bias, gates and cell update in fp32 with the library's rec_act / tanh_f; c_new, h and the
// gates tape stored fp32.  h is rounded only here, where a product takes it as an operand.
//
// Weights are PACKED ONCE (convlstm_cell_pack_bf16_kernel) into bf16 in B-fragment order with the gate columns interleaved the
// way the fp32 kernel's `bvoff` interleaves them for F = 32: fragment (tap, k-block kb of 32 input channels, column tile ct) is
// 64 lanes x 16 bytes = 1 KB; lane (li, lq) holds rows 32 kb + 8 lq + 0..7 of the column
//     gate (16 (ct % 2) + li) / 8  of unit  8 (ct / 2) + li % 8,
// i.e. a pair of column tiles is 8 units x 4 gates: tile 0 = [i | f], tile 1 = [g | o], and after one row_ror:8 the lanes
// li < 8 hold all four gates of their unit.  Rows past C + F and units past F are zero.  Both kernel forms read that buffer.
//
// convlstm_cell_patch_bf16_kernel keeps from the fp32 kernel: the halo patch of [x | h_prev] staged once per workgroup, every
// tap the same patch read at a shifted address, one barrier (behind the staging) and none after it, the epilogue.  What the
// operand type changes:
//   * the patch is staged as bf16 (fp32 buffer loads of a channel quad, pack_bf16 at the 8-byte LDS write - with C = 12 the
//     x | h boundary lies inside a 16-byte slot, which 8-byte writes do not care about): half the bytes, so a workgroup owns
//     TWICE the pixels (14 row tiles: 12 rows of an 18-wide map, patch 55 KB at 64 channels, two workgroups per CU) - a
//     smaller halo share and half the weight re-reads per pixel;
//   * a k-step is 32 channels: one ds_read_b128 per lane is the whole A fragment of (row tile, tap, k-block);
//   * pixel stride S = 32 NKB + 16 bf16 = 160 bytes (NKB = 2) or 96 bytes (NKB = 1), i.e. 10 or 6 sixteen-byte slots, s = 2 x odd.
//     A ds_read_b128 is served 16 lanes per cycle, and each of its four lane groups holds every li once, eight of them with
//     lq = 2m and eight (li + 8 of the others, mod 16 the complementary set) with lq = 2m + 1.  Lane (li, lq) reads slot
//     li * s + lq (+ a constant) of the 16 slots of a 256-byte bank row: the eight even-lq lanes have li = 0..7 mod 8, so
//     li * s = 2 * (odd * li mod 8) runs through all eight EVEN slots, the eight odd-lq lanes through all eight ODD slots -
//     sixteen distinct slots.  (A row tile that wraps to the next image row shifts part of its lanes by kw - 1 pixels, an
//     even number of slots: those tiles can pay a two-way conflict, as in the fp32 kernel.)
//   * every wave owns 8 units x 4 gates = two column tiles per A read whatever F is (F = 32: four waves side by side, all 14
//     row tiles each; F = 16: 2 x 2 waves, 7 row tiles; F = 8: four waves of 4 row tiles): an A fragment feeds two MFMAs, so
//     the LDS delivers 1 KB per 32 MFMA cycles and SIMD - half of its 256 B/clk/CU;
//   * weights arrive in fragment order straight from the packed buffer (L2), one 16-byte load per lane and fragment, a tap
//     ahead: 2 KB per wave and 28 (14) MFMAs - under 20 B/clk/CU, a quarter of what the fp32 kernel's tiling would ask for.
// convlstm_cell_plain_bf16_kernel takes every other shape (any F, C not a multiple of 4, C + F > 64, unaligned or oddly strided
// views, 1 x 1 maps, and everything under FOV_NO_CELL_PATCH=1): one wave per 16 pixels x 8 units, A gathered from global
// memory, no LDS; not tuned.
#include "bf16_common.h"

namespace fov {

namespace {

struct CellBf16Args {
    const float* x;        // (B,H,W,*) pixel stride ldx, batch stride ldb, C channels
    const float* h_prev;   // (B,H,W,*) or NULL (zero state: the packed weights then hold K alone)
    const void* wp;        // packed bf16 weights: [tap][kb][ct][lane 64][8]
    const float* bias;     // (4F) or NULL
    const float* c_prev;   // (B*H*W, F) or NULL
    float* c_new;
    float* h;              // pixel stride ldh
    float* gates;          // (B*H*W, 4F) or NULL
    long ldx, ldb, ldx2, ldb2, ldh;
    int B, H, W, C, C2, F, kh, kw;
    int rows;              // image rows per workgroup
    int groups;            // workgroups per map = ceil(H / rows)
    int nkb, ntl;          // k-blocks of 32 input channels, 16-column tiles of the packed buffer
};

constexpr int QMT = 14;     // MFMA row tiles (16 pixels) per workgroup: rows * W <= 224
constexpr int QUW = 8;      // units per wave (x 4 gates = two column tiles)
constexpr int QAHEAD = 4;   // row tiles between an A fragment's LDS read and its MFMAs

__host__ __device__ inline int cq_nkb(int Ctot) { return (Ctot + 31) / 32; }
__host__ __device__ inline int cq_ntl(int F) { return 2 * ((F + QUW - 1) / QUW); }

// bias, row_ror:8, gates, cell update and stores of one accumulator row: lanes li < 8 own (pixel m, unit)
template <int ACT>
__device__ __forceinline__ void cell_epilogue(const CellBf16Args& g, float z0, float z1, bool store, long m, int unit) {
    const float zf = qswap(z0), zo = qswap(z1);     // (i, g) in lanes 0-7, (f, o) in lanes 8-15
    if (store) {
        const int F = g.F;
        const float gi = rec_act<ACT>(z0), gf = rec_act<ACT>(zf), gg = tanh_f(z1), go = rec_act<ACT>(zo);
        const float cn = fmaf(gf, g.c_prev ? g.c_prev[m * F + unit] : 0.f, gi * gg);
        g.c_new[m * F + unit] = cn;
        g.h[m * g.ldh + unit] = go * tanh_f(cn);
        if (g.gates) {
            float* gp = g.gates + m * 4 * F + unit;
            gp[0] = gi; gp[F] = gf; gp[2 * F] = gg; gp[3 * F] = go;
        }
    }
}

template <int WAVES_N, int NKB, int ACT>
__global__ __launch_bounds__(256, 2) void convlstm_cell_patch_bf16_kernel(CellBf16Args g) {
    constexpr int WAVES_M = 4 / WAVES_N;
    constexpr int MTW = (QMT + WAVES_M - 1) / WAVES_M;   // row tiles per wave: 14 | 7 | 4
    constexpr int AH = MTW < QAHEAD ? MTW : QAHEAD;
    constexpr int PS = 32 * NKB + 16;                    // pixel stride in LDS, bf16 elements
    constexpr unsigned OOR = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned short qpatch[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lq = lane >> 4;
    const int b = blockIdx.x / g.groups, rg = blockIdx.x - b * g.groups;
    const int y0 = rg * g.rows;
    const int rows_here = g.H - y0 < g.rows ? g.H - y0 : g.rows;
    const int npix = rows_here * g.W;
    const int PW = g.W + g.kw - 1, PH = g.rows + g.kh - 1;
    const int ph = (g.kh - 1) / 2, pw = (g.kw - 1) / 2;
    const int F = g.F, Ctot = g.C + g.C2;

    // ---- stage the halo patch as bf16: [x | h_prev | zero channels up to 32 NKB] per patch pixel; outside the image: zeros ----
    {
        const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.x + (long)b * g.ldb), 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(g.h_prev ? g.h_prev + (long)b * g.ldb2 : nullptr), 0, g.h_prev ? 0x7fffffff : 0, 0x00020000);
        const int q1 = g.C >> 2, q2 = g.C2 >> 2, qz = (32 * NKB - Ctot) >> 2;
        const int npp = PH * PW;
        auto stage = [&](const __amdgpu_buffer_rsrc_t& rs, int nq, long ld, int ch0) {
            const int total = npp * nq;
#pragma unroll 4
            for (int e = tid; e < total; e += 256) {
                const int pp = e / nq, qd = e - pp * nq;
                const int py = pp / PW, px = pp - py * PW;
                const int iy = y0 - ph + py, ix = px - pw;
                const bool ok = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
                const unsigned off = ok ? (unsigned)((((long)iy * g.W + ix) * ld + 4 * qd) * 4) : OOR;
                const qu32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
                *(qu32x2*)&qpatch[pp * PS + ch0 + 4 * qd] = (qu32x2){pack_bf16(__uint_as_float(t[0]), __uint_as_float(t[1])),
                                                                     pack_bf16(__uint_as_float(t[2]), __uint_as_float(t[3]))};
            }
        };
        stage(xrs, q1, g.ldx, 0);
        if (q2 > 0) stage(hrs, q2, g.ldx2, g.C);
        if (qz > 0) {
            const int total = npp * qz;
            for (int e = tid; e < total; e += 256) {
                const int pp = e / qz, qd = e - pp * qz;
                *(qu32x2*)&qpatch[pp * PS + Ctot + 4 * qd] = (qu32x2){0u, 0u};
            }
        }
    }
    __syncthreads();

    const int wn = wave % WAVES_N, wm = wave / WAVES_N;
    const int unit0 = wn * QUW;
    // A: LDS element index of the window origin of this lane's pixel in each row tile (+ the lane group's 8 channels)
    int abase[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        int p = 16 * (wm * MTW + i) + li;
        p = p < npix ? p : npix - 1;   // pixels past the block: a valid address, results dropped
        const int y = p / g.W, x = p - y * g.W;
        abase[i] = (y * PW + x) * PS + 8 * lq;
    }
    // B: fragment (tap, kb, column tile 2 wn + j) of the packed buffer
    const int ntaps = g.kh * g.kw;
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.wp), 0, ntaps * g.nkb * g.ntl * 1024, 0x00020000);
    const unsigned bcol = (unsigned)((2 * wn) * 1024 + lane * 16);
    qu32x4 bw[NKB][2];
    auto load_b = [&](int tap, int kb) {
        const unsigned frag = (unsigned)((tap * g.nkb + kb) * g.ntl) * 1024u;
#pragma unroll
        for (int j = 0; j < 2; ++j) bw[kb][j] = __builtin_amdgcn_raw_buffer_load_b128(wrs, bcol + 1024u * j, frag, 0);
    };
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) load_b(0, kb);

    f32x4 acc[MTW][2];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int dy = 0, dx = 0;
    for (int tap = 0; tap < ntaps; ++tap) {
        const int coff = (dy * PW + dx) * PS;
        const int tap_n = tap + 1 < ntaps ? tap + 1 : tap;   // the last tap re-reads itself: no branch around loads
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const unsigned short* ap = qpatch + coff + 32 * kb;
            // AH row tiles ahead: the scheduling barriers keep every read that far in front of the MFMAs that consume it
            qu32x4 a[AH];
#pragma unroll
            for (int i = 0; i < AH; ++i) a[i] = *(const qu32x4*)(ap + abase[i]);
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
                qu32x4 an = a[i % AH];
                if (i + AH < MTW) an = *(const qu32x4*)(ap + abase[i + AH]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 2; ++j) qmfma(acc[i][j], a[i % AH], bw[kb][j]);
                __builtin_amdgcn_sched_barrier(0);
                a[i % AH] = an;
            }
            load_b(tap_n, kb);   // the registers just read: the next tap's weights have a whole tap to arrive
        }
        if (++dx == g.kw) { dx = 0; ++dy; }
    }

    // ---- epilogue: gates and cell update, lane-local after the gates of a unit have met ----
    const int unit = unit0 + (li & 7);
    const bool mine = li < 8;
    const int c0 = li < 8 ? unit : F + unit, c1 = c0 + 2 * F;       // this lane's two gate columns: (i | f), (g | o)
    const float bz0 = g.bias ? g.bias[c0] : 0.f, bz1 = g.bias ? g.bias[c1] : 0.f;
    const long mbase = ((long)b * g.H + y0) * g.W;
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = 16 * (wm * MTW + i) + 4 * lq + r;
            cell_epilogue<ACT>(g, acc[i][0][r] + bz0, acc[i][1][r] + bz1, mine && p < npix, mbase + p, unit);
        }
}

// Every other shape: a wave owns 16 consecutive pixels of the (B*H*W) row space and 8 units (two column tiles); per (tap,
// k-block) a lane gathers its 8 channels of [x | h_prev] at its pixel from global memory (zeros outside the image and beyond
// C + F), rounds them and multiplies.
template <int ACT>
__global__ __launch_bounds__(256) void convlstm_cell_plain_bf16_kernel(CellBf16Args g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.y * 4 + wave;         // unit group
    if (2 * ug >= g.ntl) return;                  // wave-uniform
    const int npix = g.H * g.W;
    const long M = (long)g.B * npix;
    const long m0 = (long)blockIdx.x * 16;
    const long m = m0 + li;
    const bool mok = m < M;
    const long bi = mok ? m / npix : 0;
    const int p = mok ? (int)(m - bi * npix) : 0;
    const int oy = p / g.W, ox = p - oy * g.W;
    const int ph = (g.kh - 1) / 2, pw = (g.kw - 1) / 2;
    const int F = g.F, Ctot = g.C + g.C2;
    const float* xb = g.x + bi * g.ldb;
    const float* hb = g.h_prev ? g.h_prev + bi * g.ldb2 : nullptr;
    const qu32x4* wp = (const qu32x4*)g.wp;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int dy = 0; dy < g.kh; ++dy)
        for (int dx = 0; dx < g.kw; ++dx) {
            const int iy = oy + dy - ph, ix = ox + dx - pw;
            const bool ok = mok && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            const long pix = ok ? (long)iy * g.W + ix : 0;
            const float* xp = xb + pix * g.ldx;
            const float* hp = hb ? hb + pix * g.ldx2 : nullptr;
            const long frag = ((long)(dy * g.kw + dx) * g.nkb) * g.ntl;
            for (int kb = 0; kb < g.nkb; ++kb) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 32 * kb + 8 * lq + j;
                    v[j] = !ok || c >= Ctot ? 0.f : (c < g.C ? xp[c] : hp[c - g.C]);
                }
                const qu32x4 a = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
                const qu32x4* bq = wp + (frag + (long)kb * g.ntl + 2 * ug) * 64 + lane;
                qmfma(acc[0], a, bq[0]);
                qmfma(acc[1], a, bq[64]);
            }
        }
    const int unit = QUW * ug + (li & 7);
    const bool mine = li < 8 && unit < F;
    const int c0 = li < 8 ? unit : F + unit, c1 = c0 + 2 * F;
    const float bz0 = g.bias && unit < F ? g.bias[c0] : 0.f, bz1 = g.bias && unit < F ? g.bias[c1] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long mm = m0 + 4 * lq + r;
        cell_epilogue<ACT>(g, acc[0][r] + bz0, acc[1][r] + bz1, mine && mm < M, mm, unit);
    }
}

// one thread per (fragment, lane): its 8 bf16 of the packed buffer
__global__ __launch_bounds__(256) void convlstm_cell_pack_bf16_kernel(const float* __restrict__ w, qu32x4* __restrict__ out, int Ctot,
                                                                      int F, int nkb, int ntl, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    const long f = idx >> 6;
    const int ct = (int)(f % ntl);
    const long f2 = f / ntl;
    const int kb = (int)(f2 % nkb);
    const long tap = f2 / nkb;
    const int q = 16 * (ct & 1) + (lane & 15);
    const int unit = QUW * (ct >> 1) + (q & 7), gate = q >> 3;
    const int k0 = 32 * kb + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (unit < F && k0 + j < Ctot) ? w[(tap * Ctot + k0 + j) * (4L * F) + gate * F + unit] : 0.f;
    out[idx] = (qu32x4){pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
}

size_t cell_patch_bf16_lds(int rows, int W, int kh, int kw, int nkb) {
    return sizeof(unsigned short) * (size_t)(rows + kh - 1) * (W + kw - 1) * (32 * nkb + 16);
}

int cell_patch_bf16_rows(int H, int W) {
    const int rows = (16 * QMT) / W;
    return rows > H ? H : rows;
}

// Shapes the patch form takes: those of the fp32 patch form (cell_patch_shape_ok) - F in {8, 16, 32}, C a multiple of four,
// at most 64 input channels per tap, 16-byte aligned channel vectors, maps at most 112 pixels wide - whose bf16 patch fits
// half of the LDS.
bool cell_patch_bf16_shape_ok(const float* x, long ldx, long ldb, int C, const float* h_prev, long ldx2, long ldb2, int F, int H, int W,
                              int kh, int kw) {
    if (env_knobs().no_cell_patch) return false;
    if (!(F == 8 || F == 16 || F == 32)) return false;
    const int Ctot = C + (h_prev ? F : 0);
    if (C <= 0 || (C & 3) || Ctot > 64) return false;
    if ((ldx & 3) || (ldb & 3) || (((uintptr_t)x) & 15)) return false;
    if (h_prev && ((ldx2 & 3) || (ldb2 & 3) || (((uintptr_t)h_prev) & 15))) return false;
    if (W < 1 || W > 112 || kh < 1 || kw < 1 || kh * kw > 64) return false;
    return cell_patch_bf16_lds(cell_patch_bf16_rows(H, W), W, kh, kw, cq_nkb(Ctot)) <= 80 * 1024;
}

template <int WAVES_N, int NKB>
int launch_patch_bf16_t(const CellBf16Args& g, int act, size_t lds, hipStream_t stream) {
    void (*kern)(CellBf16Args) = act == FOV_ACT_HARD_SIGMOID ? convlstm_cell_patch_bf16_kernel<WAVES_N, NKB, FOV_ACT_HARD_SIGMOID>
                                                             : convlstm_cell_patch_bf16_kernel<WAVES_N, NKB, FOV_ACT_SIGMOID>;
    int rc = ensure_dynamic_lds((const void*)kern, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(g.B * g.groups)), dim3(256), lds, stream, g);
    return launch_check("convlstm_cell_patch_bf16");
}

}  // namespace

size_t convlstm_cell_bf16_packed_bytes(int Ctot, int F, int kh, int kw) { return (size_t)kh * kw * cq_nkb(Ctot) * cq_ntl(F) * 1024; }

int convlstm_cell_pack_bf16(const float* w, void* packed, int Ctot, int F, int kh, int kw, hipStream_t stream) {
    const int nkb = cq_nkb(Ctot), ntl = cq_ntl(F);
    const long total = (long)kh * kw * nkb * ntl * 64;
    hipLaunchKernelGGL(convlstm_cell_pack_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, (qu32x4*)packed,
                       Ctot, F, nkb, ntl, total);
    return launch_check("convlstm_cell_pack_bf16");
}

// One ConvLSTM2D step on packed bf16 weights; the aliasing rules of convlstm_cell_fwd.
int convlstm_cell_fwd_bf16(const float* x, long ldx, long ldb, int C, const float* h_prev, long ldx2, long ldb2, const void* w_packed,
                           const float* bias, const float* c_prev, float* c_new, float* h, long ldh, float* gates, int B, int H, int W,
                           int F, int kh, int kw, int act, hipStream_t stream) {
    const long M = (long)B * H * W;
    if (M == 0 || F == 0) return FOV_OK;
    const int Ctot = C + (h_prev ? F : 0);
    // The plain kernel addresses with 64-bit pointers and would not need the 31-bit limit; it is applied to both forms on
    // purpose, so that what a call accepts does not depend on the form that runs it.
    if (!operand_fits_31bit("convlstm_cell_bf16", B, ldb, h_prev, ldb2, (long)convlstm_cell_bf16_packed_bytes(Ctot, F, kh, kw), (M + 15) / 16))
        return FOV_ERR_UNSUPPORTED;
    CellBf16Args g = {};
    g.x = x; g.h_prev = h_prev; g.wp = w_packed; g.bias = bias; g.c_prev = c_prev; g.c_new = c_new; g.h = h; g.gates = gates;
    g.ldx = ldx; g.ldb = ldb; g.ldx2 = ldx2; g.ldb2 = ldb2; g.ldh = ldh;
    g.B = B; g.H = H; g.W = W; g.C = C; g.C2 = h_prev ? F : 0; g.F = F; g.kh = kh; g.kw = kw;
    g.nkb = cq_nkb(Ctot); g.ntl = cq_ntl(F);
    if (cell_patch_bf16_shape_ok(x, ldx, ldb, C, h_prev, ldx2, ldb2, F, H, W, kh, kw)) {
        g.rows = cell_patch_bf16_rows(H, W);
        g.groups = (H + g.rows - 1) / g.rows;
        const size_t lds = cell_patch_bf16_lds(g.rows, W, kh, kw, g.nkb);
#define FOV_PATCH_KB(WN_) return g.nkb == 1 ? launch_patch_bf16_t<WN_, 1>(g, act, lds, stream) : launch_patch_bf16_t<WN_, 2>(g, act, lds, stream)
        if (F == 32) FOV_PATCH_KB(4);
        if (F == 16) FOV_PATCH_KB(2);
        FOV_PATCH_KB(1);
#undef FOV_PATCH_KB
    }
    const dim3 grid((unsigned)((M + 15) / 16), (unsigned)((g.ntl / 2 + 3) / 4));
    if (act == FOV_ACT_HARD_SIGMOID) hipLaunchKernelGGL(convlstm_cell_plain_bf16_kernel<FOV_ACT_HARD_SIGMOID>, grid, dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(convlstm_cell_plain_bf16_kernel<FOV_ACT_SIGMOID>, grid, dim3(256), 0, stream, g);
    return launch_check("convlstm_cell_plain_bf16");
}

}  // namespace fov
