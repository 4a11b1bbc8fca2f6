// fp32 GEMM of the training step on the matrix cores (v_mfma_f32_16x16x4_f32): gemm_f32_kernel, LDS-tiled
// (32|64|96|128) x (64|128|256) x 16 with a two-level k and four operand staging modes, and gemm_f32, which picks the
// tile shape and the split-K slices (summed in a fixed order by reduce_defer.hip: deterministic, no float atomics).
// skinny_tn takes the A^T . B products with a side of <= 8 columns, which are HBM-bound and would be mostly padding
// on an MFMA tile.
#include "gemm_f32.h"

namespace fov {

constexpr int GBK = 16;
typedef unsigned gu32x4 __attribute__((ext_vector_type(4)));

// Block tile BM x BN x 16 with BM = 16*MI*WAVES_M, BN = 16*NI*(4/WAVES_M); each of the 4 waves owns
// MI x NI MFMA tiles.  Global->LDS staging goes through registers one k-tile ahead.
//
// fp32 MFMA shares the VALU issue slots, so staging arithmetic is paid for in MFMA time.  The k-tiles
// therefore never straddle a ko row: tile t <-> (ko = t / ntpr, kt = t % ntpr) with ntpr = ceil(KI/16),
// its k = ko*KI + kt*16 + kk.  The tile's base address is wave-uniform (SALU) and sits in a per-tile buffer
// descriptor; each thread adds a 32-bit offset fixed for the whole kernel; invalid elements present an
// out-of-range offset and the hardware returns 0 (<= 15 zero columns per ko row; KI = 29 wastes 9 % of the
// MFMAs and saves far more).
//
// Staging mode of an operand (template parameter, so the staged registers never meet at a control-flow
// merge - a merge makes the compiler wait for the loads before the MFMAs of the current tile):
//   0  k-slow ([k][row] storage, row index contiguous), 16-byte buffer loads, LDS [k][rows]
//   1  k-slow, 4-byte buffer loads (row stride or width not a multiple of 4), LDS [k][rows]
//   2  anything else: global loads, select at stash time, LDS [k][rows]
//   3  k-fast ([row][k] storage, k contiguous, KI % 4 == 0), 16-byte buffer loads along k, LDS [rows][k]
// The MFMA k-slot of lane group lq in step s is k = 4*lq + s (for A and B alike): an operand stored
// [rows][k] gives a lane its four steps with ONE ds_read_b128, an operand stored [k][rows] reads rows
// 4*lq + s (row stride = 4 mod 8 floats: the four lane groups land on disjoint banks).
// Fragments of a [k][rows] tile (round 3): a lane used to read its four k-steps of every 16-row MFMA tile with four
// ds_read_b32 each - 32 LDS instructions per k-tile at 4 x 4 tiles per wave.  The MFMA row <-> operand row assignment is
// free as long as the epilogue uses the same one, so: MFMA tile i, row q of a wave's NTW tiles is operand row
// 64*(i/4) + 4*q + (i%4) for tiles in complete groups of four (one ds_read_b128 at [k][4*li] serves four tiles) and
// 2*q + (i%2) for a trailing pair (ds_read_b64): 8 LDS instructions per k-tile, and a lane's four column tiles are four
// CONSECUTIVE output columns (16-byte stores).  Row stride: a multiple of 16 floats keeps the b128 lane groups on distinct
// 16-byte slots, == 8 (mod 16) the two halves of a b64 read on distinct banks.  Same products in the same order: results
// are bit-identical to the old mapping.
template <int ROWS, int MODE, int NTW>
struct OperandStage {
    static_assert(NTW % 2 == 0, "tiles per wave: complete groups of four plus at most one pair");
    static constexpr bool VEC = (MODE == 0 || MODE == 3);
    static constexpr bool TR = (MODE == 3);
    static constexpr int LD = TR ? 24 : ROWS + (NTW % 4 == 0 ? 0 : 8);
    static constexpr int LDS_FLOATS = TR ? ROWS * 24 : GBK * LD;   // one buffer
    static constexpr int R = VEC ? (ROWS * 4 + 255) / 256 : ROWS / 16;     // loads per thread per k-tile
    static constexpr unsigned OOR = 0x80000000u;
    int kk[R], rr[R];
    unsigned off[R];   // byte offset from the tile base (OOR when the row is outside the matrix)
    bool ok[R];
    float sc[VEC ? 1 : R];
    f32x4 vv[VEC ? R : 1];
    int kmax;          // valid k columns of the staged tile
    int ph[R];         // periodic-shift operands: (k row of this thread's element) % period

    __device__ __forceinline__ void init(int tid, int row0, int nrows, long s_row, long s_ki) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = tid + 256 * r;
            if (MODE == 0) { kk[r] = e / (ROWS / 4); rr[r] = 4 * (e - kk[r] * (ROWS / 4)); }
            else if (MODE == 3) { rr[r] = e >> 2; kk[r] = 4 * (e & 3); }
            else if (MODE == 2 && s_ki == 1) { rr[r] = e >> 4; kk[r] = e & 15; }   // consecutive threads walk k
            else { kk[r] = e / ROWS; rr[r] = e - kk[r] * ROWS; }
            ok[r] = rr[r] < ROWS && kk[r] < GBK && row0 + rr[r] < nrows;
            off[r] = ok[r] ? (unsigned)(((long)rr[r] * s_row + (long)kk[r] * s_ki) * 4) : OOR;
        }
        kmax = 0;
    }
    // issue the loads of one tile (base = first element of the tile's first row / k)
    __device__ __forceinline__ void init_phase(long k0, int period) {
#pragma unroll
        for (int r = 0; r < R; ++r) ph[r] = period > 0 ? (int)((k0 + kk[r]) % period) : 1;
    }
    // period > 0 (k-slow modes only): elements whose k row is a multiple of the period read as zero (`base` already points
    // one row back); inc = GBK % period advances the phases to the next tile
    __device__ __forceinline__ void fetch(const float* base, int tile_kmax, long s_ki, int period = 0, int inc = 0) {
        kmax = tile_kmax;
        if constexpr (MODE == 2) {
#pragma unroll
            for (int r = 0; r < R; ++r) sc[r] = base[(ok[r] && kk[r] < tile_kmax) ? (off[r] >> 2) : 0u];
        } else {
            const int krows = tile_kmax < GBK ? tile_kmax : GBK;
            // k-slow: the descriptor ends after the last valid k row; k-fast: per-lane k test (below)
            const int nrec = TR ? 0x7fffffff : krows * (int)s_ki * 4;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, nrec, 0x00020000);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                unsigned o = (TR && kk[r] >= tile_kmax) ? OOR : off[r];
                if (!TR && period > 0) {
                    o = ph[r] == 0 ? OOR : o;
                    ph[r] += inc;
                    ph[r] -= ph[r] >= period ? period : 0;
                }
                if constexpr (VEC) {
                    const gu32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
                    vv[r] = (f32x4){__uint_as_float(t[0]), __uint_as_float(t[1]), __uint_as_float(t[2]), __uint_as_float(t[3])};
                } else {
                    sc[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0));
                }
            }
        }
    }
    __device__ __forceinline__ void stash(float* lds) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (MODE == 3) {
                if (rr[r] < ROWS) *(f32x4*)(lds + rr[r] * LD + kk[r]) = vv[r];
            } else if constexpr (MODE == 0) {
                if (kk[r] < GBK) *(f32x4*)(lds + kk[r] * LD + rr[r]) = vv[r];
            } else if constexpr (MODE == 1) {
                lds[kk[r] * LD + rr[r]] = sc[r];
            } else {
                lds[kk[r] * LD + rr[r]] = (ok[r] && kk[r] < kmax) ? sc[r] : 0.f;   // select here, after the MFMAs
            }
        }
    }
    // operand row (relative to the wave's first row) that MFMA tile i, row q stands for
    static __device__ __forceinline__ int row_of(int i, int q) {
        if constexpr (TR) return 16 * i + q;
        else return i < 4 * (NTW / 4) ? 64 * (i / 4) + 4 * q + (i & 3) : 64 * (NTW / 4) + 2 * q + (i & 1);
    }
    // fragments of the wave's NTW tiles (rows from `row0`) for this lane: out[i][s] = element (row_of(i, li), k = 4*lq + s)
    static __device__ __forceinline__ void frags(const float* lds, int row0, int li, int lq, f32x4 (&out)[NTW]) {
        if constexpr (TR) {
#pragma unroll
            for (int i = 0; i < NTW; ++i) out[i] = *(const f32x4*)(lds + (row0 + 16 * i + li) * LD + 4 * lq);
        } else {
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_) {
                const float* p = lds + (4 * lq + s_) * LD + row0;
#pragma unroll
                for (int g_ = 0; g_ < NTW / 4; ++g_) {
                    const f32x4 v = *(const f32x4*)(p + 64 * g_ + 4 * li);
                    out[4 * g_][s_] = v[0]; out[4 * g_ + 1][s_] = v[1]; out[4 * g_ + 2][s_] = v[2]; out[4 * g_ + 3][s_] = v[3];
                }
                if constexpr (NTW % 4 == 2) {
                    typedef float f32x2_ __attribute__((ext_vector_type(2)));
                    const f32x2_ v = *(const f32x2_*)(p + 64 * (NTW / 4) + 2 * li);
                    out[NTW - 2][s_] = v[0]; out[NTW - 1][s_] = v[1];
                }
            }
        }
    }
};

template <int MI, int NI, int WAVES_M, int AMODE, int BMODE>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmArgs g) {
    constexpr int WAVES_N = 4 / WAVES_M;
    constexpr int BM = 16 * MI * WAVES_M, BN = 16 * NI * WAVES_N;
    using StA = OperandStage<BM, AMODE, MI>;
    using StB = OperandStage<BN, BMODE, NI>;
    __shared__ __attribute__((aligned(16))) float As[2][StA::LDS_FLOATS];
    __shared__ __attribute__((aligned(16))) float Bs[2][StB::LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Block -> (n tile, m tile, K slice).  Workgroups are dealt round-robin to the 8 XCDs, each with its own
    // L2.  With split-K the blocks of one slice read the same K range of A and B, so a slice is kept on one
    // XCD (1-D grid, xcd = id % 8): its operands cross the fabric once instead of once per XCD.
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (g.xcd_remap) {
        const int nb = g.grid_n * g.grid_m;
        const int xcd = blockIdx.x & 7, w = blockIdx.x >> 3;
        bz = xcd + 8 * (w / nb);
        if (bz >= g.split) return;   // whole block, before any barrier
        const int tile = w - (w / nb) * nb;
        by = tile / g.grid_n;
        bx = tile - by * g.grid_n;
    }
    const int m0 = by * BM, n0 = bx * BN;
    const int ntpr = (g.KI + GBK - 1) / GBK;
    const int tiles_total = g.KO * ntpr;
    const int tbeg = bz * g.tiles_per_split;
    int tend = tbeg + g.tiles_per_split;
    if (tend > tiles_total) tend = tiles_total;
    const int wm = (wave / WAVES_N) * 16 * MI, wn = (wave % WAVES_N) * 16 * NI;
    const int li = lane & 15, lq = lane >> 4;

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    StA sa;
    StB sb;
    // which A operand this row tile reads (block-uniform)
    const bool second = g.a2 != nullptr && m0 >= g.M1;
    const int am0 = second ? m0 - g.M1 : m0;
    const long a_sko = second ? g.a2_sko : g.a_sko, a_ski = second ? g.a2_ski : g.a_ski;
    const int a_period = second ? g.a2_period : g.a_period;
    const int a_inc = a_period > 0 ? GBK % a_period : 0;
    sa.init(tid, am0, second ? g.M - g.M1 : (g.a2 ? g.M1 : g.M), g.a_sm, a_ski);
    sa.init_phase((long)tbeg * GBK, a_period);
    sb.init(tid, n0, g.N, g.b_sn, g.b_ski);
    const float* a_blk = (second ? g.a2 : g.a) + (long)am0 * g.a_sm;
    const float* b_blk = g.b + (long)n0 * g.b_sn;
    int f_ko = tbeg / ntpr, f_kt = tbeg - f_ko * ntpr;   // the tile the next fetch() loads (wave-uniform)
    int f_left = tend - tbeg;   // tiles not fetched yet
    auto fetch = [&]() {
        const int kmax = g.KI - f_kt * GBK;   // >= 16 except for the row's last tile
        // The shifted operand's phases advance only towards a tile that is really fetched next: the extra fetch of the final
        // iteration re-reads the LAST tile and must mask the same elements again.  (Round 4: with advanced phases it read
        // element k = 0 for real - the row BEFORE the tensor, `base` points one row back - whenever the slice's only tile
        // starts at k = 0, i.e. batch x time <= 16: a memory access fault when the tape begins a mapped region.)
        const int inc_now = f_left > 1 ? a_inc : 0;
        sa.fetch(a_blk + (long)f_ko * a_sko + (long)(f_kt * GBK - (a_period > 0 ? 1 : 0)) * a_ski, kmax, a_ski, a_period, inc_now);
        sb.fetch(b_blk + (long)f_ko * g.b_sko + (long)(f_kt * GBK) * g.b_ski, kmax, g.b_ski);
        // advance (scalar state only); after the last tile the position stays, so the extra fetch of the final
        // iteration re-reads that tile instead of branching around the loads
        if (--f_left > 0 && ++f_kt == ntpr) { f_kt = 0; ++f_ko; }
    };
    // Per tile: all fragment reads first (one exposed LDS latency per tile instead of one per k-step), then the
    // global loads of the next tile, then 16*MI*NI/4 back-to-back MFMAs, then the staged tile goes to the other
    // LDS buffer.  No branch separates loads, MFMAs and LDS writes (a merge would make the compiler wait for the
    // loads early): the final iteration simply stages its own tile once more, unused.
    f32x4 af[MI], bf[NI];
    auto read_frags = [&](int buf) {
        StA::frags(As[buf], wm, li, lq, af);
        StB::frags(Bs[buf], wn, li, lq, bf);
    };
    auto mfmas = [&]() {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][ks], bf[j][ks], acc[i][j], 0, 0, 0);
    };
    // bias row: column sums of B from the staged registers (row tile 0 only; B in 16-byte mode, host-checked)
    const bool bias_blk = g.bias_row && by == 0;
    f32x4 bsum[StB::VEC ? StB::R : 1];
#pragma unroll
    for (int r = 0; r < (StB::VEC ? StB::R : 1); ++r) bsum[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto add_bias = [&]() {
        if constexpr (BMODE == 0) {
#pragma unroll
            for (int r = 0; r < StB::R; ++r) bsum[r] += sb.vv[r];
        }
    };
    int buf = 0;
    if (tbeg < tend) {
        fetch();
        sa.stash(As[0]);
        sb.stash(Bs[0]);
        if (bias_blk) add_bias();
    }
    __syncthreads();
    for (int t = tbeg; t < tend; ++t) {
        read_frags(buf);
        __builtin_amdgcn_sched_barrier(0);
        fetch();
        __builtin_amdgcn_sched_barrier(0);
        mfmas();
        __builtin_amdgcn_sched_barrier(0);
        sa.stash(As[buf ^ 1]);
        sb.stash(Bs[buf ^ 1]);
        if (bias_blk && t + 1 < tend) add_bias();   // the final iteration re-stages its own tile: not summed twice
        __syncthreads();
        buf ^= 1;
    }
    float* c = g.c + (g.split > 1 ? (size_t)bz * (g.M + g.bias_row) * g.ldc : 0);
    if constexpr (BMODE == 0) {
        if (bias_blk) {   // fold the k rows of the staging map (kk = e / (BN/4)) in a fixed order through LDS
            float* red = Bs[0];
            constexpr int KR = 256 * StB::R / (BN / 4);   // distinct k rows a column quad is staged by
            static_assert(KR * BN <= 2 * StB::LDS_FLOATS, "bias reduction scratch");
#pragma unroll
            for (int r = 0; r < StB::R; ++r)
                if (sb.kk[r] < KR && sb.rr[r] < BN) *(f32x4*)(red + sb.kk[r] * BN + sb.rr[r]) = bsum[r];
            __syncthreads();
            if (tid < BN && n0 + tid < g.N) {
                float t = 0.f;
                for (int q = 0; q < KR; ++q) t += red[q * BN + tid];
                float* cp = c + (size_t)g.M * g.ldc + n0 + tid;
                *cp = g.add_c ? *cp + t : t;
            }
        }
    }
    // k-slow B with four column tiles per wave: a lane's tiles j = 0..3 are four consecutive columns -> 16-byte stores
    const bool vec_out = !StB::TR && NI == 4 && (g.ldc & 3) == 0 && (((uintptr_t)c) & 15) == 0;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm + StA::row_of(i, lq * 4 + r);
            if (m >= g.M) continue;
            if constexpr (!StB::TR && NI == 4) {
                const int nb = n0 + wn + 4 * li;
                if (vec_out && nb + 3 < g.N) {
                    f32x4* cp = (f32x4*)(c + (size_t)m * g.ldc + nb);
                    f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
                    if (g.add_c) v += *cp;
                    *cp = v;
                    continue;
                }
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int n = n0 + wn + StB::row_of(j, li);
                if (n < g.N) {
                    float* cp = c + (size_t)m * g.ldc + n;
                    *cp = g.add_c ? *cp + acc[i][j][r] : acc[i][j][r];
                }
            }
        }
}

// C (+)= A.B.  Few output tiles and a long K -> split-K: slices write partial tiles into
// `scratch` ([split][M][N]) and a fixed-order reduce adds them (deterministic, no atomics).
int gemm_f32(GemmArgs g, int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (g.M <= 0 || g.N <= 0) return FOV_OK;
    const long K = (long)g.KO * g.KI;
    if (K <= 0) {
        return accumulate ? FOV_OK : zero_grad(g.c, (size_t)g.M * g.ldc, stream);
    }
    const size_t mn = (size_t)(g.M + g.bias_row) * g.N;
    // tile shape by M: short-and-wide weight-gradient products (M = F or Out) would waste a 128-row tile
    int BM, BN, variant;
    if (g.M <= 32) { BM = 32; BN = 256; variant = 0; }
    else if (g.M <= 96) { BM = 96; BN = 256; variant = 1; }
    else { BM = 128; BN = 128; variant = 2; }
    // mid-size outputs (e.g. 512 x 1024 of a per-step projection): 128 x 128 tiles would occupy a fraction of
    // the 256 CUs and K is too short to split -> 64 x 64 tiles
    if (variant == 2 && ((g.M + 127) / 128) * ((g.N + 127) / 128) < 128 && K <= 2048) { BM = 64; BN = 64; variant = 3; }
    // short K (the weight gradients of a wide layer at a small batch: 1025 x 2048 x 320 for lstm.py's LSTMCell(400) at batch 32,
    // 144 tiles of 128 x 128): nothing to split, 64 x 64 tiles fill the chip twice over (its training step 0.415 -> 0.397 ms)
    if (variant == 2 && K <= 512 && ((g.M + 127) / 128) * ((g.N + 127) / 128) < 256) { BM = 64; BN = 64; variant = 3; }
    // the same regime with a 33..96-row output (dK of a 90-wide input: eight 96 x 256 tiles): 64 x 64 tiles as well
    if (variant == 1 && K <= 512 && g.N >= 1024) { BM = 64; BN = 64; variant = 3; }
    // mid-length K on a few dozen 128 x 128 tiles (the 512 x 1024 x 5120 weight gradients of configs[2] at T = 10: 32 tiles x 8 slices):
    // 64 x 128 tiles halve the slices - and the partials written and re-read - for the same block count; measured on the training
    // step 0.788 -> 0.775 ms.  Longer K stays (T = 30, K = 15 360: 1.955 -> 1.969 ms; configs[1], K = 30 720: 1.231 -> 1.287 ms).
    if (variant == 2 && K > 2048 && K <= 8192 && ((g.M + 127) / 128) * ((g.N + 127) / 128) <= 64) { BM = 64; BN = 128; variant = 4; }
    if (const int v = env_knobs().gemm_variant) {   // tuning knob (experiments), FOV_GEMM_VARIANT
        if (v == 2) { BM = 128; BN = 128; variant = 2; }
        if (v == 3) { BM = 64; BN = 64; variant = 3; }
        if (v == 4) { BM = 64; BN = 128; variant = 4; }
    }
    // per-thread staging offsets span one block tile: they must fit 32 bits
    {
        const long amax = (long)BM * (g.a_sm < 0 ? -g.a_sm : g.a_sm) + 16 * (g.a_ski < 0 ? -g.a_ski : g.a_ski);
        const long bmax = (long)BN * (g.b_sn < 0 ? -g.b_sn : g.b_sn) + 16 * (g.b_ski < 0 ? -g.b_ski : g.b_ski);
        if (amax >= (1L << 30) || bmax >= (1L << 30) || g.a_sm < 0 || g.a_ski < 0 || g.b_sn < 0 || g.b_ski < 0) {
            set_error("gemm_f32: operand strides out of range");
            return FOV_ERR_UNSUPPORTED;
        }
    }
    const int ntpr = (g.KI + GBK - 1) / GBK;
    const long ktiles = (long)g.KO * ntpr;
    if (ktiles > 0x7fffffffL) { set_error("gemm_f32: K too large"); return FOV_ERR_UNSUPPORTED; }
    const int tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
    int split = 1;
    if (tiles < 512 && ktiles >= 32) {
        // fewer tiles than two per CU and a long K: slices.  (256 <= tiles < 512, e.g. the 5120 x 256 x 1024 data gradient of
        // the stacked layer on 64 x 64 tiles: four slices measured 55 -> 43 us)
        // The blocks of a launch are co-resident (2-3 per CU) and share the matrix pipe, so the launch takes
        // ceil(blocks / CUs) block-times: 40 tiles x 13 slices = 520 blocks on 256 CUs cost THREE rounds for 2.03 rounds of
        // work (the 513 x 1024 weight gradients of configs[2] ran at 58 % of peak).  Among the slice counts up to the
        // old target (about 512 resp. 1024 blocks) take the one that fills its last round best; ties go to fewer slices.
        const int cus = device_cu_count() > 0 ? device_cu_count() : 256;
        const int want = ((tiles < 256 ? 512 : 1024) + tiles - 1) / tiles;
        long maxs = ktiles / 4;   // >= 4 k-tiles (64 k) per slice
        if (maxs > 64) maxs = 64;
        if (maxs > want) maxs = want;
        double best = -1.0;
        for (int sct = 1; sct <= (int)maxs; ++sct) {
            const long blocks = (long)tiles * sct;
            const long rounds = (blocks + cus - 1) / cus;
            double fill = (double)blocks / (double)(rounds * cus);
            if (blocks < cus) fill *= 0.5;                       // less than one block per CU: only if nothing else is possible
            else if (rounds == 1) fill *= 0.9;                   // one round: a second one overlaps latencies better
            if (fill > best + 1e-9) { best = fill; split = sct; }
        }
        if (split < 1) split = 1;
    } else if (tiles < 128 && ktiles >= 8) {
        // SHORT K on a few tiles (model.fit at the reference's batch of 32: B*T = 320 rows -> 20 k-tiles, dK of a layer is
        // two 96 x 256 tiles): a block's time is its k-tiles x ~2.2 us of unhidden global -> LDS -> barrier latency, so two
        // blocks took 46 us for 30 MFLOP.  Slices of >= 2 k-tiles up to about one block per CU; the reduce launch (4.5 us)
        // is paid back from 4 k-tiles per block on.
        split = (256 + tiles - 1) / tiles;
        const long maxs = ktiles / 2;
        if (split > maxs) split = (int)maxs;
        if (split > 64) split = 64;
        if (split < 1) split = 1;
    }
    if (const int v = env_knobs().gemm_split) { if (v >= 1 && v <= ktiles) split = v; }   // tuning knob, FOV_GEMM_SPLIT
    while (split > 1 && (size_t)split * mn > scratch_floats) --split;
    const long tps = (ktiles + split - 1) / split;
    split = (int)((ktiles + tps - 1) / tps);
    // accumulate with a single K slice happens in the epilogue (C += A.B, one writer per element)
    g.add_c = (accumulate && split == 1) ? 1 : 0;
    const bool via_scratch = (split > 1);
    float* c_final = g.c;
    bool deferred = false;
    if (via_scratch) {
        if (mn * split > scratch_floats) { set_error("gemm_f32: scratch too small (%zu floats needed)", mn * split); return FOV_ERR_WORKSPACE; }
        if (g.ldc != g.N) { set_error("gemm_f32: accumulate/split-K needs a dense C (ldc == N)"); return FOV_ERR_INVALID; }
        if (float* arena = defer_alloc(c_final, mn, mn * split, stream)) { scratch = arena; deferred = true; }
        g.c = scratch;
    } else {
        if (int rc_ = defer_touch(c_final, (size_t)(g.M + g.bias_row) * g.ldc, stream)) return rc_;
    }
    g.split = split;
    g.tiles_per_split = (int)tps;
    // staging modes.  k-slow: all row offsets of one k row stay below the k stride and 16 k rows fit a 31-bit
    // byte range -> buffer loads; 16-byte form when the row index is contiguous, every row start is 16-byte
    // aligned and a group of four never straddles the matrix edge.
    const int Ma = g.a2 ? g.M1 : g.M;   // width of the first A operand
    const bool a_ks = g.a_ski >= (long)(Ma - 1) * g.a_sm + 1 && g.a_ski < (1L << 24) && (((uintptr_t)g.a) & 3) == 0;
    const bool b_ks = g.b_ski >= (long)(g.N - 1) * g.b_sn + 1 && g.b_ski < (1L << 24) && (((uintptr_t)g.b) & 3) == 0;
    const bool a_v4 = a_ks && g.a_sm == 1 && (g.M & 3) == 0 && (g.a_sko & 3) == 0 && (g.a_ski & 3) == 0 && (((uintptr_t)g.a) & 15) == 0 &&
                      (!g.a2 || ((g.M1 & 3) == 0 && (g.a2_sko & 3) == 0 && (g.a2_ski & 3) == 0 && (((uintptr_t)g.a2) & 15) == 0 &&
                                 g.a2_ski >= (long)(g.M - g.M1) && g.a2_ski < (1L << 24)));
    const bool b_v4 = b_ks && g.b_sn == 1 && (g.N & 3) == 0 && (g.b_sko & 3) == 0 && (g.b_ski & 3) == 0 && (((uintptr_t)g.b) & 15) == 0;
    // k-fast: k is the contiguous index, rows and ko rows start 16-byte aligned, KI a multiple of 4
    const bool a_kf = g.a_ski == 1 && (g.KI & 3) == 0 && (g.a_sm & 3) == 0 && (g.a_sko & 3) == 0 && (((uintptr_t)g.a) & 15) == 0;
    const bool b_kf = g.b_ski == 1 && (g.KI & 3) == 0 && (g.b_sn & 3) == 0 && (g.b_sko & 3) == 0 && (((uintptr_t)g.b) & 15) == 0;
    const int amode = a_v4 ? 0 : (a_ks ? 1 : (a_kf ? 3 : 2)), bmode = b_v4 ? 0 : (b_ks ? 1 : (b_kf ? 3 : 2));
    if ((g.bias_row && bmode != 0) || ((g.a_period || g.a2_period) && (amode > 1 || g.KO != 1)) || (g.a2 && (g.M1 % BM || amode != 0))) {
        set_error("gemm_f32: fused weight gradient needs 16-byte-aligned k-slow operands and M1 a multiple of the row tile");
        return FOV_ERR_UNSUPPORTED;
    }
    g.grid_n = (g.N + BN - 1) / BN;
    g.grid_m = (g.M + BM - 1) / BM;
    g.xcd_remap = split >= 8 ? 1 : 0;
    const dim3 grid = g.xcd_remap ? dim3((unsigned)(8 * ((split + 7) / 8) * g.grid_n * g.grid_m)) : dim3(g.grid_n, g.grid_m, split);
    if (env_knobs().dbg_trace)
        fprintf(stderr, "[fov trace] gemm_f32 next: M=%d N=%d KO=%d KI=%d variant=%d amode=%d bmode=%d split=%d a2=%d periods=%d/%d bias=%d add_c=%d\n", g.M, g.N,
                g.KO, g.KI, variant, amode, bmode, split, g.a2 ? 1 : 0, g.a_period, g.a2_period, g.bias_row, g.add_c);
#define FOV_GEMM_LAUNCH(MI_, NI_, WM_, A_, B_) \
    hipLaunchKernelGGL((gemm_f32_kernel<MI_, NI_, WM_, A_, B_>), grid, dim3(256), 0, stream, g)
#define FOV_GEMM_MODES(MI_, NI_, WM_)                                                            \
    switch (amode * 4 + bmode) {                                                                 \
        case 0: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 0, 0); break;                                     \
        case 1: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 0, 1); break;                                     \
        case 2: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 0, 2); break;                                     \
        case 3: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 0, 3); break;                                     \
        case 4: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 1, 0); break;                                     \
        case 5: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 1, 1); break;                                     \
        case 6: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 1, 2); break;                                     \
        case 7: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 1, 3); break;                                     \
        case 8: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 2, 0); break;                                     \
        case 9: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 2, 1); break;                                     \
        case 10: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 2, 2); break;                                    \
        case 11: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 2, 3); break;                                    \
        case 12: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 3, 0); break;                                    \
        case 13: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 3, 1); break;                                    \
        case 14: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 3, 2); break;                                    \
        default: FOV_GEMM_LAUNCH(MI_, NI_, WM_, 3, 3); break;                                    \
    }
    if (variant == 0) { FOV_GEMM_MODES(2, 4, 1) }
    else if (variant == 1) { FOV_GEMM_MODES(6, 4, 1) }
    else if (variant == 3) { FOV_GEMM_MODES(2, 2, 2) }
    else if (variant == 4) { FOV_GEMM_MODES(2, 4, 2) }
    else { FOV_GEMM_MODES(4, 4, 2) }
#undef FOV_GEMM_MODES
#undef FOV_GEMM_LAUNCH
    int rc = launch_check("gemm_f32");
    if (rc || !via_scratch) return rc;
    return reduce_or_defer(deferred, scratch, c_final, (long)mn, split, accumulate, stream, "splitk_reduce");
}

// C (M,N) = A (M,K) . B (K,N), all row-major dense
int matmul_f32(const float* a, const float* b, float* c, int M, int K, int N, float* scratch, size_t scratch_floats, hipStream_t stream) {
    return gemm_f32(gemm_nn(a, K, b, N, c, N, M, N, K), 0, scratch, scratch_floats, stream);
}

// Skinny weight gradients: out[s][w] = sum_r S[r][s] * Wd[r][w] with ns <= 8 (dK of the decoder LSTM, F_dec = 6;
// dW of Dense(6)).  An MFMA tile would be >= 80 % padding and the product is HBM-bound anyway (Wd is read
// once): thread = column w, block = (256 columns, chunk of rows), the ns values of a row are wave-uniform
// scalar loads.  Partials land in scratch already in the output layout (element s*os + w*ow of slice
// `chunk`), and splitk_reduce adds the slices in a fixed order.
template <int NS, int VEC>
__global__ __launch_bounds__(256) void skinny_tn_kernel(const float* __restrict__ S, long ss, const float* __restrict__ Wd,
                                                        long ldw, float* __restrict__ part, long rows, int nw,
                                                        long rows_per_chunk, long os, long ow) {
    // block = 64*VEC columns x 4 row groups (wave q takes rows r0+q, r0+q+4, ...); eight rows in flight per
    // thread, VEC = 4 reads 16 bytes per lane and row
    __shared__ float red[4][NS][64 * VEC];
    const int li = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int w = (blockIdx.x * 64 + li) * VEC;
    const long r0 = (long)blockIdx.y * rows_per_chunk;
    long r1 = r0 + rows_per_chunk;
    if (r1 > rows) r1 = rows;
    float acc[NS][VEC];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[i][v] = 0.f;
    if (w < nw) {
        for (long r = r0 + q; r < r1; r += 32) {
            float wv[8][VEC];
            long rr[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool ok = r + 4 * u < r1;
                rr[u] = ok ? r + 4 * u : r;   // rows past the chunk re-read row r and contribute zero
                if (VEC == 4) {
                    const f32x4 t = *(const f32x4*)(Wd + rr[u] * ldw + w);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) wv[u][v] = ok ? t[v] : 0.f;
                } else {
                    wv[u][0] = ok ? Wd[rr[u] * ldw + w] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const float sv = S[rr[u] * ss + i];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[i][v] = fmaf(sv, wv[u][v], acc[i][v]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int v = 0; v < VEC; ++v) red[q][i][li * VEC + v] = acc[i][v];
    __syncthreads();
    if (q == 0 && w < nw) {
        float* pp = part + (long)blockIdx.y * NS * nw;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int c = li * VEC + v;
                pp[i * os + (w + v) * ow] = (red[0][i][c] + red[1][i][c]) + (red[2][i][c] + red[3][i][c]);
            }
    }
}

int skinny_tn(const float* S, long ss, int ns, const float* Wd, long ldw, int nw, long rows, float* out, long os, long ow,
              int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (ns < 1 || ns > 8 || rows < 1024) return 0;
    const bool vec = nw >= 512 && (nw & 3) == 0 && (ldw & 3) == 0 && (((uintptr_t)Wd) & 15) == 0;
    const int colblocks = (nw + (vec ? 255 : 63)) / (vec ? 256 : 64);
    long chunks = (2048 + colblocks - 1) / colblocks;   // ~2048 blocks when the rows allow it
    if (chunks > rows / 32) chunks = rows / 32;         // >= 32 rows per chunk
    if (chunks > 1024) chunks = 1024;
    const size_t n = (size_t)ns * nw;
    while (chunks > 1 && (size_t)chunks * n > scratch_floats) chunks >>= 1;
    if (chunks < 1 || (size_t)chunks * n > scratch_floats) return 0;
    const long rpc = (rows + chunks - 1) / chunks;
    const dim3 grid(colblocks, (unsigned)chunks);
    bool deferred = false;
    if (float* arena = defer_alloc(out, n, (size_t)chunks * n, stream)) { scratch = arena; deferred = true; }
    if (env_knobs().dbg_trace) fprintf(stderr, "[fov trace] skinny_tn next: ns=%d nw=%d rows=%ld vec=%d chunks=%ld\n", ns, nw, rows, (int)vec, chunks);
#define FOV_SKINNY(NSV)                                                                                                       \
    case NSV:                                                                                                                 \
        if (vec) hipLaunchKernelGGL((skinny_tn_kernel<NSV, 4>), grid, dim3(256), 0, stream, S, ss, Wd, ldw, scratch, rows, nw, \
                                    rpc, os, ow);                                                                             \
        else hipLaunchKernelGGL((skinny_tn_kernel<NSV, 1>), grid, dim3(256), 0, stream, S, ss, Wd, ldw, scratch, rows, nw,    \
                                rpc, os, ow);                                                                                 \
        break
    switch (ns) {
        FOV_SKINNY(1); FOV_SKINNY(2); FOV_SKINNY(3); FOV_SKINNY(4); FOV_SKINNY(5); FOV_SKINNY(6); FOV_SKINNY(7); FOV_SKINNY(8);
    }
#undef FOV_SKINNY
    int rc = launch_check("skinny_tn");
    if (rc) return rc;
    rc = reduce_or_defer(deferred, scratch, out, (long)n, (int)chunks, accumulate, stream, "skinny_reduce");
    return rc ? rc : 1;
}

}  // namespace fov
