// The Keras 2.1-2.2 'accuracy' metric of model.compile(metrics=['accuracy']), counted where the prediction lies:
//   mycode/given_others_gt_mean_var_seq2seq.py:308, FoV_seq2seq_mu_var.py:248, Fov_seq2seq_2layers.py:335, 3layers.py:302,
//   lstm_keras.py:87,247,392, convlstm_heatmap.py:281
// keras/engine/training.py picks, for any loss but the two crossentropies, by the output's last dim:
//   C > 1   categorical_accuracy   K.equal(K.argmax(y_true, -1), K.argmax(y_pred, -1))
//   C == 1  binary_accuracy        K.equal(y_true, K.round(y_pred))            (round half to even)
// and logs the mean; here the NUMBER of matching rows is left in a device int64 and the caller divides once per epoch.
// Arg-max follows heatmap_decode.hip (np.argmax): lowest index among equal maxima, -0.0 == +0.0, the first NaN is the maximum.
//
// A row is C contiguous floats; L lanes (a power of two, 1 <= L <= 64: a wave never splits a group) share a row, lane j on
// channels j*V .. j*V+V-1, then L*V further on, ... in increasing order.  V = 2: 8-byte loads (bases 8-byte aligned, every
// stride even); V = 1, the scalar form: 4-byte loads.  A value becomes an int key whose signed order is np.argmax's order
// (acc_key: any NaN above +inf, -0.0 = +0.0), a lane keeps its best (key, index), taking a later channel only on a strict >.
// The group's maximum key is an all-reduce over its L lanes, the arg-max a second one: the minimum index among the lanes
// that hold that key.  Both are min / max of ints, so the order of the steps cannot change the result; the steps inside 16
// lanes are DPP moves (quad permutes, mirrored half row, mirrored row), those across 16 and 32 lanes shuffles.  L = 1 is a
// thread per row (C <= 8: the LSTM models' 6 tokens).  At the heat maps' 30 channels L = 16, V = 2: a wave reads four
// 120-byte rows per load, 480 contiguous bytes when the rows are dense, and reduces without touching LDS.  Rows (i0, i1, r)
// are walked grid-stride with carried indices (no division in the loop), two rows of a group per iteration - all four loads
// first where a group covers a row in one pass.  Counts: int per thread -> wave shuffle sum -> LDS -> ONE 64-bit integer
// vector atomic per workgroup on a grid of at most AC_MAX_BLOCKS.  Integer sums: exact, the same in every run.
#include "fov_common.h"

namespace fov {

constexpr int AC_NT = 256;
constexpr int AC_MAX_BLOCKS = 2048;      // 8 workgroups of 4 waves for each of 256 CUs, 2048 atomics a call at the most (chosen, not tuned)
constexpr long AC_MAX_ROWS = 1L << 40;   // a thread's int and a workgroup's 32-bit LDS count stay far from their ends

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct AccOperand {
    const float* base;
    long s0, s1, rs;                     // floats
};

struct AccParams {
    AccOperand pred, tgt;
    long n0, n1, rows, total;            // total = n0 * n1 * rows
    int C, L;
    unsigned long long* matches;
};

struct RowPos {
    long i0, i1, r, flat;
};

// A float as an int whose signed order is np.argmax's: NaN (any) above +inf, -0.0 == +0.0, the rest by value.
__device__ __forceinline__ int acc_key(float v) {
    int b = __float_as_int(v);
    b = b == (int)0x80000000 ? 0 : b;                 // -0.0 -> +0.0
    const int k = b ^ ((b >> 31) & 0x7fffffff);       // negative floats: the larger magnitude the smaller key
    return v != v ? 0x7fffffff : k;
}
constexpr int AC_NO_KEY = (int)0x80000000;            // a lane that owns no channel: below -inf's key
constexpr int AC_NO_INDEX = 0x7fffffff;

__device__ __forceinline__ const float* acc_row(const AccOperand& o, const RowPos& q) {
    return o.base + q.i0 * o.s0 + q.i1 * o.s1 + q.r * o.rs;
}

// channels c (and c + 1 in the 8-byte form, when the row has it) of a row -> their keys; AC_NO_KEY past the row's end
template <int V>
__device__ __forceinline__ void acc_load_keys(const float* row, int c, int C, int& k0, int& k1) {
    const bool has0 = c < C, has1 = V == 2 && c + 1 < C;
    float v0 = 0.f, v1 = 0.f;
    if (has1) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(row + c);
        v0 = t.x; v1 = t.y;
    } else if (has0) {
        v0 = row[c];
    }
    k0 = has0 ? acc_key(v0) : AC_NO_KEY;
    k1 = has1 ? acc_key(v1) : AC_NO_KEY;
}

// lane j's share of one row: channels c = j*V + k*L*V (+1), k = 0, 1, ... in increasing order, a later one only on a strict >
template <int V>
__device__ __forceinline__ void acc_lane_best(const float* row, int j, int L, int C, int& key, int& idx) {
    key = AC_NO_KEY; idx = AC_NO_INDEX;
    for (int c = j * V; c < C; c += L * V) {
        int k0, k1;
        acc_load_keys<V>(row, c, C, k0, k1);
        if (idx == AC_NO_INDEX || k0 > key) { key = k0; idx = c; }
        if (k1 > key) { key = k1; idx = c + 1; }
    }
}

// All-reduce over the L lanes of a group (L a power of two, groups aligned to L lanes, the whole wave active): lanes 1, 2
// apart inside a quad, then the mirrored half row and the mirrored row (DPP: no LDS traffic), then the lanes 16 and 32 apart.
template <bool MAX>
__device__ __forceinline__ int acc_group_reduce(int x, int L) {
#define ACC_STEP(other) { const int o_ = (other); x = MAX ? (o_ > x ? o_ : x) : (o_ < x ? o_ : x); }
    if (L > 1) ACC_STEP(__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    if (L > 2) ACC_STEP(__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    if (L > 4) ACC_STEP(__builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false));   // row_half_mirror
    if (L > 8) ACC_STEP(__builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false));   // row_mirror
    if (L > 16) ACC_STEP(__shfl_xor(x, 16));
    if (L > 32) ACC_STEP(__shfl_xor(x, 32));
#undef ACC_STEP
    return x;
}

// the row's arg-max from the lanes' (key, index): the largest key, and among the lanes that hold it the lowest index
__device__ __forceinline__ int acc_group_argmax(int key, int idx, int L) {
    const int top = acc_group_reduce<true>(key, L);
    return acc_group_reduce<false>(key == top ? idx : AC_NO_INDEX, L);
}

template <int V>
__device__ __forceinline__ int acc_row_match(const float* pred_row, const float* tgt_row, int j, int L, int C) {
    int pk, pi, tk, ti;
    acc_lane_best<V>(pred_row, j, L, C, pk, pi);
    acc_lane_best<V>(tgt_row, j, L, C, tk, ti);
    return acc_group_argmax(pk, pi, L) == acc_group_argmax(tk, ti, L);
}

// the same for two rows whose channels a group covers in one pass (C <= L*V): the four loads first, then the arithmetic
template <int V>
__device__ __forceinline__ void acc_row_match2(const float* p0, const float* t0, const float* p1, const float* t1, int j, int L, int C,
                                               int& m0, int& m1) {
    const int c = j * V;
    int a0, a1, b0, b1, c0, c1, d0, d1;
    acc_load_keys<V>(p0, c, C, a0, a1);
    acc_load_keys<V>(t0, c, C, b0, b1);
    acc_load_keys<V>(p1, c, C, c0, c1);
    acc_load_keys<V>(t1, c, C, d0, d1);
    const int none = c < C ? 0 : AC_NO_INDEX;         // a lane past the row's end offers no index
    m0 = acc_group_argmax(a1 > a0 ? a1 : a0, (c + (a1 > a0)) | none, L) == acc_group_argmax(b1 > b0 ? b1 : b0, (c + (b1 > b0)) | none, L);
    m1 = acc_group_argmax(c1 > c0 ? c1 : c0, (c + (c1 > c0)) | none, L) == acc_group_argmax(d1 > d0 ? d1 : d0, (c + (d1 > d0)) | none, L);
}

// q += step, with the carries of the mixed radix (n1, rows); both are valid positions or step < total
__device__ __forceinline__ void acc_advance(RowPos& q, const RowPos& step, long n1, long rows) {
    q.flat += step.flat;
    q.r += step.r;
    if (q.r >= rows) { q.r -= rows; ++q.i1; }
    q.i1 += step.i1;
    if (q.i1 >= n1) { q.i1 -= n1; ++q.i0; }
    q.i0 += step.i0;
}

__device__ __forceinline__ RowPos acc_pos(long flat, long n1, long rows) {
    RowPos q;
    q.flat = flat;
    const long slab = flat / rows;
    q.r = flat - slab * rows;
    q.i0 = slab / n1;
    q.i1 = slab - q.i0 * n1;
    return q;
}

__device__ __forceinline__ void acc_block_sum(int cnt, unsigned long long* matches) {
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, (unsigned)cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(matches, (unsigned long long)s_cnt);
}

// C > 1.  The cross-lane steps need the whole wave active: the trip count is the same for every thread of the grid, and a
// group that has run out of rows computes on row 0 and does not count it.
template <int V>
__global__ __launch_bounds__(AC_NT) void categorical_accuracy_kernel(AccParams p) {
    const int L = p.L;
    const long tid = blockIdx.x * (long)AC_NT + threadIdx.x;
    const long groups = (long)gridDim.x * AC_NT / L;
    const int j = (int)(tid & (L - 1));
    const RowPos step = acc_pos(groups % p.total, p.n1, p.rows);      // groups > total: one pass, the step is never applied twice
    RowPos q = acc_pos((tid / L) % p.total, p.n1, p.rows);
    int cnt = 0;
    const bool one_pass = p.C <= L * V;
    const long last = ((p.total + groups - 1) / groups) * groups;     // the wave-uniform trip count
#pragma unroll 1
    for (long f = tid / L; f < last; f += 2 * groups) {
        const bool ok0 = f < p.total, ok1 = f + groups < p.total;
        RowPos q1 = q;
        if (ok1) acc_advance(q1, step, p.n1, p.rows);
        const float* p0 = ok0 ? acc_row(p.pred, q) : p.pred.base;
        const float* t0 = ok0 ? acc_row(p.tgt, q) : p.tgt.base;
        const float* p1 = ok1 ? acc_row(p.pred, q1) : p.pred.base;
        const float* t1 = ok1 ? acc_row(p.tgt, q1) : p.tgt.base;
        int m0, m1;
        if (one_pass) {
            acc_row_match2<V>(p0, t0, p1, t1, j, L, p.C, m0, m1);
        } else {
            m0 = acc_row_match<V>(p0, t0, j, L, p.C);
            m1 = acc_row_match<V>(p1, t1, j, L, p.C);
        }
        cnt += (ok0 && j == 0 ? m0 : 0) + (ok1 && j == 0 ? m1 : 0);
        q = q1;
        if (f + 2 * groups < p.total) acc_advance(q, step, p.n1, p.rows);
    }
    acc_block_sum(cnt, p.matches);
}

// C == 1: an element a thread
__global__ __launch_bounds__(AC_NT) void binary_accuracy_kernel(AccParams p) {
    const long tid = blockIdx.x * (long)AC_NT + threadIdx.x;
    const long threads = (long)gridDim.x * AC_NT;
    int cnt = 0;
    const RowPos step = acc_pos(threads % p.total, p.n1, p.rows);     // threads >= total: one pass, the step is never applied
    RowPos q = acc_pos(tid % p.total, p.n1, p.rows);
#pragma unroll 1
    for (long f = tid; f < p.total; f += threads) {
        cnt += *acc_row(p.tgt, q) == rintf(*acc_row(p.pred, q));      // v_rndne_f32: half to even; a NaN matches nothing
        if (f + threads < p.total) acc_advance(q, step, p.n1, p.rows);
    }
    acc_block_sum(cnt, p.matches);
}

static bool acc_operand_ok(const float* base, long s0, long s1, long rs, int C) {
    return base && s0 >= 0 && s1 >= 0 && rs >= C;
}

static bool acc_vector_ok(const AccOperand& o) {
    return !(((uintptr_t)o.base) & 7) && !(o.s0 & 1) && !(o.s1 & 1) && !(o.rs & 1);
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_categorical_accuracy(const float* pred, int64_t pred_s0, int64_t pred_s1, int64_t pred_row_stride,
                             const float* target, int64_t tgt_s0, int64_t tgt_s1, int64_t tgt_row_stride,
                             int64_t n0, int64_t n1, int64_t rows, int C, int64_t* matches, int accumulate, fov_stream_t stream) {
    if (C < 1 || n0 < 0 || n1 < 0 || rows < 0 || !matches || (((uintptr_t)matches) & 7)) {
        set_error("fov_categorical_accuracy: invalid argument (C >= 1, n0, n1, rows >= 0, matches not NULL and 8-byte aligned)");
        return FOV_ERR_INVALID;
    }
    long total = 0;
    if (__builtin_mul_overflow((long)n0, (long)n1, &total) || __builtin_mul_overflow(total, (long)rows, &total) || total > AC_MAX_ROWS) {
        set_error("fov_categorical_accuracy: more than 2^40 rows");
        return FOV_ERR_INVALID;
    }
    // every refusal comes before the count is touched: a refused call leaves *matches as it was
    if (total > 0 &&
        (!acc_operand_ok(pred, pred_s0, pred_s1, pred_row_stride, C) || !acc_operand_ok(target, tgt_s0, tgt_s1, tgt_row_stride, C))) {
        set_error("fov_categorical_accuracy: invalid operand (not NULL, outer strides >= 0, row_stride >= C)");
        return FOV_ERR_INVALID;
    }
    if (!accumulate) {
        const hipError_t e = hipMemsetAsync(matches, 0, sizeof(int64_t), (hipStream_t)stream);
        if (e != hipSuccess) { set_error("fov_categorical_accuracy: zeroing the count: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    }
    if (total == 0) return FOV_OK;
    AccParams p;
    p.pred = {pred, (long)pred_s0, (long)pred_s1, (long)pred_row_stride};
    p.tgt = {target, (long)tgt_s0, (long)tgt_s1, (long)tgt_row_stride};
    p.n0 = n0; p.n1 = n1; p.rows = rows; p.total = total; p.C = C;
    p.matches = reinterpret_cast<unsigned long long*>(matches);
    const dim3 block(AC_NT);
    if (C == 1) {
        p.L = 1;
        const long blocks = (total + AC_NT - 1) / AC_NT;
        hipLaunchKernelGGL(binary_accuracy_kernel, dim3((unsigned)(blocks < AC_MAX_BLOCKS ? blocks : AC_MAX_BLOCKS)), block, 0,
                           (hipStream_t)stream, p);
        return launch_check("binary_accuracy");
    }
    // 8-byte loads need every row of both operands on an 8-byte boundary; anything else: the scalar form
    const bool vec = C > 8 && acc_vector_ok(p.pred) && acc_vector_ok(p.tgt);
    int L = 1;
    if (C > 8)
        while (L < 64 && L * (vec ? 2 : 1) < C) L <<= 1;
    p.L = L;
    const long per_block = AC_NT / L;                                  // rows a workgroup takes per pass
    const long blocks = (total + 2 * per_block - 1) / (2 * per_block); // two rows of a group in flight
    const dim3 grid((unsigned)(blocks < AC_MAX_BLOCKS ? blocks : AC_MAX_BLOCKS));
    if (vec)
        hipLaunchKernelGGL(categorical_accuracy_kernel<2>, grid, block, 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(categorical_accuracy_kernel<1>, grid, block, 0, (hipStream_t)stream, p);
    return launch_check("categorical_accuracy");
}

}  // extern "C"
