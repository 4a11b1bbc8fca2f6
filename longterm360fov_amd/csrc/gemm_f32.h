// The fp32 matrix-core GEMM of the training step (gemm_f32.hip): its argument block, the three operand forms the
// callers use, and the entry points.
#pragma once
#include "fov_common.h"

namespace fov {

// ---------------------------------------------------------------------------------------
// C[m][n] = sum_k A(m,k) * B(k,n);  k = ko*KI + ki.
//   A(m,k) = a[m*a_sm + ko*a_sko + ki*a_ski],  B(k,n) = b[n*b_sn + ko*b_sko + ki*b_ski]
// The two-level k lets (batch, time) row pairs with a time shift be contracted without copies
// (dR = sum_{b,t} h_{t-1}^T dz_t).  blockIdx.z = split-K slice; slice s writes C + s*M*N when
// `split` > 1 (partials), else C directly.
// ---------------------------------------------------------------------------------------
struct GemmArgs {
    const float* a;
    const float* b;
    float* c;
    int M, N, KO, KI;
    long a_sm, a_sko, a_ski;
    long b_sn, b_sko, b_ski;
    int ldc;
    int split;       // number of K slices (grid.z)
    int tiles_per_split; // k-tiles (of 16, never straddling a ko row) per slice
    int xcd_remap, grid_n, grid_m;   // 1-D grid with slices pinned to XCDs (split >= 8)
    int add_c;       // single-slice accumulate: C += A.B in the epilogue (one writer per element, deterministic)
    // fused weight gradient [dK ; dR ; db] = [x | h_prev | 1]^T dz (one product, one reduce); k-slow operands only
    const float* a2;   // second A operand: rows [M1, M) of C come from it (M1 a multiple of the row tile), or NULL
    long a2_sko, a2_ski;
    int M1;
    int a_period, a2_period;   // T > 0 (KO == 1): k index r of the operand is its row r - 1, zero where r % T == 0 - h_{t-1}
                               // read from the (B,T,H) tape of h_t with the rows kept flat (full 16-row k-tiles)
    int bias_row;      // 1: row M of C = column sums of B (B staged with 16-byte loads)
};
// The operand forms of the training step (lda / ldb / ldc: floats between rows of the stored matrix).  wgrad_fused
// (lstm_train.hip) sets up the fourth one, with a2 / periods / bias_row, itself.
// C (M,N) = A (M,K) . B (K,N)
inline GemmArgs gemm_nn(const float* a, long lda, const float* b, long ldb, float* c, int ldc, int M, int N, int K) {
    GemmArgs g = {};
    g.a = a; g.b = b; g.c = c; g.M = M; g.N = N; g.KO = 1; g.KI = K;
    g.a_sm = lda; g.a_ski = 1; g.b_sn = 1; g.b_ski = ldb; g.ldc = ldc;
    return g;
}
// C (M,N) = A (M,K) . B^T, B stored (N,K)
inline GemmArgs gemm_nt(const float* a, long lda, const float* b, long ldb, float* c, int ldc, int M, int N, int K) {
    GemmArgs g = {};
    g.a = a; g.b = b; g.c = c; g.M = M; g.N = N; g.KO = 1; g.KI = K;
    g.a_sm = lda; g.a_ski = 1; g.b_sn = ldb; g.b_ski = 1; g.ldc = ldc;
    return g;
}
// C (M,N), dense = A^T . B over the rows (ko, ki) of A (.,M) and B (.,N): row (ko, ki) starts at ko*a_sko + ki*lda
// resp. ko*b_sko + ki*ldb (KO = 1: plain rows)
inline GemmArgs gemm_tn(const float* a, long lda, const float* b, long ldb, float* c, int M, int N, int KO, int KI,
                        long a_sko = 0, long b_sko = 0) {
    GemmArgs g = {};
    g.a = a; g.b = b; g.c = c; g.M = M; g.N = N; g.KO = KO; g.KI = KI;
    g.a_sm = 1; g.a_sko = a_sko; g.a_ski = lda; g.b_sn = 1; g.b_sko = b_sko; g.b_ski = ldb; g.ldc = N;
    return g;
}

// C (+)= A.B through the matrix cores; a long K on few tiles is split, the slices summed in a fixed order (gemm_f32.hip)
int gemm_f32(GemmArgs g, int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream);
// the same A^T . B for a side of <= 8 columns: returns 1 when the product was done, 0 when the caller should use gemm_f32, < 0 on error
int skinny_tn(const float* S, long ss, int ns, const float* Wd, long ldw, int nw, long rows, float* out, long os, long ow,
              int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream);

}  // namespace fov
