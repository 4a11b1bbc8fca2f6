// Fixed-order reductions of the training step (HBM-bound; no float atomics, so every gradient is deterministic):
// splitk_reduce_kernel sums the partial slices of a split product, the deferred-reduction regions collect a step's
// split products into ONE batched reduce launch, and colsum forms the bias gradients through the same tail.
#include <mutex>

#include "fov_common.h"

namespace fov {

// out[i] = (accumulate ? out[i] : 0) + sum_s part[s][i].  Block = 64 outputs x 4 slice groups: group q adds
// slices q, q+4, q+8, ... (eight loads in flight per thread), then the four group sums are folded in a fixed
// order through LDS - deterministic for a given (n, S), and short products with many slices are not
// serialised on one thread per output.
// VEC: four consecutive outputs per lane through 16-byte loads (n % 4 == 0, 16-byte aligned slices and output) - the
// batched reduce of a training step reads ~80 MB of slices and ran at 1.8 TB/s with 4-byte loads.  The order of additions
// per output is the same in both forms.
template <bool VEC>
__device__ __forceinline__ void splitk_reduce_body(const float* __restrict__ part, float* __restrict__ out, long n, int S,
                                                   int accumulate, long block) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ float red[4][64 * W];
    const int li = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long i = (block * 64 + li) * W;
    float s[W];
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] = 0.f;
    if (i < n) {
        int k = q;
        for (; k + 28 < S; k += 32) {
            float v[8][W];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if constexpr (VEC) {
                    const f32x4 t = *(const f32x4*)(part + (size_t)(k + 4 * u) * n + i);
                    v[u][0] = t[0]; v[u][1] = t[1]; v[u][2] = t[2]; v[u][3] = t[3];
                } else {
                    v[u][0] = part[(size_t)(k + 4 * u) * n + i];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int w = 0; w < W; ++w) s[w] += v[u][w];
        }
        for (; k < S; k += 4) {
            if constexpr (VEC) {
                const f32x4 t = *(const f32x4*)(part + (size_t)k * n + i);
                s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[3];
            } else {
                s[0] += part[(size_t)k * n + i];
            }
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) red[q][li * W + w] = s[w];
    __syncthreads();
    if (q == 0 && i < n) {
        float t[W];
#pragma unroll
        for (int w = 0; w < W; ++w) t[w] = ((red[0][li * W + w] + red[1][li * W + w]) + (red[2][li * W + w] + red[3][li * W + w]));
        if constexpr (VEC) {
            f32x4* op = (f32x4*)(out + i);
            f32x4 r = {t[0], t[1], t[2], t[3]};
            if (accumulate) r += *op;
            *op = r;
        } else {
            out[i] = accumulate ? out[i] + t[0] : t[0];
        }
    }
}
static inline bool splitk_reduce_vec(const float* part, const float* out, long n) {
    return (n & 3) == 0 && (((uintptr_t)part) & 15) == 0 && (((uintptr_t)out) & 15) == 0;
}
template <bool VEC>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                            long n, int S, int accumulate) {
    splitk_reduce_body<VEC>(part, out, n, S, accumulate, (long)blockIdx.x);
}

static inline dim3 splitk_reduce_grid(size_t n, bool vec = false) { return dim3((unsigned)((n + (vec ? 255 : 63)) / (vec ? 256 : 64))); }

// ---------------------------------------------------------------------------------------
// Deferred split reductions (round 3).  A training step runs 7-8 split products whose partial slices each needed their
// own reduce launch (4.5-9 us apiece, 30-55 us per step: 11 % of model.fit's step at the reference's batch of 32).
// Between fov_reduce_defer_begin and fov_reduce_defer_flush a product whose output lies inside the registered gradient
// buffer writes its slices into the caller's ARENA instead of the call's scratch and only RECORDS {slices, out, n, S,
// accumulate}; the flush sums all recorded products in ONE launch, with the arithmetic of splitk_reduce_kernel (same
// order: bit-identical results).  Any later write of a producer into a range that a pending record covers flushes first,
// so in-stream order is preserved; code that touches the gradient buffer by other means must flush itself
// (training.FlatParamTrainer does, before the optimizer / the all-reduce / a gradient rescale).
// ---------------------------------------------------------------------------------------

constexpr int kDeferMax = 16;
struct DeferEntry { const float* part; float* out; long n; int S; int accumulate; int block0; int vec; };
struct DeferTable { int count; int blocks; DeferEntry e[kDeferMax]; };

__global__ __launch_bounds__(256) void splitk_reduce_batch_kernel(DeferTable t) {
    int cur = 0;
#pragma unroll 1
    for (int i = 1; i < t.count; ++i)
        if ((int)blockIdx.x >= t.e[i].block0) cur = i;
    const DeferEntry e = t.e[cur];
    if (e.vec) splitk_reduce_body<true>(e.part, e.out, e.n, e.S, e.accumulate, (long)((int)blockIdx.x - e.block0));
    else splitk_reduce_body<false>(e.part, e.out, e.n, e.S, e.accumulate, (long)((int)blockIdx.x - e.block0));
}

// The deferral state is keyed by the registered gradient buffer: every trainer (thread, stream, device) that opened a region
// with fov_reduce_defer_begin owns ONE entry of the registry below - its arena, its record table - and a product finds its
// region by the address of its output.  Regions never overlap (begin replaces an overlapping one after flushing it), so two
// trainers on two threads or two GPUs of one process never see each other's arena or records; the registry itself is guarded
// by one mutex.
namespace {
struct DeferState {
    const float* gbase = nullptr; const float* gend = nullptr;
    float* arena = nullptr; size_t arena_floats = 0, used = 0;
    DeferTable table = {};
};
constexpr int kDeferRegions = 16;     // open regions per process (one per trainer in flight; begin fails beyond that)
DeferState g_defer[kDeferRegions];
int g_defer_open = 0;
std::mutex g_defer_mu;

DeferState* defer_region_of(const float* out, size_t n) {       // the region that holds [out, out + n), or NULL
    for (int i = 0; i < g_defer_open; ++i)
        if (out >= g_defer[i].gbase && out + n <= g_defer[i].gend) return &g_defer[i];
    return nullptr;
}
bool defer_overlaps(const DeferState& st, const float* out, size_t n) {
    for (int i = 0; i < st.table.count; ++i) {
        const DeferEntry& e = st.table.e[i];
        if (out < e.out + e.n && e.out < out + n) return true;
    }
    return false;
}
int defer_flush_locked(DeferState& st, hipStream_t stream) {
    DeferTable& t = st.table;
    if (t.count == 0) return FOV_OK;
    hipLaunchKernelGGL(splitk_reduce_batch_kernel, dim3((unsigned)t.blocks), dim3(256), 0, stream, t);
    t.count = 0; t.blocks = 0;
    // the arena is NOT rewound here: a caller may flush on one stream (its products run on a side stream) and go on recording
    // on another - slices are written once per begin ... end, what does not fit any more is reduced at once
    return launch_check("splitk_reduce_batch");
}
void defer_close_locked(int i) {
    g_defer[i] = g_defer[g_defer_open - 1];
    g_defer[--g_defer_open] = DeferState();
}
}  // namespace

int defer_begin(float* grad_base, size_t grad_floats, float* arena, size_t arena_floats, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    if (!grad_base || grad_floats == 0) return FOV_OK;
    // a region over (part of) the same buffer is replaced: its pending records go first
    for (int i = g_defer_open - 1; i >= 0; --i)
        if (grad_base < g_defer[i].gend && g_defer[i].gbase < grad_base + grad_floats) {
            int rc = defer_flush_locked(g_defer[i], stream);
            defer_close_locked(i);
            if (rc) return rc;
        }
    if (!arena || arena_floats == 0) return FOV_OK;
    if (g_defer_open == kDeferRegions) { set_error("fov_reduce_defer_begin: too many open regions (16 per process)"); return FOV_ERR_UNSUPPORTED; }
    DeferState& st = g_defer[g_defer_open++];
    st = DeferState();
    st.gbase = grad_base; st.gend = grad_base + grad_floats;
    st.arena = arena; st.arena_floats = arena_floats;
    return FOV_OK;
}
// grad_base = the buffer a region was opened on (any address inside it); NULL = every open region of the process
int defer_flush(const float* grad_base, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    int rc = FOV_OK;
    for (int i = 0; i < g_defer_open; ++i)
        if (!grad_base || (grad_base >= g_defer[i].gbase && grad_base < g_defer[i].gend))
            if (int r = defer_flush_locked(g_defer[i], stream)) rc = r;
    return rc;
}
int defer_end(const float* grad_base, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    int rc = FOV_OK;
    for (int i = g_defer_open - 1; i >= 0; --i)
        if (!grad_base || (grad_base >= g_defer[i].gbase && grad_base < g_defer[i].gend)) {
            if (int r = defer_flush_locked(g_defer[i], stream)) rc = r;
            defer_close_locked(i);
        }
    return rc;
}
// A producer is about to write [out, out + n) (directly, or through an immediate reduce): pending records over that range
// go first.
int defer_touch(const float* out, size_t n, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    for (int i = 0; i < g_defer_open; ++i) {
        DeferState& st = g_defer[i];
        if (out < st.gend && st.gbase < out + n && st.table.count > 0 && defer_overlaps(st, out, n))
            if (int rc = defer_flush_locked(st, stream)) return rc;
    }
    return FOV_OK;
}
// accumulate = 0 over an empty batch or sequence: [g, g + n) = 0, the gradient of an empty sum (after the pending records over it)
int zero_grad(float* g, size_t n, hipStream_t stream) {
    if (!g || n == 0) return FOV_OK;
    if (int rc = defer_touch(g, n, stream)) return rc;
    hipError_t e = hipMemsetAsync(g, 0, sizeof(float) * n, stream);
    if (e != hipSuccess) { set_error("zero_grad: %s", hipGetErrorString(e)); return FOV_ERR_LAUNCH; }
    return FOV_OK;
}
// Where a split product with output [out, out + n) may put its `floats` of partial slices, or NULL: reduce at once.
float* defer_alloc(const float* out, size_t n, size_t floats, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    DeferState* st = defer_region_of(out, n);
    if (!st) return nullptr;
    if (st->table.count > 0 && defer_overlaps(*st, out, n)) { if (defer_flush_locked(*st, stream)) return nullptr; }
    const size_t need = (floats + 63) & ~(size_t)63;
    if (st->table.count == kDeferMax && defer_flush_locked(*st, stream)) return nullptr;
    if (st->used + need > st->arena_floats) return nullptr;   // arena exhausted for this step: reduce at once
    float* p = st->arena + st->used;
    st->used += need;
    return p;
}
// (only behind a successful defer_alloc for the same output: the region exists and has a free record)
void defer_record(const float* part, float* out, long n, int S, int accumulate) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    DeferState* st = defer_region_of(out, (size_t)n);
    if (!st) return;
    DeferTable& t = st->table;
    DeferEntry& e = t.e[t.count++];
    e.part = part; e.out = out; e.n = n; e.S = S; e.accumulate = accumulate; e.block0 = t.blocks;
    e.vec = splitk_reduce_vec(part, out, n) ? 1 : 0;
    t.blocks += (int)splitk_reduce_grid((size_t)n, e.vec != 0).x;
}
// the common tail of a split product: record (slices already in the arena) or reduce now
int reduce_or_defer(bool deferred, const float* part, float* out, long n, int S, int accumulate, hipStream_t stream, const char* what) {
    if (deferred) { defer_record(part, out, n, S, accumulate); return FOV_OK; }
    int rc = defer_touch(out, (size_t)n, stream);
    if (rc) return rc;
    if (splitk_reduce_vec(part, out, n))
        hipLaunchKernelGGL(splitk_reduce_kernel<true>, splitk_reduce_grid((size_t)n, true), dim3(256), 0, stream, part, out, n, S, accumulate);
    else
        hipLaunchKernelGGL(splitk_reduce_kernel<false>, splitk_reduce_grid((size_t)n), dim3(256), 0, stream, part, out, n, S, accumulate);
    return launch_check(what);
}

int splitk_reduce(const float* part, float* out, long n, int S, int accumulate, hipStream_t stream) {
    if (n <= 0) return FOV_OK;
    return reduce_or_defer(false, part, out, n, S, accumulate, stream, "splitk_reduce");
}

// partial column sums: block (x = column block of 256, y = row chunk) -> part[y][col]
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                             long rows, int cols, long rows_per_chunk) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    const long r0 = (long)blockIdx.y * rows_per_chunk;
    long r1 = r0 + rows_per_chunk;
    if (r1 > rows) r1 = rows;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    long r = r0;
    for (; r + 4 <= r1; r += 4) {
        s0 += x[(size_t)r * cols + col];
        s1 += x[(size_t)(r + 1) * cols + col];
        s2 += x[(size_t)(r + 2) * cols + col];
        s3 += x[(size_t)(r + 3) * cols + col];
    }
    for (; r < r1; ++r) s0 += x[(size_t)r * cols + col];
    part[(size_t)blockIdx.y * cols + col] = (s0 + s1) + (s2 + s3);
}

// Narrow matrices (cols <= 16, e.g. the Dense(6) bias gradient over B*T rows): the column-per-thread kernel
// above would keep 6 lanes busy.  Here a block owns a chunk of rows, threads stride over the rows with all
// columns in registers, and a fixed-order LDS tree folds the 256 per-thread sums - deterministic.
template <int COLS>
__global__ __launch_bounds__(256) void colsum_narrow_kernel(const float* __restrict__ x, float* __restrict__ partial,
                                                            long rows, int cols, long rows_per_chunk) {
    __shared__ float red[256][COLS + 1];
    const long r0 = (long)blockIdx.x * rows_per_chunk;
    long r1 = r0 + rows_per_chunk;
    if (r1 > rows) r1 = rows;
    float acc[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) acc[c] = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
        const float* xp = x + r * cols;
#pragma unroll
        for (int c = 0; c < COLS; ++c)
            if (c < cols) acc[c] += xp[c];
    }
#pragma unroll
    for (int c = 0; c < COLS; ++c) red[threadIdx.x][c] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int c = 0; c < COLS; ++c) red[threadIdx.x][c] += red[threadIdx.x + s][c];
        __syncthreads();
    }
    if ((int)threadIdx.x < cols) partial[(long)blockIdx.x * cols + threadIdx.x] = red[0][threadIdx.x];
}

int colsum(const float* x, float* out, long rows, int cols, int accumulate, float* scratch, size_t scratch_floats,
           hipStream_t stream) {
    if (cols <= 0) return FOV_OK;
    int chunks = (int)((rows + 127) / 128);
    if (chunks < 1) chunks = 1;
    if (chunks > 256) chunks = 256;
    if ((size_t)chunks * cols > scratch_floats) { set_error("colsum: scratch too small"); return FOV_ERR_WORKSPACE; }
    long rpc = (rows + chunks - 1) / chunks;
    bool deferred = false;
    if (float* arena = defer_alloc(out, (size_t)cols, (size_t)chunks * cols, stream)) { scratch = arena; deferred = true; }   // (the narrow form below needs fewer slices)
    if (cols <= 16 && rows >= 4096) {
        chunks = (int)((rows + 2047) / 2048);
        if (chunks > 256) chunks = 256;
        rpc = (rows + chunks - 1) / chunks;
        if (cols <= 8)
            hipLaunchKernelGGL(colsum_narrow_kernel<8>, dim3(chunks), dim3(256), 0, stream, x, scratch, rows, cols, rpc);
        else
            hipLaunchKernelGGL(colsum_narrow_kernel<16>, dim3(chunks), dim3(256), 0, stream, x, scratch, rows, cols, rpc);
    } else {
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((cols + 255) / 256, chunks), dim3(256), 0, stream, x, scratch, rows,
                           cols, rpc > 0 ? rpc : 1);
    }
    int rc = launch_check("colsum_partial");
    if (rc) return rc;
    return reduce_or_defer(deferred, scratch, out, (long)cols, chunks, accumulate, stream, "colsum_reduce");
}

}  // namespace fov
