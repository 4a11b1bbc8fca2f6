// The inputs of the seq2seq LSTM models gathered from FoV tracks that stay on the device:
//   replaces: mycode/utility.py:264-305 (reshape2second_stacks), :359-446 (get_data), :483-517 (get_gt_target_xyz[_oth]),
//             mycode/given_others_gt_mean_var_seq2seq.py:675-695 (the test loop's batch slicing) and
//             mycode/data_generator_including_saliency.py:93-182 (generator_train2)
// The reference materialises every window of every (video, target user) as (N, T, 90) float64 and, with pick_user, the
// others as (num_user-1, N, T, 90), then reduces each second to its six mean / variance numbers.  Here a dataset is two
// tables: secs (rows, 3*fps), every whole second of every (video, user) track, a track a contiguous run of rows, and feat
// (rows, 6) = fov_meanvar_xyz(secs), computed once.  A window is three ints (sample: the first row of the target's track,
// the row of others_base that lists its others' tracks, the window's first second) and every model input a copy of rows
// of one of the two tables.  No arithmetic: the outputs are bit copies.
//
// ONE launch writes all five outputs.  The outputs are walked as one flat run of units (a unit: V floats, V = 2 by 8-byte
// accesses when every base is 8-byte aligned and 3*fps is even - raw seconds are 360-byte rows, 8-byte aligned and no more;
// feature rows are 24 bytes - else V = 1), output after output, a thread a unit: consecutive lanes write consecutive
// addresses, and read consecutive addresses inside a source row (45 / 3 lanes a row at V = 2).  A workgroup that straddles
// two outputs diverges once.
// Every load is guarded: a sample is taken only if all seconds it names of the target's track lie inside [0, rows), an
// others slot only if the sample is and the slot's own seconds do (and the sample's row of others_base exists); anything
// else is written as zeros and nothing outside the tables is read.
#include "fov_common.h"

namespace fov {

constexpr int WI_NT = 256;

typedef float wi_f32x2 __attribute__((ext_vector_type(2)));

struct WinParams {
    const float* secs;
    const float* feat;
    long rows;
    const int* sample;
    const int* others_base;
    long n_pairs;
    int n_others, T_in, T_out, fut_offset;
    int raw_w, enc_w;                    // floats: 3*fps, and 3*fps or 6
    float* out[5];                       // enc, dec_in, target, others, future_raw
    long end[5];                         // units up to and including each output (a NULL output adds none)
};

template <int V> struct WiVec;
template <> struct WiVec<1> { typedef float type; };
template <> struct WiVec<2> { typedef wi_f32x2 type; };

template <int V>
__global__ __launch_bounds__(WI_NT) void window_inputs_kernel(WinParams p) {
    typedef typename WiVec<V>::type vec;
    long u = blockIdx.x * (long)WI_NT + threadIdx.x;
    if (u >= p.end[4]) return;
    int seg = 0;
    while (u >= p.end[seg]) ++seg;
    if (seg) u -= p.end[seg - 1];
    vec* dst = reinterpret_cast<vec*>(p.out[seg]) + u;

    const int w6 = 6 / V, wraw = p.raw_w / V;
    // unit u of this output -> sample i, second t past the window's first, column c (units), others slot j
    long i;
    int t = 0, c, j = 0, width = 6;
    const float* table = p.feat;
    if (seg == 0) {                      // enc (n, T_in, enc_w)
        const int w = p.enc_w / V, per = p.T_in * w;
        i = u / per;
        const int r = (int)(u - i * per);
        t = r / w; c = r - t * w;
        if (p.enc_w != 6) { table = p.secs; width = p.raw_w; }
    } else if (seg == 1) {               // dec_in (n, 6): the encoder's last second
        i = u / w6;
        c = (int)(u - i * w6);
        t = p.T_in - 1;
    } else if (seg == 2) {               // target (n, T_out, 6)
        const int per = p.T_out * w6;
        i = u / per;
        const int r = (int)(u - i * per);
        t = r / w6; c = r - t * w6;
        t += p.fut_offset;
    } else if (seg == 3) {               // others (n, T_out, n_others, 6)
        const int pt = p.n_others * w6, per = p.T_out * pt;
        i = u / per;
        int r = (int)(u - i * per);
        t = r / pt; r -= t * pt;
        j = r / w6; c = r - j * w6;
        t += p.fut_offset;
    } else {                             // future_raw (n, T_out, 3*fps)
        const int per = p.T_out * wraw;
        i = u / per;
        const int r = (int)(u - i * per);
        t = r / wraw; c = r - t * wraw;
        t += p.fut_offset;
        table = p.secs; width = p.raw_w;
    }

    const long base = p.sample[3 * i], pair = p.sample[3 * i + 1], start = p.sample[3 * i + 2];
    const long fut_end = (long)p.fut_offset + p.T_out;
    const long extent = fut_end > p.T_in ? fut_end : (long)p.T_in;        // seconds of a track one sample names
    bool ok = base >= 0 && start >= 0 && base + start + extent <= p.rows;
    long row = base + start + t;
    if (seg == 3) {
        ok = ok && pair >= 0 && pair < p.n_pairs;
        long ob = -1;
        if (ok) ob = p.others_base[pair * p.n_others + j];
        ok = ok && ob >= 0 && ob + start + fut_end <= p.rows;
        row = ob + start + t;
    }
    vec v = vec(0.f);
    if (ok) v = *reinterpret_cast<const vec*>(table + row * width + (long)c * V);
    *dst = v;
}

}  // namespace fov

using namespace fov;

extern "C" {

int fov_window_inputs(const float* secs, const float* feat, int64_t rows, int fps, const int32_t* sample, int64_t n,
                      const int32_t* others_base, int64_t n_pairs, int n_others, int T_in, int T_out, int fut_offset,
                      float* enc, int enc_width, float* dec_in, float* target, float* others, float* future_raw,
                      fov_stream_t stream) {
    if (rows < 0 || fps <= 0 || fps > (1 << 20) || n < 0 || n_pairs < 0 || n_others < 0 || n_others > (1 << 20) ||
        T_in <= 0 || T_out <= 0 || fut_offset < 0 || T_in > (1 << 20) || T_out > (1 << 20) || fut_offset > (1 << 20)) {
        set_error("fov_window_inputs: invalid argument");
        return FOV_ERR_INVALID;
    }
    if (enc && enc_width != 3 * fps && enc_width != 6) {
        set_error("fov_window_inputs: enc_width must be 3*fps (raw seconds) or 6 (mean / variance), got %d", enc_width);
        return FOV_ERR_INVALID;
    }
    if (n_others == 0) others = nullptr;
    if (n == 0) return FOV_OK;
    const bool need_secs = (enc && enc_width != 6) || future_raw;
    const bool need_feat = (enc && enc_width == 6) || dec_in || target || others;
    if (!sample || (need_secs && !secs) || (need_feat && !feat) || (others && !others_base)) {
        set_error("fov_window_inputs: NULL table (sample, secs / feat for the outputs asked for, others_base with n_others > 0)");
        return FOV_ERR_INVALID;
    }
    WinParams p;
    p.secs = secs; p.feat = feat; p.rows = rows; p.sample = sample; p.others_base = others_base; p.n_pairs = n_pairs;
    p.n_others = n_others; p.T_in = T_in; p.T_out = T_out; p.fut_offset = fut_offset;
    p.raw_w = 3 * fps; p.enc_w = enc ? enc_width : 6;
    p.out[0] = enc; p.out[1] = dec_in; p.out[2] = target; p.out[3] = others; p.out[4] = future_raw;
    bool vec = (p.raw_w & 1) == 0 && !(((uintptr_t)secs) & 7) && !(((uintptr_t)feat) & 7);
    for (float* o : p.out) vec = vec && !(((uintptr_t)o) & 7);
    const long V = vec ? 2 : 1;
    // floats of one sample in each output; every one is a multiple of V and, in units, fits an int
    const long per[5] = {(long)T_in * p.enc_w, 6, (long)T_out * 6, (long)T_out * n_others * 6, (long)T_out * p.raw_w};
    long total = 0;
    for (int k = 0; k < 5; ++k) {
        long units = 0;
        if (per[k] > 0x7fffffffL || (p.out[k] && __builtin_mul_overflow((long)n, per[k] / V, &units)) ||
            __builtin_add_overflow(total, units, &total)) {
            set_error("fov_window_inputs: output too large");
            return FOV_ERR_INVALID;
        }
        p.end[k] = total;
    }
    if (total == 0) return FOV_OK;
    const long blocks = (total + WI_NT - 1) / WI_NT;
    if (blocks > 0x7fffffffL) {
        set_error("fov_window_inputs: more than 2^31 workgroups of output");
        return FOV_ERR_INVALID;
    }
    if (vec)
        hipLaunchKernelGGL(window_inputs_kernel<2>, dim3((unsigned)blocks), dim3(WI_NT), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(window_inputs_kernel<1>, dim3((unsigned)blocks), dim3(WI_NT), 0, (hipStream_t)stream, p);
    return launch_check("window_inputs");
}

}  // extern "C"
